"""The per-batch part of MCMC densification ("MCMC"; gsplat's MCMCStrategy): the two regulariser
gradients BEFORE the small attributes' Adam step, the opacity-gated position noise AFTER it.  Both touch all N rows, on
current parameters.  The refinement itself (relocation, growth) is densification.mcmc_refinement."""
import torch

from . import utils
from .clm_kernels import mcmc_inject_noise_, mcmc_reg_grad_

NOISE_SEED = 0


def enabled(args=None):
    return bool(getattr(args if args is not None else utils.get_args(), "mcmc", False))


def reg_constants(args, n, grad_div=1.0):
    """(c_o, c_s) of clm_kernels.mcmc_reg_grad_ for mcmc_opacity_reg * mean over [n,1] + mcmc_scale_reg * mean over [n,3].
    grad_div: what the optimizer step will divide the gradient table by (the engines accumulate the batch's SUM and step
    with 1 / bsz), so the constants carry the inverse."""
    return (float(args.mcmc_opacity_reg) * float(grad_div) / float(n),
            float(args.mcmc_scale_reg) * float(grad_div) / float(3 * n))


def add_reg_grads(gaussians, grad_div=1.0, packed=None, packed_grad=None):
    """The regulariser gradients added into the packed [N,12] gradient table (`packed` = the parameter mirror) or into the
    .grad of the model's opacity / scaling tensors."""
    args = utils.get_args()
    n = gaussians._xyz.shape[0]
    c_o, c_s = reg_constants(args, n, grad_div)
    if c_o == 0.0 and c_s == 0.0:
        return
    if packed is not None:
        mcmc_reg_grad_(c_o, c_s, packed=packed, packed_grad=packed_grad)
        return
    for p in (gaussians._opacity, gaussians._scaling):
        if p.grad is None:
            p.grad = torch.zeros_like(p)
    mcmc_reg_grad_(c_o, c_s, gaussians._opacity.detach(), gaussians._scaling.detach(), gaussians._opacity.grad,
                   gaussians._scaling.grad)


def noise_generator(gaussians):
    """The device generator the noise is drawn from: `gaussians.mcmc_noise_generator`, made here (seed NOISE_SEED) when
    nobody has set one."""
    g = getattr(gaussians, "mcmc_noise_generator", None)
    if g is None:
        g = gaussians.mcmc_noise_generator = torch.Generator(device=gaussians._xyz.device)
        g.manual_seed(NOISE_SEED)
    return g


def xyz_lr(gaussians):
    for g in gaussians.optimizer.param_groups:
        if g["name"] == "xyz":
            return float(g["lr"])
    raise KeyError("xyz")


def inject_noise(gaussians, packed=None):
    """xyz += Sigma (randn * gate * mcmc_noise_lr * lr_xyz) on all rows, and into columns 0..2 of the packed mirror."""
    args = utils.get_args()
    scaler = float(args.mcmc_noise_lr) * xyz_lr(gaussians)
    if scaler == 0.0:
        return
    n = gaussians._xyz.shape[0]
    noise = torch.randn((n, 3), dtype=torch.float32, device=gaussians._xyz.device, generator=noise_generator(gaussians))
    mcmc_inject_noise_(gaussians._xyz.data, gaussians._opacity.data, gaussians._scaling.data, gaussians._rotation.data,
                       noise, scaler, packed=packed)
