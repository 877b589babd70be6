"""float64 restatement of MCMC densification ("MCMC"; gsplat's MCMCStrategy).

Kernels (csrc/mcmc.hip):
  relocation   r = clamp(ratio, 1, 51);  o' = 1 - (1 - o)^(1/r)
               D = sum_{i=1..r} sum_{k=0..i-1} C(i-1,k) (-1)^k / sqrt(k+1) o'^(k+1);  new_scales = (o / D) scales
  reg_grad     g_o += c_o s (1 - s), s = sigmoid(opacity_raw);  g_s += c_s exp(scaling_raw)
  noise        gate = 1 / (1 + exp(-100 ((1 - sigmoid(opacity_raw)) - 0.995)));  Sigma = R diag(exp(scaling_raw))^2 R^T
               with R of the normalised raw quaternion (w,x,y,z);  xyz += Sigma (noise * gate * scaler)
Model surgery (strategies/base_gaussian_model.py): the inverse-CDF sampler, relocate_gs and add_new_gs applied to a dict
of float64 tables at GIVEN indices (the sampling itself is not restated: the tests hand over the indices a model drew)."""
import math

import numpy as np
import torch

MAX_RATIO = 51
F32_EPS = float(torch.finfo(torch.float32).eps)


def relocation(opacities, scales, ratios):
    """-> (new_opacities [n], new_scales [n,3], kappa [n]) in float64; kappa = sum |terms| / |sum terms| of D, the
    condition number of the alternating sum.  The double sum is written out term by term, as the specification has it."""
    o = np.asarray(opacities, dtype=np.float64).reshape(-1)
    s = np.asarray(scales, dtype=np.float64).reshape(-1, 3)
    r = np.clip(np.asarray(ratios).astype(np.int64).reshape(-1), 1, MAX_RATIO)
    op = 1.0 - np.power(1.0 - o, 1.0 / r)
    D, A = np.zeros_like(o), np.zeros_like(o)
    for i in range(1, MAX_RATIO + 1):
        on = r >= i
        for k in range(i):
            t = math.comb(i - 1, k) * (-1.0) ** k / math.sqrt(k + 1.0) * op ** (k + 1)
            D += np.where(on, t, 0.0)
            A += np.where(on, np.abs(t), 0.0)
    return op, (o / D)[:, None] * s, A / np.abs(D)


RATIOS = (0, 1, 2, 3, 8, 51, 200)  # 0 and 200 exercise the clamp


def relocation_inputs(n, seed=0):
    """The inputs of the relocation kernel test: float32 opacities in [0.005, 0.99] (both ends present from n = 2 on),
    scales log-uniform in [1e-3, 1e1], ratios drawn from RATIOS (every one present from n = 7 on)."""
    g = torch.Generator().manual_seed(1000 * seed + n)
    o = (0.005 + 0.985 * torch.rand(n, generator=g)).clamp(0.005, 0.99)
    o[0] = 0.99
    if n > 1:
        o[-1] = 0.005
    s = torch.exp(torch.rand(n, 3, generator=g) * math.log(1e4) + math.log(1e-3))
    ratios = torch.tensor(RATIOS, dtype=torch.int32)[torch.randperm(n, generator=g) % len(RATIOS)]
    return o.float(), s.float(), ratios.contiguous()


def reg_grads(opacity_raw, scaling_raw, c_o, c_s):
    """-> (dg_o [n,1], dg_s [n,3]): what reg_grad ADDS."""
    o = torch.sigmoid(opacity_raw.double())
    return float(c_o) * o * (1.0 - o), float(c_s) * torch.exp(scaling_raw.double())


def reg_loss(opacity_raw, scaling_raw, w_o, w_s):
    """w_o mean(sigmoid(opacity_raw)) + w_s mean(exp(scaling_raw)), for autograd."""
    return float(w_o) * torch.sigmoid(opacity_raw).mean() + float(w_s) * torch.exp(scaling_raw).mean()


def rotmat(q):
    q = q.double()
    q = q / q.norm(dim=1, keepdim=True)
    w, x, y, z = q.unbind(1)
    return torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y),
                        2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x),
                        2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)], dim=1).reshape(-1, 3, 3)


def noise_delta(opacity_raw, scaling_raw, rotation_raw, noise, scaler, k=100.0, x0=0.995):
    """-> (dx [n,3], mag [n,3]) in float64: the increment Sigma (noise * gate * scaler) and
    mag_i = sum_j |Sigma_ij| |noise_j| gate scaler, the scale the kernel's error is measured against."""
    gate = 1.0 / (1.0 + torch.exp(-k * ((1.0 - torch.sigmoid(opacity_raw.double())) - x0)))  # [n,1]
    R = rotmat(rotation_raw)
    S2 = torch.diag_embed(torch.exp(scaling_raw.double()) ** 2)
    Sigma = R @ S2 @ R.transpose(1, 2)
    v = noise.double() * gate * float(scaler)
    dx = (Sigma @ v[:, :, None])[:, :, 0]
    mag = (Sigma.abs() @ v.abs()[:, :, None])[:, :, 0]
    return dx, mag


def sample(p, n, generator=None):
    """The inverse-CDF sampler, restated."""
    cdf = torch.cumsum(p.double().flatten(), 0)
    u = torch.rand((int(n),), dtype=torch.float64, device=p.device, generator=generator) * cdf[-1]
    return torch.searchsorted(cdf, u, right=True).clamp(max=p.numel() - 1)


TABLES = ("xyz", "shs48", "opacity", "scaling", "rotation")


def _relocate_sources(state, src, min_opacity):
    n = state["opacity"].shape[0]
    ratios = torch.bincount(src, minlength=n)[src] + 1
    o = torch.sigmoid(state["opacity"][src, 0])
    s = torch.exp(state["scaling"][src])
    new_o, new_s, _ = relocation(o.numpy(), s.numpy(), ratios.numpy())
    # the model rounds the kernel's outputs to float32 before the clamp, the logit and the log
    new_o = torch.from_numpy(new_o).float().clamp(float(min_opacity), 1.0 - F32_EPS).double()
    new_s = torch.from_numpy(new_s).float().double()
    state["opacity"][src, 0] = torch.log(new_o / (1.0 - new_o))
    state["scaling"][src] = torch.log(new_s)


def relocate(state, dead_idx, src_idx, min_opacity):
    """relocate_gs at the given indices, in place on `state`: float64 CPU tables xyz [N,3], shs48 [N,48], opacity [N,1],
    scaling [N,3], rotation [N,4] and their moments under "m_<name>" / "v_<name>"."""
    _relocate_sources(state, src_idx, min_opacity)
    for k in TABLES:
        state[k][dead_idx] = state[k][src_idx]
        state["m_" + k][src_idx] = 0.0
        state["v_" + k][src_idx] = 0.0
    return state


def add_new(state, src_idx, min_opacity):
    """add_new_gs at the given source indices: relocation of the sources, their copies appended with zero moments, the
    sources' moments zeroed.  -> a new state dict (row order: old rows, then the copies; no re-sort)."""
    _relocate_sources(state, src_idx, min_opacity)
    out = {}
    for k in TABLES:
        out[k] = torch.cat((state[k], state[k][src_idx]), dim=0)
        for mv in ("m_", "v_"):
            t = state[mv + k].clone()
            t[src_idx] = 0.0
            out[mv + k] = torch.cat((t, torch.zeros_like(state[k][src_idx])), dim=0)
    return out
