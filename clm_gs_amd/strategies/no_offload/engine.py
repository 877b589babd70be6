"""no_offload engine (reference: strategies/no_offload/engine.py:15-177): per-camera
render over all N Gaussians, gradient accumulation over the batch, one backward through the
activations."""
import torch

from ... import utils
from ...cameras import camera_model
from ...clm_kernels import check_depth_prior_args
from ...densification import update_densification_stats_baseline_accum_grads
from ..base_engine import camera_forward_ops, camera_loss_backward, fov_camera


def baseline_accumGrads_micro_step(means3D, opacities, scales, rotations, shs, sh_degree, camera,
                                   background, mode="train", tile_size=16, render_mode="RGB",
                                   return_alpha=False):
    """One camera: K from FoV, projection(N) -> SH(masked) -> +0.5 clamp -> tile binning ->
    rasterize -> [3,H,W].  Returns (image, means2D (grad retained), radii, None); with render_mode "RGB+D" /
    "RGB+ED" / "RGB+ID" a fifth result depth[1,H,W] (accumulated / expected / inverse depth, base_engine.split_depth), and
    with return_alpha a sixth, alpha[1,H,W].  "RGB+MD" (mode="eval" only; refused by name when training: it has no
    gradient): the fifth result is the median depth (base_engine.camera_forward_ops); "RGB+RD" likewise: the ray depth."""
    viewmat, K, centre = fov_camera(camera, means3D.device)
    image, means2D, radiis, depth_alpha, _ = camera_forward_ops(
        means3D, rotations, scales, opacities, shs.unsqueeze(0), sh_degree, viewmat, K, centre, background, render_mode,
        train=mode == "train", radius_clip=utils.get_args().radius_clip, sh_masks=True, tile_size=tile_size,
        sky_camera=camera, camera_model=camera_model(camera))
    return (image, means2D, radiis, None) + depth_alpha[:2 if return_alpha else 1]


def baseline_accumGrads_impl(gaussians, scene, batched_cameras, background, scaling_modifier=1.0,
                             sparse_adam=False):
    """Activations once per batch, detached leaves accumulate over the cameras, then one
    backward through the activations.  Returns (losses, visibility | None); .grad lands on the
    model's six parameters (the optimizer step is the caller's, train.py:533-578)."""
    if getattr(utils.get_args(), "fused_front_end", True) and scaling_modifier == 1.0:
        for camera in batched_cameras:  # absgrad with a depth prior: refused for the whole batch, before any camera runs
            check_depth_prior_args(camera)
        return _baseline_fused(gaussians, scene, batched_cameras, background, sparse_adam)
    losses = []
    means3D = gaussians.get_xyz
    opacities_origin = gaussians.get_opacity
    scales_origin = gaussians.get_scaling * scaling_modifier
    rotations_origin = gaussians.get_rotation
    shs_origin = gaussians.get_features
    sh_degree = gaussians.active_sh_degree
    opacities = opacities_origin.detach().requires_grad_(True)
    scales = scales_origin.detach().requires_grad_(True)
    rotations = rotations_origin.detach().requires_grad_(True)
    shs = shs_origin.detach().requires_grad_(True)
    visibility = (torch.zeros((means3D.shape[0],), dtype=torch.bool, device=means3D.device)
                  if sparse_adam else None)
    H, W = int(utils.get_img_height()), int(utils.get_img_width())
    priors = [check_depth_prior_args(camera) for camera in batched_cameras]  # refusals before anything runs
    for camera, has_prior in zip(batched_cameras, priors):
        # a camera with an inverse-depth prior is rendered with the inverse depth as fourth channel
        rendered_image, means2D, radiis, gaussian_ids, *inv_depth = baseline_accumGrads_micro_step(
            means3D, opacities, scales, rotations, shs, sh_degree, camera, background,
            render_mode="RGB+ID" if has_prior else "RGB")
        loss, m2_grad = camera_loss_backward(rendered_image, means2D, camera, *inv_depth)
        losses.append(loss)
        with torch.no_grad():
            update_densification_stats_baseline_accum_grads(scene, gaussians, H, W, m2_grad,
                                                            radiis, gaussian_ids)
        if sparse_adam:
            visibility = visibility | (radiis > 0).squeeze()
        del loss, rendered_image, means2D, radiis
    opacities_origin.backward(opacities.grad)
    scales_origin.backward(scales.grad)
    rotations_origin.backward(rotations.grad)
    shs_origin.backward(shs.grad)
    return losses, visibility


def _baseline_fused(gaussians, scene, batched_cameras, background, sparse_adam):
    """Same batch through the fused front end (clm_gs_amd/fused.py): every camera runs over all N
    rows (filter = None), raw-parameter gradients are accumulated in place (activation VJPs are
    inside the kernel, so there is no separate "backward to origin" step), statistics follow the
    radii > 0 mask form of densification.py:105-147."""
    from ...fused import train_one_camera
    dev = gaussians._xyz.device
    N = gaussians._xyz.shape[0]
    with torch.no_grad():
        shs = gaussians.get_features.reshape(N, 48).contiguous()  # one [N,48] view of dc | rest
        g_shs = torch.zeros_like(shs)
        for p in (gaussians._xyz, gaussians._opacity, gaussians._scaling, gaussians._rotation):
            if p.grad is None:
                p.grad = torch.zeros_like(p)
        visibility = torch.zeros((N,), dtype=torch.bool, device=dev) if sparse_adam else None
        losses = []
        for camera in batched_cameras:
            losses.append(train_one_camera(gaussians, camera, None, shs, 1, g_shs, background,
                                           camera.original_image, stats_only_visible=True,
                                           visibility_out=visibility))
        g3 = g_shs.reshape(N, 16, 3)
        for p, g in ((gaussians._features_dc, g3[:, :1, :]), (gaussians._features_rest, g3[:, 1:, :])):
            p.grad = g.contiguous() if p.grad is None else p.grad + g
    return losses, visibility
