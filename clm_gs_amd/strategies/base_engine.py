"""Raster front end shared by the engines (reference: strategies/base_engine.py:15-207):
calculate_filters, the L1+SSIM training loss, and the one-camera forward used by eval."""
import math

import torch

from .. import utils
from ..cameras import camera_loss_mask, camera_model as camera_model_of, camera_sky, check_sky_background, refuse_ortho
from ..clm_kernels import apply_camera_colour, apply_camera_sky, camera_depth_term, fused_l1_ssim_loss, fused_ssim
from ..gsplat import (fully_fused_projection, isect_offset_encode, isect_tiles,
                      rasterize_median_depth, rasterize_to_pixels, ray_gaussian_depth, spherical_harmonics, visibility_radii)

LAMBDA_DSSIM = 0.2
TILE_SIZE = 16


def select_filter_words(batched_cameras, xyz_gpu, scaling_raw_gpu, rotation_raw_gpu, cam_mats, block_flags, block_sel):
    """The first of two launches of select_filters (gsplat.visibility_select_words): the ballot words of the blocks
    `block_sel` selects, on the current stream, with the camera matrices cam_mats = (viewmats[C,4,4], Ks[C,3,3]) the caller
    made on that stream -> temp for select_filters(block_sel=the other blocks, temp=temp)."""
    from ..gsplat import visibility_select_words
    args = utils.get_args()
    for c in batched_cameras:
        refuse_ortho(c, "select_filters")
    with torch.no_grad():
        return visibility_select_words(
            xyz_gpu, rotation_raw_gpu, scaling_raw_gpu, cam_mats[0], cam_mats[1], int(utils.get_img_width()),
            int(utils.get_img_height()), block_sel, radius_clip=args.radius_clip, block_flags=block_flags)


def select_filters(batched_cameras, xyz_gpu, scaling_raw_gpu, rotation_raw_gpu, block_flags=None, block_sel=None,
                   temp=None):
    """calculate_filters on the stored (raw) parameters, selected entirely on the GPU
    (gsplat.visibility_select) -> (filters, touched_rows): the same index sets as calculate_filters
    plus the union over the batch's cameras.  block_sel + temp: the second of two launches (select_filter_words)."""
    from ..gsplat import visibility_select
    args = utils.get_args()
    for c in batched_cameras:  # the selection kernels are pinhole ones
        refuse_ortho(c, "select_filters")
    with torch.no_grad():
        Ks = torch.stack([c.create_k_on_gpu() if getattr(c, "K", None) is None else c.K for c in batched_cameras])
        viewmats = torch.stack([c.world_view_transform.transpose(0, 1) for c in batched_cameras])
        filters, touched_rows = visibility_select(
            xyz_gpu, rotation_raw_gpu, scaling_raw_gpu, viewmats, Ks, int(utils.get_img_width()),
            int(utils.get_img_height()), radius_clip=args.radius_clip, block_flags=block_flags, block_sel=block_sel,
            temp=temp)
    assert all(f.numel() > 0 for f in filters), (
        "every camera must see at least one gaussian (base_engine.py:64-67)")
    return filters, touched_rows


def calculate_filters(batched_cameras, xyz_gpu, opacity_gpu, scaling_gpu, rotation_gpu,
                      return_ids=False, raw=False):
    """Per-camera visible index lists: ONE cull pass over (bsz cameras x N Gaussians).

    Same index sets as the packed projection the reference runs (base_engine.py:18-76) -- the
    cull is the projection's own (near plane, blur determinant, radius, off-screen) -- but only
    radii are written, and the (camera, gaussian) pairs are compacted with a single one-column
    nonzero over the flat [C*N] mask (camera boundaries by binary search on the sorted result).
    Returns (filters, camera_ids, gaussian_ids); the id vectors only when return_ids.
    raw=True: scaling_gpu / rotation_gpu are the stored parameters (log-scales, un-normalised
    quaternions) and the activations happen inside the cull kernel.
    A call whose cameras are all orthographic (cameras.OrthoCamera) culls with the orthographic form; a mix of the two
    kinds raises ValueError."""
    args = utils.get_args()
    models = {camera_model_of(c) for c in batched_cameras}
    if len(models) > 1:
        raise ValueError(f"calculate_filters: one call mixes camera models {sorted(models)}; cull each kind on its own")
    model = models.pop() if models else "pinhole"
    with torch.no_grad():
        Ks = torch.stack([c.create_k_on_gpu() if getattr(c, "K", None) is None else c.K for c in batched_cameras])
        viewmats = torch.stack([c.world_view_transform.transpose(0, 1) for c in batched_cameras])
        radii = visibility_radii(xyz_gpu, rotation_gpu, scaling_gpu, viewmats, Ks,
                                 int(utils.get_img_width()), int(utils.get_img_height()),
                                 radius_clip=args.radius_clip, raw=raw,
                                 **({} if model == "pinhole" else {"camera_model": model}))
        C, N = radii.shape
        flat = torch.nonzero(radii.reshape(-1) > 0).flatten()  # sorted: camera-major, then gaussian
        edges = torch.searchsorted(flat, torch.arange(0, C + 1, device=flat.device) * N)
        e = edges.tolist()  # the one host sync of the filter stage
        counts_cpu = [e[i + 1] - e[i] for i in range(C)]
        assert all(c > 0 for c in counts_cpu), (
            "every camera must see at least one gaussian (base_engine.py:64-67)")
        pieces = torch.split(flat, counts_cpu)
        filters = tuple(p - i * N if i else p for i, p in enumerate(pieces))
        camera_ids = gaussian_ids = None
        if return_ids:
            camera_ids = torch.div(flat, N, rounding_mode="floor")
            gaussian_ids = flat - camera_ids * N
    return filters, camera_ids, gaussian_ids


def loss_combined(image, image_gt, ssim_loss):
    Ll1 = torch.abs(image - image_gt).mean()
    return (1.0 - LAMBDA_DSSIM) * Ll1 + LAMBDA_DSSIM * (1.0 - ssim_loss)


def torch_compiled_loss(image, image_gt_original, loss_mask=None, loss_mask_count=None):
    """0.8 * L1 + 0.2 * (1 - SSIM) against clamp(u8/255) (base_engine.py:79-103).  The
    reference torch.compile's the L1 mix next to a fused SSIM kernel; here the whole loss
    (u8 -> float GT, L1, SSIM, mix) is one fused HIP kernel each way when the GT is uint8.
    loss_mask (uint8 [H,W], 0 = ignored; a camera's `loss_mask`) selects the masked kernels."""
    if image_gt_original.dtype == torch.uint8:
        return fused_l1_ssim_loss(image, image_gt_original, LAMBDA_DSSIM, loss_mask, loss_mask_count)
    if loss_mask is not None:
        raise ValueError("a loss mask needs the uint8 ground-truth image (the masked loss exists as the fused kernels only)")
    image_gt = torch.clamp(image_gt_original / 255.0, 0.0, 1.0)
    ssim_loss = fused_ssim(image.unsqueeze(0), image_gt.unsqueeze(0))
    return loss_combined(image, image_gt, ssim_loss)


RENDER_MODES = ("RGB", "RGB+D", "RGB+ED", "RGB+ID", "RGB+MD", "RGB+RD")
MEDIAN_DEPTH = "RGB+MD"  # no fourth colour: the 3-channel forward, then a pass of its own (gsplat.rasterize_median_depth)
RAY_DEPTH = "RGB+RD"     # "RGB+MD", then per pixel the median Gaussian's ray-intersection depth (gsplat.ray_gaussian_depth)
UNBLENDED_DEPTH = {MEDIAN_DEPTH: "median depth", RAY_DEPTH: "ray depth"}


def refuse_median_training(render_mode, where):
    """The median depth and the ray depth have no gradient: the training entries refuse the modes by name."""
    if render_mode in UNBLENDED_DEPTH:
        raise ValueError(f'{where}: render_mode "{render_mode}" ({UNBLENDED_DEPTH[render_mode]}) is not differentiable and '
                         'cannot be trained on; render it through an eval entry, or train with "RGB+ED" / "RGB+ID"')


def colors_with_depth(colors, depths, backgrounds, render_mode):
    """The rasterizer's inputs for a render mode (gsplat's rasterization(render_mode=...)): with a depth mode the
    camera-space depths[C,N] ride as a fourth colour channel whose background is 0; with "RGB+ID" (the INRIA rasterizer's
    inverse depth, the channel the depth regularisation reads) the fourth colour is 1 / depths, 0 for rows at or behind
    the camera plane (they reach no tile list)."""
    if render_mode not in RENDER_MODES:
        raise ValueError(f"render_mode must be one of {RENDER_MODES}, got {render_mode!r}")
    if render_mode == "RGB" or render_mode in UNBLENDED_DEPTH:  # not blended: three channels, backgrounds as they are
        return colors, backgrounds
    if render_mode == "RGB+ID":
        front = depths > 0
        depths = torch.where(front, 1.0 / torch.where(front, depths, torch.ones_like(depths)), torch.zeros_like(depths))
    colors = torch.cat([colors, depths.unsqueeze(-1)], dim=-1)
    if backgrounds is not None:
        backgrounds = torch.cat([backgrounds, backgrounds.new_zeros(backgrounds.shape[:-1] + (1,))], dim=-1)
    return colors, backgrounds


def split_depth(rendered, alphas, render_mode):
    """rendered[1,H,W,4], alphas[1,H,W,1] -> (image[3,H,W] view, depth[1,H,W], alpha[1,H,W]): the accumulated depth
    sum w_i z_i ("RGB+D"), the expected depth D / clamp(alpha, 1e-10) ("RGB+ED", gsplat's definition) or the blended
    channel as it is ("RGB+ID": the inverse depth sum w_i / z_i, not normalised)."""
    depth, alpha = rendered[..., 3], alphas[..., 0]
    if render_mode == "RGB+ED":
        depth = depth / alpha.clamp(min=1e-10)
    return rendered[..., :3].squeeze(0).permute(2, 0, 1), depth, alpha


def fov_camera(camera, device):
    """-> (viewmat[4,4], K[3,3], centre[1,1,3]) as the two FoV entries make them: K from the field of view as a device
    tensor, the centre by torch.inverse ON THE DEVICE.  (camera.K / camera.camtoworlds, which
    pipeline_forward_one_step_shs_inplace reads, come from the host and can differ in the last bit.)
    An orthographic camera has no field of view: its own K, and its size must be the global image size."""
    image_width, image_height = int(utils.get_img_width()), int(utils.get_img_height())
    if camera_model_of(camera) == "ortho":
        if (camera.image_width, camera.image_height) != (image_width, image_height):
            raise ValueError(f"orthographic camera {camera.image_name!r} is {camera.image_width}x{camera.image_height}, "
                             f"the global image size is {image_width}x{image_height} (utils.set_img_size)")
        viewmat = camera.world_view_transform.transpose(0, 1)
        return viewmat, camera.K.to(device), torch.inverse(viewmat.unsqueeze(0))[:, None, :3, 3]
    fx = image_width / (2 * math.tan(camera.FoVx * 0.5))
    fy = image_height / (2 * math.tan(camera.FoVy * 0.5))
    K = torch.tensor([[fx, 0, image_width / 2.0], [0, fy, image_height / 2.0], [0, 0, 1]], device=device)
    viewmat = camera.world_view_transform.transpose(0, 1)
    return viewmat, K, torch.inverse(viewmat.unsqueeze(0))[:, None, :3, 3]


def camera_forward_ops(means, quats, scales, opacities, coeffs, sh_degree, viewmat, K, centre, backgrounds, render_mode,
                       train, radius_clip=0.0, sh_masks=False, sh_autograd=True, tile_size=TILE_SIZE, sky_camera=None,
                       camera_model="pinhole"):
    """The op-by-op forward of one camera, which the three reference-named entries share: projection -> SH -> +0.5 clamp
    -> tile binning -> offsets -> (depth as fourth colour) -> rasterize.  Each entry hands in ITS K, camera centre,
    coefficient view ([1,V,16,3]) and backgrounds (None, [3] or [1,3]); the knobs are what else differs between them:
    train (means2D keeps its gradient, and the absgrad one under args.absgrad), radius_clip, sh_masks (SH only where
    radii > 0), sh_autograd (False: SH under no_grad and the colours re-leafed, for an SH backward that accumulates in
    place), tile_size and sky_camera: the camera, handed in when it carries a sky (cameras.camera_sky) -- the rasterizer
    then runs with NO background (a non-zero one is refused) and the sky is composited behind its two outputs
    (clm_kernels.apply_camera_sky) before the image is returned; None: unchanged.
    camera_model "ortho" (K in pixels per world unit): the orthographic projection, and ONE view direction for all rows,
    the world-space optical axis viewmat[2,:3] -- a parallel projection has one direction, so the image does not depend
    on how far up its axis the camera sits (gsplat keeps means - campos; DESIGN.md section 3, "Orthographic"); `centre`
    is not read.  A sky is refused with it: the map lookup is a pinhole ray.
    render_mode "RGB+MD" (eval only; train=True is refused by name): the forward runs exactly as for "RGB", then
    gsplat.rasterize_median_depth walks the same lists with the same means2D, conics, depths and the opacities the forward
    got (x compensation under rasterize_mode="antialiased"); depth is the median depth, 0.0 where nothing is accumulated,
    alpha the forward's.  A sky is composited behind the splats and changes neither.
    render_mode "RGB+RD" (eval only, refused likewise): everything "RGB+MD" runs, then gsplat.ray_gaussian_depth on the
    median ids with the means, quats, scales, viewmat, K and camera_model handed in: depth is, per pixel, the depth at which
    the median Gaussian's 3-D density peaks along the pixel's ray ("Ray depth") in place of its centre
    depth; 0.0 exactly where "RGB+MD" gives 0.0, image and alpha the same bits.  The ids do not leave this function.
    -> (image[3,H,W] view, means2D[1,V,2], radii[1,V], () | (depth[1,H,W], alpha[1,H,W]) by split_depth,
        () | (colours leaf[1,V,3], dirs[1,V,3]) without sh_autograd)."""
    if render_mode not in RENDER_MODES:
        raise ValueError(f"render_mode must be one of {RENDER_MODES}, got {render_mode!r}")
    if train:
        refuse_median_training(render_mode, "camera_forward_ops(train=True)")
    if camera_model not in ("pinhole", "ortho"):
        raise ValueError(f"camera_model must be 'pinhole' or 'ortho', got {camera_model!r}")
    ortho = camera_model == "ortho"
    if sky_camera is not None and camera_sky(sky_camera) is None:
        sky_camera = None
    if sky_camera is not None and ortho:
        raise ValueError(f"camera {getattr(sky_camera, 'image_name', sky_camera)!r} is orthographic and carries a sky: "
                         "the sky map is looked up along pinhole rays; render it without --sky")
    if sky_camera is not None:  # refused before anything is enqueued
        check_sky_background(backgrounds)
        backgrounds = None
    image_width, image_height = int(utils.get_img_width()), int(utils.get_img_height())
    radiis, means2D, depths, conics, compensations = fully_fused_projection(
        means=means, covars=None, quats=quats, scales=scales, viewmats=viewmat.unsqueeze(0), Ks=K.unsqueeze(0),
        width=image_width, height=image_height, radius_clip=radius_clip, packed=False,
        calc_compensations=utils.antialiased(), **({"camera_model": camera_model} if ortho else {}))
    if train:
        means2D.retain_grad()
    if ortho:
        dirs = viewmat[2, :3].reshape(1, 1, 3).expand(1, means.shape[0], 3)
    else:
        dirs = means[None, :, :] - centre
    sh_leaf = ()
    with torch.set_grad_enabled(sh_autograd and torch.is_grad_enabled()):
        colors = spherical_harmonics(degrees_to_use=sh_degree, dirs=dirs, coeffs=coeffs,
                                     masks=(radiis > 0) if sh_masks else None)
    if not sh_autograd:
        colors = colors.detach().requires_grad_()
        sh_leaf = (colors, dirs)
    colors = torch.clamp_min(colors + 0.5, 0.0)
    opacities = opacities.squeeze(1).unsqueeze(0)
    if compensations is not None:  # rasterize_mode="antialiased"
        opacities = opacities * compensations
    tile_width, tile_height = math.ceil(image_width / float(tile_size)), math.ceil(image_height / float(tile_size))
    _, isect_ids, flatten_ids = isect_tiles(means2d=means2D, radii=radiis, depths=depths, tile_size=tile_size,
                                            tile_width=tile_width, tile_height=tile_height, packed=False)
    isect_offsets = isect_offset_encode(isect_ids, 1, tile_width, tile_height)
    colors, backgrounds = colors_with_depth(colors, depths, backgrounds, render_mode)
    rendered_image, alphas = rasterize_to_pixels(
        means2d=means2D, conics=conics, colors=colors, opacities=opacities,
        image_width=image_width, image_height=image_height, tile_size=tile_size,
        isect_offsets=isect_offsets, flatten_ids=flatten_ids, backgrounds=backgrounds,
        absgrad=train and bool(getattr(utils.get_args(), "absgrad", False)))  # -> means2D.absgrad after backward
    if render_mode in UNBLENDED_DEPTH:
        depth, median_ids = rasterize_median_depth(means2D, conics, opacities, depths, image_width, image_height, tile_size,
                                                   isect_offsets, flatten_ids)
        if render_mode == RAY_DEPTH:
            depth = ray_gaussian_depth(means, quats, scales, viewmat.unsqueeze(0), K.unsqueeze(0), depth, median_ids,
                                       camera_model=camera_model)
        rendered_image = rendered_image.squeeze(0).permute(2, 0, 1)
        if sky_camera is not None:
            rendered_image = apply_camera_sky(rendered_image, alphas[0, ..., 0], sky_camera)
        return rendered_image, means2D, radiis, (depth, alphas[..., 0]), sh_leaf
    if render_mode != "RGB":
        rendered_image, depth, alpha = split_depth(rendered_image, alphas, render_mode)
        if sky_camera is not None:
            rendered_image = apply_camera_sky(rendered_image, alphas[0, ..., 0], sky_camera)
        return rendered_image, means2D, radiis, (depth, alpha), sh_leaf
    rendered_image = rendered_image.squeeze(0).permute(2, 0, 1)  # [3,H,W] view, no copy
    if sky_camera is not None:
        rendered_image = apply_camera_sky(rendered_image, alphas[0, ..., 0], sky_camera)
    return rendered_image, means2D, radiis, (), sh_leaf


def pipeline_forward_one_step(filtered_opacity_gpu, filtered_scaling_gpu, filtered_rotation_gpu,
                              filtered_xyz_gpu, filtered_shs, camera, scene, gaussians, background,
                              pipe_args, eval=False, render_mode="RGB", return_alpha=False):
    """One camera over the gathered rows, SH through autograd (base_engine.py:106-207).
    render_mode "RGB+D" / "RGB+ED": a fourth result depth[1,H,W] (see split_depth), and with return_alpha a fifth,
    alpha[1,H,W]."""
    viewmat, K, centre = fov_camera(camera, filtered_xyz_gpu.device)
    image, means2D, radiis, depth_alpha, _ = camera_forward_ops(
        filtered_xyz_gpu, filtered_rotation_gpu, filtered_scaling_gpu, filtered_opacity_gpu,
        filtered_shs.reshape(1, filtered_xyz_gpu.shape[0], 16, 3), gaussians.active_sh_degree, viewmat, K, centre,
        background.reshape(1, 3) if background is not None else None, render_mode, train=not eval, sky_camera=camera,
        camera_model=camera_model_of(camera))
    return (image, means2D, radiis) + depth_alpha[:2 if return_alpha else 1]


def camera_loss_backward(image, means2D, camera, inv_depth=None):
    """The op-by-op training tail of one camera, after its forward: the camera's colour stage (exposure transform or
    bilateral grid, if it has one), the L1+SSIM loss under the camera's loss mask, the depth term when the camera was
    rendered with its prior's inverse depth (inv_depth[1,H,W]), backward().
    -> (loss, detached; the means2D gradient the densification statistic is built from: gsplat's absgrad,
    sum_p |dL_p/dmean2d|, under args.absgrad, else the signed sum)."""
    image = apply_camera_colour(image, camera)
    loss = torch_compiled_loss(image, camera.original_image, *camera_loss_mask(camera))
    if inv_depth is not None:
        loss = loss + camera_depth_term(inv_depth[0], camera)
    loss.backward()
    return loss.detach(), means2D.absgrad if getattr(utils.get_args(), "absgrad", False) else means2D.grad
