"""Float64 reference of gsplat's antialiased mode (fully_fused_projection(calc_compensations=True), Mip-Splatting): a
helper, not a test.

projection() restates oracle/gs_oracle.py::fully_fused_projection operation for operation (tests/test_antialias_cpu.py
holds the two to each other) and keeps the un-blurred 2D covariance, from which
    compensation = sqrt(max(0, det(cov2d) / det(cov2d + eps2d I)))
is formed; det(cov2d) comes from the un-blurred entries directly.  guarded=True takes the square root through
GuardedSqrt, whose derivative is gsplat's 0.5 / (compensation + 1e-6), so that the reference is gsplat's arithmetic and
not a neighbouring one; guarded=False is plain autograd."""
import torch

from oracle import gs_oracle as O


class GuardedSqrt(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        y = torch.sqrt(x)
        ctx.save_for_backward(y)
        return y

    @staticmethod
    def backward(ctx, v):
        (y,) = ctx.saved_tensors
        return v * 0.5 / (y + 1e-6)


def projection(means, quats, scales, viewmats, Ks, width, height, eps2d=0.3, near_plane=0.01, far_plane=1e10,
               radius_clip=0.0, guarded=True, details=None):
    """-> radii[C,N] i32, means2d[C,N,2], depths[C,N], conics[C,N,3], compensations[C,N] (0 where culled).
    `details`: a dict that receives the values the culls compare (detached): z, the real-valued radius 3 sqrt(v1), its
    ceiling, the pixel mean and the four partial verdicts -- for tests that keep a scene clear of these decisions."""
    C, N = viewmats.shape[0], means.shape[0]
    dt = means.dtype
    Rv, tv = viewmats[:, :3, :3], viewmats[:, :3, 3]
    mean_c = torch.einsum("cij,nj->cni", Rv, means) + tv[:, None, :]
    z_raw = mean_c[..., 2]
    ok_z = (z_raw >= near_plane) & (z_raw <= far_plane)
    safe = torch.where(ok_z[..., None], mean_c, torch.tensor([0.0, 0.0, 1.0], dtype=dt))
    x, y, z = safe.unbind(-1)
    covar = O.quat_scale_to_covar(quats, scales)
    covar_c = torch.einsum("cij,njk,clk->cnil", Rv, covar, Rv)
    fx, fy = Ks[:, 0, 0][:, None], Ks[:, 1, 1][:, None]
    cx, cy = Ks[:, 0, 2][:, None], Ks[:, 1, 2][:, None]
    tan_fovx, tan_fovy = 0.5 * width / fx, 0.5 * height / fy
    lim_x_pos = (width - cx) / fx + 0.3 * tan_fovx
    lim_x_neg = cx / fx + 0.3 * tan_fovx
    lim_y_pos = (height - cy) / fy + 0.3 * tan_fovy
    lim_y_neg = cy / fy + 0.3 * tan_fovy
    rz = 1.0 / z
    rz2 = rz * rz
    tx = z * torch.minimum(lim_x_pos, torch.maximum(-lim_x_neg, x * rz))
    ty = z * torch.minimum(lim_y_pos, torch.maximum(-lim_y_neg, y * rz))
    zero = torch.zeros_like(z)
    J = torch.stack([fx * rz, zero, -fx * tx * rz2, zero, fy * rz, -fy * ty * rz2], dim=-1).reshape(C, N, 2, 3)
    cov2d = J @ covar_c @ J.transpose(-1, -2)  # un-blurred
    mu_x = fx * x * rz + cx
    mu_y = fy * y * rz + cy
    c00 = cov2d[..., 0, 0] + eps2d
    c01 = cov2d[..., 0, 1]
    c11 = cov2d[..., 1, 1] + eps2d
    det = c00 * c11 - c01 * c01
    det_orig = cov2d[..., 0, 0] * cov2d[..., 1, 1] - c01 * c01
    ok_det = det > 0
    det_s = torch.where(ok_det, det, torch.ones_like(det))
    conic = torch.stack([c11 / det_s, -c01 / det_s, c00 / det_s], dim=-1)
    b = 0.5 * (c00 + c11)
    v1 = b + torch.sqrt(torch.clamp(b * b - det, min=0.01))
    radius = torch.ceil(3.0 * torch.sqrt(v1)).detach()
    ok_r = radius > radius_clip
    ok_img = ~((mu_x + radius <= 0) | (mu_x - radius >= width) | (mu_y + radius <= 0) | (mu_y - radius >= height))
    valid = ok_z & ok_det & ok_r & ok_img
    if details is not None:
        details.update(z=z_raw.detach(), radius_real=(3.0 * torch.sqrt(v1)).detach(), radius=radius, mu_x=mu_x.detach(),
                       mu_y=mu_y.detach(), ok_z=ok_z, ok_det=ok_det, ok_r=ok_r, ok_img=ok_img, tx_over_z=(x * rz).detach(),
                       lim_x=(lim_x_neg, lim_x_pos))
    ratio = torch.clamp(det_orig / det_s, min=0.0)
    ratio = torch.where(valid, ratio, torch.ones_like(ratio))  # culled pairs: no 0/0 in the square root's derivative
    comp = (GuardedSqrt.apply(ratio) if guarded else torch.sqrt(ratio)) * valid
    radii = torch.where(valid, radius, torch.zeros_like(radius)).to(torch.int32)
    means2d = torch.stack([mu_x, mu_y], dim=-1) * valid[..., None]
    return radii, means2d, z * valid, conic * valid[..., None], comp


def scene_f64(s):
    """means, quats, scales of a tests.scenes scene as float64 leaves, and its camera [1,4,4], [1,3,3]."""
    leaves = [s[k].double().clone().requires_grad_() for k in ("means", "quats", "scales")]
    return leaves, s["viewmat"].double()[None], s["K"].double()[None]


def render_one_camera(means3D, opacities, scales, rotations, shs, sh_degree, viewmat, K, width, height, background=None,
                      tile_size=16):
    """oracle.gs_oracle.render_one_camera with rasterize_mode="antialiased": the projection above, and the oracle's SH,
    binning and rasterizer on opacities * compensations.  -> image[3,H,W], means2d, radii, aux (+ compensations)."""
    import math
    radii, means2d, depths, conics, comps = projection(means3D, rotations, scales, viewmat[None], K[None], width, height)
    dirs = means3D[None] - torch.inverse(viewmat[None])[:, None, :3, 3]
    colors = torch.clamp_min(O.spherical_harmonics(sh_degree, dirs, shs[None], masks=radii > 0) + 0.5, 0.0)
    tw, th = math.ceil(width / float(tile_size)), math.ceil(height / float(tile_size))
    _, isect_ids, flatten_ids = O.isect_tiles(means2d, radii, depths, tile_size, tw, th)
    offsets = O.isect_offset_encode(isect_ids, 1, tw, th)
    bg = background.reshape(1, 3) if background is not None else None
    img, alpha = O.rasterize_to_pixels(means2d, conics, colors, opacities.reshape(1, -1) * comps, width, height, tile_size,
                                       offsets, flatten_ids, backgrounds=bg)
    return img[0].permute(2, 0, 1).contiguous(), means2d, radii, dict(
        depths=depths, conics=conics, colors=colors, flatten_ids=flatten_ids, offsets=offsets, alpha=alpha,
        compensations=comps)
