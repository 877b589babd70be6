"""Float64 reference of the orthographic camera model (gsplat's camera_model="ortho"): a helper, not a test.

projection() restates clm_gs_amd/csrc/ortho_math.h from its formulas: p = R m + t, cull on the planes, the camera-space
covariance from the oracle's quat_scale_to_covar, the constant Jacobian J = [[sx,0,0],[0,sy,0]], cov2d = J Sc J^T (+ eps2d
on the diagonal), means2d = (sx p.x + cx, sy p.y + cy), depth = p.z; radius, radius_clip, the off-screen tests, the conic
and the guarded compensation are those of tests/antialias_reference.py (the pinhole reference).  It evaluates in the dtype
of its inputs, so the float32 evaluation the tests quote is the same code.  render() composes it with the oracle's SH --
along ONE direction, the world-space optical axis viewmat[2,:3] -- binning and rasterizer."""
import math

import torch

from oracle import gs_oracle as O
from tests.antialias_reference import GuardedSqrt


def ortho_K(pixels_per_unit, width, height, cx=None, cy=None, dtype=torch.float32):
    sx, sy = (pixels_per_unit, pixels_per_unit) if not isinstance(pixels_per_unit, (tuple, list)) else pixels_per_unit
    return torch.tensor([[sx, 0, width / 2.0 if cx is None else cx], [0, sy, height / 2.0 if cy is None else cy],
                         [0, 0, 1]], dtype=dtype)


def projection(means, quats, scales, viewmats, Ks, width, height, eps2d=0.3, near_plane=0.01, far_plane=1e10,
               radius_clip=0.0, guarded=True):
    """-> radii[C,N] i32, means2d[C,N,2], depths[C,N], conics[C,N,3], compensations[C,N] (all 0 where culled)."""
    Rv, tv = viewmats[:, :3, :3], viewmats[:, :3, 3]
    p = torch.einsum("cij,nj->cni", Rv, means) + tv[:, None, :]
    z = p[..., 2]
    ok_z = (z >= near_plane) & (z <= far_plane)
    covar = O.quat_scale_to_covar(quats, scales)
    Sc = torch.einsum("cij,njk,clk->cnil", Rv, covar, Rv)
    sx, sy = Ks[:, 0, 0][:, None], Ks[:, 1, 1][:, None]
    cx, cy = Ks[:, 0, 2][:, None], Ks[:, 1, 2][:, None]
    o00, o01, o11 = sx * sx * Sc[..., 0, 0], sx * sy * Sc[..., 0, 1], sy * sy * Sc[..., 1, 1]
    c00, c01, c11 = o00 + eps2d, o01, o11 + eps2d
    det = c00 * c11 - c01 * c01
    det_orig = o00 * o11 - o01 * o01
    ok_det = det > 0
    det_s = torch.where(ok_det, det, torch.ones_like(det))
    conic = torch.stack([c11 / det_s, -c01 / det_s, c00 / det_s], dim=-1)
    mu_x, mu_y = sx * p[..., 0] + cx, sy * p[..., 1] + cy
    b = 0.5 * (c00 + c11)
    v1 = b + torch.sqrt(torch.clamp(b * b - det, min=0.01))
    radius = torch.ceil(3.0 * torch.sqrt(v1)).detach()
    ok_r = radius > radius_clip
    ok_img = ~((mu_x + radius <= 0) | (mu_x - radius >= width) | (mu_y + radius <= 0) | (mu_y - radius >= height))
    valid = ok_z & ok_det & ok_r & ok_img
    ratio = torch.clamp(det_orig / det_s, min=0.0)
    ratio = torch.where(valid, ratio, torch.ones_like(ratio))
    comp = (GuardedSqrt.apply(ratio) if guarded else torch.sqrt(ratio)) * valid
    radii = torch.where(valid, radius, torch.zeros_like(radius)).to(torch.int32)
    means2d = torch.stack([mu_x, mu_y], dim=-1) * valid[..., None]
    return radii, means2d, z * valid, conic * valid[..., None], comp


def cull_reasons(means, quats, scales, viewmat, K, width, height, near_plane=0.01):
    """Counts for one camera: (visible, culled by the near plane, culled off-screen among the rest)."""
    r = projection(means, quats, scales, viewmat[None], K[None], width, height, near_plane=near_plane)[0][0]
    z = (viewmat[:3, :3] @ means.T).T[:, 2] + viewmat[2, 3]
    near = z < near_plane
    return int((r > 0).sum()), int(near.sum()), int(((r == 0) & ~near).sum())


def axis_dirs(viewmat, n):
    """The one view direction of a parallel projection: the world-space optical axis, for n rows -> [1,n,3]."""
    return viewmat[2, :3].reshape(1, 1, 3).expand(1, n, 3)


def render(means, opacities, scales, quats, shs, sh_degree, viewmat, K, width, height, background=None,
           antialiased=False, depth=False, dirs=None, tile_size=16):
    """One orthographic camera in the dtype of the inputs: projection above, SH along the axis (or `dirs`), oracle binning
    and rasterizer.  -> image[3,H,W], alpha[H,W], expected depth[H,W] | None (D / clamp(alpha, 1e-10): "RGB+ED")."""
    N = means.shape[0]
    radii, m2, d, cn, comps = projection(means, quats, scales, viewmat[None], K[None], width, height)
    dirs = axis_dirs(viewmat, N) if dirs is None else dirs
    colors = torch.clamp_min(O.spherical_harmonics(sh_degree, dirs, shs[None], masks=radii > 0) + 0.5, 0.0)
    tw, th = math.ceil(width / float(tile_size)), math.ceil(height / float(tile_size))
    _, ids, fids = O.isect_tiles(m2, radii, d, tile_size, tw, th)
    off = O.isect_offset_encode(ids, 1, tw, th)
    op = opacities.reshape(1, -1)
    if antialiased:
        op = op * comps
    bg = background.reshape(1, 3) if background is not None else None
    img, alpha = O.rasterize_to_pixels(m2, cn, colors, op, width, height, tile_size, off, fids, backgrounds=bg)
    ed = None
    if depth:
        zc = torch.stack([d, torch.zeros_like(d), torch.zeros_like(d)], -1)
        dimg, _ = O.rasterize_to_pixels(m2, cn, zc, op, width, height, tile_size, off, fids)
        ed = dimg[0, ..., 0] / alpha[0, ..., 0].clamp(min=1e-10)
    return img[0].permute(2, 0, 1).contiguous(), alpha[0, ..., 0], ed
