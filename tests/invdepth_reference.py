"""float64 restatement of the depth regularisation ("Depth regularisation").

  prior   = raw / 65536 * scale + offset                              raw uint16 [H,W]
  L_depth = weight * sum_p m_p |I_p - prior_p| / (H*W)                m_p = 1 unless the loss mask is 0 there
  v_I_p   = weight * m_p * sign(I_p - prior_p) / (H*W)                sign(0) = 0

and the rendered inverse depth I = sum_i w_i / z_i, composed from oracle.gs_oracle: the oracle's rasterizer is linear in
the colours, so I is channel 0 of a second, unchanged call whose colours are (1/z, 0, 0) and whose background is 0."""
import math

import torch

from oracle import gs_oracle as O


def prior_of(raw, scale, offset):
    return raw.to(torch.float64) / 65536.0 * float(scale) + float(offset)


def counted(mask, like):
    return torch.ones_like(like) if mask is None else (mask != 0).to(like.dtype)


def depth_term(I, raw, scale, offset, weight, mask=None):
    """The loss term on a float64 I [H,W]; differentiable in I (torch's d|x|/dx at 0 is 0)."""
    assert I.dtype == torch.float64 and I.dim() == 2
    H, W = I.shape
    d = I - prior_of(raw, scale, offset)
    return float(weight) * (counted(mask, d) * d.abs()).sum() / float(H * W)


def cotangent(I, raw, scale, offset, weight, mask=None):
    """v_I [H,W] float64, written out (not through autograd)."""
    H, W = I.shape
    d = I.to(torch.float64) - prior_of(raw, scale, offset)
    return float(weight) * counted(mask, d) * torch.sign(d) / float(H * W)


def render_with_inverse_depth(means3D, opacities, scales, rotations, shs, sh_degree, viewmat, K, width, height,
                              tile_size=16):
    """-> (image [3,H,W], I [H,W]) in the dtype of the inputs; oracle.gs_oracle.render_one_camera's chain with a second
    rasterize call for the inverse depth (background None in both)."""
    radii, means2d, depths, conics, _ = O.fully_fused_projection(means3D, None, rotations, scales, viewmat[None], K[None],
                                                                 width, height)
    camtoworld = torch.inverse(viewmat[None])
    dirs = means3D[None] - camtoworld[:, None, :3, 3]
    colors = torch.clamp_min(O.spherical_harmonics(sh_degree, dirs, shs[None], masks=radii > 0) + 0.5, 0.0)
    tw, th = math.ceil(width / float(tile_size)), math.ceil(height / float(tile_size))
    _, isect_ids, flatten_ids = O.isect_tiles(means2d, radii, depths, tile_size, tw, th)
    offsets = O.isect_offset_encode(isect_ids, 1, tw, th)
    op = opacities.reshape(1, -1)
    img, _ = O.rasterize_to_pixels(means2d, conics, colors, op, width, height, tile_size, offsets, flatten_ids)
    vis = radii > 0
    inv = torch.where(vis, 1.0 / torch.where(vis, depths, torch.ones_like(depths)), torch.zeros_like(depths))
    inv3 = torch.stack([inv, torch.zeros_like(inv), torch.zeros_like(inv)], -1)
    dimg, _ = O.rasterize_to_pixels(means2d, conics, inv3, op, width, height, tile_size, offsets, flatten_ids)
    return img[0].permute(2, 0, 1).contiguous(), dimg[0, ..., 0]
