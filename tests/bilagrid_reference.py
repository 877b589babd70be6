"""Bilateral-grid colour correction in float64 torch, stated from its definition ("Bilateral grid";
gsplat's `use_bilateral_grid` operator):

    G float [L,Hg,Wg,12] (coefficient 4c + k = A[c][k]), x the rendered pixel (px, py) of an H x W image:
    u = (px + .5) / W, v = (py + .5) / H, s = .299 x[0] + .587 x[1] + .114 x[2]
    A = F.grid_sample(G as [1,12,L,Hg,Wg], 2 (u, v, s) - 1, bilinear, align_corners=True, padding_mode="border")
    y[c] = A[c][0] x[0] + A[c][1] x[1] + A[c][2] x[2] + A[c][3]

gradients by autograd; composed with tests/masked_loss_reference.py for the training loss (y goes to the loss
unclamped).  `parts` restates the slice by hand (corners and weights) for the error bounds of the GPU tests; the CPU test
holds the two against each other and against a plain loop."""
import torch
import torch.nn.functional as F

from tests import masked_loss_reference as M

LUM = (0.299, 0.587, 0.114)
U = 2.0 ** -24  # unit roundoff of float32


def identity(L, Hg, Wg, dtype=torch.float64):
    eye = torch.tensor([1.0, 0, 0, 0, 0, 1.0, 0, 0, 0, 0, 1.0, 0], dtype=dtype)
    return eye.repeat(L, Hg, Wg, 1)


def luminance(x):
    return LUM[0] * x[0] + LUM[1] * x[1] + LUM[2] * x[2]


def slice_grid(x, G):
    """x [3,H,W], G [L,Hg,Wg,12] -> A [12,H,W], the per-pixel affine transform (differentiable in both)."""
    _, H, W = x.shape
    u = ((torch.arange(W, dtype=x.dtype) + 0.5) / W)[None, :].expand(H, W)
    v = ((torch.arange(H, dtype=x.dtype) + 0.5) / H)[:, None].expand(H, W)
    coords = torch.stack([u, v, luminance(x)], dim=-1) * 2.0 - 1.0
    return F.grid_sample(G.permute(3, 0, 1, 2)[None], coords[None, None], mode="bilinear", padding_mode="border",
                         align_corners=True)[0, :, 0]


def affine(A, x):
    """A [12,H,W], x [3,H,W] -> y [3,H,W]."""
    A = A.reshape(3, 4, *x.shape[1:])
    return (A[:, :3] * x[None]).sum(dim=1) + A[:, 3]


def apply(x, G):
    return affine(slice_grid(x, G), x)


def vjp(x, G, g):
    """-> (dL/dx [3,H,W], dL/dG [L,Hg,Wg,12]) of y = apply(x, G) for the cotangent g, by autograd."""
    xr, Gr = x.detach().clone().requires_grad_(), G.detach().clone().requires_grad_()
    apply(xr, Gr).backward(g)
    return xr.grad, Gr.grad


def loss(x, G, gt_u8, mask=None, lambda_dssim=0.2):
    """The training loss of a camera with a grid: masked_loss(apply(x, G), ...)."""
    return M.masked_loss(apply(x, G), gt_u8, mask, lambda_dssim)


def tv(table):
    """table [n,L,Hg,Wg,12]: (1/n) sum_axis sum (difference along the axis)^2 / (12 x differences per grid)."""
    n, L, Hg, Wg, _ = table.shape
    total = 0.0
    for dim, count in ((1, (L - 1) * Hg * Wg), (2, L * (Hg - 1) * Wg), (3, L * Hg * (Wg - 1))):
        d = table.narrow(dim, 1, table.shape[dim] - 1) - table.narrow(dim, 0, table.shape[dim] - 1)
        total = total + (d * d).sum() / (12 * count)
    return total / n


def tv_grad(table, weight):
    t = table.detach().clone().requires_grad_()
    (weight * tv(t)).backward()
    return t.grad


def parts(x, G):
    """The slice written out per pixel (float64, no autograd): lattice coordinates, the 8 corners C [H,W,2,2,2,12] (z, y, x),
    the trilinear weights w [H,W,2,2,2], node indices, A, A_lo, A_hi."""
    L, Hg, Wg, _ = G.shape
    _, H, W = x.shape
    fx = ((torch.arange(W, dtype=x.dtype) + 0.5) / W * (Wg - 1))[None, :].expand(H, W)
    fy = ((torch.arange(H, dtype=x.dtype) + 0.5) / H * (Hg - 1))[:, None].expand(H, W)
    s = luminance(x)
    fz = s.clamp(0.0, 1.0) * (L - 1)
    x0, y0, z0 = fx.floor().clamp(max=Wg - 2).long(), fy.floor().clamp(max=Hg - 2).long(), fz.floor().clamp(max=L - 2).long()
    tx, ty, tz = fx - x0, fy - y0, fz - z0
    C = torch.stack([torch.stack([torch.stack([G[z0 + dz, y0 + dy, x0 + dx] for dx in (0, 1)], dim=2) for dy in (0, 1)], dim=2)
                     for dz in (0, 1)], dim=2)
    wz, wy, wx = torch.stack([1 - tz, tz], -1), torch.stack([1 - ty, ty], -1), torch.stack([1 - tx, tx], -1)
    w = wz[..., :, None, None] * wy[..., None, :, None] * wx[..., None, None, :]
    wxy = wy[..., :, None] * wx[..., None, :]
    A_lo, A_hi = (wxy[..., None] * C[:, :, 0]).sum(dim=(2, 3)), (wxy[..., None] * C[:, :, 1]).sum(dim=(2, 3))
    A = (w[..., None] * C).sum(dim=(2, 3, 4))
    return dict(fx=fx, fy=fy, fz=fz, s=s, x0=x0, y0=y0, z0=z0, tx=tx, ty=ty, tz=tz, C=C, w=w, wz=wz, wy=wy, wx=wx, A=A,
                A_lo=A_lo, A_hi=A_hi, inside=(s > 0) & (s < 1))


def bounds(x, G, g, chain):
    """Per-element bounds of the float32 kernels' distance from this restatement, in the form U x sum of |terms| with the
    factors COUNTED from the operation chains of csrc/bilagrid.hip (first order in U; `chain` is the length of the
    summation chain behind one element of dL/dG).  With B = max |corner| per coefficient:
      coordinates   fx = ((px + .5) / W) (Wg - 1): two roundings, |dfx| <= 2 U fx (fy likewise); tx = fx - x0 is exact;
                    s: the three constants (U each, relative) + one product and two fmas: |ds| <= 4 U sum_k lum_k |x_k|;
                    fz = clamp(s) (L - 1): |dfz| <= (L - 1) |ds| + U fz, and 0 where s is clamped (the test keeps s 1e-3
                    away from 0, 1 and the level boundaries, so both precisions take the same side);
      a lerp        fmaf(t, b - a, a): U (|a| + |b|) from the subtraction + U |result| from the fma <= 3 U B; errors of the
                    inputs pass through as a convex combination: A_lo / A_hi carry 6 U B, A 9 U B;
                    a coordinate error moves A by |dA/dt| |dt| (A is linear in each t);
      y[c]          a product, two fmas, an addition: 4 U sum_k |A_ck| |x_k| + sum_k |dA_ck| |x_k|        (x_3 = 1)
      dL/dx[k]      sum_c A_ck g_c the same way (3 roundings, + 1 for the fma that adds the guidance term), and
                    lumL_k d with lumL_k = .299f (L - 1) (2 U relative), D = A_hi - A_lo (U |D| + 12 U B + its coordinate
                    part), T_c = sum_k D_ck x_k (4 roundings), d = sum_c g_c T_c (3 roundings)
      dL/dG         every term w g_c x_k: 1 - tx, 1 - ty, 1 - tz, two products for w, one for g_c x_k = 6 U relative,
                    + |dw| |g_c x_k| from the coordinates, + the chain: (chain) U sum_p |terms|.
    -> (b_y [3,H,W], b_v [3,H,W], b_G [L,Hg,Wg,12])"""
    L, Hg, Wg, _ = G.shape
    P = parts(x, G)
    _, H, W = x.shape
    C, w = P["C"], P["w"]
    B = C.abs().amax(dim=(2, 3, 4))                                          # [H,W,12]
    xa = torch.cat([x.abs(), torch.ones_like(x[:1])]).permute(1, 2, 0)        # [H,W,4], x_3 = 1
    ga = g.abs().permute(1, 2, 0)                                              # [H,W,3]
    wz, wy, wx = P["wz"], P["wy"], P["wx"]
    wyz, wxz, wxy = wz[..., :, None] * wy[..., None, :], wz[..., :, None] * wx[..., None, :], wy[..., :, None] * wx[..., None, :]
    dAx = (wyz[..., None] * (C[:, :, :, :, 1] - C[:, :, :, :, 0])).sum(dim=(2, 3)).abs()
    dAy = (wxz[..., None] * (C[:, :, :, 1] - C[:, :, :, 0])).sum(dim=(2, 3)).abs()
    D = P["A_hi"] - P["A_lo"]
    dDx = (wy[..., :, None] * ((C[:, :, 1, :, 1] - C[:, :, 1, :, 0]) - (C[:, :, 0, :, 1] - C[:, :, 0, :, 0]))).sum(dim=2).abs()
    dDy = (wx[..., :, None] * ((C[:, :, 1, 1] - C[:, :, 1, 0]) - (C[:, :, 0, 1] - C[:, :, 0, 0]))).sum(dim=2).abs()
    efx, efy = 2 * P["fx"], 2 * P["fy"]
    lum_abs = sum(LUM[k] * x[k].abs() for k in range(3))
    efz = torch.where(P["inside"], (L - 1) * 4 * lum_abs + P["fz"], torch.zeros_like(lum_abs))
    dA = 9 * B + efx[..., None] * dAx + efy[..., None] * dAy + efz[..., None] * D.abs()          # units of U
    A34, dA34 = P["A"].abs().reshape(H, W, 3, 4), dA.reshape(H, W, 3, 4)
    b_y = U * (4 * (A34 * xa[..., None, :]).sum(-1) + (dA34 * xa[..., None, :]).sum(-1)).permute(2, 0, 1)
    # dL/dx
    first = 4 * (A34[..., :3] * ga[..., :, None]).sum(2) + (dA34[..., :3] * ga[..., :, None]).sum(2)       # [H,W,3(k)]
    dD = D.abs() + 12 * B + efx[..., None] * dDx + efy[..., None] * dDy
    D34, dD34 = D.abs().reshape(H, W, 3, 4), dD.reshape(H, W, 3, 4)
    Tm = (D34 * xa[..., None, :]).sum(-1)                                      # [H,W,3(c)]
    dT = 4 * Tm + (dD34 * xa[..., None, :]).sum(-1)
    dm = (ga * Tm).sum(-1)
    dd = 3 * dm + (ga * dT).sum(-1)
    lumL = torch.tensor(LUM, dtype=x.dtype) * (L - 1)
    second = torch.where(P["inside"], dd + 3 * dm, torch.zeros_like(dm))[..., None] * lumL
    b_v = U * (first + second).permute(2, 0, 1)
    # dL/dG: scatter the per-pixel magnitudes to the nodes
    gx = (ga[..., :, None] * xa[..., None, :]).reshape(H, W, 12)                # |g_c x_k|
    dw = efx[..., None, None, None] * wyz[..., :, :, None] + efy[..., None, None, None] * wxz[..., :, None, :] \
        + efz[..., None, None, None] * wxy[..., None, :, :]
    per = ((6 + chain) * w + dw)[..., None] * gx[:, :, None, None, None, :]    # [H,W,2,2,2,12]
    b_G = torch.zeros(L * Hg * Wg, 12, dtype=x.dtype)
    for dz in (0, 1):
        for dy in (0, 1):
            for dx in (0, 1):
                idx = ((P["z0"] + dz) * Hg + (P["y0"] + dy)) * Wg + (P["x0"] + dx)
                b_G.index_add_(0, idx.reshape(-1), per[:, :, dz, dy, dx].reshape(-1, 12))
    return b_y, b_v, U * b_G.reshape(L, Hg, Wg, 12)
