"""Per-camera exposure compensation in float64 torch, stated from its definition ("Exposure"; the
convention of the INRIA 3DGS code base's exposure.json):

    E float [3,4], x the rendered pixel:   y[c] = x[0] E[0][c] + x[1] E[1][c] + x[2] E[2][c] + E[c][3]
    with g[c] = dL/dy[c]:                  dL/dx[k]    = E[k][0] g[0] + E[k][1] g[1] + E[k][2] g[2]
                                           dL/dE[k][c] = sum_p x[k] g[c]   (c < 3)
                                           dL/dE[c][3] = sum_p g[c]

composed with tests/masked_loss_reference.py for the training loss: y goes to the loss unclamped."""
import torch

from tests import masked_loss_reference as M


def identity(dtype=torch.float64):
    return torch.eye(3, 4, dtype=dtype)


def apply(x, E):
    """x [3,H,W], E [3,4] -> y [3,H,W]."""
    return torch.einsum("khw,kc->chw", x, E[:, :3]) + E[:, 3][:, None, None]


def vjp(x, E, g):
    """-> (dL/dx [3,H,W], dL/dE [3,4]) of y = apply(x, E) for the cotangent g [3,H,W], written out (not autograd)."""
    v_x = torch.einsum("kc,chw->khw", E[:, :3], g)
    v_E = torch.zeros_like(E)
    v_E[:, :3] = torch.einsum("khw,chw->kc", x, g)
    v_E[:, 3] = g.sum(dim=(1, 2))
    return v_x, v_E


def magnitude_fwd(x, E):
    """sum_k |x[k]| |E[k][c]| + |E[c][3]| per element of y: what the forward's rounding errors scale with."""
    return apply(x.abs(), E.abs())


def magnitude_vjp(x, E, g):
    """The same for the two gradients: (sum_c |E[k][c]| |g[c]|, sum_p |x[k]| |g[c]| resp. sum_p |g[c]|)."""
    return vjp(x.abs(), E.abs(), g.abs())


def loss(x, E, gt_u8, mask=None, lambda_dssim=0.2):
    """The training loss of a camera with an exposure: masked_loss(apply(x, E), ...)."""
    return M.masked_loss(apply(x, E), gt_u8, mask, lambda_dssim)
