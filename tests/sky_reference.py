"""The learnable sky in float64 torch, stated from its definition ("Sky"):

    S float [Hs,Ws,3], equirectangular, world axes; R = viewmat[:3,:3] (world -> camera), K = [[fx,0,cx],[0,fy,cy],[0,0,1]]
    dc = ((px + .5 - cx) / fx, (py + .5 - cy) / fy, 1),   d = R^T dc / |dc|
    u  = (atan2(d.x, d.z) / 2pi + .5) Ws - .5        texel column index wraps mod Ws
    v  = (asin(clamp(d.y, -1, 1)) / pi + .5) Hs - .5  texel row index clamps to [0, Hs - 1]
    s  = bilinear(S; u, v)                            four texels, weights >= 0 that sum to 1
    y  = x + (1 - alpha) s

differentiable (autograd) in x, alpha and S; the camera is a constant.  composed with tests/masked_loss_reference.py for
the training loss: y goes to the colour stage / the loss unclamped."""
import math

import torch


def directions(viewmat, K, H, W):
    """World-space unit ray of every pixel centre -> [H,W,3] float64."""
    vm, K = viewmat.double(), K.double()
    py, px = torch.meshgrid(torch.arange(H, dtype=torch.float64), torch.arange(W, dtype=torch.float64), indexing="ij")
    dc = torch.stack([(px + 0.5 - K[0, 2]) / K[0, 0], (py + 0.5 - K[1, 2]) / K[1, 1], torch.ones_like(px)], dim=-1)
    dc = dc / dc.norm(dim=-1, keepdim=True)
    return dc @ vm[:3, :3]  # row vector times R = R^T dc


def coordinates(viewmat, K, H, W, Hs, Ws):
    """(u, v) continuous texel coordinates of every pixel -> two [H,W] float64."""
    d = directions(viewmat, K, H, W)
    u = (torch.atan2(d[..., 0], d[..., 2]) / (2 * math.pi) + 0.5) * Ws - 0.5
    v = (torch.asin(d[..., 1].clamp(-1.0, 1.0)) / math.pi + 0.5) * Hs - 0.5
    return u, v


def taps(viewmat, K, H, W, Hs, Ws):
    """The four texels of every pixel and their weights -> (rows [H,W,4] int64, cols [H,W,4] int64, w [H,W,4] float64)."""
    u, v = coordinates(viewmat, K, H, W, Hs, Ws)
    iu, jv = torch.floor(u), torch.floor(v)
    fu, fv = u - iu, v - jv
    iu, jv = iu.long(), jv.long()
    c0, c1 = iu % Ws, (iu + 1) % Ws
    r0, r1 = jv.clamp(0, Hs - 1), (jv + 1).clamp(0, Hs - 1)
    rows = torch.stack([r0, r0, r1, r1], dim=-1)
    cols = torch.stack([c0, c1, c0, c1], dim=-1)
    w = torch.stack([(1 - fu) * (1 - fv), fu * (1 - fv), (1 - fu) * fv, fu * fv], dim=-1)
    return rows, cols, w


def sample(S, viewmat, K, H, W):
    """s [3,H,W]: the bilinear sample of the map along every pixel's ray (differentiable in S)."""
    Hs, Ws = S.shape[:2]
    rows, cols, w = taps(viewmat, K, H, W, Hs, Ws)
    tex = S.double()[rows, cols]  # [H,W,4,3]
    return (tex * w[..., None]).sum(dim=2).permute(2, 0, 1)


def apply(x, alpha, S, viewmat, K):
    """x [3,H,W] rendered with no background, alpha [H,W] -> y [3,H,W]."""
    _, H, W = x.shape
    return x + (1.0 - alpha.reshape(1, H, W)) * sample(S, viewmat, K, H, W)


def vjp(alpha, S, viewmat, K, g):
    """-> (dL/dalpha [H,W], dL/dS [Hs,Ws,3]) for the cotangent g [3,H,W], written out (not autograd); dL/dx = g."""
    _, H, W = g.shape
    Hs, Ws = S.shape[:2]
    rows, cols, w = taps(viewmat, K, H, W, Hs, Ws)
    s = (S.double()[rows, cols] * w[..., None]).sum(dim=2).permute(2, 0, 1)
    v_alpha = -(g * s).sum(dim=0)
    add = ((1.0 - alpha.reshape(H, W))[..., None] * w)[..., None] * g.permute(1, 2, 0)[:, :, None, :]  # [H,W,4,3]
    v_S = torch.zeros(Hs * Ws, 3, dtype=torch.float64)
    v_S.index_add_(0, (rows * Ws + cols).reshape(-1), add.reshape(-1, 3))
    return v_alpha, v_S.reshape(Hs, Ws, 3)


def look_at_camera(forward, roll=0.0):
    """A world->camera matrix [4,4] float64 at the origin whose +z axis is `forward` (world), x to the right, y down
    (world +y is down; forward = (0, 0, 1) gives the identity), rolled by `roll` radians about the view axis."""
    f = torch.tensor(forward, dtype=torch.float64)
    f = f / f.norm()
    hint = torch.tensor([0.0, 1.0, 0.0], dtype=torch.float64)
    if float(torch.linalg.cross(hint, f).norm()) < 1e-9:  # looking along the world's vertical
        hint = torch.tensor([0.0, 0.0, -1.0], dtype=torch.float64) * float(torch.sign(f[1]))
    x = torch.linalg.cross(hint, f)
    x = x / x.norm()
    y = torch.linalg.cross(f, x)
    if roll:
        c, s_ = math.cos(roll), math.sin(roll)
        x, y = c * x + s_ * y, -s_ * x + c * y
    vm = torch.eye(4, dtype=torch.float64)
    vm[0, :3], vm[1, :3], vm[2, :3] = x, y, f
    return vm


def intrinsics(W, H, fov_x_deg, fy_ratio=1.0, cx=None, cy=None):
    fx = W / (2 * math.tan(math.radians(fov_x_deg) / 2))
    return torch.tensor([[fx, 0, W / 2.0 if cx is None else cx], [0, fx * fy_ratio, H / 2.0 if cy is None else cy],
                         [0, 0, 1]], dtype=torch.float64)
