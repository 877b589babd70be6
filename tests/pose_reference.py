"""Float64 torch reference of the camera pose refinement (csrc/pose.hip, clm_gs_amd/pose.py): a helper, not a test.

pose_sums_reference is built on oracle.gs_oracle.fully_fused_projection (tests.antialias_reference.projection, its
restatement with the compensation, in antialiased mode) and oracle.gs_oracle.spherical_harmonics, with the view
matrix and the camera centre as two INDEPENDENT leaves -- the kernel does not assume campos = -Rv^T t either.
rot6d, the camera-to-world composition, Adam with weight decay and the learning-rate schedule are written here
independently of clm_gs_amd/pose.py (different operations, same mathematics)."""
import math

import torch

from oracle import gs_oracle as O
from tests import antialias_reference as AR

F64 = torch.float64


def _project(rows, viewmat, K, width, height, antialiased, dtype):
    means = rows["means"].to(dtype)
    quats = rows["quats"].to(dtype)
    scales = torch.exp(rows["log_scales"].to(dtype))
    if antialiased:
        return AR.projection(means, quats, scales, viewmat[None], K[None], width, height)
    return O.fully_fused_projection(means, None, quats, scales, viewmat[None], K[None], width, height)


def oracle_radii(rows, camera):
    """radii [V] of the float64 projection: the rows the oracle itself draws."""
    with torch.no_grad():
        return _project(rows, camera["viewmat"].to(F64), camera["K"].to(F64), camera["width"], camera["height"],
                        False, F64)[0][0]


def pose_sums_reference(rows, camera, lines, dtype=F64):
    """rows: means [V,3], quats [V,4] (raw), log_scales [V,3], opacity_raw [V], shs [V,16,3], radii [V] (the launch's:
    rows with radii <= 0 contribute nothing); camera: viewmat [4,4], K [3,3], campos [3], width, height, degree,
    antialiased; lines [V,9] = x y ca cb cc r g b o.
    -> (v_viewmat [3,4] = v_R | v_t, v_campos [3]): the autograd gradient of
       sum_i <line_i, (means2d, conics, clamp(colour + 0.5), opacity [x compensation])_i>
    with respect to the two leaves, everything evaluated in `dtype`."""
    vm = camera["viewmat"].to(dtype).clone().requires_grad_(True)
    cp = camera["campos"].to(dtype).clone().requires_grad_(True)
    K = camera["K"].to(dtype)
    aa = bool(camera.get("antialiased", False))
    deg = int(camera["degree"])
    vis = (rows["radii"] > 0)
    radii, m2, _, cn, comp = _project(rows, vm, K, camera["width"], camera["height"], aa, dtype)
    means = rows["means"].to(dtype)
    col = O.spherical_harmonics(deg, (means - cp)[None], rows["shs"].to(dtype)[None])
    col = torch.clamp_min(col + 0.5, 0.0)
    g = (lines.to(dtype) * vis[:, None].to(dtype))
    s = (m2[0] * g[:, 0:2]).sum() + (cn[0] * g[:, 2:5]).sum() + (col[0] * g[:, 5:8]).sum()
    if aa:
        s = s + (torch.sigmoid(rows["opacity_raw"].to(dtype)) * comp[0] * g[:, 8]).sum()
    if not s.requires_grad:  # no row at all
        return torch.zeros(3, 4, dtype=dtype), torch.zeros(3, dtype=dtype)
    gv, gc = torch.autograd.grad(s, (vm, cp), allow_unused=True)
    gv = torch.zeros(4, 4, dtype=dtype) if gv is None else gv
    gc = torch.zeros(3, dtype=dtype) if gc is None else gc
    return gv[:3, :4].detach(), gc.detach()


# ---------------------------------------------------------------- the host model, restated
def rot6d(d6):
    """[...,6] -> [...,3,3] (Zhou et al. 2019): rows e1, e2, e1 x e2 of the Gram-Schmidt basis of the two 3-vectors."""
    u, v = d6[..., 0:3], d6[..., 3:6]
    e1 = torch.nn.functional.normalize(u, dim=-1)
    e2 = torch.nn.functional.normalize(v - torch.einsum("...i,...i->...", e1, v)[..., None] * e1, dim=-1)
    e3 = torch.linalg.cross(e1, e2)
    return torch.cat((e1[..., None, :], e2[..., None, :], e3[..., None, :]), dim=-2)


def camtoworld(c2w0, row):
    """One camera: c2w0 [4,4], row [9] = dx | d6 -> c2w0 @ [rot6d(d6 + identity) | dx]."""
    ident = torch.tensor([1.0, 0.0, 0.0, 0.0, 1.0, 0.0], dtype=row.dtype)
    T = torch.cat((torch.cat((rot6d(row[3:] + ident), row[:3].reshape(3, 1)), dim=1),
                   torch.tensor([[0.0, 0.0, 0.0, 1.0]], dtype=row.dtype)), dim=0)
    return c2w0.to(row.dtype) @ T


def camera_of(c2w0, row):
    """-> (viewmat [4,4], campos [3]) of the refined camera, differentiable in `row`."""
    c2w = camtoworld(c2w0, row)
    return torch.linalg.inv(c2w), c2w[:3, 3]


def row_gradient(c2w0, row, v_viewmat, v_campos):
    """d/d row of <v_viewmat, viewmat[:3,:4]> + <v_campos, campos>, one camera, by autograd."""
    r = row.clone().requires_grad_(True)
    vm, cp = camera_of(c2w0, r)
    s = (v_viewmat.to(r.dtype) * vm[:3, :4]).sum() + (v_campos.to(r.dtype) * cp).sum()
    return torch.autograd.grad(s, r)[0]


def schedule(lr, t, max_steps, final_factor=0.01):
    """learning rate of the step taken after t earlier ones: exponential decay to final_factor x lr over max_steps."""
    return lr * math.exp(math.log(final_factor) * min(t, max_steps) / max_steps)


class Adam:
    """Dense Adam with L2 weight decay (torch.optim.Adam's form: the decay joins the gradient), step by step."""

    def __init__(self, table, lr, reg, max_steps, beta1=0.9, beta2=0.999, eps=1e-8):
        self.p = table.clone()
        self.m, self.v = torch.zeros_like(self.p), torch.zeros_like(self.p)
        self.lr, self.reg, self.max_steps, self.b1, self.b2, self.eps, self.t = lr, reg, max_steps, beta1, beta2, eps, 0

    def step(self, grad):
        lr = schedule(self.lr, self.t, self.max_steps)
        self.t += 1
        g = grad + self.reg * self.p
        self.m = self.b1 * self.m + (1 - self.b1) * g
        self.v = self.b2 * self.v + (1 - self.b2) * g * g
        mhat = self.m / (1 - self.b1 ** self.t)
        vhat = self.v / (1 - self.b2 ** self.t)
        self.p = self.p - lr * mhat / (vhat.sqrt() + self.eps)
        return self.p


# ---------------------------------------------------------------- end to end: the reference trajectory
def eight_cameras(base_viewmat, n=8):
    """World-to-camera matrices [n,4,4] (float32) around tests.scenes.small_scene's camera: small rotations about the
    camera's y and x axes and shifts, every one looking at the cloud."""
    out = []
    for i in range(n):
        ay, ax = 0.06 * (i - (n - 1) / 2.0), 0.04 * ((i * 3) % n - (n - 1) / 2.0)
        Ry = torch.tensor([[math.cos(ay), 0, math.sin(ay)], [0, 1, 0], [-math.sin(ay), 0, math.cos(ay)]], dtype=F64)
        Rx = torch.tensor([[1, 0, 0], [0, math.cos(ax), -math.sin(ax)], [0, math.sin(ax), math.cos(ax)]], dtype=F64)
        T = torch.eye(4, dtype=F64)
        T[:3, :3] = Rx @ Ry
        T[:3, 3] = torch.tensor([0.15 * math.sin(1.7 * i), 0.1 * math.cos(2.3 * i), 0.05 * i], dtype=F64)
        out.append((T @ base_viewmat.to(F64)).to(torch.float32))
    return torch.stack(out)


def trajectory(scene, c2w0, K, width, height, table0, gts, batches, lr, reg, max_steps, dtype=F64):
    """The float reference of a pose-only training run: per batch, for each of its cameras the oracle render at the
    refined pose (oracle.gs_oracle.render_one_camera, degree 3), oracle.gs_oracle.training_loss against gts[i], the
    gradient of the row by autograd through the composition above; then one step of Adam above on the whole table.
    scene: means, opac (activated [N,1]), scales (activated), quats, shs [N,16,3].  -> (tables [K+1,n,9], gradients: a
    list per batch of [b,9])."""
    P = [scene[k].to(dtype) for k in ("means", "opac", "scales", "quats", "shs")]
    opt = Adam(table0.to(dtype), lr, reg, max_steps)
    tables, grads = [opt.p.clone()], []
    for ids in batches:
        grad = torch.zeros_like(opt.p)
        gb = []
        for i in ids:
            r = opt.p[i].clone().requires_grad_(True)
            vm, _ = camera_of(c2w0[i].to(dtype), r)
            img, _, _, _ = O.render_one_camera(*P, 3, vm, K.to(dtype), width, height)
            g = torch.autograd.grad(O.training_loss(img, gts[i]), r)[0]
            grad[i] += g
            gb.append(g)
        grads.append(torch.stack(gb))
        tables.append(opt.step(grad).clone())
    return torch.stack(tables), grads


def mean_translation_error(c2w0, table):
    """Mean over the cameras of |centre(refined) - centre(as loaded)|."""
    return float(torch.stack([(camtoworld(c2w0[i].to(table.dtype), table[i])[:3, 3] - c2w0[i, :3, 3].to(table.dtype)).norm()
                              for i in range(table.shape[0])]).mean())
