"""Float64 reference of the fused front end (csrc/preprocess.hip) for the rows of one filter: a helper, not a test.

reference() composes what the two kernels compute: raw attributes -> exp / sigmoid (the projection normalises the
quaternion) -> tests/antialias_reference.py::projection -> the oracle's SH masked by radii > 0 -> +0.5, clamp at 0; the
opacity is multiplied by the compensation only when `aa` is set.  Given gradient lines  x y ca cb | cc r g b | o  it
returns the gradients of the five raw parameter groups, scattered to row ids, by autograd.  statistics() restates the
densification statistics in numpy.  scene() is the 400-row scene of the kernel tests with its special rows, margins()
says how far a scene keeps from the float32 kernel's decisions, tiled_scene() repeats the scene with a jitter.
tests/test_front_end_cpu.py holds all of it to independent computations."""
import functools

import numpy as np
import torch

from oracle import gs_oracle as O
from tests import antialias_reference as R

F64, F32 = torch.float64, torch.float32
GROUPS = ("xyz", "opacity", "scaling", "rotation", "shs")
MARGIN = 1e-3  # pixels / depth units: about thirty times the float32 error of a 30-pixel radius
# the culls the forward cases run: defaults, and one threshold each that has scene rows on both sides
CULLS = {"default": dict(near_plane=0.01, far_plane=1e10, radius_clip=0.0), "near": dict(near_plane=5.5, far_plane=1e10, radius_clip=0.0),
         "far": dict(near_plane=0.01, far_plane=7.0, radius_clip=0.0), "clip": dict(near_plane=0.01, far_plane=1e10, radius_clip=6.5)}
# special rows of scene(): 7 and 11 clamped in tx, 13 every colour channel below the clamp (tests/test_gpu_pose.py),
# and the five added here
SPECIAL = dict(clamped_tx=(7, 11), dark=13, one_channel=17, behind=19, far=23, tiny=29, off_screen=31)


def campos_of(viewmat):
    return torch.inverse(viewmat.double())[:3, 3]


def reference(raw, rows, cam, deg, aa, lines=None, dtype=F64, guarded=True, details=None, near_plane=0.01, far_plane=1e10,
              radius_clip=0.0):
    """raw: xyz[N,3] opacity[N] scaling[N,3] rotation[N,4] shs[N,48]; rows: int64 row ids or None (all rows, in order);
    cam: viewmat[4,4], K[3,3], width, height.  -> radii m2 dep cn col op comp (forward outputs of the rows, detached; op is
    sigmoid(o) for every row when aa is off, sigmoid(o) * compensation when it is on) and, with lines[V,>=9], grads: the
    five raw-parameter gradients [N,...] (zero outside the rows and for rows with radius 0)."""
    P = {k: raw[k].to(dtype).clone().requires_grad_() for k in GROUPS}
    idx = rows if rows is not None else torch.arange(raw["xyz"].shape[0])
    vm, K = cam["viewmat"].to(dtype), cam["K"].to(dtype)
    xyz = P["xyz"][idx]
    radii, m2, d, cn, comp = R.projection(xyz, P["rotation"][idx], torch.exp(P["scaling"][idx]), vm[None], K[None], cam["width"],
                                          cam["height"], near_plane=near_plane, far_plane=far_plane, radius_clip=radius_clip,
                                          guarded=guarded, details=details)
    dirs = xyz[None] - campos_of(cam["viewmat"]).to(dtype)
    col = torch.clamp_min(O.spherical_harmonics(deg, dirs, P["shs"][idx].reshape(1, -1, 16, 3), masks=radii > 0) + 0.5, 0.0)
    sig = torch.sigmoid(P["opacity"][idx])[None]
    op = sig * comp if aa else sig
    out = dict(radii=radii[0], m2=m2[0].detach(), dep=d[0].detach(), cn=cn[0].detach(), col=col[0].detach(), op=op[0].detach(),
               comp=comp[0].detach())
    if lines is not None:
        g = lines.to(dtype)
        vis = (radii[0] > 0).to(dtype)  # a culled row receives nothing (the compensation carries the mask itself)
        ((m2[0] * g[:, 0:2]).sum() + (cn[0] * g[:, 2:5]).sum() + (col[0] * g[:, 5:8]).sum() + (op[0] * vis * g[:, 8]).sum()).backward()
        out["grads"] = {k: (v.grad if v.grad is not None else torch.zeros_like(v)) for k, v in P.items()}
    return out


def statistics(max_radii, grad_accum, denom, rows, radii, lines, width, height, abs_pair=False, only_visible=False):
    """The densification statistics after one launch, float64 numpy: for every filter row (only_visible: every row with
    radius > 0)  max_radii = max(old, radius), grad_accum += sqrt((gx W/2)^2 + (gy H/2)^2) from words 0 and 1 of the
    row's line (abs_pair: words 10 and 11), denom += 1.  rows hold each id once."""
    as_np = lambda t: t.detach().cpu().numpy() if torch.is_tensor(t) else np.asarray(t)
    mr, ga, dn = (as_np(t).astype(np.float64) for t in (max_radii, grad_accum, denom))  # (astype copies)
    rows, radii, lines = as_np(rows), as_np(radii), as_np(lines).astype(np.float64)
    sel = radii > 0 if only_visible else np.ones(rows.shape, dtype=bool)
    a, b = (10, 11) if abs_pair else (0, 1)
    r = rows[sel]
    mr[r] = np.maximum(mr[r], radii[sel].astype(np.float64))
    ga[r] += np.sqrt((lines[sel, a] * (0.5 * width)) ** 2 + (lines[sel, b] * (0.5 * height)) ** 2)
    dn[r] += 1.0
    return mr, ga, dn


# ------------------------------------------------------------------------------------------------ scene
def margins(raw, cam, cull):
    """Distance of every row from the decisions the float32 kernel takes, as the float64 reference sees them, for one cull
    setting -> dict of [N] tensors (inf where the comparison is not reached): `ceil` |3 sqrt(v1) - nearest integer|,
    `depth` to near_plane / far_plane, `clip` |radius - radius_clip|, `image` to the four off-screen comparisons."""
    det = {}
    with torch.no_grad():
        R.projection(raw["xyz"].double(), raw["rotation"].double(), torch.exp(raw["scaling"].double()), cam["viewmat"].double()[None],
                     cam["K"].double()[None], cam["width"], cam["height"], details=det, **cull)
    inf = torch.full_like(det["z"][0], float("inf"))
    z, rr, r, mx, my = (det[k][0] for k in ("z", "radius_real", "radius", "mu_x", "mu_y"))
    reached = det["ok_z"][0] & det["ok_det"][0]
    depth = torch.minimum((z - cull["near_plane"]).abs(), (z - cull["far_plane"]).abs())
    ceil_ = torch.where(reached, (rr - torch.round(rr)).abs(), inf)
    clip = torch.where(reached, (r - cull["radius_clip"]).abs(), inf)
    img = torch.stack([(mx + r).abs(), (mx - r - cam["width"]).abs(), (my + r).abs(), (my - r - cam["height"]).abs()]).amin(0)
    image = torch.where(reached & det["ok_r"][0], img, inf)
    return dict(ceil=ceil_, depth=depth, clip=clip, image=image)


def violations(raw, cam):
    """bool[N]: rows within MARGIN of a decision under any of the CULLS."""
    bad = torch.zeros(raw["xyz"].shape[0], dtype=torch.bool)
    for cull in CULLS.values():
        for v in margins(raw, cam, cull).values():
            bad |= v < MARGIN
    return bad


def _move(raw, cam, salt):
    """Rows that violate the margins are moved (never skipped): a deterministic shift of a few hundredths, again until
    none is left."""
    for it in range(20):
        bad = violations(raw, cam)
        if not bool(bad.any()):
            return it
        g = torch.Generator().manual_seed(1000 * salt + it)
        raw["xyz"][bad] += (torch.rand(int(bad.sum()), 3, generator=g) - 0.5) * 0.04
    raise AssertionError("rows within the margin remain")


@functools.lru_cache(maxsize=None)
def scene():
    """The 400-row, 64x48 scene of tests/test_gpu_pose.py::_scene (two rows clamped in tx, one row dark in every channel)
    as the front end's raw tables, plus: a row with exactly one channel below the clamp, one behind the camera, one beyond
    the finite far_plane of CULLS, one whose radius is below the radius_clip of CULLS, one wholly off screen.
    -> raw, cam (treat both as read-only)."""
    from tests.test_gpu_pose import _scene
    src, c, _ = _scene()
    xyz, scaling, shs = src["means"].clone(), src["log_scales"].clone(), src["shs"].clone()
    Rv, t = c["viewmat"][:3, :3], c["viewmat"][:3, 3]
    place = lambda x, y, z: Rv.T @ (torch.tensor([x, y, z]) - t)  # from camera space
    S = SPECIAL
    shs[S["one_channel"], 0] = torch.tensor([-6.0, 1.0, 1.0])  # 0.282 * -6 + 0.5 < 0 in the first channel alone
    shs[S["one_channel"], 1:] *= 0.1
    xyz[S["one_channel"]] = place(0.4, -0.3, 5.0)
    xyz[S["behind"]] = place(0.3, 0.2, -2.0)
    xyz[S["far"]] = place(0.5, 0.4, 12.0)
    xyz[S["tiny"]] = place(-0.6, 0.5, 6.0)
    scaling[S["tiny"]] = torch.log(torch.tensor([2e-3, 3e-3, 2e-3]))
    xyz[S["off_screen"]] = place(9.0, 0.5, 6.0)
    scaling[S["off_screen"]] = torch.log(torch.tensor([0.05, 0.05, 0.05]))
    n = xyz.shape[0]
    raw = dict(xyz=xyz.contiguous(), opacity=src["opacity_raw"].clone(), scaling=scaling.contiguous(),
               rotation=src["quats"].clone(), shs=shs.reshape(n, 48).contiguous())
    cam = dict(viewmat=c["viewmat"], K=c["K"], width=c["width"], height=c["height"])
    _move(raw, cam, 1)
    return raw, cam


@functools.lru_cache(maxsize=None)
def tiled_scene(n):
    """n unique rows: scene()'s rows over and over, each copy shifted by up to 0.05 units per axis and its other
    attributes by a few per cent (seeded), rows that come within the margins moved as in scene()."""
    raw0, cam = scene()
    n0 = raw0["xyz"].shape[0]
    idx = torch.arange(n) % n0
    g = torch.Generator().manual_seed(77)
    raw = {k: v[idx].clone() for k, v in raw0.items()}
    raw["xyz"] += (torch.rand(n, 3, generator=g) - 0.5) * 0.1
    raw["scaling"] += (torch.rand(n, 3, generator=g) - 0.5) * 0.05
    raw["opacity"] += (torch.rand(n, generator=g) - 0.5) * 0.2
    raw["shs"][:, 3:] += (torch.rand(n, 45, generator=g) - 0.5) * 0.02
    _move(raw, cam, 2)
    return raw, cam


def scene_conditions(raw, cam):
    """What the kernel tests rely on, asserted (the CPU test calls this; the GPU tests rely on it): no row within the
    margins, and every special row in the state its name says, under the default culls and under the one meant for it."""
    assert not bool(violations(raw, cam).any())
    S, n0 = SPECIAL, 400
    out = {name: reference(raw, None, cam, 3, False, **cull) for name, cull in CULLS.items()}
    det = {}
    reference(raw, None, cam, 3, False, details=det)
    r = out["default"]["radii"]
    xr, (lim_neg, lim_pos) = det["tx_over_z"][0], det["lim_x"]
    for k in range(raw["xyz"].shape[0] // n0):  # every copy of a tiled scene
        o = k * n0
        a, b = S["clamped_tx"]
        assert r[o + a] > 0 and r[o + b] > 0 and float(xr[o + a]) > float(lim_pos) and float(xr[o + b]) < -float(lim_neg)
        with torch.no_grad():
            dirs = raw["xyz"].double()[[o + S["dark"], o + S["one_channel"]]] - campos_of(cam["viewmat"])
            pre = O.spherical_harmonics(3, dirs[None], raw["shs"].double()[[o + S["dark"], o + S["one_channel"]]].reshape(1, 2, 16, 3))[0] + 0.5
        assert r[o + S["dark"]] > 0 and bool((pre[0] < -1e-3).all())
        assert r[o + S["one_channel"]] > 0 and float(pre[1, 0]) < -1e-3 and float(pre[1, 1:].min()) > 1e-3
        assert r[o + S["behind"]] == 0 and float(det["z"][0, o + S["behind"]]) < 0
        assert r[o + S["far"]] > 0 and out["far"]["radii"][o + S["far"]] == 0 and out["near"]["radii"][o + S["far"]] > 0
        assert r[o + S["tiny"]] > 0 and out["clip"]["radii"][o + S["tiny"]] == 0
        assert r[o + S["off_screen"]] == 0 and bool(det["ok_z"][0, o + S["off_screen"]]) and not bool(det["ok_img"][0, o + S["off_screen"]])
    for name in ("near", "far", "clip"):  # rows on both sides of each threshold
        flipped = (out[name]["radii"] > 0) != (r > 0)
        assert int(flipped.sum()) >= 10 and int((out[name]["radii"] > 0).sum()) >= 10, name
    return out
