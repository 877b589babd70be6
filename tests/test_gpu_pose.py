"""-m gpu: the camera-pose gradient kernels (csrc/pose.hip) against the float64 reference of tests/pose_reference.py,
against clmgs_preprocess_bwd, from run to run, through fused.train_one_camera, as the operator's viewmats gradient,
and end to end: pose-only training against the reference trajectory.

Tolerance of the kernel tests: a camera's sums cancel between rows, so the bound is taken from the same sums evaluated
by the reference in float32 on the CPU: component by component four times |reference32 - reference64| (four: the
kernel's summation order differs from torch's), with a floor of GRAD_TOL (tests/test_gpu_ops.py, 2e-4) times the
largest entry of the component's group (v_R | v_t | v_campos).
Measured deviations are printed by every test; the recorded figures are in the note at TOLERANCES below."""
import ctypes
import functools
import json
import math
import os

import numpy as np
import pytest
import torch

from oracle import gs_oracle as O
from tests import antialias_reference as AR
from tests import pose_reference as R
from tests.scenes import small_scene
from tests.test_gpu_ops import GRAD_TOL

pytestmark = pytest.mark.gpu

F64, F32 = torch.float64, torch.float32
W0, H0, N0 = 64, 48, 400
GROUPS = ((0, 9), (9, 12), (12, 15))


def _npp(a):
    return a.ctypes.data_as(ctypes.c_void_p)


@functools.lru_cache(maxsize=None)
def _scene():
    """scenes.small_scene(n=400, 64x48) as raw rows, with the special rows the issue asks for: two rows far off axis and
    large, so that they stay on screen with tx clamped; one row whose colour falls below the clamp in every channel."""
    s = small_scene(n=N0, width=W0, height=H0, seed=0)
    means, scales, shs = s["means"].clone(), s["scales"].clone(), s["shs"].clone()
    Rv, t = s["viewmat"][:3, :3], s["viewmat"][:3, 3]
    for row, (xc, yc) in ((7, (5.6, 0.3)), (11, (-5.4, -0.2))):  # camera-space x / z = +-0.9 > the limit 0.72
        means[row] = Rv.T @ (torch.tensor([xc, yc, 6.0]) - t)
        scales[row] = torch.tensor([1.2, 0.9, 1.0])
    shs[13, 0] = -6.0  # 0.282 * -6 + 0.5 < 0 in the three channels
    raw = dict(means=means.contiguous(), quats=s["quats"].contiguous(), log_scales=torch.log(scales).contiguous(),
               opacity_raw=torch.logit(s["opac"].reshape(N0)).contiguous(), shs=shs.contiguous())
    cam = dict(viewmat=s["viewmat"].contiguous(), K=s["K"].contiguous(), width=W0, height=H0,
               campos=torch.inverse(s["viewmat"].double())[:3, 3].float())
    radii = R.oracle_radii(dict(raw), cam)
    lim = (W0 - 32.0) / 57.6 + 0.3 * 0.5 * W0 / 57.6
    pc = means @ Rv.T + t
    assert int(radii[7]) > 0 and int(radii[11]) > 0 and radii[13] > 0
    assert float(pc[7, 0] / pc[7, 2]) > lim and float(pc[11, 0] / pc[11, 2]) < -lim  # clamped in tx, both sides
    return raw, cam, radii


def _rows(filt, radii_all, force_dead=()):
    """The reference's view of the launch: rows of the filter, the launch's radii (some forced to 0)."""
    raw, _, _ = _scene()
    idx = filt if filt is not None else torch.arange(N0)
    rows = {k: v[idx] for k, v in raw.items()}
    radii = radii_all[idx].clone()
    for i in force_dead:
        radii[i] = 0
    rows["radii"] = radii
    return rows


def _tolerance(ref64, ref32):
    tol = torch.empty(15, dtype=F64)
    for a, b in GROUPS:
        floor = GRAD_TOL * float(ref64[a:b].abs().max())
        tol[a:b] = torch.clamp(4.0 * (ref32[a:b].double() - ref64[a:b]).abs(), min=floor)
    return tol


def _reference15(rows, cam, lines):
    out = []
    for dt in (F64, F32):
        vv, vc = R.pose_sums_reference(rows, cam, lines, dtype=dt)
        out.append(torch.cat((vv[:, :3].reshape(9), vv[:, 3], vc)))
    return out[0], out[1], _tolerance(out[0], out[1].double())


def _launch(dev, rows, cam, deg, pk=False, aa=False, lines=None, partials=None, row_cum=None, filt=None, table=None,
            sh_mode="by_row", repeat=1):
    """clmgs_pose_grad + clmgs_pose_grad_finish -> the 15 floats (CPU), added into zeros; `repeat` launches return a list.
    `table`: the raw rows the filter indexes (default: `rows` itself, identity)."""
    from clm_gs_amd import _lib
    from clm_gs_amd._lib import check, dptr, stream
    L = _lib.lib()
    src = table if table is not None else rows
    n = src["means"].shape[0]
    V = rows["radii"].shape[0]
    d = {k: src[k].to(dev).contiguous() for k in ("means", "quats", "log_scales", "opacity_raw")}
    if pk:
        tab = torch.zeros(n, 12, device=dev)
        tab[:, 0:3], tab[:, 3], tab[:, 4:7], tab[:, 7:11] = d["means"], d["opacity_raw"], d["log_scales"], d["quats"]
        small = (dptr(tab), None, None, None)
    else:
        small = (dptr(d["means"]), dptr(d["opacity_raw"]), dptr(d["log_scales"]), dptr(d["quats"]))
    fd = filt.to(dev) if filt is not None else None
    sh_index, by_filter = None, 1
    if sh_mode == "by_row":        # [n,48], indexed by row id
        sh = src["shs"].reshape(n, 48).to(dev).contiguous()
    elif sh_mode == "by_position":  # [V,48], indexed by position
        sh, by_filter = rows["shs"].reshape(V, 48).to(dev).contiguous(), 0
    else:                           # a shuffled staging table + its index
        g = torch.Generator().manual_seed(V)
        perm = torch.randperm(V, generator=g)
        stage = torch.empty(V + 3, 48)
        stage[perm] = rows["shs"].reshape(V, 48)
        stage[V:] = float("nan")
        sh, sh_index = stage.to(dev).contiguous(), perm.to(torch.int32).to(dev)
    if deg == 0 and sh_mode == "by_row":
        sh = None  # not read at all at degree 0
    vmh = np.ascontiguousarray(cam["viewmat"].numpy().astype(np.float32).reshape(16))
    Kh = np.ascontiguousarray(cam["K"].numpy().astype(np.float32).reshape(9))
    cph = np.ascontiguousarray(cam["campos"].numpy().astype(np.float32).reshape(3))
    radii = rows["radii"].to(torch.int32).to(dev)
    pgd = prd = rcd = None
    if lines is not None:
        pg = torch.zeros(V, 16)
        pg[:, :9] = lines
        pg[:, 9:] = 7.0  # words the kernel must not read
        pgd = pg.to(dev)
    else:
        prd, rcd = partials.to(dev).contiguous(), row_cum.to(dev)
    n_rows = int(L.clmgs_pose_grad_partials_rows(V))
    outs = []
    for _ in range(repeat):
        part = torch.full((max(n_rows, 1), 16), float("nan"), device=dev)
        grad = torch.zeros(16, device=dev)
        check(L.clmgs_pose_grad(stream(), V, dptr(fd, torch.int64, True), *small, dptr(sh, F32, True), by_filter, _npp(vmh),
                                _npp(Kh), _npp(cph), W0, H0, deg, 0.3, dptr(radii), dptr(pgd, F32, True),
                                dptr(prd, F32, True), dptr(rcd, torch.int64, True), dptr(sh_index, torch.int32, True),
                                int(aa), dptr(part)))
        check(L.clmgs_pose_grad_finish(stream(), n_rows, dptr(part), dptr(grad)))
        torch.cuda.synchronize()
        assert n_rows == 0 or bool(torch.isfinite(part[:n_rows]).all()), "every partial row is written"
        assert n_rows == 0 or float(part[:n_rows, 15].abs().max()) == 0.0
        assert float(grad[15]) == 0.0
        outs.append(grad[:15].cpu().clone())
    return outs[0] if repeat == 1 else outs


def _check(got, ref64, tol, what):
    err = (got.double() - ref64).abs()
    worst = float((err / tol.clamp_min(1e-300)).max()) if bool((tol > 0).any()) else 0.0
    rel = [float(err[a:b].max() / max(float(ref64[a:b].abs().max()), 1e-300)) for a, b in GROUPS]
    print(f"{what}: |kernel - ref64| / tol worst {worst:.3g}; relative to the group's largest entry "
          f"v_R {rel[0]:.3g} v_t {rel[1]:.3g} v_campos {rel[2]:.3g}")
    assert bool((err <= tol).all()), (what, err, tol)


def _lines(V, seed):
    return torch.randn(V, 9, generator=torch.Generator().manual_seed(seed))


# TOLERANCES, measured on an MI355X (this file with -s).  The float32 reference deviates from the float64 one by 0 .. 1.2e-7
# of its group's largest entry, so the floor (2e-4 of that entry) is what binds everywhere.  The kernel's own deviation,
# relative to the group's largest entry: v_R 5e-8 .. 2.3e-7, v_t 3e-8 .. 5.7e-7, v_campos 6e-8 .. 1.5e-6 over all cases
# of 1 .. 400 rows (worst |kernel - ref64| / tol 0.0074, at V = 63); 1.2e-6 / 5e-7 at V = 196 678 (0.006 of the bound).
# Operator form: worst |err| / tol 0.0023.


@pytest.mark.parametrize("deg", [0, 1, 2, 3])
def test_kernel_against_the_reference(dev, deg):
    """Degrees 0-3 x {four arrays, packed table} x {no filter, shuffled filter} x {plain, antialiased} on the [V,16]
    table; the three SH addressings; some rows with radius 0 (the oracle's own culls and two forced ones)."""
    raw, cam0, radii = _scene()
    for filt_on in (False, True):
        filt = torch.randperm(N0, generator=torch.Generator().manual_seed(3))[:333] if filt_on else None
        rows = _rows(filt, radii, force_dead=(5, 40))
        assert bool((rows["radii"] > 0).any()) and not bool((rows["radii"] > 0).all())
        V = rows["radii"].shape[0]
        lines = _lines(V, 10 + deg)
        for aa in (False, True):
            cam = dict(cam0, degree=deg, antialiased=aa)
            ref64, ref32, tol = _reference15(rows, cam, lines)
            assert deg == 0 or float(ref64[12:].abs().max()) > 0
            for pk in (False, True):
                got = _launch(dev, rows, cam, deg, pk=pk, aa=aa, lines=lines, filt=filt, table=raw)
                _check(got, ref64, tol, f"deg={deg} filter={filt_on} aa={aa} packed={pk}")
                if deg == 0:
                    assert float(got[12:].abs().max()) == 0.0  # no direction dependence: exactly zero
            if filt_on:  # SH rows by position, and through a staging index: the same bits as by row id
                base = _launch(dev, rows, cam, deg, aa=aa, lines=lines, filt=filt, table=raw)
                for mode in ("by_position", "staged"):
                    other = _launch(dev, rows, cam, deg, aa=aa, lines=lines, filt=filt, table=raw, sh_mode=mode)
                    assert torch.equal(other, base), (deg, aa, mode)


def test_clamped_rows_and_clamped_colours_are_in_the_sums(dev):
    """The special rows alone (tx clamped on both sides; every colour channel below the clamp) against the reference: the
    clamped branch of the projection VJP and the clamp mask of the SH VJP are what is measured."""
    raw, cam0, radii = _scene()
    cam = dict(cam0, degree=3, antialiased=False)
    filt = torch.tensor([7, 11, 13])
    rows = _rows(filt, radii)
    with torch.no_grad():
        col = O.spherical_harmonics(3, (rows["means"].double() - cam["campos"].double())[None], rows["shs"].double()[None])[0] + 0.5
    assert bool((col[2] < 0).all()) and bool((col[:2] > 0).any())
    lines = _lines(3, 5)
    ref64, ref32, tol = _reference15(rows, cam, lines)
    _check(_launch(dev, rows, cam, 3, lines=lines, filt=filt, table=raw), ref64, tol, "special rows")
    only = _rows(torch.tensor([13]), radii)
    r64, _, _ = _reference15(only, cam, lines[2:3])
    assert float(r64[12:].abs().max()) == 0.0  # below the clamp: no colour gradient reaches the camera centre
    got = _launch(dev, only, cam, 3, lines=lines[2:3], filt=torch.tensor([13]), table=raw)
    assert float(got[12:].abs().max()) == 0.0


@pytest.mark.parametrize("V", [1, 63, 64, 65])
def test_chunk_boundaries(dev, V):
    raw, cam0, radii = _scene()
    cam = dict(cam0, degree=3, antialiased=False)
    vis = torch.nonzero(radii > 0).flatten()
    g = torch.Generator().manual_seed(V)
    filt = vis[torch.randperm(vis.numel(), generator=g)[:V]] if V == 1 else torch.randperm(N0, generator=g)[:V]
    rows = _rows(filt, radii)
    lines = _lines(V, V)
    ref64, _, tol = _reference15(rows, cam, lines)
    for pk in (False, True):
        _check(_launch(dev, rows, cam, 3, pk=pk, lines=lines, filt=filt, table=raw), ref64, tol, f"V={V} packed={pk}")


def test_no_visible_row_gives_exact_zeros(dev):
    raw, cam0, radii = _scene()
    rows = _rows(None, torch.zeros_like(radii))
    for deg in (0, 3):
        got = _launch(dev, rows, dict(cam0, degree=deg), deg, lines=_lines(N0, 1), pk=True)
        assert float(got.abs().max()) == 0.0


def _partial_case(V, seed):
    """Row ranges of 0, 1, 4, 5 and 9 lines, in turn; the row's line is their float32 sum in ascending order from zero."""
    counts = torch.tensor([0, 1, 4, 5, 9])[torch.arange(V) % 5]
    row_cum = torch.cumsum(counts, 0).to(torch.int64)
    T = int(row_cum[-1])
    g = torch.Generator().manual_seed(seed)
    part = torch.zeros(max(T, 1), 16)
    part[:, :9] = torch.randn(max(T, 1), 9, generator=g)
    part[:, 9:] = 3.0  # not read
    lines = torch.zeros(V, 9)
    start = 0
    for i in range(V):
        acc = torch.zeros(9)
        for l in range(start, int(row_cum[i])):
            acc = acc + part[l, :9]  # float32, ascending
        lines[i], start = acc, int(row_cum[i])
    return part, row_cum, lines


@pytest.mark.parametrize("aa", [False, True])
def test_partial_lines_are_summed_as_the_row_backward_sums_them(dev, aa):
    """Partial lines + row_cum (ranges of 0, 1, 4, 5, 9 lines) give the bits of the [V,16] table that holds the ascending
    float32 sums, and meet the reference."""
    raw, cam0, radii = _scene()
    cam = dict(cam0, degree=3, antialiased=aa)
    filt = torch.randperm(N0, generator=torch.Generator().manual_seed(8))[:131]
    rows = _rows(filt, radii)
    part, row_cum, lines = _partial_case(131, 2)
    ref64, _, tol = _reference15(rows, cam, lines)
    for pk in (False, True):
        a = _launch(dev, rows, cam, 3, pk=pk, aa=aa, partials=part, row_cum=row_cum, filt=filt, table=raw)
        b = _launch(dev, rows, cam, 3, pk=pk, aa=aa, lines=lines, filt=filt, table=raw)
        assert torch.equal(a, b), (pk, a, b)
        _check(a, ref64, tol, f"partial lines aa={aa} packed={pk}")


def test_a_wave_runs_a_second_chunk(dev):
    """V above 64 x clmgs_pose_grad_partials_rows(V): the grid is capped, waves take a second chunk.  Degree 0 (the
    reference needs the projection only); the filter repeats the scene's rows."""
    from clm_gs_amd import _lib
    raw, cam0, radii = _scene()
    cap = int(_lib.lib().clmgs_pose_grad_partials_rows(10 ** 9))
    V = 64 * cap + 70
    assert V <= 300_000 and int(_lib.lib().clmgs_pose_grad_partials_rows(V)) == cap
    filt = torch.randint(0, N0, (V,), generator=torch.Generator().manual_seed(4))
    rows = _rows(filt, radii)
    lines = _lines(V, 6)
    cam = dict(cam0, degree=0, antialiased=False)
    ref64, _, tol = _reference15(rows, cam, lines)
    got = _launch(dev, rows, cam, 0, pk=True, lines=lines, filt=filt, table=raw)
    _check(got, ref64, tol, f"V={V}")
    # the rows of the second chunks alone are in it: without them the sums differ
    head = {k: v[:64 * cap] for k, v in rows.items()}
    r_head, _, _ = _reference15(head, cam, lines[:64 * cap])
    assert float((r_head - ref64).abs().max()) > 10 * float(tol.max())


def test_two_launches_give_the_same_bits(dev):
    raw, cam0, radii = _scene()
    filt = torch.randperm(N0, generator=torch.Generator().manual_seed(3))[:333]
    rows = _rows(filt, radii)
    part, row_cum, _ = _partial_case(333, 9)
    a, b = _launch(dev, rows, dict(cam0, degree=3), 3, pk=True, partials=part, row_cum=row_cum, filt=filt, table=raw, repeat=2)
    assert torch.equal(a, b) and float(a.abs().max()) > 0


@pytest.mark.parametrize("aa", [False, True])
def test_cross_check_against_the_row_backward(dev, aa):
    """Without the reference: sum over rows of clmgs_preprocess_bwd's g_xyz (into zeroed tables) is
    Rv^T v_t - v_campos, to the tolerance of the kernel test."""
    from clm_gs_amd import _lib
    from clm_gs_amd._lib import check, dptr, stream
    L = _lib.lib()
    raw, cam0, radii = _scene()
    cam = dict(cam0, degree=3, antialiased=aa)
    rows = _rows(None, radii)
    lines = _lines(N0, 12)
    got = _launch(dev, rows, cam, 3, aa=aa, lines=lines).double()
    ref64, _, tol = _reference15(rows, cam, lines)
    d = {k: raw[k].to(dev).contiguous() for k in raw}
    gs = [torch.zeros(N0, 3, device=dev), torch.zeros(N0, device=dev), torch.zeros(N0, 3, device=dev), torch.zeros(N0, 4, device=dev)]
    gsh = torch.zeros(N0, 48, device=dev)
    pg = torch.zeros(N0, 16)
    pg[:, :9] = lines
    pgd = pg.to(dev)
    vmh = np.ascontiguousarray(cam["viewmat"].numpy().astype(np.float32).reshape(16))
    Kh = np.ascontiguousarray(cam["K"].numpy().astype(np.float32).reshape(9))
    cph = np.ascontiguousarray(cam["campos"].numpy().astype(np.float32).reshape(3))
    rd = radii.to(torch.int32).to(dev)
    bwd = L.clmgs_preprocess_aa_bwd if aa else L.clmgs_preprocess_bwd
    check(bwd(stream(), N0, None, dptr(d["means"]), dptr(d["opacity_raw"]), dptr(d["log_scales"]), dptr(d["quats"]),
              dptr(d["shs"].reshape(N0, 48).contiguous()), 1, _npp(vmh), _npp(Kh), _npp(cph), W0, H0, 3, 0.3, dptr(rd),
              dptr(pgd), *(dptr(x) for x in gs), dptr(gsh), None, None, None, None, 0, None, None, None, None, 0))
    torch.cuda.synchronize()
    sum_xyz = gs[0].double().sum(0).cpu()
    Rv = cam["viewmat"][:3, :3].double()
    want = Rv.T @ got[9:12] - got[12:15]
    # the bound: the tolerance of v_t carried through Rv^T (|Rv| <= 1 entrywise: the three add up) plus v_campos's, and as
    # much again for the row kernel's own float32 sum of N0 terms
    bound = 2.0 * (float(tol[9:12].sum()) + tol[12:15])
    print("sum g_xyz", sum_xyz.tolist(), "Rv^T v_t - v_campos", want.tolist(), "bound", bound.tolist())
    assert bool(((sum_xyz - want).abs() <= bound).all())
    assert float(want.abs().max()) > 100 * float(bound.max())  # and it is a real signal


# ------------------------------------------------------------------------------------------------ operator
@pytest.mark.parametrize("C", [1, 3])
@pytest.mark.parametrize("comp", [False, True])
def test_projection_operator_returns_the_viewmats_gradient(dev, C, comp):
    """gsplat.fully_fused_projection(viewmats.requires_grad_()) against autograd of the float64 projection, v_depths
    included; without requires_grad on the view matrices: no gradient, and the other gradients' bits unchanged."""
    from clm_gs_amd import gsplat as G
    s = small_scene(n=N0, width=W0, height=H0, seed=2)
    vms = R.eight_cameras(s["viewmat"], n=C) if C > 1 else s["viewmat"][None].clone()
    Ks = s["K"][None].repeat(C, 1, 1)
    g = torch.Generator().manual_seed(C)
    cot = [torch.randn(C, N0, k, generator=g) for k in (2, 1, 3, 1)]  # means2d, depths, conics, compensations

    def run(dtype, device, with_vm_grad, proj):
        leaves = [s[k].to(dtype).to(device).clone().requires_grad_() for k in ("means", "quats", "scales")]
        vm = vms.to(dtype).to(device).clone().requires_grad_(with_vm_grad)
        out = proj(leaves, vm, Ks.to(dtype).to(device))
        c = [x.to(dtype).to(device) for x in cot]
        sc = (out[1] * c[0]).sum() + (out[2] * c[1][..., 0]).sum() + (out[3] * c[2]).sum()
        if comp:
            sc = sc + (out[4] * c[3][..., 0]).sum()
        sc.backward()
        return out[0], [x.grad for x in leaves], vm.grad

    prod = lambda lv, vm, K: G.fully_fused_projection(lv[0], None, lv[1], lv[2], vm, K, W0, H0, calc_compensations=comp)
    refp = (lambda lv, vm, K: AR.projection(lv[0], lv[1], lv[2], vm, K, W0, H0)) if comp else \
        (lambda lv, vm, K: O.fully_fused_projection(lv[0], None, lv[1], lv[2], vm, K, W0, H0))
    radii, grads, vg = run(F32, dev, True, prod)
    radii0, grads0, vg0 = run(F32, dev, False, prod)
    assert vg0 is None and torch.equal(radii, radii0)
    for a, b in zip(grads, grads0):
        assert torch.equal(a, b)
    r64, _, v64 = run(F64, "cpu", True, refp)
    r32, _, v32 = run(F32, "cpu", True, refp)
    assert torch.equal(radii.cpu(), r64), "the float32 and float64 culls agree on this scene"
    assert tuple(vg.shape) == (C, 4, 4) and float(vg[:, 3].abs().max()) == 0.0
    for c in range(C):
        for name, sl in (("v_R", (slice(0, 3), slice(0, 3))), ("v_t", (slice(0, 3), slice(3, 4)))):
            ref = v64[c][sl]
            tol = torch.clamp(4.0 * (v32[c][sl].double() - ref).abs(), min=GRAD_TOL * float(ref.abs().max()))
            err = (vg[c][sl].cpu().double() - ref).abs()
            print(f"C={C} comp={comp} camera {c} {name}: worst |err| / tol {float((err / tol).max()):.3g}")
            assert bool((err <= tol).all()), (c, name, err, tol)


# ------------------------------------------------------------------------------------ isolation in the engines
def _engine_batch(strategy, with_pose):
    """One batch of tests/test_gpu_engines.py's scene, the optimizer left out, with or without pose buffers on the cameras
    -> everything the batch leaves behind, on the CPU, and the pose gradient table."""
    from clm_gs_amd.pose import PoseModel
    from tests import test_gpu_engines as GE
    args, sc, cams = GE._setup(strategy)
    args.debug_skip_optimizer = True
    model = None
    if with_pose:
        model = PoseModel(len(cams), defer=False)
        model.attach(cams)  # a zero table: the cameras stay as loaded
    m = GE._make(strategy, sc, args)
    if strategy == "no_offload":
        from clm_gs_amd.strategies.no_offload import baseline_accumGrads_impl
        losses, _ = baseline_accumGrads_impl(m, GE._Scene, cams, None)
        order = list(range(GE.BSZ))
        left = [m._xyz.grad, m._opacity.grad, m._scaling.grad, m._rotation.grad, m._features_dc.grad, m._features_rest.grad,
                m.max_radii2D, m.xyz_gradient_accum, m.denom]
    else:
        from clm_gs_amd.strategies.clm_offload import clm_offload_train_one_batch
        comm, gen = torch.cuda.Stream(), torch.Generator(device="cuda").manual_seed(1)
        losses, order, _ = clm_offload_train_one_batch(m, GE._Scene, cams, m.parameters_grad_buffer, None, None, comm, gen)
        torch.cuda.synchronize()
        left = [m.small_grad(), m.parameters_grad_buffer[:GE.N], m.max_radii2D, m.xyz_gradient_accum, m.denom]
    torch.cuda.synchronize()
    lo = [0.0] * GE.BSZ
    for k, l in zip(order, losses):
        lo[k] = l.item()
    return lo, [t.detach().cpu().clone() for t in left], (model.grad.cpu().clone() if model is not None else None)


@pytest.mark.parametrize("strategy", ["no_offload", "clm_offload"])
def test_a_pose_buffer_changes_nothing_else(dev, strategy):
    """Cameras run through fused.train_one_camera / the camera pipeline with and without a pose buffer leave bit-identical
    losses, gradients, statistics and SH gradient rows; the buffers themselves are filled, and run to run identical."""
    l0, t0, _ = _engine_batch(strategy, False)
    l1, t1, g1 = _engine_batch(strategy, True)
    _, _, g2 = _engine_batch(strategy, True)
    assert l0 == l1
    for a, b in zip(t0, t1):
        assert torch.equal(a, b)
    assert bool((g1[:, :12].abs().amax(dim=1) > 0).all()) and bool((g1[:, 12:15].abs().amax(dim=1) > 0).all())
    assert float(g1[:, 15].abs().max()) == 0.0 and torch.equal(g1, g2)


# ------------------------------------------------------------------------------------------------ end to end
E2E_K, E2E_BSZ, E2E_CAMS = 30, 4, 8  # (clm_offload takes batches of 4 and up)
# Chosen on the CPU (the reference trajectory with ground truth rendered by the oracle, seeds 0-5 of the noise, learning
# rates 2e-4 and 2e-5): at noise 0.03 (seed 4) and pose_opt_lr 2e-5 the table moves by at most K * lr = 6e-4 per entry,
# two orders below the noise, so no gradient component changes sign within the K steps, and the smallest
# |g_k| / max_k |g_k| over the 120 row gradients is 8.4e-4 (8.8e-4 with the engine's ground truth; the structurally small
# components are those of the 6-D rotation along its own two vectors); with 2e-4 several components cross zero (smallest
# ratio 3e-4 .. 2e-6 over the seeds).  The mean translation error of the reference falls from 0.035552 to 0.035414.
# max_steps = 3000: the schedule is nearly flat over the K steps.
E2E_NOISE, E2E_SEED, E2E_LR, E2E_REG, E2E_MAX_STEPS = 0.03, 4, 2e-5, 1e-6, 3000
E2E_BATCHES = [[(E2E_BSZ * k + j) % E2E_CAMS for j in range(E2E_BSZ)] for k in range(E2E_K)]
# max |table32 - table64| after K steps of the SAME reference trajectory run in float32 on the CPU, with the ground truth
# the engine renders (measured once on an MI355X box, see the docstring of the test); the bound is four times this
E2E_F32_DEVIATION = 1.392904e-08


def _e2e_args(strategy):
    from clm_gs_amd import utils
    args = utils.default_args(bsz=E2E_BSZ, position_lr_init=0.0, position_lr_final=0.0, feature_lr=0.0, opacity_lr=0.0,
                              scaling_lr=0.0, rotation_lr=0.0, disable_auto_densification=True, pose_opt=True,
                              pose_opt_lr=E2E_LR, pose_opt_reg=E2E_REG, pose_noise=E2E_NOISE, defer_pose_step=False)
    setattr(args, strategy, True)
    utils.set_args(args)
    utils.set_img_size(H0, W0)
    utils.set_cur_iter(1)
    return args


def _e2e_model(strategy, args):
    s = small_scene(n=N0, width=W0, height=H0, seed=0)
    if strategy == "no_offload":
        from clm_gs_amd.strategies.no_offload import GaussianModelNoOffload as M
    else:
        from clm_gs_amd.strategies.clm_offload import GaussianModelCLMOffload as M
    m = M(3)
    raw = dict(xyz=s["means"].cuda(), shs48=s["shs"].reshape(N0, 48).cuda(), scaling=torch.log(s["scales"]).cuda(),
               rotation=s["quats"].cuda(), opacity=torch.logit(s["opac"]).reshape(N0, 1).cuda())
    m.create_from_tensors(raw["xyz"].clone(), raw["shs48"].clone(), raw["scaling"].clone(), raw["rotation"].clone(),
                          raw["opacity"].clone(), spatial_lr_scale=1.0)
    m.active_sh_degree = 3
    m.training_setup(args)
    # what the reference renders: the activations of the float32 parameters the engine holds, in float64
    ref_scene = dict(means=raw["xyz"].cpu().double(), opac=torch.sigmoid(raw["opacity"].cpu().double()),
                     scales=torch.exp(raw["scaling"].cpu().double()), quats=raw["rotation"].cpu().double(),
                     shs=raw["shs48"].cpu().double().reshape(N0, 16, 3))
    return m, ref_scene, s


def _e2e_cameras(s, gts=None):
    from clm_gs_amd.cameras import Camera
    f = 0.9 * W0
    vms = R.eight_cameras(s["viewmat"], n=E2E_CAMS)
    return [Camera(i, vms[i], 2 * math.atan(W0 / (2 * f)), 2 * math.atan(H0 / (2 * f)), W0, H0,
                   image_u8=None if gts is None else gts[i], device="cuda") for i in range(E2E_CAMS)]


@functools.lru_cache(maxsize=None)
def _e2e_ground_truth():
    """The eight images, rendered by the project's own engine (the fused front end, exact lists) at the TRUE poses."""
    from clm_gs_amd import fused
    args = _e2e_args("no_offload")
    m, _, s = _e2e_model("no_offload", args)
    shs = m.get_features.reshape(N0, 48).contiguous().detach()
    blank = torch.zeros(3, H0, W0, dtype=torch.uint8, device="cuda")
    gts = []
    for cam in _e2e_cameras(s):
        p = fused.camera_forward(m, cam, None, shs, 1, None, blank, exact=True)
        torch.cuda.synchronize()
        gts.append((p.out.clamp(0, 1) * 255).round().to(torch.uint8).permute(2, 0, 1).contiguous().cpu())
    return tuple(gts)


@functools.lru_cache(maxsize=None)
def _e2e_reference(dtype=F64):
    """The reference trajectory (oracle render, reference loss, reference optimiser), computed once for both engines."""
    from clm_gs_amd.pose import PoseModel
    gts = _e2e_ground_truth()
    args = _e2e_args("no_offload")
    _, ref_scene, s = _e2e_model("no_offload", args)
    cams = _e2e_cameras(s, gts)
    probe = PoseModel(E2E_CAMS, device=None)
    probe.attach(cams)
    c2w0 = probe.c2w0.clone()
    probe.perturb(E2E_NOISE, seed=E2E_SEED)
    tables, grads = R.trajectory(ref_scene, c2w0, cams[0].K.cpu().double(), W0, H0, probe.table.clone(), list(gts),
                                 E2E_BATCHES, E2E_LR, E2E_REG, E2E_MAX_STEPS, dtype=dtype)
    return c2w0, tables, grads


def _e2e_train(strategy):
    from clm_gs_amd import trainer, utils
    gts = _e2e_ground_truth()
    args = _e2e_args(strategy)
    m, _, s = _e2e_model(strategy, args)
    cams = _e2e_cameras(s, gts)
    pose = trainer.build_pose(cams, E2E_MAX_STEPS, "cuda", E2E_LR, E2E_REG, E2E_NOISE, defer=False, seed=E2E_SEED)
    table0 = pose.table.clone()

    class Scene:
        cameras_extent = 5.0
    comm, gen = torch.cuda.Stream(), torch.Generator(device="cuda").manual_seed(1)
    for k, ids in enumerate(E2E_BATCHES):
        it = 1 + k * E2E_BSZ
        utils.set_cur_iter(it)
        m.update_learning_rate(it)
        batch = [cams[i] for i in ids]
        if strategy == "no_offload":
            from clm_gs_amd.strategies.no_offload import baseline_accumGrads_impl
            baseline_accumGrads_impl(m, Scene, batch, None)
            trainer.no_offload_optimizer_step(m, args, E2E_BSZ)
        else:
            from clm_gs_amd.strategies.clm_offload import clm_offload_train_one_batch
            clm_offload_train_one_batch(m, Scene, batch, m.parameters_grad_buffer, None, None, comm, gen)
        pose.step(batch)  # immediate
    torch.cuda.synchronize()
    assert pose.t == E2E_K
    return table0, pose.table.clone()


@pytest.mark.parametrize("strategy", ["no_offload", "clm_offload"])
def test_pose_only_training_follows_the_reference_trajectory(dev, strategy):
    """K = 30 immediate steps, pose_noise on, the model's learning rates at zero: the final [n,9] table against the float64
    reference trajectory, within four times the float32 reference's deviation from it; the mean translation error falls,
    as the reference's does.  Measured on an MI355X: float32 reference 1.39e-8 (mean 2.7e-9) while the reference moves by
    up to 4.3e-4; no_offload 4.5e-10, clm_offload 5.0e-10 (0.03x / 0.04x the float32 reference's deviation); mean
    translation error 0.03555194 -> 0.03541446 for the reference and for both engines."""
    c2w0, tables, _ = _e2e_reference()
    table0, table = _e2e_train(strategy)
    assert torch.equal(table0, tables[0])
    dev_max = float((table - tables[-1]).abs().max())
    moved = float((tables[-1] - tables[0]).abs().max())
    e0, ek, rk = (R.mean_translation_error(c2w0, t) for t in (tables[0], table, tables[-1]))
    print(f"{strategy}: max |table - reference| {dev_max:.3e} (the reference moved {moved:.3e}); mean translation error "
          f"{e0:.6f} -> {ek:.6f} (reference {rk:.6f}); float32 reference deviation {E2E_F32_DEVIATION}")
    assert rk < e0 and ek < e0
    assert dev_max <= 4.0 * E2E_F32_DEVIATION, (dev_max, E2E_F32_DEVIATION)


def test_trainer_writes_poses_json(dev, tmp_path):
    """A trainer run with pose_opt (deferred stepping, the default) writes a poses.json that load_json reads back; training
    cameras carry a buffer and move, test cameras stay as loaded."""
    from clm_gs_amd import trainer
    from clm_gs_amd.cameras import camera_pose_grad
    from clm_gs_amd.colmap_scene import load_colmap_scene
    from clm_gs_amd.pose import PoseModel
    from tests.test_gpu_exposure import _tiny_scene
    work = _tiny_scene(tmp_path)
    out = tmp_path / "out"
    loaded = load_colmap_scene(str(work), device="cuda", load_images=False, eval=True)
    _, scene, _ = trainer.train_from_colmap(str(work), str(out), strategy="clm_offload", iterations=8, test_iterations=(5,),
                                            bsz=4, eval=True, disable_auto_densification=True, pose_opt=True,
                                            pose_opt_lr=1e-4, pose_noise=0.01)
    assert scene.pose is not None and scene.pose.t == 2 and scene.pose._pending is None
    assert scene.test_cameras and all(camera_pose_grad(c) is None for c in scene.test_cameras)
    assert all(camera_pose_grad(c) is not None for c in scene.train_cameras)
    for a, b in zip(scene.test_cameras, loaded.test_cameras):
        assert torch.equal(a.world_view_transform, b.world_view_transform)
    table = json.load(open(out / "poses.json"))
    assert sorted(table) == sorted(c.image_name for c in scene.train_cameras)
    fresh = PoseModel(len(loaded.train_cameras), device=None)
    fresh.attach(loaded.train_cameras)
    fresh.load_json(str(out / "poses.json"), loaded.train_cameras)
    assert torch.equal(fresh.table, scene.pose.table) and float(fresh.table.abs().max()) > 0
    for a, b in zip(scene.train_cameras, loaded.train_cameras):
        assert torch.equal(a.world_view_transform.cpu(), b.world_view_transform.cpu())
        w2c = torch.tensor(table[a.image_name]["world_to_camera"], dtype=F64)
        assert torch.equal(w2c.float(), a.world_view_transform.t().cpu())
    log = open(out / "python_ws=1_rk=0.log").read()
    assert "Evaluating train:" in log and "Evaluating test:" in log and "end2end total_time:" in log
    assert float(scene.pose.grad.abs().max()) == 0.0  # every collected row was cleared
    # without the flag: no model, no file, no buffers
    out2 = tmp_path / "out2"
    _, scene2, _ = trainer.train_from_colmap(str(work), str(out2), strategy="clm_offload", iterations=8, bsz=4,
                                             disable_auto_densification=True)
    assert scene2.pose is None and not os.path.exists(out2 / "poses.json")
    assert all(camera_pose_grad(c) is None for c in scene2.train_cameras)
