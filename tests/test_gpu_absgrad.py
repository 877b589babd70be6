"""-m gpu: gsplat's absgrad (rasterize_to_pixels(absgrad=True) -> means2d.absgrad; AbsGS) through the tile kernels, the
front-end backward, the operator and the engines, against the float64 reference of tests/absgrad_reference.py.

absgrad[c, g] = sum over the pixels p at which g contributes of |dL_p/dmean2d|, componentwise.  The tile backward
never forms a per-pixel gradient of the mean (it reduces moments and forms the gradient once per entry), so the pair is
new arithmetic in the blend loop; on every multi-pixel case the reference is 4 to 19 times the norm of the signed
gradient (tests/test_absgrad_cpu.py), so |signed sum| cannot pass here.

Tolerances are those of tests/test_gpu_raster_edges.py, whose derivation bounds the relative error of ONE pixel's
contribution: GRAD_TOL = 2e-4 for plain / needle / non-positive-definite rows, translucent lists and the shape cases,
SAT_TOL = 1e-3 for rows special by opacity and every row of a saturating list.  An absolute sum has no smaller
denominator than the signed one (no cancellation), so they carry over unchanged.  Rows whose reference absgrad is
exactly zero (never valid, or clamped at every valid pixel) must be exactly zero here.
"""
import math

import pytest
import torch

from oracle import gs_oracle as O
from tests import scenes as S
from tests.absgrad_reference import absgrad_reference, case_absgrad
from tests.raster_edge_worker import slots_of
from tests.scenes import rel_l2

pytestmark = pytest.mark.gpu

GRAD_TOL = 2e-4
SAT_TOL = 1e-3
GRAD_NAMES = ("means2d", "conics", "colors", "opacities")


# ------------------------------------------------------------------------------------------- kernels, C ABI
def run_abs(case, dev, slot=True):
    """Both backward entries (clmgs_rasterize_bwd, clmgs_rasterize_abs_bwd) on one forward of the case, on both routes.
    -> dict on the CPU: `<route>_<entry>_<name>` for the four gradients, `<route>_abs_abs` = v_means2d_abs [C*N,2], and
    `slot_<entry>_line` = the row-summed [N,16] gradient lines of the slot route (C == 1)."""
    from clm_gs_amd import _lib
    from clm_gs_amd._lib import check, dptr, stream

    L = _lib.lib()
    C, N = case["op"].shape
    w, h = case["w"], case["h"]
    tw, th = math.ceil(w / 16), math.ceil(h / 16)
    I = case["fids"].numel()
    m2, cn, col, op = (case[k].to(dev).contiguous() for k in ("m2", "cn", "col", "op"))
    bg = case["bg"].to(dev).contiguous() if case["bg"] is not None else None
    off, fids = case["off"].to(dev).contiguous(), case["fids"].to(dev).contiguous()
    vi, va = case["vi"].to(dev).contiguous(), case["va"].to(dev).contiguous()
    out = torch.empty((C, h, w, 3), device=dev)
    al = torch.empty((C, h, w), device=dev)
    last = torch.empty((C, h, w), dtype=torch.int32, device=dev)
    packed = torch.empty(C * N, 16, device=dev)
    check(L.clmgs_rasterize_fwd(stream(), C, N, I, dptr(m2), dptr(cn), dptr(col), dptr(op), dptr(bg, None, True), w, h, 16,
                                tw, th, dptr(off), dptr(fids), dptr(packed), dptr(out), dptr(al), dptr(last)))
    nan = float("nan")
    res = {}

    def call(route, entry, tag=None):
        tag = tag or entry
        outs = [torch.full((C, N, 2), nan, device=dev), torch.full((C, N, 3), nan, device=dev),
                torch.full((C, N, 3), nan, device=dev), torch.full((C, N), nan, device=dev)]
        pg = torch.full((C * N, 16), nan, device=dev)
        v_abs = torch.full((C * N, 2), nan, device=dev)
        if route == "slot":
            slot_i, row_cum = slots_of(case["fids"], N)
            sd, rd = slot_i.to(dev), row_cum.to(dev)
            parts = torch.full((max(I, 1), L.clmgs_rasterize_partials_bytes(1) // 4), nan, device=dev)  # every line is written
            tail = (dptr(sd), dptr(rd), dptr(parts))
        else:
            tail = (None, None, None)
        fn = L.clmgs_rasterize_abs_bwd if entry == "abs" else L.clmgs_rasterize_bwd
        check(fn(stream(), C, N, I, dptr(packed), dptr(bg, None, True), w, h, 16, tw, th, dptr(off), dptr(fids), dptr(al),
                 dptr(last), dptr(vi), dptr(va), dptr(pg), *[dptr(x) for x in outs], *tail,
                 *((dptr(v_abs),) if entry == "abs" else ())))
        res.update({f"{route}_{tag}_{n}": x for n, x in zip(GRAD_NAMES, outs)})
        res[f"{route}_{tag}_line"] = pg
        if entry == "abs":
            res[f"{route}_{tag}_abs"] = v_abs

    for route in ("atomic", "slot") if slot else ("atomic",):
        call(route, "plain")
        call(route, "abs")
        call(route, "abs", "abs2")  # a second run: the slot route reproduces itself bit for bit
    torch.cuda.synchronize()
    return {k: v.cpu() for k, v in res.items()}


def check_abs(case, x, y, tols, what):
    """Per group of rows: relative L2 within the group's tolerance; exact zeros of the reference kept."""
    x, y = x.reshape(-1, 2), y.reshape(-1, 2)
    assert torch.isfinite(x).all(), what
    zero = (y == 0).all(dim=1)
    bad = torch.nonzero(zero & (x != 0).any(dim=1)).flatten().tolist()
    assert not bad, f"{what}: rows {bad[:8]} have a zero reference absgrad but a nonzero one here"
    worst = {}
    for gname, rows in case["groups"].items():
        if not bool((rows & ~zero).any()):
            continue  # an empty group, or one whose rows are all exact zeros (held above)
        assert float(y[rows].norm()) > 0, (what, gname)
        e = rel_l2(x[rows], y[rows])
        worst[gname] = e
        print(f"{what} group {gname}: rel_l2 {e:.3g} (bound {tols[gname]})")
        assert e < tols[gname], f"{what} group {gname}: rel_l2 {e:.3g} >= {tols[gname]}"
    assert worst or bool(zero.all()), what  # (a one-entry saturating list: its only row is clamped at every pixel)
    return worst


KERNEL_CASES = [("special", None)] + [(f"list{K}_{'sat' if sat else 'tr'}", (K, sat)) for K in (1, 64, 65, 129, 300)
                                      for sat in (False, True)] + [(n, n) for n in ("1x1", "17x17", "tiles7", "tiles9_C3")]


@pytest.mark.parametrize("name,spec", KERNEL_CASES, ids=[n for n, _ in KERNEL_CASES])
def test_abs_entries_match_float64_and_move_nothing_else(dev, name, spec):
    """Worst measured rel-L2 per group: see DESIGN.md section 3, "Absgrad"."""
    if spec is None:
        case = S.special_entry_case()
        tols = {"plain": GRAD_TOL, "needle": GRAD_TOL, "nonpd": GRAD_TOL, "opacity": SAT_TOL}
    elif isinstance(spec, tuple):
        case = S.list_case(spec[0], spec[1], "single")
        tols = {"walls": SAT_TOL, "translucent": SAT_TOL if spec[1] else GRAD_TOL}
    else:
        case = S.shape_case(spec)
        tols = {"all": GRAD_TOL}
    C, N = case["op"].shape
    slot = C == 1  # the slot route takes one camera
    ref_abs, ref_sum = case_absgrad(case)
    got = run_abs(case, dev, slot=slot)
    if name == "special":
        assert int((ref_abs == 0).all(dim=1).sum()) == 26
    if name == "list300_sat":
        assert int((ref_abs == 0).all(dim=1).sum()) == 108
    for route in ("atomic", "slot") if slot else ("atomic",):
        check_abs(case, got[f"{route}_abs_abs"], ref_abs, tols, f"{name} {route}")
        # the signed gradient of the abs entry is still the signed gradient
        assert rel_l2(got[f"{route}_abs_means2d"].reshape(-1, 2), ref_sum) < max(tols.values()), route
    # nothing else moves.  Atomic route: float atomics land in any order, so within GRAD_TOL of the plain entry
    for n in GRAD_NAMES:
        a, b = got[f"atomic_abs_{n}"], got[f"atomic_plain_{n}"]
        assert torch.isfinite(a).all() and (float(b.norm()) == 0 or rel_l2(a, b) < GRAD_TOL), n
    if slot:
        # slot route: every other word of the row-summed gradient line is the plain entry's bit for bit (words 0..9; the
        # fourth float4 is not written by either), the pair itself reproduces bit for bit, and it is what was unpacked
        la, lp, l2 = got["slot_abs_line"], got["slot_plain_line"], got["slot_abs2_line"]
        assert torch.equal(la[:, :10], lp[:, :10])
        assert float(lp[:, 9:12].abs().max()) == 0.0 and float(la[:, 9].abs().max()) == 0.0
        assert torch.equal(la[:, 10:12], l2[:, 10:12]) and torch.equal(la[:, 10:12], got["slot_abs_abs"])
        for n in GRAD_NAMES:
            assert torch.equal(got[f"slot_abs_{n}"], got[f"slot_plain_{n}"]), n
        assert rel_l2(got["slot_abs_abs"], got["atomic_abs_abs"]) < 1e-5  # the routes differ by the order of their sums


def test_no_intersections_give_zero_abs_outputs(dev):
    from clm_gs_amd import _lib
    from clm_gs_amd._lib import check, dptr, stream
    L = _lib.lib()
    n, w, h = 12, 32, 16
    tw, th = 2, 1
    nan = float("nan")
    packed = torch.zeros(n, 16, device=dev)
    off = torch.zeros(1, th, tw, dtype=torch.int32, device=dev)
    al = torch.zeros(1, h, w, device=dev)
    last = torch.zeros(1, h, w, dtype=torch.int32, device=dev)
    vi = torch.ones(1, h, w, 3, device=dev)
    for slot in (False, True):
        pg = torch.full((n, 16), nan, device=dev)
        outs = [torch.full((1, n, 2), nan, device=dev), torch.full((1, n, 3), nan, device=dev),
                torch.full((1, n, 3), nan, device=dev), torch.full((1, n), nan, device=dev)]
        v_abs = torch.full((n, 2), nan, device=dev)
        parts = torch.zeros(1, 16, device=dev)
        row_cum = torch.zeros(n, dtype=torch.int64, device=dev)
        tail = (None, dptr(row_cum), dptr(parts)) if slot else (None, None, None)  # an empty emit_slot: NULL data pointer
        rc = L.clmgs_rasterize_abs_bwd(stream(), 1, n, 0, dptr(packed), None, w, h, 16, tw, th, dptr(off), None, dptr(al),
                                       dptr(last), dptr(vi), None, dptr(pg), *[dptr(x) for x in outs], *tail, dptr(v_abs))
        assert rc == 0
        torch.cuda.synchronize()
        assert float(v_abs.abs().max()) == 0.0 and float(pg.abs().max()) == 0.0
        assert all(float(x.abs().max()) == 0.0 for x in outs)


def test_operator_sets_means2d_absgrad_and_refuses_a_fourth_channel(dev):
    from clm_gs_amd import gsplat as G
    case = S.shape_case("17x17")
    C, N = case["op"].shape
    w, h = case["w"], case["h"]
    ref = run_abs(case, dev, slot=False)
    grads = {}
    for flag in (False, True):
        m2, cn, col, op = (case[k].to(dev).requires_grad_() for k in ("m2", "cn", "col", "op"))
        img, al = G.rasterize_to_pixels(m2, cn, col, op, w, h, 16, case["off"].to(dev), case["fids"].to(dev),
                                        backgrounds=case["bg"].to(dev), absgrad=flag)
        ((img * case["vi"].to(dev)).sum() + (al[..., 0] * case["va"].to(dev)).sum()).backward()
        grads[flag] = (m2.grad.cpu(), cn.grad.cpu(), col.grad.cpu(), op.grad.cpu())
        if flag:
            assert m2.absgrad.shape == m2.shape and m2.absgrad.dtype == torch.float32
            assert rel_l2(m2.absgrad.cpu().reshape(-1, 2), ref["atomic_abs_abs"]) < 1e-5  # (atomics: order only)
            ref_abs, _ = case_absgrad(case)
            assert rel_l2(m2.absgrad.cpu().reshape(-1, 2), ref_abs) < GRAD_TOL
        else:
            assert not hasattr(m2, "absgrad")
    for a, b in zip(grads[True], grads[False]):
        assert rel_l2(a, b) < GRAD_TOL
    # four channels: refused before anything runs (no output exists, no input is touched)
    m2, cn, col, op = (case[k].to(dev) for k in ("m2", "cn", "col", "op"))
    col4 = torch.cat([col, torch.ones(C, N, 1, device=dev)], -1).requires_grad_()
    with pytest.raises(NotImplementedError):
        G.rasterize_to_pixels(m2.requires_grad_(), cn, col4, op, w, h, 16, case["off"].to(dev), case["fids"].to(dev),
                              absgrad=True)
    assert not hasattr(m2, "absgrad") and col4.grad is None


# ------------------------------------------------------------------------------------------- engines
W, H, N, BSZ = 96, 64, 3000, 4


def _setup(strategy, residency="hbm", absgrad=True, fused=True, seed=0):
    from clm_gs_amd import utils
    from clm_gs_amd.synthetic import nadir_cameras, synth_gaussians
    staging = {}
    if residency == "host_batch":  # host-resident rows staged as the union of the batch
        residency, staging = "host", {"host_staging": "batch"}
    args = utils.default_args(bsz=BSZ, sh_residency=residency, fused_front_end=fused, absgrad=absgrad, **staging)
    setattr(args, strategy, True)
    utils.set_args(args)
    utils.set_img_size(H, W)
    utils.set_cur_iter(1)
    sc = synth_gaussians(N, seed=seed, device="cuda")
    cams = nadir_cameras(BSZ, N, W, H, 0.35, seed=seed, device="cuda")
    g = torch.Generator().manual_seed(5)
    for c in cams:
        c.original_image = (torch.rand(3, H, W, generator=g) * 255).to(torch.uint8).cuda()
    return args, sc, cams


def _make(strategy, sc, args):
    if strategy == "no_offload":
        from clm_gs_amd.strategies.no_offload import GaussianModelNoOffload as M
    else:
        from clm_gs_amd.strategies.clm_offload import GaussianModelCLMOffload as M
    m = M(3)
    m.create_from_tensors(sc["xyz"].clone(), sc["shs48"].clone(), sc["scaling"].clone(),
                          sc["rotation"].clone(), sc["opacity"].clone(), spatial_lr_scale=1.0)
    m.active_sh_degree = 3
    m.training_setup(args)
    return m


class _Scene:
    cameras_extent = 30.0


_BATCHES = {}


def _batch(strategy, residency="hbm", absgrad=True, fused=True):
    """One batch of the engine (clm: + flush_lazy_rows) -> statistics, losses and parameters on the CPU; run once per
    configuration and shared by the tests below."""
    key = (strategy, residency, absgrad, fused)
    if key in _BATCHES:
        return _BATCHES[key]
    args, sc, cams = _setup(strategy, residency, absgrad, fused)
    m = _make(strategy, sc, args)
    if strategy == "no_offload":
        from clm_gs_amd.strategies.no_offload import baseline_accumGrads_impl
        losses, _ = baseline_accumGrads_impl(m, _Scene, cams, None)
        order = list(range(BSZ))
        shs = None
    else:
        from clm_gs_amd.strategies.clm_offload import clm_offload_train_one_batch
        comm = torch.cuda.Stream()
        gen = torch.Generator(device="cuda").manual_seed(1)
        losses, order, _ = clm_offload_train_one_batch(m, _Scene, cams, m.parameters_grad_buffer, None, None, comm, gen)
        m.flush_lazy_rows()
        shs = m._parameters.detach().cpu().clone()
    torch.cuda.synchronize()
    lo = [0.0] * BSZ
    for k, l in zip(order, losses):
        lo[k] = l.item()
    r = dict(accum=m.xyz_gradient_accum.detach().cpu().reshape(-1).clone(), denom=m.denom.detach().cpu().reshape(-1).clone(),
             maxr=m.max_radii2D.detach().cpu().reshape(-1).clone(), losses=lo, shs=shs,
             small=[t.detach().cpu().clone() for t in (m._xyz, m._opacity, m._scaling, m._rotation)])
    _BATCHES[key] = r
    return r


@pytest.fixture(scope="module")
def float64_statistic():
    """xyz_gradient_accum of one batch with absgrad, composed in float64 per camera: the oracle's projection, SH, binning
    and training_loss image cotangent, the per-pixel reference, then ||abs * (W/2, H/2)|| over the rows with radius > 0."""
    _, sc, cams = _setup("no_offload")
    P = {k: sc[k].detach().cpu().double() for k in ("xyz", "opacity", "scaling", "rotation", "shs48")}
    acc = torch.zeros(N, dtype=torch.float64)
    for c in cams:
        vm = c.world_view_transform.t().cpu().double()
        with torch.no_grad():
            img, m2, radii, aux = O.render_one_camera(P["xyz"], torch.sigmoid(P["opacity"]), torch.exp(P["scaling"]),
                                                      torch.nn.functional.normalize(P["rotation"]),
                                                      P["shs48"].reshape(-1, 16, 3), 3, vm, c.K.cpu().double(), W, H)
        leaf = img.detach().requires_grad_()
        O.training_loss(leaf, c.original_image.cpu()).backward()
        vi = leaf.grad.permute(1, 2, 0)[None].contiguous()
        a, _ = absgrad_reference(m2, aux["conics"], aux["colors"], torch.sigmoid(P["opacity"]).reshape(1, -1), W, H,
                                 aux["offsets"], aux["flatten_ids"], vi)
        stat = ((a[:, 0] * (W / 2)) ** 2 + (a[:, 1] * (H / 2)) ** 2).sqrt()
        acc += torch.where(radii.reshape(-1) > 0, stat, torch.zeros_like(stat))
    return acc


def test_no_offload_statistic_matches_the_float64_composition(dev, float64_statistic):
    on, off = _batch("no_offload", absgrad=True), _batch("no_offload", absgrad=False)
    e = rel_l2(on["accum"], float64_statistic)
    print(f"fused no_offload xyz_gradient_accum vs float64: rel_l2 {e:.3g}")
    assert e < 1e-3  # the bound of test_no_offload_batch_matches_oracle for whole-path gradients
    assert torch.equal(on["denom"], off["denom"]) and torch.equal(on["maxr"], off["maxr"])
    assert float(on["accum"].norm()) > 2 * float(off["accum"].norm())


@pytest.mark.parametrize("strategy", ["clm_offload", "no_offload"])
def test_fused_equals_op_by_op_under_absgrad(dev, strategy, float64_statistic):
    a, b = _batch(strategy, fused=True), _batch(strategy, fused=False)
    assert torch.allclose(a["denom"], b["denom"]) and torch.allclose(a["maxr"], b["maxr"])
    e = rel_l2(a["accum"], b["accum"])
    print(f"{strategy} fused vs op-by-op xyz_gradient_accum: rel_l2 {e:.3g}")
    assert e < 1e-4  # the bounds of test_fused_front_end_equals_op_by_op_path
    assert rel_l2(b["accum"], float64_statistic) < 1e-3  # and the op-by-op path really took the absgrad


def test_engines_agree_on_the_statistic(dev):
    ref = _batch("no_offload")
    for residency in ("hbm", "host", "host_batch"):
        e = rel_l2(_batch("clm_offload", residency)["accum"], ref["accum"])
        print(f"clm_offload {residency} vs no_offload xyz_gradient_accum: rel_l2 {e:.3g}")
        assert e < 1e-4, residency


def test_absgrad_changes_only_the_statistic_on_clm_hbm(dev):
    on, off = _batch("clm_offload", absgrad=True), _batch("clm_offload", absgrad=False)
    assert on["losses"] == off["losses"]
    for a, b in zip(on["small"], off["small"]):
        assert torch.equal(a, b)
    assert torch.equal(on["shs"], off["shs"])
    assert torch.equal(on["denom"], off["denom"]) and torch.equal(on["maxr"], off["maxr"])
    assert float(on["accum"].norm()) > 2 * float(off["accum"].norm())


def test_camera_without_intersections_counts_its_filter_rows(dev):
    """clm exact-filter form: every filter row of a camera that sees nothing gets 0 added to the accumulator and 1 to
    denom; rows outside the filter are not touched."""
    from clm_gs_amd import fused
    args, sc, cams = _setup("clm_offload")
    m = _make("clm_offload", sc, args)
    with torch.no_grad():  # the whole scene behind the camera
        m._xyz[:, 2] += 1.0e4
    m.invalidate_small_packed()
    rows = torch.arange(0, N, 3, dtype=torch.int64, device="cuda")
    for p in (m._xyz, m._opacity, m._scaling, m._rotation):
        p.grad = torch.zeros_like(p)
    acc0, den0 = m.xyz_gradient_accum.clone(), m.denom.clone()
    g_sh = torch.zeros((N, 48), device="cuda")
    p = fused.camera_forward(m, cams[0], rows, m._parameters.data, 1, None, cams[0].original_image)
    fused.camera_backward(m, p, g_sh, update_stats=True)
    torch.cuda.synchronize()
    hit = torch.zeros(N, dtype=torch.bool, device="cuda")
    hit[rows] = True
    assert torch.equal(m.xyz_gradient_accum, acc0)
    assert torch.equal(m.denom.reshape(-1), den0.reshape(-1) + hit.float())
    assert float(g_sh.abs().sum()) == 0.0
