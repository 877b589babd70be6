"""-m gpu: contribution pruning -- the blend-weight kernel (csrc/contrib.hip) against float64, its bit reproducibility,
its tie to the shipped forward, the scoring pass on the three engines, the prune itself, and the trainer / CLI end to end.

Tolerances are those of tests/test_gpu_raster_edges.py (GRAD_TOL 2e-4; SAT_TOL 1e-3 for opacity-special rows and every
row of a saturating list): the sums have no cancellation, so the per-pixel bounds on alpha and T carry over.  Pixel
counts may differ by a row's allowance, the number of fragile pixels of the tiles that list it
(tests/contribution_reference.py).  Every test prints the figures it asserts on.

Worst figures measured on an MI355X: see DESIGN.md section 3, "Contribution pruning".
"""
import math
import os

import pytest
import torch

from oracle import gs_oracle as O
from tests import contribution_reference as R
from tests.scenes import rel_l2, small_scene

pytestmark = pytest.mark.gpu

CASES = R.case_names()


def _dev_inputs(case, dev):
    return (case["m2"].to(dev), case["cn"].to(dev), case["op"].to(dev), case["w"], case["h"], 16, case["off"].to(dev),
            case["fids"].to(dev))


def _run_raw(case, dev, raw=None, rows=None):
    """One launch on a raster case -> the raw triple (wsum_q, wmax_bits, pixels) it added into."""
    from clm_gs_amd import gsplat as G
    C, N = case["op"].shape
    if raw is None:
        raw = G.contribution_arrays(C * N, dev)
    G.rasterize_contributions(*_dev_inputs(case, dev), rows=rows, out=raw)
    torch.cuda.synchronize()
    return raw


def _values(raw):
    from clm_gs_amd import gsplat as G
    return tuple(t.cpu() for t in G.contribution_values(raw))


# ------------------------------------------------------------------------------------------- 1. kernel against float64
@pytest.mark.parametrize("name", CASES)
def test_kernel_matches_float64(dev, name):
    case, ref = R.cached(name)
    C, N = case["op"].shape
    wsum, wmax, pixels = _values(_run_raw(case, dev))
    assert wsum.dtype == torch.float64 and wmax.dtype == torch.float32 and pixels.dtype == torch.int64
    assert wsum.shape == wmax.shape == pixels.shape == (C * N,)
    assert torch.isfinite(wsum).all() and torch.isfinite(wmax).all()
    tols = R.row_tolerances(name, case)
    for gname, rows in case["groups"].items():
        rows = rows.reshape(-1)
        tol = tols[gname]
        for what, x, y in (("wsum", wsum, ref["wsum"]), ("wmax", wmax, ref["wmax"])):
            if float(y[rows].norm()) > 0:
                e = rel_l2(x[rows], y[rows])
                print(f"{name} {gname} {what}: rel_l2 {e:.3g} (tolerance {tol})")
                assert e < tol, (name, gname, what, e)
        sure = rows & (ref["allowance"] == 0)
        d = (wmax[sure].double() - ref["wmax"][sure]).abs()
        worst = float((d / ref["wmax"][sure].clamp_min(1e-300)).max()) if int(sure.sum()) else 0.0
        print(f"{name} {gname}: worst elementwise wmax error of rows with allowance 0: {worst:.3g}")
        assert bool((d <= tol * ref["wmax"][sure]).all()), (name, gname, worst)
    dp = (pixels - ref["pixels"]).abs()
    print(f"{name}: pixel counts differ on {int((dp > 0).sum())} rows, worst {int(dp.max())}, "
          f"largest allowance {int(ref['allowance'].max())}")
    assert bool((dp <= ref["allowance"]).all()), torch.nonzero(dp > ref["allowance"]).flatten().tolist()[:8]
    zero = ref["pixels"] == 0
    assert torch.equal(zero, ref["wsum"] == 0) and torch.equal(zero, ref["wmax"] == 0)
    for what, x in (("wsum", wsum), ("wmax", wmax), ("pixels", pixels)):
        bad = torch.nonzero(zero & (x != 0)).flatten().tolist()
        assert not bad, f"{name} {what}: rows {bad[:8]} are exactly zero in the reference"


# ------------------------------------------------------------------------------------------- 2. bits and accumulation
@pytest.mark.parametrize("name", CASES)
def test_bit_reproducible_and_accumulating(dev, name):
    case, _ = R.cached(name)
    a, b = _run_raw(case, dev), _run_raw(case, dev)
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    first = [t.clone() for t in a]
    _run_raw(case, dev, raw=a)  # a second launch into the same arrays
    assert torch.equal(a[0], 2 * first[0]) and torch.equal(a[2], 2 * first[2]) and torch.equal(a[1], first[1])
    assert bool((a[1] >= 0).all())


def test_rows_scatter(dev):
    from clm_gs_amd import gsplat as G
    case, _ = R.cached("tiles7")
    C, N = case["op"].shape
    base = _run_raw(case, dev)
    perm = torch.randperm(N, generator=torch.Generator().manual_seed(3)).to(dev)
    got = _run_raw(case, dev, raw=G.contribution_arrays(N, dev), rows=perm)
    for x, y in zip(got, base):
        want = torch.zeros_like(y)
        want[perm] = y
        assert torch.equal(x, want)
    # a longer table: rows beyond the case's stay untouched; a destination outside the arrays is dropped, not written
    wide = _run_raw(case, dev, raw=G.contribution_arrays(N + 5, dev), rows=perm + 5)
    assert all(int(t[:5].abs().sum()) == 0 for t in wide) and torch.equal(wide[0][5:], got[0])
    out_of_range = perm.clone()
    out_of_range[perm == 0] = N + 100
    out_of_range[perm == 1] = -1
    part = _run_raw(case, dev, raw=G.contribution_arrays(N, dev), rows=out_of_range)
    keep = torch.ones(N, dtype=torch.bool, device=dev)
    keep[:2] = False
    assert all(torch.equal(p[keep], g_[keep]) and int(p[:2].abs().sum()) == 0 for p, g_ in zip(part, got))


def test_rows_fold_cameras_onto_one_table(dev):
    """tiles9_C3: cameras 0 and 1 scattered through one row table = the sum / max of the per-camera results, exactly."""
    from clm_gs_amd import gsplat as G
    case, _ = R.cached("tiles9_C3")
    C, N = case["op"].shape
    per_cam = _run_raw(case, dev)  # row cam * N + g
    th, tw = case["off"].shape[1:]
    end01 = int(case["off"].reshape(C, -1)[2, 0])  # the lists of cameras 0 and 1 come first
    two = dict(case, m2=case["m2"][:2], cn=case["cn"][:2], op=case["op"][:2], off=case["off"][:2], fids=case["fids"][:end01])
    table = torch.arange(N, device=dev)
    folded = _run_raw(two, dev, raw=G.contribution_arrays(N, dev), rows=table)
    assert torch.equal(folded[0], per_cam[0][:N] + per_cam[0][N:2 * N])
    assert torch.equal(folded[2], per_cam[2][:N] + per_cam[2][N:2 * N])
    assert torch.equal(folded[1], torch.maximum(per_cam[1][:N], per_cam[1][N:2 * N]))
    assert int(per_cam[2][:N].sum()) > 0 and int(per_cam[2][N:2 * N].sum()) > 0
    # (int32 order of the bit patterns = float order: all are non-negative floats)
    assert torch.equal(folded[1].view(torch.float32), torch.maximum(per_cam[1][:N].view(torch.float32),
                                                                    per_cam[1][N:2 * N].view(torch.float32)))


# ------------------------------------------------------------------------------------------- 3. the shipped forward
@pytest.mark.parametrize("name", CASES)
def test_sum_equals_the_forward_alpha_image(dev, name):
    from tests.raster_edge_worker import run
    case, _ = R.cached(name)
    wsum, _, pixels = _values(_run_raw(case, dev))
    alpha = run(case, dev, atomic=False, slots=False)["alpha"].double()
    got, want = float(wsum.sum()), float(alpha.sum())
    print(f"{name}: sum(wsum) {got:.9g} forward alpha sum {want:.9g} rel {abs(got - want) / want:.3g}")
    assert abs(got - want) <= 1e-5 * want
    assert int(pixels.sum()) > 0


def test_nothing_listed_writes_nothing(dev):
    from clm_gs_amd import _lib, gsplat as G
    from clm_gs_amd._lib import check, dptr, stream
    from tests import scenes as S
    case, _ = R.cached("17x17")
    C, N = case["op"].shape
    L = _lib.lib()
    m2, cn, op, w, h, _, off, fids = _dev_inputs(case, dev)
    raw = G.contribution_arrays(N, dev)
    packed = torch.empty(L.clmgs_rasterize_contrib_pack_bytes(C, N), dtype=torch.uint8, device=dev)
    zero_off = torch.zeros_like(off)
    args = lambda n, f, o: (stream(), C, N, n, dptr(m2), dptr(cn), dptr(op), w, h, 16, off.shape[2], off.shape[1], dptr(o),
                            f, None, N, dptr(packed), dptr(raw[0]), dptr(raw[1]), dptr(raw[2]))
    check(L.clmgs_rasterize_contrib(*args(0, None, zero_off)))  # n_isects == 0, no list at all
    torch.cuda.synchronize()
    assert all(int(t.abs().sum()) == 0 for t in raw)
    # argument errors are refused before anything is written
    assert L.clmgs_rasterize_contrib(*args(fids.numel(), None, off)) != 0            # a count without a list
    bad = list(args(fids.numel(), dptr(fids), off))
    bad[9] = 8                                                                       # tile size
    assert L.clmgs_rasterize_contrib(*bad) != 0
    bad = list(args(fids.numel(), dptr(fids), off))
    bad[15] = N - 1                                                                  # arrays shorter than C*N, no row table
    assert L.clmgs_rasterize_contrib(*bad) != 0
    torch.cuda.synchronize()
    assert all(int(t.abs().sum()) == 0 for t in raw)
    # an empty camera next to a full one: its rows stay zero, the other camera's are those of a run on its own
    one = S.shape_case("17x17")
    m2e = torch.cat([one["m2"], one["m2"] - 1000.0])
    cat2 = lambda k: torch.cat([one[k], one[k]])
    radii = torch.cat([torch.full((1, N), 6, dtype=torch.int32), torch.zeros((1, N), dtype=torch.int32)])
    depths = torch.arange(N, dtype=torch.float32)[None].repeat(2, 1) + 1.0
    both = S._finish_case(m2e, cat2("cn"), cat2("col"), cat2("op"), radii, depths, one["w"], one["h"])
    assert int(both["off"].reshape(2, -1)[1].min()) == both["fids"].numel() > 0
    r2 = _run_raw(both, dev)
    solo = dict(both, m2=both["m2"][:1], cn=both["cn"][:1], op=both["op"][:1], off=both["off"][:1])
    r1 = _run_raw(solo, dev)
    assert all(torch.equal(a[:N], b) and int(a[N:].abs().sum()) == 0 for a, b in zip(r2, r1)) and int(r1[2].sum()) > 0


# ------------------------------------------------------------------------------------------- 4. the scoring pass
W, H, N_SCENE, N_CAMS = 64, 48, 400, 4
ENGINES = [("no_offload", "hbm"), ("clm_offload", "hbm"), ("clm_offload", "host")]


class _Scene:
    cameras_extent = 5.0


def _cameras(s):
    from clm_gs_amd.cameras import Camera
    f = 0.9 * W
    fovx, fovy = 2 * math.atan(W / (2 * f)), 2 * math.atan(H / (2 * f))
    g = torch.Generator().manual_seed(5)
    cams = []
    for c in range(N_CAMS):
        vm = s["viewmat"].clone()
        vm[:3, 3] += torch.tensor([0.4 * c, -0.25 * c, 0.5 * c])
        cams.append(Camera(c, vm, fovx, fovy, W, H, image_u8=(torch.rand(3, H, W, generator=g) * 255).to(torch.uint8)))
    return cams


def _model(strategy, residency, mode="classic", **over):
    from clm_gs_amd import utils
    args = utils.default_args(bsz=N_CAMS, sh_residency=residency, rasterize_mode=mode, **over)
    setattr(args, strategy, True)
    utils.set_args(args)
    utils.set_img_size(H, W)
    utils.set_cur_iter(1)
    s = small_scene(n=N_SCENE, width=W, height=H)
    if strategy == "no_offload":
        from clm_gs_amd.strategies.no_offload import GaussianModelNoOffload as M
    else:
        from clm_gs_amd.strategies.clm_offload import GaussianModelCLMOffload as M
    m = M(3)
    m.create_from_tensors(s["means"].cuda(), s["shs"].reshape(N_SCENE, 48).cuda(), torch.log(s["scales"]).cuda(),
                          s["quats"].cuda(), torch.logit(s["opac"]).cuda(), spatial_lr_scale=1.0)
    m.active_sh_degree = 3
    m.training_setup(args)
    return args, s, m, _cameras(s)


def _eval_alpha(strategy, m, cam):
    bg = torch.zeros(3, device="cuda")
    with torch.no_grad():
        if strategy == "clm_offload":
            from clm_gs_amd.strategies.clm_offload import clm_offload_eval_one_cam
            return clm_offload_eval_one_cam(cam, m, bg, _Scene, render_mode="RGB+D", return_alpha=True)[2]
        from clm_gs_amd.strategies.no_offload import baseline_accumGrads_micro_step
        res = baseline_accumGrads_micro_step(m.get_xyz, m.get_opacity, m.get_scaling, m.get_rotation, m.get_features, 3,
                                             cam, bg, mode="eval", render_mode="RGB+D", return_alpha=True)
        return res[5]


def _eval_image(m, cam):
    from clm_gs_amd.strategies.no_offload import baseline_accumGrads_micro_step
    with torch.no_grad():
        return baseline_accumGrads_micro_step(m.get_xyz, m.get_opacity, m.get_scaling, m.get_rotation, m.get_features, 3,
                                              cam, torch.zeros(3, device="cuda"), mode="eval")[0].clone()


@pytest.fixture(scope="module")
def engine_scores(dev):
    """score_cameras on the three engines (raw arrays on the CPU) and, per camera, (sum of wsum, sum of the eval alpha)."""
    from clm_gs_amd import contribution
    out = {}
    for strategy, residency in ENGINES:
        _, _, m, cams = _model(strategy, residency)
        st = contribution.score_cameras(m, cams)
        per_cam = []
        for cam in cams:
            one = contribution.score_cameras(m, [cam])
            per_cam.append((float(one.wsum.sum()), float(_eval_alpha(strategy, m, cam).double().sum())))
        torch.cuda.synchronize()
        out[(strategy, residency)] = (tuple(t.cpu() for t in st.raw), per_cam)
    return out


def test_scoring_pass_is_identical_on_the_three_engines(dev, engine_scores):
    ref = engine_scores[ENGINES[0]][0]
    assert int(ref[2].sum()) > 0 and int((ref[2] > 0).sum()) > N_SCENE // 4
    for key in ENGINES[1:]:
        for a, b in zip(engine_scores[key][0], ref):
            assert torch.equal(a, b), key


def test_scoring_pass_sums_to_the_eval_alpha(dev, engine_scores):
    for key in ENGINES:
        for i, (got, want) in enumerate(engine_scores[key][1]):
            print(f"{key} camera {i}: sum(wsum) {got:.9g} eval alpha sum {want:.9g} rel {abs(got - want) / want:.3g}")
            assert want > 10 and abs(got - want) <= 1e-4 * want


def test_antialiased_scores_match_float64(dev, engine_scores):
    """--antialiased changes the scores, and they are those of the float64 blend fed with opacity x compensation.  Bound:
    1e-3, the one the float32 engines are held to against the float64 composition (tests/test_gpu_antialias.py): the
    projection's float32 conics and means enter here, not the blend alone."""
    from clm_gs_amd import contribution
    from tests import antialias_reference as AR
    _, s, m, cams = _model("no_offload", "hbm", mode="antialiased")
    st = contribution.score_cameras(m, cams)
    wsum, wmax, pixels = st.wsum.cpu(), st.wmax.cpu(), st.pixels.cpu()
    classic = engine_scores[("no_offload", "hbm")][0]
    assert not torch.equal(st.wsum_q.cpu(), classic[0])
    assert float(wsum.sum()) < float(classic[0].sum()) * 2.0 ** -28  # thinner everywhere
    rs, rm, rp = torch.zeros(N_SCENE, dtype=torch.float64), torch.zeros(N_SCENE, dtype=torch.float64), torch.zeros(N_SCENE, dtype=torch.int64)
    means, quats, scales = s["means"].double(), torch.nn.functional.normalize(s["quats"].double()), s["scales"].double()
    tw, th = math.ceil(W / 16), math.ceil(H / 16)
    for cam in cams:
        vm, K = cam.world_view_transform.t().cpu().double()[None], cam.K.cpu().double()[None]
        radii, m2, depths, conics, comps = AR.projection(means, quats, scales, vm, K, W, H)
        _, ids, fids = O.isect_tiles(m2, radii, depths, 16, tw, th)
        off = O.isect_offset_encode(ids, 1, tw, th)
        r = R.contribution_reference(m2, conics, s["opac"].double().reshape(1, -1) * comps, W, H, off, fids)
        rs += r["wsum"]; rm = torch.maximum(rm, r["wmax"]); rp += r["pixels"]
    e_s, e_m = rel_l2(wsum, rs), rel_l2(wmax, rm)
    print(f"antialiased scores vs float64: wsum rel_l2 {e_s:.3g}, wmax rel_l2 {e_m:.3g}, pixel counts differ on "
          f"{int((pixels != rp).sum())} of {N_SCENE} rows (total {int(pixels.sum())} vs {int(rp.sum())})")
    assert e_s < 1e-3 and e_m < 1e-3
    from clm_gs_amd import utils
    utils.set_args(utils.default_args())


# ------------------------------------------------------------------------------------------- 5. pruning
def _tables(m):
    return [t.detach().clone() for tr in m._mcmc_tables() for t in tr if t is not None]


def test_sum_mode_prunes_exactly_the_lowest_rows(dev):
    """no_offload after one optimizer step (non-zero moments): contribution_prune(sum, 0.3) leaves N - floor(0.3 N) rows,
    the highest-scored ones, every parameter and moment row as it was -- and is prune_points on the same mask."""
    from clm_gs_amd import contribution, trainer
    from clm_gs_amd.strategies.no_offload import baseline_accumGrads_impl
    models = []
    for _ in range(2):
        args, _, m, cams = _model("no_offload", "hbm")
        baseline_accumGrads_impl(m, _Scene, cams, None)
        trainer.no_offload_optimizer_step(m, args, N_CAMS)
        models.append((m, cams))
    (a, cams), (b, _) = models
    before = _tables(a)
    assert len(before) == 18 and all(torch.equal(x, y) for x, y in zip(before, _tables(b)))
    assert float(before[1].abs().max()) > 0  # moments exist
    st = contribution.score_cameras(a, cams)
    mask = contribution.lowest_fraction_mask(st.wsum, 0.3)
    k = int(math.floor(0.3 * N_SCENE))
    assert int(mask.sum()) == k
    order = torch.sort(st.wsum, stable=True).indices
    assert torch.equal(torch.nonzero(mask).flatten(), order[:k].sort().values)
    n0, n1, _ = contribution.contribution_prune(a, cams, "sum", ratio=0.3)
    assert (n0, n1) == (N_SCENE, N_SCENE - k) and a.get_xyz.shape[0] == N_SCENE - k
    b.prune_points(mask)
    after_a, after_b = _tables(a), _tables(b)
    for x, y, z in zip(after_a, after_b, before):
        assert torch.equal(x, y) and torch.equal(x, z[~mask])
    assert a.xyz_gradient_accum.shape[0] == a.denom.shape[0] == a.max_radii2D.shape[0] == N_SCENE - k
    # the clm_offload model (HBM rows) through the same call: the same rows leave
    _, _, c, cams_c = _model("clm_offload", "hbm")
    xyz0, par0 = c._xyz.detach().clone(), c._parameters.detach().clone()
    contribution.contribution_prune(c, cams_c, "sum", ratio=0.3)
    assert torch.equal(c._xyz.detach(), xyz0[~mask]) and torch.equal(c._parameters.detach(), par0[~mask])


def test_pruning_rows_without_pixels_changes_no_render(dev):
    """Bit identity is expected (a zero-weight entry adds +0 to every accumulator); the bound asserted is 1e-6 absolute."""
    from clm_gs_amd import contribution
    _, _, m, cams = _model("no_offload", "hbm")
    st = contribution.score_cameras(m, cams)
    mask = st.pixels == 0
    assert 0 < int(mask.sum()) < N_SCENE
    before = [_eval_image(m, c) for c in cams]
    m.prune_points(mask)
    after = [_eval_image(m, c) for c in cams]
    worst = max(float((x - y).abs().max()) for x, y in zip(before, after))
    identical = all(torch.equal(x, y) for x, y in zip(before, after))
    print(f"pruned {int(mask.sum())} rows without pixels: worst render change {worst:.3g}, bit-identical: {identical}")
    assert worst <= 1e-6
    st2 = contribution.score_cameras(m, cams)
    keep = ~mask
    assert torch.equal(st2.wsum_q, st.wsum_q[keep]) and torch.equal(st2.pixels, st.pixels[keep])
    assert torch.equal(st2.wmax_bits, st.wmax_bits[keep])


def test_max_mode_and_no_pending_steps(dev):
    """mode max on clm_offload with deferred small-attribute steps waiting: the scores are those of the flushed model."""
    from clm_gs_amd import contribution
    from clm_gs_amd.strategies.clm_offload import clm_offload_train_one_batch
    _, _, m, cams = _model("clm_offload", "hbm")
    comm, gen = torch.cuda.Stream(), torch.Generator(device="cuda").manual_seed(1)
    clm_offload_train_one_batch(m, _Scene, cams, m.parameters_grad_buffer, None, None, comm, gen)
    st = contribution.score_cameras(m, cams)  # flushes first
    m.flush_lazy_rows()
    st2 = contribution.score_cameras(m, cams)
    assert all(torch.equal(x, y) for x, y in zip(st.raw, st2.raw))
    mask = contribution.below_max_mask(st.wmax, 0.01)
    assert torch.equal(mask, st.wmax < 0.01) and 0 < int(mask.sum()) < N_SCENE
    n0, n1, _ = contribution.contribution_prune(m, cams, "max", threshold=0.01)
    assert n1 == n0 - int(mask.sum())


# ------------------------------------------------------------------------------------------- 6. end to end
@pytest.mark.parametrize("strategy,residency", ENGINES)
def test_trainer_prunes_logs_and_evaluates(dev, tmp_path, strategy, residency):
    from clm_gs_amd import io_ply, prune_model, trainer
    from tests.test_gpu_exposure import _tiny_scene
    work, out = _tiny_scene(tmp_path), tmp_path / "out"
    gaussians, scene, _ = trainer.train_from_colmap(
        str(work), str(out), strategy=strategy, iterations=60, test_iterations=(57,), bsz=4, sh_residency=residency,
        disable_auto_densification=True, contrib_prune_iterations=(40,), contrib_prune_ratio=0.2)
    n0 = 150 * len(scene.train_cameras)
    want = n0 - int(math.floor(0.2 * n0))
    log = open(out / "python_ws=1_rk=0.log").read()
    lines = [l for l in log.splitlines() if l.startswith("contribution prune")]
    print(lines)
    assert len(lines) == 1 and f"at iteration 37: mode sum rows {n0} -> {want} " in lines[0] and "scoring pass" in lines[0]
    assert gaussians.get_xyz.shape[0] == want
    assert f"contribution_prune. Now num of 3dgs: {want}." in log
    ev = [l for l in log.splitlines() if "Evaluating train:" in l]
    assert len(ev) == 1 and math.isfinite(float(ev[0].split("PSNR ")[1]))
    assert log.index("contribution prune") < log.index("Evaluating train:")
    assert log.count(" loss: ") == 15 and "end2end total_time:" in log
    ply = out / "point_cloud" / "iteration_60" / "point_cloud.ply"
    saved = io_ply.load_ply(str(ply))
    assert saved["xyz"].shape[0] == want
    if strategy != "clm_offload" or residency != "hbm":
        return
    # the post-hoc CLI on the saved model: the kept rows, in order, bit for bit
    pruned = tmp_path / "pruned.ply"
    assert prune_model.main(["-m", str(out), "-s", str(work), "--mode", "sum", "--ratio", "0.25", "-o", str(pruned)]) == 0
    got = io_ply.load_ply(str(pruned))
    k = int(math.floor(0.25 * want))
    assert got["xyz"].shape[0] == want - k
    from clm_gs_amd import contribution
    st = contribution.score_cameras(contribution.tensors_model(saved["xyz"], saved["opacity"], saved["scaling"],
                                                               saved["rotation"]), scene.train_cameras)
    keep = (~contribution.lowest_fraction_mask(st.wsum, 0.25)).cpu()
    for name in ("xyz", "shs48", "opacity", "scaling", "rotation"):
        assert torch.equal(got[name], saved[name][keep]), name
    assert prune_model.main(["-m", str(ply), "-s", str(work), "--mode", "max", "--threshold", "0.01", "-o", str(pruned)]) == 0
    assert io_ply.load_ply(str(pruned))["xyz"].shape[0] == int((st.wmax >= 0.01).sum())
