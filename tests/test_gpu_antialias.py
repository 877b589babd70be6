"""-m gpu: gsplat's rasterize_mode="antialiased" (Mip-Splatting opacity compensation) through the operator, the fused
front-end kernels and the engines, against the float64 reference of tests/antialias_reference.py.

Bounds (tests/test_antialias_cpu.py derives and measures them on the fp32 formulas): compensation rel-L2 < 1e-5 (the
conics' bound of tests/test_gpu_ops.py::test_projection_fwd_bwd), gradients rel-L2 < GRAD_TOL = 2e-4, engine paths
against each other 1e-4 and against the float64 composition 1e-3 (tests/test_gpu_engines.py).  Scene A = small_scene()
(compensation 0.68-0.99), scene B = small_scene(log_scale=-3.5) (0.043-0.63).  Every test prints the figure it
asserts on."""
import ctypes
import math

import numpy as np
import pytest
import torch

from oracle import gs_oracle as O
from tests import antialias_reference as R
from tests.scenes import psnr, rel_l2, small_scene

pytestmark = pytest.mark.gpu

GRAD_TOL = 2e-4
COMP_TOL = 1e-5
SCENES = {"A": {}, "B": {"log_scale": -3.5}}


def _cams(s, C):
    """C cameras: the scene's, then copies moved sideways and back."""
    vms = []
    for c in range(C):
        vm = s["viewmat"].clone()
        vm[:3, 3] += torch.tensor([0.4 * c, -0.25 * c, 0.5 * c])
        vms.append(vm)
    return torch.stack(vms), s["K"][None].repeat(C, 1, 1).contiguous()


# ------------------------------------------------------------------------------------------- operator
@pytest.mark.parametrize("C", [1, 3])
@pytest.mark.parametrize("name", ["A", "B"])
def test_operator_compensations_and_gradients(dev, name, C):
    from clm_gs_amd import gsplat as G
    s = small_scene(**SCENES[name])
    N, w, h = s["means"].shape[0], s["width"], s["height"]
    vms, Ks = _cams(s, C)
    (m0, q0, s0), _, _ = R.scene_f64(s)
    r_ref, m2_ref, d_ref, cn_ref, k_ref = R.projection(m0, q0, s0, vms.double(), Ks.double(), w, h)
    g = torch.Generator().manual_seed(11)
    v2, vc, vd, vk = (torch.randn(C, N, 2, generator=g), torch.randn(C, N, 3, generator=g), torch.randn(C, N, generator=g),
                      torch.randn(C, N, generator=g))
    ((m2_ref * v2).sum() + (cn_ref * vc).sum() + (d_ref * vd).sum() + (k_ref * vk).sum()).backward()

    m, q, sc = (s[k].to(dev).requires_grad_() for k in ("means", "quats", "scales"))
    radii, m2, d, cn, comp = G.fully_fused_projection(m, None, q, sc, vms.to(dev), Ks.to(dev), w, h, calc_compensations=True)
    assert comp.shape == (C, N) and comp.dtype == torch.float32 and comp.requires_grad
    ((m2 * v2.to(dev)).sum() + (cn * vc.to(dev)).sum() + (d * vd.to(dev)).sum() + (comp * vk.to(dev)).sum()).backward()
    assert torch.equal(radii.cpu(), r_ref)
    ok = r_ref > 0
    assert float(comp.detach().cpu()[~ok].abs().max()) == 0.0
    e = rel_l2(comp.detach().cpu()[ok], k_ref.detach()[ok])
    print(f"scene {name} C={C}: compensation rel_l2 {e:.3g}")
    assert e < COMP_TOL
    for pname, x, y in (("means", m, m0), ("quats", q, q0), ("scales", sc, s0)):
        e = rel_l2(x.grad.cpu(), y.grad)
        print(f"scene {name} C={C}: v_{pname} rel_l2 {e:.3g}")
        assert e < GRAD_TOL, (pname, e)
    # flag off: the plain entry, None in the fifth place, and the same four outputs bit for bit
    with torch.no_grad():
        r1, m21, d1, cn1, none = G.fully_fused_projection(m, None, q, sc, vms.to(dev), Ks.to(dev), w, h)
        assert none is None
        for a, b in ((radii, r1), (m2, m21), (d, d1), (cn, cn1)):
            assert torch.equal(a.detach(), b)
        # packed form: the same values at (camera_ids, gaussian_ids)
        ci, gi, rp, m2p, dp, cnp, kp = G.fully_fused_projection(m, None, q, sc, vms.to(dev), Ks.to(dev), w, h, packed=True,
                                                                calc_compensations=True)
        assert kp.shape == (int(ok.sum()),)
        assert torch.equal(kp, comp.detach()[ci, gi]) and torch.equal(rp, radii[ci, gi]) and torch.equal(cnp, cn.detach()[ci, gi])
        assert G.fully_fused_projection(m, None, q, sc, vms.to(dev), Ks.to(dev), w, h, packed=True)[6] is None


# ------------------------------------------------------------------------------------------- fused kernels, C ABI
W0, H0 = 64, 48


def _pre_case(V, with_filter):
    """Raw parameters of N rows (scene B's regime), a tenth of them behind the camera, and the filter (or None: all rows)."""
    N = max(2 * V, 4) if with_filter else V
    s = small_scene(n=N, log_scale=-3.5, seed=1)
    means = s["means"].clone()
    behind = (torch.arange(N) % 10) == 5
    means[behind, 2] = -6.0
    g = torch.Generator().manual_seed(100 + V)
    filt = None
    if with_filter:
        filt = torch.randperm(N, generator=g)[:V].sort().values
        if V == 1:  # a row that is on screen
            with torch.no_grad():
                r = R.projection(means.double(), s["quats"].double(), s["scales"].double(), s["viewmat"].double()[None],
                                 s["K"].double()[None], W0, H0)[0]
            filt = torch.nonzero(r[0] > 0).flatten()[:1]
    raw = dict(xyz=means.contiguous(), opacity=torch.logit(s["opac"].reshape(N)).contiguous(),
               scaling=torch.log(s["scales"]).contiguous(), rotation=s["quats"].contiguous(),
               shs=s["shs"].reshape(N, 48).contiguous())
    pg = torch.randn(V, 16, generator=g)
    pg[:, 9:] = 0.0
    pg[:, 10:12] = torch.rand(V, 2, generator=g)  # the abs pair (read by the abs entries only)
    return raw, filt, s["viewmat"].contiguous(), s["K"].contiguous(), pg, N


def _reference(raw, filt, vm, K, pg, deg):
    """Float64 composition over the filter's rows: reference projection, the oracle's SH, clamp, opacity * compensation;
    gradients of the raw parameters from the gradient lines  x y ca cb | cc r g b | o  (tests/front_end_reference.py, which
    tests/test_front_end_cpu.py holds to the composition that stood here)."""
    from tests import front_end_reference as FR
    return FR.reference(raw, filt, dict(viewmat=vm, K=K, width=W0, height=H0), deg, True, lines=pg)


def _run_pre(dev, raw, filt, vm, K, pg, N, V, deg, pk, fwd_name, bwd_name):
    from clm_gs_amd import _lib
    from clm_gs_amd._lib import check, dptr, stream
    L = _lib.lib()
    npp = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    vmh = np.ascontiguousarray(vm.numpy().astype(np.float32).reshape(16))
    Kh = np.ascontiguousarray(K.numpy().astype(np.float32).reshape(9))
    cp = np.ascontiguousarray(np.linalg.inv(vm.numpy().astype(np.float64))[:3, 3].astype(np.float32))
    d = {k: v.to(dev) for k, v in raw.items()}
    fd = filt.to(dev) if filt is not None else None
    if pk:
        tab = torch.zeros(N, 12, device=dev)
        tab[:, 0:3], tab[:, 3], tab[:, 4:7], tab[:, 7:11] = d["xyz"], d["opacity"], d["scaling"], d["rotation"]
        small = (dptr(tab), None, None, None)
    else:
        small = (dptr(d["xyz"]), dptr(d["opacity"]), dptr(d["scaling"]), dptr(d["rotation"]))
    nan = float("nan")
    radii = torch.full((V,), -7, dtype=torch.int32, device=dev)
    m2, dep, cn, col, op = (torch.full(s_, nan, device=dev) for s_ in ((V, 2), (V,), (V, 3), (V, 3), (V,)))
    packed = torch.full((V, 16), nan, device=dev)
    check(getattr(L, fwd_name)(stream(), V, dptr(fd, torch.int64, True), *small, dptr(d["shs"]), 1, npp(vmh), npp(Kh), npp(cp),
                               W0, H0, deg, 0.3, 0.01, 1e10, 0.0, dptr(radii), dptr(m2), dptr(dep), dptr(cn), dptr(col),
                               dptr(op), dptr(packed), None))
    out = dict(radii=radii, m2=m2, dep=dep, cn=cn, col=col, op=op, packed=packed)
    if bwd_name is not None:
        if pk:
            gtab = torch.zeros(N, 12, device=dev)
            gsmall = (dptr(gtab), None, None, None)
        else:
            gs = [torch.zeros(N, 3, device=dev), torch.zeros(N, device=dev), torch.zeros(N, 3, device=dev),
                  torch.zeros(N, 4, device=dev)]
            gsmall = tuple(dptr(x) for x in gs)
        gsh = torch.zeros(N, 48, device=dev)
        maxr, acc, den = (torch.zeros(N, device=dev) for _ in range(3))
        pgd = pg.to(dev).contiguous()
        tail = (None,) if bwd_name.endswith("abs_bwd") else ()
        check(getattr(L, bwd_name)(stream(), V, dptr(fd, torch.int64, True), *small, dptr(d["shs"]), 1, npp(vmh), npp(Kh),
                                   npp(cp), W0, H0, deg, 0.3, dptr(radii), dptr(pgd), *gsmall, dptr(gsh), dptr(maxr),
                                   dptr(acc), dptr(den), None, 0, None, None, None, None, 0, *tail))
        if pk:
            gs = [gtab[:, 0:3], gtab[:, 3], gtab[:, 4:7], gtab[:, 7:11]]
        out.update(g_xyz=gs[0], g_opacity=gs[1], g_scaling=gs[2], g_rotation=gs[3], g_shs=gsh, maxr=maxr, acc=acc, den=den)
    torch.cuda.synchronize()
    return {k: v.detach().cpu().clone() for k, v in out.items()}


@pytest.mark.parametrize("V", [1, 63, 64, 65, 400])
def test_fused_aa_kernels_against_the_composition(dev, V):
    """clmgs_preprocess_aa_fwd / _aa_bwd / _aa_abs_bwd for DEG in {0, 3}, packed and unpacked small attributes, with a
    filter (overlapped staging) and without one (identity, rows culled: the non-overlapped route)."""
    from clm_gs_amd import gsplat as G
    for with_filter in (True, False):
        raw, filt, vm, K, pg, N = _pre_case(V, with_filter)
        rows = filt if filt is not None else torch.arange(N)
        for deg in (0, 3):
            ref = _reference(raw, filt, vm, K, pg, deg)
            vis = ref["radii"] > 0
            assert bool(vis.any()) and (V < 10 or not bool(vis.all()))
            for pk in (False, True):
                what = f"V={V} filter={with_filter} deg={deg} pk={pk}"
                plain = _run_pre(dev, raw, filt, vm, K, pg, N, V, deg, pk, "clmgs_preprocess_fwd", "clmgs_preprocess_bwd")
                aa = _run_pre(dev, raw, filt, vm, K, pg, N, V, deg, pk, "clmgs_preprocess_aa_fwd", "clmgs_preprocess_aa_bwd")
                ab = _run_pre(dev, raw, filt, vm, K, pg, N, V, deg, pk, "clmgs_preprocess_aa_fwd", "clmgs_preprocess_aa_abs_bwd")
                pab = _run_pre(dev, raw, filt, vm, K, pg, N, V, deg, pk, "clmgs_preprocess_fwd", "clmgs_preprocess_abs_bwd")
                assert torch.equal(aa["radii"], ref["radii"]), what
                for k in ("radii", "m2", "dep", "cn", "col"):
                    assert torch.equal(aa[k], plain[k]), (what, k)
                # the record: x y o ca | cb cc r g | b; only the opacity word moves
                assert torch.equal(aa["packed"][:, 2], aa["op"]), what
                keep = [0, 1, 3, 4, 5, 6, 7, 8]
                assert torch.equal(aa["packed"][:, keep], plain["packed"][:, keep]), what
                assert float(aa["op"][~vis].abs().max() if bool((~vis).any()) else 0.0) == 0.0, what
                e = rel_l2(aa["op"][vis], plain["op"][vis].double() * ref["comp"][vis])
                assert e < COMP_TOL, (what, "opacity x compensation", e)
                assert rel_l2(aa["op"][vis], ref["op"][vis]) < COMP_TOL, what
                assert bool((aa["op"][vis] < plain["op"][vis]).all()), what
                worst = 0.0
                for k in ("xyz", "opacity", "scaling", "rotation", "shs"):
                    y = ref["grads"][k].reshape(aa["g_" + k].shape)
                    e = rel_l2(aa["g_" + k], y)
                    worst = max(worst, e)
                    assert e < GRAD_TOL, (what, k, e)
                    assert torch.equal(ab["g_" + k], aa["g_" + k]), (what, k, "abs entry")
                print(f"{what}: worst gradient rel_l2 {worst:.3g}")
                # the compensation's cotangent really arrives: without it the scale gradient is another one
                assert rel_l2(plain["g_scaling"], ref["grads"]["scaling"]) > 10 * GRAD_TOL, what
                assert torch.equal(aa["den"], plain["den"]) and torch.equal(aa["maxr"], plain["maxr"]), what
                assert torch.equal(aa["acc"], plain["acc"]), what
                assert torch.equal(ab["den"], plain["den"]) and torch.equal(ab["maxr"], plain["maxr"]), what
                assert torch.equal(ab["acc"], pab["acc"]), what  # the statistic of the abs pair, as the plain abs entry
                want = torch.zeros(N)
                want[rows] = ((pg[:, 10] * (0.5 * W0)) ** 2 + (pg[:, 11] * (0.5 * H0)) ** 2).sqrt()
                assert rel_l2(ab["acc"], want) < 1e-6, what
            if deg == 3 and V == 400:  # ... and the op-by-op composition on the GPU gives the same opacities
                with torch.no_grad():
                    r_, _, _, _, k_ = G.fully_fused_projection(
                        raw["xyz"][rows].to(dev), None, raw["rotation"][rows].to(dev), torch.exp(raw["scaling"][rows]).to(dev),
                        vm[None].to(dev), K[None].to(dev), W0, H0, calc_compensations=True)
                    op_ = torch.sigmoid(raw["opacity"][rows]).to(dev) * k_[0]
                assert torch.equal(r_[0].cpu(), aa["radii"]) and rel_l2(aa["op"], op_.cpu()) < COMP_TOL


# ------------------------------------------------------------------------------------------- engines
W, H, N, BSZ = 96, 64, 3000, 4  # tests/test_gpu_absgrad.py
LOG_SHRINK = 1.0  # the synthetic default (scale 0.7 units = 1.7 px here) gives compensations near 0.9: shrunk in this test


def _setup(strategy, residency="hbm", mode="antialiased", fused=True, seed=0, **over):
    from clm_gs_amd import utils
    from clm_gs_amd.synthetic import nadir_cameras, synth_gaussians
    extra = dict(over)
    if residency == "host_batch":
        residency, extra["host_staging"] = "host", "batch"
    if residency == "host_budget":  # about half of the rows resident in HBM (768 B per row)
        residency, extra["sh_hbm_budget_gb"] = "host", 1500 * 768 / 1e9
    if mode is not None:
        extra["rasterize_mode"] = mode
    args = utils.default_args(bsz=BSZ, sh_residency=residency, fused_front_end=fused, **extra)
    setattr(args, strategy, True)
    utils.set_args(args)
    utils.set_img_size(H, W)
    utils.set_cur_iter(1)
    sc = synth_gaussians(N, seed=seed, device="cuda")
    sc["scaling"] = sc["scaling"] - LOG_SHRINK
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


def _batch(strategy, residency="hbm", mode="antialiased", fused=True):
    """One batch, the optimizer left out (debug_skip_optimizer; no_offload never steps inside the engine) -> losses by
    camera, the five gradients (sums over the cameras), statistics, filter sizes and intersection counts, on the CPU."""
    from clm_gs_amd import _lib
    key = (strategy, residency, mode, fused)
    if key in _BATCHES:
        return _BATCHES[key]
    args, sc, cams = _setup(strategy, residency, mode, fused, debug_skip_optimizer=True)
    m = _make(strategy, sc, args)
    n0 = len(_lib.STATS["n_isects"])
    sparsity = None
    if strategy == "no_offload":
        from clm_gs_amd.strategies.no_offload import baseline_accumGrads_impl
        losses, _ = baseline_accumGrads_impl(m, _Scene, cams, None)
        order = list(range(BSZ))
        gsh = torch.cat((m._features_dc.grad, m._features_rest.grad), dim=1).reshape(-1, 48)
        small = [m._xyz.grad, m._opacity.grad, m._scaling.grad, m._rotation.grad]
    else:
        from clm_gs_amd.strategies.clm_offload import clm_offload_train_one_batch
        comm = torch.cuda.Stream()
        gen = torch.Generator(device="cuda").manual_seed(1)
        losses, order, sparsity = clm_offload_train_one_batch(m, _Scene, cams, m.parameters_grad_buffer, None, None, comm, gen)
        torch.cuda.synchronize()
        gsh = m.parameters_grad_buffer[:N]
        if residency == "hbm" and fused:
            gk = m.small_grad()
            small = [gk[:, 0:3], gk[:, 3:4], gk[:, 4:7], gk[:, 7:11]]
        else:
            small = [m._xyz.grad, m._opacity.grad, m._scaling.grad, m._rotation.grad]
    torch.cuda.synchronize()
    lo = [0.0] * BSZ
    for k, l in zip(order, losses):
        lo[k] = l.item()
    names = ("xyz", "opacity", "scaling", "rotation")
    r = dict(losses=lo, grads={**{n: t.detach().cpu().reshape(N, -1).clone() for n, t in zip(names, small)},
                               "shs": gsh.detach().cpu().reshape(N, 48).clone()},
             accum=m.xyz_gradient_accum.detach().cpu().reshape(-1).clone(), denom=m.denom.detach().cpu().reshape(-1).clone(),
             maxr=m.max_radii2D.detach().cpu().reshape(-1).clone(),
             filters=sorted(round(s * N) for s in sparsity) if sparsity is not None else None,
             n_isects=list(_lib.STATS["n_isects"][n0:]))
    _BATCHES[key] = r
    return r


def _close(a, b, tol, what):
    for u, v in zip(a["losses"], b["losses"]):
        assert abs(u - v) < tol, (what, "loss", u, v)
    for k in a["grads"]:
        e = rel_l2(a["grads"][k], b["grads"][k])
        print(f"{what}: {k} gradient rel_l2 {e:.3g}")
        assert e < tol, (what, k, e)


@pytest.fixture(scope="module")
def float64_batch(dev):
    """The batch in float64: reference projection + the oracle's SH, binning, rasterizer and training_loss."""
    _, sc, cams = _setup("no_offload")
    P = {k: sc[k].detach().cpu().double().requires_grad_() for k in ("xyz", "opacity", "scaling", "rotation", "shs48")}
    losses, images, comps = [], [], []
    for c in cams:
        vm = c.world_view_transform.t().cpu().double()
        img, _, radii, aux = R.render_one_camera(P["xyz"], torch.sigmoid(P["opacity"]), torch.exp(P["scaling"]),
                                                 torch.nn.functional.normalize(P["rotation"]),
                                                 P["shs48"].reshape(-1, 16, 3), 3, vm, c.K.cpu().double(), W, H)
        l = O.training_loss(img, c.original_image.cpu())
        l.backward()
        losses.append(l.item())
        images.append(img.detach())
        comps.append(aux["compensations"].detach()[0][radii[0] > 0])
    grads = {"xyz": P["xyz"].grad, "opacity": P["opacity"].grad.reshape(N, -1), "scaling": P["scaling"].grad,
             "rotation": P["rotation"].grad, "shs": P["shs48"].grad.reshape(N, 48)}
    return dict(losses=losses, grads=grads, images=images, comps=torch.cat(comps))


def test_scene_exercises_the_mode(dev, float64_batch):
    med = float(float64_batch["comps"].median())
    print(f"engine scene: median compensation of the visible rows {med:.3g}")
    assert med <= 0.8


@pytest.mark.parametrize("strategy", ["clm_offload", "no_offload"])
def test_fused_equals_op_by_op_antialiased(dev, strategy):
    _close(_batch(strategy, fused=True), _batch(strategy, fused=False), 1e-4, f"{strategy} fused vs op-by-op")


def test_residencies_agree_with_no_offload(dev):
    ref = _batch("no_offload")
    for residency in ("hbm", "host", "host_batch", "host_budget"):
        _close(_batch("clm_offload", residency), ref, 1e-4, f"clm_offload {residency} vs no_offload")


def test_no_offload_matches_the_float64_composition(dev, float64_batch):
    b = _batch("no_offload")
    for u, v in zip(b["losses"], float64_batch["losses"]):
        assert abs(u - v) < 2e-5
    for k in b["grads"]:
        e = rel_l2(b["grads"][k], float64_batch["grads"][k])
        print(f"no_offload antialiased vs float64: {k} gradient rel_l2 {e:.3g}")
        assert e < 1e-3, (k, e)


def _eval_image(strategy, mode, render_mode="RGB", white=False):
    """The strategy's eval render over a black background -> image[3,H,W] (and depth, alpha) on the CPU."""
    args, sc, cams = _setup(strategy, mode=mode)
    if white:  # every colour exactly 1: the image is the accumulated opacity
        sc["shs48"] = torch.zeros_like(sc["shs48"])
        sc["shs48"][:, 0:3] = 0.5 / O.SH_C0
    m = _make(strategy, sc, args)
    bg = torch.zeros(3, device="cuda")
    kw = {} if render_mode == "RGB" else dict(render_mode=render_mode, return_alpha=True)
    with torch.no_grad():
        if strategy == "clm_offload":
            from clm_gs_amd.strategies.clm_offload import clm_offload_eval_one_cam
            res = clm_offload_eval_one_cam(cams[0], m, bg, _Scene, **kw)
        else:
            from clm_gs_amd.strategies.no_offload import baseline_accumGrads_micro_step
            res = baseline_accumGrads_micro_step(m.get_xyz, m.get_opacity, m.get_scaling, m.get_rotation, m.get_features,
                                                 3, cams[0], bg, mode="eval", **kw)
            res = res[0] if render_mode == "RGB" else (res[0],) + tuple(res[4:])
    torch.cuda.synchronize()
    return res.cpu() if render_mode == "RGB" else tuple(t.cpu() for t in res)


def test_classic_against_antialiased(dev):
    """Same batch in both modes.  Equal: filters, radii (through max_radii2D), denom and the intersection totals of the
    op-by-op route (its binning does not read the opacity).  Different: every loss.  Darker or equal at every pixel over a
    black background, up to 1e-6: asserted where it is a theorem -- on the accumulated opacity (every factor 1 - alpha_i
    grows when every opacity shrinks), which is the image of the same Gaussians in one colour.  With colours that differ
    it does not hold pixel by pixel: a dark Gaussian in front of a bright one hides less of it once both are thinner
    (0.2 a + 0.8 a (1 - a) is 0.252 at a = 0.9 and 0.288 at a = 0.45)."""
    aa, cl = _batch("no_offload", fused=False), _batch("no_offload", mode="classic", fused=False)
    assert torch.equal(aa["denom"], cl["denom"]) and torch.equal(aa["maxr"], cl["maxr"])
    assert aa["n_isects"] == cl["n_isects"] and len(aa["n_isects"]) == BSZ and min(aa["n_isects"]) > 0
    assert all(abs(u - v) > 1e-6 for u, v in zip(aa["losses"], cl["losses"]))
    assert _batch("clm_offload", fused=False)["filters"] == _batch("clm_offload", mode="classic", fused=False)["filters"]
    a_img, c_img = _eval_image("no_offload", "antialiased", white=True), _eval_image("no_offload", "classic", white=True)
    over = float((a_img - c_img).max())
    print(f"one-colour image, antialiased - classic: max {over:.3g}, mean {float((a_img - c_img).mean()):.3g}")
    assert over <= 1e-6
    assert float((c_img - a_img).max()) > 0.01


def test_mode_off_is_the_parent(dev):
    """Guards the dispatch: a "classic" batch is bit-identical to one whose args were never given the flag."""
    for strategy in ("clm_offload", "no_offload"):
        a, b = _batch(strategy, mode="classic"), _batch(strategy, mode=None)
        assert a["losses"] == b["losses"]
        for k in a["grads"]:
            assert torch.equal(a["grads"][k], b["grads"][k]), (strategy, k)
        assert torch.equal(a["accum"], b["accum"]) and torch.equal(a["denom"], b["denom"])
    from clm_gs_amd import utils
    args = utils.default_args()
    del args.rasterize_mode  # an args object from before the flag
    utils.set_args(args)
    assert not utils.antialiased()


def test_eval_and_depth_modes(dev, float64_batch):
    """Depth modes go through the op-by-op chain and get the mode for free."""
    for strategy in ("clm_offload", "no_offload"):
        img = _eval_image(strategy, "antialiased")
        ps = psnr(img, float64_batch["images"][0])
        print(f"{strategy} antialiased eval render vs float64: {ps:.1f} dB")
        assert ps >= 60
        img_d, depth, alpha = _eval_image(strategy, "antialiased", render_mode="RGB+ED")
        assert torch.isfinite(depth).all() and float(depth.max()) > 0
        assert torch.equal(img_d, img)


def test_unknown_mode_raises_at_the_first_render(dev):
    from clm_gs_amd.strategies.no_offload import baseline_accumGrads_impl
    for fused in (True, False):
        args, sc, cams = _setup("no_offload", mode="bogus", fused=fused)
        m = _make("no_offload", sc, args)
        with pytest.raises(ValueError):
            baseline_accumGrads_impl(m, _Scene, cams, None)
    with pytest.raises(ValueError):
        _eval_image("clm_offload", "bogus")
    from clm_gs_amd import utils
    utils.set_args(utils.default_args())
