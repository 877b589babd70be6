"""GPU: the orthographic camera model (gsplat's camera_model="ortho") from the operator to the orthophoto tool, against
the float64 reference of tests/ortho_reference.py.  Tolerances are those of tests/test_gpu_ops.py: images PSNR >= 60 dB
and max-abs <= 2e-4, gradients rel-L2 <= GRAD_TOL, integer outputs bit-exact."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from oracle import gs_oracle as O
from tests import ortho_reference as R
from tests.scenes import psnr, rel_l2, small_scene
from tests.test_ortho_cpu import PPU, ortho_scene

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GRAD_TOL = 2e-4
IMG_TOL = 2e-4


def check_image(got, ref, what=""):
    got, ref = got.detach().cpu().double(), ref.detach().double()
    e, p = float((got - ref).abs().max()), psnr(got, ref)
    print(f"{what}: max-abs {e:.3g}, PSNR {p:.1f} dB")
    assert e <= IMG_TOL and p >= 60.0, (what, e, p)


def check_grad(got, ref, what):
    ref = ref.detach()
    if float(ref.abs().max()) == 0.0:
        assert float(got.abs().max()) == 0.0, what
        return
    e = rel_l2(got.detach().cpu(), ref)
    print(f"{what}: rel_l2 {e:.3g}")
    assert e < GRAD_TOL, (what, e)


# ------------------------------------------------------------------------------------------------ 1. operator
@functools.lru_cache(maxsize=None)
def op_reference(C):
    """Scene four on C cameras (shifted as in test_projection_fwd_bwd): float64 outputs, cotangents, and the gradients of
    sum(outputs * cotangents) without and with the compensation's cotangent.  Shared, never modified."""
    s = ortho_scene("large")
    vms = torch.stack([s["viewmat"]] * C)
    for c in range(C):
        vms[c, 0, 3] += 0.4 * c
    Ks = torch.stack([s["K"]] * C)
    m, q, sc = [s[k].double().clone().requires_grad_() for k in ("means", "quats", "scales")]
    r0, m0, d0, c0, k0 = R.projection(m, q, sc, vms.double(), Ks.double(), 200, 120)
    g = torch.Generator().manual_seed(5)
    cot = [torch.randn(t.shape, generator=g) for t in (m0, d0, c0, k0)]
    plain = (m0 * cot[0].double()).sum() + (d0 * cot[1].double()).sum() + (c0 * cot[2].double()).sum()
    g_plain = torch.autograd.grad(plain, (m, q, sc), retain_graph=True)
    g_aa = torch.autograd.grad(plain + (k0 * cot[3].double()).sum(), (m, q, sc))
    return dict(s=s, vms=vms, Ks=Ks, out=tuple(t.detach() for t in (r0, m0, d0, c0, k0)), cot=cot, plain=g_plain, aa=g_aa)


def run_operator(dev, ref, n, aa):
    from clm_gs_amd import gsplat as G
    s = ref["s"]
    leaves = [s[k][:n].clone().to(dev).requires_grad_() for k in ("means", "quats", "scales")]
    out = G.fully_fused_projection(leaves[0], None, leaves[1], leaves[2], ref["vms"].to(dev), ref["Ks"].to(dev), 200, 120,
                                   calc_compensations=aa, camera_model="ortho")
    return leaves, out


@pytest.mark.parametrize("aa", [False, True])
@pytest.mark.parametrize("C", [1, 3])
def test_operator_fwd_bwd(dev, C, aa):
    ref = op_reference(C)
    r0, m0, d0, c0, k0 = ref["out"]
    N = r0.shape[1]
    leaves, (r1, m1, d1, c1, k1) = run_operator(dev, ref, N, aa)
    assert torch.equal(r1.cpu(), r0), "radii must be bit-exact"
    ok = r0 > 0
    assert all(int(ok[c].sum()) > 1000 for c in range(C))
    assert float(((m1.detach().cpu() - m0.float()).abs() / (1 + m0.float().abs()))[ok].max()) < 1e-5
    assert rel_l2(d1.cpu()[ok], d0[ok]) < 1e-6
    assert rel_l2(c1.cpu()[ok], c0[ok]) < 1e-5
    for t in (m1, d1, c1):
        assert float(t.detach().cpu()[~ok].abs().max()) == 0.0, "culled entries are zero"
    loss = sum((a * v.to(dev)).sum() for a, v in zip((m1, d1, c1), ref["cot"]))
    if aa:
        assert rel_l2(k1.cpu()[ok], k0[ok]) < 1e-5 and float(k1.detach().cpu()[~ok].abs().max()) == 0.0
        loss = loss + (k1 * ref["cot"][3].to(dev)).sum()
    else:
        assert k1 is None
    loss.backward()
    for name, x, y in zip(("means", "quats", "scales"), leaves, ref["aa" if aa else "plain"]):
        check_grad(x.grad, y, f"C={C} aa={aa} v_{name}")


@pytest.mark.parametrize("n", [0, 1, 255, 256, 257])
def test_operator_row_count_edges(dev, n):
    """Prefixes of the scene at the block and grid-stride edges; every row is projected on its own, so the reference of
    the whole scene, sliced, is the reference of the prefix."""
    ref = op_reference(3)
    leaves, (r1, m1, d1, c1, k1) = run_operator(dev, ref, n, True)
    r0, m0, d0, c0, k0 = (t[:, :n] for t in ref["out"])
    assert r1.shape == (3, n) and m1.shape == (3, n, 2) and k1.shape == (3, n)
    if n == 0:
        return
    assert torch.equal(r1.cpu(), r0)
    ok = r0 > 0
    if n > 1:
        assert int(ok.sum()) > 0
    assert float(((m1.detach().cpu() - m0.float()).abs() / (1 + m0.float().abs())).max()) < 1e-5
    for a, b, tol in ((d1, d0, 1e-6), (c1, c0, 1e-5), (k1, k0, 1e-5)):
        assert float(a.detach().cpu()[~ok].abs().max() if (~ok).any() else 0.0) == 0.0
        if ok.any():
            assert rel_l2(a.cpu()[ok], b[ok]) < tol
    sum((a * v[:, :n].to(dev)).sum() for a, v in zip((m1, d1, c1, k1), ref["cot"])).backward()
    for name, x, y in zip(("means", "quats", "scales"), leaves, ref["aa"]):
        check_grad(x.grad, y[:n], f"N={n} v_{name}")


# ------------------------------------------------------------------------------------------------ 2. operator forms
@pytest.mark.parametrize("name", ["large", "near"])
def test_packed_and_visibility_radii(dev, name):
    from clm_gs_amd import gsplat as G
    s = ortho_scene(name)
    w, h = s["width"], s["height"]
    vms = torch.stack([s["viewmat"], s["viewmat"]])
    vms[1, 0, 3] -= 1.0
    Ks = torch.stack([s["K"]] * 2)
    with torch.no_grad():
        r0, m0, d0, c0, k0 = R.projection(s["means"].double(), s["quats"].double(), s["scales"].double(), vms.double(),
                                          Ks.double(), w, h)
    cam0, gid0 = torch.nonzero(r0 > 0, as_tuple=True)
    assert cam0.numel() > 500 and int((r0 == 0).sum()) > 0
    a = [t.to(dev) for t in (s["means"], s["quats"], s["scales"], vms, Ks)]
    out = G.fully_fused_projection(a[0], None, *a[1:], w, h, packed=True, calc_compensations=True, camera_model="ortho")
    assert torch.equal(out[0].cpu(), cam0) and torch.equal(out[1].cpu(), gid0)
    assert torch.equal(out[2].cpu(), r0[cam0, gid0])
    assert float(((out[3].cpu() - m0[cam0, gid0].float()).abs() / (1 + m0[cam0, gid0].float().abs())).max()) < 1e-5
    assert rel_l2(out[4].cpu(), d0[cam0, gid0]) < 1e-6 and rel_l2(out[5].cpu(), c0[cam0, gid0]) < 1e-5
    assert rel_l2(out[6].cpu(), k0[cam0, gid0]) < 1e-5
    assert G.fully_fused_projection(a[0], None, *a[1:], w, h, packed=True, camera_model="ortho")[6] is None
    rad = G.visibility_radii(*a, w, h, camera_model="ortho")
    assert torch.equal(rad.cpu(), r0)
    with pytest.raises(NotImplementedError):
        G.visibility_radii(*a, w, h, camera_model="ortho", raw=True)


def test_default_is_pinhole_and_bad_models_raise(dev):
    from clm_gs_amd import gsplat as G
    s = small_scene(n=6000, width=200, height=120, seed=1, spread=3.0, depth=5.0)
    a = [t.to(dev) for t in (s["means"], s["quats"], s["scales"], s["viewmat"][None], s["K"][None])]
    for aa in (False, True):
        x = G.fully_fused_projection(a[0], None, *a[1:], 200, 120, calc_compensations=aa)
        y = G.fully_fused_projection(a[0], None, *a[1:], 200, 120, calc_compensations=aa, camera_model="pinhole")
        for p, q in zip(x, y):
            assert (p is None and q is None) or torch.equal(p, q)
    r0, m0, d0, c0, _ = O.fully_fused_projection(s["means"].double(), None, s["quats"].double(), s["scales"].double(),
                                                 s["viewmat"].double()[None], s["K"].double()[None], 200, 120)
    ok = r0 > 0
    assert torch.equal(x[0].cpu(), r0) and rel_l2(x[3].cpu()[ok], c0[ok]) < 1e-5
    assert torch.equal(G.visibility_radii(*a, 200, 120), G.visibility_radii(*a, 200, 120, camera_model="pinhole"))
    assert torch.equal(G.visibility_radii(*a, 200, 120).cpu(), r0)
    assert not torch.equal(G.visibility_radii(*a, 200, 120, camera_model="ortho").cpu(), r0)
    for bad in ("fisheye", "Ortho", None):
        with pytest.raises(ValueError):
            G.fully_fused_projection(a[0], None, *a[1:], 200, 120, camera_model=bad)
        with pytest.raises(ValueError):
            G.visibility_radii(*a, 200, 120, camera_model=bad)
    vm = a[3].clone().requires_grad_()
    with pytest.raises(NotImplementedError):
        G.fully_fused_projection(a[0], None, a[1], a[2], vm, a[4], 200, 120, camera_model="ortho")


# ------------------------------------------------------------------------------------------------ 3. camera_forward_ops
def _leaves64(s):
    return [s[k].double().clone().requires_grad_() for k in ("means", "opac", "scales", "quats", "shs")]


def _forward_ops(dev, s, render_mode, train=False, viewmat=None):
    from clm_gs_amd.strategies.base_engine import camera_forward_ops
    p = [s[k].clone().to(dev).requires_grad_(train) for k in ("means", "quats", "scales", "opac", "shs")]
    vm = (s["viewmat"] if viewmat is None else viewmat).to(dev)
    centre = torch.inverse(vm[None])[:, None, :3, 3]
    out = camera_forward_ops(p[0], p[1], p[2], p[3], p[4][None], 3, vm, s["K"].to(dev), centre, None, render_mode,
                             train=train, camera_model="ortho")
    return p, out


@pytest.mark.parametrize("mode", ["classic", "antialiased"])
@pytest.mark.parametrize("name", ["first", "small"])
def test_camera_forward_ops_against_the_composition(dev, name, mode):
    from clm_gs_amd import utils
    s = ortho_scene(name)
    w, h = s["width"], s["height"]
    utils.set_args(utils.default_args(rasterize_mode=mode))
    utils.set_img_size(h, w)
    try:
        L = _leaves64(s)
        img0, al0, ed0 = R.render(*L, 3, s["viewmat"].double(), s["K"].double(), w, h, antialiased=mode == "antialiased",
                                  depth=True)
        assert float(al0.detach().max()) > 0.3, "the camera sees the scene (0.47 on the small-scale scene under antialiasing)"
        with torch.no_grad():
            _, (img1, _, radii, extra, _) = _forward_ops(dev, s, "RGB")
            assert extra == ()
            check_image(img1, img0, f"{name} {mode} RGB")
            _, (img2, _, _, (ed2, al2), _) = _forward_ops(dev, s, "RGB+ED")
        check_image(img2, img0, f"{name} {mode} RGB+ED image")
        check_image(al2[0], al0, f"{name} {mode} alpha")
        # the blended depth channel D = ED * alpha at the image tolerance scaled by the channel's range
        zmax = float((s["viewmat"][:3, :3] @ s["means"].T)[2].max() + s["viewmat"][2, 3])
        eD = float((ed2[0].cpu().double() * al2[0].cpu().double() - ed0.detach() * al0.detach()).abs().max())
        print(f"{name} {mode}: accumulated depth max-abs {eD:.3g} (bound {IMG_TOL * zmax:.3g})")
        assert eD <= IMG_TOL * zmax
        # gradients under a random image cotangent
        g = torch.Generator().manual_seed(11)
        cot = torch.randn(3, h, w, generator=g)
        (img0 * cot.double()).sum().backward()
        p, (img3, m2d, _, _, _) = _forward_ops(dev, s, "RGB", train=True)
        (img3 * cot.to(dev)).sum().backward()
        assert m2d.grad is not None
        for pname, x, y in (("means", p[0], L[0]), ("quats", p[1], L[3]), ("scales", p[2], L[2]), ("opacities", p[3], L[1]),
                            ("shs", p[4], L[4])):
            check_grad(x.grad, y.grad, f"{name} {mode} v_{pname}")
    finally:
        utils.set_args(utils.default_args())


def test_view_direction_is_the_axis(dev):
    """Moving the camera 3 units back along its axis: one direction, the same x, y, depths shifted alike -- the image
    stays.  With means - centre directions (gsplat's) it would not."""
    from clm_gs_amd import utils
    s = ortho_scene("first")
    w, h = s["width"], s["height"]
    utils.set_args(utils.default_args())
    utils.set_img_size(h, w)
    back = s["viewmat"].clone()
    back[2, 3] += 3.0
    with torch.no_grad():
        L = [t.detach() for t in _leaves64(s)]
        per_row = []
        for vm in (s["viewmat"].double(), back.double()):
            dirs = L[0][None] - torch.inverse(vm[None])[:, None, :3, 3]
            per_row.append(R.render(*L, 3, vm, s["K"].double(), w, h, dirs=dirs)[0])
        assert float((per_row[0] - per_row[1]).abs().max()) > 1e-3, "precondition: means - centre directions do move the image"
        a = _forward_ops(dev, s, "RGB")[1][0]
        b = _forward_ops(dev, s, "RGB", viewmat=back)[1][0]
    e = float((a - b).abs().max())
    print(f"camera moved 3 units up its axis: RGB max-abs {e:.3g}")
    assert e <= IMG_TOL
    check_image(b, R.render(*L, 3, back.double(), s["K"].double(), w, h)[0], "shifted camera against the composition")


def test_ortho_sky_is_refused(dev):
    from clm_gs_amd import utils
    from clm_gs_amd.cameras import OrthoCamera
    from clm_gs_amd.strategies.base_engine import camera_forward_ops
    s = ortho_scene("first")
    utils.set_args(utils.default_args())
    utils.set_img_size(s["height"], s["width"])
    cam = OrthoCamera(0, s["viewmat"], PPU, s["width"], s["height"], image_name="sky_ortho")
    cam.sky = torch.zeros(8, 16, 3, device=dev)
    p = [s[k].to(dev) for k in ("means", "quats", "scales", "opac", "shs")]
    with pytest.raises(ValueError, match="sky_ortho"):
        camera_forward_ops(p[0], p[1], p[2], p[3], p[4][None], 3, s["viewmat"].to(dev), cam.K, None, None, "RGB",
                           train=False, sky_camera=cam, camera_model="ortho")


# ------------------------------------------------------------------------------------------------ 4. engines
EW, EH, EN = 96, 64, 3000
STRATEGIES = (("no_offload", "hbm"), ("naive_offload", "hbm"), ("clm_offload", "hbm"), ("clm_offload", "host"))


def _engine_args(strategy, residency="hbm"):
    from clm_gs_amd import utils
    args = utils.default_args(bsz=4, sh_residency=residency)
    setattr(args, strategy, True)
    utils.set_args(args)
    utils.set_img_size(EH, EW)
    utils.set_cur_iter(1)
    return args


def _model(strategy, sc, rendering=True):
    if strategy == "clm_offload":
        from clm_gs_amd.strategies.clm_offload import GaussianModelCLMOffload as M
    elif strategy == "no_offload":
        from clm_gs_amd.strategies.no_offload import GaussianModelNoOffload as M
    else:
        from clm_gs_amd.strategies.naive_offload import GaussianModelNaiveOffload as M
    m = M(3, only_for_rendering=rendering)
    m.create_from_tensors(sc["xyz"].clone(), sc["shs48"].clone(), sc["scaling"].clone(), sc["rotation"].clone(),
                          sc["opacity"].clone(), spatial_lr_scale=1.0)
    m.active_sh_degree = 3
    return m


def _down_camera(sc, ortho=True):
    from clm_gs_amd.cameras import Camera, OrthoCamera
    Rm = torch.tensor([[1.0, 0, 0], [0, -1.0, 0], [0, 0, -1.0]])
    C = torch.tensor([1.5, -2.0, 0.1 * sc["extent"] + 5.0])
    w2c = torch.eye(4)
    w2c[:3, :3] = Rm
    w2c[:3, 3] = -Rm @ C
    if ortho:
        return OrthoCamera(7, w2c, 2.0, EW, EH, image_name="ortho_down")
    return Camera(8, w2c, 1.1, 0.8, EW, EH)


def test_engines_eval_entries(dev):
    from clm_gs_amd import utils
    from clm_gs_amd.render_trajectory import eval_one_cam
    from clm_gs_amd.synthetic import synth_gaussians
    try:
        _engine_args("no_offload")
        sc = synth_gaussians(EN, seed=0, device="cuda")
        cam = _down_camera(sc)
        P = [sc[k].detach().cpu().double() for k in ("xyz", "opacity", "scaling", "rotation", "shs48")]
        with torch.no_grad():
            img0, al0, _ = R.render(P[0], torch.sigmoid(P[1]), torch.exp(P[2]), torch.nn.functional.normalize(P[3]),
                                    P[4].reshape(-1, 16, 3), 3, cam.world_view_transform.t().cpu().double(),
                                    cam.K.cpu().double(), EW, EH, depth=False)
        assert float(al0.max()) > 0.9 and float(al0.mean()) > 0.3
        got = {}
        for strategy, residency in STRATEGIES:
            args = _engine_args(strategy, residency)
            m = _model(strategy, sc)
            with torch.no_grad():
                img, depth, alpha = eval_one_cam(cam, m, None, args, render_mode="RGB+ED")
                rgb = eval_one_cam(cam, m, None, args)
            assert img.shape == (3, EH, EW) and depth.shape == (1, EH, EW) and alpha.shape == (1, EH, EW)
            check_image(img, img0, f"{strategy}/{residency} image")
            check_image(alpha[0], al0, f"{strategy}/{residency} alpha")
            check_image(rgb, img0, f"{strategy}/{residency} RGB")
            got[(strategy, residency)] = (img.clone(), depth.clone(), alpha.clone())
        first = got[STRATEGIES[0]]
        for key, val in got.items():
            for a, b in zip(val, first):
                assert float((a - b).abs().max()) < 1e-4, key
    finally:
        utils.set_args(utils.default_args())


def test_mixed_batch_and_training_entries_refuse(dev):
    from clm_gs_amd import contribution, fused, utils
    from clm_gs_amd.strategies.base_engine import calculate_filters, fov_camera, select_filters
    from clm_gs_amd.strategies.naive_offload import naive_offload_train_one_batch
    from clm_gs_amd.synthetic import synth_gaussians
    try:
        args = _engine_args("clm_offload")
        sc = synth_gaussians(EN, seed=0, device="cuda")
        m = _model("clm_offload", sc)
        ortho, pin = _down_camera(sc), _down_camera(sc, ortho=False)
        small = (m.get_xyz, m.get_opacity, m.get_scaling, m.get_rotation)
        with pytest.raises(ValueError, match="mixes"):
            calculate_filters([ortho, pin], *small)
        with pytest.raises(ValueError, match="mixes"):
            calculate_filters([pin, ortho], *small)
        f_o = calculate_filters([ortho, ortho], *small)[0]
        f_p = calculate_filters([pin], *small)[0]
        assert torch.equal(f_o[0], f_o[1]) and not torch.equal(f_o[0], f_p[0])
        with pytest.raises(ValueError, match="ortho_down"):
            select_filters([pin, ortho], m._xyz.detach(), m._scaling.detach(), m._rotation.detach())
        with pytest.raises(ValueError, match="ortho_down"):
            fused.camera_front(m, ortho, None, None, 1, None, None)
        with pytest.raises(ValueError, match="ortho_down"):
            contribution.score_cameras(m, [pin, ortho])
        _engine_args("naive_offload")
        with pytest.raises(ValueError, match="ortho_down"):
            naive_offload_train_one_batch(_model("naive_offload", sc), None, [pin, ortho], None)
        utils.set_img_size(EH + 16, EW)  # an orthographic camera of another size than the global image is refused
        with pytest.raises(ValueError, match="ortho_down"):
            fov_camera(ortho, dev)
    finally:
        utils.set_args(utils.default_args())


# ------------------------------------------------------------------------------------------------ 5. mosaic
UP = (0.0, 0.0, -1.0)  # the scene lies in front of a camera looking along +z: "up" is -z, the map camera looks along +z
GSD = 0.1


def _mosaic_setup(path=None):
    """small_scene(n=400, 64x64) as a no_offload model (optionally saved as a .ply and loaded back)."""
    from clm_gs_amd import utils
    from clm_gs_amd.strategies.no_offload import GaussianModelNoOffload
    args = utils.default_args(bsz=4)
    args.no_offload = True
    utils.set_args(args)
    utils.set_img_size(64, 64)
    s = small_scene(n=400, width=64, height=64)
    m = GaussianModelNoOffload(3, only_for_rendering=True)
    m.create_from_tensors(s["means"].cuda(), s["shs"].reshape(-1, 48).cuda(), torch.log(s["scales"]).cuda(),
                          s["quats"].cuda(), torch.logit(s["opac"]).cuda(), spatial_lr_scale=1.0)
    m.active_sh_degree = 3
    if path is not None:
        m.save_ply(path)
        m = GaussianModelNoOffload(3, only_for_rendering=True)
        m.load_ply(path)
        m.active_sh_degree = 3
    return args, m


def _geometry(m, bounds):
    from clm_gs_amd.render_ortho import MapGeometry, default_camera_height, map_frame
    frame = map_frame(UP)
    return MapGeometry(frame, bounds, GSD, default_camera_height(m.get_xyz.detach(), frame))


def _one_shot(geo, m, args, w, h, background=None):
    from clm_gs_amd import utils
    from clm_gs_amd.render_ortho import render_window
    utils.set_img_size(h, w)
    with torch.no_grad():
        img, ed, al = render_window(geo.camera(0, 0, w, h), m, background, args)
    return img.permute(1, 2, 0).cpu().numpy(), ed.cpu().numpy(), al.cpu().numpy()


def test_mosaic_against_one_render(dev):
    from clm_gs_amd import utils
    from clm_gs_amd.render_ortho import render_mosaic
    try:
        args, m = _mosaic_setup()
        geo = _geometry(m, (-3.2, -3.2, 3.2, 3.2))
        assert (geo.width, geo.height) == (64, 64)
        rgb, height, alpha = render_mosaic(m, geo, args, tile=32)  # four windows
        one, ed, al = _one_shot(geo, m, args, 64, 64)
        assert float(al.max()) > 0.9 and 0.05 < float((al >= 0.5).mean()) < 0.999
        check_image(torch.from_numpy(rgb), torch.from_numpy(one), "four windows against one render")
        check_image(torch.from_numpy(alpha), torch.from_numpy(al), "alpha, four windows against one render")
        # height = camera_height - expected depth where alpha >= 0.5, NaN elsewhere.  ED = D / alpha with D at the image
        # tolerance scaled by the depth range and alpha >= 0.5 (and not within the tolerance of the threshold)
        solid = (al >= 0.5 + IMG_TOL) & (alpha >= 0.5)
        empty = (al < 0.5 - IMG_TOL) & (alpha < 0.5)
        assert np.isnan(height[empty]).all() and np.isfinite(height[solid]).all() and int(solid.sum()) > 100
        zmax = float(ed[solid].max())
        eh = float(np.abs(height[solid] - (geo.camera_height - ed[solid])).max())
        print(f"height against camera_height - ED: max-abs {eh:.3g} (bound {4 * IMG_TOL * zmax:.3g})")
        assert eh <= 4 * IMG_TOL * zmax
        whole, h1, a1 = render_mosaic(m, geo, args, tile=64)  # one window: the same launch as the one-shot render
        assert np.array_equal(np.isnan(h1), a1 < 0.5)
        assert np.allclose(h1[a1 >= 0.5], (geo.camera_height - ed)[a1 >= 0.5], atol=4 * IMG_TOL * zmax)
        # a 70 x 50 map in 32-pixel windows = the crop of one 96 x 64 render
        geo2 = _geometry(m, (-3.5, -2.5, 3.5, 2.5))
        assert (geo2.width, geo2.height) == (70, 50)
        rgb2, _, alpha2 = render_mosaic(m, geo2, args, tile=32)
        one2, _, al2 = _one_shot(geo2, m, args, 96, 64)
        assert rgb2.shape == (50, 70, 3)
        check_image(torch.from_numpy(rgb2), torch.from_numpy(one2[:50, :70]), "70x50 in windows against the 96x64 crop")
        check_image(torch.from_numpy(alpha2), torch.from_numpy(al2[:50, :70]), "70x50 alpha")
        # a map placed off the scene: background, alpha 0, height NaN -- not an error
        geo3 = _geometry(m, (100.0, 100.0, 103.2, 101.6))
        for bg in (None, torch.tensor([1.0, 1.0, 1.0], device=dev)):
            rgb3, h3, a3 = render_mosaic(m, geo3, args, tile=32, background=bg)
            assert rgb3.shape == (16, 32, 3) and (rgb3 == (0.0 if bg is None else 1.0)).all()
            assert (a3 == 0).all() and np.isnan(h3).all()
        with pytest.raises(ValueError, match="multiple of 16"):
            render_mosaic(m, geo, args, tile=40)
    finally:
        utils.set_args(utils.default_args())


# ------------------------------------------------------------------------------------------------ 6. CLI
def test_cli_writes_the_four_files(dev, tmp_path):
    import json

    from clm_gs_amd import utils
    from clm_gs_amd.render_ortho import JSON_FIELDS, render_mosaic
    from clm_gs_amd.render_trajectory import read_png
    try:
        ply, out = str(tmp_path / "model.ply"), str(tmp_path / "out")
        args, m = _mosaic_setup(ply)
        geo = _geometry(m, (-3.5, -2.5, 3.5, 2.5))
        from clm_gs_amd.render_ortho import main
        with pytest.raises(SystemExit, match="multiple of 16"):  # refused before anything is loaded or written
            main(["-m", ply, "--no_offload", "--gsd", "0.1", "--tile", "40", "--output_dir", out])
        assert not os.path.exists(out)
        r = subprocess.run([sys.executable, "-m", "clm_gs_amd.render_ortho", "-m", ply, "--no_offload", "--gsd", str(GSD),
                            "--tile", "32", "--up", *map(str, UP), "--bounds", "-3.5", "-2.5", "3.5", "2.5",
                            "--output_dir", out], cwd=ROOT, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-2000:]
        rgb, height, alpha = render_mosaic(m, geo, args, tile=32, quantise=True)
        assert rgb.dtype == np.uint8 and rgb.shape == (50, 70, 3)
        assert np.array_equal(read_png(os.path.join(out, "ortho.png")), rgb)
        h = np.load(os.path.join(out, "ortho_height.npy"))
        a = np.load(os.path.join(out, "ortho_alpha.npy"))
        assert h.dtype == np.float32 and a.dtype == np.float32 and h.shape == a.shape == (50, 70)
        assert np.array_equal(h, height, equal_nan=True) and np.array_equal(a, alpha)
        d = json.load(open(os.path.join(out, "ortho.json")))
        assert sorted(d) == sorted(JSON_FIELDS) and (d["width"], d["height"], d["gsd"]) == (70, 50, GSD)
        assert abs(d["camera_height"] - geo.camera_height) < 1e-6 and np.allclose(d["origin"], geo.origin)
        assert np.allclose(d["up"], UP)
    finally:
        utils.set_args(utils.default_args())
