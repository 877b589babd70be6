"""CPU-only: the orthographic camera model.  The float64 reference of tests/ortho_reference.py is held to its scenes'
preconditions and to the far-pinhole limit of the oracle's projection; the product's fp32 formulas
(clm_gs_amd/csrc/ortho_math.h, compiled with plain g++) to the reference; the map frame, the percentile bounds and the
metadata of clm_gs_amd.render_ortho to their definitions; the two new C entries to the binding table and the library."""
import ctypes
import json
import os
import subprocess

import numpy as np
import pytest
import torch

from oracle import gs_oracle as O
from tests import ortho_reference as R
from tests.scenes import rel_l2, small_scene

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GRAD_TOL = 2e-4  # tests/test_gpu_ops.py
NEW_SYMBOLS = ("clmgs_projection_ortho_fwd", "clmgs_projection_ortho_bwd")
PPU = 10.0  # pixels per world unit of every scene below

# scene arguments -> (visible, culled by the near plane, culled off-screen)
SCENES = {
    "first": ({}, (369, 0, 31)),
    "small": ({"log_scale": -3.5}, (348, None, None)),
    "near": ({"depth": 1.0}, (309, 78, 13)),
    "large": ({"n": 6000, "width": 200, "height": 120, "seed": 1, "spread": 3.0, "depth": 5.0}, (5589, None, None)),
}


def ortho_scene(name):
    s = small_scene(**SCENES[name][0])
    s["K"] = R.ortho_K(PPU, s["width"], s["height"])
    return s


def f64(s):
    leaves = [s[k].double().clone().requires_grad_() for k in ("means", "quats", "scales")]
    return leaves, s["viewmat"].double()[None], s["K"].double()[None]


@pytest.fixture(scope="module")
def shim():
    out = os.path.join("/tmp", f"ortho_math_shim_{os.getpid()}.so")
    subprocess.check_call(["g++", "-O2", "-shared", "-fPIC", "-I", os.path.join(ROOT, "clm_gs_amd", "csrc"),
                           os.path.join(ROOT, "tests", "host_shim", "ortho_math_shim.cpp"), "-o", out])
    return ctypes.CDLL(out)


def _P(t):
    return ctypes.c_void_p(t.data_ptr())


def shim_fwd(shim, s, near_plane=0.01):
    N, f = s["means"].shape[0], ctypes.c_float
    means, quats, scales = s["means"].contiguous(), s["quats"].contiguous(), s["scales"].contiguous()
    vm, K = s["viewmat"].contiguous(), s["K"].contiguous()
    radii = torch.zeros(N, dtype=torch.int32)
    m2, d, cn, comp = torch.zeros(N, 2), torch.zeros(N), torch.zeros(N, 3), torch.full((N,), float("nan"))
    shim.shim_project_ortho_fwd(N, _P(means), _P(quats), _P(scales), _P(vm), _P(K), f(s["width"]), f(s["height"]), f(0.3),
                                f(near_plane), f(1e10), f(0.0), _P(radii), _P(m2), _P(d), _P(cn), _P(comp))
    return radii, m2, d, cn, comp


def shim_bwd(shim, s, radii, vm2, vd, vc, vk):
    N, f = s["means"].shape[0], ctypes.c_float
    means, quats, scales = s["means"].contiguous(), s["quats"].contiguous(), s["scales"].contiguous()
    vm, K = s["viewmat"].contiguous(), s["K"].contiguous()
    vmn, vq, vs = torch.zeros(N, 3), torch.zeros(N, 4), torch.zeros(N, 3)
    shim.shim_project_ortho_bwd(N, _P(means), _P(quats), _P(scales), _P(vm), _P(K), f(0.3), _P(radii),
                                _P(vm2.contiguous()), _P(vd.contiguous()), _P(vc.contiguous()), _P(vk.contiguous()),
                                _P(vmn), _P(vq), _P(vs))
    return vmn, vq, vs


# ------------------------------------------------------------------------------------------------ (a) preconditions
@pytest.mark.parametrize("name", list(SCENES))
def test_scene_preconditions(name):
    s = ortho_scene(name)
    (m, q, sc), vm, K = f64(s)
    with torch.no_grad():
        vis, near, off = R.cull_reasons(m, q, sc, vm[0], K[0], s["width"], s["height"])
        r64 = R.projection(m, q, sc, vm, K, s["width"], s["height"])[0]
        r32 = R.projection(s["means"], s["quats"], s["scales"], s["viewmat"][None], s["K"][None], s["width"], s["height"])[0]
    print(f"scene {name}: visible {vis}, near plane {near}, off-screen {off}")
    want = SCENES[name][1]
    assert vis == want[0]
    if want[1] is not None:
        assert (near, off) == want[1:]
    assert torch.equal(r32, r64), "the float32 evaluation gives the float64 radii: bit-exact radii are a fair demand"


def test_pinhole_radii_differ():
    """A pinhole kernel cannot pass: with the scene's own K its radii differ in 316 of the 400 rows."""
    s = small_scene()
    (m, q, sc), vm, _ = f64(s)
    with torch.no_grad():
        rp = O.fully_fused_projection(m, None, q, sc, vm, s["K"].double()[None], s["width"], s["height"])[0]
        ro = R.projection(m, q, sc, vm, R.ortho_K(PPU, 64, 48, dtype=torch.float64)[None], s["width"], s["height"])[0]
    assert int((rp != ro).sum()) == 316


# ------------------------------------------------------------------------------------------------ (b) far-pinhole limit
def test_far_pinhole_limit():
    """A pinhole camera moved back by D along its axis with focal 10 (D + 6) converges to the orthographic one as 1/D."""
    s = ortho_scene("first")
    (m, q, sc), vm, K = f64(s)
    err = {}
    with torch.no_grad():
        ro, mo = R.projection(m, q, sc, vm, K, s["width"], s["height"])[:2]
        for D in (1e3, 1e5):
            vmD = vm.clone()
            vmD[0, 2, 3] += D
            f = PPU * (D + 6.0)
            KD = torch.tensor([[f, 0, s["width"] / 2.0], [0, f, s["height"] / 2.0], [0, 0, 1]], dtype=torch.float64)[None]
            rp, mp = O.fully_fused_projection(m, None, q, sc, vmD, KD, s["width"], s["height"])[:2]
            both = (rp[0] > 0) & (ro[0] > 0)
            assert int(both.sum()) > 300
            err[D] = float((mp[0][both] - mo[0][both]).abs().max())
            print(f"D = {D:g}: max |means2d(pinhole) - means2d(ortho)| = {err[D]:.3g} px over {int(both.sum())} rows")
    assert err[1e5] < 0.01
    assert 50.0 <= err[1e3] / err[1e5] <= 200.0


# ------------------------------------------------------------------------------------------------ (c) product formulas
@pytest.mark.parametrize("name", list(SCENES))
def test_product_forward_against_the_reference(shim, name):
    s = ortho_scene(name)
    radii, m2, d, cn, comp = shim_fwd(shim, s)
    (m, q, sc), vm, K = f64(s)
    with torch.no_grad():
        r0, m0, d0, c0, k0 = R.projection(m, q, sc, vm, K, s["width"], s["height"])
    assert torch.equal(r0[0], radii)
    ok = radii > 0
    for t in (m2, d, cn, comp):
        assert float(t[~ok].abs().max()) == 0.0, "culled entries are zero"
    e_m = float(((m2.double() - m0[0]).abs() / (1 + m0[0].abs()))[ok].max())
    e_d = rel_l2(d[ok], d0[0][ok])  # the forms and bounds of tests/test_gpu_ops.py::test_projection_fwd_bwd
    e_c, e_k = rel_l2(cn[ok], c0[0][ok]), rel_l2(comp[ok], k0[0][ok])
    print(f"scene {name}: means2d {e_m:.3g}, depths {e_d:.3g}, conics {e_c:.3g}, compensations {e_k:.3g}")
    assert e_m < 1e-5 and e_d < 1e-6 and e_c < 1e-5 and e_k < 1e-5


@pytest.mark.parametrize("name", ["first", "small", "near"])
def test_product_vjp_against_the_reference(shim, name):
    s = ortho_scene(name)
    N = s["means"].shape[0]
    radii = shim_fwd(shim, s)[0]
    ok = radii > 0
    (m, q, sc), vm, K = f64(s)
    r0, m0, d0, c0, k0 = R.projection(m, q, sc, vm, K, s["width"], s["height"])
    g = torch.Generator().manual_seed(1)
    cot = dict(means2d=torch.randn(N, 2, generator=g), depth=torch.randn(N, generator=g),
               conic=torch.randn(N, 3, generator=g), compensation=torch.randn(N, generator=g))
    for what in ("all", "means2d", "depth", "conic", "compensation"):
        a2, ad, ac, ak = (cot[k] if what in ("all", k) else torch.zeros_like(cot[k])
                          for k in ("means2d", "depth", "conic", "compensation"))
        for t in (m, q, sc):
            t.grad = None
        ((m0[0] * a2.double()).sum() + (d0[0] * ad.double()).sum() + (c0[0] * ac.double()).sum()
         + (k0[0] * ak.double()).sum()).backward(retain_graph=True)
        vmn, vq, vs = shim_bwd(shim, s, radii, a2, ad, ac, ak)
        for pname, x, y in (("means", vmn, m.grad), ("quats", vq, q.grad), ("scales", vs, sc.grad)):
            if float(y.abs().max()) == 0.0:  # means2d / depth alone: no path to quats and scales
                assert float(x.abs().max()) == 0.0, (what, pname)
                continue
            e = rel_l2(x[ok], y[ok])
            print(f"scene {name}, cotangent {what}: v_{pname} rel_l2 {e:.3g}")
            assert e < GRAD_TOL, (what, pname, e)
        assert float(vmn[~ok].abs().max()) == 0.0


# ------------------------------------------------------------------------------------------------ (d) map frame
TILTED = (0.2, -0.3, 0.9)


@pytest.mark.parametrize("up,east", [((0, 0, 1), (1, 0, 0)), ((0, 1, 0), (1, 0, 0)), (TILTED, (1, 0, 0)),
                                     ((0, 0, 2), (0, 0, 5)), ((1, 0, 0), (1, 0, 0)), ((0, 1, 0), (0, -3, 0))])
def test_map_frame_is_orthonormal_and_right_handed(up, east):
    from clm_gs_amd.render_ortho import map_frame, world_to_cam
    e, n, u = map_frame(up, east)
    M = np.stack([e, n, u])
    assert np.allclose(M @ M.T, np.eye(3), atol=1e-12)
    assert np.allclose(np.cross(e, n), u, atol=1e-12) and abs(np.linalg.det(M) - 1.0) < 1e-12
    assert np.allclose(u, np.asarray(up, float) / np.linalg.norm(up), atol=1e-12)
    Rc = world_to_cam((e, n, u), 7.0)[:3, :3]
    assert np.allclose(Rc @ Rc.T, np.eye(3), atol=1e-12) and abs(np.linalg.det(Rc) - 1.0) < 1e-12
    assert np.allclose(Rc[2], -u), "the camera looks straight down"
    assert np.allclose(Rc[1], -n), "image row 0 is north"


@pytest.mark.parametrize("up", [(0, 0, 1), (0, 1, 0), TILTED])
def test_pixel_centre_round_trip_and_json(up, tmp_path):
    from clm_gs_amd.render_ortho import JSON_FIELDS, MapGeometry, map_frame, write_outputs
    from clm_gs_amd.render_trajectory import read_png
    geo = MapGeometry(map_frame(up), (-3.25, -1.5, 4.0, 2.75), 0.125, 9.0)
    assert (geo.width, geo.height) == (58, 34)
    cam = geo.camera(16, 16, 32, 32, device="cpu")
    assert cam.camera_model == "ortho" and (cam.image_width, cam.image_height) == (32, 32)
    vm, K = cam.world_view_transform.t().double()[None], cam.K.double()[None]
    px = [(c, r, h) for c in (0, 17, 57) for r in (0, 16, 33) for h in (0.0, 2.5)]
    world = torch.tensor(np.stack([geo.pixel_to_world(c, r, h) for c, r, h in px]))
    p = torch.einsum("ij,nj->ni", vm[0, :3, :3], world) + vm[0, :3, 3]
    got = torch.stack([K[0, 0, 0] * p[:, 0] + K[0, 0, 2], K[0, 1, 1] * p[:, 1] + K[0, 1, 2]], -1)
    want = torch.tensor([[c + 0.5 - 16, r + 0.5 - 16] for c, r, _ in px], dtype=torch.float64)
    assert float((got - want).abs().max()) < 1e-5
    assert np.allclose(p[:, 2].numpy(), [9.0 - h for _, _, h in px], atol=1e-6), "depth = camera_height - height"
    rgb = np.random.default_rng(0).integers(0, 256, (geo.height, geo.width, 3), dtype=np.uint8)
    hm = np.random.default_rng(1).random((geo.height, geo.width), dtype=np.float32)
    hm[0, 0] = np.nan
    write_outputs(str(tmp_path), geo, rgb, hm, hm * 0.5)
    d = json.load(open(tmp_path / "ortho.json"))
    assert sorted(d) == sorted(JSON_FIELDS)
    back = MapGeometry.from_json(d)
    assert (back.width, back.height, back.gsd, back.camera_height) == (geo.width, geo.height, geo.gsd, geo.camera_height)
    assert np.allclose(back.origin, geo.origin, atol=1e-12)
    for c, r in ((0, 0), (57, 33)):
        assert np.allclose(back.pixel_to_world(c, r), geo.pixel_to_world(c, r), atol=1e-9)
    assert np.allclose(d["origin"], geo.pixel_to_world(-0.5, -0.5), atol=1e-12), "origin = top-left pixel CORNER"
    assert np.array_equal(read_png(str(tmp_path / "ortho.png")), rgb)
    h2 = np.load(tmp_path / "ortho_height.npy")
    assert h2.dtype == np.float32 and np.array_equal(h2, hm, equal_nan=True)
    assert np.load(tmp_path / "ortho_alpha.npy").shape == (geo.height, geo.width)


def test_tile_must_be_a_multiple_of_16():
    from clm_gs_amd.render_ortho import check_tile
    assert check_tile(32) == 32 and check_tile(4096) == 4096
    for bad in (40, 0, -16, 8):
        with pytest.raises(ValueError):
            check_tile(bad)


# ------------------------------------------------------------------------------------------------ (e) percentiles
def test_percentile_bounds_match_numpy():
    from clm_gs_amd.render_ortho import map_frame, percentile_1d, percentile_bounds
    g = torch.Generator().manual_seed(0)
    for n in (1, 2, 7, 100, 1001):
        x = torch.randn(n, generator=g, dtype=torch.float64)
        for q in (0, 1, 37.5, 50, 99, 100):
            assert abs(percentile_1d(x, q) - float(np.percentile(x.numpy(), q))) < 1e-12, (n, q)
    means = torch.randn(500, 3, generator=g, dtype=torch.float64) * torch.tensor([5.0, 2.0, 1.0], dtype=torch.float64)
    frame = map_frame(TILTED, (1, 0.5, 0))
    emin, nmin, emax, nmax = percentile_bounds(means, frame)
    e, n, _ = frame
    ce, cn = means.numpy() @ e, means.numpy() @ n
    want = (np.percentile(ce, 1), np.percentile(cn, 1), np.percentile(ce, 99), np.percentile(cn, 99))
    assert np.allclose((emin, nmin, emax, nmax), want, atol=1e-12)


def test_percentile_accepts_more_than_2_24_points():
    from clm_gs_amd.render_ortho import percentile_1d
    n = (1 << 24) + 1
    x = torch.arange(n, dtype=torch.float32)
    x = x.flip(0).contiguous()
    assert percentile_1d(x, 50) == float(n - 1) / 2  # one sort; ordered input, the worst case of a selection


# ------------------------------------------------------------------------------------------------ (f) bindings
def test_bindings():
    from clm_gs_amd import _lib
    for name in NEW_SYMBOLS:
        assert name in _lib.SIGNATURES, name
    assert _lib.SIGNATURES["clmgs_projection_ortho_fwd"] == _lib.SIGNATURES["clmgs_projection_aa_fwd"]
    assert _lib.SIGNATURES["clmgs_projection_ortho_bwd"] == _lib.SIGNATURES["clmgs_projection_aa_bwd"]
    l = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert hasattr(l, name), name


def test_camera_model_reader_and_ortho_camera():
    from clm_gs_amd.cameras import Camera, OrthoCamera, camera_model, refuse_ortho
    w2c = torch.eye(4)
    w2c[:3, 3] = torch.tensor([0.5, -1.0, 4.0])
    o = OrthoCamera(3, w2c, (10.0, 12.0), 64, 48, device="cpu")
    assert camera_model(o) == "ortho" and camera_model(object()) == "pinhole"
    assert camera_model(Camera(0, w2c, 1.0, 0.8, 64, 48, device="cpu")) == "pinhole"
    assert torch.equal(o.K, torch.tensor([[10.0, 0, 32.0], [0, 12.0, 24.0], [0, 0, 1]]))
    assert torch.equal(o.world_view_transform, w2c.t()) and o.camtoworlds.shape == (1, 4, 4)
    vm, K, centre = o._clmgs_host
    assert np.array_equal(vm.reshape(4, 4), w2c.numpy()) and np.array_equal(K.reshape(3, 3), o.K.numpy())
    assert np.allclose(centre, [-0.5, 1.0, -4.0])
    far = OrthoCamera(4, w2c, 10.0, 64, 48, cx=-1000.0, cy=5000.0, device="cpu")  # a mosaic window: outside the image
    assert float(far.K[0, 2]) == -1000.0 and float(far.K[1, 2]) == 5000.0
    assert o.original_image is None
    with pytest.raises(ValueError, match="ortho_00003"):
        refuse_ortho(o, "here")
    with pytest.raises(ValueError):
        OrthoCamera(5, w2c, 0.0, 64, 48, device="cpu")
