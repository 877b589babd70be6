"""CPU-only: the ray depth.  clm_gs_amd/csrc/ray_math.h (compiled with plain g++) against its numpy restatement
tests/ray_depth_reference.py bit for bit; the fallbacks; closed forms; the tilted plane and its derived bound; the render
mode and the four command lines."""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import torch

from tests import ray_depth_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def shim():
    out = os.path.join("/tmp", f"ray_math_shim_{os.getpid()}.so")
    subprocess.check_call(["g++", "-O2", "-shared", "-fPIC", "-I", os.path.join(ROOT, "clm_gs_amd", "csrc"),
                           os.path.join(ROOT, "tests", "host_shim", "ray_math_shim.cpp"), "-o", out])
    return ctypes.CDLL(out)


def run_shim(shim, mu, q, s, cam, px, py, ortho, near, centre):
    n = mu.shape[0]
    arrs = [np.ascontiguousarray(np.broadcast_to(a, shape), dtype=np.float64)
            for a, shape in ((mu, (n, 3)), (q, (n, 4)), (s, (n, 3)), (cam, (n, 16)), (px, (n,)), (py, (n,)))]
    centre = np.ascontiguousarray(np.broadcast_to(centre, (n,)), dtype=np.float32)
    t, d = np.empty(n, dtype=np.float64), np.empty(n, dtype=np.float32)
    P = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    shim.shim_ray_depth(n, *(P(a) for a in arrs), ctypes.c_int(int(ortho)), ctypes.c_double(near), P(centre), P(t), P(d))
    return t, d


def f32(a):
    return np.asarray(a, dtype=np.float32).astype(np.float64)


def random_rotations(rng, n):
    q = rng.normal(size=(n, 4))
    return np.stack([np.stack(R.quat_to_rotmat(qi)).reshape(3, 3) for qi in q])


def random_case(seed, n_cams=8, rows=400):
    """Per camera: a random rigid view matrix and intrinsics, rows in front of it with scales 1e-6 .. 1e2 and unnormalised
    quaternions, random pixels: everything a float32 value widened.  -> list of (cam [16], mu, q, s, px, py, centre)."""
    rng = np.random.default_rng(seed)
    cases = []
    for Rv in random_rotations(rng, n_cams):
        t = rng.normal(size=3) * 2.0
        cam = f32(np.concatenate([np.concatenate([Rv, t[:, None]], 1).reshape(12), rng.uniform(30, 2000, 2),
                                  rng.uniform(0, 64, 2)]))
        m_cam = rng.normal(size=(rows, 3)) * np.array([2.0, 2.0, 1.5]) + np.array([0.0, 0.0, 6.0])
        mu = f32((m_cam - t) @ Rv)  # Rv mu + t = m_cam
        q = f32(rng.normal(size=(rows, 4)) * 10.0 ** rng.uniform(-1, 1, (rows, 1)))
        s = f32(10.0 ** rng.uniform(-6, 2, (rows, 3)))
        px, py = rng.integers(0, 64, rows).astype(np.float64), rng.integers(0, 48, rows).astype(np.float64)
        centre = rng.uniform(0.5, 10.0, rows).astype(np.float32)
        cases.append((cam, mu, q, s, px, py, centre))
    return cases


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    nan = np.isnan(a)
    kind = {4: np.int32, 8: np.int64}[a.dtype.itemsize]
    return np.array_equal(nan, np.isnan(b)) and np.array_equal(a[~nan].view(kind), b[~nan].view(kind))


# ------------------------------------------------------------------------------------------------ 1. shim against reference
@pytest.mark.parametrize("ortho", [False, True])
def test_shim_matches_the_reference_bit_for_bit(shim, ortho):
    used = fell_back = 0
    for cam, mu, q, s, px, py, centre in random_case(3 if ortho else 2):
        t_ref = R.ray_tstar(mu, q, s, cam, px, py, ortho)
        d_ref = R.ray_depth(mu, q, s, cam, px, py, ortho, 0.01, centre)
        t, d = run_shim(shim, mu, q, s, cam, px, py, ortho, 0.01, centre)
        assert same_bits(t, t_ref) and same_bits(d, d_ref)
        used += int((d != centre).sum())
        fell_back += int((d == centre).sum())
    print(f"ortho={ortho}: {used} ray depths, {fell_back} fallbacks")
    assert used > 1000  # the cases exercise the formula, not the fallback


# ------------------------------------------------------------------------------------------------ 2. fallbacks
def test_fallbacks_return_the_centre_depth_bit_for_bit(shim):
    cam = R.pinhole_record()
    mu, q, s = np.array([[0.3, -0.2, 4.0]]), np.array([[0.9, 0.1, -0.3, 0.2]]), np.array([[0.3, 0.2, 0.05]])
    centre = np.array([4.0000005], dtype=np.float32)
    px, py = np.array([40.0]), np.array([20.0])
    ok = R.ray_depth(mu, q, s, cam, px, py, False, 0.01, centre)
    assert ok[0] != centre[0] and abs(float(ok[0]) - 4.0) < 0.5  # the baseline is a ray depth, not a fallback
    cases = {}
    for j in range(3):
        z = s.copy(); z[0, j] = 0.0
        cases[f"zero scale {j}"] = dict(s=z)
    cases["all scales zero"] = dict(s=np.zeros((1, 3)))
    cases["all scales infinite"] = dict(s=np.full((1, 3), np.inf))
    cases["behind the near plane"] = dict(mu=np.array([[0.3, -0.2, -4.0]]))
    cases["maximum below near"] = dict(near=100.0)
    cases["zero quaternion"] = dict(q=np.zeros((1, 4)))
    for name, arr, width in (("mu", mu, 3), ("q", q, 4), ("s", s, 3)):
        for j in range(width):
            bad = arr.copy(); bad[0, j] = np.nan
            cases[f"NaN {name}[{j}]"] = {name: bad}
    for j in range(3):
        bad = mu.copy(); bad[0, j] = np.inf
        cases[f"inf mu[{j}]"] = dict(mu=bad)
    bad = q.copy(); bad[0, 2] = -np.inf
    cases["inf q"] = dict(q=bad)
    for k in (0, 3, 11, 12, 15):
        bad = cam.copy(); bad[k] = np.nan
        cases[f"NaN cam[{k}]"] = dict(cam=bad)
    bad = cam.copy(); bad[12] = 0.0
    cases["fx = 0"] = dict(cam=bad)
    for ortho in (False, True):
        for what, kw in cases.items():
            a = dict(mu=mu, q=q, s=s, cam=cam, near=0.01)
            a.update(kw)
            for c in (centre, np.array([np.float32(0.0)]), np.array([np.float32(-3.25)])):  # handed back, whatever it is
                ref = R.ray_depth(a["mu"], a["q"], a["s"], a["cam"], px, py, ortho, a["near"], c)
                _, got = run_shim(shim, a["mu"], a["q"], a["s"], a["cam"], px, py, ortho, a["near"], c)
                assert same_bits(ref, c) and same_bits(got, c), (what, ortho, ref, got)


# ------------------------------------------------------------------------------------------------ 3. closed forms
def test_closed_forms(shim):
    rng = np.random.default_rng(11)
    n = 500
    cam = R.pinhole_record()
    px, py = rng.integers(0, R.W, n).astype(np.float64), rng.integers(0, R.H, n).astype(np.float64)
    d = np.stack([(px + 0.5 - cam[14]) / cam[12], (py + 0.5 - cam[15]) / cam[13], np.ones(n)], -1)
    mu = f32(rng.normal(size=(n, 3)) * np.array([1.0, 1.0, 0.5]) + np.array([0.0, 0.0, 5.0]))
    q = f32(rng.normal(size=(n, 4)))
    s = f32(10.0 ** rng.uniform(-3, 0, (n, 3)))
    # isotropic: S is a multiple of the identity, t* = d.m / d.d whatever the rotation
    iso = np.repeat(s[:, :1], 3, axis=1)
    t = R.ray_tstar(mu, q, iso, cam, px, py, False)
    want = (d * mu).sum(-1) / (d * d).sum(-1)
    print(f"isotropic: max relative deviation {np.abs(t / want - 1).max():.2e}")
    assert np.abs(t / want - 1).max() < 1e-12
    # the centre on the pixel's ray: the maximum is the centre, whatever the shape
    z = rng.uniform(1.0, 9.0, n)
    on_ray = d * z[:, None]
    t = R.ray_tstar(on_ray, q, s, cam, px, py, False)
    print(f"centre on the ray: max relative deviation {np.abs(t / z - 1).max():.2e}")
    assert np.abs(t / z - 1).max() < 1e-9  # flat and oblique: g.g and g.p each carry the 1e6 spread of 1 / s^2
    # a common factor 2 on the scales (exact in binary) changes no bit: reference and shim
    t1, t2 = R.ray_tstar(mu, q, s, cam, px, py, False), R.ray_tstar(mu, q, 2.0 * s, cam, px, py, False)
    assert same_bits(t1, t2)
    a, _ = run_shim(shim, mu, q, s, cam, px, py, False, 0.01, np.float32(1.0))
    b, _ = run_shim(shim, mu, q, 2.0 * s, cam, px, py, False, 0.01, np.float32(1.0))
    assert same_bits(a, b) and same_bits(a, t1)
    # orthographic camera, axis-aligned Gaussian: the ray runs along a principal axis, t* = m_z wherever the pixel is
    ident = np.broadcast_to(np.array([1.0, 0.0, 0.0, 0.0]), (n, 4))
    t = R.ray_tstar(mu, ident, s, R.ortho_record(), px, py, True)
    assert np.abs(t / mu[:, 2] - 1).max() < 1e-15
    half_turn = np.broadcast_to(np.array([0.0, 3.0, 0.0, 0.0]), (n, 4))  # about x, unnormalised: still axis-aligned
    t = R.ray_tstar(mu, half_turn, s, R.ortho_record(), px, py, True)
    assert np.abs(t / mu[:, 2] - 1).max() < 1e-15


# ------------------------------------------------------------------------------------------------ 4. the tilted plane
@pytest.mark.parametrize("ortho", [False, True])
def test_tilted_plane_ray_depth_lies_on_the_plane(ortho):
    """Every Gaussian whose footprint holds the pixel (in-plane offset of the ray's hit <= FOOT s), at every pixel: the ray
    depth lies within GEOM of the Gaussian's own plane (the exact inequality (1) of the reference's docstring, plus 1e-12
    for float64 rounding) and within GEOM + PLACE of the analytic plane; the centre depth misses the analytic plane by more
    than 100 x that bound."""
    cam = R.ortho_record() if ortho else R.pinhole_record()
    xyz, quats, scales, n_cam, c0 = R.plane_rows()
    bnd, geom, place = R.bound(cam, ortho, n_cam, xyz, quats, scales, n_cam, c0)
    hit = R.plane_hit(cam, ortho, n_cam, c0)                                   # [H,W]
    assert abs(hit[R.H // 2, R.W // 2] - R.PLANE_DEPTH) < 0.05
    o, d = R.pixel_rays(cam, ortho)
    mu, q, s = xyz.astype(np.float64), quats.astype(np.float64), scales.astype(np.float64)
    Rm = np.stack(R.quat_to_rotmat(q[0])).reshape(3, 3)                        # the rows share one float32 quaternion
    n_own = Rm[:, 2]
    assert np.abs(n_own - n_cam).max() < 1e-7
    worst_ray = worst_own = worst_centre = 0.0
    held = 0
    py, px = np.meshgrid(np.arange(R.H, dtype=np.float64), np.arange(R.W, dtype=np.float64), indexing="ij")
    for i in range(mu.shape[0]):
        t_own = ((mu[i] - o) @ n_own) / (d @ n_own)                            # the ray's hit on this Gaussian's own plane
        h = o + t_own[..., None] * d - mu[i]
        inside = np.sqrt((h * h).sum(-1)) <= R.FOOT * R.S_TANGENT
        if not inside.any():
            continue
        t = R.ray_tstar(mu[i], q[i], s[i], cam, px, py, ortho)
        held += int(inside.sum())
        worst_own = max(worst_own, float(np.abs(t - t_own)[inside].max()))
        worst_ray = max(worst_ray, float(np.abs(t - hit)[inside].max()))
        worst_centre = max(worst_centre, float(np.abs(mu[i] @ np.array([0.0, 0.0, 1.0]) - hit)[inside].max()))
        got32 = R.ray_depth(mu[i], q[i], s[i], cam, px, py, ortho, 0.01, np.float32(mu[i][2]))
        assert (got32[inside] == t.astype(np.float32)[inside]).all()           # none of them falls back
    print(f"ortho={ortho}: bound {bnd:.3e} (GEOM {geom:.3e} + PLACE {place:.3e}); {held} (pixel, Gaussian) pairs; ray depth "
          f"misses its own plane by {worst_own:.3e}, the analytic plane by {worst_ray:.3e}; the centre depth by {worst_centre:.3e}")
    assert held > 25 * R.W * R.H  # pi (FOOT s)^2 / SPACING^2 = 32 Gaussians hold a pixel
    assert worst_own <= geom + 1e-12
    assert worst_ray <= bnd
    assert worst_centre > 100 * bnd


def test_best_matching_gaussian_reproduces_the_measured_figures():
    """The prototype's selection: per pixel the Gaussian nearest the ray in its own metric.  Its centre depth misses the
    plane by some cm, its ray depth by the float32 placement of the rows."""
    cam = R.pinhole_record()
    xyz, quats, scales, n_cam, c0 = R.plane_rows()
    bnd, _, _ = R.bound(cam, False, n_cam, xyz, quats, scales, n_cam, c0)
    hit = R.plane_hit(cam, False, n_cam, c0)
    o, d = R.pixel_rays(cam, False)
    mu = xyz.astype(np.float64)
    point = o + hit[..., None] * d                                             # where the ray meets the plane
    dist = np.linalg.norm(point[:, :, None, :] - mu[None, None], axis=-1)      # in-plane: the metric is isotropic there
    ids = dist.argmin(-1).astype(np.int32)
    centre = xyz[:, 2][ids][None]
    viewmat, K = np.eye(4, dtype=np.float32)[None], np.array([[[R.FOCAL, 0, R.W / 2], [0, R.FOCAL, R.H / 2], [0, 0, 1]]])
    ray = R.ray_depth_map(xyz, quats, scales, viewmat, K, centre, ids[None])[0]
    e_ray, e_centre = np.abs(ray.astype(np.float64) - hit).max(), np.abs(centre[0].astype(np.float64) - hit).max()
    print(f"best match: centre depth misses the plane by {e_centre:.3e}, ray depth by {e_ray:.3e} (bound {bnd:.3e})")
    assert e_ray <= bnd + 2.0 ** -22 * 7.0  # the float32 rounding of a depth below 8 on top
    assert e_centre > 100 * bnd and e_centre > 0.04


# ------------------------------------------------------------------------------------------------ 5. mode plumbing
def test_render_mode_is_known():
    from clm_gs_amd.strategies import base_engine as B
    assert "RGB+RD" in B.RENDER_MODES and "RGB+XD" not in B.RENDER_MODES
    col, bg = torch.rand(1, 5, 3), torch.rand(1, 3)
    c2, b2 = B.colors_with_depth(col, torch.rand(1, 5), bg, "RGB+RD")  # no fourth colour, the backgrounds as they are
    assert c2 is col and b2 is bg and c2.shape[-1] == 3
    with pytest.raises(ValueError, match="RGB\\+RD"):
        B.refuse_median_training("RGB+RD", "training entry")
    with pytest.raises(ValueError, match="RGB\\+MD"):
        B.refuse_median_training("RGB+MD", "training entry")
    B.refuse_median_training("RGB+ED", "training entry")
    with pytest.raises(ValueError, match="render_mode must be one of"):
        B.colors_with_depth(col, torch.rand(1, 5), bg, "RGB+XD")


def test_binding_table_and_header_carry_the_entry():
    from clm_gs_amd import _lib
    assert "clmgs_ray_depth" in _lib.SIGNATURES
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), "clmgs_ray_depth")


def test_command_lines_accept_ray_and_refuse_before_anything_is_loaded(tmp_path):
    from clm_gs_amd import mesh_model, render_ortho, render_trajectory, trainer, utils
    missing, out = str(tmp_path / "no_model"), tmp_path / "out"
    assert render_trajectory.depth_render_mode("ray") == "RGB+RD"
    # mesh_model
    mesh_model.check_options(0.1, depth_mode="ray")
    with pytest.raises(ValueError, match="--depth_mode"):
        mesh_model.check_options(0.1, depth_mode="rays")
    with pytest.raises(SystemExit, match="--depth_mode"):
        mesh_model.main(["-m", missing, "-s", missing, "-o", str(out / "mesh.ply"), "--voxel", "0.1", "--depth_mode", "mode7"])
    # render_trajectory: accepted with --render_depth, refused by name without it
    render_trajectory.check_depth_options(True, "ray")
    with pytest.raises(ValueError, match="--depth_mode ray has effect only with --render_depth"):
        render_trajectory.check_depth_options(False, "ray")
    with pytest.raises(SystemExit, match="--depth_mode ray has effect only with --render_depth"):
        render_trajectory.main(["-m", missing, "--output_dir", str(out), "--depth_mode", "ray"])
    # render_ortho: the parser takes the mode, and an unknown one is refused before the model is looked for
    with pytest.raises(SystemExit, match="--depth_mode"):
        render_ortho.main(["-m", missing, "--output_dir", str(out), "--gsd", "0.1", "--depth_mode", "mode7"])
    render_trajectory.depth_render_mode("ray", flag="--depth_mode")
    # trainer
    rules = trainer.mesh_rules(utils.default_args(mesh_depth_mode="ray"))
    assert any(r and "--mesh_depth_mode ray has effect only with --mesh_voxel" in m for r, m in rules)
    assert not any(r for r, _ in trainer.mesh_rules(utils.default_args(mesh_voxel=0.1, mesh_depth_mode="ray")))
    rules = trainer.mesh_rules(utils.default_args(mesh_voxel=0.1, mesh_depth_mode="mode7"))
    assert any(r and "--mesh_depth_mode must be one of" in m for r, m in rules)
    with pytest.raises(ValueError, match="--mesh_depth_mode ray has effect only with --mesh_voxel"):
        trainer.main(["-s", missing, "-m", str(out), "--mesh_depth_mode", "ray"])
    ns = trainer.build_arg_parser().parse_args(["-s", "a", "-m", "b", "--mesh_voxel", "0.25", "--mesh_depth_mode", "ray"])
    assert trainer.train_kwargs(ns)["mesh_depth_mode"] == "ray"
    assert not out.exists()
    utils.set_args(utils.default_args())
