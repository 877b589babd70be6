"""Mesh smoothing and vertex normals without a GPU ("Mesh smoothing and normals"): the numpy
restatement of the contract (tests/mesh_smooth_reference.py) on the analytic grids of tests/tsdf_reference.py -- what the
smoothing does to a noisy sphere, measured against the analytic surface, which assumes nothing about the code under test
-- the vertex and face rules, the .ply layouts, the refusals of every entry before anything is read, and the records."""
import json
import struct

import numpy as np
import pytest

from tests import mesh_smooth_reference as S
from tests import tsdf_reference as R

_MESHES = {}


def mesh(name):
    """(verts, colours, faces) of an analytic 20^3 grid, extracted once."""
    if name not in _MESHES:
        sdf = dict(sphere=R.sphere_sdf, torus=R.torus_sdf)[name]()
        _MESHES[name] = R.extract(R.grid_from_sdf(sdf), 2.0, R.G2W)[:3]
    return _MESHES[name]


def noisy_sphere():
    verts, colours, faces = mesh("sphere")
    noise = np.random.default_rng(7).normal(0.0, 0.02, size=verts.shape)
    return (verts.astype(np.float64) + noise).astype(np.float32), colours, faces


def radius(v):
    return np.linalg.norm(np.asarray(v, dtype=np.float64), axis=1)


# ------------------------------------------------------------------------------------------------ the two forms agree
def test_vectorised_form_equals_the_loops_bit_for_bit():
    for verts, colours, faces in (noisy_sphere(), mesh("torus")):
        lists = S.incidence(faces, len(verts))
        for c in (0.5, -0.53):
            assert np.array_equal(S.smooth_step(verts, faces, c, lists), S.smooth_step_loop(verts, faces, c, lists))
        assert np.array_equal(S.vertex_normals(verts, faces, lists), S.vertex_normals_loop(verts, faces, lists))
    verts, colours, faces = noisy_sphere()
    a = S.smooth(verts, colours, faces, 2)[0]
    b = S.smooth(verts, colours, faces, 2, step=S.smooth_step_loop)[0]
    assert a.dtype == np.float32 and np.array_equal(a, b) and not np.array_equal(a, verts)


def test_incidence_lists():
    faces = np.array([[2, 0, 1], [0, 2, 3], [3, 3, 0]], dtype=np.int32)
    order, start = S.incidence(faces, 6)
    assert order.dtype == np.int64 and start.dtype == np.int64
    assert order.tolist() == [1, 3, 8, 2, 0, 4, 5, 6, 7]  # faces ascending, then corners; vertex 3 twice from face 2
    assert start.tolist() == [0, 3, 4, 6, 9, 9, 9]


# ------------------------------------------------------------------------------------------------ normals
def test_sphere_normals_are_unit_and_radial():
    verts, colours, faces = mesh("sphere")
    assert (len(verts), len(faces)) == (746, 1488)
    n = S.vertex_normals(verts, faces)
    assert n.dtype == np.float32 and n.shape == verts.shape
    length = np.linalg.norm(n.astype(np.float64), axis=1)
    radial = verts.astype(np.float64) / radius(verts)[:, None]
    dot = (n.astype(np.float64) * radial).sum(axis=1)
    print(f"sphere normals: |n| - 1 max {np.abs(length - 1).max():.2e}, normal . radial min {dot.min():.4f}")
    assert np.abs(length - 1).max() <= 1e-6
    assert dot.min() >= 0.99


def test_torus_normals_are_unit():
    verts, colours, faces = mesh("torus")
    length = np.linalg.norm(S.vertex_normals(verts, faces).astype(np.float64), axis=1)
    assert np.abs(length - 1).max() <= 1e-6


# ------------------------------------------------------------------------------------------------ smoothing
def test_taubin_removes_noise_and_keeps_the_volume():
    verts, colours, faces = noisy_sphere()
    t_in = R.topology(verts, faces)
    v, c, f, rep = S.smooth(verts, colours, faces, 10)
    assert c is colours and f is faces and v.dtype == np.float32 and v.shape == verts.shape
    assert rep == dict(iterations=10, lam=0.5, mu=-0.53, vertices=746, faces=1488, vertices_fixed=0)
    assert tuple(rep) == S.REPORT_KEYS
    t = R.topology(v, faces)
    std_in, std_out = radius(verts).std(), radius(v).std()
    print(f"noisy sphere: radius std {std_in:.4f} -> {std_out:.4f} ({std_out / std_in:.2f} x) after 10 passes, "
          f"{radius(S.smooth(verts, colours, faces, 5)[0]).std():.4f} after 5; volume {t_in['volume']:.3f} -> "
          f"{t['volume']:.3f} ({100 * (t['volume'] / t_in['volume'] - 1):+.1f} %)")
    assert std_out < 0.5 * std_in
    assert abs(t["volume"] / t_in["volume"] - 1) <= 0.02
    assert t["closed"] and t["oriented"] and t["euler"] == 2
    assert (t["closed"], t["oriented"], t["euler"], t["V"], t["F"]) == \
           (t_in["closed"], t_in["oriented"], t_in["euler"], t_in["V"], t_in["F"])


def test_plain_laplacian_shrinks():
    verts, colours, faces = noisy_sphere()
    v = S.smooth(verts, colours, faces, 20, lam=0.5, mu=0)[0]
    print(f"noisy sphere: mean radius {radius(verts).mean():.3f} -> {radius(v).mean():.3f} after 20 plain steps")
    assert radius(v).mean() < 0.75 < radius(verts).mean()
    t = R.topology(v, faces)
    assert t["closed"] and t["oriented"] and t["euler"] == 2


# ------------------------------------------------------------------------------------------------ vertex and face rules
def test_unreferenced_vertex_keeps_its_bits_and_gets_the_zero_normal():
    verts = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0.123456789, -7.5, 3e-7], [0, 0, 1]], dtype=np.float32)
    faces = np.array([[0, 1, 2], [0, 2, 4]], dtype=np.int32)
    colours = np.zeros((5, 3), dtype=np.uint8)
    for step in (S.smooth_step, S.smooth_step_loop):
        v, c, f, rep = S.smooth(verts, colours, faces, 3, step=step)
        assert v[3].tobytes() == verts[3].tobytes() and not np.array_equal(v[0], verts[0])
        assert rep["vertices_fixed"] == 1
    for normals in (S.vertex_normals, S.vertex_normals_loop):
        n = normals(verts, faces)
        assert n[3].tolist() == [0.0, 0.0, 0.0]
        assert n[1].tolist() == [0.0, 0.0, 1.0] and n[4].tolist() == [1.0, 0.0, 0.0]  # one face each


def test_a_face_naming_a_vertex_twice_follows_the_contract():
    verts = np.array([[0, 0, 0], [1, 0, 0], [0, 2, 0], [0, 0, 4]], dtype=np.float32)
    faces = np.array([[0, 1, 2], [3, 3, 0], [1, 1, 1]], dtype=np.int32)
    order, start = S.incidence(faces, 4)
    assert order[start[3]:start[4]].tolist() == [3, 4] and order[start[1]:start[2]].tolist() == [1, 6, 7, 8]
    for step in (S.smooth_step, S.smooth_step_loop):
        v = step(verts, faces, 0.5)
        # vertex 3: entry (1,0) adds p3 and p0, entry (1,1) adds p0 and p3: the mean of (p3, p0, p0, p3), half way there
        assert v[3].tolist() == [0.0, 0.0, 3.0]
        # vertex 0: (0,0) adds p1, p2; (1,2) adds p3, p3: mean (1/4, 2/4, 8/4)
        assert v[0].tolist() == [0.125, 0.25, 1.0]
        # vertex 1: (0,1) adds p2, p0; the face (1,1,1) adds p1 six times: mean (6/8, 2/8, 0)
        assert v[1].tolist() == [0.875, 0.125, 0.0]
    for normals in (S.vertex_normals, S.vertex_normals_loop):
        n = normals(verts, faces)
        assert n[3].tolist() == [0.0, 0.0, 0.0]  # its only face has no area
        assert n[0].tolist() == [0.0, 0.0, 1.0] and n[1].tolist() == [0.0, 0.0, 1.0]


def test_zero_iterations_return_the_objects_passed_in():
    from clm_gs_amd import mesh_smooth
    a, b, c = object(), object(), object()
    for module in (S, mesh_smooth):
        out = module.smooth(a, b, c, 0)
        assert out[0] is a and out[1] is b and out[2] is c and out[3] is None
        out = module.smooth(a, b, c, 0, 0.3, 0)
        assert out[0] is a and out[3] is None
    assert mesh_smooth.REPORT_KEYS == S.REPORT_KEYS


# ------------------------------------------------------------------------------------------------ options
def test_options_are_refused_by_name():
    from clm_gs_amd import mesh_smooth
    assert mesh_smooth.check_options(3, 0.5, -0.53) == (3, 0.5, -0.53) and mesh_smooth.check_options() == (0, 0.5, -0.53)
    assert mesh_smooth.check_options(2, 1, -1) == (2, 1.0, -1.0) and mesh_smooth.check_options(2, 1e-3, 0) == (2, 0.001, 0.0)
    for bad in (-1, 1.5, "2", None, True, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="--smooth_iterations must be a non-negative integer"):
            mesh_smooth.check_options(bad)
        with pytest.raises(ValueError, match="iterations must be a non-negative integer"):
            mesh_smooth.smooth(None, None, None, bad)
    for bad in (0, 0.0, -0.5, 1.0001, float("nan"), float("inf"), "0.5", None, True):
        with pytest.raises(ValueError, match=r"--smooth_lambda must be a finite number in \(0, 1\]"):
            mesh_smooth.check_options(1, bad)
        with pytest.raises(ValueError, match=r"lam must be a finite number in \(0, 1\]"):
            mesh_smooth.smooth(None, None, None, 1, bad)
    for bad in (0.01, -1.0001, float("nan"), float("-inf"), "-0.5", None, True):
        with pytest.raises(ValueError, match=r"--smooth_mu must be a finite number in \[-1, 0\]"):
            mesh_smooth.check_options(1, 0.5, bad)
        with pytest.raises(ValueError, match=r"mu must be a finite number in \[-1, 0\]"):
            mesh_smooth.smooth(None, None, None, 0, 0.5, bad)  # (refused even when off)
    with pytest.raises(ValueError, match="--mesh_smooth_mu"):
        mesh_smooth.check_options(1, 0.5, 1, names=("--mesh_smooth_iterations", "--mesh_smooth_lambda", "--mesh_smooth_mu"))
    for bad in ((-1, 0.5, -0.53), (1, 2.0, -0.53), (1, 0.5, 0.5)):
        with pytest.raises(ValueError):
            S.smooth(*mesh("sphere"), *bad)


def test_refusals_come_before_any_path_is_touched(tmp_path):
    from clm_gs_amd import mesh_clean, mesh_model
    missing = str(tmp_path / "no_such_dir" / "mesh.ply")
    out = tmp_path / "out"
    for flag, bad, match in (("--smooth_iterations", "-1", "--smooth_iterations must be a non-negative integer"),
                             ("--smooth_lambda", "0", r"--smooth_lambda must be a finite number in \(0, 1\]"),
                             ("--smooth_lambda", "nan", "--smooth_lambda must be a finite number"),
                             ("--smooth_mu", "0.1", r"--smooth_mu must be a finite number in \[-1, 0\]"),
                             ("--smooth_mu", "-inf", "--smooth_mu must be a finite number")):
        with pytest.raises(SystemExit, match=match):
            mesh_clean.main(["-i", missing, "-o", str(out / "clean.ply"), "--smooth_iterations", "1", f"{flag}={bad}"])
        with pytest.raises(SystemExit, match=match):
            mesh_model.main(["-m", missing, "-s", missing, "-o", str(out / "mesh.ply"), "--voxel", "1", f"{flag}={bad}"])
        assert not out.exists()
    with pytest.raises(ValueError, match="--smooth_iterations"):
        mesh_model.check_options(0.1, smooth_iterations=-2)
    with pytest.raises(ValueError, match="--smooth_lambda"):
        mesh_model.check_options(0.1, smooth_iterations=1, smooth_lambda=1.5)
    with pytest.raises(ValueError, match="--smooth_mu"):
        mesh_model.check_options(0.1, smooth_mu=-2.0)
    mesh_model.check_options(0.1, smooth_iterations=5, smooth_lambda=0.3, smooth_mu=-0.31)
    # the positional callers of before: eleven arguments, `decimate_cell` the last
    mesh_model.check_options(0.1, None, 16.0, 4.0, 2.0, 1, "expected", 0, 0, False, 0.0)
    with pytest.raises(ValueError, match="--smooth_iterations"):  # before a camera or the model is looked at
        mesh_model.build_mesh(None, None, None, str(out / "mesh.ply"), 0.1, smooth_iterations=-1)
    with pytest.raises(ValueError, match="--smooth_mu"):
        mesh_model.build_mesh(None, None, None, str(out / "mesh.ply"), 0.1, smooth_mu=0.5, normals=True)
    assert not out.exists()


def test_clean_mesh_nothing_to_do():
    from clm_gs_amd import mesh_clean
    with pytest.raises(SystemExit, match=r"nothing to do: give --min_faces N, --keep_largest K, --decimate_cell C, "
                                         r"--smooth_iterations N or --normals"):
        mesh_clean.main(["-i", "no_such.ply", "-o", "no_such_out.ply"])
    with pytest.raises(SystemExit, match="nothing to do"):  # the factors alone do nothing
        mesh_clean.main(["-i", "no_such.ply", "-o", "no_such_out.ply", "--smooth_iterations", "0", "--smooth_lambda", "0.3"])
    for flags in (["--smooth_iterations", "2"], ["--normals"]):  # accepted: the next thing that fails is the missing file
        with pytest.raises(FileNotFoundError):
            mesh_clean.main(["-i", "no_such.ply", "-o", "no_such_out.ply"] + flags)


# ------------------------------------------------------------------------------------------------ the file
def _todays_bytes(verts, colours, faces):
    """The layout of the mesh .ply before normals existed, assembled by hand."""
    head = ("ply\nformat binary_little_endian 1.0\nelement vertex %d\nproperty float x\nproperty float y\nproperty float z\n"
            "property uchar red\nproperty uchar green\nproperty uchar blue\nelement face %d\n"
            "property list uchar int vertex_indices\nend_header\n" % (len(verts), len(faces))).encode("ascii")
    body = b"".join(struct.pack("<3f3B", *map(float, v), *map(int, c)) for v, c in zip(verts, colours))
    return head + body + b"".join(struct.pack("<B3i", 3, *map(int, f)) for f in faces)


def test_ply_without_normals_is_byte_for_byte_the_file_of_before(tmp_path):
    from clm_gs_amd import io_ply
    verts, colours, faces = mesh("sphere")
    a, b = str(tmp_path / "a.ply"), str(tmp_path / "b.ply")
    io_ply.save_mesh_ply(a, verts, colours, faces)  # the call of before: no keyword
    io_ply.save_mesh_ply(b, verts, colours, faces, normals=None)
    assert open(a, "rb").read() == open(b, "rb").read() == _todays_bytes(verts, colours, faces)
    out = io_ply.load_mesh_ply(a)
    assert len(out) == 3 and all(np.array_equal(x, y) for x, y in zip(out, (verts, colours, faces)))
    out = io_ply.load_mesh_ply(a, with_normals=True)
    assert len(out) == 4 and out[3] is None and all(np.array_equal(x, y) for x, y in zip(out[:3], (verts, colours, faces)))


def test_ply_round_trip_with_normals(tmp_path):
    from clm_gs_amd import io_ply
    verts, colours, faces = mesh("sphere")
    normals = S.vertex_normals(verts, faces)
    path = str(tmp_path / "n.ply")
    io_ply.save_mesh_ply(path, verts, colours, faces, normals=normals)
    raw = open(path, "rb").read()
    head = raw[:raw.index(b"end_header\n")].decode().split("\n")
    assert [l.split()[-1] for l in head if l.startswith("property") and "list" not in l] == \
           ["x", "y", "z", "nx", "ny", "nz", "red", "green", "blue"]
    assert len(raw) == raw.index(b"end_header\n") + 11 + len(verts) * 27 + len(faces) * 13
    out = io_ply.load_mesh_ply(path)
    assert len(out) == 3 and all(np.array_equal(x, y) for x, y in zip(out, (verts, colours, faces)))
    v, c, f, n = io_ply.load_mesh_ply(path, with_normals=True)
    assert n.dtype == np.float32 and np.array_equal(n, normals) and np.array_equal(v, verts) and np.array_equal(f, faces)
    import torch
    io_ply.save_mesh_ply(str(tmp_path / "t.ply"), torch.from_numpy(verts), torch.from_numpy(colours), torch.from_numpy(faces),
                         torch.from_numpy(normals))
    assert open(tmp_path / "t.ply", "rb").read() == raw
    empty = str(tmp_path / "empty.ply")  # V = F = 0 with normals is a valid file too
    io_ply.save_mesh_ply(empty, verts[:0], colours[:0], faces[:0], normals[:0])
    assert [x.shape for x in io_ply.load_mesh_ply(empty, with_normals=True)] == [(0, 3)] * 4


def test_ply_refusals(tmp_path):
    from clm_gs_amd import io_ply
    verts, colours, faces = mesh("sphere")
    normals = S.vertex_normals(verts, faces)
    for bad in (normals[:-1], normals[:, :2], normals.reshape(-1), np.zeros((len(verts), 4), dtype=np.float32)):
        with pytest.raises(ValueError, match=r"save_mesh_ply: normals must be float32 \[746,3\]"):
            io_ply.save_mesh_ply(str(tmp_path / "bad.ply"), verts, colours, faces, bad)
    assert not (tmp_path / "bad.ply").exists()
    good = str(tmp_path / "n.ply")
    io_ply.save_mesh_ply(good, verts, colours, faces, normals)
    raw = open(good, "rb").read()
    three = b"property float nx\nproperty float ny\nproperty float nz\n"
    layouts = (raw.replace(b"property float nz\n", b""),                                        # two of three normals
               raw.replace(b"property float nx\n", b"property float u\n"),                     # another property
               raw.replace(three, b"").replace(b"property uchar blue\n", b"property uchar blue\n" + three),  # another order
               raw.replace(b"property uchar blue\n", b"property uchar blue\nproperty uchar alpha\n"))
    for k, data in enumerate(layouts):
        path = str(tmp_path / f"layout{k}.ply")
        assert data != raw
        open(path, "wb").write(data)
        for kw in ({}, dict(with_normals=True)):
            with pytest.raises(ValueError, match="not a mesh written by save_mesh_ply"):
                io_ply.load_mesh_ply(path, **kw)
    open(tmp_path / "short.ply", "wb").write(raw[:-13])  # one face short
    with pytest.raises(ValueError, match="truncated"):
        io_ply.load_mesh_ply(str(tmp_path / "short.ply"), with_normals=True)


# ------------------------------------------------------------------------------------------------ trainer and records
def test_trainer_options_reach_default_args_and_bad_values_are_refused(tmp_path):
    from clm_gs_amd import trainer, utils
    a = utils.default_args()
    assert (a.mesh_smooth_iterations, a.mesh_smooth_lambda, a.mesh_smooth_mu, a.mesh_normals) == (0, 0.5, -0.53, False)
    ap = trainer.build_arg_parser()
    kw = trainer.train_kwargs(ap.parse_args(["-s", "a", "-m", "b"]))
    assert (kw["mesh_smooth_iterations"], kw["mesh_smooth_lambda"], kw["mesh_smooth_mu"], kw["mesh_normals"]) == \
           (0, 0.5, -0.53, False)
    kw = trainer.train_kwargs(ap.parse_args(["-s", "a", "-m", "b", "--mesh_voxel", "0.25", "--mesh_smooth_iterations", "7",
                                             "--mesh_smooth_lambda", "0.4", "--mesh_smooth_mu", "-0.42", "--mesh_normals"]))
    assert (kw["mesh_smooth_iterations"], kw["mesh_smooth_lambda"], kw["mesh_smooth_mu"], kw["mesh_normals"]) == \
           (7, 0.4, -0.42, True)
    b = utils.default_args(**{k: v for k, v in kw.items() if hasattr(a, k)})
    assert (b.mesh_smooth_iterations, b.mesh_smooth_lambda, b.mesh_smooth_mu, b.mesh_normals) == (7, 0.4, -0.42, True)
    assert trainer.mesh_rules(utils.default_args()) == []
    assert trainer.mesh_rules(utils.default_args(mesh_smooth_lambda=0.3, mesh_smooth_mu=-0.3)) == []  # factors alone: off
    assert not any(r for r, _ in trainer.mesh_rules(utils.default_args(mesh_voxel=0.1, mesh_smooth_iterations=3,
                                                                       mesh_normals=True)))
    for over, flag in ((dict(mesh_smooth_iterations=3), "--mesh_smooth_iterations"), (dict(mesh_normals=True), "--mesh_normals")):
        rules = trainer.mesh_rules(utils.default_args(**over))
        assert any(r and f"{flag} has effect only with --mesh_voxel: give both, or neither" in m for r, m in rules), rules
        with pytest.raises(ValueError, match=f"{flag} has effect only with --mesh_voxel"):
            trainer.train_from_colmap(str(tmp_path / "no_such_scene"), str(tmp_path / "out"), **over)
        assert not (tmp_path / "out").exists()
    for over, match in ((dict(mesh_smooth_iterations=-1), "--mesh_smooth_iterations must be a non-negative integer"),
                        (dict(mesh_smooth_iterations=1.5), "--mesh_smooth_iterations must be a non-negative integer"),
                        (dict(mesh_smooth_lambda=0.0), r"--mesh_smooth_lambda must be a finite number in \(0, 1\]"),
                        (dict(mesh_smooth_lambda=float("nan")), "--mesh_smooth_lambda must be a finite number"),
                        (dict(mesh_smooth_mu=0.2), r"--mesh_smooth_mu must be a finite number in \[-1, 0\]"),
                        (dict(mesh_smooth_mu=float("-inf")), "--mesh_smooth_mu must be a finite number")):
        for voxel in (0.0, 0.1):
            with pytest.raises(ValueError, match=match):
                trainer.check_training(utils.default_args(clm_offload=True, mesh_voxel=voxel, **over))
        with pytest.raises(ValueError, match=match):  # the source directory does not exist
            trainer.train_from_colmap(str(tmp_path / "no_such_scene"), str(tmp_path / "out"), mesh_voxel=0.1, **over)
        assert not (tmp_path / "out").exists()


def test_json_record_and_log_words():
    from clm_gs_amd import mesh_smooth
    meta = dict(voxel=0.5, vertices=746, faces=1488, camera_names=["a", "b"])
    report = S.smooth(*noisy_sphere(), 2)[3]
    assert mesh_smooth.json_record(meta) == meta and mesh_smooth.json_record(meta) is not meta
    out = mesh_smooth.json_record(meta, report, True)
    assert meta == dict(voxel=0.5, vertices=746, faces=1488, camera_names=["a", "b"])  # not modified
    assert out == dict(voxel=0.5, vertices=746, faces=1488, camera_names=["a", "b"], smoothing=report, normals=True)
    assert out["smoothing"] is not report and tuple(out["smoothing"]) == S.REPORT_KEYS
    assert json.loads(json.dumps(out)) == out
    assert mesh_smooth.json_record(meta, None, True) == dict(meta, normals=True)
    assert mesh_smooth.json_record(meta, report) == dict(meta, smoothing=report)
    assert mesh_smooth.log_words() == ""
    assert mesh_smooth.log_words(report) == " smoothed 2 x (0.5, -0.53)"
    assert mesh_smooth.log_words(None, True) == " normals"
    assert mesh_smooth.log_words(dict(report, mu=0.0), True) == " smoothed 2 x (0.5, 0) normals"
