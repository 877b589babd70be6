"""Mesh export without a GPU ("Mesh export"): the topology of the numpy Surface Nets reference
(tests/tsdf_reference.py) on two analytic grids, the mesh .ply round trip, the sizing of tsdf.TsdfVolume's grid and the
refusals of the command line."""
import os

import numpy as np
import pytest

from tests import tsdf_reference as R

# (signed distance, V, F, Euler characteristic): grid 20^3, voxel 0.125
SHAPES = {"sphere": (R.sphere_sdf, 746, 1488, 2), "torus": (R.torus_sdf, 728, 1456, 0)}


@pytest.mark.parametrize("name", sorted(SHAPES))
def test_reference_topology_on_analytic_grids(name):
    sdf, V, F, euler = SHAPES[name]
    verts, colours, faces, cells = R.extract(R.grid_from_sdf(sdf()), 2.0, R.G2W)
    assert verts.dtype == np.float32 and colours.dtype == np.uint8 and faces.dtype == np.int32
    assert (len(verts), len(faces)) == (V, F) and colours.shape == (V, 3)
    t = R.check_closed_surface(verts, faces, cells, R.G2W, euler)
    print(name, t)
    # the surface is where it should be: every vertex within a voxel's diagonal of the zero set
    x, y, z = verts[:, 0].astype(np.float64), verts[:, 1].astype(np.float64), verts[:, 2].astype(np.float64)
    d = np.sqrt(x * x + y * y + z * z) - 0.8 if name == "sphere" else \
        np.sqrt((np.sqrt(x * x + y * y) - 0.75) ** 2 + z * z) - 0.3
    assert np.abs(d).max() < 0.5 * R.VOXEL
    # colours follow the position (grid_from_sdf: 0.5 + 0.4 coordinate), to the interpolation error of a voxel
    assert np.abs(colours.astype(np.float64) / 255.0 - np.clip(0.5 + 0.4 * verts, 0, 1)).max() < 0.4 * R.VOXEL + 1 / 255


@pytest.mark.parametrize("name", sorted(SHAPES))
def test_unseen_interior_gives_the_same_mesh(name):
    sdf = SHAPES[name][0]()
    trunc = 1.75 * R.VOXEL  # above a cell's diagonal (1.732 voxels): no voxel of an active cell is unseen; 56 torus voxels are
    full = R.extract(R.grid_from_sdf(sdf, trunc=trunc), 2.0, R.G2W)
    holed = R.grid_from_sdf(sdf, unseen_interior=True, trunc=trunc)
    assert int((holed[1] == 0).sum()) > 0
    seen = R.extract(holed, 2.0, R.G2W)
    assert (len(full[0]), len(full[2])) == SHAPES[name][1:3]
    for a, b in zip(full, seen):
        assert np.array_equal(a, b)


def test_reference_edge_cases():
    g = R.grid_from_sdf(R.sphere_sdf())
    g[0] = np.abs(g[0]) + 1  # all outside
    v, c, f, _ = R.extract(g, 2.0, R.G2W)
    assert v.shape == (0, 3) and c.shape == (0, 3) and f.shape == (0, 3)
    g = R.grid_from_sdf(R.sphere_sdf())
    v, c, f, _ = R.extract(g, 4.0, R.G2W)  # nothing is valid
    assert len(v) == 0 and len(f) == 0
    # a voxel without colour contributes grey
    g = R.grid_from_sdf(R.sphere_sdf(), colour=False)
    _, c, _, _ = R.extract(g, 2.0, R.G2W)
    assert (c == 128).all()


def test_reference_integration_of_one_pixel_camera():
    """The update rule on numbers that can be checked by hand: an orthogonal-looking camera down the z axis of a 2x2x4
    grid whose single pixel covers everything, surface at depth 2.25, trunc 1."""
    cams = np.array([[1e-3, 0, 0, -1e-3, 0, 1e-3, 0, -1e-3, 0, 0, 1, 0, 1, 1, 0.5, 0.5]], dtype=np.float64)
    depth = np.full((1, 1, 1), 2.25, dtype=np.float32)
    alpha = np.ones((1, 1, 1), dtype=np.float32)
    rgb = np.array([0.25, 2.0, -1.0], dtype=np.float32).reshape(1, 3, 1, 1)
    g0 = np.zeros((6, 4, 2, 2), dtype=np.float32)
    g, band = R.integrate(g0, cams, depth, alpha, rgb, 0.01, 100.0, 0.5, 1.0)
    # z = k + 0.5 -> sdf = 1.75, 0.75, -0.25, -1.25: far in front (tsum 1, no colour), in the band twice, behind
    assert np.array_equal(g[0][:, 0, 0], np.array([1.0, 0.75, -0.25, 0.0], dtype=np.float32))
    assert np.array_equal(g[1][:, 0, 0], np.array([1.0, 1.0, 1.0, 0.0], dtype=np.float32))
    assert np.array_equal(g[5][:, 0, 0], np.array([0.0, 1.0, 1.0, 0.0], dtype=np.float32))
    assert np.array_equal(g[2:5, 1, 1, 1], np.array([0.25, 1.0, 0.0], dtype=np.float32))
    assert not band.any() and not g0.any()
    for kw in (dict(alpha_min=1.5), dict(depth_max=2.0), dict(near=5.0)):
        args = dict(near=0.01, depth_max=100.0, alpha_min=0.5, trunc=1.0)
        args.update(kw)
        assert not R.integrate(g0, cams, depth, alpha, rgb, **args)[0].any(), kw
    twice, _ = R.integrate(g, cams, depth, alpha, rgb, 0.01, 100.0, 0.5, 1.0)
    assert np.array_equal(twice, 2 * g)


def test_mesh_ply_round_trip(tmp_path):
    from clm_gs_amd import io_ply
    verts, colours, faces, _ = R.extract(R.grid_from_sdf(R.sphere_sdf()), 2.0, R.G2W)
    path = str(tmp_path / "mesh.ply")
    io_ply.save_mesh_ply(path, verts, colours, faces)
    head = open(path, "rb").read(400).decode("latin1")
    assert head.startswith("ply\nformat binary_little_endian 1.0\nelement vertex 746\n")
    for line in ("property float x", "property uchar red", "property uchar blue", "element face 1488",
                 "property list uchar int vertex_indices", "end_header"):
        assert line in head
    assert os.path.getsize(path) == head.index("end_header\n") + 11 + 746 * 15 + 1488 * 13
    v, c, f = io_ply.load_mesh_ply(path)
    assert v.dtype == np.float32 and c.dtype == np.uint8 and f.dtype == np.int32
    assert np.array_equal(v, verts) and np.array_equal(c, colours) and np.array_equal(f, faces)
    import torch
    io_ply.save_mesh_ply(path, torch.from_numpy(verts), torch.from_numpy(colours), torch.from_numpy(faces))  # tensors too
    assert np.array_equal(io_ply.load_mesh_ply(path)[2], faces)
    empty = str(tmp_path / "empty.ply")
    io_ply.save_mesh_ply(empty, np.zeros((0, 3), np.float32), np.zeros((0, 3), np.uint8), np.zeros((0, 3), np.int32))
    v, c, f = io_ply.load_mesh_ply(empty)
    assert v.shape == (0, 3) and c.shape == (0, 3) and f.shape == (0, 3)
    with pytest.raises(ValueError, match="outside"):
        io_ply.save_mesh_ply(empty, verts[:10], colours[:10], faces)
    model = str(tmp_path / "model.ply")  # the model functions are unchanged and refuse a mesh / are refused as one
    z = torch.zeros
    io_ply.save_ply(model, z(2, 3), z(2, 48), z(2, 1), z(2, 3), z(2, 4))
    with pytest.raises(ValueError, match="not a mesh"):
        io_ply.load_mesh_ply(model)


def test_volume_sizing():
    from clm_gs_amd import tsdf
    assert tsdf.grid_shape((0, 0, 0, 10, 5, 2.5), 0.25) == (40, 20, 10)
    assert tsdf.grid_shape((0, 0, 0, 10, 5, 2.6), 0.25) == (40, 20, 11)       # a started voxel counts
    assert tsdf.grid_shape((-1, -1, -1, 1, 1, -0.99), 1.0) == (2, 2, 2)      # 2 at the least
    assert tsdf.grid_shape((0, 0, 0, 0.3, 0.3, 0.3), 0.1) == (3, 3, 3)       # 0.3 / 0.1 = 2.9999999999999996
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="--voxel"):
            tsdf.grid_shape((0, 0, 0, 1, 1, 1), bad)
    for bounds in ((0, 0, 0, 1, 1, 0), (0, 0, 0, -1, 1, 1), (0, 2, 0, 1, 1, 1), (0, 0, 0, 1, 1)):
        with pytest.raises(ValueError, match="--bounds"):
            tsdf.grid_shape(bounds, 0.1)
    assert tsdf.check_grid((0, 0, 0, 100, 100, 25), 0.1, grid_gb=16) == (1000, 1000, 250)  # 6 GB
    with pytest.raises(ValueError) as e:
        tsdf.check_grid((0, 0, 0, 100, 100, 25), 0.1, grid_gb=1)
    msg = str(e.value)
    assert "--grid_gb 1" in msg and "1000 x 1000 x 250" in msg and "fits" in msg
    fit = float(msg.split("; --voxel ")[1].split()[0])
    nx, ny, nz = tsdf.check_grid((0, 0, 0, 100, 100, 25), fit, grid_gb=1)  # the voxel it names does fit ...
    assert nx * ny * nz * 24 <= 1e9 and 0.1 < fit < 0.2                  # ... and is not far off (the cube root is 0.182)
    with pytest.raises(ValueError, match="2\\^31 voxels"):
        tsdf.check_grid((0, 0, 0, 2000, 2000, 1000), 1.0, grid_gb=1000)
    frame = (np.array([0.0, 1.0, 0.0]), np.array([-1.0, 0.0, 0.0]), np.array([0.0, 0.0, 1.0]))
    g = tsdf.grid_to_world(frame, (1.0, 2.0, 3.0, 5.0, 6.0, 7.0), 0.5)
    p = g @ np.array([0.5, 0.5, 0.5, 1.0])  # voxel (0, 0, 0): map coordinates (1.25, 2.25, 3.25)
    assert np.allclose(p, 1.25 * frame[0] + 2.25 * frame[1] + 3.25 * frame[2])
    p = g @ np.array([2.5, 0.5, 4.5, 1.0])
    assert np.allclose(p, 2.25 * frame[0] + 2.25 * frame[1] + 5.25 * frame[2])


def test_camera_record_composes_in_float64():
    from types import SimpleNamespace
    from clm_gs_amd import tsdf
    w2c = np.eye(4, dtype=np.float32)
    w2c[:3, 3] = (1.0, 2.0, 3.0)
    K = np.array([[100.0, 0, 32.0], [0, 110.0, 24.0], [0, 0, 1]], dtype=np.float32)
    cam = SimpleNamespace(_clmgs_host=(w2c.reshape(16), K.reshape(9), None), image_name="c")
    g2w = tsdf.grid_to_world((np.eye(3)[0], np.eye(3)[1], np.eye(3)[2]), (0, 0, 0, 1, 1, 1), 0.25)
    rec = tsdf.camera_record(cam, g2w)
    assert rec.dtype == np.float64 and rec.shape == (16,)
    assert np.allclose(rec[:12].reshape(3, 4), [[0.25, 0, 0, 1], [0, 0.25, 0, 2], [0, 0, 0.25, 3]])
    assert list(rec[12:]) == [100.0, 110.0, 32.0, 24.0]
    with pytest.raises(ValueError, match="orthographic"):
        tsdf.camera_record(SimpleNamespace(camera_model="ortho", image_name="o"), g2w)


def test_cli_refusals_come_before_anything_is_loaded(tmp_path):
    from clm_gs_amd import mesh_model
    out = tmp_path / "out"
    base = ["-m", str(tmp_path / "no_such_model.ply"), "-s", str(tmp_path / "no_such_scene"), "-o", str(out / "mesh.ply")]
    box = ["--bounds", "0", "0", "0", "100", "100", "25"]
    for extra, match in ((["--voxel", "0"], "--voxel must be positive"),
                         (["--voxel", "-0.5"], "--voxel must be positive"),
                         (["--voxel", "0.1", "--bounds", "0", "0", "0", "1", "-1", "1"], "--bounds"),
                         (["--voxel", "0.1", "--grid_gb", "1"] + box, "--grid_gb 1; --voxel 0.18"),
                         (["--voxel", "0.001", "--grid_gb", "1e6"] + box, "2\\^31 voxels; --voxel"),
                         (["--voxel", "0.1", "--min_weight", "0"], "--min_weight"),
                         (["--voxel", "0.1", "--every", "0"], "--every"),
                         (["--voxel", "0.1", "--up", "0", "0", "0"], "--up")):
        with pytest.raises(SystemExit, match=match):
            mesh_model.main(base + extra)
        assert not out.exists()


def test_trainer_refuses_a_bad_mesh_voxel_by_name():
    from clm_gs_amd import trainer, utils
    assert trainer.mesh_rules(utils.default_args()) == []  # off by default
    rules = trainer.mesh_rules(utils.default_args(mesh_voxel=-1.0))
    assert any(r and "--mesh_voxel must be positive" in m for r, m in rules)
    rules = trainer.mesh_rules(utils.default_args(mesh_voxel=0.1, mesh_min_weight=0.0))
    assert any(r and "--mesh_min_weight" in m for r, m in rules)
    assert not any(r for r, _ in trainer.mesh_rules(utils.default_args(mesh_voxel=0.1)))
    ns = trainer.build_arg_parser().parse_args(["-s", "a", "-m", "b", "--mesh_voxel", "0.25"])
    assert trainer.train_kwargs(ns)["mesh_voxel"] == 0.25
    assert trainer.train_kwargs(trainer.build_arg_parser().parse_args(["-s", "a", "-m", "b"]))["mesh_voxel"] == 0.0
