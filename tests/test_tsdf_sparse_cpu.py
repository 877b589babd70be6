"""Sparse volume without a GPU ("Sparse volume"): the equality argument on the numpy restatements
(tests/tsdf_sparse_reference.py, tests/tsdf_reference.py) -- the marked bricks cover every voxel within 1 voxel of a voxel
with a negative term, and the dense grid restricted to them extracts the identical mesh -- the marked share of the sphere
scene, a nadir camera whose marked set can be written down, and the refusals of tsdf.SparseTsdfVolume, mesh_model --sparse
and trainer --mesh_sparse."""
import numpy as np
import pytest

from tests import tsdf_reference as R
from tests import tsdf_sparse_reference as SR


def test_marked_bricks_cover_the_dilated_negative_set():
    sc = SR.sphere_scene()
    marks, band, slabs, lo, hi = SR.scene_marks(sc)
    N = SR.scene_negative(sc)
    need = SR.dilate(N, 1)
    assert int(N.sum()) > 1000 and int(need.sum()) > int(N.sum())
    assert (SR.voxels(marks, sc["shape"]) | ~need).all()          # dilate(N, 1) is stored ...
    assert (SR.voxels(lo, sc["shape"]) | ~need).all()             # ... even with every box narrowed by the band
    assert (marks | ~lo).all() and (hi | ~marks).all()
    # a condition on the inputs: fewer than half of the 150 bricks (the minimal set, the bricks of dilate(N, 1), is 36)
    print(f"sphere scene: {int(marks.sum())} of {marks.size} bricks marked, band {band} of {slabs} pixel-slabs, "
          f"|N| {int(N.sum())}, |dilate(N, 1)| {int(need.sum())} of {need.size} voxels")
    assert marks.shape == (5, 5, 6) and 0 < int(marks.sum()) < marks.size / 2
    assert band <= 1e-3 * slabs


@pytest.mark.parametrize("min_weight", [1.0, 2.0, 4.0])
def test_restricted_grid_extracts_the_identical_mesh(min_weight):
    sc = SR.sphere_scene()
    grid, _ = SR.scene_dense(sc)
    marks = SR.scene_marks(sc)[0]
    dense = R.extract(grid, min_weight, sc["g2w"])
    sparse = R.extract(SR.restrict(grid, marks), min_weight, sc["g2w"])
    assert len(dense[0]) > 0 and len(dense[2]) > 0
    for a, b in zip(dense, sparse):
        assert np.array_equal(a, b)
    assert np.array_equal(dense[0].view(np.int32), sparse[0].view(np.int32))
    # without the 1-voxel expansion the mesh differs: the test can fail
    N = SR.scene_negative(sc)
    bare = R.extract(np.where(N[None], grid, np.float32(0.0)), min_weight, sc["g2w"])
    assert len(bare[0]) != len(dense[0])


def test_dilate_and_restrict():
    m = np.zeros((5, 6, 7), dtype=bool)
    m[2, 3, 4] = m[0, 0, 0] = True
    d = SR.dilate(m, 1)
    assert int(d.sum()) == 27 + 8 and d[1:4, 2:5, 3:6].all() and d[:2, :2, :2].all()
    marks = np.zeros((2, 2, 2), dtype=bool)
    marks[1, 0, 1] = True
    g = np.ones((6, 12, 10, 14), dtype=np.float32)
    r = SR.restrict(g, marks)
    assert r[:, 8:12, 0:8, 8:14].all() and int(r[0].sum()) == 4 * 8 * 6


def _nadir_case():
    """A camera 3 above the plane u = 0 at (0.3, -0.2), looking down, 40 x 40 pixels, focal length 100; the box
    [-1.6, 1.6]^2 x [-0.6, 1.0] at voxel 0.1: 32 x 32 x 16 voxels, 4 x 4 x 2 bricks."""
    shape, voxel, trunc, height, cam_xy = (32, 32, 16), 0.1, 0.4, 3.0, (0.3, -0.2)
    g2w = np.array([[voxel, 0, 0, -1.6], [0, voxel, 0, -1.6], [0, 0, voxel, -0.6]], dtype=np.float64)
    Rm = np.diag([1.0, -1.0, -1.0])
    w2c = np.eye(4)
    w2c[:3, :3] = Rm
    w2c[:3, 3] = -Rm @ np.array([cam_xy[0], cam_xy[1], height])
    cams = np.concatenate([(w2c @ np.vstack([g2w, [0, 0, 0, 1.0]]))[:3].reshape(12), [100.0, 100.0, 20.0, 20.0]])[None]
    depth = np.full((1, 40, 40), height, dtype=np.float32)
    return shape, voxel, trunc, height, cam_xy, cams, depth


def test_nadir_camera_marks_one_layer_under_the_footprint():
    shape, voxel, trunc, height, cam_xy, cams, depth = _nadir_case()
    marks, band, slabs, lo, hi = SR.mark(shape, SR.invert_records(cams), depth, np.ones_like(depth), 0.01, float("inf"), 0.5,
                                         trunc, voxel)
    assert band == 0 and np.array_equal(lo, hi)
    # the surface voxels have u in [-0.4, 0): grid z in [2, 6), with the expansion the indices 1 .. 6: the lower layer only
    assert marks[0].any() and not marks[1].any()
    # the footprint at the far depth 3.4 is 0.2 * 3.4 = 0.68 either side of the camera; with 1 voxel more, the voxel
    # centres i + 0.5 inside it, in bricks of 8
    want = np.zeros((4, 4), dtype=bool)
    rng = []
    for c in cam_xy:
        a, b = (c - 0.68 + 1.6) / voxel - 1.0, (c + 0.68 + 1.6) / voxel + 1.0
        rng.append((int(np.ceil(a - 0.5)) >> 3, int(np.floor(b - 0.5)) >> 3))
    want[rng[1][0]:rng[1][1] + 1, rng[0][0]:rng[0][1] + 1] = True
    assert rng == [(1, 3), (0, 2)]
    assert np.array_equal(marks[0], want)
    # nothing is marked through a gate: alpha below alpha_min, a depth beyond depth_max, the band behind the near plane
    for kw in (dict(alpha=0.4), dict(depth_max=2.0), dict(near=3.5)):
        args = dict(alpha=1.0, near=0.01, depth_max=float("inf"))
        args.update(kw)
        m = SR.mark(shape, SR.invert_records(cams), depth, np.full_like(depth, args["alpha"]), args["near"], args["depth_max"],
                    0.5, trunc, voxel)[0]
        assert not m.any(), kw


def test_sparse_sizing_and_refusals():
    import torch
    from clm_gs_amd import tsdf
    # the box of the issue: 300 m x 300 m x 60 m at 5 cm, twenty times the dense index limit
    shape, nb = tsdf.check_brick_grid((0, 0, 0, 300, 300, 60), 0.05, grid_gb=16)
    assert shape == (6000, 6000, 1200) and nb == (750, 750, 150)
    with pytest.raises(ValueError, match="2\\^31 voxels"):
        tsdf.check_grid((0, 0, 0, 300, 300, 60), 0.05, grid_gb=1000)
    with pytest.raises(ValueError, match="above 2\\^30 bricks; about --voxel .* fits \\(an estimate"):
        tsdf.check_brick_grid((0, 0, 0, 10000, 10000, 10000), 0.001)
    with pytest.raises(ValueError, match="brick table of 1000 x 1000 x 1000 = 1000000000 bricks takes 5.00 GB .* --grid_gb 1"):
        tsdf.check_brick_grid((0, 0, 0, 8000, 8000, 8000), 1.0, grid_gb=1)
    with pytest.raises(ValueError, match="--voxel must be positive"):
        tsdf.check_brick_grid((0, 0, 0, 1, 1, 1), 0.0)
    assert tsdf.check_sparse_size(1000, 10 ** 6, 0.05, grid_gb=16) == 5 * 10 ** 6 + 1000 * 12288
    with pytest.raises(ValueError) as e:
        tsdf.check_sparse_size(10 ** 6, 10 ** 8, 0.05, grid_gb=1)
    msg = str(e.value)
    assert "1000000 of 100000000 bricks" in msg and "12.79 GB" in msg and "--grid_gb 1" in msg and "an estimate" in msg
    fit = float(msg.split("about --voxel ")[1].split()[0])
    assert abs(fit - 0.05 * (12.788 / 1.0) ** 0.5) < 2e-3
    with pytest.raises(ValueError, match="2\\^31 stored voxels"):
        tsdf.check_sparse_size(1 << 22, 1 << 24, 0.05, grid_gb=1000)
    tsdf.check_sparse_size((1 << 22) - 1, 1 << 24, 0.05, grid_gb=1000)
    # the volume itself, on the host: the order of the calls and the size at allocate()
    frame = (np.eye(3)[0], np.eye(3)[1], np.eye(3)[2])
    v = tsdf.SparseTsdfVolume(frame, (-2.4, -2, -2, 2.4, 2, 2), 0.1, device="cpu", grid_gb=1e-3)
    assert v.shape == (48, 40, 40) and (v.nbx, v.nby, v.nbz) == (6, 5, 5) and v.bricks_total == 150
    with pytest.raises(ValueError, match="add\\(\\) before allocate"):
        v.add(None, torch.zeros(3, 4, 4), torch.zeros(4, 4), torch.zeros(4, 4))
    v.marks.fill_(1)
    with pytest.raises(ValueError, match="150 of 150 bricks are marked, marks \\+ table \\+ pool take 0.00 GB, above --grid_gb 0.001"):
        v.allocate()
    v.marks.zero_()
    v.marks[1, 2, 3] = v.marks[4, 0, 5] = 1
    assert v.allocate() == 2 and v.S == 2
    assert v.bricks.tolist() == [(1 * 5 + 2) * 6 + 3, (4 * 5 + 0) * 6 + 5] and v.bricks.dtype == torch.int32
    assert v.table.dtype == torch.int32 and v.table[1, 2, 3] == 0 and v.table[4, 0, 5] == 1 and int((v.table == -1).sum()) == 148
    assert v.pool.shape == (2, 6, 8, 8, 8) and not v.pool.any()
    with pytest.raises(ValueError, match="mark\\(\\) after allocate"):
        v.mark(None, torch.zeros(4, 4), torch.zeros(4, 4))
    with pytest.raises(ValueError, match="allocate\\(\\) has been called"):
        v.allocate()
    v.pool[1, 2, 7, 0, 3] = 5.0  # plane 2 of the voxel (x, y, z) = (5 * 8 + 3, 0, 4 * 8 + 7)
    d = v.to_dense()
    assert d.shape == (6, 40, 40, 48) and float(d[2, 39, 0, 43]) == 5.0 and int(d.count_nonzero()) == 1
    empty = tsdf.SparseTsdfVolume(frame, (-2.4, -2, -2, 2.4, 2, 2), 0.1, device="cpu")
    assert empty.allocate() == 0 and not empty.to_dense().any()
    with pytest.raises(ValueError, match="--trunc_voxels"):
        tsdf.SparseTsdfVolume(frame, (-2.4, -2, -2, 2.4, 2, 2), 0.1, trunc_voxels=0.0, device="cpu")


def test_mark_record_is_the_inverse_of_the_camera_record():
    from types import SimpleNamespace
    from clm_gs_amd import tsdf
    w2c = SR.look_at(np.array([1.0, -2.0, 3.0]), np.zeros(3), np.array([0.0, 0.0, 1.0])).astype(np.float32)
    K = np.array([[100.0, 0, 32.0], [0, 110.0, 24.0], [0, 0, 1]], dtype=np.float32)
    cam = SimpleNamespace(_clmgs_host=(w2c.reshape(16), K.reshape(9), None), image_name="c")
    g2w = tsdf.grid_to_world((np.eye(3)[0], np.eye(3)[1], np.eye(3)[2]), (0, 0, 0, 1, 1, 1), 0.25)
    rec, inv = tsdf.camera_record(cam, g2w), tsdf.camera_mark_record(cam, g2w)
    assert inv.dtype == np.float64 and inv.shape == (16,) and list(inv[12:]) == list(rec[12:])
    prod = np.vstack([rec[:12].reshape(3, 4), [0, 0, 0, 1]]) @ np.vstack([inv[:12].reshape(3, 4), [0, 0, 0, 1]])
    assert np.allclose(prod, np.eye(4), atol=1e-12)
    assert np.array_equal(inv, SR.invert_records(rec[None])[0])


def test_cli_sparse_refusals_come_before_anything_is_loaded(tmp_path):
    from clm_gs_amd import mesh_model
    out = tmp_path / "out"
    base = ["-m", str(tmp_path / "no_such_model.ply"), "-s", str(tmp_path / "no_such_scene"), "-o", str(out / "mesh.ply"),
            "--sparse"]
    for extra, match in ((["--voxel", "0"], "--voxel must be positive"),
                         (["--voxel", "0.001", "--bounds", "0", "0", "0", "10000", "10000", "10000"], "above 2\\^30 bricks"),
                         (["--voxel", "1", "--grid_gb", "1", "--bounds", "0", "0", "0", "8000", "8000", "8000"], "brick table"),
                         (["--voxel", "1e-7", "--bounds", "0", "0", "0", "1000", "1", "1"], "a side of 2\\^31 voxels"),
                         (["--voxel", "0.1", "--min_weight", "0"], "--min_weight")):
        with pytest.raises(SystemExit, match=match):
            mesh_model.main(base + extra)
        assert not out.exists()
    # a box the dense volume refuses passes the checks of the sparse one
    box = (0, 0, 0, 300, 300, 60)
    with pytest.raises(ValueError, match="2\\^31 voxels"):
        mesh_model.check_options(0.05, box, grid_gb=1000.0)
    mesh_model.check_options(0.05, box, grid_gb=16.0, sparse=True)


def test_trainer_mesh_sparse_rule():
    from clm_gs_amd import trainer, utils
    assert utils.default_args().mesh_sparse is False
    rules = trainer.mesh_rules(utils.default_args(mesh_sparse=True))
    assert any(r and "--mesh_sparse has effect only with --mesh_voxel" in m for r, m in rules)
    assert not any(r for r, _ in trainer.mesh_rules(utils.default_args(mesh_sparse=True, mesh_voxel=0.1)))
    assert not any(r for r, _ in trainer.mesh_rules(utils.default_args(mesh_voxel=0.1)))
    ns = trainer.build_arg_parser().parse_args(["-s", "a", "-m", "b", "--mesh_voxel", "0.25", "--mesh_sparse"])
    assert trainer.train_kwargs(ns)["mesh_sparse"] is True
    assert trainer.train_kwargs(trainer.build_arg_parser().parse_args(["-s", "a", "-m", "b"]))["mesh_sparse"] is False
