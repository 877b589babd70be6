"""Mesh decimation without a GPU ("Mesh decimation"): the numpy restatement of the contract
(tests/mesh_decimate_reference.py) on the analytic grids of tests/tsdf_reference.py -- counts, topology, and the accuracy of
the quadric placement measured against the analytic surfaces, which assumes nothing about the code under test -- the
fallbacks on hand-built meshes, the face rules, the refusals of every entry before anything is read, and the records."""
import json

import numpy as np
import pytest

from tests import mesh_decimate_reference as D
from tests import tsdf_reference as R

BOX_H = 0.61
PLANE_N = np.array([0.3, -0.5, 0.81]) / np.linalg.norm([0.3, -0.5, 0.81])
PLANE_D = 0.07


def box_sdf(h=BOX_H):
    x, y, z = R.centres()
    q = np.stack([np.abs(x) - h, np.abs(y) - h, np.abs(z) - h])
    return np.sqrt((np.maximum(q, 0) ** 2).sum(0)) + np.minimum(q.max(0), 0)


def plane_sdf():
    x, y, z = R.centres()
    return PLANE_N[0] * x + PLANE_N[1] * y + PLANE_N[2] * z - PLANE_D


_MESHES = {}


def mesh(name):
    """(verts, colours, faces) of an analytic 20^3 grid, extracted once."""
    if name not in _MESHES:
        sdf = dict(sphere=R.sphere_sdf, torus=R.torus_sdf, box=box_sdf, plane=plane_sdf)[name]()
        _MESHES[name] = R.extract(R.grid_from_sdf(sdf), 2.0, R.G2W)[:3]
    return _MESHES[name]


def box_distance(p, h=BOX_H):
    """Distance of points to the surface of the axis-aligned box of half-size h."""
    q = np.abs(np.asarray(p, dtype=np.float64)) - h
    outside = np.sqrt((np.maximum(q, 0) ** 2).sum(1))
    return np.where((q <= 0).all(1), -q.max(1), outside)


# ------------------------------------------------------------------------------------------------ counts and topology
@pytest.mark.parametrize("name,n_in,cell,n_out,euler", [
    ("sphere", (746, 1488), 0.3, (104, 204), 2), ("sphere", (746, 1488), 0.5, (56, 108), 2),
    ("torus", (728, 1456), 0.25, (186, 372), 0), ("torus", (728, 1456), 0.3, (96, 192), 0),
    ("torus", (728, 1456), 0.375, (64, 128), 0), ("torus", (728, 1456), 0.5, (48, 96), 0),
    ("box", (602, 1200), 0.3, (128, 252), 2)])
def test_counts_and_topology(name, n_in, cell, n_out, euler):
    verts, colours, faces = mesh(name)
    assert (len(verts), len(faces)) == n_in
    v, c, f, rep = D.decimate(verts, colours, faces, cell)
    assert v.dtype == np.float32 and c.dtype == np.uint8 and f.dtype == np.int32
    assert (len(v), len(f)) == n_out and tuple(rep) == D.REPORT_KEYS
    t = R.topology(v, f)
    assert t["closed"] and t["oriented"] and t["euler"] == euler and t["volume"] > 0, t
    assert rep == dict(cell=cell, vertices_in=n_in[0], faces_in=n_in[1], vertices=n_out[0], faces=n_out[1],
                       faces_collapsed=n_in[1] - n_out[1] - rep["faces_duplicate"], faces_duplicate=rep["faces_duplicate"],
                       placed_quadric=n_out[0], placed_mean_degenerate=0, placed_mean_outside=0)
    assert (f[:, 0] < f[:, 1]).all() and (f[:, 0] < f[:, 2]).all()  # rotated: the smallest index first


def test_sphere_at_a_quarter_is_not_a_manifold_and_loses_six_duplicates():
    """The result does not guarantee a manifold: cell 0.25 on the sphere."""
    v, c, f, rep = D.decimate(*mesh("sphere"), 0.25)
    t = R.topology(v, f)
    assert rep["faces_duplicate"] == 6 and rep["placed_quadric"] == rep["vertices"] == len(v)
    assert not (t["closed"] and t["oriented"]), t
    assert len(np.unique(f, axis=0)) == len(f)


# ------------------------------------------------------------------------------------------------ accuracy
def test_box_quadric_placement_beats_the_mean_and_the_input():
    verts, colours, faces = mesh("box")
    vq = D.decimate(verts, colours, faces, 0.3)[0]
    vm = D.decimate(verts, colours, faces, 0.3, placement="mean")[0]
    dq, dm, d_in = np.abs(box_distance(vq)), np.abs(box_distance(vm)), np.abs(box_distance(verts))
    print(f"box, cell 0.3: quadric max {dq.max():.4f} mean {dq.mean():.4f} | mean placement max {dm.max():.4f} mean "
          f"{dm.mean():.4f} | input max {d_in.max():.4f}")
    assert dq.max() < dm.max() and dq.mean() < dm.mean()
    assert dq.max() <= d_in.max()


@pytest.mark.parametrize("cell", [0.3, 0.5])
def test_sphere_quadric_placement_beats_the_mean(cell):
    verts, colours, faces = mesh("sphere")
    err = lambda v: np.abs(np.linalg.norm(v.astype(np.float64), axis=1) - 0.8).mean()
    eq, em = err(D.decimate(verts, colours, faces, cell)[0]), err(D.decimate(verts, colours, faces, cell, placement="mean")[0])
    print(f"sphere, cell {cell}: mean radial error quadric {eq:.4f} mean placement {em:.4f}")
    assert eq < em


@pytest.mark.parametrize("cell", [0.3, 0.5])
def test_tilted_plane_rank_one_quadric(cell):
    """Every face lies in one plane: A has rank one, the regulariser picks the point of the plane nearest the mean."""
    verts, colours, faces = mesh("plane")
    on_plane = lambda v: np.abs(v.astype(np.float64) @ PLANE_N - PLANE_D)
    # the extraction's own float32 vertices lie this close to the plane; an output coordinate is below 2 in magnitude, so
    # its rounding to float32 moves it by at most 2^-24 per axis, |n|_1 2^-24 along the normal
    slack = on_plane(verts).max() + np.abs(PLANE_N).sum() * 2.0 ** -24
    v, c, f, rep = D.decimate(verts, colours, faces, cell)
    print(f"plane, cell {cell}: input off-plane {on_plane(verts).max():.3e} output {on_plane(v).max():.3e} bound {slack:.3e}")
    assert rep["placed_quadric"] == rep["vertices"] > 0 and len(f) > 0
    assert on_plane(v).max() <= slack


# ------------------------------------------------------------------------------------------------ fallbacks
def degenerate_mesh():
    """Cell 1.  Vertices 0, 1, 2 lie on a line inside cell (0,0,0): their face has zero area and collapses.  Face (0, 3, 4)
    lies on the same line, through the cells (1,0,0) and (2,0,0): it survives, and every cluster sees only zero normals."""
    verts = np.array([[0.5, 0.5, 0.5], [0.25, 0.5, 0.5], [0.75, 0.5, 0.5], [1.5, 0.5, 0.5], [2.5, 0.5, 0.5]], dtype=np.float32)
    faces = np.array([[0, 1, 2], [0, 3, 4]], dtype=np.int32)
    colours = np.array([[10, 20, 30], [11, 21, 31], [12, 23, 33], [0, 0, 0], [255, 255, 255]], dtype=np.uint8)
    return verts, colours, faces, 1.0


def crease_mesh():
    """Cell 1.  Two faces with a corner each in cell (0,0,0), in the planes z = 0.5 +- 0.1 (x - 4): nearly parallel, they
    meet in the line x = 4, z = 0.5, three and a half cells away.  The quadric's minimiser for that cell runs along to the
    crease (its pull, 2 * 0.1^2 of the trace, is thirty times the regulariser's 2^-10 / 3) and the vertex is placed at the
    mean instead.  Each face has its corners in three different cells, so both survive."""
    up, down = (lambda x: 0.5 + 0.1 * (x - 4.0)), (lambda x: 0.5 - 0.1 * (x - 4.0))
    verts = np.array([[0.2, 0.2, up(0.2)], [1.2, 0.2, up(1.2)], [0.2, 1.2, up(0.2)],
                      [0.6, 0.6, down(0.6)], [0.6, 1.6, down(0.6)], [-0.4, 0.6, down(-0.4)]], dtype=np.float32)
    faces = np.array([[0, 1, 2], [3, 4, 5]], dtype=np.int32)
    colours = np.full((6, 3), 100, dtype=np.uint8)
    colours[3] = [101, 103, 100]
    return verts, colours, faces, 1.0


def test_fallback_degenerate_quadric():
    verts, colours, faces, cell = degenerate_mesh()
    v, c, f, rep = D.decimate(verts, colours, faces, cell)
    assert rep["vertices"] == 3 and rep["placed_mean_degenerate"] == 3 and rep["placed_quadric"] == 0
    assert rep["faces"] == 1 and rep["faces_collapsed"] == 1 and f.tolist() == [[0, 1, 2]]
    assert np.array_equal(v[0], np.array([0.5, 0.5, 0.5], dtype=np.float32))  # the mean of the three members
    assert c[0].tolist() == [11, 21, 31]  # the channel sums 33, 64, 94 over 3 members


def test_fallback_minimiser_outside():
    verts, colours, faces, cell = crease_mesh()
    v, c, f, rep = D.decimate(verts, colours, faces, cell)
    print(rep)
    # the keys ascend with (i, j, k): (-1,0,0) vertex 5, (0,0,0) vertices 0 and 3, (0,1,0) vertices 2 and 4, (1,0,0) vertex 1;
    # the two cells that see both faces take the branch, the two that see one plane are rank one and stay on it
    assert rep["vertices"] == 4 and rep["placed_mean_outside"] == 2 and rep["placed_quadric"] == 2, rep
    k = 1
    want = ((verts[0].astype(np.float64) - 0.5) + (verts[3].astype(np.float64) - 0.5)) / 2.0 + 0.5
    assert np.array_equal(v[k], want.astype(np.float32))
    assert c[k].tolist() == [101, 102, 100]  # 100.5 rounds up, 101.5 rounds up
    assert f.tolist() == [[1, 3, 2], [0, 1, 2]] and rep["faces_collapsed"] == rep["faces_duplicate"] == 0


# ------------------------------------------------------------------------------------------------ face and vertex rules
def test_unreferenced_vertices_are_dropped_and_face_order_is_kept():
    verts = np.array([[0.5, 0.5, 0.5], [9.5, 9.5, 9.5], [1.5, 0.5, 0.5], [0.5, 1.5, 0.5], [0.5, 0.5, 1.5], [np.nan, 0, 0]],
                     dtype=np.float32)
    colours = np.arange(18, dtype=np.uint8).reshape(6, 3)
    faces = np.array([[4, 0, 3], [3, 2, 0], [2, 4, 0]], dtype=np.int32)
    v, c, f, rep = D.decimate(verts, colours, faces, 1.0)  # vertices 1 and 5 (a NaN) are named by no face
    assert rep["vertices_in"] == 6 and rep["vertices"] == 4 == len(v) and rep["faces"] == 3
    # keys ascend with (i, j, k): (0,0,0) v0, (0,0,1) v4, (0,1,0) v3, (1,0,0) v2
    assert f.tolist() == [[0, 2, 1], [0, 2, 3], [0, 3, 1]]
    assert c.tolist() == [colours[0].tolist(), colours[4].tolist(), colours[3].tolist(), colours[2].tolist()]


def test_twins():
    verts = np.array([[0.5, 0.5, 0.5], [1.5, 0.5, 0.5], [0.5, 1.5, 0.5], [0.6, 0.6, 0.6]], dtype=np.float32)
    colours = np.zeros((4, 3), dtype=np.uint8)
    faces = np.array([[0, 1, 2], [2, 1, 0], [1, 2, 3], [2, 3, 1], [1, 0, 2]], dtype=np.int32)
    v, c, f, rep = D.decimate(verts, colours, faces, 1.0)  # clusters: 0 = {v0, v3}, 1 = v2, 2 = v1
    # opposite orientations both stay; (1,2,3) and (2,3,1) repeat the first face and go; (1,0,2) repeats the second
    assert f.tolist() == [[0, 2, 1], [0, 1, 2]] and rep["faces_duplicate"] == 3 and rep["faces_collapsed"] == 0


def test_negative_cells_a_mesh_straddling_the_origin():
    verts = np.array([[-0.25, -0.25, -0.25], [0.25, -0.25, -0.25], [-0.25, 0.25, -0.25], [-0.75, -0.75, -0.75],
                      [-1e-30, 0.1, 0.1]], dtype=np.float32)
    colours = np.zeros((5, 3), dtype=np.uint8)
    faces = np.array([[0, 1, 2], [3, 1, 2], [4, 1, 2]], dtype=np.int32)
    ijk, key = D.cell_keys(verts, np.ones(5, dtype=bool), 0.5)
    assert ijk.tolist() == [[-1, -1, -1], [0, -1, -1], [-1, 0, -1], [-2, -2, -2], [-1, 0, 0]]
    assert (key >= 0).all() and list(np.argsort(key)) == [3, 0, 2, 4, 1]
    v, c, f, rep = D.decimate(verts, colours, faces, 0.5)
    assert rep["vertices"] == 5 and f.tolist() == [[1, 4, 2], [0, 4, 2], [2, 3, 4]]  # (3, 4, 2) rotated
    assert np.abs(v - verts[[3, 0, 2, 4, 1]]).max() < 0.5


def test_range_and_non_finite_are_refused_by_name():
    tri = np.array([[0, 1, 2]], dtype=np.int32)
    col = np.zeros((3, 3), dtype=np.uint8)
    far = np.array([[0, 0, 0], [1, 0, 0], [0, 1100.0, 0]], dtype=np.float32)
    with pytest.raises(ValueError, match=r"cell index outside \[-2\^20, 2\^20\).*smallest cell"):
        D.decimate(far, col, tri, 0.001)  # 1100 / 0.001 > 2^20
    D.decimate(far, col, tri, 0.0011)
    edge = np.array([[0, 0, 0], [1, 0, 0], [0, -1024.0, 0]], dtype=np.float32)
    assert D.decimate(edge, col, tri, 2.0 ** -10)[3]["vertices"] == 3  # index -2^20 is the last that fits
    with pytest.raises(ValueError, match="cell index outside"):
        D.decimate(-edge, col, tri, 2.0 ** -10)  # index +2^20 does not
    for bad in (np.nan, np.inf, -np.inf):
        nan = np.array([[0, 0, 0], [1, 0, 0], [0, bad, 0]], dtype=np.float32)
        with pytest.raises(ValueError, match="non-finite vertex coordinate"):
            D.decimate(nan, col, tri, 0.5)
    for bad in (-1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="cell must be"):
            D.decimate(far, col, tri, bad)
    same = D.decimate(far, col, tri, 0)
    assert same[0] is far and same[1] is col and same[2] is tri and same[3] is None
    v, c, f, rep = D.decimate(far, col, np.zeros((0, 3), dtype=np.int32), 0.5)
    assert v.shape == (0, 3) and c.shape == (0, 3) and f.shape == (0, 3) and rep["vertices"] == 0 and rep["vertices_in"] == 3


# ------------------------------------------------------------------------------------------------ options and records
def test_refusals_come_before_any_path_is_touched(tmp_path):
    from clm_gs_amd import mesh_clean, mesh_decimate, mesh_model
    missing = str(tmp_path / "no_such_dir" / "mesh.ply")
    out = tmp_path / "out"
    for bad in ("-1", "nan", "inf"):
        with pytest.raises(SystemExit, match="--decimate_cell must be a finite number >= 0"):
            mesh_clean.main(["-i", missing, "-o", str(out / "clean.ply"), "--decimate_cell", bad])
        with pytest.raises(SystemExit, match="--decimate_cell must be a finite number >= 0"):
            mesh_model.main(["-m", missing, "-s", missing, "-o", str(out / "mesh.ply"), "--voxel", "1", "--decimate_cell", bad])
        with pytest.raises(ValueError, match="--decimate_cell"):
            mesh_model.check_options(0.1, decimate_cell=float(bad))
        with pytest.raises(ValueError, match="cell must be a finite number >= 0"):
            mesh_decimate.decimate(None, None, None, float(bad))
        assert not out.exists()
    with pytest.raises(SystemExit, match=r"nothing to do.*--decimate_cell"):
        mesh_clean.main(["-i", missing, "-o", str(out / "clean.ply"), "--decimate_cell", "0"])
    with pytest.raises(ValueError, match="--decimate_cell"):
        mesh_model.check_options(0.1, decimate_cell="0.5")
    mesh_model.check_options(0.1, decimate_cell=0.25)
    # the positional callers of before: ten arguments, `sparse` the last
    mesh_model.check_options(0.1, None, 16.0, 4.0, 2.0, 1, "expected", 0, 0, False)
    with pytest.raises(ValueError, match="--decimate_cell"):
        mesh_model.check_options(0.1, None, 16.0, 4.0, 2.0, 1, "expected", 0, 0, False, -0.5)
    with pytest.raises(ValueError, match="--decimate_cell"):  # before a camera or the model is looked at
        mesh_model.build_mesh(None, None, None, str(out / "mesh.ply"), 0.1, decimate_cell=-1.0)
    assert not out.exists()
    a, b, c = object(), object(), object()  # off: the inputs come back untouched, nothing is looked at
    assert mesh_decimate.decimate(a, b, c, 0.0) == (a, b, c, None) and mesh_decimate.decimate(a, b, c, 0) == (a, b, c, None)
    assert mesh_decimate.REPORT_KEYS == D.REPORT_KEYS


def test_trainer_option_reaches_default_args_and_bad_values_are_refused(tmp_path):
    from clm_gs_amd import trainer, utils
    a = utils.default_args()
    assert a.mesh_decimate_cell == 0.0
    ap = trainer.build_arg_parser()
    assert trainer.train_kwargs(ap.parse_args(["-s", "a", "-m", "b"]))["mesh_decimate_cell"] == 0.0
    kw = trainer.train_kwargs(ap.parse_args(["-s", "a", "-m", "b", "--mesh_voxel", "0.25", "--mesh_decimate_cell", "0.75"]))
    assert kw["mesh_decimate_cell"] == 0.75
    assert utils.default_args(**{k: v for k, v in kw.items() if hasattr(a, k)}).mesh_decimate_cell == 0.75
    assert trainer.mesh_rules(utils.default_args()) == []
    assert not any(r for r, _ in trainer.mesh_rules(utils.default_args(mesh_voxel=0.1, mesh_decimate_cell=0.4)))
    rules = trainer.mesh_rules(utils.default_args(mesh_decimate_cell=0.4))
    assert any(r and "--mesh_decimate_cell has effect only with --mesh_voxel" in m for r, m in rules)
    for bad in (-1.0, float("nan"), float("inf")):
        for voxel in (0.0, 0.1):
            with pytest.raises(ValueError, match="--mesh_decimate_cell must be a finite number >= 0"):
                trainer.check_training(utils.default_args(clm_offload=True, mesh_voxel=voxel, mesh_decimate_cell=bad))
        with pytest.raises(ValueError, match="--mesh_decimate_cell"):  # the source directory does not exist
            trainer.train_from_colmap(str(tmp_path / "no_such_scene"), str(tmp_path / "out"), mesh_voxel=0.1,
                                      mesh_decimate_cell=bad)
        assert not (tmp_path / "out").exists()
    with pytest.raises(ValueError, match="--mesh_decimate_cell has effect only with --mesh_voxel"):
        trainer.train_from_colmap(str(tmp_path / "no_such_scene"), str(tmp_path / "out"), mesh_decimate_cell=0.5)
    assert not (tmp_path / "out").exists()


def test_json_record_and_log_words():
    from clm_gs_amd import mesh_decimate
    meta = dict(voxel=0.5, vertices=746, faces=1488, camera_names=["a", "b"])
    report = D.decimate(*mesh("sphere"), 0.3)[3]
    out = mesh_decimate.json_record(meta, report, 104, 204)
    assert meta == dict(voxel=0.5, vertices=746, faces=1488, camera_names=["a", "b"])  # not modified
    assert out == dict(voxel=0.5, vertices=104, faces=204, camera_names=["a", "b"], decimation=report)
    assert out["decimation"] is not report and tuple(out["decimation"]) == D.REPORT_KEYS
    assert json.loads(json.dumps(out)) == out
    assert mesh_decimate.log_words(report) == " decimated 746 -> 104 vertices 1488 -> 204 faces cell 0.3"
