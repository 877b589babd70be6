"""Mesh cleanup on the CPU ("Mesh cleanup"): the numpy restatement (tests/mesh_clean_reference.py)
against a brute-force search, the selection rule, the refusals that come before anything is read, the trainer's option
table and the json record.  Every comparison is exact."""
import numpy as np
import pytest

from tests import mesh_clean_reference as M
from tests import tsdf_reference as R


def test_reference_labels_equal_a_breadth_first_search():
    rng = np.random.default_rng(3)
    for case in range(40):
        V = int(rng.integers(1, 60))
        F = int(rng.integers(0, 40))
        faces = rng.integers(0, V, size=(F, 3)).astype(np.int32)  # degenerate faces included
        lab = M.labels(faces, V)
        assert np.array_equal(lab, M.bfs_labels(faces, V)), case
        assert (lab <= np.arange(V)).all() and np.array_equal(lab[lab], lab)
        named = np.zeros(V, dtype=bool)
        named[faces.reshape(-1)] = True
        assert np.array_equal(lab[~named], np.arange(V)[~named])  # a vertex no face names is its own label
        count = M.sizes(faces, lab)
        assert int(count.sum()) == F and (count[lab != np.arange(V)] == 0).all()


def _islands(sizes):
    """Fans of the given face counts, one after the other: island k has sizes[k] + 2 vertices of its own."""
    faces, base = [], 0
    for n in sizes:
        faces += [(base, base + i + 1, base + i + 2) for i in range(n)]
        base += n + 2
    return np.array(faces, dtype=np.int32).reshape(-1, 3), base


def _mesh(faces, V):
    verts = (np.arange(3 * V, dtype=np.float32) * 0.25).reshape(V, 3)
    colours = (np.arange(3 * V) % 251).astype(np.uint8).reshape(V, 3)
    return verts, colours, faces


def test_ranking_ties_go_to_the_smaller_label():
    faces, V = _islands([3, 5, 5, 2, 5])        # labels 0, 5, 12, 19, 23
    lab = M.labels(faces, V)
    count = M.sizes(faces, lab)
    comp, kept = M.kept_labels(count, keep_largest=2)
    assert comp.tolist() == [0, 5, 12, 19, 23] and kept.tolist() == [5, 12]
    assert M.kept_labels(count, keep_largest=1)[1].tolist() == [5]
    assert M.kept_labels(count, keep_largest=4)[1].tolist() == [0, 5, 12, 23]
    assert M.kept_labels(count, keep_largest=9)[1].tolist() == [0, 5, 12, 19, 23]


def test_min_faces_and_keep_largest_alone_and_together():
    faces, V = _islands([3, 5, 5, 2, 7])
    count = M.sizes(faces, M.labels(faces, V))
    assert M.kept_labels(count, min_faces=0, keep_largest=0)[1].tolist() == [0, 5, 12, 19, 23]
    assert M.kept_labels(count, min_faces=3)[1].tolist() == [0, 5, 12, 23]
    assert M.kept_labels(count, min_faces=6)[1].tolist() == [23]
    assert M.kept_labels(count, min_faces=8)[1].tolist() == []
    assert M.kept_labels(count, keep_largest=3)[1].tolist() == [5, 12, 23]
    # together: the rank is among ALL components, so min_faces cannot promote a component into the K largest
    assert M.kept_labels(count, min_faces=6, keep_largest=3)[1].tolist() == [23]
    assert M.kept_labels(count, min_faces=4, keep_largest=2)[1].tolist() == [5, 23]
    v, c, f, rep = M.clean(*_mesh(faces, V), min_faces=4, keep_largest=2)
    assert rep == dict(components=5, components_kept=2, vertices_removed=V - 16, faces_removed=22 - 12, largest_faces=7)
    assert len(v) == len(c) == 16 and len(f) == 12 and int(f.max()) == 15


def test_unreferenced_vertices_go_and_order_stays():
    rng = np.random.default_rng(11)
    faces, V0 = _islands([4, 1, 6])
    V = V0 + 9
    perm = rng.permutation(V)                   # the nine unreferenced vertices land anywhere
    faces = perm[faces].astype(np.int32)[rng.permutation(len(faces))]
    verts, colours, _ = _mesh(faces, V)
    v, c, f, rep = M.clean(verts, colours, faces, min_faces=1)
    assert rep["components"] == rep["components_kept"] == 3 and rep["vertices_removed"] == 9 and rep["faces_removed"] == 0
    used = np.unique(faces)
    assert np.array_equal(v, verts[used]) and np.array_equal(c, colours[used])  # kept vertices in their original order
    assert np.array_equal(used[f], faces)       # kept faces in their order, naming the same vertices
    v, c, f, rep = M.clean(verts, colours, faces, min_faces=2)
    lab = M.labels(faces, V)
    big = M.sizes(faces, lab)[lab[faces[:, 0]]] >= 2
    used = np.unique(faces[big])
    assert np.array_equal(v, verts[used]) and np.array_equal(used[f], faces[big]) and rep["faces_removed"] == 1


def test_two_spheres_of_the_analytic_grid():
    """The figures the GPU test holds the kernels to, from the references alone."""
    verts, colours, faces, _ = R.extract(*two_spheres())
    assert (len(verts), len(faces)) == (658, 1308)
    lab = M.labels(faces, len(verts))
    count = M.sizes(faces, lab)
    assert np.nonzero(count)[0].tolist() == [0, 590] and count[[0, 590]].tolist() == [1176, 132]
    for kw in (dict(min_faces=133), dict(keep_largest=1)):
        v, c, f, rep = M.clean(verts, colours, faces, **kw)
        t = R.topology(v, f)
        assert (t["V"], t["F"], t["euler"], t["closed"], t["oriented"]) == (590, 1176, 2, True, True)
        assert rep == dict(components=2, components_kept=1, vertices_removed=68, faces_removed=132, largest_faces=1176)
    small = M.clean(verts[lab == 590], colours[lab == 590], faces[lab[faces[:, 0]] == 590] - 590, min_faces=1)
    t = R.topology(small[0], small[2])
    assert (t["V"], t["F"], t["euler"], t["closed"], t["oriented"]) == (68, 132, 2, True, True)


def two_spheres():
    x, y, z = R.centres()
    ball = lambda c, r: np.sqrt((x - c) ** 2 + (y - c) ** 2 + (z - c) ** 2) - r
    return R.grid_from_sdf(np.minimum(ball(-0.3, 0.7), ball(0.8, 0.25))), 2.0, R.G2W


def test_refusals_come_before_any_path_is_touched(tmp_path):
    from clm_gs_amd import clean_mesh, mesh_clean, mesh_model
    assert clean_mesh.main is mesh_clean.main
    missing = str(tmp_path / "no_such_dir" / "mesh.ply")
    out = tmp_path / "out"
    for extra, match in ((["--min_faces", "-1"], "--min_faces must be a non-negative integer"),
                         (["--keep_largest", "-3"], "--keep_largest must be a non-negative integer"),
                         ([], "nothing to do")):
        with pytest.raises(SystemExit, match=match):
            mesh_clean.main(["-i", missing, "-o", str(out / "clean.ply")] + extra)
        assert not out.exists()
    with pytest.raises(ValueError, match="--min_component_faces must be a non-negative integer"):
        mesh_model.check_options(0.1, min_component_faces=-1)
    with pytest.raises(ValueError, match="--keep_components must be a non-negative integer"):
        mesh_model.check_options(0.1, keep_components=-2)
    with pytest.raises(ValueError, match="--keep_components"):
        mesh_model.check_options(0.1, keep_components=1.5)
    mesh_model.check_options(0.1, min_component_faces=10, keep_components=1)
    for extra, match in ((["--min_component_faces", "-1"], "--min_component_faces"), (["--keep_components", "-1"], "--keep_components")):
        with pytest.raises(SystemExit, match=match):
            mesh_model.main(["-m", missing, "-s", missing, "-o", str(out / "mesh.ply"), "--voxel", "1"] + extra)
        assert not out.exists()
    with pytest.raises(ValueError, match="min_faces"):
        mesh_clean.clean(None, None, None, min_faces=-1)
    with pytest.raises(ValueError, match="keep_largest"):
        mesh_clean.clean(None, None, None, keep_largest=-1)
    a, b, c = object(), object(), object()      # both off: the inputs come back untouched, nothing is looked at
    assert mesh_clean.clean(a, b, c) == (a, b, c, None)


def test_trainer_options_reach_default_args_and_negative_values_are_refused(tmp_path):
    from clm_gs_amd import trainer, utils
    a = utils.default_args()
    assert a.mesh_min_component_faces == 0 and a.mesh_keep_components == 0
    ap = trainer.build_arg_parser()
    kw = trainer.train_kwargs(ap.parse_args(["-s", "a", "-m", "b"]))
    assert kw["mesh_min_component_faces"] == 0 and kw["mesh_keep_components"] == 0
    kw = trainer.train_kwargs(ap.parse_args(["-s", "a", "-m", "b", "--mesh_voxel", "0.25", "--mesh_min_component_faces", "50",
                                             "--mesh_keep_components", "2"]))
    assert kw["mesh_min_component_faces"] == 50 and kw["mesh_keep_components"] == 2
    assert getattr(utils.default_args(**{k: v for k, v in kw.items() if hasattr(a, k)}), "mesh_keep_components") == 2
    assert not any(r for r, _ in trainer.mesh_rules(utils.default_args(mesh_voxel=0.1, mesh_min_component_faces=50,
                                                                        mesh_keep_components=2)))
    for bad, name in ((dict(mesh_min_component_faces=-1), "--mesh_min_component_faces"),
                      (dict(mesh_keep_components=-1), "--mesh_keep_components")):
        for voxel in (0.0, 0.1):
            with pytest.raises(ValueError, match=name + " must be a non-negative integer"):
                trainer.check_training(utils.default_args(clm_offload=True, mesh_voxel=voxel, **bad))
        with pytest.raises(ValueError, match=name):  # before anything is loaded: the source directory does not exist
            trainer.train_from_colmap(str(tmp_path / "no_such_scene"), str(tmp_path / "out"), mesh_voxel=0.1, **bad)
        assert not (tmp_path / "out").exists()


def test_json_record():
    from clm_gs_amd import mesh_clean
    meta = dict(voxel=0.5, vertices=658, faces=1308, camera_names=["a", "b"])
    report = dict(components=2, components_kept=1, vertices_removed=68, faces_removed=132, largest_faces=1176, rounds=4)
    out = mesh_clean.json_record(meta, 133, 0, report, 590, 1176)
    assert meta == dict(voxel=0.5, vertices=658, faces=1308, camera_names=["a", "b"])  # not modified
    assert out == dict(voxel=0.5, vertices=590, faces=1176, camera_names=["a", "b"],
                       cleanup=dict(min_faces=133, keep_largest=0, components=2, components_kept=1, vertices_removed=68,
                                    faces_removed=132, largest_faces=1176, rounds=4))
    assert list(out)[:4] == list(meta)          # the keys of the input first, in their order
    assert out["vertices"] + out["cleanup"]["vertices_removed"] == meta["vertices"]
    assert out["faces"] + out["cleanup"]["faces_removed"] == meta["faces"]
    assert mesh_clean.json_path("/x/y/mesh.ply") == "/x/y/mesh.json"
