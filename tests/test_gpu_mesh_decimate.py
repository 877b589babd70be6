"""Mesh decimation on the device ("Mesh decimation"): csrc/mesh_decimate.hip through
clm_kernels.mesh_decimate_*, mesh_decimate.decimate, the mesh export, the clean_mesh tool and the trainer, against the numpy
restatement of the contract (tests/mesh_decimate_reference.py).  Every comparison is exact: array_equal on the float32
positions, the colours and the indices."""
import json
import os

import numpy as np
import pytest
import torch

from tests import mesh_decimate_reference as D
from tests import tsdf_reference as R
from tests.test_mesh_decimate_cpu import box_sdf, crease_mesh, degenerate_mesh

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _dev(dev, verts, colours, faces):
    return (torch.from_numpy(np.ascontiguousarray(verts, dtype=np.float32)).to(dev),
            torch.from_numpy(np.ascontiguousarray(colours, dtype=np.uint8)).to(dev),
            torch.from_numpy(np.ascontiguousarray(faces, dtype=np.int32).reshape(-1, 3)).to(dev))


def _check(dev, verts, colours, faces, cell, what):
    """The kernels on (verts, colours, faces) == the reference, bit for bit.  -> what the reference returned."""
    from clm_gs_amd import mesh_decimate
    v, c, f, rep = mesh_decimate.decimate(*_dev(dev, verts, colours, faces), cell)
    assert v.dtype == torch.float32 and c.dtype == torch.uint8 and f.dtype == torch.int32
    assert v.is_contiguous() and c.is_contiguous() and f.is_contiguous() and v.is_cuda and c.is_cuda and f.is_cuda
    wv, wc, wf, wrep = D.decimate(verts, colours, faces, cell)
    print(f"{what}: {wrep}")
    v, c, f = v.cpu().numpy(), c.cpu().numpy(), f.cpu().numpy()
    assert v.shape == wv.shape and c.shape == wc.shape and f.shape == wf.shape, what
    bad = np.nonzero((v != wv).any(axis=1))[0]
    assert np.array_equal(v, wv), f"{what}: {len(bad)} of {len(wv)} vertices differ, first {bad[:1]}: {v[bad[:1]]} != {wv[bad[:1]]}"
    assert np.array_equal(c, wc), what
    assert np.array_equal(f, wf), what
    assert rep == wrep and tuple(rep) == D.REPORT_KEYS, (what, rep, wrep)
    return wv, wc, wf, wrep


def _extract(dev, sdf):
    from clm_gs_amd import clm_kernels
    return tuple(t.cpu().numpy() for t in clm_kernels.tsdf_extract(torch.from_numpy(R.grid_from_sdf(sdf)).to(dev), 2.0, R.G2W))


# ------------------------------------------------------------------------------------------------ 1. analytic grids
@pytest.mark.parametrize("name", ["sphere", "torus", "box", "two_spheres"])
def test_analytic_grids_through_the_extraction(dev, name):
    x, y, z = R.centres()
    ball = lambda c, r: np.sqrt((x - c) ** 2 + (y - c) ** 2 + (z - c) ** 2) - r
    sdf = dict(sphere=R.sphere_sdf, torus=R.torus_sdf, box=box_sdf,
               two_spheres=lambda: np.minimum(ball(-0.3, 0.7), ball(0.8, 0.25)))[name]()
    verts, colours, faces = _extract(dev, sdf)
    assert (len(verts), len(faces)) == dict(sphere=(746, 1488), torus=(728, 1456), box=(602, 1200), two_spheres=(658, 1308))[name]
    for cell in (0.3, 0.5):
        wv, wc, wf, rep = _check(dev, verts, colours, faces, cell, f"{name}, cell {cell}")
        assert rep["placed_quadric"] == rep["vertices"] and 0 < rep["faces"] < len(faces)
        if name != "two_spheres":
            t = R.topology(wv, wf)
            assert t["closed"] and t["oriented"] and t["euler"] == (0 if name == "torus" else 2), t


def test_shuffled_faces_and_a_second_run(dev):
    """The face order enters only through the order of the sums (and the order of the output faces): compared with the
    reference on the same shuffled faces; counts, colours and the set of faces equal the unshuffled run."""
    from clm_gs_amd import mesh_decimate
    verts, colours, faces = _extract(dev, R.sphere_sdf())
    wv, wc, wf, rep = _check(dev, verts, colours, faces, 0.3, "sphere")
    shuffled = faces[np.random.default_rng(44).permutation(len(faces))]
    sv, sc, sf, srep = _check(dev, verts, colours, shuffled, 0.3, "sphere, shuffled")
    assert srep == rep and np.array_equal(sc, wc)
    assert sorted(map(tuple, sf.tolist())) == sorted(map(tuple, wf.tolist()))
    again = mesh_decimate.decimate(*_dev(dev, verts, colours, shuffled), 0.3)
    assert np.array_equal(again[0].cpu().numpy(), sv) and np.array_equal(again[1].cpu().numpy(), sc)
    assert np.array_equal(again[2].cpu().numpy(), sf) and again[3] == srep


# ------------------------------------------------------------------------------------------------ 2. random triples
def _random_mesh():
    rng = np.random.default_rng(45)
    V, F = 20000, 15000
    verts = (rng.random((V, 3)) * 6.0 - 3.0).astype(np.float32)
    colours = rng.integers(0, 256, size=(V, 3)).astype(np.uint8)
    faces = rng.integers(0, V, size=(F, 3)).astype(np.int32)
    faces[::50, 1] = faces[::50, 0]             # degenerate faces: a == b, and a == b == c
    faces[::250, 2] = faces[::250, 0]
    return verts, colours, faces


def test_random_triples_coarse_and_fine(dev):
    verts, colours, faces = _random_mesh()
    wv, wc, wf, rep = _check(dev, verts, colours, faces, 0.5, "random, cell 0.5")
    assert rep["vertices"] == 12 ** 3 and rep["faces_collapsed"] > 300  # many faces per cluster
    wv, wc, wf, rep = _check(dev, verts, colours, faces, 0.01, "random, cell 0.01")
    assert rep["vertices"] > 0.99 * len(np.unique(faces)) and rep["placed_mean_degenerate"] > 0  # nearly one vertex per cluster


def test_one_cluster_holding_everything(dev):
    """Every vertex in one cell: every face collapses.  The contract decides participation by the INPUT faces, so the
    cluster keeps its vertex: 1 vertex, 0 faces (the reference says the same)."""
    verts, colours, faces = _random_mesh()
    wv, wc, wf, rep = _check(dev, verts + np.float32(3.0), colours, faces, 100.0, "one cluster")
    assert rep["vertices"] == 1 and rep["faces"] == 0 and rep["faces_collapsed"] == len(faces) and wf.shape == (0, 3)
    wv, wc, wf, rep = _check(dev, verts, colours, faces, 100.0, "eight clusters around the origin")
    assert rep["vertices"] == 8 and rep["faces_duplicate"] > 9000  # the cells are aligned to the origin; most faces repeat


# ------------------------------------------------------------------------------------------------ 3. segment lengths
def test_segment_lengths_of_the_placement_kernel(dev):
    """Fans of 63, 64, 65, 255, 256 and 257 faces around a hub each, every hub alone in its cell and every rim vertex in a
    cell of its own: the hub's cluster has exactly that many incidences."""
    sizes = [63, 64, 65, 255, 256, 257]
    rng = np.random.default_rng(46)
    verts, faces = [], []
    for k, n in enumerate(sizes):
        base = len(verts)
        verts.append([10.0 * k + 0.5, 0.5, 0.5])  # the hub: cell (10 k, 0, 0)
        for i in range(n + 1):                      # the rim: one vertex per cell along y, heights vary
            verts.append([10.0 * k + 1.5 + rng.random() * 0.9, i + 0.05 + rng.random() * 0.9, 0.05 + rng.random() * 0.9])
        faces += [(base, base + 1 + i, base + 2 + i) for i in range(n)]
    verts, faces = np.array(verts, dtype=np.float32), np.array(faces, dtype=np.int32)
    colours = rng.integers(0, 256, size=(len(verts), 3)).astype(np.uint8)
    contiguous = faces
    interleaved = np.stack([faces[sum(sizes[:k]) + i] for i in range(max(sizes)) for k in range(len(sizes)) if i < sizes[k]])
    for what, f in (("contiguous", contiguous), ("interleaved", interleaved)):
        wv, wc, wf, rep = _check(dev, verts, colours, f, 1.0, "fans, " + what)
        assert rep["vertices"] == len(verts) and rep["faces"] == sum(sizes) and rep["faces_collapsed"] == 0


# ------------------------------------------------------------------------------------------------ 4. fallbacks, empties
def test_fallback_meshes(dev):
    rep = _check(dev, *degenerate_mesh(), "degenerate")[3]
    assert rep["placed_mean_degenerate"] == 3 and rep["placed_quadric"] == 0
    rep = _check(dev, *crease_mesh(), "crease")[3]
    assert rep["placed_mean_outside"] == 2 and rep["placed_quadric"] == 2


def test_empty_inputs(dev):
    from clm_gs_amd import mesh_decimate
    verts, colours = torch.zeros((5, 3), device=dev), torch.zeros((5, 3), dtype=torch.uint8, device=dev)
    none = torch.empty((0, 3), dtype=torch.int32, device=dev)
    for vv, cc in ((verts, colours), (verts[:0], colours[:0])):
        v, c, f, rep = mesh_decimate.decimate(vv, cc, none, 0.5)
        assert v.shape == (0, 3) and c.shape == (0, 3) and f.shape == (0, 3)
        assert v.dtype == torch.float32 and c.dtype == torch.uint8 and f.dtype == torch.int32
        assert rep == D.decimate(vv.cpu().numpy(), cc.cpu().numpy(), none.cpu().numpy(), 0.5)[3]
    same = mesh_decimate.decimate(verts, colours, none, 0.0)
    assert same[0] is verts and same[1] is colours and same[2] is none and same[3] is None
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ 5. refusals
def test_refusals_come_before_any_launch(dev):
    from clm_gs_amd import _lib, clm_kernels, mesh_decimate
    verts = torch.rand((5, 3), device=dev)
    colours = torch.zeros((5, 3), dtype=torch.uint8, device=dev)
    good = torch.tensor([[0, 1, 2], [2, 3, 4]], dtype=torch.int32, device=dev)
    wide = torch.zeros((5, 6), device=dev)
    cases = [((verts.cpu(), colours, good), "verts must be a tensor on the device"),
             ((verts, colours.cpu(), good), "colours must be a tensor on the device"),
             ((verts, colours, good.cpu()), "faces must be a tensor on the device"),
             ((verts.double(), colours, good), r"verts must be float32 \[N,3\]"),
             ((verts, colours.int(), good), r"colours must be uint8 \[5,3\]"),
             ((verts, colours, good.long()), r"faces must be int32 \[F,3\]"),
             ((torch.zeros((5, 4), device=dev), colours, good), r"verts must be float32 \[N,3\]"),
             ((verts, colours[:4], good), r"colours must be uint8 \[5,3\]"),
             ((verts, colours, torch.zeros((2, 4), dtype=torch.int32, device=dev)), r"faces must be int32 \[F,3\]"),
             ((wide[:, ::2], colours, good), "verts must be contiguous"),
             ((verts, torch.zeros((5, 6), dtype=torch.uint8, device=dev)[:, ::2], good), "colours must be contiguous"),
             ((verts, colours, torch.zeros((2, 6), dtype=torch.int32, device=dev)[:, ::2]), "faces must be contiguous"),
             ((verts, colours, torch.tensor([[0, 1, 5]], dtype=torch.int32, device=dev)), r"outside \[0, 5\)"),
             ((verts, colours, torch.tensor([[0, -1, 2]], dtype=torch.int32, device=dev)), r"outside \[0, 5\)")]
    for args, match in cases:
        with pytest.raises(_lib.ClmgsError, match=match):
            mesh_decimate.decimate(*args, 0.5)
    for bad in (-1.0, float("nan"), float("inf"), "1"):
        with pytest.raises(ValueError, match="cell must be a finite number >= 0"):
            mesh_decimate.decimate(verts, colours, good, bad)
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="cell must be a positive finite number"):
            clm_kernels.mesh_decimate_keys(verts, good, bad)
    # the key pass's flag: read once, before anything else is launched
    launched = []
    faces_pass = clm_kernels.mesh_decimate_faces
    try:
        clm_kernels.mesh_decimate_faces = lambda *a, **k: launched.append(1) or faces_pass(*a, **k)
        far = verts.clone()
        far[3, 1] = 1100.0
        with pytest.raises(ValueError, match=r"cell index outside \[-2\^20, 2\^20\).*smallest cell that fits is about 0\.00104"):
            mesh_decimate.decimate(far, colours, good, 0.001)
        far[3, 1] = float("nan")
        with pytest.raises(ValueError, match="non-finite vertex coordinate"):
            mesh_decimate.decimate(far, colours, good, 0.5)
        assert not launched
        only = torch.tensor([[0, 1, 2]], dtype=torch.int32, device=dev)  # vertex 3 is named by no face: it takes no part
        v, c, f, rep = mesh_decimate.decimate(far, colours, only, 0.001)
        assert launched and rep["vertices_in"] == 5 and 1 <= rep["vertices"] <= 3
    finally:
        clm_kernels.mesh_decimate_faces = faces_pass
    keys, flag = clm_kernels.mesh_decimate_keys(far, good, 0.5)
    assert int(flag) == clm_kernels.MESH_DECIMATE_NONFINITE and int(keys[3]) == -1 and int(keys[0]) >= 0
    v, c, f, rep = mesh_decimate.decimate(verts, colours, good, 0.001)  # (the good input runs)
    assert rep["vertices"] == 5 and rep["faces"] == 2


# ------------------------------------------------------------------------------------------------ 6. end to end
def test_export_with_and_without_decimation_and_the_tool(dev, tmp_path, capsys, monkeypatch):
    from clm_gs_amd import io_ply, mesh_clean, mesh_model, tsdf, utils
    from clm_gs_amd.render_ortho import map_frame
    from tests import mesh_clean_reference as M
    from tests.test_gpu_mesh_clean import _shell_scene
    extracted = []
    extract = tsdf.TsdfVolume.extract

    def recording(self, *a, **kw):
        out = extract(self, *a, **kw)
        extracted.append(tuple(t.cpu().numpy() for t in out))
        return out

    monkeypatch.setattr(tsdf.TsdfVolume, "extract", recording)
    try:
        gaussians, cams, args = _shell_scene(tmp_path)
        kw = dict(frame=map_frame(), bounds=(-14.0,) * 3 + (14.0,) * 3, min_weight=1.0)
        plain, small, both = (str(tmp_path / d / "mesh.ply") for d in ("plain", "small", "both"))
        capsys.readouterr()
        meta0 = mesh_model.build_mesh(gaussians, cams, args, plain, 1.0, **kw)
        line0 = capsys.readouterr().out
        meta1 = mesh_model.build_mesh(gaussians, cams, args, small, 1.0, decimate_cell=2.0, **kw)
        line1 = capsys.readouterr().out
        meta2 = mesh_model.build_mesh(gaussians, cams, args, both, 1.0, decimate_cell=2.0, keep_components=1, **kw)
        line2 = capsys.readouterr().out
    finally:
        utils.set_args(utils.default_args())
    # without the option: what the extraction returned, no word of the decimation anywhere
    v0, c0, f0 = io_ply.load_mesh_ply(plain)
    assert len(extracted) == 3 and all(np.array_equal(a, b) for a, b in zip((v0, c0, f0), extracted[0]))
    assert len(f0) > 0 and meta0 == json.load(open(plain[:-4] + ".json"))
    assert "decimation" not in meta0 and "decimated" not in line0 and meta0["faces"] == len(f0)
    # with it: the reference applied to the first mesh
    wv, wc, wf, wrep = D.decimate(v0, c0, f0, 2.0)
    v1, c1, f1 = io_ply.load_mesh_ply(small)
    print(line1.strip(), "|", wrep)
    assert np.array_equal(v1, wv) and np.array_equal(c1, wc) and np.array_equal(f1, wf)
    assert meta1 == json.load(open(small[:-4] + ".json")) and meta1["decimation"] == wrep
    assert 0 < len(f1) < len(f0) and meta1["vertices"] == len(v1) and meta1["faces"] == len(f1) and "cleanup" not in meta1
    assert {k: v for k, v in meta1.items() if k not in ("vertices", "faces", "decimation")} == \
           {k: v for k, v in meta0.items() if k not in ("vertices", "faces")}
    assert " decimated {} -> {} vertices {} -> {} faces cell 2 -> ".format(len(v0), len(v1), len(f0), len(f1)) in line1
    # after the cleanup, which sees the full-resolution mesh
    kv, kc, kf, krep = M.clean(v0, c0, f0, keep_largest=1)
    wv, wc, wf, wrep = D.decimate(kv, kc, kf, 2.0)
    v2, c2, f2 = io_ply.load_mesh_ply(both)
    assert np.array_equal(v2, wv) and np.array_equal(c2, wc) and np.array_equal(f2, wf)
    assert meta2["decimation"] == wrep and meta2["cleanup"]["components_kept"] == 1 and meta2["faces"] == len(f2)
    assert " components " in line2 and " decimated {} -> {} vertices".format(len(kv), len(v2)) in line2
    # the tool on the first file writes the bytes of the second export, and of the third with the filter as well
    for extra, want in (([], small), (["--keep_largest", "1"], both)):
        tool = str(tmp_path / ("tool%d" % len(extra)) / "out.ply")
        capsys.readouterr()
        assert mesh_clean.main(["-i", plain, "-o", tool, "--decimate_cell", "2.0"] + extra) == 0
        line = capsys.readouterr().out
        assert line.startswith("mesh cleanup:") and " decimated {} ->".format(len(kv) if extra else len(v0)) in line, line
        assert open(tool, "rb").read() == open(want, "rb").read()
        assert json.load(open(tool[:-4] + ".json")) == json.load(open(want[:-4] + ".json"))


def test_trainer_decimates(dev, tmp_path):
    """trainer --mesh_voxel --mesh_decimate_cell, in the shape of test_gpu_mesh_clean.test_trainer_keeps_one_component."""
    from clm_gs_amd import io_ply, trainer
    from tests.test_gpu_exposure import _tiny_scene
    work = _tiny_scene(tmp_path)
    counts = {}
    for name, kw in (("plain", {}), ("small", dict(mesh_decimate_cell=1.5))):
        out = tmp_path / name
        trainer.train_from_colmap(str(work), str(out), strategy="clm_offload", iterations=8, bsz=4,
                                  disable_auto_densification=True, mesh_voxel=0.5, mesh_min_weight=1.0, **kw)
        verts, colours, faces = io_ply.load_mesh_ply(str(out / "mesh.ply"))
        meta = json.load(open(out / "mesh.json"))
        log = open(out / "python_ws=1_rk=0.log").read()
        assert meta["faces"] == len(faces) and meta["vertices"] == len(verts)
        assert ("decimation" in meta) == bool(kw) and (" decimated " in log) == bool(kw)
        counts[name] = (len(faces), meta)
    meta = counts["small"][1]
    print("trainer mesh:", counts["plain"][0], "->", counts["small"][0], meta["decimation"])
    assert 0 < counts["small"][0] < counts["plain"][0]
    assert meta["decimation"]["cell"] == 1.5 and meta["decimation"]["faces"] == counts["small"][0] < meta["decimation"]["faces_in"]
    assert " decimated {} -> {} vertices".format(meta["decimation"]["vertices_in"], meta["vertices"]) in log
