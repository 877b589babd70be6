"""Mesh evaluation on the device ("Mesh evaluation"): csrc/mesh_distance.hip through
clm_kernels.mesh_sample / mesh_distance_grid / mesh_distance, mesh_eval.evaluate, the eval_mesh tool and the mesh export,
against the numpy restatement of the contract (tests/mesh_eval_reference.py).  Samples, distances and primitive indices are
compared exactly (array_equal), for every cell size; the float64 sums of the metrics within rtol 1e-9 (the rounding bound of
a sum of at most 2^20 non-negative terms in any order is about 2^20 x 2^-53 = 1.2e-10)."""
import functools
import json
import math

import numpy as np
import pytest
import torch

from tests import mesh_eval_reference as E
from tests import tsdf_reference as R
from tests.test_mesh_decimate_cpu import box_sdf
from tests.test_mesh_eval_cpu import distance_cases, mixed_mesh

pytestmark = pytest.mark.gpu


def _dev(dev, verts, faces=None):
    v = torch.from_numpy(np.ascontiguousarray(verts, dtype=np.float32).reshape(-1, 3)).to(dev)
    return v, None if faces is None else torch.from_numpy(np.ascontiguousarray(faces, dtype=np.int32).reshape(-1, 3)).to(dev)


@functools.lru_cache(maxsize=None)
def analytic(name):
    """(verts, faces) of an analytic 20^3 grid through the numpy extraction, once."""
    sdf = dict(sphere=R.sphere_sdf, box=box_sdf)[name]()
    verts, _, faces = R.extract(R.grid_from_sdf(sdf), 2.0, R.G2W)[:3]
    return verts, faces


@functools.lru_cache(maxsize=None)
def sphere_report():
    """The reference's report of the sphere against a shifted copy of itself, once."""
    verts, faces = analytic("sphere")
    shifted = (verts + np.float32([0.03, -0.02, 0.01])).astype(np.float32)
    return shifted, E.evaluate(verts, faces, shifted, faces, taus=[0.05, 0.02], spacing=0.05, max_distance=0.03)


def _same_report(got, want):
    from clm_gs_amd import mesh_eval
    assert tuple(got) == mesh_eval.REPORT_KEYS
    for k in want:
        if k in E.SUM_KEYS:
            assert np.allclose(got[k], want[k], rtol=1e-9, atol=0.0), (k, got[k], want[k])
        else:
            assert got[k] == want[k], (k, got[k], want[k])
    assert got["ref_cell"] > 0 and got["mesh_cell"] > 0 and got["ref_pairs"] >= 1 and got["mesh_pairs"] >= got["faces"] - got["degenerate_faces"]


# ------------------------------------------------------------------------------------------------ 1. the sampler
def _check_sample(dev, verts, faces, spacing, what):
    from clm_gs_amd import clm_kernels
    v, f = _dev(dev, verts, faces)
    got = clm_kernels.mesh_sample(v, f, spacing)
    want = E.sample(verts, faces, spacing)
    for g, w, name in zip(got, want, ("points", "face", "weight", "area")):
        g = g.cpu().numpy()
        assert g.dtype == w.dtype and g.shape == w.shape and np.array_equal(g, w), f"{what}: {name}"
    return got, want


def test_sampler_on_extracted_meshes(dev):
    from clm_gs_amd import clm_kernels
    for name, counts in (("sphere", (746, 1488)), ("box", (602, 1200))):
        sdf = dict(sphere=R.sphere_sdf, box=box_sdf)[name]()
        verts, _, faces = (t.cpu().numpy() for t in clm_kernels.tsdf_extract(torch.from_numpy(R.grid_from_sdf(sdf)).to(dev), 2.0, R.G2W))
        assert (len(verts), len(faces)) == counts
        for spacing in (0.05, 0.5):
            got, want = _check_sample(dev, verts, faces, spacing, f"{name}, spacing {spacing}")
            assert len(want[0]) >= len(faces)


def test_sampler_on_faces_of_every_size(dev):
    verts, faces = mixed_mesh()
    got, want = _check_sample(dev, verts, faces, 0.125, "mixed")
    assert np.bincount(want[1], minlength=len(faces)).tolist() == [0, 1, 0, 63, 64, 0, 65, 5000, 0]
    a, b = (_check_sample(dev, verts, faces, 0.125, "again")[0] for _ in range(2))
    assert all(torch.equal(x, y) for x, y in zip(a, b))


def test_sampler_refusals(dev):
    from clm_gs_amd import _lib, clm_kernels
    verts, faces = mixed_mesh()
    v, f = _dev(dev, verts, faces)
    with pytest.raises(ValueError, match=r"spacing 0.125 gives 5193 samples, above max_samples 1000; a spacing of [0-9.]+ fits") as e:
        clm_kernels.mesh_sample(v, f, 0.125, max_samples=1000)
    fits = float(str(e.value).split("a spacing of ")[1].split(" fits")[0])
    assert 0.125 < fits < 0.5 and 900 <= len(clm_kernels.mesh_sample(v, f, fits, max_samples=1000)[0]) <= 1000
    with pytest.raises(ValueError, match="above --max_samples 4; no spacing fits: 5 faces have an area"):
        clm_kernels.mesh_sample(v, f, 0.125, max_samples=4, name="--max_samples")
    for bad in (0, -1.0, float("nan"), float("inf"), None, "1"):
        with pytest.raises(ValueError, match="spacing must be a positive finite number"):
            clm_kernels.mesh_sample(v, f, bad)
    with pytest.raises(_lib.ClmgsError, match="verts must be a tensor on the device"):
        clm_kernels.mesh_sample(v.cpu(), f, 0.1)
    with pytest.raises(_lib.ClmgsError, match=r"outside \[0, 27\)"):
        clm_kernels.mesh_sample(v, f + 1, 0.1)
    empty = clm_kernels.mesh_sample(v, f[:0], 0.1)
    assert [tuple(t.shape) for t in empty] == [(0, 3), (0,), (0,), (0,)]
    none = clm_kernels.mesh_sample(v, f[[0, 2, 5]].contiguous(), 0.1)  # degenerate faces only
    assert none[0].shape == (0, 3) and none[3].shape == (3,)


# ------------------------------------------------------------------------------------------------ 2. the distance
def _check_distance(dev, verts, faces, queries, max_distance, cells, what):
    """dist and prim == the brute force, bit for bit, for every cell size of `cells` (None = the default, a float = that
    size, ("x", s) = s times the default).  -> the device grids."""
    from clm_gs_amd import clm_kernels
    v, f = _dev(dev, verts, faces)
    q = torch.from_numpy(np.ascontiguousarray(queries, dtype=np.float32)).to(dev)
    want = E.brute(queries, verts, faces, max_distance)
    default, out = None, []
    for cell in cells:
        if isinstance(cell, tuple):
            cell = cell[1] * default
        grid = clm_kernels.mesh_distance_grid(v, f, cell)
        default = grid.h if default is None else default
        assert cell is None or grid.h == cell
        dist, prim, evaluated = clm_kernels.mesh_distance(q, grid, max_distance, with_evaluated=True)
        assert dist.dtype == torch.float32 and prim.dtype == torch.int32 and dist.shape == prim.shape == (len(queries),)
        dist, prim = dist.cpu().numpy(), prim.cpu().numpy()
        bad = np.nonzero((dist != want[0]) | (prim != want[1]))[0]
        assert len(bad) == 0, (f"{what}, h {grid.h:g} dims {grid.dims}: {len(bad)} of {len(queries)} queries differ, first {bad[:1]}: "
                               f"{dist[bad[:1]]} {prim[bad[:1]]} != {want[0][bad[:1]]} {want[1][bad[:1]]}")
        assert int(evaluated.max()) <= grid.pairs
        out.append((grid, evaluated.cpu().numpy()))
    return out, want


def test_distance_boundary_cases_at_every_cell_size(dev):
    for name, verts, faces, queries, max_distance, h in distance_cases():
        grids, want = _check_distance(dev, verts, faces, queries, max_distance, (None, ("x", 0.5), ("x", 4.0), h, 0.5 * h), name)
        if name == "a grid of one cell":
            assert grids[3][0].dims == (1, 1, 1)
        if name == "integer lattice, h = 1":
            assert grids[3][0].dims == (5, 5, 1) and not want[0][:25].any()
        if name == "random":
            assert grids[0][0].degenerate == 9 and grids[0][0].primitives == 51
        if name == "points":
            assert grids[0][0].degenerate == 1 and grids[0][0].faces is None


@pytest.mark.parametrize("P", [1, 63, 64, 257, 4000])
def test_distance_query_counts_both_instantiations(dev, P):
    verts, faces = analytic("sphere")
    rng = np.random.default_rng(P)
    queries = (rng.normal(size=(P, 3)) * 0.7).astype(np.float32)
    queries[::5] = (queries[::5] * 3).astype(np.float32)
    if P == 4000:  # half of them near the surface, as the samples of an evaluation are
        queries[2000:] = (verts[rng.integers(0, len(verts), size=2000)] + rng.normal(size=(2000, 3)) * 0.01).astype(np.float32)
    if P >= 63:
        queries[7], queries[11] = [np.nan, 0, 0], [0, -np.inf, 0]
        queries[13:20] = verts[100:107]  # on vertices: up to six faces tie
    for prims in (faces, None):
        for max_distance in ((math.inf, 0.5) if P < 4000 else (0.5,)):
            grids, want = _check_distance(dev, verts, prims, queries, max_distance, (None, ("x", 0.5), ("x", 4.0)),
                                          f"sphere {'triangles' if prims is not None else 'points'}, P {P}")
        if P == 4000:
            # the stopping rule at work: a lane whose best distance is below h SLACK stops after shell 1 -- it cannot stop
            # after shell 0, whose reach is zero -- so it has evaluated exactly the pairs of the 3 x 3 x 3 cells around its own
            for grid, evaluated in grids:
                nx, ny, nz = grid.dims
                padded = np.pad(np.diff(grid.cell_start.cpu().numpy()).reshape(nz, ny, nx), 1)
                box = sum(padded[dz:dz + nz, dy:dy + ny, dx:dx + nx] for dz in range(3) for dy in range(3) for dx in range(3))
                c = [E.cell_index(np.nan_to_num(queries[:, d]), grid.origin[d], grid.h, grid.dims[d]) for d in range(3)]
                near = np.isfinite(queries).all(axis=1) & (want[0].astype(np.float64) < 0.99 * grid.h)
                assert near.sum() >= 1000 and np.array_equal(evaluated[near], box[c[2][near], c[1][near], c[0][near]])
                print(f"sphere {'triangles' if prims is not None else 'points'}, h {grid.h:g} dims {grid.dims} pairs {grid.pairs}: "
                      f"primitives evaluated per query {evaluated.mean():.1f} ({evaluated[near].mean():.1f} over the {near.sum()} "
                      f"within h of the surface) of {grid.primitives}")


def test_grid_refusals_and_empties(dev):
    from clm_gs_amd import _lib, clm_kernels
    verts, faces = analytic("sphere")
    v, f = _dev(dev, verts, faces)
    q = v[:10].contiguous()
    with pytest.raises(ValueError, match=r"cell 1e-07 breaks the limits of the grid .*; [0-9.e-]+ fits") as e:
        clm_kernels.mesh_distance_grid(v, f, 1e-7)
    fits = float(str(e.value).rsplit("; ", 1)[1].split(" fits")[0])
    assert clm_kernels.mesh_distance_grid(v, f, fits * 1.001).h == fits * 1.001
    with pytest.raises(ValueError, match=r"--cell 0.01 breaks the limits .* grid_gb 0.0001"):
        clm_kernels.mesh_distance_grid(v, f, 0.01, grid_gb=1e-4, name="--cell")
    with pytest.raises(ValueError, match="no cell size fits grid_gb 1e-06: 1488 primitives need 47616 B"):
        clm_kernels.mesh_distance_grid(v, f, None, grid_gb=1e-6)
    small = clm_kernels.mesh_distance_grid(v, f, None, grid_gb=1e-4)  # the default gives way to the limit
    assert small.pairs * clm_kernels.MESH_GRID_PAIR_BYTES <= 1e5
    assert np.array_equal(clm_kernels.mesh_distance(q, small)[0].cpu().numpy(), E.brute(verts[:10], verts, faces)[0])
    for bad in (0, -1.0, float("nan"), float("inf"), "1"):
        with pytest.raises(ValueError, match="cell must be a positive finite number"):
            clm_kernels.mesh_distance_grid(v, f, bad)
    grid = clm_kernels.mesh_distance_grid(v, f)
    for bad in (0, -1.0, float("nan"), None):
        with pytest.raises(ValueError, match="max_distance must be a positive number"):
            clm_kernels.mesh_distance(q, grid, bad)
    with pytest.raises(ValueError, match="grid must come from mesh_distance_grid"):
        clm_kernels.mesh_distance(q, None)
    with pytest.raises(_lib.ClmgsError, match="points must be a tensor on the device"):
        clm_kernels.mesh_distance(q.cpu(), grid)
    with pytest.raises(_lib.ClmgsError, match=r"outside \[0, 746\)"):
        clm_kernels.mesh_distance_grid(v, f + 1)
    # nothing to measure against: every query is answered (+inf, -1)
    for g in (clm_kernels.mesh_distance_grid(v, f[:0]), clm_kernels.mesh_distance_grid(v, torch.zeros_like(f)),
              clm_kernels.mesh_distance_grid(torch.full_like(v, float("nan")))):
        dist, prim = clm_kernels.mesh_distance(q, g)
        assert g.primitives == 0 and g.pairs == 0 and torch.isinf(dist).all() and (prim == -1).all()
    dist, prim = clm_kernels.mesh_distance(q[:0], grid)
    assert dist.shape == prim.shape == (0,)
    # the C entry itself: sizes and a grid beyond the limits are CLMGS_EINVAL, before any launch
    L, p = _lib.lib(), _lib.dptr
    d, w = torch.empty(10, device=dev), torch.empty(10, dtype=torch.int32, device=dev)
    args = lambda P, gx, h, md: (_lib.stream(), P, p(q), 746, 1488, p(v), p(f), 0.0, 0.0, 0.0, h, gx, 1, 1, p(grid.cell_start),
                                 p(grid.pair_prim), grid.pairs, md, p(d), p(w), None)
    for bad in (args(0, 1, 1.0, 1.0), args(10, 0, 1.0, 1.0), args(10, (1 << 20) + 1, 1.0, 1.0), args(10, 1, 0.0, 1.0),
                args(10, 1, float("nan"), 1.0), args(10, 1, 1.0, 0.0), args(10, 1, 1.0, float("nan"))):
        with pytest.raises(_lib.ClmgsError):
            _lib.check(L.clmgs_mesh_distance(*bad))
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ 3. the metrics
def test_evaluate_equals_the_reference(dev):
    from clm_gs_amd import mesh_eval
    verts, faces = analytic("sphere")
    shifted, want = sphere_report()
    v, f = _dev(dev, verts, faces)
    s, _ = _dev(dev, shifted)
    timings = {}
    got = mesh_eval.evaluate(v, f, s, f, [0.05, 0.02], 0.05, 0.03, timings=timings)
    _same_report(got, want)
    assert 0 < got["mesh_beyond"] < got["mesh_queries"] and 0 < got["precision"][1] < got["precision"][0] <= 1
    assert set(timings) == {"sampling", "grid_reference", "distance_mesh_to_reference", "grid_mesh", "distance_reference_to_mesh"}
    other = mesh_eval.evaluate(v, f, s, f, [0.05, 0.02], 0.05, 0.03, cell=0.3)  # another grid: the same distances, so the same sums
    assert other["ref_cell"] == other["mesh_cell"] == 0.3 and other["ref_pairs"] != got["ref_pairs"]
    assert {k: x for k, x in other.items() if k not in E.GRID_KEYS} == {k: x for k, x in got.items() if k not in E.GRID_KEYS}
    # a reference of points, every third, inside a crop box that halves both sides
    bounds = [0.0, -2.0, -2.0, 2.0, 2.0, 2.0]
    got = mesh_eval.evaluate(v, f, s, None, [0.05], 0.1, bounds=bounds, ref_every=3)
    want = E.evaluate(verts, faces, shifted, None, [0.05], 0.1, bounds=bounds, ref_every=3)
    _same_report(got, want)
    assert got["ref_samples"] == 249 and got["ref_queries"] < 249 and got["mesh_queries"] < got["mesh_samples"]
    # the squares: the analytic answer
    (v0, f0), (v1, f1) = E.squares(0.25)
    got = mesh_eval.evaluate(*_dev(dev, v0, f0), *_dev(dev, v1, f1), [0.5, 0.25], 1 / 32)
    _same_report(got, E.evaluate(v0, f0, v1, f1, [0.5, 0.25], 1 / 32))
    assert got["accuracy"] == got["completeness"] == got["chamfer"] == 0.25 and got["fscore"] == [1.0, 0.0]
    assert got["mesh_samples"] == 1024 and got["spacing"] == 1 / 32 and got["max_distance"] == 5.0


def test_evaluate_refusals(dev):
    from clm_gs_amd import mesh_eval
    verts, faces = analytic("sphere")
    v, f = _dev(dev, verts, faces)
    flat = torch.zeros_like(f)
    for args, kw, match in (((v, f[:0], v, None), {}, "an empty mesh"), ((v[:0], f[:0], v, None), {}, "an empty mesh"),
                            ((v, flat, v, None), {}, "an empty mesh"), ((v, f, v[:0], None), {}, "an empty reference"),
                            ((v, f, v, f[:0]), {}, "an empty reference"), ((v, f, v, flat), {}, "an empty reference"),
                            ((v, f, torch.full_like(v, float("inf")), None), {}, "an empty reference"),
                            ((v, f, v, None), dict(ref_every=747), "ref_every 747 is larger than the reference's 746 points"),
                            ((v, f, v, f), dict(ref_every=2), "ref_every applies to a reference without faces"),
                            ((v, f, v, None), dict(bounds=[5, 5, 5, 6, 6, 6]), "no mesh sample lies inside bounds"),
                            ((v, f, v, None), dict(max_samples=100), "above max_samples 100"),
                            ((v, f, v, None), dict(cell=1e-8), "cell 1e-08 breaks the limits"),
                            ((v, f, v, None), dict(spacing=0), "spacing must be a positive finite number")):
        with pytest.raises(ValueError, match=match):
            mesh_eval.evaluate(*args, [0.05], **kw)


# ------------------------------------------------------------------------------------------------ 4. the tools
def test_eval_mesh_end_to_end(dev, tmp_path, capsys):
    from clm_gs_amd import clm_kernels, io_ply, mesh_eval
    verts, faces = analytic("sphere")
    shifted, want = sphere_report()
    colours = np.full((len(verts), 3), 200, dtype=np.uint8)
    normals = (verts / np.linalg.norm(verts, axis=1, keepdims=True)).astype(np.float32)
    mesh, ref, err = (str(tmp_path / n) for n in ("mesh.ply", "ref.ply", "out/err.ply"))
    io_ply.save_mesh_ply(mesh, verts, colours, faces, normals)
    io_ply.save_mesh_ply(ref, shifted, colours, faces)
    capsys.readouterr()
    assert mesh_eval.main(["-i", mesh, "-r", ref, "--tau", "0.05", "0.02", "--spacing", "0.05", "--max_distance", "0.03",
                           "--error_mesh", err]) == 0
    line = capsys.readouterr().out
    record = json.load(open(tmp_path / "mesh.eval.json"))
    assert tuple(record) == ("mesh", "reference") + mesh_eval.REPORT_KEYS and record["mesh"] == mesh and record["reference"] == ref
    _same_report({k: record[k] for k in mesh_eval.REPORT_KEYS}, want)
    assert line.startswith(mesh_eval.summary_line(record) + " in ") and line.rstrip().endswith("-> " + str(tmp_path / "mesh.eval.json"))
    assert " | tau 0.05 precision " in line and " | tau 0.02 precision " in line
    ev, ec, ef, en = io_ply.load_mesh_ply(err, with_normals=True)
    d = E.brute(verts, shifted, faces, 0.03)[0]
    assert np.array_equal(ev, verts) and np.array_equal(ef, faces) and np.array_equal(en, normals)
    assert np.array_equal(ec, E.error_colours(d, 0.05)) and np.isinf(d).any() and len(np.unique(ec[:, 0])) > 10
    # a cloud as the reference, a crop, -o, and no normals in the input: none in the error mesh
    out = str(tmp_path / "deep" / "eval.json")
    io_ply.save_mesh_ply(mesh, verts, colours, faces)
    cloud = str(tmp_path / "cloud.ply")
    io_ply.save_mesh_ply(cloud, shifted[::3], colours[::3], faces[:0])
    assert mesh_eval.main(["-i", mesh, "-r", cloud, "--tau", "0.05", "-o", out,
                           "--bounds", "0", "-2", "-2", "2", "2", "2", "--cell", "0.25", "--error_mesh", err]) == 0
    record = json.load(open(out))
    assert record["bounds"] == [0.0, -2.0, -2.0, 2.0, 2.0, 2.0] and record["ref_cell"] == record["mesh_cell"] == 0.25
    assert record["spacing"] == 0.025 and record["max_distance"] == 0.5 and record["mesh_queries"] < record["mesh_samples"]
    assert record["ref_faces"] is None and record["ref_points"] == record["ref_samples"] == 249
    assert len(io_ply.load_mesh_ply(err, with_normals=True)) == 4 and io_ply.load_mesh_ply(err, with_normals=True)[3] is None
    with pytest.raises(SystemExit, match="--ref_every applies to a reference without faces"):
        mesh_eval.main(["-i", mesh, "-r", ref, "--tau", "0.05", "--ref_every", "2"])
    with pytest.raises(SystemExit, match="--cell 1e-09 breaks the limits"):
        mesh_eval.main(["-i", mesh, "-r", ref, "--tau", "0.05", "--cell", "1e-9"])


def test_mesh_export_with_a_reference(dev, tmp_path, capsys):
    from clm_gs_amd import io_ply, mesh_model, utils
    from clm_gs_amd.render_ortho import map_frame
    from tests.test_gpu_mesh_clean import _shell_scene
    try:
        gaussians, cams, args = _shell_scene(tmp_path)
        kw = dict(frame=map_frame(), bounds=(-14.0,) * 3 + (14.0,) * 3, min_weight=1.0)
        plain, evaluated = (str(tmp_path / d / "mesh.ply") for d in ("plain", "evaluated"))
        capsys.readouterr()
        meta0 = mesh_model.build_mesh(gaussians, cams, args, plain, 1.0, **kw)
        line0 = capsys.readouterr().out
        v0, c0, f0 = io_ply.load_mesh_ply(plain)
        ref = str(tmp_path / "reference.ply")  # a cloud: every 20th vertex, displaced
        cloud = (v0[::20] + np.float32([0.4, 0.0, -0.3])).astype(np.float32)
        io_ply.save_mesh_ply(ref, cloud, np.zeros((len(cloud), 3), dtype=np.uint8), np.zeros((0, 3), dtype=np.int32))
        meta1 = mesh_model.build_mesh(gaussians, cams, args, evaluated, 1.0, reference=ref, eval_taus=[1.0, 0.5],
                                      eval_spacing=2.0, **kw)
        line1 = capsys.readouterr().out
    finally:
        utils.set_args(utils.default_args())
    # without the flag: the keys and the line of before, no word of an evaluation
    assert len(f0) > 0 and "evaluation" not in meta0 and " F " not in line0 and "@tau" not in line0
    assert open(plain[:-4] + ".json").read() == json.dumps(meta0, indent=1)
    assert list(meta0) == ["east", "north", "up", "bounds", "voxel", "trunc", "grid", "min_weight", "alpha_min", "depth_max",
                           "vertices", "faces", "cameras", "camera_names"]
    # with it: the same mesh.ply, the report of the reference, the words at the end of the line
    assert open(evaluated, "rb").read() == open(plain, "rb").read()
    assert meta1 == json.load(open(evaluated[:-4] + ".json")) and {k: v for k, v in meta1.items() if k != "evaluation"} == meta0
    want = E.evaluate(v0, f0, cloud, None, [1.0, 0.5], 2.0)
    print(line1.strip(), "|", {k: want[k] for k in E.SUM_KEYS})
    _same_report(meta1["evaluation"], want)
    assert meta1["evaluation"]["max_distance"] == 10.0 and meta1["evaluation"]["ref_faces"] is None
    words = " F {:.4f}@tau 1 F {:.4f}@tau 0.5 -> ".format(*meta1["evaluation"]["fscore"])
    assert words in line1 and line1.replace(words, " -> ").split(" vertices ")[1].replace(evaluated, plain) == line0.split(" vertices ")[1]
