"""Mesh evaluation without a GPU ("Mesh evaluation"): csrc/mesh_distance_math.h, compiled for the
host, against the numpy restatement (tests/mesh_eval_reference.py) bit for bit; the sampler's invariants; the restated
grid walk -- binning, shells and the stopping rule -- against the brute force over all primitives, on the boundary cases
the GPU test runs; the metrics on shapes whose answer is known; the reference loader; and every refusal, by name, before
anything is read."""
import ctypes
import json
import math
import os
import subprocess

import numpy as np
import pytest

from tests import mesh_eval_reference as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F64 = np.float64


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("mesh_distance_math") / "shim.so")
    subprocess.check_call(["g++", "-O2", "-ffp-contract=off", "-shared", "-fPIC", "-I", os.path.join(ROOT, "clm_gs_amd", "csrc"),
                           os.path.join(ROOT, "tests", "host_shim", "mesh_distance_math_shim.cpp"), "-o", out])
    return ctypes.CDLL(out)


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def _c(a, dtype=F64):
    return np.ascontiguousarray(a, dtype=dtype)


def shim_closest(shim, p, a, b, c):
    p, a, b, c = (_c(np.broadcast_to(x, np.broadcast_shapes(np.shape(p), np.shape(a)))) for x in (p, a, b, c))
    out = np.empty(len(p), dtype=F64)
    shim.shim_closest_d2(len(p), _p(p), _p(a), _p(b), _p(c), _p(out))
    return out


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


# ------------------------------------------------------------------------------------------------ 1. the header
def test_closest_point_equals_the_restatement_on_random_triangles(shim):
    rng = np.random.default_rng(0)
    n = 40000
    scale = 10.0 ** rng.integers(-3, 4, size=(n, 1))
    a, b, c = (rng.normal(size=(n, 3)).astype(np.float32).astype(F64) * scale for _ in range(3))
    p = (rng.normal(size=(n, 3)) * 2).astype(np.float32).astype(F64) * scale
    got = shim_closest(shim, p, a, b, c)
    want, region = E.closest_d2(p, a, b, c, with_region=True)
    assert sorted(set(region.tolist())) == list(range(7))  # every branch is reached
    assert same_bits(got, want)
    out = np.empty(n, dtype=F64)
    shim.shim_point_d2(n, _p(_c(p)), _p(_c(a)), _p(out))
    assert same_bits(out, E.point_d2(p, a))


def test_one_constructed_case_per_voronoi_region(shim):
    a, b, c = (np.array(x, dtype=F64) for x in ([0, 0, 0], [1, 0, 0], [0, 1, 0]))
    cases = [("A", [-1, -1, 1], 3.0), ("B", [2, -1, 0.5], 2.25), ("AB", [0.5, -1, 0.5], 1.25), ("C", [-1, 2, 0.5], 2.25),
             ("AC", [-1, 0.5, 0.5], 1.25), ("BC", [1, 1, 0.5], 0.75), ("interior", [0.25, 0.25, 1], 1.0)]
    p = np.array([x[1] for x in cases], dtype=F64)
    want, region = E.closest_d2(p, a, b, c, with_region=True)
    assert [E.REGIONS[r] for r in region] == [x[0] for x in cases]
    assert want.tolist() == [x[2] for x in cases]
    assert same_bits(shim_closest(shim, p, a, b, c), want)


def test_points_on_edges_and_vertices(shim):
    rng = np.random.default_rng(1)
    n = 5000
    a, b, c = (rng.integers(-50, 50, size=(n, 3)).astype(F64) for _ in range(3))
    ok = E.area_ok(E.face_area(a, b, c))
    a, b, c = a[ok], b[ok], c[ok]
    for p in (a, b, c, (a + b) / 2, (a + c) / 2, (b + c) / 2, (a + b + c + a) / 4):
        got, want = shim_closest(shim, p, a, b, c), E.closest_d2(p, a, b, c)
        assert same_bits(got, want)
    for p in (a, b, c):  # a corner is at distance exactly zero
        assert not shim_closest(shim, p, a, b, c).any()
    assert (E.closest_d2((a + b) / 2, a, b, c) <= 1e-20).all()


def test_degenerate_faces_are_flagged_and_counts_agree(shim):
    rng = np.random.default_rng(2)
    n = 3000
    a, b = (rng.normal(size=(n, 3)).astype(np.float32).astype(F64) for _ in range(2))
    c = rng.normal(size=(n, 3)).astype(np.float32).astype(F64)
    c[0::6] = a[0::6]                                  # c == a
    b[1::6] = a[1::6]                                  # b == a
    c[2::6] = a[2::6] + 2.0 * (b[2::6] - a[2::6])      # collinear (exactly, where the doubling is exact)
    b[3::6], c[3::6] = a[3::6], a[3::6]                # a point
    a[4::600] = np.nan
    b[5::600] = np.inf
    for spacing in (0.05, 1.0, 1e-9):
        area, ok, count = np.empty(n, dtype=F64), np.empty(n, dtype=np.uint8), np.empty(n, dtype=np.int64)
        shim.shim_face_area(n, _p(a), _p(b), _p(c), ctypes.c_double(spacing), _p(area), _p(ok), _p(count))
        want = E.face_area(a, b, c)
        assert same_bits(area, want) and np.array_equal(ok.astype(bool), E.area_ok(want))
        assert np.array_equal(count, E.sample_count(want, spacing))
        assert not ok[0::6].any() and not ok[1::6].any() and not ok[3::6].any() and not ok[4::600].any() and not ok[5::600].any()
        assert (count[~ok.astype(bool)] == 0).all() and (count[ok.astype(bool)] >= 1).all()
    assert count.max() == E.MAX_FACE_SAMPLES  # (spacing 1e-9: the cap)
    # Ericson's quotients on a face without area are 0 / 0 (here a == b: the edge AB branch): why such faces are not
    # primitives
    assert np.isnan(E.closest_d2([0.5, 1.0, 0.0], [0, 0, 0], [0, 0, 0], [1, 0, 0]))
    assert np.isnan(shim_closest(shim, np.array([[0.5, 1.0, 0.0]]), np.array([[0.0, 0, 0]]), np.array([[0.0, 0, 0]]),
                                 np.array([[1.0, 0, 0]]))[0])


def test_sample_positions_and_cells(shim):
    rng = np.random.default_rng(3)
    k = np.concatenate([np.arange(10001), rng.integers(0, 1 << 28, size=5000)]).astype(np.int64)
    n = len(k)
    a, b, c = (rng.normal(size=(n, 3)).astype(np.float32).astype(F64) * 3 for _ in range(3))
    uv, out = np.empty((n, 2), dtype=F64), np.empty((n, 3), dtype=np.float32)
    shim.shim_sample_position(n, _p(k), _p(a), _p(b), _p(c), _p(uv), _p(out))
    u, v = E.sample_uv(k)
    assert same_bits(uv[:, 0].copy(), u) and same_bits(uv[:, 1].copy(), v)
    assert same_bits(out, E.sample_position(k, a, b, c))
    assert (u >= 0).all() and (v >= 0).all() and (u + v <= 1).all()
    x = np.concatenate([rng.normal(size=4000) * 5, np.arange(-3, 12).astype(F64), [1e300, -1e300, np.inf, -np.inf]])
    for o, h, g in ((0.0, 1.0, 8), (-2.5, 0.3, 17), (1.0, 1e-3, 1 << 20), (0.0, 7.0, 1)):
        cells = np.empty(len(x), dtype=np.int32)
        shim.shim_cell(len(x), _p(_c(x)), ctypes.c_double(o), ctypes.c_double(h), g, _p(cells))
        assert np.array_equal(cells, E.cell_index(x, o, h, g)) and cells.min() >= 0 and cells.max() <= g - 1
        order = np.argsort(x)
        assert (np.diff(cells[order]) >= 0).all()  # monotone


# ------------------------------------------------------------------------------------------------ 2. the sampler
def mixed_mesh():
    """Faces of 0, 1, 63, 64, 65 and 5000 samples at spacing 0.125, degenerate faces in between."""
    s2 = 0.125 ** 2
    verts, faces = [], []
    for k, n in enumerate((0, 1, 0, 63, 64, 0, 65, 5000, 0)):
        base, x0 = len(verts), 20.0 * k
        if n == 0:  # collinear, coincident, a point
            kind = len(faces) % 3
            pts = [[x0, 0, 0], [x0 + 1, 0, 0], [x0 + 2, 0, 0]] if kind == 0 else \
                [[x0, 0, 0], [x0, 0, 0], [x0, 1, 0]] if kind == 2 else [[x0, 1, 1]] * 3
        else:  # a right triangle of area (n - 0.5) s2
            pts = [[x0, 0, 0.5], [x0 + 2 * (n - 0.5) * s2, 0, 0.5], [x0, 1, 0.5]]
        verts += pts
        faces.append([base, base + 1, base + 2])
    return np.array(verts, dtype=np.float32), np.array(faces, dtype=np.int32)


def test_sampler_restatement():
    verts, faces = mixed_mesh()
    points, face, weight, area = E.sample(verts, faces, 0.125)
    assert np.bincount(face, minlength=len(faces)).tolist() == [0, 1, 0, 63, 64, 0, 65, 5000, 0]
    assert points.dtype == np.float32 and face.dtype == np.int32 and weight.dtype == F64 and area.dtype == F64
    for f in np.nonzero(E.area_ok(area))[0]:
        assert abs(weight[face == f].sum() - area[f]) <= 1e-12 * area[f]
    assert abs(weight.sum() - area[E.area_ok(area)].sum()) <= 1e-12 * weight.sum()
    # every sample lies in its triangle (here: in the plane z = 0.5, inside the right triangle, up to float32 rounding)
    a, b, c = E.corners(verts, faces)
    x = (points[:, 0] - a[face, 0]) / (b[face, 0] - a[face, 0])
    y = points[:, 1].astype(F64)
    assert (points[:, 2] == 0.5).all() and (x >= -1e-6).all() and (y >= 0).all() and (x + y <= 1 + 1e-6).all()


# ------------------------------------------------------------------------------------------------ 3. the grid walk
def _queries(rng, lo, hi, n):
    """Inside, outside and far outside the box, and non-finite ones."""
    size = hi - lo
    q = np.concatenate([rng.uniform(lo, hi, size=(n // 2, 3)), rng.uniform(lo - size, hi + size, size=(n - n // 2 - 8, 3)),
                        rng.uniform(lo - 100 * size, hi + 100 * size, size=(4, 3))]).astype(np.float32)
    bad = np.array([[np.nan, 0, 0], [0, np.inf, 0], [0, 0, -np.inf], [np.nan, np.nan, np.nan]], dtype=np.float32)
    return np.concatenate([q, bad])[rng.permutation(n)]


def _small_triangles(rng, n, lo, hi, size):
    a = rng.uniform(lo, hi, size=(n, 3))
    verts = np.concatenate([a, a + rng.normal(size=(n, 3)) * size, a + rng.normal(size=(n, 3)) * size]).astype(np.float32)
    return verts, np.stack([np.arange(n), np.arange(n) + n, np.arange(n) + 2 * n], axis=1).astype(np.int32)


def distance_cases():
    """(name, verts, faces or None, queries, max_distance, h): the boundary cases of the distance kernel."""
    rng = np.random.default_rng(5)
    cases = []
    verts, faces = _small_triangles(rng, 60, 0.0, 2.0, 0.15)
    faces[::7, 2] = faces[::7, 1]  # degenerate faces in between
    lo, hi = verts.min(0).astype(F64), verts.max(0).astype(F64)
    cases.append(("random", verts, faces, _queries(rng, lo, hi, 257), math.inf, 0.4))
    cases.append(("beyond max_distance", verts, faces, _queries(rng, lo, hi, 64), 0.3, 0.4))
    # integer coordinates and h = 1: every vertex and query on a cell face; queries on shared vertices and edges tie
    n = 4
    gx, gy = np.meshgrid(np.arange(n + 1), np.arange(n + 1), indexing="ij")
    verts = np.stack([gx.ravel(), gy.ravel(), np.zeros(gx.size)], axis=1).astype(np.float32)
    idx = lambda i, j: i * (n + 1) + j
    faces = np.array([t for i in range(n) for j in range(n)
                      for t in ([idx(i, j), idx(i + 1, j), idx(i + 1, j + 1)], [idx(i, j), idx(i + 1, j + 1), idx(i, j + 1)])],
                     dtype=np.int32)
    faces = faces[rng.permutation(len(faces))]  # (so that the smaller index is not the first met)
    on = np.concatenate([verts, verts + [0.5, 0, 0], verts + [0, 0.5, 0], verts + [0.5, 0.5, 0], verts + [0, 0, 2],
                         verts + [0.5, 0.5, -3], verts + [-2, 0, 1], verts + [3, 3, 3]]).astype(np.float32)
    cases.append(("integer lattice, h = 1", verts, faces, on, math.inf, 1.0))
    cases.append(("integer lattice, h = 1, max_distance 2", verts, faces, on, 2.0, 1.0))
    one_v = np.array([[0.25, 0.5, 1.0], [1.75, 0.25, 1.5], [0.5, 2.0, 0.75]], dtype=np.float32)
    one_f = np.array([[0, 1, 2]], dtype=np.int32)
    cases.append(("one triangle", one_v, one_f, _queries(rng, one_v.min(0).astype(F64), one_v.max(0).astype(F64), 63), math.inf, 0.5))
    verts, faces = _small_triangles(rng, 40, 0.0, 2.0, 0.05)
    big = np.array([[-0.5, -0.5, -0.5], [2.5, -0.5, 2.5], [-0.5, 2.5, 2.5]], dtype=np.float32)
    faces = np.concatenate([faces[:20], [[len(verts), len(verts) + 1, len(verts) + 2]], faces[20:]]).astype(np.int32)
    verts = np.concatenate([verts, big]).astype(np.float32)
    cases.append(("one triangle spanning the grid", verts, faces, _queries(rng, np.full(3, -0.5), np.full(3, 2.5), 64), math.inf, 0.35))
    cases.append(("a grid of one cell", verts, faces, _queries(rng, np.full(3, -0.5), np.full(3, 2.5), 64), math.inf, 100.0))
    pts = rng.uniform(0, 2, size=(300, 3)).astype(np.float32)
    pts[150:170] = pts[10:30]  # duplicates: ties go to the smaller index
    pts[40] = [np.nan, 1, 1]   # no primitive
    q = np.concatenate([_queries(rng, np.zeros(3), np.full(3, 2.0), 64), pts[[15, 160, 299, 150]]]).astype(np.float32)
    cases.append(("points", pts, None, q, math.inf, 0.3))
    cases.append(("points, beyond max_distance", pts, None, q, 0.25, 0.3))
    return cases


def test_grid_walk_equals_the_brute_force():
    ties = 0
    for name, verts, faces, queries, max_distance, h in distance_cases():
        want = E.brute(queries, verts, faces, max_distance)
        for scale in (0.5, 1.0, 4.0):
            grid = E.build_grid(verts, faces, h * scale)
            dist, prim, evaluated = E.grid_walk(queries, grid, max_distance)
            assert np.array_equal(dist, want[0]) and np.array_equal(prim, want[1]), (name, scale)
        bad = ~np.isfinite(queries).all(axis=1)
        assert np.isinf(want[0][bad]).all() and (want[1][bad] == -1).all()
        if max_distance < math.inf:
            assert np.isinf(want[0]).sum() > bad.sum(), name  # some finite query is beyond
            assert (want[0][np.isfinite(want[0])] <= max_distance).all()
        if name == "integer lattice, h = 1":
            # a query on a shared vertex ties between up to six faces: the smallest index is reported
            a, b, c, valid = E.primitives(verts, faces)
            d2 = E.closest_d2(queries[:25, None, :].astype(F64), a[None], b[None], c[None])
            ties += int(((d2 == d2.min(axis=1, keepdims=True)).sum(axis=1) > 1).sum())
            assert np.array_equal(want[1][:25], np.argmin(d2, axis=1)) and not want[0][:25].any()
        if name == "points":
            assert want[1][-4:].tolist() == [15, 20, 299, 10] and not want[0][-4:].any()  # duplicates: the smaller index
    assert ties >= 20


def test_the_walk_stops_after_the_first_shell_that_proves_the_minimum():
    """A query whose best distance is below h SLACK stops after shell 1 (never after shell 0, whose reach is zero): it has
    evaluated exactly the pairs of the 3 x 3 x 3 cells around its own."""
    name, verts, faces, queries, max_distance, h = distance_cases()[0]
    grid = E.build_grid(verts, faces, 0.2)
    points = np.asarray(E.sample(verts, faces, 0.1)[0][:60])
    dist, prim, evaluated = E.grid_walk(points, grid)
    assert np.array_equal(dist, E.brute(points, verts, faces)[0]) and (dist < 0.99 * 0.2).all()
    for p, q in enumerate(points):
        c = [int(E.cell_index(q[d], grid["lo"][d], grid["h"], grid["dims"][d])) for d in range(3)]
        box = sum(len(grid["lists"].get((c[0] + dx, c[1] + dy, c[2] + dz), ())) for dx in (-1, 0, 1) for dy in (-1, 0, 1) for dz in (-1, 0, 1))
        assert evaluated[p] == box
    assert evaluated.max() < grid["pairs"]


# ------------------------------------------------------------------------------------------------ 4. metrics
def test_two_squares_have_the_analytic_answer():
    (v0, f0), (v1, f1) = E.squares(0.25)
    points, face, weight, area = E.sample(v0, f0, 1 / 32)
    assert len(points) == 1024 and abs(weight.sum() - 1.0) <= 1e-15 and area.tolist() == [0.5, 0.5]
    dist, prim = E.brute(points, v1, f1)
    assert (dist == np.float32(0.25)).all()
    rep = E.evaluate(v0, f0, v1, f1, taus=[0.5, 0.25], spacing=1 / 32)
    assert rep["accuracy"] == rep["completeness"] == rep["chamfer"] == 0.25
    assert rep["precision"] == [1.0, 0.0] and rep["recall"] == [1.0, 0.0] and rep["fscore"] == [1.0, 0.0]  # strict: d < tau
    assert rep["mesh_samples"] == rep["ref_samples"] == rep["mesh_queries"] == rep["ref_queries"] == 1024
    assert rep["max_distance"] == 5.0 and rep["mesh_beyond"] == rep["ref_beyond"] == 0 and rep["degenerate_faces"] == 0
    capped = E.evaluate(v0, f0, v1, f1, taus=[0.5], spacing=1 / 32, max_distance=0.125)
    assert capped["accuracy"] == capped["completeness"] == 0.125 and capped["mesh_beyond"] == capped["ref_beyond"] == 1024
    assert capped["precision"] == [0.0]
    # a reference of points: its points count with weight one
    rep = E.evaluate(v0, f0, points + np.float32([0, 0, 0.25]), None, taus=[0.5], spacing=1 / 32, ref_every=3)
    assert rep["ref_samples"] == rep["ref_queries"] == 342 and rep["completeness"] == 0.25 and rep["recall"] == [1.0]
    assert 0.25 <= rep["accuracy"] < 0.2501 + 1 / 32


def test_half_coverage_gives_half_recall():
    (v0, f0), (v1, f1) = E.squares(0.0, x1=0.5)
    for tau, proto in ((1 / 64, 0.5146), (1 / 16, 0.5615)):
        rep = E.evaluate(v0, f0, v1, f1, taus=[tau], spacing=1 / 32)
        print(f"half coverage, tau {tau:g}: recall {rep['recall'][0]:.4f} precision {rep['precision'][0]:.4f}")
        assert abs(rep["recall"][0] - (0.5 + tau)) <= 1 / 32
        assert abs(rep["recall"][0] - proto) <= 5e-4
        assert rep["precision"] == [1.0] and rep["accuracy"] <= 1e-15  # (the samples lie in the plane up to rounding)
    inside = E.evaluate(v0, f0, v1, f1, taus=[1 / 64], spacing=1 / 32, bounds=[0, 0, -1, 0.5, 1, 1])
    assert inside["recall"] == [1.0] and inside["ref_queries"] < inside["ref_samples"] == 1024  # the crop drops queries only


def test_error_ramp():
    d = np.array([0.0, 0.0125, 0.05, 0.1, np.inf, 0.0499], dtype=np.float32)
    col = E.error_colours(d, 0.05)
    assert col.dtype == np.uint8 and col[:, 2].tolist() == [0] * 6
    assert col[:, 0].tolist() == [0, 64, 255, 255, 255, 254] and col[:, 1].tolist() == [255, 191, 0, 0, 0, 1]


# ------------------------------------------------------------------------------------------------ 5. the loader
def _write_ply(path, fmt, verts, faces=None, vertex_props=(("x", "float"), ("y", "float"), ("z", "float")), index="int",
               count="uchar", face_name="vertex_indices", corners=3, face_extra=False):
    """A .ply written by hand with numpy: any order and type of vertex properties (the others hold their column number)."""
    np_t = dict(float="<f4", double="<f8", uchar="u1", int="<i4", uint="<u4", short="<i2")
    head = f"ply\nformat {fmt} 1.0\ncomment written by a test\nelement vertex {len(verts)}\n"
    head += "".join(f"property {t} {n}\n" for n, t in vertex_props)
    if faces is not None:
        head += f"element face {len(faces)}\n" + ("property uchar flag\n" if face_extra else "")
        head += f"property list {count} {index} {face_name}\n"
    head += "end_header\n"
    cols = {n: (verts[:, "xyz".index(n)] if n in "xyz" else np.full(len(verts), k)) for k, (n, t) in enumerate(vertex_props)}
    with open(path, "wb") as f:
        f.write(head.encode("ascii"))
        if fmt == "ascii":
            for i in range(len(verts)):
                f.write((" ".join(repr(float(cols[n][i])) if t in ("float", "double") else str(int(cols[n][i]))
                                  for n, t in vertex_props) + "\n").encode())
            for row in (faces if faces is not None else ()):
                f.write((("7 " if face_extra else "") + f"{corners} " + " ".join(str(int(v)) for v in row[:corners]) + "\n").encode())
        else:
            rec = np.empty(len(verts), dtype=[(n, np_t[t]) for n, t in vertex_props])
            for n, t in vertex_props:
                rec[n] = cols[n]
            f.write(rec.tobytes())
            if faces is not None:
                fields = ([("flag", "u1")] if face_extra else []) + [("n", np_t[count]), ("v", np_t[index], (corners,))]
                rec = np.empty(len(faces), dtype=fields)
                rec["n"], rec["v"] = corners, np.asarray(faces)[:, :corners]
                if face_extra:
                    rec["flag"] = 7
                f.write(rec.tobytes())


def test_loader_reads_binary_and_ascii(tmp_path):
    from clm_gs_amd import io_ply
    rng = np.random.default_rng(6)
    verts = rng.normal(size=(50, 3)).astype(np.float32)
    faces = rng.integers(0, 50, size=(30, 4)).astype(np.int32)
    extra = (("red", "uchar"), ("x", "float"), ("nx", "double"), ("z", "float"), ("label", "short"), ("y", "float"), ("w", "int"))
    doubles = (("x", "double"), ("y", "double"), ("z", "double"))
    path = str(tmp_path / "r.ply")
    for fmt in ("binary_little_endian", "ascii"):
        for props in ((("x", "float"), ("y", "float"), ("z", "float")), extra, doubles):
            _write_ply(path, fmt, verts, None, props)
            points, none = io_ply.load_reference_ply(path)
            assert none is None and points.dtype == np.float32 and points.flags.c_contiguous and np.array_equal(points, verts)
            for kw in (dict(), dict(index="uint", count="int", face_name="vertex_index"), dict(face_extra=True),
                       dict(index="uchar")):
                _write_ply(path, fmt, verts, faces, props, **kw)
                points, got = io_ply.load_reference_ply(path)
                assert np.array_equal(points, verts) and got.dtype == np.int32 and np.array_equal(got, faces[:, :3])
        _write_ply(path, fmt, verts, faces[:0])
        assert io_ply.load_reference_ply(path)[1] is None  # zero faces: a cloud
    # the project's own meshes are references too, with and without normals
    colours = np.zeros((50, 3), dtype=np.uint8)
    for normals in (None, verts):
        io_ply.save_mesh_ply(path, verts, colours, faces[:, :3], normals)
        points, got = io_ply.load_reference_ply(path)
        assert np.array_equal(points, verts) and np.array_equal(got, faces[:, :3])


def test_loader_refusals(tmp_path):
    from clm_gs_amd import io_ply
    rng = np.random.default_rng(7)
    verts = rng.normal(size=(20, 3)).astype(np.float32)
    faces = rng.integers(0, 20, size=(9, 4)).astype(np.int32)
    path = str(tmp_path / "bad.ply")

    def refused(match):
        with pytest.raises(ValueError, match=match):
            io_ply.load_reference_ply(path)

    for fmt in ("binary_little_endian", "ascii"):
        _write_ply(path, fmt, verts, faces, corners=4)
        refused("a face with 4 corners")
        _write_ply(path, fmt, verts, faces, (("x", "float"), ("z", "float"), ("red", "uchar")))
        refused("the vertex element has no property y")
        _write_ply(path, fmt, verts, faces, (("x", "float"), ("y", "int"), ("z", "float")))
        refused("x, y and z must be float or double")
        _write_ply(path, fmt, verts, faces)
        raw = open(path, "rb").read()
        open(path, "wb").write(raw[:-20])
        refused("truncated")
        open(path, "wb").write(raw[:raw.index(b"end_header") + 11 + 30])
        refused("truncated")
        open(path, "wb").write(raw[:raw.index(b"end_header")])
        refused("truncated")
        bad = faces.copy()
        bad[4, 1] = 20
        _write_ply(path, fmt, verts, bad)
        refused(r"a face index lies outside \[0, 20\)")
        _write_ply(path, fmt, verts, faces, face_name="texcoord")
        refused("the face element needs one list property vertex_indices")
    _write_ply(path, "binary_big_endian", verts, faces)
    refused("big-endian")
    open(path, "wb").write(b"not a ply\n")
    refused("not a .ply file")
    with pytest.raises(FileNotFoundError):
        io_ply.load_reference_ply(str(tmp_path / "no_such.ply"))


# ------------------------------------------------------------------------------------------------ 6. options
def test_options_are_refused_by_name():
    from clm_gs_amd import mesh_eval
    assert mesh_eval.check_options([0.05, 0.01]) == ([0.05, 0.01], 0.005, 0.5, None, 1, None, 4.0, 1 << 28)
    assert mesh_eval.check_options(0.1, 0.02, 3, (0, 0, 0, 1, 1, 1), 4, 0.5, 2, 1000) == \
        ([0.1], 0.02, 3.0, [0.0, 0.0, 0.0, 1.0, 1.0, 1.0], 4, 0.5, 2.0, 1000)
    nan, inf = float("nan"), float("inf")
    for bad in (0, -1.0, nan, inf, "1", None, True):
        for kw, name in ((dict(taus=[0.1, bad]), "--tau"), (dict(taus=[0.1], spacing=bad), "--spacing"),
                         (dict(taus=[0.1], max_distance=bad), "--max_distance"), (dict(taus=[0.1], cell=bad), "--cell"),
                         (dict(taus=[0.1], grid_gb=bad), "--grid_gb")):
            if bad is None and name in ("--spacing", "--max_distance", "--cell"):
                continue  # (None is the default)
            with pytest.raises(ValueError, match=f"{name} must be a positive finite number"):
                mesh_eval.check_options(**kw)
    for bad in ([], (), None, "0.1"):
        with pytest.raises(ValueError, match="--tau needs at least one"):
            mesh_eval.check_options(bad)
    for bad in ((1, 0, 0, 0, 1, 1), (0, 0, 2, 1, 1, 1)):
        with pytest.raises(ValueError, match="--bounds is inverted"):
            mesh_eval.check_options([0.1], bounds=bad)
    for bad in ((0, 0, 0, 1, 1), (0, 0, 0, 1, 1, nan), (0, 0, 0, 1, 1, inf), "000111"):
        with pytest.raises(ValueError, match="--bounds must be six finite numbers"):
            mesh_eval.check_options([0.1], bounds=bad)
    for bad in (0, -3, 1.5, None, True):
        with pytest.raises(ValueError, match="--ref_every must be an integer >= 1"):
            mesh_eval.check_options([0.1], ref_every=bad)
    for bad in (0, -1, 1 << 31, 2.5, None):
        with pytest.raises(ValueError, match="--max_samples must be an integer in"):
            mesh_eval.check_options([0.1], max_samples=bad)
    with pytest.raises(ValueError, match="--eval_spacing must be a positive finite number"):
        mesh_eval.check_options([0.1], spacing=-1, names=mesh_eval.MODEL_NAMES)
    assert tuple(mesh_eval.REPORT_KEYS[:len(mesh_eval.REPORT_KEYS) - 4]) == tuple(
        E.evaluate(*E.squares()[0], *E.squares()[1], taus=[0.5], spacing=0.25)) and mesh_eval.REPORT_KEYS[-4:] == E.GRID_KEYS


def test_tools_refuse_bad_values_before_any_path_is_touched(tmp_path):
    from clm_gs_amd import mesh_eval, mesh_model
    missing = str(tmp_path / "no_such_dir" / "mesh.ply")
    out = tmp_path / "out"
    for flags, match in ((["--tau", "0"], "--tau must be a positive finite number"),
                         (["--tau", "0.1", "nan"], "--tau must be a positive finite number"),
                         (["--tau", "0.1", "--spacing", "-1"], "--spacing must be a positive finite number"),
                         (["--tau", "0.1", "--max_distance", "inf"], "--max_distance must be a positive finite number"),
                         (["--tau", "0.1", "--cell", "0"], "--cell must be a positive finite number"),
                         (["--tau", "0.1", "--ref_every", "0"], "--ref_every must be an integer >= 1"),
                         (["--tau", "0.1", "--bounds", "1", "0", "0", "0", "1", "1"], "--bounds is inverted"),
                         (["--tau", "0.1", "--max_samples", "0"], "--max_samples must be an integer")):
        with pytest.raises(SystemExit, match=match):
            mesh_eval.main(["-i", missing, "-r", missing, "-o", str(out / "eval.json")] + flags)
    with pytest.raises(FileNotFoundError):  # accepted: the next thing that fails is the missing file
        mesh_eval.main(["-i", missing, "-r", missing, "-o", str(out / "eval.json"), "--tau", "0.1"])
    base = ["-m", missing, "-s", missing, "-o", str(out / "mesh.ply"), "--voxel", "1"]
    for flags, match in ((["--reference", missing], "--reference and --eval_tau come together"),
                         (["--eval_tau", "0.1"], "--reference and --eval_tau come together"),
                         (["--eval_spacing", "0.1"], "--eval_spacing and --eval_max_distance have effect only with"),
                         (["--reference", missing, "--eval_tau", "-1"], "--eval_tau must be a positive finite number"),
                         (["--reference", missing, "--eval_tau", "0.1", "--eval_spacing", "0"], "--eval_spacing must be a positive"),
                         (["--reference", missing, "--eval_tau", "0.1", "--eval_max_distance", "nan"], "--eval_max_distance must be")):
        with pytest.raises(SystemExit, match=match):
            mesh_model.main(base + flags)
    with pytest.raises(ValueError, match="--eval_tau"):
        mesh_model.check_options(0.1, reference=missing, eval_taus=[0.0])
    with pytest.raises(ValueError, match="--reference and --eval_tau come together"):  # before a camera or the model is looked at
        mesh_model.build_mesh(None, None, None, str(out / "mesh.ply"), 0.1, reference=missing)
    mesh_model.check_options(0.1, reference=missing, eval_taus=[0.1, 0.2], eval_spacing=0.05, eval_max_distance=1.0)
    # the positional callers of before: fourteen arguments, `smooth_mu` the last
    mesh_model.check_options(0.1, None, 16.0, 4.0, 2.0, 1, "expected", 0, 0, False, 0.0, 0, 0.5, -0.53)
    assert not out.exists()


def test_records_and_words():
    from clm_gs_amd import mesh_eval
    meta = dict(voxel=0.5, vertices=4, faces=2)
    report = E.evaluate(*E.squares()[0], *E.squares()[1], taus=[0.5, 0.25], spacing=0.25)
    assert mesh_eval.json_record(meta) == meta and mesh_eval.json_record(meta) is not meta
    out = mesh_eval.json_record(meta, report)
    assert out == dict(meta, evaluation=report) and out["evaluation"] is not report and meta == dict(voxel=0.5, vertices=4, faces=2)
    assert json.loads(json.dumps(out)) == out
    assert mesh_eval.log_words() == "" and mesh_eval.log_words(report) == " F 1.0000@tau 0.5 F 0.0000@tau 0.25"
    assert mesh_eval.summary_line(report) == ("mesh evaluation: chamfer 0.25 accuracy 0.25 completeness 0.25 | tau 0.5 precision "
                                              "1.0000 recall 1.0000 F 1.0000 | tau 0.25 precision 0.0000 recall 0.0000 F 0.0000")
