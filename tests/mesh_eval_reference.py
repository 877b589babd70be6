"""The contract of the mesh evaluation ("Mesh evaluation") restated in numpy: the arithmetic of
csrc/mesh_distance_math.h operation by operation (float64, every operation rounded on its own, in the written order), the
sampler, the brute-force distance over ALL primitives, a restatement of the grid walk (binning, shells, stopping rule), the
metrics and the error ramp.  Nothing here imports the code under test."""
import math

import numpy as np

F64 = np.float64
R2_U, R2_V = 0.7548776662466927, 0.5698402909980532
MAX_FACE_SAMPLES = 1 << 31
SLACK = 1.0 - 2.0 ** -16
REGIONS = ("A", "B", "AB", "C", "AC", "BC", "interior")


def dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def point_d2(p, a):
    d = np.asarray(p, dtype=F64) - np.asarray(a, dtype=F64)
    return dot(d, d)


def closest_d2(p, a, b, c, with_region=False):
    """Ericson 5.1.5 with the region tests in the book's order; p, a, b, c broadcast to [..., 3].  -> |p - q|^2, and the
    index into REGIONS of the branch taken."""
    p, a, b, c = np.broadcast_arrays(*(np.asarray(x, dtype=F64) for x in (p, a, b, c)))
    with np.errstate(all="ignore"):
        ab, ac, ap = b - a, c - a, p - a
        d1, d2 = dot(ab, ap), dot(ac, ap)
        bp = p - b
        d3, d4 = dot(ab, bp), dot(ac, bp)
        vc = d1 * d4 - d3 * d2
        cp = p - c
        d5, d6 = dot(ab, cp), dot(ac, cp)
        vb = d5 * d2 - d1 * d6
        va = d3 * d6 - d5 * d4
        e43, e56 = d4 - d3, d5 - d6
        v_ab = (d1 / (d1 - d3))[..., None]
        w_ac = (d2 / (d2 - d6))[..., None]
        w_bc = (e43 / (e43 + e56))[..., None]
        denom = 1.0 / ((va + vb) + vc)
        v, w = (vb * denom)[..., None], (vc * denom)[..., None]
        q = [a, b, a + v_ab * ab, c, a + w_ac * ac, b + w_bc * (c - b), (a + ab * v) + ac * w]
        conds = [(d1 <= 0) & (d2 <= 0), (d3 >= 0) & (d4 <= d3), (vc <= 0) & (d1 >= 0) & (d3 <= 0), (d6 >= 0) & (d5 <= d6),
                 (vb <= 0) & (d2 >= 0) & (d6 <= 0), (va <= 0) & (e43 >= 0) & (e56 >= 0)]
        region = np.full(d1.shape, 6, dtype=np.int64)
        for k in range(5, -1, -1):
            region = np.where(conds[k], k, region)
        out = point_d2(p, q[6])
        for k in range(6):
            out = np.where(region == k, point_d2(p, q[k]), out)
    return (out, region) if with_region else out


def face_area(a, b, c):
    a, b, c = (np.asarray(x, dtype=F64) for x in (a, b, c))
    with np.errstate(all="ignore"):
        ab, ac = b - a, c - a
        n = np.stack([ab[..., 1] * ac[..., 2] - ab[..., 2] * ac[..., 1], ab[..., 2] * ac[..., 0] - ab[..., 0] * ac[..., 2],
                      ab[..., 0] * ac[..., 1] - ab[..., 1] * ac[..., 0]], axis=-1)
        return 0.5 * np.sqrt(dot(n, n))


def area_ok(area):
    return (area > 0) & np.isfinite(area)


def sample_count(area, spacing):
    area = np.asarray(area, dtype=F64)
    with np.errstate(all="ignore"):
        n = np.ceil(area / (F64(spacing) * F64(spacing)))
    n = np.where(n < MAX_FACE_SAMPLES, np.maximum(n, 1.0), float(MAX_FACE_SAMPLES))
    return np.where(area_ok(area), n, 0.0).astype(np.int64)


def sample_uv(k):
    i = (np.asarray(k, dtype=np.int64) + 1).astype(F64)
    tu, tv = 0.5 + i * R2_U, 0.5 + i * R2_V
    u, v = tu - np.floor(tu), tv - np.floor(tv)
    flip = u + v > 1.0
    return np.where(flip, 1.0 - u, u), np.where(flip, 1.0 - v, v)


def sample_position(k, a, b, c):
    a, b, c = (np.asarray(x, dtype=F64) for x in (a, b, c))
    u, v = sample_uv(k)
    return ((a + u[..., None] * (b - a)) + v[..., None] * (c - a)).astype(np.float32)


def corners(verts, faces):
    v = np.asarray(verts, dtype=np.float32).astype(F64)
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    return v[f[:, 0]], v[f[:, 1]], v[f[:, 2]]


def sample(verts, faces, spacing):
    """-> (points float32 [S,3], face int32 [S], weight float64 [S], area float64 [F])."""
    a, b, c = corners(verts, faces)
    area = face_area(a, b, c)
    n = sample_count(area, spacing)
    face = np.repeat(np.arange(len(n), dtype=np.int32), n)
    offsets = np.concatenate([[0], np.cumsum(n)])
    k = np.arange(len(face), dtype=np.int64) - offsets[face]
    points = sample_position(k, a[face], b[face], c[face]).reshape(-1, 3)
    weight = (area[face] / n[face].astype(F64)).astype(F64)
    return points, face, weight, area


# ------------------------------------------------------------------------------------------------ primitives and brute force
def primitives(verts, faces):
    """-> (a, b, c or None, valid): the corners of every primitive in float64 and which of them are primitives."""
    if faces is None:
        a = np.asarray(verts, dtype=np.float32).astype(F64).reshape(-1, 3)
        return a, None, None, np.isfinite(a).all(axis=1)
    a, b, c = corners(verts, faces)
    return a, b, c, area_ok(face_area(a, b, c))


def _finish(points, d2, prim, max_distance):
    finite = np.isfinite(np.asarray(points, dtype=np.float32)).all(axis=1)
    with np.errstate(all="ignore"):
        d = np.sqrt(d2)
    none = ~finite | (prim < 0) | (d > max_distance)
    dist = np.where(none, np.inf, d).astype(np.float32)
    return dist, np.where(none, -1, prim).astype(np.int32)


def brute(points, verts, faces=None, max_distance=math.inf, chunk=128):
    """The minimum over ALL primitives, the smallest index on ties; (+inf, -1) beyond max_distance, without a primitive and
    for a non-finite query.  -> (dist float32 [P], prim int32 [P])."""
    points = np.asarray(points, dtype=np.float32).reshape(-1, 3)
    a, b, c, valid = primitives(verts, faces)
    P = len(points)
    d2, prim = np.full(P, np.inf), np.full(P, -1, dtype=np.int64)
    if valid.any():
        q = np.nan_to_num(points.astype(F64), nan=0.0, posinf=0.0, neginf=0.0)
        for s in range(0, P, chunk):
            qq = q[s:s + chunk, None, :]
            d = point_d2(qq, a[None]) if b is None else closest_d2(qq, a[None], b[None], c[None])
            d = np.where(valid[None] & ~np.isnan(d), d, np.inf)
            i = np.argmin(d, axis=1)  # (the first minimum: the smallest index)
            best = d[np.arange(len(i)), i]
            d2[s:s + chunk], prim[s:s + chunk] = best, np.where(np.isfinite(best), i, -1)
    return _finish(points, d2, prim, max_distance)


# ------------------------------------------------------------------------------------------------ the grid walk
def cell_index(x, o, h, g):
    with np.errstate(all="ignore"):
        t = np.floor((np.asarray(x, dtype=F64) - o) / h)
    return np.where(t >= 0, np.minimum(t, g - 1), 0).astype(np.int64)


def build_grid(verts, faces, h):
    """The binning restated: a dict cell -> ascending list of primitives, over the float64 box of the primitives."""
    a, b, c, valid = primitives(verts, faces)
    pts = np.stack([a, a, a] if b is None else [a, b, c], axis=1)  # [N,3 corners,3]
    used = pts[valid]
    lo, hi = used.reshape(-1, 3).min(axis=0), used.reshape(-1, 3).max(axis=0)
    dims = [int(math.floor((hi[d] - lo[d]) / h)) + 1 for d in range(3)]
    lists, pairs = {}, 0
    for i in np.nonzero(valid)[0]:
        r = [(int(cell_index(pts[i, :, d].min(), lo[d], h, dims[d])), int(cell_index(pts[i, :, d].max(), lo[d], h, dims[d])))
             for d in range(3)]
        for z in range(r[2][0], r[2][1] + 1):
            for y in range(r[1][0], r[1][1] + 1):
                for x in range(r[0][0], r[0][1] + 1):
                    lists.setdefault((x, y, z), []).append(int(i))
                    pairs += 1
    return dict(a=a, b=b, c=c, lo=lo, h=float(h), dims=dims, lists=lists, pairs=pairs)


def grid_walk(points, grid, max_distance=math.inf):
    """The kernel's walk restated: Chebyshev shells around the clamped cell, the minimum with ties to the smaller index,
    stop after shell R once best < (R h SLACK)^2 or R h SLACK > max_distance.  -> (dist, prim, evaluated)."""
    points = np.asarray(points, dtype=np.float32).reshape(-1, 3)
    a, b, c, lo, h, dims, lists = (grid[k] for k in ("a", "b", "c", "lo", "h", "dims", "lists"))
    P = len(points)
    d2, prim, evaluated = np.full(P, np.inf), np.full(P, -1, dtype=np.int64), np.zeros(P, dtype=np.int64)
    for p in range(P):
        if not np.isfinite(points[p]).all():
            continue
        q = points[p].astype(F64)
        cc = [int(cell_index(q[d], lo[d], h, dims[d])) for d in range(3)]
        last = max(max(cc[d], dims[d] - 1 - cc[d]) for d in range(3))
        best, who = np.inf, -1
        for R in range(last + 1):
            shell = []  # (the rule of the minimum does not depend on the order: the shell is evaluated in one call)
            for z in range(max(cc[2] - R, 0), min(cc[2] + R, dims[2] - 1) + 1):
                for y in range(max(cc[1] - R, 0), min(cc[1] + R, dims[1] - 1) + 1):
                    if abs(z - cc[2]) == R or abs(y - cc[1]) == R:
                        xs = range(max(cc[0] - R, 0), min(cc[0] + R, dims[0] - 1) + 1)
                    else:
                        xs = [x for x in (cc[0] - R, cc[0] + R) if 0 <= x < dims[0]]
                    for x in xs:
                        shell += lists.get((x, y, z), ())
            if shell:
                ids = np.asarray(shell)
                d = point_d2(q, a[ids]) if b is None else closest_d2(q, a[ids], b[ids], c[ids])
                evaluated[p] += len(ids)
                d = np.where(np.isnan(d), np.inf, d)
                i = ids[d == d.min()].min()
                if d.min() < best or (d.min() == best and i < who):
                    best, who = float(d.min()), int(i)
            reach = (float(R) * h) * SLACK
            if best < reach * reach or reach > max_distance:
                break
        d2[p], prim[p] = best, who
    dist, prim = _finish(points, d2, prim, max_distance)
    return dist, prim, evaluated


# ------------------------------------------------------------------------------------------------ metrics
def _inside(points, bounds):
    if bounds is None:
        return np.ones(len(points), dtype=bool)
    lo, hi = np.asarray(bounds[:3], dtype=F64), np.asarray(bounds[3:], dtype=F64)
    return ((points >= lo) & (points <= hi)).all(axis=1)


def _side(points, weight, bounds, verts, faces, max_distance, taus):
    finite = np.isfinite(points).all(axis=1)
    keep = finite & _inside(points.astype(F64), bounds)
    q, w = points[keep], weight[keep]
    dist, _ = brute(q, verts, faces, max_distance)
    d = np.minimum(dist.astype(F64), max_distance)
    total = w.sum()
    return dict(candidates=len(points), queries=len(q), nonfinite=int((~finite).sum()), beyond=int(np.isinf(dist).sum()),
                mean=float((w * d).sum() / total), below=[float((w * (dist.astype(F64) < t)).sum() / total) for t in taus])


def evaluate(verts, faces, ref_points, ref_faces, taus, spacing=None, max_distance=None, bounds=None, ref_every=1):
    """The report of mesh_eval.evaluate without the four entries that describe the grids (a speed choice)."""
    taus = [float(t) for t in taus]
    spacing = min(taus) / 2 if spacing is None else float(spacing)
    max_distance = 10 * max(taus) if max_distance is None else float(max_distance)
    verts, ref_points = np.asarray(verts, dtype=np.float32), np.asarray(ref_points, dtype=np.float32)
    mp, _, mw, marea = sample(verts, faces, spacing)
    if ref_faces is None:
        rp = ref_points[::ref_every]
        rw, rdeg = np.ones(len(rp), dtype=F64), 0
    else:
        rp, _, rw, rarea = sample(ref_points, ref_faces, spacing)
        rdeg = int((~area_ok(rarea)).sum())
    m = _side(mp, mw, bounds, ref_points, ref_faces, max_distance, taus)
    r = _side(rp, rw, bounds, verts, faces, max_distance, taus)
    f = [2 * p * q / (p + q) if p + q > 0 else 0.0 for p, q in zip(m["below"], r["below"])]
    return dict(taus=taus, spacing=spacing, max_distance=max_distance, bounds=None if bounds is None else [float(b) for b in bounds],
                ref_every=int(ref_every), accuracy=m["mean"], completeness=r["mean"], chamfer=(m["mean"] + r["mean"]) / 2,
                precision=m["below"], recall=r["below"], fscore=f,
                vertices=len(verts), faces=len(faces), degenerate_faces=int((~area_ok(marea)).sum()),
                mesh_samples=m["candidates"], mesh_queries=m["queries"], mesh_beyond=m["beyond"], mesh_nonfinite=m["nonfinite"],
                ref_points=len(ref_points), ref_faces=None if ref_faces is None else len(ref_faces), ref_degenerate_faces=rdeg,
                ref_samples=r["candidates"], ref_queries=r["queries"], ref_beyond=r["beyond"], ref_nonfinite=r["nonfinite"])


GRID_KEYS = ("ref_cell", "ref_pairs", "mesh_cell", "mesh_pairs")
SUM_KEYS = ("accuracy", "completeness", "chamfer", "precision", "recall", "fscore")


def error_colours(dist, tau):
    """The ramp of --error_mesh: t = min(d / tau, 1), 1 for +inf; red floor(255 t + 0.5), green floor(255 (1 - t) + 0.5)."""
    d = np.asarray(dist, dtype=np.float32).astype(F64)
    t = np.where(np.isinf(d), 1.0, np.minimum(d / float(tau), 1.0))
    out = np.zeros((len(d), 3), dtype=np.uint8)
    out[:, 0] = np.floor(255.0 * t + 0.5).astype(np.uint8)
    out[:, 1] = np.floor(255.0 * (1.0 - t) + 0.5).astype(np.uint8)
    return out


def squares(z=0.25, x1=1.0):
    """Two unit squares of two triangles each, at height 0 and z; the first covers x in [0, x1]."""
    def square(zz, xx):
        return (np.array([[0, 0, zz], [xx, 0, zz], [xx, 1, zz], [0, 1, zz]], dtype=np.float32),
                np.array([[0, 1, 2], [0, 2, 3]], dtype=np.int32))
    return square(0.0, x1), square(z, 1.0)
