"""The numpy restatement of the contract of mesh smoothing and vertex normals ("Mesh smoothing and
normals"; csrc/mesh_vertex_math.h, csrc/mesh_smooth.hip).  Everything is float64, every operation rounded on its own
(numpy never contracts a product and a sum), in the order stated; the device must give the same bits.

Two forms: explicit per-vertex loops in the stated order (`smooth_step_loop`, `vertex_normals_loop`), which ARE the
contract, and vectorised ones on np.add.at (`smooth_step`, `vertex_normals`), which adds its terms one after the other in
index order and so forms the same left-to-right sums; tests/test_mesh_smooth_cpu.py holds the second to the first bit for
bit before anything larger uses it.
"""
import math

import numpy as np

REPORT_KEYS = ("iterations", "lam", "mu", "vertices", "faces", "vertices_fixed")


def incidence(faces, V):
    """faces int32 [F,3] -> (order int64 [3F], start int64 [V+1]): the corner slots e = 3 f + k in a stable ascending sort
    by the vertex they name, and the segment boundaries."""
    flat = np.asarray(faces, dtype=np.int32).reshape(-1)
    order = np.argsort(flat, kind="stable").astype(np.int64)
    start = np.searchsorted(flat[order], np.arange(V + 1)).astype(np.int64)
    return order, start


def _mesh(verts, faces):
    verts = np.ascontiguousarray(verts, dtype=np.float32).reshape(-1, 3)
    faces = np.ascontiguousarray(faces, dtype=np.int32).reshape(-1, 3)
    return verts, faces, verts.astype(np.float64)


# ---------------------------------------------------------------------------------------------- the contract, as loops
def smooth_step_loop(verts, faces, c, lists=None):
    """One step with factor c -> float32 [V,3] (a new array)."""
    verts, faces, p = _mesh(verts, faces)
    order, start = lists or incidence(faces, len(verts))
    c = np.float64(c)
    out = verts.copy()
    for v in range(len(verts)):
        s, n = np.zeros(3, dtype=np.float64), 0
        for e in order[start[v]:start[v + 1]]:
            f, k = int(e) // 3, int(e) % 3
            s = s + p[faces[f, (k + 1) % 3]]
            s = s + p[faces[f, (k + 2) % 3]]
            n += 2
        if n > 0:
            m = s / np.float64(n)
            out[v] = (p[v] + c * (m - p[v])).astype(np.float32)
    return out


def vertex_normals_loop(verts, faces, lists=None):
    """Area-weighted vertex normals -> float32 [V,3]."""
    verts, faces, p = _mesh(verts, faces)
    order, start = lists or incidence(faces, len(verts))
    out = np.zeros((len(verts), 3), dtype=np.float32)
    with np.errstate(all="ignore"):
        for v in range(len(verts)):
            a = np.zeros(3, dtype=np.float64)
            for e in order[start[v]:start[v + 1]]:
                p0, p1, p2 = (p[i] for i in faces[int(e) // 3])
                e1, e2 = p1 - p0, p2 - p0
                a[0] = a[0] + (e1[1] * e2[2] - e1[2] * e2[1])
                a[1] = a[1] + (e1[2] * e2[0] - e1[0] * e2[2])
                a[2] = a[2] + (e1[0] * e2[1] - e1[1] * e2[0])
            q = (a[0] * a[0] + a[1] * a[1]) + a[2] * a[2]
            if q > 0 and np.isfinite(q):
                inv = np.float64(1.0) / np.sqrt(q)
                out[v] = (a * inv).astype(np.float32)
    return out


# ---------------------------------------------------------------------------------------------- the same sums, vectorised
def smooth_step(verts, faces, c, lists=None):
    verts, faces, p = _mesh(verts, faces)
    V = len(verts)
    order, start = lists or incidence(faces, V)
    f, k = order // 3, order % 3
    owner = faces[f, k].astype(np.int64)
    # per entry its two terms, one after the other: np.add.at adds them in this order
    terms = np.stack([p[faces[f, (k + 1) % 3]], p[faces[f, (k + 2) % 3]]], axis=1).reshape(-1, 3)
    s = np.zeros((V, 3), dtype=np.float64)
    np.add.at(s, np.repeat(owner, 2), terms)
    n = 2 * (start[1:] - start[:-1])
    with np.errstate(all="ignore"):
        m = s / np.maximum(n, 1).astype(np.float64)[:, None]
        moved = (p + np.float64(c) * (m - p)).astype(np.float32)
    return np.where((n > 0)[:, None], moved, verts)


def vertex_normals(verts, faces, lists=None):
    verts, faces, p = _mesh(verts, faces)
    V = len(verts)
    order, start = lists or incidence(faces, V)
    with np.errstate(all="ignore"):
        p0, p1, p2 = p[faces[:, 0]], p[faces[:, 1]], p[faces[:, 2]]
        e1, e2 = p1 - p0, p2 - p0
        cross = np.stack([e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1], e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2],
                          e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]], axis=1)
        f, k = order // 3, order % 3
        a = np.zeros((V, 3), dtype=np.float64)
        np.add.at(a, faces[f, k].astype(np.int64), cross[f])
        q = (a[:, 0] * a[:, 0] + a[:, 1] * a[:, 1]) + a[:, 2] * a[:, 2]
        ok = (q > 0) & np.isfinite(q)
        inv = np.float64(1.0) / np.sqrt(np.where(ok, q, 1.0))
        out = (a * inv[:, None]).astype(np.float32)
    return np.where(ok[:, None], out, np.float32(0.0))


# ---------------------------------------------------------------------------------------------- smooth
def check_options(iterations, lam, mu):
    if isinstance(iterations, bool) or not isinstance(iterations, (int, np.integer)) or iterations < 0:
        raise ValueError(f"iterations must be a non-negative integer, got {iterations!r}")
    if not (math.isfinite(lam) and 0 < lam <= 1):
        raise ValueError(f"lam must be a finite number in (0, 1], got {lam!r}")
    if not (math.isfinite(mu) and -1 <= mu <= 0):
        raise ValueError(f"mu must be a finite number in [-1, 0], got {mu!r}")


def smooth(verts, colours, faces, iterations, lam=0.5, mu=-0.53, step=smooth_step):
    """-> (verts, colours, faces, report): `iterations` times a step with lam, then (mu != 0) a step with mu.
    iterations == 0 returns the inputs themselves and report None."""
    check_options(iterations, lam, mu)
    if iterations == 0:
        return verts, colours, faces, None
    v, f, _ = _mesh(verts, faces)
    lists = incidence(f, len(v))
    for _ in range(int(iterations)):
        v = step(v, f, lam, lists)
        if mu != 0:
            v = step(v, f, mu, lists)
    report = dict(iterations=int(iterations), lam=float(lam), mu=float(mu), vertices=len(v), faces=len(f),
                  vertices_fixed=int((lists[1][1:] == lists[1][:-1]).sum()))
    return v, colours, faces, report
