"""numpy restatement of the mesh decimation contract ("Mesh decimation"), written from the contract and
not from csrc/mesh_decimate.hip.  It is the authority on the order of operations: every float64 product, quotient and sum
below is one numpy ufunc call (or one step of np.add.at, which adds its operands one after the other, in index order), so
each is rounded on its own.

Vertex clustering on a world-aligned grid of `cell` units with quadric-error representatives (Lindstrom 2000; quadrics
after Garland & Heckbert 1997):
  cells      (i, j, k) = floor(float64(x) / cell) per axis; key = ((i + 2^20) << 42) | ((j + 2^20) << 21) | (k + 2^20).
             A non-finite coordinate or an index outside [-2^20, 2^20) of a PARTICIPATING vertex is a ValueError.
  clusters   the distinct keys of the vertices that at least one face names; new index = rank of the key, ascending.
  faces      corners -> clusters; two equal corners: dropped (faces_collapsed); rotated so that the smallest index comes
             first; of equal rotated triples the first in input order stays (faces_duplicate); input order is kept.
  colour     (2 S + n) // (2 n) of the integer channel sums S over the n member vertices.
  position   centre c = (i + 0.5) cell; mean m = (sum (p - c)) / n over the members in ascending vertex index; per face
             nrm = (p1 - p0) x (p2 - p0), once per DISTINCT cluster among its corners: a = p0 - c,
             d = -((nrm0 a0 + nrm1 a1) + nrm2 a2), A += nrm nrm^T (six sums), r += -d nrm, in ascending face index;
             tr = (A00 + A11) + A22, mu = (tr 2^-10) / 3, (A + mu I) x = r + mu m by the adjugate; x = m when tr or det is
             not > 0 or x is not finite (placed_mean_degenerate), or some |x_d| > cell (placed_mean_outside); vertex =
             float32(c + x).
"""
import numpy as np

F64 = np.float64
BIAS = 1 << 20
REPORT_KEYS = ("cell", "vertices_in", "faces_in", "vertices", "faces", "faces_collapsed", "faces_duplicate",
               "placed_quadric", "placed_mean_degenerate", "placed_mean_outside")
QUADRIC, MEAN_DEGENERATE, MEAN_OUTSIDE = 0, 1, 2


def check_cell(cell, name="cell"):
    if isinstance(cell, bool) or not isinstance(cell, (int, float)) or not np.isfinite(cell) or cell < 0:
        raise ValueError(f"{name} must be a finite number >= 0, got {cell!r}")
    return float(cell)


def cell_keys(verts, part, cell):
    """-> (ijk int64 [V,3], key int64 [V]); rows of vertices outside `part` are -1."""
    p = np.asarray(verts, dtype=np.float32).astype(F64)
    if not np.isfinite(p[part]).all():
        raise ValueError("mesh decimation: a non-finite vertex coordinate")
    q = np.floor(p / F64(cell))                          # one float64 division, then floor
    qp = q[part]
    if qp.size and (qp.min() < -BIAS or qp.max() >= BIAS):
        big = float(np.abs(p[part]).max())
        raise ValueError(f"mesh decimation: a cell index outside [-2^20, 2^20) at cell {cell:g}; the smallest cell that "
                         f"fits is about {big / BIAS:.9g}")
    ijk = np.full(q.shape, -1, dtype=np.int64)
    ijk[part] = qp.astype(np.int64)
    key = np.full(len(p), -1, dtype=np.int64)
    key[part] = ((ijk[part, 0] + BIAS) << 42) | ((ijk[part, 1] + BIAS) << 21) | (ijk[part, 2] + BIAS)
    return ijk, key


def decimate(verts, colours, faces, cell, placement="quadric"):
    """-> (verts float32 [C,3], colours uint8 [C,3], faces int32 [F',3], report).  cell == 0: the inputs, report None.
    placement "mean" places every vertex at its mean (the comparison of the accuracy tests; its report counts every
    cluster as placed_mean_degenerate)."""
    cell = check_cell(cell)
    if cell == 0:
        return verts, colours, faces, None
    verts = np.asarray(verts, dtype=np.float32).reshape(-1, 3)
    colours = np.asarray(colours, dtype=np.uint8).reshape(-1, 3)
    faces = np.asarray(faces, dtype=np.int32).reshape(-1, 3)
    V, F = len(verts), len(faces)
    if F and (faces.min() < 0 or faces.max() >= V):
        raise ValueError(f"mesh decimation: a face index lies outside [0, {V})")
    part = np.zeros(V, dtype=bool)
    part[faces.reshape(-1)] = True
    ijk, key = cell_keys(verts, part, cell)
    ukeys, inverse = np.unique(key[part], return_inverse=True)
    C = len(ukeys)
    cluster = np.full(V, -1, dtype=np.int64)
    cluster[part] = inverse
    members = np.nonzero(part)[0]                        # ascending vertex index
    cl_m = cluster[members]
    # ---- centres, means, colours
    uijk = np.stack([(ukeys >> 42) - BIAS, ((ukeys >> 21) & (2 * BIAS - 1)) - BIAS, (ukeys & (2 * BIAS - 1)) - BIAS], 1)
    centre = (uijk.astype(F64) + 0.5) * F64(cell)
    p = verts.astype(F64)
    n = np.bincount(cl_m, minlength=C).astype(np.int64)
    msum = np.zeros((C, 3), dtype=F64)
    np.add.at(msum, cl_m, p[members] - centre[cl_m])
    mean = msum / n.astype(F64)[:, None]
    S = np.zeros((C, 3), dtype=np.int64)
    np.add.at(S, cl_m, colours[members].astype(np.int64))
    out_colours = ((2 * S + n[:, None]) // (2 * n[:, None])).astype(np.uint8)
    # ---- faces
    cf = cluster[faces.astype(np.int64)]                 # [F,3]
    collapsed = (cf[:, 0] == cf[:, 1]) | (cf[:, 1] == cf[:, 2]) | (cf[:, 0] == cf[:, 2])
    surv = cf[~collapsed]
    first = np.argmin(surv, axis=1) if len(surv) else np.zeros(0, dtype=np.int64)
    rot = np.stack([surv[np.arange(len(surv)), (first + e) % 3] for e in range(3)], 1).reshape(-1, 3)
    seen, keep = set(), np.zeros(len(rot), dtype=bool)
    for t, tri in enumerate(map(tuple, rot.tolist())):
        if tri not in seen:
            seen.add(tri)
            keep[t] = True
    out_faces = rot[keep].astype(np.int32).reshape(-1, 3)
    # ---- quadrics: the incidences (cluster, face), distinct per face, ordered by cluster then face
    fid = np.arange(F, dtype=np.int64)
    inc_c = np.concatenate([cf[:, 0], cf[:, 1][cf[:, 1] != cf[:, 0]], cf[:, 2][(cf[:, 2] != cf[:, 0]) & (cf[:, 2] != cf[:, 1])]])
    inc_f = np.concatenate([fid, fid[cf[:, 1] != cf[:, 0]], fid[(cf[:, 2] != cf[:, 0]) & (cf[:, 2] != cf[:, 1])]])
    order = np.lexsort((inc_f, inc_c))
    inc_c, inc_f = inc_c[order], inc_f[order]
    p0, p1, p2 = (p[faces[inc_f, e]] for e in range(3))
    e1, e2 = p1 - p0, p2 - p0
    nrm = np.stack([e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1],
                    e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2],
                    e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]], 1)
    a = p0 - centre[inc_c]
    d = -((nrm[:, 0] * a[:, 0] + nrm[:, 1] * a[:, 1]) + nrm[:, 2] * a[:, 2])
    A = np.zeros((C, 6), dtype=F64)                      # 00 01 02 11 12 22
    np.add.at(A, inc_c, np.stack([nrm[:, 0] * nrm[:, 0], nrm[:, 0] * nrm[:, 1], nrm[:, 0] * nrm[:, 2],
                                  nrm[:, 1] * nrm[:, 1], nrm[:, 1] * nrm[:, 2], nrm[:, 2] * nrm[:, 2]], 1))
    r = np.zeros((C, 3), dtype=F64)
    np.add.at(r, inc_c, (-d)[:, None] * nrm)
    # ---- solve
    with np.errstate(all="ignore"):
        tr = (A[:, 0] + A[:, 3]) + A[:, 5]
        mu = (tr * F64(2.0 ** -10)) / F64(3.0)
        a00, a01, a02, a11, a12, a22 = A[:, 0] + mu, A[:, 1], A[:, 2], A[:, 3] + mu, A[:, 4], A[:, 5] + mu
        b = [r[:, e] + mu * mean[:, e] for e in range(3)]
        c00 = a11 * a22 - a12 * a12
        c01 = a02 * a12 - a01 * a22
        c02 = a01 * a12 - a02 * a11
        c11 = a00 * a22 - a02 * a02
        c12 = a01 * a02 - a00 * a12
        c22 = a00 * a11 - a01 * a01
        det = (a00 * c00 + a01 * c01) + a02 * c02
        x = np.stack([((c00 * b[0] + c01 * b[1]) + c02 * b[2]) / det,
                      ((c01 * b[0] + c11 * b[1]) + c12 * b[2]) / det,
                      ((c02 * b[0] + c12 * b[1]) + c22 * b[2]) / det], 1)
        degenerate = ~(tr > 0) | ~(det > 0) | ~np.isfinite(x).all(axis=1)
        outside = ~degenerate & (np.abs(x) > F64(cell)).any(axis=1)
    code = np.where(degenerate, MEAN_DEGENERATE, np.where(outside, MEAN_OUTSIDE, QUADRIC))
    if placement == "mean":
        code = np.full(C, MEAN_DEGENERATE)
    elif placement != "quadric":
        raise ValueError(placement)
    x = np.where((code == QUADRIC)[:, None], x, mean)
    out_verts = (centre + x).astype(np.float32).reshape(-1, 3)
    report = dict(cell=cell, vertices_in=V, faces_in=F, vertices=C, faces=len(out_faces),
                  faces_collapsed=int(collapsed.sum()), faces_duplicate=int(len(rot) - keep.sum()),
                  placed_quadric=int((code == QUADRIC).sum()), placed_mean_degenerate=int((code == MEAN_DEGENERATE).sum()),
                  placed_mean_outside=int((code == MEAN_OUTSIDE).sum()))
    return out_verts, out_colours.reshape(-1, 3), out_faces, report
