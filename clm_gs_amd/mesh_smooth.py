"""Mesh smoothing and vertex normals ("Mesh smoothing and normals"): Taubin's lambda | mu smoothing
(Taubin, "A signal processing approach to fair surface design", 1995; open3d's filter_smooth_taubin) and area-weighted
vertex normals, both over the vertex -> face incidence lists of the mesh.

    python -m clm_gs_amd.mesh_model ... --smooth_iterations N [--smooth_lambda 0.5 --smooth_mu -0.53] [--normals]
    python -m clm_gs_amd.clean_mesh -i <mesh.ply> -o <out.ply> --smooth_iterations N --normals

One step with factor c moves every vertex by c towards the mean of its neighbours, taken over its incidences: per face
that names the vertex, the two other corners.  That is the umbrella operator with each neighbour weighted by the number of
faces sharing the edge: on a closed manifold every edge has two faces and the weights equal the uniform ones of open3d; on
a boundary the boundary neighbours weigh half.  One iteration is a step with lam and, unless mu == 0, a step with mu < 0,
which undoes the shrinkage of the first; mu == 0 is plain Laplacian smoothing.  Steps are Jacobi (two buffers).  Colours,
faces and the vertex count never change, and a vertex no face names keeps its bits.  Non-finite coordinates are not
refused: they propagate through the arithmetic to every neighbour.

A vertex normal is the normalised sum of (p1 - p0) x (p2 - p0) over the faces that name the vertex (area-weighted), zero
where that sum has no direction.  The extraction orients faces outward, so the normals point out of closed shapes.

The kernels (clm_kernels.mesh_smooth_step / mesh_vertex_normals, csrc/mesh_smooth.hip) fix every bit: positions and
normals equal the numpy restatement of the contract (tests/mesh_smooth_reference.py) exactly.  The incidence lists (a
stable sort and a searchsorted) are torch, built once per call.
"""
import math

import torch

from . import _lib, clm_kernels

REPORT_KEYS = ("iterations", "lam", "mu", "vertices", "faces", "vertices_fixed")
NAMES = ("--smooth_iterations", "--smooth_lambda", "--smooth_mu")


def check_options(iterations=0, lam=0.5, mu=-0.53, names=NAMES):
    """iterations a non-negative integer (0 = off), lam in (0, 1], mu in [-1, 0], or ValueError by the option's name.
    -> (iterations, lam, mu) as int, float, float."""
    n = iterations
    if isinstance(n, bool) or not isinstance(n, int):
        if not (isinstance(n, float) and math.isfinite(n) and n == int(n)):
            raise ValueError(f"{names[0]} must be a non-negative integer (0 = off), got {n!r}")
        n = int(n)
    if n < 0:
        raise ValueError(f"{names[0]} must be a non-negative integer (0 = off), got {n}")
    for value, name, rule, ok in ((lam, names[1], "in (0, 1]", lambda x: 0 < x <= 1),
                                  (mu, names[2], "in [-1, 0] (0 = plain Laplacian smoothing)", lambda x: -1 <= x <= 0)):
        if isinstance(value, bool) or not isinstance(value, (int, float)) or not math.isfinite(value) or not ok(value):
            raise ValueError(f"{name} must be a finite number {rule}, got {value!r}")
    return n, float(lam), float(mu)


@torch.no_grad()
def smooth(verts, colours, faces, iterations, lam=0.5, mu=-0.53):
    """verts float32 [V,3], colours uint8 [V,3], faces int32 [F,3] on the device -> (verts, colours, faces, report):
    `iterations` times a step with lam, then (mu != 0) a step with mu.  colours and faces are the objects passed in.
    report: iterations, lam, mu, vertices, faces, vertices_fixed (the vertices no face names).  With iterations == 0 the
    inputs come back untouched, nothing runs on the device and report is None.  Bad options are refused with ValueError,
    by name."""
    iterations, lam, mu = check_options(iterations, lam, mu, ("iterations", "lam", "mu"))
    if iterations == 0:
        return verts, colours, faces, None
    what = "mesh smoothing"
    clm_kernels._mesh_dev(verts, torch.float32, (None, 3), what, "verts")
    V = int(verts.shape[0])
    clm_kernels._mesh_dev(colours, torch.uint8, (V, 3), what, "colours")
    order, start = clm_kernels.mesh_incidence(faces, V)  # (checks faces); built once for all the steps
    F = int(faces.shape[0])
    report = dict(iterations=iterations, lam=lam, mu=mu, vertices=V, faces=F,
                  vertices_fixed=int((start[1:] == start[:-1]).sum()) if V else 0)
    if F == 0 or V == 0:
        return verts, colours, faces, report
    clm_kernels._mesh_lists(verts, faces, order, start, what)
    factors = ((lam, mu) if mu != 0 else (lam,)) * iterations
    # two buffers, written in turn (Jacobi: a step reads only its input); the caller's tensor is read, never written
    buffers = [torch.empty_like(verts) for _ in range(min(len(factors), 2))]
    L, src = _lib.lib(), verts
    for i, c in enumerate(factors):
        dst = buffers[i % 2]
        _lib.check(L.clmgs_mesh_smooth_step(_lib.stream(), V, F, _lib.dptr(src, torch.float32), _lib.dptr(faces, torch.int32),
                                            _lib.dptr(order, torch.int64), _lib.dptr(start, torch.int64), c,
                                            _lib.dptr(dst, torch.float32)))
        src = dst
    return src, colours, faces, report


@torch.no_grad()
def vertex_normals(verts, faces):
    """verts float32 [V,3], faces int32 [F,3] on the device -> normals float32 [V,3] on the device."""
    clm_kernels._mesh_dev(verts, torch.float32, (None, 3), "mesh normals", "verts")
    order, start = clm_kernels.mesh_incidence(faces, int(verts.shape[0]))
    return clm_kernels.mesh_vertex_normals(verts, faces, order, start)


def json_record(meta, report=None, normals=False):
    """The dict written next to a smoothed mesh: `meta` (not modified) with a "smoothing" entry holding the report when
    there is one, and "normals": true when the file carries them."""
    out = dict(meta)
    if report is not None:
        out["smoothing"] = dict(report)
    if normals:
        out["normals"] = True
    return out


def log_words(report=None, normals=False):
    """What the log line of an export or of the tool gains: " smoothed N x (lam, mu)" and " normals"."""
    words = "" if report is None else " smoothed {} x ({:g}, {:g})".format(report["iterations"], report["lam"], report["mu"])
    return words + (" normals" if normals else "")
