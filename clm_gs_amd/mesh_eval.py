"""Mesh evaluation ("Mesh evaluation"): the distance between a mesh and a reference -- a laser scan's
points or another mesh -- in the form the Tanks-and-Temples and DTU protocols report: accuracy, completeness, chamfer
distance and precision / recall / F-score at one or more thresholds tau.

    python -m clm_gs_amd.eval_mesh -i <mesh.ply> -r <reference.ply> --tau T [T ...] [--spacing S] [--max_distance D]
        [--bounds xmin ymin zmin xmax ymax zmax] [--ref_every K] [--cell H] [--grid_gb G] [--max_samples N] [-o eval.json]
        [--error_mesh err.ply]
    python -m clm_gs_amd.mesh_model ... --reference <reference.ply> --eval_tau T [T ...] [--eval_spacing S --eval_max_distance D]

mesh -> reference: the mesh is sampled (clm_kernels.mesh_sample: ceil(area / spacing^2) samples per face at the points of
the R2 sequence, each of weight area / n, so that every metric is weighted by area exactly) and every sample is measured
against the reference's triangles, or its points when it has no faces (clm_kernels.mesh_distance: the exact minimum over
all primitives).  reference -> mesh: the reference's points with weight 1 (every ref_every-th), or samples of the
reference mesh, against the mesh's triangles.  With weights w and d' = min(d, max_distance):

    accuracy = sum w d' / sum w (mesh -> reference)     completeness = the same for reference -> mesh
    chamfer = (accuracy + completeness) / 2
    precision(tau) = sum w [d < tau] / sum w (mesh -> reference)     recall(tau) likewise     fscore = 2 P R / (P + R), 0 for P + R = 0

(float64 sums on the device).  bounds, a world-space box that stands in for a benchmark's crop volume, drops QUERIES
outside it on both sides, never primitives: a surface just outside the crop still counts as a match.  A query with a
non-finite coordinate is dropped and counted.  --spacing defaults to the smallest tau / 2 and --max_distance to 10 x the
largest tau: conventions, stated in the report, not measurements.  Registration of the mesh to the reference is the
caller's: both are taken to be in one frame.
"""
import argparse
import json
import math
import os
import sys
import time

import torch

from . import clm_kernels

REPORT_KEYS = ("taus", "spacing", "max_distance", "bounds", "ref_every", "accuracy", "completeness", "chamfer", "precision",
               "recall", "fscore", "vertices", "faces", "degenerate_faces", "mesh_samples", "mesh_queries", "mesh_beyond",
               "mesh_nonfinite", "ref_points", "ref_faces", "ref_degenerate_faces", "ref_samples", "ref_queries", "ref_beyond",
               "ref_nonfinite", "ref_cell", "ref_pairs", "mesh_cell", "mesh_pairs")
NAMES = dict(taus="--tau", spacing="--spacing", max_distance="--max_distance", bounds="--bounds", ref_every="--ref_every",
             cell="--cell", grid_gb="--grid_gb", max_samples="--max_samples")
MODEL_NAMES = dict(NAMES, taus="--eval_tau", spacing="--eval_spacing", max_distance="--eval_max_distance")


def _positive(value, name):
    if isinstance(value, bool) or not isinstance(value, (int, float)) or not (0 < value < math.inf):
        raise ValueError(f"{name} must be a positive finite number, got {value!r}")
    return float(value)


def check_options(taus, spacing=None, max_distance=None, bounds=None, ref_every=1, cell=None, grid_gb=4.0,
                  max_samples=clm_kernels.MESH_MAX_SAMPLES, names=NAMES):
    """The refusals that need nothing loaded (ValueError by the option's name) and the defaults: spacing = the smallest
    tau / 2, max_distance = 10 x the largest tau.  -> (taus, spacing, max_distance, bounds, ref_every, cell, grid_gb,
    max_samples)."""
    if isinstance(taus, (int, float)) and not isinstance(taus, bool):
        taus = [taus]
    if not isinstance(taus, (list, tuple)) or len(taus) == 0:
        raise ValueError(f"{names['taus']} needs at least one positive finite number, got {taus!r}")
    taus = [_positive(t, names["taus"]) for t in taus]
    spacing = min(taus) / 2 if spacing is None else _positive(spacing, names["spacing"])
    max_distance = 10 * max(taus) if max_distance is None else _positive(max_distance, names["max_distance"])
    if bounds is not None:
        if not isinstance(bounds, (list, tuple)) or len(bounds) != 6 or \
                any(isinstance(b, bool) or not isinstance(b, (int, float)) or not math.isfinite(b) for b in bounds):
            raise ValueError(f"{names['bounds']} must be six finite numbers xmin ymin zmin xmax ymax zmax, got {bounds!r}")
        bounds = [float(b) for b in bounds]
        if any(bounds[k] > bounds[k + 3] for k in range(3)):
            raise ValueError(f"{names['bounds']} is inverted: a minimum above its maximum in {bounds}")
    if isinstance(ref_every, bool) or not isinstance(ref_every, int) or ref_every < 1:
        raise ValueError(f"{names['ref_every']} must be an integer >= 1, got {ref_every!r}")
    cell = None if cell is None else _positive(cell, names["cell"])
    grid_gb = _positive(grid_gb, names["grid_gb"])
    if isinstance(max_samples, bool) or not isinstance(max_samples, int) or not 1 <= max_samples < 1 << 31:
        raise ValueError(f"{names['max_samples']} must be an integer in [1, 2^31), got {max_samples!r}")
    return taus, spacing, max_distance, bounds, ref_every, cell, grid_gb, max_samples


def _side(points, weight, bounds, grid, max_distance, taus):
    """One direction: the queries that are finite and inside the bounds against the grid.  -> dict of counts and sums."""
    finite = torch.isfinite(points).all(dim=1)
    keep = finite
    if bounds is not None:
        p = points.double()
        lo = torch.tensor(bounds[:3], dtype=torch.float64, device=points.device)
        hi = torch.tensor(bounds[3:], dtype=torch.float64, device=points.device)
        keep = finite & ((p >= lo) & (p <= hi)).all(dim=1)
    q, w = points[keep].contiguous(), weight[keep]
    if q.shape[0] == 0:
        return None
    dist, _ = clm_kernels.mesh_distance(q, grid, max_distance)
    d = dist.double()
    total = w.sum()
    return dict(candidates=int(points.shape[0]), queries=int(q.shape[0]), nonfinite=int((~finite).sum()),
                beyond=int(torch.isinf(dist).sum()), mean=float((w * d.clamp(max=max_distance)).sum() / total),
                below=[float((w * (d < t)).sum() / total) for t in taus])


@torch.no_grad()
def evaluate(verts, faces, ref_points, ref_faces, taus, spacing=None, max_distance=None, bounds=None, ref_every=1, cell=None,
             grid_gb=4.0, max_samples=clm_kernels.MESH_MAX_SAMPLES, names=None, timings=None):
    """verts float32 [V,3] and faces int32 [F,3] (the evaluated mesh), ref_points float32 [P,3] and ref_faces int32 [G,3] or
    None (the reference), all on the device -> the report, a dict with REPORT_KEYS.  Bad options, an empty mesh, an empty
    reference and a ref_every beyond the reference's size are refused with ValueError, by name.  timings: a dict that
    receives the seconds of every stage (the device is synchronised around each)."""
    names = names or {k: k for k in NAMES}
    taus, spacing, max_distance, bounds, ref_every, cell, grid_gb, max_samples = check_options(
        taus, spacing, max_distance, bounds, ref_every, cell, grid_gb, max_samples, names)
    what = "mesh evaluation"
    clm_kernels._mesh_dev(verts, torch.float32, (None, 3), what, "verts")
    clm_kernels._mesh_dev(ref_points, torch.float32, (None, 3), what, "ref_points")
    V, P = int(verts.shape[0]), int(ref_points.shape[0])
    F = clm_kernels._mesh_faces(faces, V, what)
    G = None if ref_faces is None else clm_kernels._mesh_faces(ref_faces, P, what)
    if V == 0 or F == 0:
        raise ValueError(f"{what}: an empty mesh ({V} vertices, {F} faces)")
    if P == 0 or G == 0:
        raise ValueError(f"{what}: an empty reference ({P} points, {G} faces)")
    if ref_faces is None and ref_every > P:
        raise ValueError(f"{what}: {names['ref_every']} {ref_every} is larger than the reference's {P} points")
    if ref_faces is not None and ref_every != 1:
        raise ValueError(f"{what}: {names['ref_every']} applies to a reference without faces")
    t0 = [0.0]

    def lap(stage):
        if timings is not None:
            torch.cuda.synchronize()
            now = time.perf_counter()
            if stage is not None:
                timings[stage] = timings.get(stage, 0.0) + (now - t0[0])
            t0[0] = now

    lap(None)
    mp, _, mw, marea = clm_kernels.mesh_sample(verts, faces, spacing, max_samples, names["max_samples"])
    degenerate = F - int(((marea > 0) & torch.isfinite(marea)).sum())
    if mp.shape[0] == 0:
        raise ValueError(f"{what}: an empty mesh (none of its {F} faces has an area)")
    if ref_faces is None:
        rp = ref_points[::ref_every].contiguous()
        rw, rdeg = torch.ones((rp.shape[0],), dtype=torch.float64, device=rp.device), 0
    else:
        rp, _, rw, rarea = clm_kernels.mesh_sample(ref_points, ref_faces, spacing, max_samples, names["max_samples"])
        rdeg = G - int(((rarea > 0) & torch.isfinite(rarea)).sum())
        if rp.shape[0] == 0:
            raise ValueError(f"{what}: an empty reference (none of its {G} faces has an area)")
    lap("sampling")
    rgrid = clm_kernels.mesh_distance_grid(ref_points, ref_faces, cell, grid_gb, names["cell"])
    if rgrid.primitives == 0:
        raise ValueError(f"{what}: an empty reference (none of its {P} points is finite)")
    lap("grid_reference")
    m = _side(mp, mw, bounds, rgrid, max_distance, taus)
    lap("distance_mesh_to_reference")
    rcell, rpairs = rgrid.h, rgrid.pairs
    del rgrid
    mgrid = clm_kernels.mesh_distance_grid(verts, faces, cell, grid_gb, names["cell"])
    lap("grid_mesh")
    r = _side(rp, rw, bounds, mgrid, max_distance, taus)
    lap("distance_reference_to_mesh")
    if m is None or r is None:
        raise ValueError(f"{what}: no {'mesh sample' if m is None else 'reference point'} lies inside {names['bounds']} {bounds}")
    fscore = [2 * p * q / (p + q) if p + q > 0 else 0.0 for p, q in zip(m["below"], r["below"])]
    return dict(taus=taus, spacing=spacing, max_distance=max_distance, bounds=bounds, ref_every=ref_every,
                accuracy=m["mean"], completeness=r["mean"], chamfer=(m["mean"] + r["mean"]) / 2, precision=m["below"],
                recall=r["below"], fscore=fscore, vertices=V, faces=F, degenerate_faces=degenerate,
                mesh_samples=m["candidates"], mesh_queries=m["queries"], mesh_beyond=m["beyond"], mesh_nonfinite=m["nonfinite"],
                ref_points=P, ref_faces=G, ref_degenerate_faces=rdeg, ref_samples=r["candidates"], ref_queries=r["queries"],
                ref_beyond=r["beyond"], ref_nonfinite=r["nonfinite"], ref_cell=rcell, ref_pairs=rpairs, mesh_cell=mgrid.h,
                mesh_pairs=mgrid.pairs)


@torch.no_grad()
def error_colours(verts, ref_points, ref_faces, tau, max_distance, cell=None, grid_gb=4.0):
    """uint8 [V,3] on the device: the ramp of every VERTEX's distance d to the reference, t = min(d / tau, 1) and 1 beyond
    max_distance: red floor(255 t + 0.5), green floor(255 (1 - t) + 0.5), blue 0."""
    grid = clm_kernels.mesh_distance_grid(ref_points, ref_faces, cell, grid_gb)
    dist, _ = clm_kernels.mesh_distance(verts, grid, max_distance)
    d = dist.double()
    t = torch.where(torch.isinf(d), torch.ones_like(d), (d / float(tau)).clamp(max=1.0))
    out = torch.zeros((verts.shape[0], 3), dtype=torch.uint8, device=verts.device)
    out[:, 0] = torch.floor(255.0 * t + 0.5).to(torch.uint8)
    out[:, 1] = torch.floor(255.0 * (1.0 - t) + 0.5).to(torch.uint8)
    return out


def json_record(meta, report=None):
    """The dict written next to an evaluated mesh: `meta` (not modified) with an "evaluation" entry holding the report when
    there is one."""
    out = dict(meta)
    if report is not None:
        out["evaluation"] = dict(report)
    return out


def log_words(report=None):
    """What the log line of an export gains: " F <fscore>@tau <tau>" per threshold."""
    if report is None:
        return ""
    return "".join(" F {:.4f}@tau {:g}".format(f, t) for f, t in zip(report["fscore"], report["taus"]))


def summary_line(report):
    """The line the tool prints: chamfer, accuracy and completeness, then precision, recall and F per tau."""
    line = "mesh evaluation: chamfer {:.6g} accuracy {:.6g} completeness {:.6g}".format(
        report["chamfer"], report["accuracy"], report["completeness"])
    for t, p, r, f in zip(report["taus"], report["precision"], report["recall"], report["fscore"]):
        line += " | tau {:g} precision {:.4f} recall {:.4f} F {:.4f}".format(t, p, r, f)
    return line


def load_reference(path, device="cuda"):
    """io_ply.load_reference_ply on the device: (points float32 [P,3], faces int32 [F,3] or None)."""
    from . import io_ply
    points, faces = io_ply.load_reference_ply(path)
    return (torch.from_numpy(points).to(device), None if faces is None else torch.from_numpy(faces).to(device))


def main(argv=None):
    ap = argparse.ArgumentParser(prog="clm_gs_amd.eval_mesh",
                                 description="accuracy, completeness, chamfer distance and precision / recall / F-score of a "
                                             "mesh written by clm_gs_amd.mesh_model against a reference scan or mesh")
    ap.add_argument("-i", "--input", required=True, help="the evaluated mesh (.ply as io_ply.save_mesh_ply writes it)")
    ap.add_argument("-r", "--reference", required=True,
                    help="the reference (.ply, ascii or binary little-endian): points, or a triangle mesh")
    ap.add_argument("--tau", type=float, nargs="+", required=True, metavar="T", help="the distance thresholds of the F-score")
    ap.add_argument("--spacing", type=float, default=None, metavar="S",
                    help="the sampling distance on surfaces (default: the smallest tau / 2)")
    ap.add_argument("--max_distance", type=float, default=None, metavar="D",
                    help="distances are capped here (default: 10 x the largest tau)")
    ap.add_argument("--bounds", type=float, nargs=6, default=None, metavar=("XMIN", "YMIN", "ZMIN", "XMAX", "YMAX", "ZMAX"),
                    help="only queries inside this world-space box count (primitives outside still match)")
    ap.add_argument("--ref_every", type=int, default=1, metavar="K", help="use every K-th point of a reference without faces")
    ap.add_argument("--cell", type=float, default=None, metavar="H", help="the cell size of both grids (a speed choice)")
    ap.add_argument("--grid_gb", type=float, default=4.0, metavar="G", help="the largest list of (cell, primitive) pairs")
    ap.add_argument("--max_samples", type=int, default=clm_kernels.MESH_MAX_SAMPLES, metavar="N",
                    help="the most samples a surface may get")
    ap.add_argument("-o", "--output", default=None, help="the report (.json); default: <input without .ply>.eval.json")
    ap.add_argument("--error_mesh", default=None, metavar="PLY",
                    help="write the mesh with every vertex coloured by its distance to the reference (green 0 ... red >= tau[0])")
    a = ap.parse_args(argv)
    try:  # refusals before anything is read
        opts = check_options(a.tau, a.spacing, a.max_distance, a.bounds, a.ref_every, a.cell, a.grid_gb, a.max_samples)
    except ValueError as e:
        raise SystemExit(str(e))
    from . import io_ply
    t0 = time.perf_counter()
    verts, colours, faces, normals = io_ply.load_mesh_ply(a.input, with_normals=True)
    try:
        ref_points, ref_faces = load_reference(a.reference)
        verts, faces = torch.from_numpy(verts).to("cuda"), torch.from_numpy(faces).to("cuda")
        report = evaluate(verts, faces, ref_points, ref_faces, *opts, names=NAMES)
    except ValueError as e:
        raise SystemExit(str(e))
    out = a.output or os.path.splitext(a.input)[0] + ".eval.json"
    for path in (out, a.error_mesh):
        if path and os.path.dirname(path):
            os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(out, "w") as f:
        json.dump(dict(mesh=a.input, reference=a.reference, **report), f, indent=1)
    if a.error_mesh:
        ramp = error_colours(verts, ref_points, ref_faces, report["taus"][0], report["max_distance"], opts[5], opts[6])
        io_ply.save_mesh_ply(a.error_mesh, verts, ramp, faces, normals)
    print(summary_line(report) + " in {:.3f} s -> {}".format(time.perf_counter() - t0, out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
