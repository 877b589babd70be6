"""Mesh cleanup ("Mesh cleanup"): drops the small connected components of a triangle mesh.

    python -m clm_gs_amd.clean_mesh -i <mesh.ply> -o <out.ply> [--min_faces N] [--keep_largest K] [--decimate_cell C]
        [--smooth_iterations N --smooth_lambda 0.5 --smooth_mu -0.53] [--normals]

(--decimate_cell: mesh_decimate.decimate after the two filters, or alone; DESIGN.md section 3, "Mesh decimation".
--smooth_iterations: mesh_smooth.smooth between the filters and the decimation; --normals: the vertex normals of the
OUTPUT mesh in the file; DESIGN.md section 3, "Mesh smoothing and normals".  The input may be either layout of
io_ply.save_mesh_ply; normals it stores are ignored, never carried through.)

The components are labelled on the device (clm_kernels.mesh_components / mesh_component_faces, csrc/mesh.hip): two vertices
are connected when a face names both, a component's label is its smallest vertex index and its size its number of faces.
The rule: a component is kept iff it has at least max(min_faces, 1) faces and, with keep_largest = K > 0, its rank among
ALL components is below K, ranked by face count descending, then label ascending.  The kept vertices are exactly those a
kept face names; kept vertices and faces stay in their order, the indices are remapped.  Labels, counts and rule are
integers, so the result is the same bits as the numpy restatement of the rule (tests/mesh_clean_reference.py).  The
compaction (keep masks, a prefix sum, two gathers) is torch.
"""
import argparse
import json
import os
import sys
import time

import torch

from . import clm_kernels


def check_options(min_faces=0, keep_largest=0, names=("--min_faces", "--keep_largest")):
    """Non-negative integers, or ValueError by the flag's name.  -> (min_faces, keep_largest) as ints."""
    out = []
    for value, name in zip((min_faces, keep_largest), names):
        if isinstance(value, bool) or not isinstance(value, int):
            if not (isinstance(value, float) and value == int(value)):
                raise ValueError(f"{name} must be a non-negative integer, got {value!r}")
            value = int(value)
        if value < 0:
            raise ValueError(f"{name} must be a non-negative integer, got {value}")
        out.append(value)
    return tuple(out)


@torch.no_grad()
def clean(verts, colours, faces, min_faces=0, keep_largest=0):
    """verts float32 [V,3], colours uint8 [V,3], faces int32 [F,3] on the device -> (verts, colours, faces, report) with
    the components the rule drops removed.  report: components (those with at least one face), components_kept,
    vertices_removed, faces_removed, largest_faces, rounds (of the labelling).  With min_faces == 0 and keep_largest == 0
    the inputs come back untouched, nothing runs on the device and report is None.  Negative options are refused by
    name."""
    min_faces, keep_largest = check_options(min_faces, keep_largest, ("min_faces", "keep_largest"))
    if min_faces == 0 and keep_largest == 0:
        return verts, colours, faces, None
    if not (isinstance(verts, torch.Tensor) and isinstance(colours, torch.Tensor) and verts.dim() == 2
            and colours.dim() == 2 and verts.shape[0] == colours.shape[0]):
        raise ValueError(f"mesh cleanup: verts [V,3] and colours [V,3] expected, got {tuple(getattr(verts, 'shape', ()))} and "
                         f"{tuple(getattr(colours, 'shape', ()))}")
    V = int(verts.shape[0])
    labels, rounds = clm_kernels.mesh_components(faces, V)
    count = clm_kernels.mesh_component_faces(faces, labels)
    F, dev = int(faces.shape[0]), faces.device
    comp = torch.nonzero(count).flatten()  # the labels of the components with a face, ascending
    sizes = count[comp]
    keep = sizes >= max(min_faces, 1)
    if keep_largest > 0:  # rank: face count descending, then label ascending (a stable sort of ascending labels)
        order = torch.sort(sizes, descending=True, stable=True).indices
        rank = torch.empty_like(order)
        rank[order] = torch.arange(order.numel(), device=dev)
        keep &= rank < keep_largest
    keep_label = torch.zeros((V,), dtype=torch.bool, device=dev)
    keep_label[comp[keep]] = True
    if F:
        faces_kept = faces[keep_label[labels[faces[:, 0].long()].long()]]
    else:
        faces_kept = faces
    keep_vert = torch.zeros((V,), dtype=torch.bool, device=dev)
    keep_vert[faces_kept.reshape(-1).long()] = True
    remap = torch.cumsum(keep_vert, 0, dtype=torch.int32) - 1
    new_faces = remap[faces_kept.long()].contiguous()
    new_verts, new_colours = verts[keep_vert].contiguous(), colours[keep_vert].contiguous()
    report = dict(components=int(comp.numel()), components_kept=int(keep.sum()),
                  vertices_removed=V - int(new_verts.shape[0]), faces_removed=F - int(new_faces.shape[0]),
                  largest_faces=int(sizes.max()) if comp.numel() else 0, rounds=int(rounds))
    return new_verts, new_colours, new_faces, report


def json_record(meta, min_faces, keep_largest, report, vertices, faces):
    """The dict written next to a cleaned mesh: `meta` (not modified) with "vertices" and "faces" updated and a "cleanup"
    entry holding the options and the report."""
    out = dict(meta)
    out["vertices"], out["faces"] = int(vertices), int(faces)
    out["cleanup"] = dict(min_faces=int(min_faces), keep_largest=int(keep_largest), **report)
    return out


def json_path(mesh_path):
    return os.path.splitext(mesh_path)[0] + ".json"


def main(argv=None):
    from . import mesh_decimate, mesh_smooth
    ap = argparse.ArgumentParser(prog="clm_gs_amd.clean_mesh",
                                 description="drop the small connected components of a mesh written by clm_gs_amd.mesh_model, "
                                             "and / or smooth it, decimate it, give it vertex normals")
    ap.add_argument("-i", "--input", required=True, help="the mesh (.ply as io_ply.save_mesh_ply writes it)")
    ap.add_argument("-o", "--output", required=True, help="the cleaned mesh; <output>.json is written when <input>.json exists")
    ap.add_argument("--min_faces", type=int, default=0, metavar="N", help="drop the components with fewer than N faces")
    ap.add_argument("--keep_largest", type=int, default=0, metavar="K", help="keep only the K components with the most faces")
    ap.add_argument("--decimate_cell", type=float, default=0.0, metavar="C",
                    help="after the two filters, merge the vertices of every cell of C world units (mesh_decimate.decimate)")
    ap.add_argument("--smooth_iterations", type=int, default=0, metavar="N",
                    help="after the two filters and before the decimation, N Taubin smoothing passes (mesh_smooth.smooth)")
    ap.add_argument("--smooth_lambda", type=float, default=0.5, metavar="L", help="the factor of a pass's first step, in (0, 1]")
    ap.add_argument("--smooth_mu", type=float, default=-0.53, metavar="M",
                    help="the factor of a pass's second step, in [-1, 0]; 0 = plain Laplacian smoothing")
    ap.add_argument("--normals", action="store_true",
                    help="write area-weighted vertex normals of the output mesh (nx ny nz) into the file")
    a = ap.parse_args(argv)
    try:  # refusals before anything is read
        check_options(a.min_faces, a.keep_largest)
        mesh_decimate.check_cell(a.decimate_cell)
        mesh_smooth.check_options(a.smooth_iterations, a.smooth_lambda, a.smooth_mu)
        if a.min_faces == 0 and a.keep_largest == 0 and a.decimate_cell == 0 and a.smooth_iterations == 0 and not a.normals:
            raise ValueError("nothing to do: give --min_faces N, --keep_largest K, --decimate_cell C, --smooth_iterations N "
                             "or --normals")
    except ValueError as e:
        raise SystemExit(str(e))
    from . import io_ply
    t0 = time.perf_counter()
    verts, colours, faces = (torch.from_numpy(t).to("cuda") for t in io_ply.load_mesh_ply(a.input))
    V, F = int(verts.shape[0]), int(faces.shape[0])
    try:
        verts, colours, faces, report = clean(verts, colours, faces, a.min_faces, a.keep_largest)
        verts, colours, faces, smoothing = mesh_smooth.smooth(verts, colours, faces, a.smooth_iterations, a.smooth_lambda,
                                                              a.smooth_mu)
        verts, colours, faces, decimation = mesh_decimate.decimate(verts, colours, faces, a.decimate_cell)
    except ValueError as e:  # (a cell too small for the mesh's extent)
        raise SystemExit(str(e))
    normals = mesh_smooth.vertex_normals(verts, faces) if a.normals else None
    d = os.path.dirname(a.output)
    if d:
        os.makedirs(d, exist_ok=True)
    io_ply.save_mesh_ply(a.output, verts, colours, faces, normals)
    if os.path.exists(json_path(a.input)):
        with open(json_path(a.input)) as f:
            meta = json.load(f)
        if report is not None:
            meta = json_record(meta, a.min_faces, a.keep_largest, report, verts.shape[0], faces.shape[0])
        if decimation is not None:
            meta = mesh_decimate.json_record(meta, decimation, verts.shape[0], faces.shape[0])
        meta.pop("normals", None)  # (of the input file: they are not carried through)
        meta = mesh_smooth.json_record(meta, smoothing, a.normals)
        with open(json_path(a.output), "w") as f:
            json.dump(meta, f, indent=1)
    print("mesh cleanup:{} vertices {} -> {} faces {} -> {}{}{}{} in {:.3f} s -> {}".format(
        "" if report is None else " components {} kept {}".format(report["components"], report["components_kept"]),
        V, int(verts.shape[0]), F, int(faces.shape[0]), "" if report is None else " rounds {}".format(report["rounds"]),
        "" if decimation is None else mesh_decimate.log_words(decimation), mesh_smooth.log_words(smoothing, a.normals),
        time.perf_counter() - t0, a.output))
    return 0


if __name__ == "__main__":
    sys.exit(main())
