"""Mesh decimation ("Mesh decimation"): vertex clustering on a world-aligned grid with quadric-error
representatives (Lindstrom, "Out-of-core simplification of large polygonal models", 2000; quadrics after Garland &
Heckbert 1997).

    python -m clm_gs_amd.mesh_model ... --decimate_cell C
    python -m clm_gs_amd.clean_mesh -i <mesh.ply> -o <out.ply> --decimate_cell C

All vertices a face names that fall into one cell of C world units (cells aligned to the world origin) become one vertex;
faces that lose a corner that way are dropped, faces that become equal are kept once.  The new vertex minimises the sum of
the squared (area-weighted) distances to the planes of the faces that touch the cell, regularised towards the mean of the
merged vertices, and falls back to that mean where the minimiser is undefined or leaves the cell's neighbourhood; its
colour is the rounded mean of the merged colours.  The kernels (clm_kernels.mesh_decimate_*, csrc/mesh_decimate.hip) fix
every bit: the result equals the numpy restatement of the contract (tests/mesh_decimate_reference.py) exactly.  The sorts,
prefix sums and compactions between the kernels are torch.  The result is NOT guaranteed to be a manifold.
"""
import torch

from . import _lib, clm_kernels

REPORT_KEYS = ("cell", "vertices_in", "faces_in", "vertices", "faces", "faces_collapsed", "faces_duplicate",
               "placed_quadric", "placed_mean_degenerate", "placed_mean_outside")


def check_cell(cell, name="--decimate_cell"):
    """A finite number >= 0 (0 = off), or ValueError by the option's name.  -> cell as a float."""
    if isinstance(cell, bool) or not isinstance(cell, (int, float)) or not (0 <= cell < float("inf")):
        raise ValueError(f"{name} must be a finite number >= 0 (world units; 0 = off), got {cell!r}")
    return float(cell)


def _refuse(bits, verts, faces, cell):
    """The ValueError of a raised key flag; only this path looks at the coordinates from the host."""
    if bits & clm_kernels.MESH_DECIMATE_NONFINITE:
        raise ValueError("mesh decimation: a non-finite vertex coordinate among the vertices the faces name")
    big = float(verts[faces.reshape(-1).long()].abs().max())
    raise ValueError(f"mesh decimation: a cell index outside [-2^20, 2^20) at cell {cell:g} (a coordinate of magnitude "
                     f"{big:g}); the smallest cell that fits is about {big / 2 ** 20:.9g}")


@torch.no_grad()
def decimate(verts, colours, faces, cell):
    """verts float32 [V,3], colours uint8 [V,3], faces int32 [F,3] on the device, cell >= 0 in world units -> (verts,
    colours, faces, report).  report: cell, vertices_in, faces_in, vertices, faces, faces_collapsed, faces_duplicate,
    placed_quadric, placed_mean_degenerate, placed_mean_outside.  With cell == 0 the inputs come back untouched, nothing
    runs on the device and report is None.  A negative or non-finite cell, a non-finite coordinate and a cell index outside
    [-2^20, 2^20) are refused with ValueError, by name; the last two after the key pass and before anything else is
    launched."""
    cell = check_cell(cell, "cell")
    if cell == 0:
        return verts, colours, faces, None
    what = "mesh decimation"
    clm_kernels._mesh_dev(verts, torch.float32, (None, 3), what, "verts")
    V = int(verts.shape[0])
    clm_kernels._mesh_dev(colours, torch.uint8, (V, 3), what, "colours")
    keys, flag = clm_kernels.mesh_decimate_keys(verts, faces, cell)  # (checks faces)
    F, dev = int(faces.shape[0]), verts.device
    if colours.device != dev or faces.device != dev:
        raise _lib.ClmgsError(f"{what}: verts are on {dev}, colours on {colours.device}, faces on {faces.device}")
    report = dict(cell=cell, vertices_in=V, faces_in=F, vertices=0, faces=0, faces_collapsed=0, faces_duplicate=0,
                  placed_quadric=0, placed_mean_degenerate=0, placed_mean_outside=0)
    if F == 0 or V == 0:
        return verts[:0].contiguous(), colours[:0].contiguous(), faces[:0].contiguous(), report
    bits = int(flag)  # the one value read before anything else is launched
    if bits:
        _refuse(bits, verts, faces, cell)
    # ---- clusters: the distinct keys of the participating vertices, ascending; members by cluster, then index
    skeys, order = torch.sort(keys, stable=True)
    del keys
    first = int(torch.searchsorted(skeys, torch.zeros((1,), dtype=torch.int64, device=dev)))  # unreferenced: key -1
    skeys, order = skeys[first:], order[first:]
    head = torch.ones_like(skeys, dtype=torch.bool)
    head[1:] = skeys[1:] != skeys[:-1]
    cluster_keys = skeys[head]
    C, M = int(cluster_keys.shape[0]), int(skeys.shape[0])
    cluster = torch.full((V,), -1, dtype=torch.int32, device=dev)
    cluster[order] = (torch.cumsum(head, 0, dtype=torch.int32) - 1)
    vert_start = torch.cat([torch.nonzero(head).flatten(), torch.full((1,), M, dtype=torch.int64, device=dev)])
    vert_order = order.to(torch.int32)
    del skeys, order, head
    # ---- the lanes of the placement take the clusters in the order of their first member: ascending keys run along z first,
    # the vertices and faces of an extracted mesh along x first, and a wave whose lanes gather from 64 far-apart places
    # reads a cache line per vertex; neighbours in memory on neighbouring lanes share their lines.  Any order gives the
    # same bits
    lane_order = torch.sort(vert_order[vert_start[:-1]]).indices.to(torch.int32)
    # ---- faces: corners -> clusters, rotated; the (cluster, face) incidences, ordered by cluster then face
    rotated, collapsed, inc = clm_kernels.mesh_decimate_faces(faces, cluster, C)
    del cluster
    inc = torch.sort(inc).values
    inc_start = torch.searchsorted(inc, torch.arange(C + 1, dtype=torch.int64, device=dev) << 32)
    inc = inc[:int(inc_start[-1])].contiguous()  # (the unused slots sort last)
    new_verts, new_colours, code = clm_kernels.mesh_decimate_place(verts, colours, faces, cluster_keys, vert_order, vert_start,
                                                                   inc, inc_start, lane_order, cell)
    del inc, inc_start, vert_order, vert_start, lane_order
    # ---- drop the collapsed faces, then all but the first of equal rotated triples; input order is kept
    surv = rotated[collapsed == 0]
    S = int(surv.shape[0])
    del rotated, collapsed
    if S:
        o = torch.sort(surv[:, 2], stable=True).indices
        o = o[torch.sort(((surv[:, 0].long() << 31) | surv[:, 1].long())[o], stable=True).indices]
        s = surv[o]
        lead = torch.ones((S,), dtype=torch.bool, device=dev)
        lead[1:] = (s[1:] != s[:-1]).any(dim=1)
        keep = torch.empty((S,), dtype=torch.bool, device=dev)
        keep[o] = lead  # stable sorts: the lead of a run of equal triples is the first of them in input order
        new_faces = surv[keep].contiguous()
    else:
        new_faces = surv.contiguous()
    placed = torch.bincount(code.long(), minlength=3).tolist()
    report.update(vertices=C, faces=int(new_faces.shape[0]), faces_collapsed=F - S, faces_duplicate=S - int(new_faces.shape[0]),
                  placed_quadric=placed[0], placed_mean_degenerate=placed[1], placed_mean_outside=placed[2])
    return new_verts, new_colours, new_faces, report


def json_record(meta, report, vertices, faces):
    """The dict written next to a decimated mesh: `meta` (not modified) with "vertices" and "faces" updated and a
    "decimation" entry holding the report."""
    out = dict(meta)
    out["vertices"], out["faces"] = int(vertices), int(faces)
    out["decimation"] = dict(report)
    return out


def log_words(report):
    """What the log line of an export or of the tool gains: " decimated V -> V' vertices F -> F' faces cell C"."""
    return " decimated {} -> {} vertices {} -> {} faces cell {:g}".format(
        report["vertices_in"], report["vertices"], report["faces_in"], report["faces"], report["cell"])
