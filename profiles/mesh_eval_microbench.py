"""python profiles/mesh_eval_microbench.py [256 512 ...]: the measurement of DESIGN.md section 3, "Mesh evaluation"
(profiles/mesh_eval_microbench.txt): analytic gyroid grids of that many voxels per side, period 48 voxels, voxel 1,
extracted on the device, evaluated against a copy displaced by one voxel along x (tau 1 and 2, spacing 0.5, max_distance
20).  Per direction: sampling, binning (count + emit kernels), the sort of the pairs with the searchsorted, the query sort
and the distance kernel; the mean primitives evaluated per query; evaluate() in all and its peak memory above the two
meshes.  Host clock around work that ends in a synchronise, the fastest of three after a warm-up."""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from clm_gs_amd import clm_kernels, mesh_eval  # noqa: E402
from mesh_smooth_microbench import best, gyroid_grid, say  # noqa: E402


def measure(n, cell=None):
    dev = torch.device("cuda:0")
    g2w = np.array([[1.0, 0, 0, 0], [0, 1.0, 0, 0], [0, 0, 1.0, 0]], dtype=np.float64)
    grid = gyroid_grid(n, dev)
    verts, _, faces = clm_kernels.tsdf_extract(grid, 2.0, g2w)
    del grid
    torch.cuda.empty_cache()
    ref = (verts + torch.tensor([1.0, 0.0, 0.0], device=dev)).contiguous()
    V, F = int(verts.shape[0]), int(faces.shape[0])
    say(f"grid {n}^3: V {V} F {F}" + ("" if cell is None else f" cell {cell:g}"))
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    for what, qv, pv in (("mesh -> reference", verts, ref), ("reference -> mesh", ref, verts)):
        t_sample = best(lambda: clm_kernels.mesh_sample(qv, faces, 0.5))
        points = clm_kernels.mesh_sample(qv, faces, 0.5)[0]
        t_grid = best(lambda: clm_kernels.mesh_distance_grid(pv, faces, cell))
        g = clm_kernels.mesh_distance_grid(pv, faces, cell)
        cells = torch.randint(0, g.dims[0] * g.dims[1] * g.dims[2], (g.pairs,), dtype=torch.int64, device=dev)
        prims = torch.empty((g.pairs,), dtype=torch.int32, device=dev)

        def sort():
            c, order = torch.sort(cells, stable=True)
            prims[order]
            torch.searchsorted(c, torch.arange(g.dims[0] * g.dims[1] * g.dims[2] + 1, dtype=torch.int64, device=dev))

        t_sort = best(sort)
        del cells, prims
        t_dist = best(lambda: clm_kernels.mesh_distance(points, g, 20.0))
        _lib = clm_kernels._lib
        _lib.TIMING = {}
        dist, prim, evaluated = clm_kernels.mesh_distance(points, g, 20.0, with_evaluated=True)
        torch.cuda.synchronize()
        t_kernel = _lib.timing_summary()["clmgs_mesh_distance"][1]
        _lib.TIMING = None
        say(f"  {what}: {points.shape[0]} queries; sampling {t_sample:.1f} ms; grid h {g.h:g} dims {g.dims} pairs {g.pairs} in "
            f"{t_grid:.1f} ms (of which sort + searchsorted {t_sort:.1f} ms); distance {t_dist:.1f} ms (kernel {t_kernel:.1f} ms, "
            f"the rest the query sort and scatter); primitives evaluated per query {evaluated.double().mean():.1f}; "
            f"mean distance {dist.double().mean():.4f}")
        del g, points, dist, prim, evaluated
        torch.cuda.empty_cache()
    t_all = best(lambda: mesh_eval.evaluate(verts, faces, ref, faces, [1.0, 2.0], 0.5, 20.0, cell=cell))
    torch.cuda.reset_peak_memory_stats()
    report = mesh_eval.evaluate(verts, faces, ref, faces, [1.0, 2.0], 0.5, 20.0, cell=cell)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    say(f"  evaluate in all {t_all:.1f} ms, peak above the two meshes {peak / 2**30:.2f} GiB; " + mesh_eval.summary_line(report))


if __name__ == "__main__":
    args = sys.argv[1:]
    cell = None
    if "--cell" in args:
        i = args.index("--cell")
        cell = float(args[i + 1])
        del args[i:i + 2]
    for n in [int(a) for a in args] or [256]:
        measure(n, cell)
