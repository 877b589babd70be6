"""The sparse-volume kernels (csrc/tsdf_sparse.hip) against the dense ones on the aerial block of profiles/tsdf_microbench.py:
    python profiles/tsdf_sparse_microbench.py [reps] [big]
The 1024 x 1024 x 256 grid (voxel = 1 unit) and the 16 synthetic 4608 x 3456 cameras of that script.  One process, legs
alternated, event-timed on the launch stream after one warm-up of each, the median of `reps`:
  dense integrate B=16    clmgs_tsdf_integrate with the cull (the number of tsdf_microbench.py, re-measured here)
  mark B=16               clmgs_tsdf_mark into zeroed marks (zeroed outside the timing)
  sparse integrate B=16   clmgs_tsdf_sparse_integrate on the bricks the 16 cameras mark
  dense / sparse extract  clm_kernels.tsdf_extract against tsdf_sparse_extract (its two sorts and the index remap included),
                          each on its volume fused twice (every observed voxel at weight 2); the meshes are compared
and the allocated share and the pool's GB.  With `big` one more run at a box the dense path refuses: the same terrain at
voxel 1/8, 8192 x 8192 x 2048 voxels (2^37), the first 8 cameras: bricks, GB and the times of the three passes.  The shader
and memory clocks are read before and after."""
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import tsdf_microbench as base  # noqa: E402  (its scene(), timed() and clocks(); it puts the repository on sys.path)
from clm_gs_amd import clm_kernels  # noqa: E402

reps, TRUNC = base.reps, base.TRUNC
NX, NY, NZ, B = base.NX, base.NY, base.NZ, base.B


def invert(cams):
    out = cams.copy()
    for b in range(len(cams)):
        out[b, :12] = np.linalg.inv(np.vstack([cams[b, :12].reshape(3, 4), [0.0, 0.0, 0.0, 1.0]]))[:3].reshape(12)
    return out


def allocate(marks):
    flat = marks.reshape(-1) != 0
    scan = torch.cumsum(flat, 0, dtype=torch.int32)
    table = torch.where(flat, scan - 1, torch.full_like(scan, -1)).reshape(marks.shape).contiguous()
    bricks = torch.nonzero(flat).reshape(-1).to(torch.int32)
    return table, bricks, torch.zeros((bricks.shape[0], 6, 8, 8, 8), dtype=torch.float32, device=marks.device)


def median_of(legs, before=None):
    times = {k: [] for k in legs}
    for k, fn in legs.items():  # warm-up
        if before and k in before:
            before[k]()
        base.timed(fn)
    for _ in range(reps):
        for k, fn in legs.items():
            if before and k in before:
                before[k]()
                torch.cuda.synchronize()
            times[k].append(base.timed(fn))
    for k, ts in times.items():
        print(f"{k:>24}: median {statistics.median(ts):8.2f} ms  min {min(ts):8.2f} ms")
    return times


def main():
    dev = torch.device("cuda:0")
    print("clocks before:", base.clocks())
    cams, depth, alpha, rgb = base.scene(dev)
    inv = invert(cams)
    shape = (NX, NY, NZ)
    gates = dict(near=0.01, trunc=TRUNC)
    grid = torch.zeros((6, NZ, NY, NX), dtype=torch.float32, device=dev)
    nb = clm_kernels.tsdf_brick_grid(*shape)
    marks = torch.zeros((nb[2], nb[1], nb[0]), dtype=torch.uint8, device=dev)
    mark = lambda: clm_kernels.tsdf_mark(marks, shape, depth, alpha, inv, voxel_cam=1.0, **gates)
    mark()
    table, bricks, pool = allocate(marks)
    S, total = int(bricks.shape[0]), marks.numel()
    print(f"grid {NX} x {NY} x {NZ}, depth maps {base.W} x {base.H}, reps {reps}; bricks marked {S} of {total} "
          f"({100.0 * S / total:.1f} %), pool {S * 12288 / 1e9:.3f} GB against {NX * NY * NZ * 24 / 1e9:.2f} GB dense")
    median_of({"dense integrate B=16": lambda: clm_kernels.tsdf_integrate(grid, depth, alpha, rgb, cams, cull=True, **gates),
               "mark B=16": mark,
               "sparse integrate B=16": lambda: clm_kernels.tsdf_sparse_integrate(pool, bricks, shape, depth, alpha, rgb, cams,
                                                                                  cull=True, **gates)},
              before={"mark B=16": lambda: marks.zero_()})
    grid.zero_()
    pool.zero_()
    for _ in range(2):  # every observed voxel at weight 2
        clm_kernels.tsdf_integrate(grid, depth, alpha, rgb, cams, **gates)
        clm_kernels.tsdf_sparse_integrate(pool, bricks, shape, depth, alpha, rgb, cams, **gates)
    g2w = np.concatenate([np.eye(3), np.zeros((3, 1))], axis=1)
    median_of({"dense extract": lambda: clm_kernels.tsdf_extract(grid, 2.0, g2w),
               "sparse extract": lambda: clm_kernels.tsdf_sparse_extract(pool, bricks, table, shape, 2.0, g2w)})
    d, s = clm_kernels.tsdf_extract(grid, 2.0, g2w), clm_kernels.tsdf_sparse_extract(pool, bricks, table, shape, 2.0, g2w)
    same = all(torch.equal(a.view(torch.int32) if a.dtype == torch.float32 else a, b.view(torch.int32) if b.dtype == torch.float32 else b)
               for a, b in zip(d, s))
    print(f"vertices {d[0].shape[0]} faces {d[2].shape[0]}; sparse mesh == dense mesh: {same}")
    if "big" in sys.argv[2:]:
        del grid, pool, table, bricks, marks, d, s
        torch.cuda.empty_cache()
        big(dev, cams[:8], depth[:8], alpha[:8], rgb[:8])
    print("clocks after:", base.clocks())


def big(dev, cams, depth, alpha, rgb, scale=8):
    """The same terrain at voxel 1 / scale: a box of 2^37 voxels.  One timing per pass (a first launch, clocks as they are)."""
    shape = (NX * scale, NY * scale, NZ * scale)
    fine = cams.copy()
    for b in range(len(fine)):  # grid -> world is now a scaling by 1 / scale
        m = fine[b, :12].reshape(3, 4)
        m[:, :3] /= scale
    inv = invert(fine)
    gates = dict(near=0.01, trunc=TRUNC / scale)
    nb = clm_kernels.tsdf_brick_grid(*shape)
    marks = torch.zeros((nb[2], nb[1], nb[0]), dtype=torch.uint8, device=dev)
    t_mark = base.timed(lambda: clm_kernels.tsdf_mark(marks, shape, depth, alpha, inv, voxel_cam=1.0 / scale, **gates))
    table, bricks, pool = allocate(marks)
    S = int(bricks.shape[0])
    print(f"big: grid {shape[0]} x {shape[1]} x {shape[2]} = 2^{int(np.log2(float(shape[0]) * shape[1] * shape[2]))} voxels, "
          f"{len(cams)} cameras; bricks {S} of {marks.numel()} ({100.0 * S / marks.numel():.2f} %), pool {S * 12288 / 1e9:.2f} GB, "
          f"marks + table {marks.numel() * 5 / 1e9:.2f} GB")
    t_fuse = base.timed(lambda: clm_kernels.tsdf_sparse_integrate(pool, bricks, shape, depth, alpha, rgb, fine, **gates))
    g2w = np.concatenate([np.eye(3) / scale, np.zeros((3, 1))], axis=1)
    out = []
    t_ext = base.timed(lambda: out.append(clm_kernels.tsdf_sparse_extract(pool, bricks, table, shape, 1.0, g2w)))
    print(f"big: mark {t_mark:.2f} ms, sparse integrate {t_fuse:.2f} ms, sparse extract (min_weight 1) {t_ext:.2f} ms, "
          f"vertices {out[0][0].shape[0]} faces {out[0][2].shape[0]}")


if __name__ == "__main__":
    main()
