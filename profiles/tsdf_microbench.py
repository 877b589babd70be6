"""The mesh-export kernels (csrc/tsdf.hip) at the size of a survey:
    python profiles/tsdf_microbench.py [reps]
A 1024 x 1024 x 256 grid (6.4 GB; voxel = 1 unit) and 4608 x 3456 depth maps of a synthetic aerial block: 16 cameras
600 units above gently rolling ground in the middle of the grid's height, tilted by up to 0.1 rad, at random positions over
the grid, each seeing about 400 x 300 units of it (so a camera observes about a ninth of the columns, and of those only the
voxels from the camera down to `trunc` = 4 below the ground).  Event-timed on the launch stream after one warm-up of each
leg, legs alternated, the median of `reps`:
  copy            a device-to-device copy of the grid's 24 B per voxel (the yardstick: what touching every voxel costs)
  integrate B     clmgs_tsdf_integrate for the first B = 1 and B = 16 cameras, with and without the brick-level cull
  away B          the same cameras turned away from the grid: with the cull every workgroup skips every camera (the floor of
                  a launch), without it every voxel computes z and stops
  extract         clm_kernels.tsdf_extract on the grid the 16 cameras leave (four passes and two prefix sums)
The shader and memory clocks are read before and after."""
import math
import os
import statistics
import subprocess
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from clm_gs_amd import clm_kernels  # noqa: E402

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 3
NX, NY, NZ, H, W, B = 1024, 1024, 256, 3456, 4608, 16
ALT, FX, TRUNC = 600.0, 4608 * 600.0 / 400.0, 4.0


def clocks():
    try:
        out = subprocess.run(["rocm-smi", "--showclocks", "-d", "0"], capture_output=True, text=True, timeout=30).stdout
        return [l.strip() for l in out.splitlines() if "sclk" in l or "mclk" in l]
    except Exception as e:  # the numbers stand without it; say so
        return [f"not read: {e}"]


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def scene(dev):
    """cams [16,16] (grid coordinates = world: voxel 1, origin 0), depth / alpha / rgb on the device.  The depth of pixel
    (c, r) is the distance along z of the camera to the ground under the pixel's ray (one fixed-point step from the plane)."""
    rng = np.random.default_rng(0)
    cams = np.empty((B, 16))
    depth = torch.empty((B, H, W), dtype=torch.float32, device=dev)
    ys, xs = torch.meshgrid(torch.arange(H, device=dev, dtype=torch.float32) + 0.5,
                            torch.arange(W, device=dev, dtype=torch.float32) + 0.5, indexing="ij")
    for b in range(B):
        C = np.array([rng.uniform(150, NX - 150), rng.uniform(150, NY - 150), NZ / 2 + ALT])
        ax, ay = rng.uniform(-0.1, 0.1, size=2)
        Rx = np.array([[1, 0, 0], [0, math.cos(ax), -math.sin(ax)], [0, math.sin(ax), math.cos(ax)]])
        Ry = np.array([[math.cos(ay), 0, math.sin(ay)], [0, 1, 0], [-math.sin(ay), 0, math.cos(ay)]])
        Rm = Rx @ Ry @ np.diag([1.0, -1.0, -1.0])  # world -> camera: looking down
        cams[b, :12] = np.concatenate([Rm, (-Rm @ C)[:, None]], axis=1).reshape(12)
        cams[b, 12:] = (FX, FX, W / 2, H / 2)
        ray = torch.stack([(xs - W / 2) / FX, (ys - H / 2) / FX, torch.ones_like(xs)], -1) @ torch.tensor(Rm, dtype=torch.float32, device=dev)
        t = (NZ / 2 - C[2]) / ray[..., 2]                       # to the plane z = NZ / 2 (ray = camera ray in world axes)
        gx, gy = C[0] + t * ray[..., 0], C[1] + t * ray[..., 1]
        ground = NZ / 2 + 20.0 * torch.sin(gx * 0.02) * torch.cos(gy * 0.015)
        depth[b] = (ground - C[2]) / ray[..., 2]                # camera depth (z) of the ground point
    alpha = torch.ones((B, H, W), dtype=torch.float32, device=dev)
    rgb = torch.rand((B, 3, H, W), dtype=torch.float32, device=dev)
    return cams, depth, alpha, rgb


def main():
    dev = torch.device("cuda:0")
    print("clocks before:", clocks())
    cams, depth, alpha, rgb = scene(dev)
    grid = torch.zeros((6, NZ, NY, NX), dtype=torch.float32, device=dev)
    other = torch.empty_like(grid)
    fuse = lambda nb, cull: clm_kernels.tsdf_integrate(grid, depth[:nb], alpha[:nb], rgb[:nb], cams[:nb], near=0.01,
                                                       trunc=TRUNC, cull=cull)
    legs = {"copy": lambda: other.copy_(grid), "integrate B=1 cull": lambda: fuse(1, True),
            "integrate B=1 no cull": lambda: fuse(1, False), "integrate B=16 cull": lambda: fuse(16, True),
            "integrate B=16 no cull": lambda: fuse(16, False)}
    away = cams.copy()  # the same cameras looking away from the grid: every brick culled / every voxel behind the camera
    away[:, :12] *= -1.0
    turned = lambda nb, cull: clm_kernels.tsdf_integrate(grid, depth[:nb], alpha[:nb], rgb[:nb], away[:nb], near=0.01,
                                                         trunc=TRUNC, cull=cull)
    legs.update({"away B=16 cull": lambda: turned(16, True), "away B=16 no cull": lambda: turned(16, False),
                 "away B=1 cull": lambda: turned(1, True)})
    times = {k: [] for k in legs}
    for k, fn in legs.items():  # warm-up
        timed(fn)
    for _ in range(reps):
        for k, fn in legs.items():
            times[k].append(timed(fn))
    touched = int((grid[1] > 0).sum())
    n = NX * NY * NZ
    print(f"grid {NX} x {NY} x {NZ} = {n} voxels ({n * 24 / 1e9:.2f} GB), depth maps {W} x {H}, reps {reps}; voxels observed by "
          f"the 16 cameras: {touched} ({100.0 * touched / n:.1f} %)")
    for k, ts in times.items():
        med = statistics.median(ts)
        extra = f"  {2 * n * 24 / med / 1e6:.0f} GB/s read + written" if k == "copy" else \
            f"  {med / int(k.split('=')[1].split()[0]):.3f} ms per camera"
        print(f"{k:>24}: median {med:8.2f} ms  min {min(ts):8.2f} ms{extra}")
    del other
    grid.zero_()
    fuse(16, True)
    fuse(16, True)  # every observed voxel at weight 2
    g2w = np.concatenate([np.eye(3), np.zeros((3, 1))], axis=1)
    out, ts = None, []
    for _ in range(reps + 1):
        torch.cuda.synchronize()
        ts.append(timed(lambda: clm_kernels.tsdf_extract(grid, 2.0, g2w)))
    verts, colours, faces = clm_kernels.tsdf_extract(grid, 2.0, g2w)
    print(f"{'extract':>24}: median {statistics.median(ts[1:]):8.2f} ms  min {min(ts[1:]):8.2f} ms  vertices {verts.shape[0]} "
          f"faces {faces.shape[0]} (the host reads two counts back inside)")
    print("clocks after:", clocks())


if __name__ == "__main__":
    main()
