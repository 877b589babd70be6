"""python profiles/mesh_smooth_microbench.py [768 1280 ...]: the measurement of DESIGN.md section 3, "Mesh smoothing and
normals" (profiles/mesh_smooth_microbench.txt): analytic gyroid grids of that many voxels per side, period 48 voxels, voxel
1, extracted on the device; the incidence sort, one smoothing step, the normals kernel, smooth(N=10) in all, the peak
memory above the mesh, and next to each kernel a device-to-device copy that reads and writes in all the bytes the kernel
must move (per entry 8 B of order, a 12 B face row and two or three 12 B vertices; per vertex its boundary, its own row
and the output row).  Host clock around work that ends in a synchronise, the fastest of three after a warm-up."""
import math
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from clm_gs_amd import clm_kernels, mesh_smooth  # noqa: E402


def say(*a):
    print(" ".join(str(x) for x in a), flush=True)


def best(fn, n=3):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(n):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return min(ts) * 1e3


def gyroid_grid(n, dev, period=48.0, trunc=4.0, weight=3.0):
    g = torch.zeros((6, n, n, n), dtype=torch.float32, device=dev)
    k = 2.0 * math.pi / period
    c = (torch.arange(n, device=dev, dtype=torch.float32) + 0.5) * k
    s, co = torch.sin(c), torch.cos(c)
    for z in range(n):  # plane by plane: no second grid-sized temporary
        val = s[None, :] * co[:, None] + s[:, None] * co[z] + s[z] * co[None, :]  # [y, x]
        g[0, z] = weight * torch.clamp(val / k / trunc, -1.0, 1.0)
    g[1] = weight
    g[2:5] = 0.5 * weight
    g[5] = weight
    return g


def copy_ms(nbytes):
    """A device-to-device copy that reads and writes `nbytes` in all (a buffer of half that)."""
    a = torch.empty((nbytes // 2,), dtype=torch.uint8, device="cuda")
    b = torch.empty_like(a)
    return best(lambda: b.copy_(a))


def measure(n):
    dev = torch.device("cuda:0")
    g2w = [[1.0, 0, 0, 0], [0, 1.0, 0, 0], [0, 0, 1.0, 0]]
    import numpy as np
    grid = gyroid_grid(n, dev)
    verts, colours, faces = clm_kernels.tsdf_extract(grid, 2.0, np.array(g2w, dtype=np.float64))
    del grid
    torch.cuda.empty_cache()
    V, F = int(verts.shape[0]), int(faces.shape[0])
    say(f"grid {n}^3: V {V} F {F}")
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    t_inc = best(lambda: clm_kernels.mesh_incidence(faces, V))
    torch.cuda.reset_peak_memory_stats()
    order, start = clm_kernels.mesh_incidence(faces, V)
    torch.cuda.synchronize()
    peak_inc = torch.cuda.max_memory_allocated() - base
    L = clm_kernels._lib.lib()
    out = torch.empty_like(verts)
    from clm_gs_amd._lib import check, dptr, stream
    f32, i32, i64 = torch.float32, torch.int32, torch.int64

    def step():
        check(L.clmgs_mesh_smooth_step(stream(), V, F, dptr(verts, f32), dptr(faces, i32), dptr(order, i64), dptr(start, i64), 0.5,
                                       dptr(out, f32)))

    def normals():
        check(L.clmgs_mesh_vertex_normals(stream(), V, F, dptr(verts, f32), dptr(faces, i32), dptr(order, i64), dptr(start, i64),
                                          dptr(out, f32)))

    t_step, t_norm = best(step), best(normals)
    b_step = 3 * F * (8 + 12 + 24) + V * (8 + 12 + 12)
    b_norm = 3 * F * (8 + 12 + 36) + V * (8 + 12)
    c_step, c_norm = copy_ms(b_step), copy_ms(b_norm)
    del order, start, out
    torch.cuda.empty_cache()
    t_smooth = best(lambda: mesh_smooth.smooth(verts, colours, faces, 10))
    torch.cuda.reset_peak_memory_stats()
    mesh_smooth.smooth(verts, colours, faces, 10)
    torch.cuda.synchronize()
    peak_smooth = torch.cuda.max_memory_allocated() - base
    t_vn = best(lambda: mesh_smooth.vertex_normals(verts, faces))
    say(f"  incidence sort (torch) {t_inc:.1f} ms, peak above the mesh {peak_inc / 2**30:.2f} GiB")
    say(f"  one smoothing step {t_step:.2f} ms; bytes {b_step / 1e9:.2f} GB, copy {c_step:.2f} ms, ratio {t_step / c_step:.1f}")
    say(f"  normals kernel {t_norm:.2f} ms; bytes {b_norm / 1e9:.2f} GB, copy {c_norm:.2f} ms, ratio {t_norm / c_norm:.1f}")
    say(f"  smooth(N=10) in all {t_smooth:.1f} ms, peak above the mesh {peak_smooth / 2**30:.2f} GiB")
    say(f"  vertex_normals in all (lists + kernel) {t_vn:.1f} ms")


if __name__ == "__main__":
    for n in [int(a) for a in sys.argv[1:]] or [768]:
        measure(n)
