"""Solo timing of the bilateral-grid kernels (csrc/bilagrid.hip) at a given image size against a device-to-device copy
of the same number of bytes, in the same process (python profiles/bilagrid_microbench.py [W H]); CLMGS_LIB_PATH selects
a library build.  Forward: 24 B per pixel (read x, write y) against a copy of one [H,W,3] float image; backward in
place: 36 B per pixel (read x, read g, write v_x over g) plus the slab it stores, against a copy that moves as many bytes
(it reads half of them and writes half);
tv_grad: the table of N_CAMERAS grids read once and the gradient table read and written, against a copy of one and a
half tables.  Kernels and copies are timed alternately, ROUNDS windows of REPS launches each; per kernel the median,
fastest and slowest window, and per round the kernel / copy ratio.  The colours are uniform in [0, 1): every wave meets
every level of the grid, the worst case for the backward's level loop; `smooth` repeats the backward on an image whose
luminance varies slowly (a wave then touches two or three levels), which is what a render looks like."""
import statistics
import sys
import torch
sys.path.insert(0, ".")
from clm_gs_amd import _lib
from clm_gs_amd._lib import check, dptr, stream
W, H = (int(sys.argv[1]), int(sys.argv[2])) if len(sys.argv) > 2 else (4608, 3456)
WG, HG, LZ = 16, 16, 8
N_CAMERAS = 400
ROUNDS, REPS = 7, 10
L = _lib.lib()
dev = "cuda"
g0 = torch.Generator(device=dev).manual_seed(0)
# close to the identity, rows of A[:, :3] summing to 1: the in-place backward is applied to the same buffer many times
eye = torch.tensor([1.0, 0, 0, 0, 0, 1.0, 0, 0, 0, 0, 1.0, 0], device=dev)
G = (eye + 0.01 * torch.randn((LZ, HG, WG, 12), device=dev, generator=g0)).contiguous()
rows = int(L.clmgs_bilagrid_partials_rows(H, W, HG, WG))
partials = torch.empty((rows, LZ * 48), device=dev)
grad = torch.zeros_like(G)
table = G.repeat(N_CAMERAS, 1, 1, 1, 1).contiguous()
table_grad = torch.zeros_like(table)
src24, dst24 = torch.rand((H, W, 3), device=dev, generator=g0), torch.empty((H, W, 3), device=dev)
n36 = (36 * H * W + partials.numel() * 4) // 8  # floats: a copy reads and writes each of them
src36, dst36 = torch.rand((n36,), device=dev, generator=g0), torch.empty((n36,), device=dev)
n_tv = table.numel() * 3 // 2
src_tv, dst_tv = torch.rand((n_tv,), device=dev, generator=g0), torch.empty((n_tv,), device=dev)


def window(f):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(REPS):
        f()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / REPS


res = {"size": [W, H], "grid": [WG, HG, LZ], "slab_rows": rows, "slab_bytes": partials.numel() * 4,
       "bytes_fwd": 24 * H * W, "bytes_bwd": n36 * 8, "bytes_tv": n_tv * 8}
yy = torch.linspace(0, 1, H, device=dev)[:, None, None]
xx = torch.linspace(0, 1, W, device=dev)[None, :, None]
images = {"interleaved": (torch.rand((H, W, 3), device=dev, generator=g0), (1, 3 * W, 3)),
          "interleaved4": (torch.rand((H, W, 4), device=dev, generator=g0), (1, 4 * W, 4)),
          "planar": (torch.rand((3, H, W), device=dev, generator=g0), (H * W, W, 1)),
          "smooth": ((0.1 + 0.8 * (0.5 * yy + 0.5 * xx)).expand(H, W, 3).contiguous(), (1, 3 * W, 3))}
for name, (x, st) in images.items():
    y, g = torch.empty_like(x), torch.rand(x.shape, device=dev, generator=g0) * 1e-3

    def fwd():
        check(L.clmgs_bilagrid_fwd(stream(), H, W, dptr(x), *st, dptr(G), LZ, HG, WG, dptr(y), *st))

    def bwd_in_place():
        check(L.clmgs_bilagrid_bwd(stream(), H, W, dptr(x), *st, dptr(G), LZ, HG, WG, dptr(g), *st, dptr(g), *st,
                                   dptr(partials)))

    def finish():
        check(L.clmgs_bilagrid_grad_finish(stream(), H, W, LZ, HG, WG, dptr(partials), dptr(grad)))

    def tv_grad():
        check(L.clmgs_bilagrid_tv_grad(stream(), dptr(table), N_CAMERAS, LZ, HG, WG, 10.0, dptr(table_grad)))

    def copy24():
        dst24.copy_(src24)

    def copy36():
        dst36.copy_(src36)

    def copy_tv():
        dst_tv.copy_(src_tv)

    kernels = [("fwd", fwd), ("copy24", copy24), ("bwd_in_place", bwd_in_place), ("copy36", copy36), ("grad_finish", finish)]
    if name == "interleaved":
        kernels += [("tv_grad", tv_grad), ("copy_tv", copy_tv)]
    times = {k: [] for k, _ in kernels}
    for rnd in range(ROUNDS + 1):  # round 0 warms every kernel up
        for k, f in kernels:
            if rnd == 0:
                for _ in range(2):
                    f()
                torch.cuda.synchronize()
            else:
                times[k].append(window(f))
    for k, t in times.items():
        res[f"{name}_{k}_ms"] = {"median": round(statistics.median(t), 4), "min": round(min(t), 4), "max": round(max(t), 4)}
    pairs = [("fwd", "copy24"), ("bwd_in_place", "copy36")] + ([("tv_grad", "copy_tv")] if name == "interleaved" else [])
    for k, c in pairs:
        ratios = [a / b for a, b in zip(times[k], times[c])]
        res[f"{name}_{k}_over_{c}"] = {"median": round(statistics.median(ratios), 4), "min": round(min(ratios), 4),
                                       "max": round(max(ratios), 4)}
    fwd()  # sanity: the kernels did their work
    res[f"{name}_y_mean"] = float(y.double().mean())
    res[f"{name}_g_abs_mean_after_in_place"] = float(g.double().abs().mean())
    del x, y, g
for k, v in res.items():
    print(k, v)
