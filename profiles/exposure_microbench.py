"""Solo timing of the exposure kernels (csrc/exposure.hip) at a given image size against a device-to-device copy of the
same number of bytes, in the same process (python profiles/exposure_microbench.py [W H]); CLMGS_LIB_PATH selects a
library build.  Forward: 24 B per pixel (read x, write y) against a copy of one [H,W,3] float image; backward in place:
36 B per pixel (read x, read g, write v_x over g) against a copy of one and a half images.  The kernels and the copies
are timed alternately, ROUNDS windows of REPS launches each; per kernel the median, fastest and slowest window, and per
round the kernel / copy ratio.  The planar layout (generic path) is timed for the record; the engine never uses it."""
import statistics
import sys
import torch
sys.path.insert(0, ".")
from clm_gs_amd import _lib
from clm_gs_amd._lib import check, dptr, stream
W, H = (int(sys.argv[1]), int(sys.argv[2])) if len(sys.argv) > 2 else (4608, 3456)
ROUNDS, REPS = 7, 20
L = _lib.lib()
dev = "cuda"
g0 = torch.Generator(device=dev).manual_seed(0)
# a contraction (rows of E[:, :3] sum to 1): the in-place backward is applied to the same buffer hundreds of times
E = torch.tensor([[0.9, 0.05, 0.05, 0.01], [0.05, 0.9, 0.05, -0.02], [0.05, 0.05, 0.9, 0.03]], device=dev)
rows = int(L.clmgs_exposure_partials_rows(H, W))
partials = torch.empty((rows, 12), device=dev)
grad12 = torch.zeros(12, device=dev)
src24, dst24 = torch.rand((H, W, 3), device=dev, generator=g0), torch.empty((H, W, 3), device=dev)
n36 = H * W * 9 // 2
src36, dst36 = torch.rand((n36,), device=dev, generator=g0), torch.empty((n36,), device=dev)


def window(f):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(REPS):
        f()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / REPS


res = {"size": [W, H], "partial_rows": rows, "bytes_fwd": 24 * H * W, "bytes_bwd": 36 * H * W}
for name in ("interleaved", "planar"):
    if name == "planar":
        x = torch.rand((3, H, W), device=dev, generator=g0); st = (H * W, W, 1)
    else:
        x = torch.rand((H, W, 3), device=dev, generator=g0); st = (1, 3 * W, 3)
    y, g, v = torch.empty_like(x), torch.rand(x.shape, device=dev, generator=g0) * 1e-3, torch.empty_like(x)

    def fwd():
        check(L.clmgs_exposure_fwd(stream(), H, W, dptr(x), *st, dptr(E), dptr(y), *st))

    def bwd_in_place():
        check(L.clmgs_exposure_bwd(stream(), H, W, dptr(x), *st, dptr(E), dptr(g), *st, dptr(g), *st, dptr(partials)))

    def bwd_out_of_place():
        check(L.clmgs_exposure_bwd(stream(), H, W, dptr(x), *st, dptr(E), dptr(g), *st, dptr(v), *st, dptr(partials)))

    def finish():
        check(L.clmgs_exposure_grad_finish(stream(), rows, dptr(partials), dptr(grad12)))

    def copy24():
        dst24.copy_(src24)

    def copy36():
        dst36.copy_(src36)

    kernels = [("fwd", fwd), ("copy24", copy24), ("bwd_in_place", bwd_in_place), ("copy36", copy36),
               ("bwd_out_of_place", bwd_out_of_place), ("grad_finish", finish)]
    times = {k: [] for k, _ in kernels}
    for rnd in range(ROUNDS + 1):  # round 0 warms every kernel up
        for k, f in kernels:
            if rnd == 0:
                for _ in range(3):
                    f()
                torch.cuda.synchronize()
            else:
                times[k].append(window(f))
    for k, t in times.items():
        res[f"{name}_{k}_ms"] = {"median": round(statistics.median(t), 4), "min": round(min(t), 4), "max": round(max(t), 4)}
    for k, c, nbytes in (("fwd", "copy24", 24), ("bwd_in_place", "copy36", 36), ("bwd_out_of_place", "copy36", 36)):
        ratios = [a / b for a, b in zip(times[k], times[c])]
        res[f"{name}_{k}_over_{c}"] = {"median": round(statistics.median(ratios), 4), "min": round(min(ratios), 4),
                                       "max": round(max(ratios), 4)}
        res[f"{name}_{k}_TB_per_s"] = round(nbytes * H * W / (statistics.median(times[k]) * 1e-3) / 1e12, 3)
    for c, nbytes in (("copy24", 24), ("copy36", 36)):
        res[f"{name}_{c}_TB_per_s"] = round(nbytes * H * W / (statistics.median(times[c]) * 1e-3) / 1e12, 3)
    # sanity: the kernels did their work
    fwd()
    res[f"{name}_y_mean"] = float(y.double().mean())
    res[f"{name}_g_abs_mean_after_in_place"] = float(g.double().abs().mean())
    del x, y, g, v
for k, v in res.items():
    print(k, v)
