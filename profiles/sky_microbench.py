"""Solo timing of the sky kernels (csrc/sky.hip) against device-to-device copies of as many bytes, in the same process
(python profiles/sky_microbench.py [W H Hs Ws [ROUNDS REPS]]); CLMGS_LIB_PATH selects a library build (a build with
DEFS=-DCLMGS_SKY_WIN_TEXELS=0 sends every tile down the direct path).  Interleaved [H,W,3] image, a camera of about 60
degrees.  Forward in place: 28 B per pixel (read x and alpha, write y) against a copy that moves 28 B per pixel; backward:
20 B per pixel (read g and alpha, write v_alphas) plus the scatter into the int64 accumulator, against a copy that moves
20 B per pixel.  Kernels and copies are timed alternately, ROUNDS windows of REPS launches each; per kernel the median,
fastest and slowest window, and per round the kernel / copy ratio.  The tiles' paths (LDS window / direct) are counted
on the host from the same rule (a sample of the tiles at large sizes)."""
import math
import statistics
import sys
import numpy as np
import torch
sys.path.insert(0, ".")
from clm_gs_amd import _lib
from clm_gs_amd._lib import check, dptr, stream
a_ = [int(v) for v in sys.argv[1:]]
W, H = (a_[0], a_[1]) if len(a_) > 1 else (4608, 3456)
Hs, Ws = (a_[2], a_[3]) if len(a_) > 3 else (256, 512)
ROUNDS, REPS = (a_[4], a_[5]) if len(a_) > 5 else (7, 20)
L = _lib.lib()
dev = "cuda"
g0 = torch.Generator(device=dev).manual_seed(0)
fx = W / (2 * math.tan(math.radians(60.0) / 2))
f = np.array([0.3, -0.2, 1.0]); f /= np.linalg.norm(f)
xax = np.cross([0.0, 1.0, 0.0], f); xax /= np.linalg.norm(xax)
vm = np.eye(4, dtype=np.float32); vm[0, :3], vm[1, :3], vm[2, :3] = xax, np.cross(f, xax), f
vm = np.ascontiguousarray(vm.reshape(-1))
K = np.array([fx, 0, W / 2, 0, fx, H / 2, 0, 0, 1], dtype=np.float32)
vp, kp = vm.ctypes.data_as(_lib.ctypes.c_void_p), K.ctypes.data_as(_lib.ctypes.c_void_p)
sky = torch.rand((Hs, Ws, 3), device=dev, generator=g0)
acc = torch.zeros((Hs, Ws, 3), dtype=torch.int64, device=dev)
grad = torch.zeros((Hs, Ws, 3), device=dev)
x = torch.rand((H, W, 3), device=dev, generator=g0)
g = (torch.rand((H, W, 3), device=dev, generator=g0) - 0.5) * (2.0 / (3 * H * W))  # a training cotangent's size
alphas = torch.rand((H, W), device=dev, generator=g0)
v_alphas = torch.empty((H, W), device=dev)
st = (1, 3 * W, 3)
n28, n20 = H * W * 7 // 2, H * W * 5 // 2  # floats: a copy reads and writes each byte once
src28, dst28 = torch.rand((n28,), device=dev, generator=g0), torch.empty((n28,), device=dev)
src20, dst20 = torch.rand((n20,), device=dev, generator=g0), torch.empty((n20,), device=dev)


def fwd():
    check(L.clmgs_sky_fwd(stream(), H, W, dptr(x), *st, dptr(alphas), vp, kp, dptr(sky), Hs, Ws, dptr(x), *st))


def bwd():
    check(L.clmgs_sky_bwd(stream(), H, W, dptr(g), *st, dptr(alphas), vp, kp, dptr(sky), Hs, Ws, dptr(v_alphas), dptr(acc)))


def convert():
    check(L.clmgs_sky_grad_convert(stream(), acc.numel(), dptr(acc), dptr(grad)))


def copy28():
    dst28.copy_(src28)


def copy20():
    dst20.copy_(src20)


def window(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(REPS):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / REPS


res = {"image": [W, H], "map": [Hs, Ws], "lib": _lib.LIB_PATH.split("/")[-1], "bytes_fwd": 28 * H * W, "bytes_bwd": 20 * H * W}
kernels = [("fwd_in_place", fwd), ("copy28", copy28), ("bwd", bwd), ("copy20", copy20), ("grad_convert", convert)]
times = {k: [] for k, _ in kernels}
for rnd in range(ROUNDS + 1):  # round 0 warms every kernel up
    for k, fn in kernels:
        if rnd == 0:
            for _ in range(2):
                fn()
            torch.cuda.synchronize()
        else:
            times[k].append(window(fn))
for k, t in times.items():
    res[f"{k}_ms"] = {"median": round(statistics.median(t), 4), "min": round(min(t), 4), "max": round(max(t), 4)}
for k, c, nbytes in (("fwd_in_place", "copy28", 28), ("bwd", "copy20", 20)):
    ratios = [a / b for a, b in zip(times[k], times[c])]
    res[f"{k}_over_{c}"] = {"median": round(statistics.median(ratios), 4), "min": round(min(ratios), 4), "max": round(max(ratios), 4)}
    res[f"{k}_TB_per_s"] = round(nbytes * H * W / (statistics.median(times[k]) * 1e-3) / 1e12, 3)
    res[f"{c}_TB_per_s"] = round(nbytes * H * W / (statistics.median(times[c]) * 1e-3) / 1e12, 3)
res["bwd_addends_per_s"] = round(12 * H * W / (statistics.median(times["bwd"]) * 1e-3) / 1e9, 2)  # G/s, zero addends included
# the window rule on a sample of tiles (host, float64): how many go through the LDS window
ty = torch.arange(0, H, 16)[:: max(1, (H // 16) // 24)]
tx = torch.arange(0, W, 16)[:: max(1, (W // 16) // 32)]
py, px = torch.meshgrid(torch.arange(16, dtype=torch.float64), torch.arange(16, dtype=torch.float64), indexing="ij")
R3 = torch.from_numpy(vm.reshape(4, 4)[:3, :3].astype(np.float64))
lds = tot = 0
words = []
for y0 in ty.tolist():
    for x0 in tx.tolist():
        yy, xx = (py + y0).clamp(max=H - 1), (px + x0).clamp(max=W - 1)
        dc = torch.stack([(xx + 0.5 - W / 2) / fx, (yy + 0.5 - H / 2) / fx, torch.ones_like(xx)], -1)
        d = (dc / dc.norm(dim=-1, keepdim=True)) @ R3
        u = (torch.atan2(d[..., 0], d[..., 2]) / (2 * math.pi) + 0.5) * Ws - 0.5
        v = (torch.asin(d[..., 1].clamp(-1, 1)) / math.pi + 0.5) * Hs - 0.5
        iu, jv = torch.floor(u), torch.floor(v)
        wc = int(iu.max() - iu.min()) + 2
        wr = int((jv + 1).clamp(0, Hs - 1).max() - jv.clamp(0, Hs - 1).min()) + 1
        tot += 1
        if wc * wr <= 256:
            lds += 1
            words.append(wc * wr * 3)
res["tiles_sampled"], res["tiles_through_the_window"] = tot, lds
res["window_words_mean"] = round(sum(words) / max(1, len(words)), 1)
torch.cuda.synchronize()
res["y_mean"], res["v_alphas_abs_mean"] = float(x.double().mean()), float(v_alphas.double().abs().mean())
convert()
res["map_gradient_abs_sum"] = float(grad.double().abs().sum())
for k, v in res.items():
    print(k, v)
