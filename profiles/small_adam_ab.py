"""A/B of the packed small-attribute Adam kernel: this build's clmgs_adam_small_packed against another build's (path of
its libclmgs_hip.so as argv[1]) in ONE process on one box, 28 M rows, first-touch stamps on 38 % of the rows; and
clmgs_adam_small_deferred on the same tables (every block four steps behind, flushed)."""
import ctypes
import json
import sys
import time

import torch

sys.path.insert(0, ".")
from clm_gs_amd import _lib

n = 28_000_000
other = ctypes.CDLL(sys.argv[1]) if len(sys.argv) > 1 else None
g = torch.Generator(device="cuda").manual_seed(0)
widths = (3, 1, 3, 4)
ps = [torch.randn(n, w, device="cuda", generator=g) for w in widths]
ms = [torch.zeros(n, w, device="cuda") for w in widths]
vs = [torch.zeros(n, w, device="cuda") for w in widths]
pk = torch.zeros(n, 12, device="cuda")
gk = torch.randn(n, 12, device="cuda", generator=g)
stamp = torch.where(torch.rand(n, device="cuda", generator=g) < 0.38, 7, 3).to(torch.int32)
arr = lambda xs: (ctypes.c_void_p * 4)(*[x.data_ptr() for x in xs])
lrs = (ctypes.c_double * 4)(1e-4, 5e-2, 5e-3, 1e-3)
VP, I64, D, I, F = ctypes.c_void_p, ctypes.c_int64, ctypes.c_double, ctypes.c_int, ctypes.c_float


def call(lib, step, ranged):
    f = lib.clmgs_adam_small_packed_range  # ranged: the per-row range test of camera-DP's row owners (all rows but 2 000)
    f.restype = I
    f.argtypes = [VP, I64, I64, I64, VP, VP, VP, VP, VP, VP, D, D, D, I, I, F, VP, I]
    lo, hi = (1000, n - 1000) if ranged else (0, -1)
    rc = f(_lib.stream(), n, lo, hi, arr(ps), arr(ms), arr(vs), lrs, pk.data_ptr(), gk.data_ptr(), 0.9, 0.999, 1e-15, step,
           1, 0.25, stamp.data_ptr(), 7)
    assert rc == 0


def timed(lib, ranged=False, reps=20):
    for s in range(3):
        call(lib, 1 + s, ranged)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for s in range(reps):
        call(lib, 4 + s, ranged)
    torch.cuda.synchronize()
    return round((time.perf_counter() - t0) / reps * 1e3, 4)


# the deferred form, like for like: every block four steps behind, flushed (no cameras), the same stamps waiting
blk = torch.empty((n + 255) // 256, dtype=torch.int32, device="cuda")
hist_lr = (ctypes.c_double * 16)(*([1e-4, 5e-2, 5e-3, 1e-3] * 4))
hist_idx = (ctypes.c_int32 * 4)(10, 9, 8, 7)
margins = (ctypes.c_float * 5)(*[1e-12 + 0.1 * k for k in range(5)])
gains = (ctypes.c_float * 5)(*[1.001 + 0.01 * k for k in range(5)])


def call_deferred(lib):
    f = lib.clmgs_adam_small_deferred
    f.restype = I
    f.argtypes = [VP, I64, VP, VP, VP, VP, VP, VP, VP, I, I, VP, VP, VP, VP, D, D, D, F, I, VP, VP, I, I, F, F, F, I, VP]
    blk.fill_(6)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    rc = f(_lib.stream(), n, arr(ps), arr(ms), arr(vs), pk.data_ptr(), gk.data_ptr(), stamp.data_ptr(), blk.data_ptr(), 10,
           4, hist_lr, hist_idx, margins, gains, 0.9, 0.999, 1e-15, 0.25, 0, None, None, 0, 0, 0.3, 0.01, 1e10, 1, None)
    e1.record()
    assert rc == 0
    return e0, e1


def timed_deferred(lib, reps=10):
    for _ in range(2):
        call_deferred(lib)
    evs = [call_deferred(lib) for _ in range(reps)]
    torch.cuda.synchronize()
    return round(sorted(a.elapsed_time(b) for a, b in evs)[reps // 2], 4)


res = {}
for rnd in range(3):
    this = ctypes.CDLL(_lib.LIB_PATH)
    res.setdefault("this_build_ms", []).append(timed(this))
    res.setdefault("this_build_ranged_ms", []).append(timed(this, True))
    res.setdefault("this_build_deferred_ms", []).append(timed_deferred(this))
    if other is not None:
        res.setdefault("other_build_ms", []).append(timed(other))
        res.setdefault("other_build_ranged_ms", []).append(timed(other, True))
        res.setdefault("other_build_deferred_ms", []).append(timed_deferred(other))
print("SMALLADAM " + json.dumps(res))
