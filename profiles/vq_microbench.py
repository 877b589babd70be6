"""The vector-quantisation kernels (csrc/vq.hip) at the sizes a model is compressed at:
    python profiles/vq_microbench.py [kernels|model|all] [reps]
kernels: clmgs_vq_assign at N = 2^22 and N = 28 M rows against K = 4096 and K = 65536 centroids, event-timed on the launch
stream after one warm-up launch of the same shape, the median of `reps` launches (one launch runs for long enough to be
its own window), reported as achieved f32 TFLOP/s = 2 N K 48 / t (the arithmetic the kernel does, the DC columns' zeros
included) next to the kernel guide's 122 TFLOP/s of an untuned LDS-tiled f32-MFMA GEMM; in the same process the obvious
torch restatement on the same data (row-chunked x @ c.T, + |c|^2, argmin; chunks of 2^28 / K rows) and the fraction of
rows on which the two agree; and clmgs_vq_accumulate as bytes of atomic traffic (8 B per row and column + 8 B per row)
per second next to the guide's ~1.3 TB/s of added bytes.  The shader and memory clocks are read before and after.
model: the wall time of compress.compress + save_compressed on the synthetic 28 M-row model (synthetic.synth_gaussians),
split into fit, full assignment, quantisation and file write (what compress_model logs)."""
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from clm_gs_amd import _lib, compress  # noqa: E402
from clm_gs_amd._lib import check, dptr  # noqa: E402
from clm_gs_amd.synthetic import synth_gaussians  # noqa: E402

what = sys.argv[1] if len(sys.argv) > 1 else "all"
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 3
N_BIG, GUIDE_TF, GUIDE_ATOMIC_TBS = 28_000_000, 122.0, 1.3


def clocks():
    try:
        out = subprocess.run(["rocm-smi", "--showclocks", "-d", "0"], capture_output=True, text=True, timeout=30).stdout
        return [l.strip() for l in out.splitlines() if "sclk" in l or "mclk" in l]
    except Exception as e:  # the numbers stand without it; say so
        return [f"not read: {e}"]


def timed(fn, n):
    ts = []
    for _ in range(n):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1))
    return statistics.median(ts), min(ts)


def torch_assign(x, c):
    """argmin_k |c_k|^2 - 2 x.c_k over columns 3..47, row-chunked so that the [chunk, K] scores stay at 1 GiB."""
    ct = c[:, 3:].t().contiguous()
    cn = (c[:, 3:] * c[:, 3:]).sum(1)
    chunk = max(1, (1 << 28) // c.shape[0])
    out = torch.empty(x.shape[0], dtype=torch.int64, device=x.device)
    for a in range(0, x.shape[0], chunk):
        out[a:a + chunk] = torch.addmm(cn[None], x[a:a + chunk, 3:], ct, alpha=-2.0).argmin(1)
    return out


def kernels():
    L, st = _lib.lib(), _lib.stream()
    g = torch.Generator(device="cuda").manual_seed(0)
    rows = torch.randn((N_BIG, 48), generator=g, device="cuda") * 0.1
    res = {"clocks_before": clocks(), "reps": reps, "legs": []}
    for n in (1 << 22, N_BIG):
        x = rows[:n]
        for K in (4096, 65536):
            cb = x[(torch.arange(K, device="cuda") * n) // K].contiguous() + 0.01
            idx = torch.empty(n, dtype=torch.int32, device="cuda")
            nb = int(L.clmgs_vq_assign_temp_bytes(K))
            temp = torch.empty(nb, dtype=torch.uint8, device="cuda")
            run = lambda: check(L.clmgs_vq_assign(st, n, K, dptr(x), dptr(cb), dptr(idx), None, dptr(temp), nb))
            run()
            torch.cuda.synchronize()
            med, lo = timed(run, reps)
            ref = torch_assign(x[:1 << 16], cb)  # warm-up of the torch shapes
            t_med, t_lo = timed(lambda: torch_assign(x, cb), 1 if n * K > 1 << 36 else reps)
            agree = float((torch_assign(x[:1 << 20], cb) == idx[:1 << 20].long()).double().mean())
            flop = 2.0 * n * K * 48
            leg = {"N": n, "K": K, "vq_assign_ms": round(med, 3), "vq_assign_min_ms": round(lo, 3),
                   "vq_assign_tflops": round(flop / med / 1e9, 2), "of_guide_122tf": round(flop / med / 1e9 / GUIDE_TF, 3),
                   "torch_ms": round(t_med, 3), "torch_tflops": round(flop / t_med / 1e9, 2),
                   "torch_over_kernel": round(t_med / med, 3), "agree_first_2^20_rows": agree}
            if K == 65536:
                acc = torch.zeros((K, 45), dtype=torch.int64, device="cuda")
                cnt = torch.zeros((K,), dtype=torch.int64, device="cuda")
                scale = 2.0 ** 30
                add = lambda: check(L.clmgs_vq_accumulate(st, n, K, dptr(x), dptr(idx), scale, dptr(acc), dptr(cnt)))
                add()
                torch.cuda.synchronize()
                a_med, a_lo = timed(add, max(reps, 5))
                nbytes = n * 46 * 8
                leg.update(vq_accumulate_ms=round(a_med, 3), atomic_gbs=round(nbytes / a_med / 1e6, 1),
                           of_guide_1p3tbs=round(nbytes / a_med / 1e9 / GUIDE_ATOMIC_TBS, 3))
            del ref
            res["legs"].append(leg)
            print(json.dumps(leg), flush=True)
    res["clocks_after"] = clocks()
    return res


def model():
    sc = synth_gaussians(N_BIG, seed=0, device="cuda")
    rows = {k: sc[k].cpu() for k in compress.KEYS}
    del sc
    torch.cuda.empty_cache()
    timings = {}
    t0 = time.perf_counter()
    arrays, meta = compress.compress(rows, timings=timings)
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "model.vq.npz")
        t1 = time.perf_counter()
        compress.save_compressed(path, arrays, meta)
        timings["write_s"] = time.perf_counter() - t1
        size = os.path.getsize(path)
    timings["total_s"] = time.perf_counter() - t0
    return {"rows": N_BIG, "bytes_before": N_BIG * 248, "bytes_arrays": compress.expected_nbytes(meta), "bytes_file": size,
            "K": meta["K"], "empty": meta["empty"], "distortion": meta["distortion"], "history": meta["history"],
            **{k: round(v, 2) for k, v in timings.items()}}


out = {"lib": os.path.basename(_lib.LIB_PATH), "device": torch.cuda.get_device_name(0)}
if what in ("kernels", "all"):
    out["kernels"] = kernels()
if what in ("model", "all"):
    out["model"] = model()
print(json.dumps(out))
