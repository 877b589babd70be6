"""Resolution schedule: the kernel of csrc/resample.hip against a device-to-device copy of the same source bytes, in one
process:  python profiles/resample_microbench.py [reps] [rounds]
Source: one uint8 [3,3456,4608] image (47.8 MB).  Legs, alternated within a round so that all see the same box and clocks,
`rounds` rounds of `reps` launches, event-timed; the median round per leg, in microseconds per launch:
  copy      dst.copy_(src): reads 47.8 MB, writes 47.8 MB
  u8_L1     clmgs_area_resample_u8 at level 1: reads 47.8 MB, writes 11.9 MB          (the exact instantiation)
  u8_L2     ... at level 2: reads 47.8 MB, writes 3.0 MB
  u8_L1_odd / u8_L2_odd   the same on [3,3455,4607]: the weighted instantiation, unaligned rows
  u16_L2    one uint16 [3456,4608] plane (31.9 MB) at level 2;  mask_L2  one uint8 plane (15.9 MB) + the count
Eight images are cycled through (382 MB: more than the 256 MiB Infinity Cache) so that every leg reads from HBM.
Prints one JSON line."""
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from clm_gs_amd import clm_kernels as K  # noqa: E402

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 16
rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 9
H, W, NSRC = 3456, 4608, 8
g = torch.Generator(device="cuda").manual_seed(0)
src = [(torch.rand((3, H, W), device="cuda", generator=g) * 256).to(torch.uint8) for _ in range(NSRC)]
odd = [s[:, :H - 1, :W - 1].contiguous() for s in src]
u16 = [(torch.rand((H, W), device="cuda", generator=g) * 65536).to(torch.int32).to(torch.uint16) for _ in range(NSRC)]
msk = [(torch.rand((H, W), device="cuda", generator=g) < 0.8).to(torch.uint8) for _ in range(NSRC)]
copy_dst = torch.empty_like(src[0])
count = torch.zeros((1,), dtype=torch.int64, device="cuda")


def out_for(t, level):
    return torch.empty(tuple(t.shape[:-2]) + K.level_size(t.shape[-2], t.shape[-1], level), dtype=t.dtype, device="cuda")


outs = {("u8", 1): out_for(src[0], 1), ("u8", 2): out_for(src[0], 2), ("odd", 1): out_for(odd[0], 1),
        ("odd", 2): out_for(odd[0], 2), ("u16", 2): out_for(u16[0], 2), ("mask", 2): out_for(msk[0], 2)}
legs = {
    "copy": lambda i: copy_dst.copy_(src[i]),
    "u8_L1": lambda i: K.area_resample(src[i], 1, out=outs["u8", 1]),
    "u8_L2": lambda i: K.area_resample(src[i], 2, out=outs["u8", 2]),
    "u8_L1_odd": lambda i: K.area_resample(odd[i], 1, out=outs["odd", 1]),
    "u8_L2_odd": lambda i: K.area_resample(odd[i], 2, out=outs["odd", 2]),
    "u16_L2": lambda i: K.area_resample(u16[i], 2, out=outs["u16", 2]),
    "mask_L2": lambda i: K.area_resample(msk[i], 2, out=outs["mask", 2], mask=True, count=count),
}
for fn in legs.values():  # warm-up: every shape of the timed window
    for i in range(NSRC):
        fn(i)
torch.cuda.synchronize()
times = {k: [] for k in legs}
for _ in range(rounds):
    for name, fn in legs.items():
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for r in range(reps):
            fn(r % NSRC)
        b.record()
        b.synchronize()
        times[name].append(a.elapsed_time(b) * 1e3 / reps)
res = {"size": [W, H], "reps": reps, "rounds": rounds,
       "us_median": {k: round(statistics.median(v), 2) for k, v in times.items()},
       "us_min_max": {k: [round(min(v), 2), round(max(v), 2)] for k, v in times.items()}}
src_bytes = 3 * H * W
res["source_GBps"] = {k: round(src_bytes / (res["us_median"][k] * 1e-6) / 1e9, 1) for k in ("copy", "u8_L1", "u8_L2")}
print(json.dumps(res))
