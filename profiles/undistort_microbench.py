"""Lens distortion: the kernel of csrc/undistort.hip against a device-to-device copy of the same image bytes, in one
process:  python profiles/undistort_microbench.py [reps] [rounds]
Source: one uint8 [3,3456,4608] image (47.8 MB) onto the centred pinhole of the same size.  Legs, alternated within a round
so that all see the same box and clocks, `rounds` rounds of `reps` launches, event-timed; the median round per leg, in
microseconds per launch:
  copy           dst.copy_(src): reads 47.8 MB, writes 47.8 MB
  opencv         clmgs_undistort_u8, an OPENCV lens: reads 47.8 MB (every source pixel once, through the cache), writes
                 47.8 MB
  opencv_valid   ... with the valid map (+ 15.9 MB written) and the count
  opencv_masked  ... and a source mask (+ 15.9 MB read)
  fisheye_valid  an OPENCV_FISHEYE lens at zoom 0.8 with the valid map and the count
  u16            clmgs_undistort_u16, one uint16 [3456,4608] plane (31.9 MB read, 31.9 MB written), the OPENCV lens
Eight images are cycled through (382 MB: more than the 256 MiB Infinity Cache) so that every leg reads from HBM.
Prints one JSON line."""
import ctypes
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from clm_gs_amd import _lib  # noqa: E402
from clm_gs_amd import clm_kernels as K  # noqa: E402

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 16
rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 9
H, W, NSRC = 3456, 4608, 8
g = torch.Generator(device="cuda").manual_seed(0)
src = [(torch.rand((3, H, W), device="cuda", generator=g) * 256).to(torch.uint8) for _ in range(NSRC)]
u16 = [(torch.rand((H, W), device="cuda", generator=g) * 65536).to(torch.int32).to(torch.uint16) for _ in range(NSRC)]
msk = [(torch.rand((H, W), device="cuda", generator=g) < 0.98).to(torch.uint8) for _ in range(NSRC)]
copy_dst, dst, dst16 = torch.empty_like(src[0]), torch.empty_like(src[0]), torch.empty_like(u16[0])
valid = torch.empty((H, W), dtype=torch.uint8, device="cuda")
count = torch.zeros((1,), dtype=torch.int64, device="cuda")
opencv = K.Lens("OPENCV", (3900.0, 3880.0, W / 2 + 11.3, H / 2 - 7.6, -0.12, 0.03, 0.0004, -0.0003), W, H)
fisheye = K.Lens("OPENCV_FISHEYE", (2400.0, 2390.0, W / 2 + 11.3, H / 2 - 7.6, -0.04, 0.01, -0.003, 0.0007), W, H)
L = _lib.lib()


def u8(i, lens, zoom, mask=None, want=False):  # the entry itself with preallocated outputs: nothing is allocated per launch
    rec = (ctypes.c_double * 10)(*lens.record())
    _lib.check(L.clmgs_undistort_u8(_lib.stream(), 3, H, W, H, W, rec, int(lens.fisheye), lens.fx * zoom, lens.fy * zoom,
                                    _lib.dptr(src[i]), _lib.dptr(mask, allow_none=True), _lib.dptr(dst),
                                    _lib.dptr(valid if want else None, allow_none=True),
                                    _lib.dptr(count if want else None, allow_none=True)))


legs = {
    "copy": lambda i: copy_dst.copy_(src[i]),
    "opencv": lambda i: u8(i, opencv, 1.0),
    "opencv_valid": lambda i: u8(i, opencv, 1.0, want=True),
    "opencv_masked": lambda i: u8(i, opencv, 1.0, mask=msk[i], want=True),
    "fisheye_valid": lambda i: u8(i, fisheye, 0.8, want=True),
    "u16": lambda i: K.undistort(u16[i], opencv, out=dst16),
}
for fn in legs.values():  # warm-up: every shape of the timed window
    for i in range(NSRC):
        fn(i)
torch.cuda.synchronize()
lost = {}
for name in ("opencv_valid", "fisheye_valid"):
    legs[name](0)
    lost[name] = round(1.0 - int(count.item()) / float(H * W), 4)
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
       "us_min_max": {k: [round(min(v), 2), round(max(v), 2)] for k, v in times.items()},
       "share_without_source": lost}
res["ratio_to_copy"] = {k: round(res["us_median"][k] / res["us_median"]["copy"], 2) for k in legs if k != "copy"}
print(json.dumps(res))
