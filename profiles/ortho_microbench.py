"""The orthographic projection forward (csrc/ortho.hip) against the pinhole one (csrc/projection.hip) on the same rows and
image, in ONE process:
    python profiles/ortho_microbench.py [rows] [rounds] [reps]
Each round times `reps` back-to-back launches of clmgs_projection_fwd, then of clmgs_projection_ortho_fwd (four outputs,
no compensations: the same 28 B written per pair), event-timed on the launch stream; the order of the two legs alternates
from round to round.  Median, minimum and maximum per launch over the rounds, and the bytes moved per second.  No speed
is claimed for the orthographic kernel; this shows it streams like its sibling."""
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from clm_gs_amd import _lib  # noqa: E402
from clm_gs_amd._lib import check, dptr  # noqa: E402
from clm_gs_amd.synthetic import synth_gaussians  # noqa: E402

N = int(sys.argv[1]) if len(sys.argv) > 1 else 28_000_000
rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 9
reps = int(sys.argv[3]) if len(sys.argv) > 3 else 10
W, H = 4096, 4096
sc = synth_gaussians(N, seed=0, device="cuda")
means = sc["xyz"].contiguous()
quats = torch.nn.functional.normalize(sc["rotation"]).contiguous()
scales = torch.exp(sc["scaling"]).contiguous()
L_ext = sc["extent"]
del sc
height = 0.1 * L_ext + 0.35 * L_ext  # both cameras see about the same share of the slab
w2c = torch.eye(4)
w2c[:3, :3] = torch.tensor([[1.0, 0, 0], [0, -1.0, 0], [0, 0, -1.0]])
w2c[2, 3] = height
vm = w2c[None].cuda().contiguous()
f = 0.8 * W
K_pin = torch.tensor([[[f, 0, W / 2], [0, f, H / 2], [0, 0, 1.0]]], device="cuda")
K_ortho = torch.tensor([[[f / height, 0, W / 2], [0, f / height, H / 2], [0, 0, 1.0]]], device="cuda")  # same scale at depth `height`
radii = torch.empty((1, N), dtype=torch.int32, device="cuda")
m2, d, cn = (torch.empty((1, N, k), device="cuda") for k in (2, 1, 3))
L = _lib.lib()
st = _lib.stream()
common = lambda K: (st, 1, N, dptr(means), dptr(quats), dptr(scales), dptr(vm), dptr(K), W, H, 0.3, 0.01, 1e10, 0.0,
                    dptr(radii), dptr(m2), dptr(d), dptr(cn))
legs = {
    "pinhole": lambda: check(L.clmgs_projection_fwd(*common(K_pin))),
    "ortho": lambda: check(L.clmgs_projection_ortho_fwd(*common(K_ortho), None)),
}


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / reps


visible = {}
for name, fn in legs.items():  # warm-up, and the share of rows each camera keeps
    fn()
    torch.cuda.synchronize()
    visible[name] = int((radii > 0).sum())
times = {k: [] for k in legs}
for r in range(rounds):
    for name in (("pinhole", "ortho") if r % 2 == 0 else ("ortho", "pinhole")):
        times[name].append(timed(legs[name]))
res = dict(rows=N, rounds=rounds, reps=reps, visible=visible)
for name, t in times.items():
    med = statistics.median(t)
    res[name] = dict(median_ms=round(med, 4), min_ms=round(min(t), 4), max_ms=round(max(t), 4),
                     gb_per_s=round(N * (40 + 28) / med / 1e6, 1))
res["ortho_over_pinhole"] = round(res["ortho"]["median_ms"] / res["pinhole"]["median_ms"], 4)
print(json.dumps(res))
