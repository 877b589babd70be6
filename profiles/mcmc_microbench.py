"""MCMC densification: the two per-batch passes of csrc/mcmc.hip against device copies of the bytes they must move, at
the bench scene's row count (28 M):
    python profiles/mcmc_microbench.py [rows] [reps] [rounds]
Legs, alternated within a round so that all see the same box and clocks, `rounds` rounds of `reps` launches, event-timed;
the median round per leg:
  noise         clmgs_mcmc_noise on xyz / opacity / scaling / rotation / noise     | 68 B per row: xyz read + written 24,
                                                                                    noise 12, scaling 12, rotation 16, opacity 4
  noise_mirror  the same with the packed [N,12] mirror (columns 0..2 written)      | 80 B per row
  noise_unaligned  the same tensors one float off 16 B alignment (the rotation read as four dwords instead of 16 B)
  randn         torch.randn((N,3)) from a device generator: what drawing the noise adds (12 B per row written)
  reg           clmgs_mcmc_reg_grad on the four separate tensors                   | 48 B per row: opacity 4, scaling 12, their
                                                                                    gradients read + written 32
  reg_packed    the same on the packed [N,12] parameter and gradient tables        | 48 B per row needed; two 48 B rows touched
  relocation    clmgs_mcmc_relocation on 1.4 M rows (5 % of 28 M), ratios 1..51 (once per refinement; for the record)
A copy "moving n bytes" copies n / 2 bytes (read + written)."""
import json
import math
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from clm_gs_amd import clm_kernels as K  # noqa: E402

N = int(sys.argv[1]) if len(sys.argv) > 1 else 28_000_000
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 10
rounds = int(sys.argv[3]) if len(sys.argv) > 3 else 5
dev = "cuda"
g = torch.Generator(device=dev).manual_seed(0)
xyz = torch.randn((N, 3), device=dev, generator=g) * 50
opacity = torch.randn((N, 1), device=dev, generator=g) * 1.5
opacity[::16] = math.log(0.004 / 0.996)  # some open gates
scaling = torch.randn((N, 3), device=dev, generator=g) * 0.4 - 4.0
rotation = torch.randn((N, 4), device=dev, generator=g)
noise = torch.randn((N, 3), device=dev, generator=g)
g_o, g_s = torch.zeros((N, 1), device=dev), torch.zeros((N, 3), device=dev)
pk, gk = torch.randn((N, 12), device=dev, generator=g), torch.zeros((N, 12), device=dev)
pk[:, 3:4], pk[:, 4:7] = opacity, scaling


def off(t):
    big = torch.empty(t.numel() + 1, device=dev)
    big[1:] = t.flatten()
    return big[1:].view(t.shape)


u = [off(t) for t in (xyz, opacity, scaling, rotation, noise)]
M = N // 20
ro = torch.rand((M,), device=dev, generator=g) * 0.98 + 0.005
rs = torch.rand((M, 3), device=dev, generator=g)
rr = torch.randint(1, 52, (M,), device=dev, generator=g, dtype=torch.int32)
SCALER = 1e-9  # (the arithmetic does not depend on it; positions stay where they are over thousands of launches)


def copy_leg(nbytes):
    a = torch.empty((nbytes // 8,), dtype=torch.float32, device=dev)
    b = torch.empty_like(a)
    return lambda: b.copy_(a)


legs = {
    "noise": lambda: K.mcmc_inject_noise_(xyz, opacity, scaling, rotation, noise, SCALER),
    "copy_68B": copy_leg(68 * N),
    "noise_mirror": lambda: K.mcmc_inject_noise_(xyz, opacity, scaling, rotation, noise, SCALER, packed=pk),
    "copy_80B": copy_leg(80 * N),
    "noise_unaligned": lambda: K.mcmc_inject_noise_(*u, SCALER),
    "randn": lambda: torch.randn((N, 3), dtype=torch.float32, device=dev, generator=g),
    "copy_12B": copy_leg(12 * N),
    "reg": lambda: K.mcmc_reg_grad_(1e-9, 1e-9, opacity, scaling, g_o, g_s),
    "reg_packed": lambda: K.mcmc_reg_grad_(1e-9, 1e-9, packed=pk, packed_grad=gk),
    "copy_48B": copy_leg(48 * N),
    "relocation": lambda: K.mcmc_relocation(ro, rs, rr),
}
times = {k: [] for k in legs}
for fn in legs.values():  # warm-up (lazily loaded device code)
    fn()
torch.cuda.synchronize()
for _ in range(rounds):
    for name, fn in legs.items():
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        for _ in range(reps):
            fn()
        e.record()
        e.synchronize()
        times[name].append(s.elapsed_time(e) / reps)
med = {k: statistics.median(v) for k, v in times.items()}
spread = {k: (max(v) - min(v)) / statistics.median(v) for k, v in times.items()}
pairs = (("noise", "copy_68B", 68), ("noise_mirror", "copy_80B", 80), ("noise_unaligned", "copy_68B", 68),
         ("randn", "copy_12B", 12), ("reg", "copy_48B", 48), ("reg_packed", "copy_48B", 48))
print(f"rows {N}, {rounds} rounds of {reps} launches, median round; spread = (max - min) / median over the rounds")
print(f"{'leg':16s} {'B/row':>6s} {'ms':>9s} {'copy ms':>9s} {'ratio':>6s} {'GB/s needed':>12s} {'spread':>7s}")
for leg, cp, nb in pairs:
    print(f"{leg:16s} {nb:6d} {med[leg]:9.4f} {med[cp]:9.4f} {med[leg] / med[cp]:6.2f} {nb * N / med[leg] / 1e6:12.0f} "
          f"{spread[leg]:7.3f}")
print(f"{'relocation':16s} {M} rows: {med['relocation']:.4f} ms")
print(json.dumps({"rows": N, "reps": reps, "rounds": rounds, "ms": {k: round(v, 5) for k, v in med.items()},
                  "spread": {k: round(v, 4) for k, v in spread.items()}}))
