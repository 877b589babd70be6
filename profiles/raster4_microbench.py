"""3-channel vs 4-channel tile kernels on one camera of the bench scene (28 M slab, 4608x3456):
    python profiles/raster4_microbench.py [slab|heavy] [reps] [rounds]
One forward of camera 1 through the fused path (fused.camera_forward, exact sizes) gives the camera's lists and its
records; conics / colours / opacities are read back out of the `packed` records and the depths from the pass object,
and packed again with the depth as fourth channel through clmgs_rasterize4_fwd.  Then, after a warm-up of each shape,
`rounds` rounds of `reps` back-to-back launches per leg, the legs alternated within a round so that all of them see
the same box and clocks; event-timed on the launch stream; the median round per leg is reported.
Forward legs: clmgs_rasterize_fwd / clmgs_rasterize4_fwd on records already packed (means2d = NULL: the tile kernel
alone).  Backward legs: the atomic route of both (emit_slot = NULL, packed gradient lines out, no unpack), the same RGB
cotangents (the loss gradient of the fused pass) and a seeded N(0, 1/100) cotangent on the depth channel."""
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from clm_gs_amd import _lib, fused, utils  # noqa: E402
from clm_gs_amd._lib import check, dptr  # noqa: E402
from clm_gs_amd.strategies.base_engine import select_filters  # noqa: E402
from clm_gs_amd.strategies.clm_offload import GaussianModelCLMOffload  # noqa: E402
from clm_gs_amd.synthetic import nadir_cameras, synth_gaussians  # noqa: E402

kind = sys.argv[1] if len(sys.argv) > 1 else "slab"
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 10
rounds = int(sys.argv[3]) if len(sys.argv) > 3 else 5
N, W, H = 28_000_000, 4608, 3456
args = utils.default_args(bsz=4, sh_residency="hbm")
args.clm_offload = True
utils.set_args(args)
utils.set_img_size(H, W)
sc = synth_gaussians(N, seed=0, device="cuda", kind=kind)
order = utils.morton_order(sc["xyz"])
for k in ("xyz", "scaling", "rotation", "opacity", "shs48"):
    sc[k] = utils.gather_rows(sc[k], order)
m = GaussianModelCLMOffload(3, only_for_rendering=True)
m.create_from_tensors(sc["xyz"], sc["shs48"], sc["scaling"], sc["rotation"], sc["opacity"])
m.active_sh_degree = 3
cam = nadir_cameras(4, N, W, H, 0.10, seed=0, device="cuda")[1]
with torch.no_grad():
    filters, _ = select_filters([cam], m._xyz.detach(), m._scaling.detach(), m._rotation.detach())
f = filters[0]
g = torch.Generator().manual_seed(1)
cam.original_image = (torch.rand(3, H, W, generator=g) * 255).to(torch.uint8).cuda()
p = fused.camera_forward(m, cam, f, m._parameters.data, 1, None, cam.original_image)
torch.cuda.synchronize()
L = _lib.lib()
V, I = p.V, p.fids.numel()
tw, th = (W + 15) // 16, (H + 15) // 16
st = _lib.stream()

# the camera's operator inputs out of its records: x y o ca | cb cc r g | b
rec = p.packed[:V]
means2d, opac = rec[:, 0:2].contiguous(), rec[:, 2].contiguous()
conics, colors = rec[:, 3:6].contiguous(), rec[:, 6:9].contiguous()
depths = p.aux[[t is p.means2d for t in p.aux].index(True) + 1].reshape(-1)[:V]  # (means2d, depths) of the front end
visible = p.radii.reshape(-1)[:V] > 0
colors4 = torch.cat([colors, torch.where(visible, depths, torch.zeros_like(depths))[:, None]], 1).contiguous()
packed4 = torch.empty_like(rec)
out3, out4 = torch.empty((H, W, 3), device="cuda"), torch.empty((H, W, 4), device="cuda")
al, last = torch.empty_like(p.alphas), torch.empty_like(p.last_ids)
check(L.clmgs_rasterize4_fwd(st, 1, V, I, dptr(means2d), dptr(conics), dptr(colors4), dptr(opac), None, W, H, 16, tw, th,
                             dptr(p.offsets), dptr(p.fids), dptr(packed4), dptr(out4), dptr(al), dptr(last)))
torch.cuda.synchronize()
assert torch.equal(out4[..., :3], p.out) and torch.equal(last, p.last_ids) and torch.equal(al, p.alphas)
g = torch.Generator().manual_seed(2)
v4 = torch.cat([p.v_out, (0.01 * torch.randn(H, W, 1, generator=g)).cuda()], 2).contiguous()
pg3, pg4 = torch.empty_like(rec), torch.empty_like(rec)

legs = {
    "fwd3": lambda: check(L.clmgs_rasterize_fwd(st, 1, V, I, None, None, None, None, None, W, H, 16, tw, th, dptr(p.offsets),
                                                dptr(p.fids), dptr(p.packed), dptr(out3), dptr(al), dptr(last))),
    "fwd4": lambda: check(L.clmgs_rasterize4_fwd(st, 1, V, I, None, None, None, None, None, W, H, 16, tw, th, dptr(p.offsets),
                                                 dptr(p.fids), dptr(packed4), dptr(out4), dptr(al), dptr(last))),
    "bwd3": lambda: check(L.clmgs_rasterize_bwd(st, 1, V, I, dptr(p.packed), None, W, H, 16, tw, th, dptr(p.offsets),
                                                dptr(p.fids), dptr(p.alphas), dptr(p.last_ids), dptr(p.v_out), None,
                                                dptr(pg3), None, None, None, None, None, None, None)),
    "bwd4": lambda: check(L.clmgs_rasterize4_bwd(st, 1, V, I, dptr(packed4), None, W, H, 16, tw, th, dptr(p.offsets),
                                                 dptr(p.fids), dptr(p.alphas), dptr(p.last_ids), dptr(v4), None,
                                                 dptr(pg4), None, None, None, None, None, None, None)),
}
for fn in legs.values():  # warm-up of each shape
    fn()
torch.cuda.synchronize()
times = {k: [] for k in legs}
for _ in range(rounds):
    for k, fn in legs.items():
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        times[k].append(e0.elapsed_time(e1) / reps)
assert torch.equal(out3, p.out) and torch.equal(out4[..., :3], p.out)
med = {k: statistics.median(v) for k, v in times.items()}
print(json.dumps({"lib": os.path.basename(_lib.LIB_PATH), "scene": kind, "V": V, "I_emitted": I, "reps": reps, "rounds": rounds,
                  "rasterize_fwd_ms": round(med["fwd3"], 4), "rasterize4_fwd_ms": round(med["fwd4"], 4),
                  "fwd_ratio": round(med["fwd4"] / med["fwd3"], 4),
                  "rasterize_bwd_atomic_ms": round(med["bwd3"], 4), "rasterize4_bwd_atomic_ms": round(med["bwd4"], 4),
                  "bwd_ratio": round(med["bwd4"] / med["bwd3"], 4),
                  "spread_ms": {k: [round(min(v), 4), round(max(v), 4)] for k, v in times.items()},
                  "depth_image_mean": float(out4[..., 3].double().mean()),
                  "v_depth_abs_sum": float(pg4[:, 9].double().abs().sum())}))
