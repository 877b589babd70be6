"""Slot-route tile backward, plain against absgrad, on one camera of the bench scene (28 M slab, 4608x3456):
    python profiles/raster_abs_microbench.py [slab|heavy] [reps] [rounds]
One forward of camera 1 through the fused path (fused.camera_forward, exact sizes) gives the camera's lists, records,
emit slots and the loss cotangent.  Then, after a warm-up of each leg, `rounds` rounds of `reps` back-to-back launches
per leg, the legs alternated within a round so that both see the same box and clocks; event-timed on the launch stream;
the median round per leg is reported.  Legs: clmgs_rasterize_bwd / clmgs_rasterize_abs_bwd in slot mode (the engine's
form: partial lines out, no row sum), and clmgs_preprocess_bwd / clmgs_preprocess_abs_bwd summing those lines into
scratch gradient tables.  The yardstick is the plain kernel of the same run."""
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
part = {k: torch.empty((max(I, 1), 16), device="cuda") for k in ("plain", "abs")}


def raster(kind_):
    fn, extra = (L.clmgs_rasterize_abs_bwd, (None,)) if kind_ == "abs" else (L.clmgs_rasterize_bwd, ())
    check(fn(st, 1, V, I, dptr(p.packed), None, W, H, 16, tw, th, dptr(p.offsets), dptr(p.fids), dptr(p.alphas),
             dptr(p.last_ids), dptr(p.v_out), None, None, None, None, None, None, dptr(p.emit_slot), dptr(p.row_cum),
             dptr(part[kind_]), *extra))


# the front-end backward on those lines: scratch gradient and statistics tables of the model's size
vm, K, campos = p.cam
g_small = [torch.zeros_like(t) for t in (m._xyz, m._opacity, m._scaling, m._rotation)]
g_sh = torch.zeros_like(m._parameters.data)
stats = [torch.zeros(m._xyz.shape[0], device="cuda") for _ in range(3)]


def front(kind_):
    fn, extra = (L.clmgs_preprocess_abs_bwd, (None,)) if kind_ == "abs" else (L.clmgs_preprocess_bwd, ())
    check(fn(st, V, dptr(p.filt, torch.int64, True), *p.small_in, dptr(m._parameters.data), 1, fused._np(vm), fused._np(K),
             fused._np(campos), W, H, p.deg, 0.3, dptr(p.radii), None, *[dptr(t) for t in g_small], dptr(g_sh),
             *[dptr(t) for t in stats], None, 0, dptr(part[kind_]), dptr(p.row_cum), None, None, 0, *extra))


legs = {"raster_plain": lambda: raster("plain"), "raster_abs": lambda: raster("abs"),
        "front_plain": lambda: front("plain"), "front_abs": lambda: front("abs")}
for fn in legs.values():  # warm-up of each leg (and the partial lines the front-end legs read)
    fn()
torch.cuda.synchronize()
assert torch.equal(part["plain"][:I, :10], part["abs"][:I, :10]), "words 0..9 of the partial lines are the plain kernel's"
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
med = {k: statistics.median(v) for k, v in times.items()}
a = part["abs"][:I, 10:12].double()
print(json.dumps({"lib": os.path.basename(_lib.LIB_PATH), "scene": kind, "V": V, "I_emitted": I, "reps": reps, "rounds": rounds,
                  "rasterize_bwd_slot_ms": round(med["raster_plain"], 4), "rasterize_abs_bwd_slot_ms": round(med["raster_abs"], 4),
                  "raster_ratio": round(med["raster_abs"] / med["raster_plain"], 4),
                  "preprocess_bwd_ms": round(med["front_plain"], 4), "preprocess_abs_bwd_ms": round(med["front_abs"], 4),
                  "front_ratio": round(med["front_abs"] / med["front_plain"], 4),
                  "spread_ms": {k: [round(min(v), 4), round(max(v), 4)] for k, v in times.items()},
                  "abs_pair_sum": float(a.sum()), "signed_xy_abs_sum": float(part["abs"][:I, 0:2].double().abs().sum())}))
