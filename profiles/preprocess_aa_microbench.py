"""Fused front end, plain against antialiased, on one camera of the bench scene (28 M slab, 4608x3456):
    python profiles/preprocess_aa_microbench.py [slab|heavy] [reps] [rounds]
One forward of camera 1 through the fused path (fused.camera_forward, exact sizes) and one slot-route tile backward give
the camera's filter, radii, row ranges and partial gradient lines.  Then, after a warm-up of each leg, `rounds` rounds of
`reps` back-to-back launches per leg, the legs alternated within a round so that both see the same box and clocks;
event-timed on the launch stream; the median round per leg and the spread between rounds are reported.  Legs:
clmgs_preprocess_fwd / clmgs_preprocess_aa_fwd into scratch outputs, and clmgs_preprocess_bwd / clmgs_preprocess_aa_bwd
summing the same partial lines into scratch gradient and statistics tables.  The yardstick is the plain kernel of the
same run."""
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
part = torch.empty((max(I, 1), 16), device="cuda")
check(L.clmgs_rasterize_bwd(st, 1, V, I, dptr(p.packed), None, W, H, 16, tw, th, dptr(p.offsets), dptr(p.fids), dptr(p.alphas),
                            dptr(p.last_ids), dptr(p.v_out), None, None, None, None, None, None, dptr(p.emit_slot),
                            dptr(p.row_cum), dptr(part)))
vm, K, campos = p.cam
out = {k: dict(radii=torch.empty(V, dtype=torch.int32, device="cuda"), m2=torch.empty(V, 2, device="cuda"),
               dep=torch.empty(V, device="cuda"), packed=torch.empty(V, 16, device="cuda")) for k in ("plain", "aa")}
g_small = [torch.zeros_like(t) for t in (m._xyz, m._opacity, m._scaling, m._rotation)]
g_sh = torch.zeros_like(m._parameters.data)
stats = [torch.zeros(m._xyz.shape[0], device="cuda") for _ in range(3)]


def fwd(kind_):
    fn, o = (L.clmgs_preprocess_aa_fwd if kind_ == "aa" else L.clmgs_preprocess_fwd), out[kind_]
    check(fn(st, V, dptr(p.filt, torch.int64, True), *p.small_in, dptr(m._parameters.data), 1, fused._np(vm), fused._np(K),
             fused._np(campos), W, H, p.deg, 0.3, 0.01, 1e10, 0.0, dptr(o["radii"]), dptr(o["m2"]), dptr(o["dep"]), None, None,
             None, dptr(o["packed"]), None))


def bwd(kind_):
    fn = L.clmgs_preprocess_aa_bwd if kind_ == "aa" else L.clmgs_preprocess_bwd
    check(fn(st, V, dptr(p.filt, torch.int64, True), *p.small_in, dptr(m._parameters.data), 1, fused._np(vm), fused._np(K),
             fused._np(campos), W, H, p.deg, 0.3, dptr(p.radii), None, *[dptr(t) for t in g_small], dptr(g_sh),
             *[dptr(t) for t in stats], None, 0, dptr(part), dptr(p.row_cum), None, None, 0))


legs = {"fwd_plain": lambda: fwd("plain"), "fwd_aa": lambda: fwd("aa"), "bwd_plain": lambda: bwd("plain"), "bwd_aa": lambda: bwd("aa")}
for fn in legs.values():  # warm-up of each leg
    fn()
torch.cuda.synchronize()
assert torch.equal(out["plain"]["radii"], out["aa"]["radii"]) and torch.equal(out["plain"]["radii"], p.radii.reshape(-1)[:V])
keep = [0, 1, 3, 4, 5, 6, 7, 8]
assert torch.equal(out["plain"]["packed"][:, keep], out["aa"]["packed"][:, keep]), "only the opacity word moves"
vis = out["aa"]["radii"] > 0
comp = (out["aa"]["packed"][:, 2] / out["plain"]["packed"][:, 2])[vis]
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
print(json.dumps({"lib": os.path.basename(_lib.LIB_PATH), "scene": kind, "V": V, "visible": int(vis.sum()), "I_emitted": I,
                  "reps": reps, "rounds": rounds,
                  "preprocess_fwd_ms": round(med["fwd_plain"], 4), "preprocess_aa_fwd_ms": round(med["fwd_aa"], 4),
                  "fwd_ratio": round(med["fwd_aa"] / med["fwd_plain"], 4),
                  "preprocess_bwd_ms": round(med["bwd_plain"], 4), "preprocess_aa_bwd_ms": round(med["bwd_aa"], 4),
                  "bwd_ratio": round(med["bwd_aa"] / med["bwd_plain"], 4),
                  "spread_ms": {k: [round(min(v), 4), round(max(v), 4)] for k, v in times.items()},
                  "median_compensation": round(float(comp.median()), 4)}))
