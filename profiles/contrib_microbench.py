"""The contribution kernel (csrc/contrib.hip) against the shipped forward tile kernel on the same lists, and the wall
time of the scoring pass per camera:
    python profiles/contrib_microbench.py [slab|heavy] [rounds] [reps]
One forward of camera 1 of the bench scene (fused.camera_forward, exact sizes, as profiles/raster_microbench.py), then
`rounds` interleaved rounds in ONE process of `reps` back-to-back launches of clmgs_rasterize_fwd and of
clmgs_rasterize_contrib (its record pack included; the pack alone is timed too) on the camera's own lists, event-timed on
the launch stream; median and minimum over the rounds.  Then contribution.score_cameras over four cameras, wall time.
The forward kernel is, instruction for instruction, the one of the commit before contrib.hip existed."""
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from clm_gs_amd import _lib, contribution, fused, utils  # noqa: E402
from clm_gs_amd import gsplat as G  # noqa: E402
from clm_gs_amd._lib import check, dptr  # noqa: E402
from clm_gs_amd.strategies.base_engine import select_filters  # noqa: E402
from clm_gs_amd.strategies.clm_offload import GaussianModelCLMOffload  # noqa: E402
from clm_gs_amd.synthetic import nadir_cameras, synth_gaussians  # noqa: E402

kind = sys.argv[1] if len(sys.argv) > 1 else "slab"
rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 5
reps = int(sys.argv[3]) if len(sys.argv) > 3 else 10
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
cams = nadir_cameras(4, N, W, H, 0.10, seed=0, device="cuda")
cam = cams[1]
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
rec = p.packed.reshape(V, 16)
m2, op, cn = rec[:, 0:2].contiguous(), rec[:, 2].contiguous(), rec[:, 3:6].contiguous()
raw = G.contribution_arrays(V, "cuda")
cpk = torch.empty(L.clmgs_rasterize_contrib_pack_bytes(1, V), dtype=torch.uint8, device="cuda")
out, al, last = torch.empty_like(p.out), torch.empty_like(p.alphas), torch.empty_like(p.last_ids)


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def fwd():
    check(L.clmgs_rasterize_fwd(st, 1, V, I, None, None, None, None, None, W, H, 16, tw, th, dptr(p.offsets), dptr(p.fids),
                                dptr(p.packed), dptr(out), dptr(al), dptr(last)))


def contrib():
    check(L.clmgs_rasterize_contrib(st, 1, V, I, dptr(m2), dptr(cn), dptr(op), W, H, 16, tw, th, dptr(p.offsets), dptr(p.fids),
                                    None, V, dptr(cpk), dptr(raw[0]), dptr(raw[1]), dptr(raw[2])))


def pack_only():  # one listed entry in an otherwise empty image: the pack pass and a tile kernel with nothing to walk
    check(L.clmgs_rasterize_contrib(st, 1, V, 1, dptr(m2), dptr(cn), dptr(op), W, H, 16, tw, th, dptr(zero_off), dptr(p.fids),
                                    None, V, dptr(cpk), dptr(scratch[0]), dptr(scratch[1]), dptr(scratch[2])))


zero_off = torch.ones_like(p.offsets)
zero_off.view(-1)[0] = 0
scratch = G.contribution_arrays(V, "cuda")
for fn in (fwd, contrib, pack_only):
    fn()
torch.cuda.synchronize()
t = {"fwd": [], "contrib": [], "pack": []}
for _ in range(rounds):
    t["fwd"].append(timed(fwd))
    t["contrib"].append(timed(contrib))
    t["pack"].append(timed(pack_only))
n_launch = 1 + rounds * reps
wsum = raw[0].double().sum().item() * G.WSUM_UNIT / n_launch
alpha_sum = al.double().sum().item()
for c in cams:
    c.original_image = cam.original_image
contribution.score_cameras(m, cams[:1])  # warm
torch.cuda.synchronize()
t0 = time.perf_counter()
stats = contribution.score_cameras(m, cams)
torch.cuda.synchronize()
score_s = time.perf_counter() - t0
med = {k: statistics.median(v) for k, v in t.items()}
print(json.dumps({"lib": os.path.basename(_lib.LIB_PATH), "scene": kind, "V": V, "I_emitted": I, "rounds": rounds, "reps": reps,
                  "rasterize_fwd_ms": {"median": round(med["fwd"], 4), "min": round(min(t["fwd"]), 4)},
                  "rasterize_contrib_ms": {"median": round(med["contrib"], 4), "min": round(min(t["contrib"]), 4)},
                  "contrib_pack_and_empty_walk_ms": {"median": round(med["pack"], 4), "min": round(min(t["pack"]), 4)},
                  "contrib_over_fwd": round(med["contrib"] / med["fwd"], 3),
                  "wsum_per_launch": wsum, "forward_alpha_sum": alpha_sum, "rel": abs(wsum - alpha_sum) / alpha_sum,
                  "score_cameras_s_per_camera": round(score_s / len(cams), 4), "score_cameras_cameras": len(cams),
                  "rows": N, "rows_with_pixels": int((stats.pixels > 0).sum())}))
