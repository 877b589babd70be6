"""The median-depth pass (csrc/median.hip) against the shipped forward tile kernels on the same lists:
    python profiles/median_microbench.py [slab|heavy] [rounds] [reps]
One forward of camera 1 of the bench scene (fused.camera_forward, exact sizes, as profiles/contrib_microbench.py), then
`rounds` interleaved rounds in ONE process of `reps` back-to-back launches of
    clmgs_rasterize_fwd                      the 3-channel forward              ("RGB", and the first half of "RGB+MD")
    clmgs_rasterize4_fwd                     the 4-channel forward              ("RGB+ED": the depth as fourth colour)
    clmgs_rasterize_median, nothing to walk  its record pack alone (one listed entry in an otherwise empty image)
    clmgs_rasterize_median                   the median pass with its pack      (the second half of "RGB+MD")
on the camera's own lists, event-timed on the launch stream; median and minimum over the rounds after a warm-up.  The
quantity of interest is RGB+MD (3-channel forward + median pass) against RGB+ED (4-channel forward).  Also counted, on the
device from the pass's own ids: the share of list entries at or before the deepest median entry of their tile (the whole
list of a tile in which a pixel stays above one half) -- the prefix the pass cannot avoid walking.
The two forward kernels are, instruction for instruction, those of the commit before median.hip existed."""
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
rec = p.packed.reshape(V, 16)
m2, op, cn = rec[:, 0:2].contiguous(), rec[:, 2].contiguous(), rec[:, 3:6].contiguous()
# the projection's camera-space depths of the V visible rows: kept alive next to the means2d in p.aux
depths = p.aux[next(i for i, x in enumerate(p.aux) if x is p.means2d) + 1]
assert depths.shape == (1, V) and depths.dtype == torch.float32
depths = depths.reshape(-1).contiguous()
rec4 = rec.clone()
rec4[:, 9] = depths  # the fourth colour's word of the 64 B record (raster_tile.h)
mpk = torch.empty(L.clmgs_rasterize_median_pack_bytes(1, V), dtype=torch.uint8, device="cuda")
out, al, last = torch.empty_like(p.out), torch.empty_like(p.alphas), torch.empty_like(p.last_ids)
out4 = torch.empty((1, H, W, 4), dtype=torch.float32, device="cuda")
md, mi = torch.empty((1, H, W), dtype=torch.float32, device="cuda"), torch.empty((1, H, W), dtype=torch.int32, device="cuda")
md0, mi0 = torch.empty_like(md), torch.empty_like(mi)
one_entry = torch.ones_like(p.offsets)  # every tile's list starts at 1 = the end, but the first tile's, which holds entry 0
one_entry.view(-1)[0] = 0


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def fwd3():
    check(L.clmgs_rasterize_fwd(st, 1, V, I, None, None, None, None, None, W, H, 16, tw, th, dptr(p.offsets), dptr(p.fids),
                                dptr(p.packed), dptr(out), dptr(al), dptr(last)))


def fwd4():
    check(L.clmgs_rasterize4_fwd(st, 1, V, I, None, None, None, None, None, W, H, 16, tw, th, dptr(p.offsets), dptr(p.fids),
                                 dptr(rec4), dptr(out4), dptr(al), dptr(last)))


def median():
    check(L.clmgs_rasterize_median(st, 1, V, I, dptr(m2), dptr(cn), dptr(op), dptr(depths), W, H, 16, tw, th,
                                   dptr(p.offsets), dptr(p.fids), dptr(mpk), dptr(md), dptr(mi)))


def pack_only():  # the pack pass and a tile kernel with nothing to walk (it still writes every pixel)
    check(L.clmgs_rasterize_median(st, 1, V, 1, dptr(m2), dptr(cn), dptr(op), dptr(depths), W, H, 16, tw, th,
                                   dptr(one_entry), dptr(p.fids), dptr(mpk), dptr(md0), dptr(mi0)))


legs = {"fwd3": fwd3, "fwd4": fwd4, "pack": pack_only, "median": median}
for fn in legs.values():  # warm-up
    fn()
torch.cuda.synchronize()
t = {k: [] for k in legs}
for _ in range(rounds):
    for k, fn in legs.items():
        t[k].append(timed(fn))
med = {k: statistics.median(v) for k, v in t.items()}

# sanity: the 4-channel forward's expected depth and the median depth on the opaque pixels
alpha = al.reshape(H, W)
opaque = alpha >= 0.5
ed = out4[0, ..., 3] / alpha.clamp(min=1e-10)
listed = int((mi[0] >= 0).sum())
# the prefix of each list that holds a median entry: position of every pixel's id in its tile's list, on the device
share = None
try:
    offs = p.offsets.reshape(-1).long()
    ends = torch.cat([offs[1:], torch.tensor([I], device=offs.device)])
    lens = ends - offs
    tile_of_entry = torch.repeat_interleave(torch.arange(offs.numel(), device=offs.device), lens)
    keys, perm = torch.sort(tile_of_entry * V + p.fids.long())
    ys, xs = torch.meshgrid(torch.arange(H, device=offs.device), torch.arange(W, device=offs.device), indexing="ij")
    tile_of_pixel = (ys // 16) * tw + xs // 16
    has = mi[0] >= 0
    q = tile_of_pixel[has] * V + mi[0][has].long()
    at = torch.searchsorted(keys, q).clamp(max=I - 1)
    assert bool((keys[at] == q).all()), "a median id is not in its tile's list"
    pos = perm[at] - offs[tile_of_pixel[has]]
    deepest = torch.zeros(offs.numel(), dtype=torch.long, device=offs.device)
    deepest.scatter_reduce_(0, tile_of_pixel[has], pos + 1, reduce="amax")
    still_open = torch.zeros(offs.numel(), dtype=torch.bool, device=offs.device)
    still_open[tile_of_pixel[~opaque]] = True
    share = float(torch.where(still_open, lens, deepest).sum()) / I
except Exception as e:  # the timings stand without it
    share = f"not counted: {e}"
print(json.dumps({
    "lib": os.path.basename(_lib.LIB_PATH), "scene": kind, "V": V, "I_emitted": I, "rounds": rounds, "reps": reps,
    "rasterize_fwd_ms": {"median": round(med["fwd3"], 4), "min": round(min(t["fwd3"]), 4)},
    "rasterize4_fwd_ms": {"median": round(med["fwd4"], 4), "min": round(min(t["fwd4"]), 4)},
    "median_pack_and_empty_walk_ms": {"median": round(med["pack"], 4), "min": round(min(t["pack"]), 4)},
    "rasterize_median_ms": {"median": round(med["median"], 4), "min": round(min(t["median"]), 4)},
    "median_over_fwd3": round(med["median"] / med["fwd3"], 3),
    "rgb_md_ms": round(med["fwd3"] + med["median"], 4), "rgb_ed_ms": round(med["fwd4"], 4),
    "rgb_md_over_rgb_ed": round((med["fwd3"] + med["median"]) / med["fwd4"], 3),
    "pixels_with_an_entry": listed, "pixels_alpha_ge_half": int(opaque.sum()), "pixels": W * H,
    "mean_expected_minus_median_depth_on_opaque": float((ed - md[0])[opaque].double().mean()),
    "mean_abs_expected_minus_median_depth_on_opaque": float((ed - md[0])[opaque].double().abs().mean()),
    "share_of_list_entries_up_to_the_median": share}))
