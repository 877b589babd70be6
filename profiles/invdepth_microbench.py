"""Depth regularisation: the three kernels of csrc/invdepth.hip and the 4-channel slot route against their yardsticks, on
one camera of the bench scene (28 M slab, 4608x3456; the scene and camera of profiles/raster4_microbench.py):
    python profiles/invdepth_microbench.py [slab|heavy] [reps] [rounds]
One forward of camera 1 through the fused path (exact sizes) gives the camera's lists, records, depths and loss cotangent.
Legs, alternated within a round so that all see the same box and clocks, `rounds` rounds of `reps` launches, event-timed;
the median round per leg:
  pack       clmgs_invdepth_pack over the camera's V records         | copy moving 12 B per row (radii 4 + depths 4 + word 4)
  loss       clmgs_invdepth_l1_fwd_bwd, channel 3 of [H,W,4] buffers  | copy moving 10 B per pixel (I 4 + prior 2 + v_I 4)
  loss_mask  the same with a uint8 mask                               | copy moving 11 B per pixel
  loss_planar  planar I and v_I (the generic path, for the record)
  fwd3_dev / fwd4_dev    clmgs_rasterize_fwd_dev / clmgs_rasterize4_fwd_dev, capacity = count
  bwd3_slot / bwd4_slot  clmgs_rasterize_bwd / clmgs_rasterize4_slot_bwd, partial lines out (no per-row sum)
  rows       clmgs_invdepth_rows_bwd on the [V,12] table from the 4-channel partial lines
             | copy moving 4 + 4 + 8 + 24 B per row + 4 B per line (radii, depths, row_cum, xyz read + written, word 9)
A copy "moving n bytes" copies n / 2 bytes (read + written).  The kernels touch more than the bytes they need: a pixel's
or record's word sits in a 16 B pixel / 64 B line that the memory system moves whole."""
import ctypes
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
g = torch.Generator().manual_seed(1)
cam.original_image = (torch.rand(3, H, W, generator=g) * 255).to(torch.uint8).cuda()
p = fused.camera_forward(m, cam, filters[0], m._parameters.data, 1, None, cam.original_image)
torch.cuda.synchronize()
L = _lib.lib()
V, I = p.V, p.fids.numel()
tw, th = (W + 15) // 16, (H + 15) // 16
st = _lib.stream()
vm = p.cam[0]
radii = p.radii.reshape(-1)
depths = p.aux[[t is p.means2d for t in p.aux].index(True) + 1].reshape(-1)  # (means2d, depths) of the front end
packed4 = p.packed.clone()
check(L.clmgs_invdepth_pack(st, V, dptr(radii), dptr(depths), dptr(packed4)))
n_dev = torch.tensor([I, I], dtype=torch.int64, device="cuda")
out3, out4 = torch.empty((H, W, 3), device="cuda"), torch.empty((H, W, 4), device="cuda")
al, last = torch.empty_like(p.alphas), torch.empty_like(p.last_ids)
check(L.clmgs_rasterize4_fwd_dev(st, 1, V, I, dptr(n_dev), None, W, H, 16, tw, th, dptr(p.offsets), dptr(p.fids),
                                 dptr(packed4), dptr(out4), dptr(al), dptr(last)))
torch.cuda.synchronize()
assert torch.equal(out4[..., :3], p.out) and torch.equal(last, p.last_ids) and torch.equal(al, p.alphas)
# a prior a little off the render, as the depth maps of a scene in training are
g = torch.Generator(device="cuda").manual_seed(2)
imax = float(out4[..., 3].max())
scale, offset = 1.1 * imax, -0.05 * imax
noise = 0.02 * imax * torch.randn((H, W), device="cuda", generator=g)
raw = ((out4[..., 3] + noise - offset) / scale * 65536).round().clamp(0, 65535).to(torch.int32).to(torch.uint16)
mask = (torch.rand((H, W), device="cuda", generator=g) < 0.8).to(torch.uint8)
v4 = torch.zeros((H, W, 4), device="cuda")
v4[..., :3] = p.v_out
rows_l = int(L.clmgs_invdepth_partials_rows(H, W))
part_l = torch.empty((rows_l,), device="cuda")
ch3 = 12


def loss(mk=None):
    check(L.clmgs_invdepth_l1_fwd_bwd(st, H, W, ctypes.c_void_p(out4.data_ptr() + ch3), 4 * W, 4, dptr(raw), scale, offset,
                                      dptr(mk, None, True), 1.0, ctypes.c_void_p(v4.data_ptr() + ch3), 4 * W, 4, dptr(part_l)))


I_pl, v_pl = out4[..., 3].contiguous(), torch.empty((H, W), device="cuda")
loss()
torch.cuda.synchronize()
parts3 = torch.empty((I, 16), device="cuda")
parts4 = torch.empty((I, 16), device="cuda")
table = torch.zeros((V, 12), device="cuda")
vmp = vm.ctypes.data_as(ctypes.c_void_p)


def copy_moving(nbytes):
    n = max(int(nbytes) // 8, 1)  # float32 elements of a buffer of nbytes / 2
    a, b = torch.empty((n,), device="cuda"), torch.empty((n,), device="cuda")
    return lambda: b.copy_(a)


bytes_pack, bytes_loss, bytes_mask = 12 * V, 10 * H * W, 11 * H * W
bytes_rows = (4 + 4 + 8 + 24) * V + 4 * I
slot_args = (W, H, 16, tw, th, dptr(p.offsets), dptr(p.fids), dptr(p.alphas), dptr(p.last_ids))
legs = {
    "pack": lambda: check(L.clmgs_invdepth_pack(st, V, dptr(radii), dptr(depths), dptr(packed4))),
    "pack_copy": copy_moving(bytes_pack),
    "loss": loss,
    "loss_copy": copy_moving(bytes_loss),
    "loss_mask": lambda: loss(mask),
    "loss_mask_copy": copy_moving(bytes_mask),
    "loss_planar": lambda: check(L.clmgs_invdepth_l1_fwd_bwd(st, H, W, dptr(I_pl), W, 1, dptr(raw), scale, offset, None, 1.0,
                                                             dptr(v_pl), W, 1, dptr(part_l))),
    "fwd3_dev": lambda: check(L.clmgs_rasterize_fwd_dev(st, 1, V, I, dptr(n_dev), None, W, H, 16, tw, th, dptr(p.offsets),
                                                        dptr(p.fids), dptr(p.packed), dptr(out3), dptr(al), dptr(last))),
    "fwd4_dev": lambda: check(L.clmgs_rasterize4_fwd_dev(st, 1, V, I, dptr(n_dev), None, W, H, 16, tw, th, dptr(p.offsets),
                                                         dptr(p.fids), dptr(packed4), dptr(out4), dptr(al), dptr(last))),
    "bwd3_slot": lambda: check(L.clmgs_rasterize_bwd(st, 1, V, I, dptr(p.packed), None, *slot_args, dptr(p.v_out), None, None,
                                                     None, None, None, None, dptr(p.emit_slot), dptr(p.row_cum),
                                                     dptr(parts3))),
    "bwd4_slot": lambda: check(L.clmgs_rasterize4_slot_bwd(st, 1, V, I, dptr(packed4), None, *slot_args, dptr(v4), None, None,
                                                           None, None, None, None, dptr(p.emit_slot), dptr(p.row_cum),
                                                           dptr(parts4))),
    "rows": lambda: check(L.clmgs_invdepth_rows_bwd(st, V, None, dptr(radii), dptr(depths), vmp, dptr(parts4),
                                                    dptr(p.row_cum), None, dptr(table), 1)),
    "rows_copy": copy_moving(bytes_rows),
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
med = {k: statistics.median(v) for k, v in times.items()}
res = {"lib": os.path.basename(_lib.LIB_PATH), "scene": kind, "size": [W, H], "V": V, "I_emitted": I, "reps": reps,
       "rounds": rounds, "ms": {k: round(v, 4) for k, v in med.items()},
       "spread_ms": {k: [round(min(v), 4), round(max(v), 4)] for k, v in times.items()},
       "bytes": {"pack": bytes_pack, "loss": bytes_loss, "loss_mask": bytes_mask, "rows": bytes_rows},
       "pack_over_copy": round(med["pack"] / med["pack_copy"], 3),
       "loss_over_copy": round(med["loss"] / med["loss_copy"], 3),
       "loss_mask_over_copy": round(med["loss_mask"] / med["loss_mask_copy"], 3),
       "rows_over_copy": round(med["rows"] / med["rows_copy"], 3),
       "fwd_dev_ratio_4_over_3": round(med["fwd4_dev"] / med["fwd3_dev"], 4),
       "bwd_slot_ratio_4_over_3": round(med["bwd4_slot"] / med["bwd3_slot"], 4),
       "lines_per_row": round(I / max(V, 1), 3), "inverse_depth_max": imax,
       "v_I_abs_sum": float(v4[..., 3].double().abs().sum()), "g_d_abs_sum": float(parts4[:, 9].double().abs().sum()),
       "xyz_table_abs_sum": float(table[:, :3].double().abs().sum())}
print(json.dumps(res))
