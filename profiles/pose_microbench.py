"""Camera pose gradient: clmgs_pose_grad + clmgs_pose_grad_finish next to clmgs_preprocess_bwd, on one camera of the bench
scene (28 M slab, 4608x3456; the scene and camera of profiles/invdepth_microbench.py), degree 3, packed rows, partial
lines:
    python profiles/pose_microbench.py [slab|heavy] [reps] [rounds]
One forward + tile backward of camera 1 through the fused path (exact sizes) gives the camera's rows, radii and partial
lines.  Legs, alternated within a round so that all see the same box and clocks, `rounds` rounds of `reps` launches,
event-timed; the median round per leg:
  pre_bwd    clmgs_preprocess_bwd: packed rows in, packed gradient rows and the [N,48] SH gradient rows read + written
             (no statistics, no stamps), the partial lines summed per row
  pose       clmgs_pose_grad + clmgs_pose_grad_finish: the same reads, 16 floats per workgroup out
  pose_deg0  the same at degree 0 (no SH rows)
  copy       a device copy moving the pose kernel's bytes (below), read + written halves
Bytes of the pose kernel per row: filter 8 + radius 4 + row_cum 8 + packed row 48 + SH row 192 (visible rows only) and
64 per partial line; it writes 64 B per workgroup."""
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from clm_gs_amd import _lib, fused, utils  # noqa: E402
from clm_gs_amd._lib import check, dptr  # noqa: E402
from clm_gs_amd.gsplat import empty_bucketed  # noqa: E402
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
pk = m.small_packed()
p = fused.camera_forward(m, cam, filters[0], m._parameters.data, 1, None, cam.original_image, small_packed=pk)
torch.cuda.synchronize()
L = _lib.lib()
V, I = p.V, p.fids.numel()
tw, th = (W + 15) // 16, (H + 15) // 16
st = _lib.stream()
vm, K, campos = p.cam
np_ = fused._np
partials = empty_bucketed(max(I, 1), (16,), torch.float32, "cuda")
check(L.clmgs_rasterize_bwd(st, 1, V, I, dptr(p.packed), None, W, H, 16, tw, th, dptr(p.offsets), dptr(p.fids),
                            dptr(p.alphas), dptr(p.last_ids), dptr(p.v_out), None, None, None, None, None, None,
                            dptr(p.emit_slot), dptr(p.row_cum), dptr(partials)))
torch.cuda.synchronize()
gk = torch.zeros((N, 12), device="cuda")
gsh = torch.zeros((N, 48), device="cuda")
rows = int(L.clmgs_pose_grad_partials_rows(V))
pose_rows = torch.empty((rows, 16), device="cuda")
grad15 = torch.zeros(16, device="cuda")
n_vis = int((p.radii.reshape(-1) > 0).sum())
pose_bytes = V * (8 + 4 + 8) + n_vis * (48 + 192) + I * 64 + rows * 64
copy_src = torch.empty(pose_bytes // 8, dtype=torch.float32, device="cuda")
copy_dst = torch.empty_like(copy_src)


def pre_bwd():
    check(L.clmgs_preprocess_bwd(st, V, dptr(p.filt, torch.int64, True), *p.small_in, dptr(p.sh_rows), 1, np_(vm), np_(K),
                                 np_(campos), W, H, 3, 0.3, dptr(p.radii), None, dptr(gk), None, None, None, dptr(gsh),
                                 None, None, None, None, 0, dptr(partials), dptr(p.row_cum), None, None, 0))


def pose(deg=3):
    check(L.clmgs_pose_grad(st, V, dptr(p.filt, torch.int64, True), *p.small_in, dptr(p.sh_rows), 1, np_(vm), np_(K),
                            np_(campos), W, H, deg, 0.3, dptr(p.radii), None, dptr(partials), dptr(p.row_cum), None, 0,
                            dptr(pose_rows)))
    check(L.clmgs_pose_grad_finish(st, rows, dptr(pose_rows), dptr(grad15)))


legs = {"pre_bwd": pre_bwd, "pose": pose, "pose_deg0": lambda: pose(0), "copy": lambda: copy_dst.copy_(copy_src)}
for f in legs.values():
    f()
torch.cuda.synchronize()
a = grad15.clone()
grad15.zero_(); pose(); torch.cuda.synchronize()
b = grad15.clone()
grad15.zero_(); pose(); torch.cuda.synchronize()
assert torch.equal(b, grad15) and bool(torch.isfinite(a).all()), "two launches, the same bits"
times = {k: [] for k in legs}
for _ in range(rounds):
    for name, f in legs.items():
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        for _ in range(reps):
            f()
        e.record()
        torch.cuda.synchronize()
        times[name].append(s.elapsed_time(e) / reps)
med = {k: statistics.median(v) for k, v in times.items()}
out = dict(scene=kind, N=N, V=V, visible=n_vis, intersections=I, pose_partial_rows=rows, pose_bytes=pose_bytes,
           ms={k: round(v, 4) for k, v in med.items()}, ms_rounds={k: [round(x, 4) for x in v] for k, v in times.items()},
           pose_over_pre_bwd=round(med["pose"] / med["pre_bwd"], 3),
           pose_GBps=round(pose_bytes / med["pose"] / 1e6, 1), copy_GBps=round(pose_bytes / med["copy"] / 1e6, 1),
           pose_fraction_of_copy_bound=round(med["copy"] / med["pose"], 3), grad15=b[:15].tolist())
print(json.dumps(out))
