"""The ray-depth pass (csrc/ray_depth.hip) against a device copy of the bytes it moves, and "RGB+RD" against "RGB+MD":
    python profiles/ray_depth_microbench.py [slab|heavy] [rounds] [reps] [rows]
Camera 1 of the 28 M bench scene at 4608x3456 (as profiles/median_microbench.py).  The camera's visible rows go once
through the operators camera_forward_ops runs (projection, binning, rasterize_median_depth), which leaves the median ids
and depths; then `rounds` interleaved rounds in ONE process of `reps` back-to-back runs of
    clmgs_ray_depth                          the pass alone, its camera table made beforehand
    a device-to-device copy of 12 B / pixel  the bytes the pass must move (ids and centre depths in, ray depths out; the
                                             touched rows come on top)
    "RGB+MD" through clm_offload_eval_one_cam
    "RGB+RD" through clm_offload_eval_one_cam
event-timed on the launch stream; median and minimum over the rounds after a warm-up.  A report, not a gate."""
import json
import math
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from clm_gs_amd import _lib, gsplat as G, utils  # noqa: E402
from clm_gs_amd._lib import check, dptr  # noqa: E402
from clm_gs_amd.strategies.base_engine import calculate_filters, fov_camera  # noqa: E402
from clm_gs_amd.strategies.clm_offload import GaussianModelCLMOffload, clm_offload_eval_one_cam  # noqa: E402
from clm_gs_amd.synthetic import nadir_cameras, synth_gaussians  # noqa: E402

kind = sys.argv[1] if len(sys.argv) > 1 else "slab"
rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 5
reps = int(sys.argv[3]) if len(sys.argv) > 3 else 5
N, W, H = (int(sys.argv[4]) if len(sys.argv) > 4 else 28_000_000), 4608, 3456
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
del sc
cam = nadir_cameras(4, N, W, H, 0.10, seed=0, device="cuda")[1]


class Scene:
    cameras_extent = 1.0


with torch.no_grad():
    filters, _, _ = calculate_filters([cam], m.get_xyz, m.get_opacity, m.get_scaling, m.get_rotation)
    f = filters[0]
    xyz = m._xyz.detach()[f].contiguous()
    sca = m.scaling_activation(m._scaling.detach()[f]).contiguous()
    rot = m.rotation_activation(m._rotation.detach()[f]).contiguous()
    opa = m.opacity_activation(m._opacity.detach()[f]).squeeze(1).unsqueeze(0)
    viewmat, K, _ = fov_camera(cam, xyz.device)
    radii, m2, depths, conics, _ = G.fully_fused_projection(xyz, None, rot, sca, viewmat[None], K[None], W, H,
                                                            radius_clip=args.radius_clip)
    tw, th = math.ceil(W / 16), math.ceil(H / 16)
    _, isect_ids, fids = G.isect_tiles(m2, radii, depths, 16, tw, th)
    off = G.isect_offset_encode(isect_ids, 1, tw, th)
    md, ids = G.rasterize_median_depth(m2, conics, opa, depths, W, H, 16, off, fids)
    del isect_ids, fids, off, m2, conics, radii
    cams = G.ray_camera_table(viewmat[None], K[None])
torch.cuda.synchronize()
L = _lib.lib()
st = _lib.stream()
V = int(xyz.shape[0])
rd = torch.empty((1, H, W), dtype=torch.float32, device="cuda")
src = torch.empty((H * W * 12 // 2,), dtype=torch.uint8, device="cuda")  # a copy reads and writes: 6 B each way per pixel
dst = torch.empty_like(src)


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def ray():
    check(L.clmgs_ray_depth(st, 1, V, H, W, dptr(xyz), dptr(rot), dptr(sca), dptr(cams), dptr(ids), dptr(md), 0.01, 0, dptr(rd)))


def copy():
    dst.copy_(src)


def rgb_md():
    clm_offload_eval_one_cam(cam, m, None, Scene, render_mode="RGB+MD", return_alpha=True)


def rgb_rd():
    clm_offload_eval_one_cam(cam, m, None, Scene, render_mode="RGB+RD", return_alpha=True)


legs = {"ray": ray, "copy": copy, "rgb_md": rgb_md, "rgb_rd": rgb_rd}
for fn in legs.values():  # warm-up
    fn()
torch.cuda.synchronize()
t = {k: [] for k in legs}
for _ in range(rounds):
    for k, fn in legs.items():
        t[k].append(timed(fn))
med = {k: statistics.median(v) for k, v in t.items()}

# sanity: the engine's map is the pass's map, and what the pass changes
_, depth_rd, alpha = clm_offload_eval_one_cam(cam, m, None, Scene, render_mode="RGB+RD", return_alpha=True)
torch.cuda.synchronize()
listed = ids[0] >= 0
touched = int(torch.unique(ids[0][listed]).numel())
diff = (rd[0] - md[0])[listed].double()
print(json.dumps({
    "lib": os.path.basename(_lib.LIB_PATH), "scene": kind, "rows": N, "V": V, "pixels": W * H, "rounds": rounds, "reps": reps,
    "ray_depth_ms": {"median": round(med["ray"], 4), "min": round(min(t["ray"]), 4)},
    "copy_12B_per_pixel_ms": {"median": round(med["copy"], 4), "min": round(min(t["copy"]), 4)},
    "ray_depth_over_copy": round(med["ray"] / med["copy"], 3),
    "ray_depth_GBps_of_12B_per_pixel": round(W * H * 12 / med["ray"] / 1e6, 1),
    "rgb_md_ms": {"median": round(med["rgb_md"], 4), "min": round(min(t["rgb_md"]), 4)},
    "rgb_rd_ms": {"median": round(med["rgb_rd"], 4), "min": round(min(t["rgb_rd"]), 4)},
    "rgb_rd_over_rgb_md": round(med["rgb_rd"] / med["rgb_md"], 3),
    "pixels_with_an_entry": int(listed.sum()), "rows_touched": touched, "row_bytes_touched": touched * 40,
    "engine_map_equals_the_pass": bool(torch.equal(depth_rd.view(torch.int32), rd.view(torch.int32))),
    "pixels_where_ray_differs_from_centre_depth": int((diff != 0).sum()),
    "mean_abs_ray_minus_centre_depth": float(diff.abs().mean()) if diff.numel() else None}))
