"""Resolution schedule end to end: `trainer.training` on a synthetic slab (8 M Gaussians, 24 cameras at 4608x3456, bsz 4,
240 images, no densification), a whole run at each level -- num_downscales = L with a resolution_schedule longer than the
run -- against num_downscales = 0, alternated (warm-up, 0, 1, 2, 0, 1, 2) in one process, a fresh model per run:
    python profiles/resample_trainer_leg.py [N] [images]
Prints one JSON line with the ms per batch of every run.  The ground truth is random bytes: the cost of a step does not
depend on its values."""
import io
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from clm_gs_amd import trainer, utils  # noqa: E402
from clm_gs_amd.strategies.clm_offload import GaussianModelCLMOffload  # noqa: E402
from clm_gs_amd.synthetic import nadir_cameras, synth_gaussians  # noqa: E402

N = int(sys.argv[1]) if len(sys.argv) > 1 else 8_000_000
n_img = int(sys.argv[2]) if len(sys.argv) > 2 else 240
W, H, BSZ, CAMS = 4608, 3456, 4, 24
cams = nadir_cameras(CAMS, N, W, H, 0.10, seed=0, device="cuda")
g0 = torch.Generator(device="cuda").manual_seed(1)
for c in cams:
    c.original_image = (torch.rand((3, H, W), device="cuda", generator=g0) * 255).to(torch.uint8)


class _Scene:
    cameras_extent = 30.0


def run(level):
    args = utils.default_args(bsz=BSZ, sh_residency="hbm", iterations=n_img, disable_auto_densification=True,
                              num_downscales=level, resolution_schedule=10 * n_img)
    args.clm_offload = True
    utils.set_args(args)
    utils.set_img_size(H, W)
    sc = synth_gaussians(N, seed=0, device="cuda", kind="slab")
    m = GaussianModelCLMOffload(3)
    m.create_from_tensors(sc["xyz"], sc["shs48"], sc["scaling"], sc["rotation"], sc["opacity"], spatial_lr_scale=30.0)
    del sc
    m.active_sh_degree = 3
    m.training_setup(args)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    trainer.training(m, _Scene, cams, [], io.StringIO(), iterations=n_img)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    del m
    torch.cuda.empty_cache()
    return round(dt * 1e3 / (n_img / BSZ), 3)


res = {"N": N, "size": [W, H], "bsz": BSZ, "images": n_img, "cameras": CAMS, "warmup_ms_per_batch": run(2)}
res["ms_per_batch"] = {f"level{l}_{k}": run(l) for k in (1, 2) for l in (0, 1, 2)}
print(json.dumps(res))
