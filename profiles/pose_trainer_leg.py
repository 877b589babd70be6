"""Camera pose refinement in the training loop: ms per batch of four cameras at the bench scene (28 M slab, 4608x3456,
clm_offload, SH rows in HBM), without pose refinement, with the deferred step (default) and with the immediate step:
    python profiles/pose_trainer_leg.py [batches] [warmup]
One model, twelve cameras in a fixed cyclic order, the engine's own batch call and, in the pose modes, PoseModel.step
after it -- what trainer.training does per batch.  Wall time from the first timed batch's enqueue to the device being
idle after the last, divided by the number of batches; the three modes alternate, twice."""
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from clm_gs_amd import utils  # noqa: E402
from clm_gs_amd.pose import PoseModel  # noqa: E402
from clm_gs_amd.strategies.clm_offload import GaussianModelCLMOffload, clm_offload_train_one_batch  # noqa: E402
from clm_gs_amd.synthetic import LR_EXTENT, nadir_cameras, synth_gaussians  # noqa: E402

n_batches = int(sys.argv[1]) if len(sys.argv) > 1 else 12
warmup = int(sys.argv[2]) if len(sys.argv) > 2 else 3
N, W, H, BSZ, NCAM = 28_000_000, 4608, 3456, 4, 12
args = utils.default_args(bsz=BSZ, sh_residency="hbm", disable_auto_densification=True)
args.clm_offload = True
utils.set_args(args)
utils.set_img_size(H, W)
utils.set_cur_iter(1)
sc = synth_gaussians(N, seed=0, device="cuda")
order = utils.morton_order(sc["xyz"])
for k in ("xyz", "scaling", "rotation", "opacity", "shs48"):
    sc[k] = utils.gather_rows(sc[k], order)
m = GaussianModelCLMOffload(3)
m.create_from_tensors(sc["xyz"], sc["shs48"], sc["scaling"], sc["rotation"], sc["opacity"], spatial_lr_scale=LR_EXTENT)
m.active_sh_degree = 3
m.training_setup(args)
del sc
cams = nadir_cameras(NCAM, N, W, H, 0.10, seed=0, device="cuda")
g = torch.Generator().manual_seed(1)
for c in cams:
    c.original_image = (torch.rand(3, H, W, generator=g) * 255).to(torch.uint8).cuda()


class Scene:
    cameras_extent = LR_EXTENT


comm, gen = torch.cuda.Stream(), torch.Generator(device="cuda").manual_seed(1)
state = {"it": 1, "b": 0}


def run(pose, n):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        batch = [cams[(state["b"] * BSZ + j) % NCAM] for j in range(BSZ)]
        utils.set_cur_iter(state["it"])
        m.update_learning_rate(state["it"])
        clm_offload_train_one_batch(m, Scene, batch, m.parameters_grad_buffer, None, None, comm, gen)
        if pose is not None:
            pose.step(batch)
        state["it"] += BSZ
        state["b"] += 1
    if pose is not None:
        pose.flush()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / n


def set_mode(mode):
    if mode == "off":
        for c in cams:
            c.pose_grad = None
        return None
    pose = PoseModel(NCAM, lr=1e-7, max_steps=30000, defer=(mode == "deferred"))
    pose.attach(cams)
    return pose


run(None, warmup)
res = {"off": [], "deferred": [], "immediate": []}
for _ in range(2):
    for mode in res:
        pose = set_mode(mode)
        run(pose, 2)
        res[mode].append(round(run(pose, n_batches), 3))
set_mode("off")
print(json.dumps(dict(N=N, image=[W, H], bsz=BSZ, batches=n_batches, ms_per_batch=res,
                      best={k: min(v) for k, v in res.items()})))
