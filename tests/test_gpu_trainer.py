"""-m gpu: the trainer loop end to end on a small synthetic scene (scope row f1): LR schedule,
SH ramp, engine, densification (clone/split/prune + opacity reset), evaluation, and the exact log
strings release_scripts/log2csv.py:54-102 parses."""
import io
import os

import pytest
import torch

pytestmark = pytest.mark.gpu


def _parse_like_log2csv(text):
    """Same string surgery as release_scripts/log2csv.py:54-102 (restated, not imported)."""
    m = {}
    for line in reversed(text.splitlines()):
        if "total_time_s" not in m and "end2end total_time:" in line:
            m["total_time_s"] = float(line.split("end2end total_time: ")[1].split(" s")[0])
            m["iterations"] = int(line.split("iterations: ")[1].split(",")[0])
            m["throughput"] = float(line.split("throughput ")[1].split(" it/s")[0])
        if "test_psnr" not in m and "Evaluating test:" in line:
            m["test_psnr"] = float(line.split("PSNR ")[1].strip())
        if "train_psnr" not in m and "Evaluating train:" in line:
            m["train_psnr"] = float(line.split("PSNR ")[1].strip())
        if "num_3dgs" not in m and "Now num of 3dgs:" in line and "Max Memory usage:" in line and "Now Pinned Memory:" in line:
            m["num_3dgs"] = int(line.split("Now num of 3dgs: ")[1].split(".")[0])
            m["max_gpu_memory_gb"] = float(line.split("Max Memory usage: ")[1].split(" GB")[0])
            m["pinned_cpu_memory_gb"] = float(line.split("Now Pinned Memory: ")[1].split(" GB")[0])
    return m


@pytest.mark.parametrize("strategy,residency", [("clm_offload", "hbm"), ("no_offload", "hbm"), ("clm_offload", "host"),
                                                ("clm_offload", "host_budget"), ("naive_offload", "hbm")])
def test_training_loop_improves_psnr_and_logs(dev, strategy, residency):
    from clm_gs_amd import trainer, utils
    from clm_gs_amd.strategies.clm_offload import GaussianModelCLMOffload, clm_offload_eval_one_cam
    from clm_gs_amd.strategies.no_offload import GaussianModelNoOffload
    from clm_gs_amd.synthetic import nadir_cameras, synth_gaussians
    N, W, H, bsz = 20000, 160, 128, 4
    budget = {}
    if residency == "host_budget":  # host-resident rows, 12 000 of them kept and stepped in HBM (sh_hbm_budget_gb): the
        residency, budget = "host", {"sh_hbm_budget_gb": 12000 * 768 / 1e9 + 1e-9}  # evaluations write them back, the
    args = utils.default_args(bsz=bsz, sh_residency=residency, densify_from_iter=100, densification_interval=100,  # densifications reload them
                              densify_until_iter=300, densify_grad_threshold=0.00005, **budget)
    setattr(args, strategy, True)
    utils.set_args(args)
    utils.set_img_size(H, W)
    utils.set_cur_iter(1)
    truth = synth_gaussians(N, seed=7, device="cuda")
    cams = nadir_cameras(28, N, W, H, 0.3, seed=7, device="cuda")
    gt_model = GaussianModelCLMOffload(3, only_for_rendering=True)
    args_gt = utils.default_args(bsz=bsz, sh_residency="hbm")
    gt_model.args = args_gt
    gt_model.create_from_tensors(truth["xyz"], truth["shs48"], truth["scaling"], truth["rotation"], truth["opacity"])
    gt_model.active_sh_degree = 3
    for c in cams:
        c.original_image = (clm_offload_eval_one_cam(c, gt_model, None, None).clamp(0, 1) * 255).round().to(torch.uint8)
    g = torch.Generator(device="cuda").manual_seed(1)
    noisy_sh = truth["shs48"].clone()
    noisy_sh[:, :3] += torch.randn((N, 3), generator=g, device="cuda") * 0.6   # wrong base colours
    from clm_gs_amd.strategies.naive_offload import GaussianModelNaiveOffload
    model = {"clm_offload": GaussianModelCLMOffload, "no_offload": GaussianModelNoOffload,
             "naive_offload": GaussianModelNaiveOffload}[strategy](3)
    model.create_from_tensors(truth["xyz"] + torch.randn((N, 3), generator=g, device="cuda") * 0.05, noisy_sh,
                              truth["scaling"], truth["rotation"], truth["opacity"], spatial_lr_scale=truth["extent"])
    model.training_setup(args)
    model.split_generator = torch.Generator(device="cuda").manual_seed(5)

    class Scene:
        cameras_extent = truth["extent"]

    log = io.StringIO()
    train_cams, test_cams = cams[:24], cams[24:]
    timer = trainer.training(model, Scene, train_cams, test_cams, log, iterations=400,
                             test_iterations=(1, 397))
    text = log.getvalue()
    m = _parse_like_log2csv(text)
    for k in ("total_time_s", "iterations", "throughput", "test_psnr", "train_psnr", "num_3dgs",
              "max_gpu_memory_gb", "pinned_cpu_memory_gb"):
        assert k in m, (k, text[-800:])
    assert m["iterations"] == 401 and m["throughput"] > 1
    first_test = [l for l in text.splitlines() if "Evaluating test:" in l][0]
    p0 = float(first_test.split("PSNR ")[1])
    loss_lines = [l.split(" image:")[0] for l in text.splitlines() if " loss: " in l]
    assert m["test_psnr"] > p0 + 1.0, (p0, m["test_psnr"], loss_lines[:3], loss_lines[-3:])
    assert m["num_3dgs"] != N, "densification must have changed the model"
    assert "Number of split gaussians" in text and "Number of cloned gaussians" in text
    assert model.active_sh_degree == 0  # the first ramp step is at image 1000 (train.py:253-254)
    if residency == "host":
        assert m["pinned_cpu_memory_gb"] > 0
    if budget:
        assert model._hbm_prefix is not None and model._hbm_prefix["K"] == 12000 and not model._hbm_prefix["dirty"]


def _reloaded(name, model, path, cameras):
    """The table of a side model's file, read back through the model's own loader -> (table in the file, table in memory)."""
    from clm_gs_amd.bilagrid import BilagridModel
    from clm_gs_amd.exposure import ExposureModel
    from clm_gs_amd.pose import PoseModel
    from clm_gs_amd.sky import SkyModel
    if name == "exposure":
        fresh = ExposureModel(len(cameras), "cuda")
        fresh.load_json(str(path), cameras)
    elif name == "bilagrid":
        fresh = BilagridModel(len(cameras), "cuda")
        fresh.load(str(path), cameras)
    elif name == "sky":
        fresh = SkyModel.from_file(str(path.parent), "cuda")
    else:
        fresh = PoseModel(len(cameras), device=None)
        fresh.load_json(str(path), cameras)
        return fresh.table, model.table
    return fresh.param.detach(), model.param.detach()


@pytest.mark.parametrize("flags,names", [
    (dict(exposure=True, pose_opt=True, defer_pose_step=False), ("exposure", "pose")),
    (dict(bilagrid=True, sky=True, sky_shape=(8, 16)), ("bilagrid", "sky")),
], ids=["exposure+pose", "bilagrid+sky"])
def test_two_side_models_step_in_one_batch_and_are_saved(dev, tmp_path, flags, names):
    """8 images in two batches of 4 with two side models on: both are stepped through trainer.SIDE_MODELS, both files are
    written and hold what the scene holds."""
    from clm_gs_amd import trainer
    from clm_gs_amd.bilagrid import IDENTITY
    from tests.test_gpu_exposure import _tiny_scene
    work = _tiny_scene(tmp_path)
    out = tmp_path / "out"
    _, scene, _ = trainer.train_from_colmap(str(work), str(out), strategy="clm_offload", iterations=8, bsz=4,
                                            disable_auto_densification=True, **flags)
    rows = {r.name: r for r in trainer.SIDE_MODELS}
    for row in rows.values():
        assert (getattr(scene, row.name) is not None) == (row.name in names), row.name
        assert os.path.exists(out / row.file) == (row.name in names), row.file
    for name in names:
        model = getattr(scene, name)
        in_file, in_memory = _reloaded(name, model, out / rows[name].file, scene.train_cameras)
        assert torch.equal(in_file, in_memory), name
    initial = {"exposure": lambda m: torch.eye(3, 4, device="cuda").expand_as(m.param),
               "bilagrid": lambda m: torch.tensor(IDENTITY, device="cuda").expand_as(m.param),
               "sky": lambda m: torch.full_like(m.param, 0.5),
               "pose": lambda m: torch.zeros_like(m.table)}
    for name in names:
        model = getattr(scene, name)
        table = model.table if name == "pose" else model.param.detach()
        moved = float((table - initial[name](model)).abs().max())
        print(f"{name}: the table moved by at most {moved:.3e} in two batches")
        assert moved > 0.0, name
    log = open(out / "python_ws=1_rk=0.log").read().splitlines()
    assert [l.split(" loss: ")[0] for l in log if " loss: " in l] == ["iteration[1,5)", "iteration[5,9)"]
    assert log[-3].startswith("end2end total_time: ") and "iterations: 9," in log[-3]


def test_longer_pipelined_run_with_densification_is_stable(dev):
    """1200 images through the pipelined, synchronisation-free clm_offload engine with several
    densification rounds and one opacity reset (the model is resized while the previous batch's per-camera tensors are
    still alive): finite losses and parameters, PSNR keeps rising, the model grows."""
    import math
    from clm_gs_amd import trainer, utils
    from clm_gs_amd.strategies.clm_offload import GaussianModelCLMOffload, clm_offload_eval_one_cam
    from clm_gs_amd.synthetic import nadir_cameras, synth_gaussians
    N, W, H, bsz = 60000, 320, 192, 4
    args = utils.default_args(bsz=bsz, sh_residency="hbm", densify_from_iter=100, densification_interval=100,
                              densify_until_iter=900, densify_grad_threshold=0.00005, opacity_reset_interval=600)
    args.clm_offload = True
    utils.set_args(args)
    utils.set_img_size(H, W)
    utils.set_cur_iter(1)
    truth = synth_gaussians(N, seed=11, device="cuda")
    cams = nadir_cameras(44, N, W, H, 0.3, seed=11, device="cuda")
    gt_model = GaussianModelCLMOffload(3, only_for_rendering=True)
    gt_model.args = utils.default_args(bsz=bsz, sh_residency="hbm")
    gt_model.create_from_tensors(truth["xyz"], truth["shs48"], truth["scaling"], truth["rotation"], truth["opacity"])
    gt_model.active_sh_degree = 3
    for c in cams:
        c.original_image = (clm_offload_eval_one_cam(c, gt_model, None, None).clamp(0, 1) * 255).round().to(torch.uint8)
    g = torch.Generator(device="cuda").manual_seed(2)
    noisy_sh = truth["shs48"].clone()
    noisy_sh[:, :3] += torch.randn((N, 3), generator=g, device="cuda") * 0.6
    model = GaussianModelCLMOffload(3)
    model.create_from_tensors(truth["xyz"] + torch.randn((N, 3), generator=g, device="cuda") * 0.05, noisy_sh,
                              truth["scaling"], truth["rotation"], truth["opacity"], spatial_lr_scale=truth["extent"])
    model.training_setup(args)
    model.split_generator = torch.Generator(device="cuda").manual_seed(5)

    class Scene:
        cameras_extent = truth["extent"]

    log = io.StringIO()
    trainer.training(model, Scene, cams[:40], cams[40:], log, iterations=1200,
                     test_iterations=(1, 597, 617, 1197))
    text = log.getvalue()
    psnrs = [float(l.split("PSNR ")[1]) for l in text.splitlines() if "Evaluating test:" in l]
    # rises until the opacity reset at image 600 (every opacity back to <= 0.01: the render goes
    # dark), then recovers from the post-reset level
    assert len(psnrs) == 4 and all(math.isfinite(x) for x in psnrs), psnrs
    assert psnrs[1] > psnrs[0] + 1.0 and psnrs[2] < psnrs[1] and psnrs[3] > psnrs[2] + 1.0, psnrs
    losses = [float(x) for l in text.splitlines() if " loss: " in l for x in l.split(" loss: ")[1].split(" image:")[0].split()]
    assert len(losses) == 1200 and all(math.isfinite(x) for x in losses)
    sizes = [int(l.split("Now num of 3dgs: ")[1].split(".")[0]) for l in text.splitlines() if "densify_and_prune. Now num" in l]
    assert len(set(sizes)) >= 3, sizes
    model.flush_lazy_rows()
    for t in (model._xyz, model._opacity, model._scaling, model._rotation, model._parameters):
        assert bool(torch.isfinite(t).all())
