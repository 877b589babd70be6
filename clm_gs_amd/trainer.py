"""Thin training loop around the engines (scope row f1; reference: train.py:68-666).

Keeps what the published numbers depend on: the image-strided iteration counter
(train.py:202-204), xyz LR schedule per image index, SH-degree ramp every 1000 images
(:253-254), the engine call (:316-432), gsplat_densification (:452), the no_offload optimizer
epilogue (:533-578), the end-to-end timer that pauses during evaluation (:438-447, utils/timer.py:
87-111), and the exact log strings release_scripts/log2csv.py:54-102 scrapes.  `training` takes cameras
as objects; `train_from_colmap` (and `python -m clm_gs_amd.trainer -s ... -m ...`) builds them from a COLMAP
directory (colmap_scene.py).  MatrixCity / Blender readers, checkpoint directories and the rest of the
reference's CLI are out of scope.
"""
import contextlib
import gc
import os
import random
import time
from collections import namedtuple

import torch

from . import dp, mcmc, utils
from .bilagrid import BilagridModel
from .cameras import LevelCameras, camera_loss_mask
from .clm_kernels import apply_camera_colour, check_undistort_zoom
from .contribution import check_contrib_prune_args, contribution_prune, prune_iterations
from .densification import check_mcmc_args, gsplat_densification, mcmc_refinement
from .exposure import ExposureModel
from .pose import PoseModel, check_pose_args
from .sky import SkyModel


class End2endTimer:
    """utils/timer.py:87-111: wall clock that can be paused; throughput = iterations / total."""

    def __init__(self):
        self.total_time = 0.0
        self.last_time_point = None

    def start(self):
        torch.cuda.synchronize()
        self.last_time_point = time.time()

    def stop(self):
        torch.cuda.synchronize()
        self.total_time += time.time() - self.last_time_point
        self.last_time_point = None

    def print_time(self, log_file, n_iterations):
        log_file.write("end2end total_time: {:.3f} s, iterations: {}, throughput {:.2f} it/s\n".format(
            self.total_time, n_iterations, n_iterations / max(self.total_time, 1e-9)))


def clm_hbm_only(args):
    return bool(getattr(args, "clm_offload", False)) and getattr(args, "sh_residency", "hbm") == "hbm"


def psnr(img1, img2):
    mse = ((img1 - img2) ** 2).reshape(img1.shape[0], -1).mean(1, keepdim=True)
    return 20 * torch.log10(1.0 / torch.sqrt(mse))


def _pinned_gb(gaussians):
    tot = 0
    names = ("parameters_buffer", "parameters_grad_buffer", "_exp_avg_buffer", "_exp_avg_sq_buffer")
    if hasattr(gaussians, "_small"):  # naive_offload: its own two pinned tables (+ grads are transient)
        names = ("_small", "_parameters")
    for name in names:
        t = getattr(gaussians, name, None)
        if isinstance(t, torch.Tensor) and t.numel() and not t.is_cuda:
            tot += t.numel() * t.element_size()
    return tot / 2 ** 30


def memory_line(iteration, bsz, gaussians, what="densify_and_prune"):
    """utils/general_utils.py:216-240 format (the part log2csv.py reads)."""
    return ("iteration[{},{}) {}. Now num of 3dgs: {}. Now Memory usage: {} GB. Max Memory usage: {} GB. "
            "Now Pinned Memory: {} GB\n").format(
        iteration, iteration + bsz, what, gaussians.get_xyz.shape[0],
        torch.cuda.memory_allocated() / 2 ** 30, torch.cuda.max_memory_allocated() / 2 ** 30,
        _pinned_gb(gaussians))


@torch.no_grad()
def evaluate(name, iteration, cameras, render_fn, log_file, max_images=10 ** 9):
    """train.py:669-846 in essence: mean L1 / PSNR over a camera set.  A camera with a loss mask is measured over its
    counted pixels only; one whose mask counts no pixel at all has nothing to measure and is left out of the means."""
    l1s, ps = [], []
    for cam in cameras[:max_images]:
        mask, count = camera_loss_mask(cam)
        if mask is not None and count == 0:
            continue
        img = torch.clamp(render_fn(cam), 0.0, 1.0)
        gt = torch.clamp(cam.original_image.float() / 255.0, 0.0, 1.0)
        if mask is None:
            l1s.append((img - gt).abs().mean().item())
            ps.append(psnr(img[None], gt[None]).mean().item())
        else:  # a reported metric: sums over the counted pixels, divided by their number (3 * count values)
            m = (mask != 0).to(img.dtype)[None]
            n = float(3 * count)
            l1s.append((((img - gt).abs() * m).sum() / n).item())
            mse = (((img - gt) ** 2) * m).sum() / n
            ps.append((20 * torch.log10(1.0 / torch.sqrt(mse))).item())
    l1, p = sum(l1s) / max(len(l1s), 1), sum(ps) / max(len(ps), 1)
    log_file.write("[ITER {}] Evaluating {}: L1 {} PSNR {}\n".format(iteration, name, l1, p))
    return l1, p


class _LossLog:
    """The `iteration[a,b) loss: ...` line of a batch needs the batch's loss VALUES on the host.  The reference reads
    them right after the batch (train.py: torch.stack(losses).cpu()), which drains the device before the next batch is
    enqueued; here the values travel on a side stream behind an event recorded after the batch, and the line is written
    when the NEXT batch has been enqueued (same text, same order): the host never waits for a device that has nothing
    queued behind it.  `defer_loss_log=False` in the args restores the immediate read."""

    def __init__(self, log_file, defer):
        self.log_file, self.defer, self.pending, self.stream = log_file, defer, None, None
        self.hosts, self.turn = {}, 0  # two pinned buffers per batch size, used alternately (no allocation per batch)

    def _write(self, head, host_vals, tail):
        self.log_file.write(head + " ".join("%.6f" % l for l in host_vals.tolist()) + tail)

    def push(self, head, losses, tail):
        if not self.defer:
            self._write(head, torch.stack(losses).cpu(), tail)
            return
        prev = self.pending
        if self.stream is None:
            self.stream = torch.cuda.Stream()
        stacked = torch.stack(losses)  # enqueued on the current stream, right behind the batch
        ev2 = torch.cuda.Event()
        ev2.record(torch.cuda.current_stream())
        self.turn ^= 1
        key = (tuple(stacked.shape), self.turn)
        host = self.hosts.get(key)
        if host is None:
            host = self.hosts[key] = torch.empty(stacked.shape, dtype=stacked.dtype, pin_memory=True)
        with torch.cuda.stream(self.stream):
            self.stream.wait_event(ev2)
            host.copy_(stacked, non_blocking=True)
            done = torch.cuda.Event()
            done.record(self.stream)
        stacked.record_stream(self.stream)
        self.pending = (head, host, tail, done)
        if prev is not None:
            self._flush(prev)

    def _flush(self, item):
        head, host, tail, done = item
        done.synchronize()
        self._write(head, host, tail)

    def flush(self):
        if self.pending is not None:
            self._flush(self.pending)
            self.pending = None


def _warm_structural_ops(device, n=70_000):
    """The torch operators of a densification (masks, selections, concatenations, the split's sampling, the Z-order
    keys) run ONCE on small tensors.  ROCm loads device code lazily, at the first launch out of each code object: the
    first densify_and_prune of a process paid 110-130 ms for that on top of its 30 ms of work (bench.py --trainer-trace),
    inside the end-to-end clock.  SETUP, like the allocator reservation below; private generator (the global random
    stream and the model's split generator are not touched), nothing of the model is read or written."""
    from .utils import build_rotation, inverse_sigmoid, morton_order, select_rows, take_rows
    with torch.no_grad():
        gen = torch.Generator(device=device)
        gen.manual_seed(0)
        acc = torch.rand((n, 1), device=device, generator=gen)
        den = (torch.rand((n, 1), device=device, generator=gen) > 0.3).float()
        mr = torch.zeros((n,), device=device)
        d4 = torch.rand((n, 4), device=device, generator=gen)
        mr = torch.maximum(mr, d4[:, 0]); acc = acc + d4[:, 1:2]; den = den + d4[:, 2:3]; d4.zero_()
        grads = acc / den
        grads[grads.isnan()] = 0.0
        xyz = torch.randn((n, 3), device=device, generator=gen)
        scal = torch.randn((n, 3), device=device, generator=gen) - 3.0
        rot = torch.randn((n, 4), device=device, generator=gen)
        opa = torch.randn((n, 1), device=device, generator=gen)
        shs = torch.rand((n, 48), device=device, generator=gen)
        sel = torch.norm(grads, dim=-1) >= 0.5
        sel &= torch.max(torch.exp(scal), dim=1).values <= 0.06
        k = int(sel.sum())
        new = [select_rows(t, sel) for t in (xyz, shs, opa, scal, rot)]
        cat = [torch.cat((t, e), dim=0) for t, e in zip((xyz, shs, opa, scal, rot), new)]
        mom = torch.cat((torch.zeros_like(xyz), torch.zeros_like(new[0])), dim=0)
        padded = torch.zeros((n + k,), device=device)
        padded[:n] = grads.squeeze()
        sel2 = padded >= 0.5
        sel2 &= torch.max(torch.exp(cat[3]), dim=1).values > 0.06
        stds = select_rows(torch.exp(cat[3]), sel2).repeat(2, 1)
        samples = torch.normal(mean=torch.zeros_like(stds), std=stds, generator=gen)
        rots = build_rotation(select_rows(cat[4], sel2)).repeat(2, 1, 1)
        new_xyz = torch.bmm(rots, samples.unsqueeze(-1)).squeeze(-1) + select_rows(cat[0], sel2).repeat(2, 1)
        new_scal = torch.log(select_rows(torch.exp(cat[3]), sel2).repeat(2, 1) / 1.6)
        prune = torch.cat((sel2, torch.zeros(2 * int(sel2.sum()), device=device, dtype=torch.bool)))
        xyz2 = torch.cat((cat[0], new_xyz), dim=0)
        opa2 = torch.cat((cat[2], select_rows(cat[2], sel2).repeat(2, 1)), dim=0)
        scal2 = torch.cat((cat[3], new_scal), dim=0)
        mask = (torch.sigmoid(opa2) < 0.005).squeeze()
        mask = torch.logical_or(mask, torch.exp(scal2).max(dim=1).values > 0.1)
        mask = torch.logical_or(mask, prune)
        keep = ~mask
        m = int(keep.sum())
        idx = torch.nonzero(keep).flatten()
        idx = take_rows(idx, morton_order(take_rows(xyz2, idx)))
        stamps = torch.zeros((xyz2.shape[0],), dtype=torch.int32, device=device)
        stamps[:m] = 7
        new_opa = inverse_sigmoid(torch.min(torch.sigmoid(opa2), torch.ones_like(opa2) * 0.01))
        _ = (torch.zeros_like(new_opa), mom, mr, idx, stamps)
    torch.cuda.synchronize()


def no_offload_optimizer_step(gaussians, args, bsz, visibility=None):
    """The no_offload optimizer epilogue of a batch (train.py:533-578): gradients / bsz, step, zero_grad.  In MCMC mode
    the two regulariser gradients are added before the step and the position noise is injected after it."""
    use_mcmc = mcmc.enabled(args)
    if args.lr_scale_mode != "accumu":
        for p in gaussians.all_parameters():
            if p.grad is not None:
                p.grad /= bsz
    if use_mcmc:  # (one regulariser term per optimizer step, added to what the step consumes: no batch scale)
        mcmc.add_reg_grads(gaussians)
    if args.sparse_adam:
        gaussians.optimizer.step(visibility=visibility)
    else:
        gaussians.optimizer.step()
    gaussians.optimizer.zero_grad(set_to_none=True)
    if use_mcmc:
        mcmc.inject_noise(gaussians)


def build_exposure(train_cameras, iterations, device="cuda", lr_init=0.01, lr_final=0.001):
    """`--exposure`: an exposure.ExposureModel with one row per TRAINING camera, attached to the cameras (test cameras and
    novel views carry no exposure and are rendered as the model is).  Refused under camera-DP: every rank would step its
    own copy of the table; the all-reduce of the table's gradient is a later change."""
    _refuse([camera_dp_rule("exposure")])
    model = ExposureModel(len(train_cameras), device, lr_init=lr_init, lr_final=lr_final, max_steps=int(iterations))
    model.attach(train_cameras)
    return model


def build_bilagrid(train_cameras, iterations, device="cuda", grid=(16, 16, 8), lr_init=2e-3, lr_final=2e-5, tv_weight=10.0):
    """`--bilagrid`: a bilagrid.BilagridModel with one grid per TRAINING camera, attached to the cameras (test cameras and
    novel views carry none and are rendered as the model is).  Refused under camera-DP, for the reason of build_exposure."""
    _refuse([camera_dp_rule("bilagrid")])
    model = BilagridModel(len(train_cameras), device, grid=tuple(grid), lr_init=lr_init, lr_final=lr_final,
                          max_steps=int(iterations), tv_weight=tv_weight)
    model.attach(train_cameras)
    return model


def build_sky(train_cameras, other_cameras, iterations, device="cuda", shape=(256, 512), init=(0.5, 0.5, 0.5),
              lr_init=0.01, lr_final=0.001):
    """`--sky`: a sky.SkyModel, one map for the scene.  The training cameras train it; every other camera (test cameras,
    novel views) is rendered in front of it.  Refused under camera-DP, for the reason of build_exposure."""
    _refuse([camera_dp_rule("sky")])
    model = SkyModel(tuple(shape), device, init=tuple(init), lr_init=lr_init, lr_final=lr_final, max_steps=int(iterations))
    model.attach(train_cameras, train=True)
    model.attach(other_cameras, train=False)
    return model


def build_pose(train_cameras, iterations, device="cuda", lr=1e-5, reg=1e-6, noise=0.0, defer=True, seed=0):
    """`--pose_opt`: a pose.PoseModel with one row per TRAINING camera, attached to the cameras (test cameras carry no
    buffer and are evaluated as loaded).  `noise` > 0: gsplat's pose_noise, a seeded perturbation of the training poses."""
    model = PoseModel(len(train_cameras), lr=lr, reg=reg, max_steps=int(iterations), defer=defer, device=device)
    model.attach(train_cameras)
    if noise:
        model.perturb(float(noise), seed=seed)
    return model


# The side models of a run, in the order a batch steps them; each has end_batch(iteration, batch_cameras), flush() and
# save_to(model_dir, cameras).  `name`: the keyword of training() and the attribute of the scene; `flag`: its entry of
# utils.default_args; `file`: what save_to() writes; `not_shared`: why camera-DP refuses it (None: pose.check_pose_args).
SideModel = namedtuple("SideModel", "name flag build file not_shared")
SIDE_MODELS = (
    SideModel("exposure", "exposure", lambda a, train, other: build_exposure(
        train, a.iterations, "cuda", float(a.exposure_lr_init), float(a.exposure_lr_final)),
        ExposureModel.FILE, "the exposure table is not reduced"),
    SideModel("bilagrid", "bilagrid", lambda a, train, other: build_bilagrid(
        train, a.iterations, "cuda", tuple(a.bilagrid_shape), float(a.bilagrid_lr_init), float(a.bilagrid_lr_final),
        float(a.bilagrid_tv_weight)), BilagridModel.FILE, "the grid table is not reduced"),
    SideModel("sky", "sky", lambda a, train, other: build_sky(
        train, other, a.iterations, "cuda", tuple(a.sky_shape), tuple(a.sky_init), float(a.sky_lr_init),
        float(a.sky_lr_final)), SkyModel.FILE, "the map's gradient accumulator is not reduced"),
    SideModel("pose", "pose_opt", lambda a, train, other: build_pose(
        train, a.iterations, "cuda", float(a.pose_opt_lr), float(a.pose_opt_reg), float(a.pose_noise),
        bool(a.defer_pose_step)), PoseModel.FILE, None),
)


def camera_dp_rule(flag, on=True):
    """The (condition, message) rule of a side model whose table every rank would step on its own."""
    ws = dp.world_size()
    what = next(r.not_shared for r in SIDE_MODELS if r.flag == flag)
    return on and ws > 1, "--{0} is not supported with {1}; train on one GPU or without --{0}".format(
        flag, dp.refusal(ws, what))


def _refuse(rules):
    for refused, message in rules:
        if refused:
            raise ValueError(message)


def check_training(args, depth_priors=False, models=None, num_downscales=None, resolution_schedule=None, image_size=None):
    """Every refusal of a run, in one fixed order; train_from_colmap calls it before anything is loaded, training() at its
    top.  `depth_priors`: a depth directory was asked for, or a training camera carries a prior.  `models`
    ({SideModel.name: model}): a model handed in counts as its flag being set.  `num_downscales`,
    `resolution_schedule`: the values in force when they are not the args' own (training()'s parameters); `image_size`:
    (H, W) of the images once it is known (training(); train_from_colmap checks that one rule right after loading).  The trainer's own
    rules first, then the owners of pose refinement, MCMC and contribution pruning."""
    given = {r.flag for r in SIDE_MODELS if (models or {}).get(r.name) is not None}
    on = lambda flag: flag in given or bool(getattr(args, flag, False))
    _refuse([
        (depth_priors and on("absgrad"), "--absgrad together with --depths is not supported: absgrad blends three channels "
         "only, the depth regularisation renders the inverse depth as a fourth; drop one of the two"),
        (on("exposure") and on("bilagrid"), "--exposure and --bilagrid together are refused: the order in which the "
         "exposure transform and the bilateral grid compose is not defined; choose one"),
        (on("sky") and on("white_background"),
         "--sky and --white_background together are refused: the sky map is the background"),
        (on("sky") and on("pose_opt"), "--sky and --pose_opt together are refused: the sky's gradient with respect to the "
         "camera (the ray direction of the lookup) is not carried"),
    ] + undistort_rules(args) + compress_rules(args) + mesh_rules(args) + resolution_rules(args, on("pose_opt"), num_downscales, resolution_schedule, image_size) + [camera_dp_rule(r.flag, on(r.flag)) for r in SIDE_MODELS if r.not_shared])
    check_pose_args(args, depth_priors, enabled=on("pose_opt"))
    check_mcmc_args(args)
    check_contrib_prune_args(args)


def mesh_rules(args):
    """The (condition, message) rules of --mesh_voxel for check_training: checked before anything is loaded."""
    voxel = getattr(args, "mesh_voxel", 0.0)
    depth_mode = getattr(args, "mesh_depth_mode", None)
    components = (getattr(args, "mesh_min_component_faces", 0), getattr(args, "mesh_keep_components", 0))
    try:  # (refused with and without --mesh_voxel)
        from .mesh_clean import check_options as check_components
        check_components(*components, names=("--mesh_min_component_faces", "--mesh_keep_components"))
        from .mesh_decimate import check_cell
        decimate_cell = check_cell(getattr(args, "mesh_decimate_cell", 0.0), "--mesh_decimate_cell")
        from .mesh_smooth import check_options as check_smoothing
        smooth_iterations = check_smoothing(getattr(args, "mesh_smooth_iterations", 0), getattr(args, "mesh_smooth_lambda", 0.5),
                                            getattr(args, "mesh_smooth_mu", -0.53),
                                            ("--mesh_smooth_iterations", "--mesh_smooth_lambda", "--mesh_smooth_mu"))[0]
    except ValueError as e:
        return [(True, str(e))]
    if not voxel:
        return ([] if depth_mode is None else [(True, f"--mesh_depth_mode {depth_mode} has effect only with --mesh_voxel: "
                                                       "give both, or neither")]) + \
            ([(True, "--mesh_sparse has effect only with --mesh_voxel: give both, or neither")]
             if getattr(args, "mesh_sparse", False) else []) + \
            ([(True, "--mesh_decimate_cell has effect only with --mesh_voxel: give both, or neither")]
             if decimate_cell else []) + \
            [(True, f"{flag} has effect only with --mesh_voxel: give both, or neither")
             for flag, on in (("--mesh_smooth_iterations", smooth_iterations),
                              ("--mesh_normals", getattr(args, "mesh_normals", False))) if on]
    from .mesh_model import check_options
    try:
        check_options(voxel, None, getattr(args, "mesh_grid_gb", 16.0), getattr(args, "mesh_trunc_voxels", 4.0),
                      getattr(args, "mesh_min_weight", 2.0), getattr(args, "mesh_every", 1), depth_mode or "expected",
                      sparse=bool(getattr(args, "mesh_sparse", False)))
    except ValueError as e:
        return [(True, str(e).replace("--voxel", "--mesh_voxel").replace("--trunc_voxels", "--mesh_trunc_voxels")
                 .replace("--depth_mode", "--mesh_depth_mode")
                 .replace("--min_weight", "--mesh_min_weight").replace("--every", "--mesh_every").replace("--grid_gb", "--mesh_grid_gb"))]
    ws = dp.world_size()
    return [(ws > 1, "--mesh_voxel is not supported with {}; train on one GPU, or mesh the saved model with "
             "clm_gs_amd.mesh_model".format(dp.refusal(ws, "the eval entry renders every training camera on one rank")))]


def compress_bits(args):
    """The bit widths of --compress as compress.check_bits takes them (raises on one outside [1, 16])."""
    from .compress import BITS, check_bits
    return check_bits({b: getattr(args, "compress_" + b, v) for b, v in BITS.items()})


def compress_rules(args):
    """The (condition, message) rules of --compress for check_training: the knobs are checked before anything is loaded."""
    if not getattr(args, "compress", False):
        return []
    rules = [(not 1 <= int(getattr(args, "compress_codebook", 65536)) <= 65536,
              f"--compress_codebook must be in [1, 65536], got {getattr(args, 'compress_codebook', None)}"),
             (int(getattr(args, "compress_iters", 10)) < 0 or int(getattr(args, "compress_sample", 1)) < 1,
              "--compress_iters must be >= 0 and --compress_sample >= 1"),
             (int(getattr(args, "sh_degree", 3)) != 3, "--compress: SH degrees other than 3 are not supported")]
    try:
        compress_bits(args)
    except ValueError as e:
        rules.append((True, str(e)))
    return rules


def undistort_rules(args):
    """The (condition, message) rule of --undistort_zoom for check_training (the message is clm_kernels')."""
    try:
        check_undistort_zoom(getattr(args, "undistort_zoom", 1.0))
    except ValueError as e:
        return [(bool(getattr(args, "undistort", False)), str(e))]
    return []


# ---------------------------------------------------------------------------------------------- resolution schedule
MIN_LEVEL_SIDE = 16  # the shorter side of the coarsest level: one tile


def schedule_level(iteration, first_iteration, num_downscales, resolution_schedule):
    """The level a batch trains at: L = max(D - (it - it0) // R, 0), `it` the batch's first image counter (the `a` of
    its `iteration[a,b)` line), `it0` the first batch's.  nerfstudio splatfacto's num_downscales / resolution_schedule."""
    return max(int(num_downscales) - (int(iteration) - int(first_iteration)) // int(resolution_schedule), 0)


def resolution_rules(args, pose_opt=False, num_downscales=None, resolution_schedule=None, image_size=None):
    """The (condition, message) rules of --num_downscales / --resolution_schedule for check_training."""
    D = int(getattr(args, "num_downscales", 0) if num_downscales is None else num_downscales)
    R = int(getattr(args, "resolution_schedule", 3000) if resolution_schedule is None else resolution_schedule)
    ws = dp.world_size()
    side = None if image_size is None or D < 0 else -(-min(int(image_size[0]), int(image_size[1])) // (1 << min(D, 30)))
    return [
        (D < 0, "--num_downscales must be >= 0, got {}".format(D)),
        (R <= 0, "--resolution_schedule must be > 0 (images per level), got {}".format(R)),
        (D > 0 and pose_opt, "--num_downscales and --pose_opt together are refused: pose refinement rewrites the camera "
         "objects it was attached to, and the level views of the resolution schedule would go stale"),
        (D > 0 and ws > 1, "--num_downscales is not supported with {}; train on one GPU or without --num_downscales".format(
            dp.refusal(ws, "the level switch is not agreed"))),
        (D > 0 and side is not None and side < MIN_LEVEL_SIDE, "--num_downscales {} is too large for {} images: the shorter "
         "side of the coarsest level would be {} pixels, fewer than {}".format(
             D, "x".join(str(int(v)) for v in (image_size or (0, 0))[::-1]), side, MIN_LEVEL_SIDE)),
    ]


class _Resolution:
    """The resolution schedule of a run (D = --num_downscales > 0): which level a batch trains at, the LevelCameras of
    that level (one at a time; none at level 0), the global image size that goes with it, and full_size(), the one way
    anything outside the training step renders a full-size camera."""

    def __init__(self, train_cameras, num_downscales, resolution_schedule, bsz, first_iteration, log_file):
        self.cameras, self.bsz, self.it0, self.log_file = train_cameras, bsz, first_iteration, log_file
        self.D, self.R = int(num_downscales), int(resolution_schedule)
        self.full = (int(train_cameras[0].image_height), int(train_cameras[0].image_width))
        self.level, self.levels = None, None

    def level_at(self, iteration):
        return schedule_level(iteration, self.it0, self.D, self.R)

    def size(self):
        return self.levels.size if self.levels is not None else self.full

    def enter(self, iteration):
        """Called at the head of every batch: switches the level when the schedule says so."""
        level = self.level_at(iteration)
        if level == self.level:
            return
        self.level, self.levels = level, None  # the previous level's buffers are dropped before the new ones are built
        if level > 0:
            self.levels = LevelCameras(self.cameras, level, self.bsz)
        h, w = self.size()
        utils.set_img_size(h, w)
        self.log_file.write("resolution level {}: {}x{} from iteration {}\n".format(level, w, h, iteration))

    def batch(self, batch):
        return batch if self.levels is None else self.levels.batch(batch)

    def shells(self, iteration, batch):
        """A coming batch's cameras as that batch will get them (no image yet), or None across a level switch."""
        if batch is None or self.level_at(iteration) != self.level:
            return None
        return batch if self.levels is None else [self.levels.views[id(c)] for c in batch]

    @contextlib.contextmanager
    def full_size(self):
        """Inside: the global image size is the full one (evaluation, contribution pruning, anything that renders a camera
        outside the training step); the level's size is restored afterwards."""
        utils.set_img_size(*self.full)
        try:
            yield
        finally:
            utils.set_img_size(*self.size())

    def close(self):
        self.levels = None
        utils.set_img_size(*self.full)


class _BatchSource:
    """The shuffled camera order of a run (training()'s docstring), one batch ahead of the engine: the host-resident engine
    stages the next batch's untouched rows early.  With `locality` (camera-DP, locality exchange, dp.py) a rank draws from
    the cameras that look mostly at the rows it owns (index ranges of the Z-ordered tables = spatial regions)."""

    def __init__(self, train_cameras, gaussians, bsz, shuffle_seed, locality, log_file):
        self.cameras, self.gaussians, self.bsz, self.locality, self.log_file = train_cameras, gaussians, bsz, locality, log_file
        self.ws, self.rk, self.rng = dp.world_size(), dp.rank(), random.Random(shuffle_seed)
        self.order, self.pool, self.dealt_at, self.ahead = [], None, 0, None
        if locality:
            self.deal()

    def deal(self):
        ranks_of, _ = dp.deal_cameras(self.cameras, self.gaussians, self.ws)
        self.dealt_at, self.order = self.gaussians.get_xyz.shape[0], []
        # every rank computes the same deal, so every rank sees the same smallest pool -- no collective needed to agree.
        # A rank with fewer than bsz cameras could not draw a batch while the others are already inside the batch's
        # collectives (hang): then ALL ranks fall back to the strided deal of the global shuffled order (the locality
        # exchange is correct for any camera assignment, it just moves more border rows).
        smallest = min(sum(1 for q in ranks_of if q == r_) for r_ in range(self.ws))
        if smallest < self.bsz:
            self.pool = None
            self.log_file.write("camera-DP locality deal: smallest pool {} < bsz {} ({} cameras / {} ranks): strided deal\n".format(
                smallest, self.bsz, len(self.cameras), self.ws))
        else:
            self.pool = [i for i, q in enumerate(ranks_of) if q == self.rk]

    def draw(self):
        if self.locality and self.pool is not None:
            if len(self.order) < self.bsz:  # new epoch of THIS rank's pool
                self.order = list(self.pool)
                self.rng.shuffle(self.order)
            return [self.cameras[self.order.pop()] for _ in range(self.bsz)]
        gbsz = self.bsz * self.ws
        if len(self.order) < gbsz:  # new epoch: shuffle, drop_last (train.py:156-167)
            self.order = list(range(len(self.cameras)))
            self.rng.shuffle(self.order)
        return [self.cameras[self.order.pop()] for _ in range(gbsz)][self.rk::self.ws]

    def next(self, more):
        """-> (this batch, the batch after it or None when `more` is false)."""
        batch = self.ahead if self.ahead is not None else self.draw()
        self.ahead = self.draw() if more else None
        return batch, self.ahead

    def resorted(self):
        """After a re-sort of a model that changed size: a new deal once it is 10 % away from the last one."""
        if self.locality and abs(self.gaussians.get_xyz.shape[0] - self.dealt_at) > 0.1 * self.dealt_at:
            self.deal()
            self.ahead = None  # drawn from the old pool


def _strategy(args, gaussians, scene, background):
    """-> (run_batch, render_fn) of the engine the args name.  run_batch(batch) -> (losses, image names in the order of the
    losses, sparsity or None, visibility or None); render_fn(camera) -> the evaluation image."""
    if bool(getattr(args, "clm_offload", False)) and not bool(getattr(args, "naive_offload", False)):
        from .strategies.clm_offload import clm_offload_eval_one_cam, clm_offload_train_one_batch
        comm_stream = torch.cuda.Stream()
        perm_generator = torch.Generator(device="cuda")
        perm_generator.manual_seed(1)

        def run_batch(batch):
            losses, ordered_cams, sparsity = clm_offload_train_one_batch(
                gaussians, scene, batch, gaussians.parameters_grad_buffer, background, None, comm_stream,
                perm_generator)
            return losses, [batch[i].image_name for i in ordered_cams], sparsity, None
        return run_batch, lambda cam: clm_offload_eval_one_cam(cam, gaussians, background, scene)
    if bool(getattr(args, "naive_offload", False)):
        from .strategies.naive_offload import naive_offload_eval_one_cam, naive_offload_train_one_batch as one_batch
        render_fn = lambda cam: naive_offload_eval_one_cam(gaussians, scene, cam, background)
    else:
        from .strategies.no_offload import baseline_accumGrads_impl as one_batch, baseline_accumGrads_micro_step

        def render_fn(cam):
            img, _, _, _ = baseline_accumGrads_micro_step(
                gaussians.get_xyz, gaussians.get_opacity, gaussians.get_scaling, gaussians.get_rotation,
                gaussians.get_features, gaussians.active_sh_degree, cam, background, mode="test")
            return apply_camera_colour(img, cam)  # a training camera is rendered as it was trained

    def run_batch(batch):
        losses, visibility = one_batch(gaussians, scene, batch, background, sparse_adam=args.sparse_adam)
        return losses, [c.image_name for c in batch], None, visibility
    return run_batch, render_fn


def _acc(pt, key, t_start):
    pt[key] = pt.get(key, 0.0) + time.perf_counter() - t_start


def _setup_before_clock(args, gaussians, pt):
    """What a run pays once, before the end-to-end clock starts (utils/timer.py:87-111 starts it at the first iteration);
    the wall times go into `pt` as phases "reserve" and "warm_ops"."""
    # a full cyclic GC pass over torch's ~10^6 long-lived objects stalls the enqueueing thread for
    # ~100 ms: freeze what exists now, later collections only see what the loop allocates
    gc.collect()
    gc.freeze()
    if clm_hbm_only(args) and getattr(args, "allocator_reservoir", True) and getattr(args, "fused_front_end", True):
        # allocator warm-up: one block per stream pool instead of dozens of hipMalloc calls spread over the first batches
        # and every densification (strategies/clm_offload/engine.py reserve_working_set).  SETUP, like the reference's
        # --prealloc_capacity buffers (train.py:107-115).  (Fresh device memory costs ~0.1 s per GB on some boxes and
        # nothing on others -- measured 0.002 .. 1.3 s for the same 10 GB.)
        from .strategies.clm_offload.engine import reserve_working_set
        _t = time.perf_counter()
        pt["reserved_bytes"] = float(sum(reserve_working_set(gaussians).values()))
        torch.cuda.synchronize()
        _acc(pt, "reserve", _t)
        if not args.disable_auto_densification and getattr(args, "warm_structural_ops", True):
            _t = time.perf_counter()
            _warm_structural_ops(gaussians._xyz.device)
            _acc(pt, "warm_ops", _t)
    if torch.cuda.is_available():  # (diagnosis: how many hipMallocs happen INSIDE the end-to-end clock -- bench.py reports it)
        pt["device_mallocs_before_clock"] = float(torch.cuda.memory_stats().get("num_device_alloc", 0))


def training(gaussians, scene, train_cameras, test_cameras, log_file, iterations=None,
             test_iterations=(), background=None, shuffle_seed=0, phase_times=None, num_downscales=None,
             resolution_schedule=None, **side_models):
    """Runs `iterations` images of training; returns the End2endTimer.
    `side_models`: exposure=, bilagrid=, sky=, pose= (the names of SIDE_MODELS; each optional, attached to its cameras by
    its build_* function).  All are stepped after every batch in the table's order (end_batch), on the current stream --
    every engine has joined its camera streams into it by the time it returns -- and flushed before the training cameras
    are rendered (evaluation, contribution pruning) and at the end.  A model handed in is refused like its flag.
    `phase_times` (optional dict): host wall time per phase inside the end-to-end clock is accumulated into it
    ("engine" = enqueueing the batches, "densify" = gsplat_densification incl. the device work it waits for,
    "resort" = the Z-order re-sort after a densification, "log" = waiting for loss values, "final_sync"); a callable under
    "iter_hook" is removed from the dict and called with the image counter after every iteration (diagnosis).

    Camera-DP: when a process group is up every rank runs this same loop over the same shuffled order, takes
    cameras rank::ranks of each GLOBAL batch (bsz x ranks images), and the image counter strides by the global batch; the
    engine does the one exchange per batch, densification reduces its statistics and draws identical split samples.

    Resolution schedule (`num_downscales` D, `resolution_schedule` R; None: the values of the args):
    with D > 0 a batch whose first image counter is `it` trains at level schedule_level(it, 1, D, R) on the level's views of
    its cameras (cameras.LevelCameras) with the global image size set to the level's; evaluation and contribution pruning
    run at full size (_Resolution.full_size).  When training returns or raises, the global image size is the full one."""
    args = utils.get_args()
    D = int(getattr(args, "num_downscales", 0) if num_downscales is None else num_downscales)
    R = int(getattr(args, "resolution_schedule", 3000) if resolution_schedule is None else resolution_schedule)
    # the schedule: None when off -- no LevelCameras, no new kernel, not one call differs
    res = _Resolution(train_cameras, D, R, args.bsz, 1, log_file) if D > 0 and R > 0 and train_cameras else None
    try:
        return _training(gaussians, scene, train_cameras, test_cameras, log_file, iterations, test_iterations, background,
                         shuffle_seed, phase_times, side_models, D, R, res)
    finally:
        if res is not None:
            res.close()


def _training(gaussians, scene, train_cameras, test_cameras, log_file, iterations, test_iterations, background,
              shuffle_seed, phase_times, side_models, num_downscales, resolution_schedule, res):
    args = utils.get_args()
    if set(side_models) - {r.name for r in SIDE_MODELS}:
        raise TypeError("training() got unexpected keyword arguments {}".format(sorted(side_models)))
    models = [side_models[r.name] for r in SIDE_MODELS if side_models.get(r.name) is not None]
    depth_priors = any(getattr(c, "invdepth", None) is not None for c in train_cameras)
    check_training(args, depth_priors, side_models, num_downscales, resolution_schedule,
                   (train_cameras[0].image_height, train_cameras[0].image_width) if train_cameras else None)
    bsz, ws = args.bsz, dp.world_size()
    gbsz = bsz * ws
    if ws > 1:
        assert clm_hbm_only(args), "camera-DP trains clm_offload with sh_residency='hbm'"
        if getattr(gaussians, "split_generator", None) is None:
            dp.seed_split_generator(gaussians)
    iterations = iterations or args.iterations
    utils.set_log_file(log_file)
    clm, naive = bool(getattr(args, "clm_offload", False)), bool(getattr(args, "naive_offload", False))
    no_offload = not clm and not naive
    run_batch, render_fn = _strategy(args, gaussians, scene, background)
    host_rows = clm and getattr(args, "sh_residency", "hbm") == "host"
    if host_rows:
        from .strategies.clm_offload.engine import hint_next_batch
    spatial = bool(getattr(args, "spatial_row_order", True)) and hasattr(gaussians, "spatial_sort") and not naive
    if spatial:
        gaussians.spatial_sort()  # rows along a Z-order curve: a camera's rows become contiguous runs
        # the prune that ends a densification re-sorts in the same pass over the row tables (clm_offload model, HBM rows)
        gaussians.fuse_sort_into_prune = clm_hbm_only(args)
    locality = ws > 1 and bool(getattr(args, "dp_locality", False))
    assert spatial or not locality, "dp_locality needs the Z-ordered row tables (spatial_row_order)"
    batches = _BatchSource(train_cameras, gaussians, bsz, shuffle_seed, locality, log_file)
    from . import _lib
    # wherever the host has just synchronised: an asynchronous device fault / a raised device error word (the deferred
    # small-attribute Adam) surfaces THERE, not at the end of the run with the model unsaved
    _check_device = _lib.check_device_errors
    defer = bool(getattr(args, "defer_loss_log", True))
    contrib_iters = prune_iterations(args)
    use_mcmc = mcmc.enabled(args)
    loss_log = _LossLog(log_file, defer)
    pt = phase_times if phase_times is not None else {}
    iter_hook = pt.pop("iter_hook", None)  # diagnosis only (bench.py --trainer-trace): called after every iteration
    _setup_before_clock(args, gaussians, pt)
    timer = End2endTimer()
    full_size = res.full_size if res is not None else contextlib.nullcontext
    timer.start()
    for iteration in range(1, iterations + 1, gbsz):
        utils.set_cur_iter(iteration)
        gaussians.update_learning_rate(iteration)
        if utils.check_update_at_this_iter(iteration, gbsz, 1000, 0):
            gaussians.oneupSHdegree()
        batch, next_batch = batches.next(more=iteration + gbsz <= iterations)
        level_batch = batch
        if res is not None:  # the batch's level: its cameras' views, their ground truth resampled into the ring
            res.enter(iteration)
            level_batch, next_batch = res.batch(batch), res.shells(iteration + gbsz, next_batch)
        if host_rows:
            hint_next_batch(gaussians, next_batch)
        _t = time.perf_counter()
        losses, names, sparsity, visibility = run_batch(level_batch)
        _acc(pt, "engine", _t)
        _t = time.perf_counter()
        # with depth priors: the depth term's weight of this iteration, next to the losses it is part of
        depth_note = " depth_l1_weight: {:.6f}".format(utils.depth_l1_weight(iteration)) if depth_priors else ""
        loss_log.push("iteration[{},{}) loss: ".format(iteration, iteration + gbsz), losses,
                      depth_note + " image: {}".format(names) + ((" sparsity: " + " ".join("%.4f" % s for s in sparsity) + "\n")
                                                   if sparsity else "\n"))
        _acc(pt, "log", _t)
        if any(iteration <= t < iteration + gbsz for t in test_iterations):
            loss_log.flush()
            for model in models:
                model.flush()  # training cameras are evaluated at their refined pose
            timer.stop()  # evaluation is excluded from the throughput figure
            _check_device()
            if hasattr(gaussians, "flush_lazy_rows"):  # deferred row steps (and, owner-computes DP, the exchange)
                gaussians.flush_lazy_rows()
            with full_size():
                evaluate("train", iteration, train_cameras, render_fn, log_file, max_images=5)
                if test_cameras:
                    evaluate("test", iteration, test_cameras, render_fn, log_file)
            timer.start()
        n_before = gaussians.get_xyz.shape[0]
        _t = time.perf_counter()
        if use_mcmc:
            # the batch's optimizer step and noise come first (clm_offload: inside the engine): a refinement moves rows of
            # stepped parameters, and the gradients of a batch belong to the rows as they were rendered
            if no_offload:
                no_offload_optimizer_step(gaussians, args, bsz, visibility)
            mcmc_refinement(iteration, scene, gaussians)
        else:
            gsplat_densification(iteration, scene, gaussians, None)
        _acc(pt, "densify", _t)
        if gaussians.get_xyz.shape[0] != n_before:
            _check_device()  # (densify_and_prune read its counts back: the device is drained)
        if spatial and gaussians.get_xyz.shape[0] != n_before:
            _t = time.perf_counter()
            gaussians.spatial_sort()  # clones / splits were appended at the end of the tables
            _acc(pt, "resort", _t)
            batches.resorted()
        if gaussians.get_xyz.shape[0] != n_before or utils.check_update_at_this_iter(
                iteration, gbsz, args.mcmc_refine_every if use_mcmc else args.densification_interval, 0):
            loss_log.flush()  # keep the reference's line order: the batch's loss line, then the memory line
            log_file.write(memory_line(iteration, gbsz, gaussians))
        if no_offload and not use_mcmc:  # train.py:533-578
            no_offload_optimizer_step(gaussians, args, bsz, visibility)
        for model in models:
            model.end_batch(iteration, batch)
        if contrib_iters and any(iteration <= t < iteration + gbsz for t in contrib_iters):
            # contribution pruning (contribution.py): after the batch's optimizer step, so no gradient is waiting for rows
            # that leave; the training cameras are scored at the poses they carry
            loss_log.flush()
            for model in models:
                model.flush()
            _t = time.perf_counter()
            with full_size():
                contribution_prune(gaussians, train_cameras, getattr(args, "contrib_prune_mode", "sum"),
                                   float(getattr(args, "contrib_prune_ratio", 0.3)),
                                   float(getattr(args, "contrib_prune_threshold", 0.01)),
                                   resort=spatial and bool(getattr(gaussians, "fuse_sort_into_prune", False)),
                                   log_file=log_file, iteration=iteration)
            if spatial:
                gaussians.spatial_sort()
            _acc(pt, "contrib_prune", _t)
            _check_device()
            log_file.write(memory_line(iteration, gbsz, gaussians, what="contribution_prune"))
        if not defer:
            torch.cuda.synchronize()
        if iter_hook is not None:
            iter_hook(iteration)
    _t = time.perf_counter()
    loss_log.flush()
    for model in models:
        model.flush()
    timer.stop()
    _acc(pt, "final_sync", _t)
    _check_device()
    n_done = ((iterations - 1) // gbsz + 1) * gbsz + 1
    timer.print_time(log_file, n_done)
    log_file.write(memory_line(iteration, gbsz, gaussians, what="final"))
    log_file.write("Max Memory usage: {} GB.\n".format(torch.cuda.max_memory_allocated() / 2 ** 30))
    return timer


def train_from_colmap(source_path, model_path, strategy="clm_offload", iterations=None, eval=False, resolution=1,
                      images="images", test_iterations=(), save=True, masks=None, alpha_mask=False, depths=None,
                      num_downscales=0, resolution_schedule=3000, undistort=False, undistort_zoom=1.0, **arg_overrides):
    """A COLMAP directory -> trained model (row f1): `colmap_scene.load_colmap_scene` (cameras, held-out
    split, scene radius, sparse points) -> `create_from_pcd` with `spatial_lr_scale = cameras_extent` ->
    `training_setup` -> `training` (log lines of the reference in `<model_path>/python_ws=1_rk=0.log`) ->
    `point_cloud/iteration_N/point_cloud.ply` (scene/__init__.py:41-143, train.py:60-131 for the order of
    these steps).  `strategy`: clm_offload | no_offload | naive_offload; `masks` / `alpha_mask` / `depths`: the arguments of
    colmap_scene.load_colmap_scene; `num_downscales` / `resolution_schedule`: the
    resolution schedule (training()); `undistort` / `undistort_zoom`: distorted COLMAP cameras and off-centre principal
    points are remapped onto centred pinholes on the device at load (load_colmap_scene; its per-camera lines head the
    log); `arg_overrides`: any flag of `utils.default_args`, described there and, for the ones the
    command line has, in OPTIONS.  Every refusal is raised by check_training before anything is loaded.  A side model that
    is asked for (SIDE_MODELS) is written next to the ply and stays reachable as `scene.<name>`, None when off.
    Returns (gaussians, scene, timer)."""
    from .colmap_scene import load_colmap_scene
    from .strategies.clm_offload import GaussianModelCLMOffload
    from .strategies.naive_offload import GaussianModelNaiveOffload
    from .strategies.no_offload import GaussianModelNoOffload
    assert strategy in ("clm_offload", "no_offload", "naive_offload"), strategy
    args = utils.default_args(num_downscales=int(num_downscales), resolution_schedule=int(resolution_schedule),
                              undistort=bool(undistort), undistort_zoom=float(undistort_zoom), **arg_overrides)
    setattr(args, strategy, True)
    args.source_path, args.model_path, args.eval = source_path, model_path, bool(eval)
    if iterations is not None:
        args.iterations = int(iterations)
    args.depths = depths or ""
    check_training(args, bool(depths))  # raises: before anything is loaded
    utils.set_args(args)
    scene = load_colmap_scene(source_path, images=images, eval=eval, resolution=resolution, device="cuda",
                              masks=masks, alpha_mask=alpha_mask, depths=depths, undistort=args.undistort,
                              undistort_zoom=args.undistort_zoom)
    if scene.point_cloud is None:
        raise ValueError(f"{source_path}/sparse/0 holds no points3D.bin / points3D.txt to initialise from")
    sizes = {(c.image_height, c.image_width) for c in scene.train_cameras + scene.test_cameras}
    assert len(sizes) == 1, f"all images must share one size (utils.get_img_width/height are global): {sizes}"
    h, w = next(iter(sizes))
    _refuse(resolution_rules(args, image_size=(h, w)))  # (the one rule that needs the images' size)
    utils.set_img_size(h, w)
    utils.set_cur_iter(1)
    gaussians = {"clm_offload": GaussianModelCLMOffload, "no_offload": GaussianModelNoOffload,
                 "naive_offload": GaussianModelNaiveOffload}[strategy](args.sh_degree)
    gaussians.create_from_pcd(scene.point_cloud, scene.cameras_extent)
    gaussians.training_setup(args)
    for row in SIDE_MODELS:
        setattr(scene, row.name, row.build(args, scene.train_cameras, scene.test_cameras) if getattr(args, row.flag) else None)
    os.makedirs(model_path, exist_ok=True)
    prev_log = utils.get_log_file()
    try:
        with open(os.path.join(model_path, "python_ws=1_rk=0.log"), "w") as log_file:
            for line in scene.undistort_log:
                log_file.write(line + "\n")
            timer = training(gaussians, scene, scene.train_cameras, scene.test_cameras, log_file,
                             iterations=args.iterations, test_iterations=test_iterations,
                             **{row.name: getattr(scene, row.name) for row in SIDE_MODELS})
    finally:
        utils.set_log_file(prev_log)  # never leave a closed file as the process-wide log
    if save:
        if hasattr(gaussians, "flush_lazy_rows"):
            gaussians.flush_lazy_rows()  # ALL ranks (a collective under owner-computes / locality camera-DP) ...
        if dp.rank() == 0:               # ... then rank-0-only I/O (no collective left inside save_ply: nothing is dirty)
            ply = os.path.join(model_path, "point_cloud", f"iteration_{args.iterations}", "point_cloud.ply")
            gaussians.save_ply(ply)
            if args.compress:
                from .compress_model import compress_file
                with open(os.path.join(model_path, "python_ws=1_rk=0.log"), "a") as log_file:
                    compress_file(ply, ply[:-4] + ".vq.npz", args.compress_codebook, args.compress_iters, args.compress_sample,
                                  compress_bits(args), log=log_file)
            if args.mesh_voxel:
                from .mesh_model import build_mesh
                with open(os.path.join(model_path, "python_ws=1_rk=0.log"), "a") as log_file:
                    build_mesh(gaussians, scene.train_cameras, args, os.path.join(model_path, "mesh.ply"), args.mesh_voxel,
                               trunc_voxels=args.mesh_trunc_voxels, every=args.mesh_every, min_weight=args.mesh_min_weight,
                               grid_gb=args.mesh_grid_gb, log=log_file,
                               depth_mode=getattr(args, "mesh_depth_mode", None) or "expected",
                               min_component_faces=getattr(args, "mesh_min_component_faces", 0),
                               keep_components=getattr(args, "mesh_keep_components", 0),
                               sparse=bool(getattr(args, "mesh_sparse", False)),
                               decimate_cell=getattr(args, "mesh_decimate_cell", 0.0),
                               smooth_iterations=getattr(args, "mesh_smooth_iterations", 0),
                               smooth_lambda=getattr(args, "mesh_smooth_lambda", 0.5),
                               smooth_mu=getattr(args, "mesh_smooth_mu", -0.53),
                               normals=bool(getattr(args, "mesh_normals", False)))
            for row in SIDE_MODELS:
                if getattr(scene, row.name) is not None:
                    getattr(scene, row.name).save_to(model_path, scene.train_cameras)
    return gaussians, scene, timer


def _opt(*names, to=None, conv=None, **kw):
    """One option -> (argparse's names, its keyword arguments, the attribute of the parsed namespace, the name
    train_from_colmap / utils.default_args knows the value by, a converter of the parsed value or None).  An option that
    states no default (and is no switch) takes the one of utils.default_args."""
    dest = kw.get("dest") or next(n for n in names if n.startswith("--"))[2:]
    return names, kw, dest, to or dest, conv


OPTIONS = (
    _opt("-s", "--source_path", required=True), _opt("-m", "--model_path", required=True),
    _opt("-i", "--images", default="images"), _opt("-r", "--resolution", type=float, default=1),
    _opt("--eval", action="store_true"), _opt("--iterations", type=int), _opt("--bsz", type=int, default=4),
    _opt("--test_iterations", type=int, nargs="*", default=[7000, 30000], conv=tuple),
    *(_opt("--" + s, action="store_const", const=s, dest="strategy", default="clm_offload", exclusive=True)
      for s in ("clm_offload", "no_offload", "naive_offload")),
    _opt("--sh_residency", choices=["hbm", "host"]),
    _opt("--sh_hbm_budget_gb", type=float,
         help="sh_residency=host: HBM that keeps the first rows of the Z-ordered SH table resident (768 B per row)"),
    _opt("--absgrad", action="store_true",
         help="densify on sum_p |dL_p/dmean2d| (gsplat's absgrad); gsplat's recipe raises the threshold to 8e-4"),
    _opt("--antialiased", action="store_true", to="rasterize_mode", conv=lambda on: "antialiased" if on else "classic",
         help="gsplat's rasterize_mode=\"antialiased\" (Mip-Splatting opacity compensation); render the model with it too"),
    _opt("--masks", default=None, metavar="DIR", help="directory of per-image loss masks (NAME.EXT.png or NAME.png, 0 = "
         "pixel ignored by the loss), relative to the source path or absolute"),
    _opt("--alpha_mask", action="store_true",
         help="images with an alpha channel and no mask file: the loss ignores pixels with alpha 0"),
    _opt("--exposure", action="store_true", help="per-camera exposure compensation: a learnable 3x4 affine colour "
         "transform per training image, written to <model_path>/exposure.json (single GPU)"),
    _opt("--exposure_lr_init", type=float), _opt("--exposure_lr_final", type=float),
    _opt("--bilagrid", action="store_true", help="bilateral-grid colour correction (gsplat's use_bilateral_grid): a "
         "learnable lattice of 3x4 affine colour transforms per training image, sliced by position and luminance, written to "
         "<model_path>/bilagrid.npz (single GPU; not with --exposure)"),
    _opt("--bilagrid_shape", type=int, nargs=3, metavar=("WG", "HG", "L"), conv=tuple),
    _opt("--bilagrid_lr_init", type=float), _opt("--bilagrid_lr_final", type=float), _opt("--bilagrid_tv_weight", type=float),
    _opt("--sky", action="store_true", help="learnable sky: one equirectangular environment map composited behind the "
         "splats and trained by the same loss, written to <model_path>/sky.npz; render the model with --sky too (single GPU; "
         "not with --white_background or --pose_opt)"),
    _opt("--sky_shape", type=int, nargs=2, metavar=("HS", "WS"), conv=tuple),
    _opt("--sky_init", type=float, nargs=3, metavar=("R", "G", "B"), conv=tuple),
    _opt("--sky_lr_init", type=float), _opt("--sky_lr_final", type=float),
    _opt("-d", "--depths", default=None, metavar="DIR", help="depth regularisation: directory (relative to the source path "
         "or absolute) of 16-bit inverse-depth PNGs NAME.png, scaled by sparse/0/depth_params.json; an L1 term on the rendered "
         "inverse depth of every training image with a reliable prior (not with --absgrad)"),
    _opt("--depth_l1_weight_init", type=float), _opt("--depth_l1_weight_final", type=float),
    _opt("--pose_opt", action="store_true", help="camera pose refinement (gsplat's pose_opt): a learnable rigid correction "
         "per training image, written to <model_path>/poses.json (fused front end, SH rows in HBM, single GPU; not with "
         "--depths)"),
    _opt("--pose_opt_lr", type=float), _opt("--pose_opt_reg", type=float),
    _opt("--pose_noise", type=float,
         help="--pose_opt: seeded random perturbation of the training poses at the start (experiments)"),
    _opt("--immediate_pose_step", action="store_true", to="defer_pose_step", conv=lambda on: not on,
         help="--pose_opt: apply a batch's pose step before the next batch is enqueued (the host waits)"),
    _opt("--mcmc", action="store_true", help="3DGS-MCMC densification (gsplat's MCMCStrategy): a fixed budget of --cap_max "
         "Gaussians, dead ones relocated instead of pruned, 5 %% growth per refinement, position noise after every step "
         "(no_offload, or clm_offload with --sh_residency hbm; single GPU)"),
    _opt("--cap_max", type=int, to="mcmc_cap_max", help="--mcmc: the number of Gaussians the model grows to"),
    _opt("--mcmc_noise_lr", type=float), _opt("--mcmc_refine_start_iter", type=int),
    _opt("--mcmc_refine_stop_iter", type=int), _opt("--mcmc_refine_every", type=int),
    _opt("--mcmc_min_opacity", type=float), _opt("--mcmc_opacity_reg", type=float), _opt("--mcmc_scale_reg", type=float),
    _opt("--disable_auto_densification", action="store_true"),
    _opt("--num_downscales", type=int, metavar="D", help="resolution schedule (splatfacto's num_downscales): train at 1/2^D "
         "of the size first and double it every --resolution_schedule images; ground truth, masks and depth priors are "
         "area-resampled on the device; evaluation and the final model are full size (single GPU; not with --pose_opt)"),
    _opt("--resolution_schedule", type=int, metavar="R", help="--num_downscales: images trained at each coarse level"),
    _opt("--undistort", action="store_true", help="lens distortion: SIMPLE_RADIAL / RADIAL / OPENCV / OPENCV_FISHEYE cameras "
         "and off-centre principal points are remapped onto centred pinholes on the device at load (images, masks, depth "
         "priors); pixels without a source are ignored by the loss"),
    _opt("--undistort_zoom", type=float, metavar="Z", help="--undistort: the pinhole's focal length is Z x the lens'; Z < 1 "
         "widens it to keep more of a barrel or fisheye frame"),
    _opt("--contrib_prune_iterations", type=int, nargs="*", metavar="I", conv=tuple, help="contribution pruning: image "
         "counters at which the training cameras are scored by blend weight and the model is pruned; each after "
         "densify_until_iter unless --disable_auto_densification (no_offload or clm_offload; single GPU; not with --mcmc)"),
    _opt("--contrib_prune_mode", choices=["sum", "max"], help="sum: prune the lowest --contrib_prune_ratio of rows by "
         "summed weight; max: prune rows whose largest weight is below --contrib_prune_threshold"),
    _opt("--contrib_prune_ratio", type=float), _opt("--contrib_prune_threshold", type=float),
    _opt("--compress", action="store_true", help="compressed export: after the final .ply also write point_cloud.vq.npz next "
         "to it (SH vector quantisation + quantised attributes, clm_gs_amd.compress_model) and log its size line"),
    _opt("--compress_codebook", type=int, metavar="K", help="--compress: number of SH centroids (<= 65536)"),
    _opt("--compress_iters", type=int), _opt("--compress_sample", type=int),
    *(_opt("--compress_" + b, type=int) for b in ("pos_bits", "scale_bits", "opacity_bits", "rot_bits", "dc_bits")),
    _opt("--mesh_voxel", type=float, metavar="V", help="mesh export: after the final .ply also write <model_path>/mesh.ply, "
         "the training cameras' depth maps fused into a TSDF volume of V world units per voxel and its surface "
         "(clm_gs_amd.mesh_model; single GPU); 0 = off"),
    _opt("--mesh_trunc_voxels", type=float), _opt("--mesh_min_weight", type=float), _opt("--mesh_every", type=int),
    _opt("--mesh_grid_gb", type=float),
    _opt("--mesh_depth_mode", metavar="expected|median|ray", help="--mesh_voxel: fuse the expected depth (default), the "
         "median depth, the depth of the Gaussian at which the transmittance falls through one half, or the ray depth, "
         "the depth at which that Gaussian's density peaks along the pixel's ray"),
    _opt("--mesh_min_component_faces", type=int, metavar="N", help="--mesh_voxel: drop the connected components of the mesh "
         "with fewer than N faces (clm_gs_amd.mesh_clean); 0 = off"),
    _opt("--mesh_keep_components", type=int, metavar="K", help="--mesh_voxel: keep only the K connected components with the "
         "most faces; 0 = off"),
    _opt("--mesh_sparse", action="store_true", help="--mesh_voxel: the brick-allocated volume (mesh_model --sparse): the same "
         "mesh.ply, on boxes beyond the dense volume's 2^31 voxels; renders every camera twice"),
    _opt("--mesh_decimate_cell", type=float, metavar="C", help="--mesh_voxel: decimate the mesh before it is written: merge "
         "the vertices of every cell of C world units (quadric vertex clustering, clm_gs_amd.mesh_decimate); 0 = off"),
    _opt("--mesh_smooth_iterations", type=int, metavar="N", help="--mesh_voxel: smooth the mesh before the decimation: N "
         "passes of Taubin's lambda | mu smoothing (clm_gs_amd.mesh_smooth); 0 = off"),
    _opt("--mesh_smooth_lambda", type=float, metavar="L", help="--mesh_smooth_iterations: the factor of a pass's first "
         "step, in (0, 1]"),
    _opt("--mesh_smooth_mu", type=float, metavar="M", help="--mesh_smooth_iterations: the factor of a pass's second step, "
         "in [-1, 0]; 0 = plain Laplacian smoothing"),
    _opt("--mesh_normals", action="store_true", help="--mesh_voxel: write area-weighted vertex normals (nx ny nz) into "
         "mesh.ply"),
)


def build_arg_parser():
    """The command line of `python -m clm_gs_amd.trainer`, from OPTIONS."""
    import argparse
    ap = argparse.ArgumentParser(description="train a 3DGS model from a COLMAP directory (flag names of train.py)")
    defaults, exclusive = utils.default_args(), ap.add_mutually_exclusive_group()
    for names, kw, _, to, _ in OPTIONS:
        kw = dict(kw)
        if "default" not in kw and "required" not in kw and kw.get("action") != "store_true":
            kw["default"] = list(getattr(defaults, to)) if "nargs" in kw else getattr(defaults, to)
        (exclusive if kw.pop("exclusive", False) else ap).add_argument(*names, **kw)
    return ap


def train_kwargs(namespace):
    """A namespace of build_arg_parser() -> the keyword arguments of train_from_colmap."""
    return {to: conv(getattr(namespace, dest)) if conv else getattr(namespace, dest) for _, _, dest, to, conv in OPTIONS}


def main(argv=None):
    """python -m clm_gs_amd.trainer -s <colmap dir> -m <output dir> [--clm_offload] ...  (clm_gs_amd/__init__.py has applied
    runtime_env.single_gpu_runtime_defaults() before torch was imported: bench.py's hardware-queue default is the trainer's)"""
    train_from_colmap(**train_kwargs(build_arg_parser().parse_args(argv)))
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
