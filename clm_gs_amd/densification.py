"""Densification schedule and per-micro-batch statistics (reference: densification.py:5-147)."""

from . import dp, utils
from .clm_kernels import densify_stats


def _in_window(args, iteration):
    return (not args.disable_auto_densification) and iteration <= args.densify_until_iter


def gsplat_densification(iteration, scene, gaussians, batched_screenspace_pkg=None):
    """Every densification_interval images inside (densify_from_iter, densify_until_iter]:
    densify_and_prune; every opacity_reset_interval images: reset_opacity (densification.py:5-56).
    Triggers use the bsz-stride test so no image index is skipped (camera-DP: the image counter
    strides by the GLOBAL batch, bsz x ranks)."""
    args = utils.get_args()
    gbsz = args.bsz * dp.world_size()
    timers = utils.get_timers()
    if not _in_window(args, iteration):
        return
    timers.start("densification")
    if iteration > args.densify_from_iter and utils.check_update_at_this_iter(
            iteration, gbsz, args.densification_interval, 0):
        assert not args.stop_update_param
        gaussians.optimizer.zero_grad(set_to_none=True)
        if getattr(gaussians, "small_owner", False):
            # camera-DP with the small attributes at their owners: scales / opacities / positions of foreign rows are
            # stale until the replicas are completed -- the clone / split / prune masks are computed from them
            gaussians.flush_lazy_rows()
        if getattr(gaussians, "small_deferred", False):
            gaussians.flush_small()  # single GPU, small attributes stepped per block: the same, for the waiting steps
        dp.allreduce_densify_stats(gaussians)  # camera-DP: sum / sum / max over ranks
        timers.start("densify_and_prune")
        size_threshold = 20 if iteration > args.opacity_reset_interval else None
        gaussians.densify_and_prune(args.densify_grad_threshold, args.min_opacity,
                                    scene.cameras_extent, size_threshold)
        timers.stop("densify_and_prune")
        utils.inc_densify_iter()
    if utils.check_update_at_this_iter(iteration, gbsz, args.opacity_reset_interval, 0):
        timers.start("reset_opacity")
        gaussians.reset_opacity()
        timers.stop("reset_opacity")
    timers.stop("densification")


def check_mcmc_args(args):
    """MCMC densification runs on no_offload and on clm_offload with the SH rows in HBM and the fused front end; every
    other combination is refused here, before training starts, with a message naming the flag."""
    if not bool(getattr(args, "mcmc", False)):
        return
    why = None
    if getattr(args, "sh_residency", "hbm") == "host":
        why = 'sh_residency="host": relocation rewrites SH rows and their moments in place, in HBM'
    elif float(getattr(args, "sh_hbm_budget_gb", 0.0) or 0.0) > 0.0:
        why = "sh_hbm_budget_gb > 0: the HBM-resident prefix belongs to the host-resident mode"
    elif bool(getattr(args, "naive_offload", False)):
        why = "naive_offload: its model keeps the parameters in pinned host tables"
    elif dp.world_size() > 1:
        why = dp.refusal(dp.world_size(), "sampling, noise and row surgery are not replicated")
    elif bool(getattr(args, "sparse_adam", False)):
        why = "sparse_adam: the noise and the regularisers step every row, a visibility-masked optimizer does not"
    elif bool(getattr(args, "stop_update_param", False)):
        why = "stop_update_param: there is no optimizer step to add the regularisers to or to inject noise after"
    elif bool(getattr(args, "clm_offload", False)) and not bool(getattr(args, "fused_front_end", True)):
        why = "clm_offload with fused_front_end=False: the MCMC passes work on the packed tables of the fused front end"
    if why:
        raise ValueError("mcmc is not supported with " + why)


def mcmc_in_window(args, iteration):
    return args.mcmc_refine_start_iter < iteration < args.mcmc_refine_stop_iter


def mcmc_refinement(iteration, scene, gaussians):
    """MCMC mode's replacement of gsplat_densification (no clone / split, no pruning, no opacity reset, no densification
    statistics): inside (mcmc_refine_start_iter, mcmc_refine_stop_iter), whenever the image counter crosses a multiple of
    mcmc_refine_every (the bsz-stride test, so no multiple is skipped), dead Gaussians are relocated onto live ones and
    the model grows by 5 % up to mcmc_cap_max.  -> whether it refined."""
    args = utils.get_args()
    gbsz = args.bsz * dp.world_size()
    if not (mcmc_in_window(args, iteration)
            and utils.check_update_at_this_iter(iteration, gbsz, args.mcmc_refine_every, 0)):
        return False
    timers = utils.get_timers()
    timers.start("densification")
    gen = getattr(gaussians, "split_generator", None)
    dead, _ = gaussians.relocate_gs(args.mcmc_min_opacity, gen)
    added = gaussians.add_new_gs(args.mcmc_cap_max, gen)
    utils.get_log_file().write("MCMC refinement: relocated {} added {}\n".format(int(dead.numel()), int(added.numel())))
    utils.inc_densify_iter()
    timers.stop("densification")
    return True


def update_densification_stats_offload_accum_grads(scene, gaussians, image_height, image_width,
                                                   send2gpu_final_filter_indices, means2d_grad,
                                                   radii):
    """densification.py:59-102 -> GaussianModel.gsplat_add_densification_stats_exact_filter."""
    args = utils.get_args()
    assert radii.shape[0] == send2gpu_final_filter_indices.shape[0] == means2d_grad.shape[0]
    if _in_window(args, utils.get_cur_iter()):
        gaussians.gsplat_add_densification_stats_exact_filter(
            means2d_grad, radii, send2gpu_final_filter_indices, image_width, image_height)


def update_densification_stats_baseline_accum_grads(scene, gaussians, image_height, image_width,
                                                    means2d_grad, radii, visibility):
    """densification.py:105-147: max_radii2D, |grad| accumulation and counts over radii > 0."""
    args = utils.get_args()
    if _in_window(args, utils.get_cur_iter()):
        densify_stats(None, means2d_grad.reshape(-1, 2), radii.reshape(-1), image_width,
                      image_height, gaussians.max_radii2D, gaussians.xyz_gradient_accum,
                      gaussians.denom, only_visible=True)
