"""Contribution pruning: what every Gaussian contributes to a set of views, and the two prune policies built on it.

The measure is the blend weight w = alpha * T of a Gaussian at a pixel -- the factor its colour enters the image with.
gsplat.rasterize_contributions (csrc/contrib.hip) walks a view's tile lists with the forward's blend rules and adds, per
Gaussian, the sum of w (Mini-Splatting / LightGaussian prune the lowest fraction by it), the maximum of w (RadSplat prunes
rows whose largest weight over all training rays stays below 0.01) and the number of pixels it reached.  score_cameras runs
that pass over a list of cameras on a model or on the tensors of a finished one; nothing here is on the training step.
"""
import math
import time
from types import SimpleNamespace

import torch

from . import dp, utils
from . import gsplat as G
from .cameras import refuse_ortho

PRUNE_MODES = ("sum", "max")
SCORE_CHUNK = 8  # cameras per visibility pass (one host read each)


class ContributionStats:
    """The three raw accumulators of n rows (gsplat.contribution_arrays): wsum_q (fixed point, unit 2^-28), wmax_bits
    (the bit pattern of a non-negative float32) and pixels.  Integer sums and a maximum: bit-reproducible, whatever the
    order of the cameras."""

    def __init__(self, n, device):
        self.wsum_q, self.wmax_bits, self.pixels = G.contribution_arrays(int(n), device)

    @property
    def raw(self):
        return self.wsum_q, self.wmax_bits, self.pixels

    def zero_(self):
        for t in self.raw:
            t.zero_()
        return self

    @property
    def wsum(self):
        return self.wsum_q.to(torch.float64) * G.WSUM_UNIT

    @property
    def wmax(self):
        return self.wmax_bits.view(torch.float32)


def lowest_fraction_mask(wsum, ratio):
    """bool mask of exactly floor(ratio * N) rows: the lowest sums, ties broken by the lower row index (a stable sort;
    torch.quantile stops at 16 M elements)."""
    ratio = float(ratio)
    if not 0.0 <= ratio <= 1.0:
        raise ValueError(f"contrib_prune_ratio must lie in [0, 1], got {ratio}")
    n = wsum.numel()
    k = min(n, int(math.floor(ratio * n)))
    mask = torch.zeros((n,), dtype=torch.bool, device=wsum.device)
    if k:
        order = torch.sort(wsum.reshape(-1), stable=True).indices
        mask[order[:k]] = True
    return mask


def below_max_mask(wmax, threshold):
    """bool mask of the rows whose largest blend weight is below `threshold` (RadSplat: 0.01)."""
    return wmax.reshape(-1) < float(threshold)


def prune_mask(stats, mode, ratio=0.3, threshold=0.01):
    if mode == "sum":
        return lowest_fraction_mask(stats.wsum, ratio)
    if mode == "max":
        return below_max_mask(stats.wmax, threshold)
    raise ValueError(f"contrib_prune_mode must be one of {PRUNE_MODES}, got {mode!r}")


def prune_iterations(args):
    its = getattr(args, "contrib_prune_iterations", None) or ()
    return tuple(int(i) for i in its)


def check_contrib_prune_args(args):
    """Contribution pruning runs on no_offload and on clm_offload (both residencies), on one GPU, after the densification
    window; every other combination is refused here, before training starts, with a message naming the flag."""
    its = prune_iterations(args)
    if not its:
        return
    mode = getattr(args, "contrib_prune_mode", "sum")
    if mode not in PRUNE_MODES:
        raise ValueError(f"contrib_prune_mode must be one of {PRUNE_MODES}, got {mode!r}")
    ratio = float(getattr(args, "contrib_prune_ratio", 0.3))
    if not 0.0 <= ratio <= 1.0:
        raise ValueError(f"contrib_prune_ratio must lie in [0, 1], got {ratio}")
    why = None
    if bool(getattr(args, "naive_offload", False)):
        why = "naive_offload: its model keeps the parameters in pinned host tables, the scoring pass reads them in HBM"
    elif dp.world_size() > 1:
        why = dp.refusal(dp.world_size(), "the scores and the row surgery are not replicated")
    elif bool(getattr(args, "mcmc", False)):
        why = "mcmc: a fixed Gaussian budget relocates dead rows instead of pruning"
    if why:
        raise ValueError("contrib_prune_iterations is not supported with " + why)
    if not bool(getattr(args, "disable_auto_densification", False)):
        early = [i for i in its if i <= int(args.densify_until_iter)]
        if early:
            raise ValueError("contrib_prune_iterations {} lie inside the densification window (densify_until_iter {}): "
                             "clone / split would regrow what the prune removes; prune after it or pass "
                             "disable_auto_densification".format(early, int(args.densify_until_iter)))


def _flush(gaussians):
    """Pending deferred steps first, as gsplat_densification does: the scores belong to the parameters an eager run holds."""
    if hasattr(gaussians, "flush_lazy_rows"):
        gaussians.flush_lazy_rows()
    elif hasattr(gaussians, "flush_small"):
        gaussians.flush_small()


@torch.no_grad()
def score_cameras(gaussians, cameras):
    """-> ContributionStats over the model's rows, accumulated over `cameras`: per camera the visibility filter, a gather
    of the selected small-attribute rows, the projection with the trainer's planes (and opacity x compensation under
    rasterize_mode "antialiased"), the binning and gsplat.rasterize_contributions(rows=filter).  Reads positions,
    opacities, scales and rotations only -- what every strategy keeps in HBM -- so SH rows are never touched and the
    result does not depend on sh_residency.  Pose refinement is seen through the poses the cameras carry; exposure,
    bilateral grid, masks and depth priors change no blend weight and are ignored.  `gaussians`: a model, or any object
    with _xyz, _opacity, _scaling, _rotation (stored parameters, device tensors)."""
    args = utils.get_args()
    for c in cameras:  # the selection kernels are pinhole ones; refused before anything is enqueued
        refuse_ortho(c, "contribution.score_cameras")
    _flush(gaussians)
    xyz, opa, sca, rot = (getattr(gaussians, a).detach() for a in ("_xyz", "_opacity", "_scaling", "_rotation"))
    if not xyz.is_cuda:
        raise ValueError("score_cameras reads the small attributes in HBM (not a naive_offload model)")
    n, dev = xyz.shape[0], xyz.device
    stats = ContributionStats(n, dev)
    W, H = int(utils.get_img_width()), int(utils.get_img_height())
    tile = 16
    tw, th = math.ceil(W / tile), math.ceil(H / tile)
    radius_clip = float(getattr(args, "radius_clip", 0.0))
    route = getattr(args, "binning", "tile")
    aa = utils.antialiased()
    if n == 0:
        return stats
    for c0 in range(0, len(cameras), SCORE_CHUNK):
        chunk = cameras[c0:c0 + SCORE_CHUNK]
        Ks = torch.stack([c.create_k_on_gpu() if getattr(c, "K", None) is None else c.K for c in chunk]).contiguous()
        vms = torch.stack([c.world_view_transform.transpose(0, 1) for c in chunk]).contiguous()
        filters, _ = G.visibility_select(xyz, rot, sca, vms, Ks, W, H, eps2d=0.3, near_plane=0.01, far_plane=1e10,
                                         radius_clip=radius_clip)
        for i, f in enumerate(filters):
            if f.numel() == 0:
                continue
            means = utils.take_rows(xyz, f)
            quats = torch.nn.functional.normalize(utils.take_rows(rot, f))
            scales = torch.exp(utils.take_rows(sca, f))
            opac = torch.sigmoid(utils.take_rows(opa, f)).reshape(1, -1)
            radii, m2, depths, conics, comps = G.fully_fused_projection(
                means, None, quats, scales, vms[i:i + 1], Ks[i:i + 1], W, H, eps2d=0.3, near_plane=0.01, far_plane=1e10,
                radius_clip=radius_clip, calc_compensations=aa)
            if comps is not None:
                opac = opac * comps
            fids, offsets, _ = G.isect_finish(G.isect_begin(route, m2, radii, depths, tile, tw, th))
            G.rasterize_contributions(m2, conics, opac.contiguous(), W, H, tile, offsets, fids, rows=f, out=stats.raw)
    return stats


def tensors_model(xyz, opacity, scaling, rotation, device="cuda"):
    """The stored small attributes of a finished model (io_ply.load_ply) as something score_cameras takes."""
    put = lambda t: t.to(device=device, dtype=torch.float32).contiguous()
    return SimpleNamespace(_xyz=put(xyz), _opacity=put(opacity).reshape(-1, 1), _scaling=put(scaling),
                           _rotation=put(rotation))


def contribution_prune(gaussians, cameras, mode="sum", ratio=0.3, threshold=0.01, resort=False, log_file=None,
                       iteration=None):
    """One scoring pass over `cameras` and one prune through the model's own prune_points(mask) -- its optimizer-state
    surgery and (resort) its Z-order re-sort.  One log line per event.  -> (rows before, rows after, pass seconds)."""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    stats = score_cameras(gaussians, cameras)
    mask = prune_mask(stats, mode, ratio, threshold)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    n0 = int(gaussians.get_xyz.shape[0])
    if int(mask.sum()):
        if getattr(gaussians, "optimizer", None) is not None:
            gaussians.optimizer.zero_grad(set_to_none=True)
        if resort:
            gaussians.prune_points(mask, resort=True)
        else:
            gaussians.prune_points(mask)
    n1 = int(gaussians.get_xyz.shape[0])
    (log_file or utils.get_log_file()).write(
        "contribution prune{}: mode {} rows {} -> {} scoring pass {:.3f} s over {} cameras\n".format(
            "" if iteration is None else " at iteration {}".format(iteration), mode, n0, n1, dt, len(cameras)))
    return n0, n1, dt
