"""Contribution pruning of a finished model:

    python -m clm_gs_amd.prune_model -m <model dir | .ply> -s <colmap dir> [--mode sum|max --ratio R --threshold T
                                     --antialiased --undistort --undistort_zoom Z] -o <out.ply>

scores the model over the scene's training cameras (contribution.score_cameras: blend weights w = alpha * T by
csrc/contrib.hip) and writes the kept rows, in their order, as a .ply (io_ply).  The scoring pass reads positions,
opacities, scales and rotations only; the SH rows stay on the host and are copied through.
"""
import argparse
import sys
import time

import torch

from . import contribution, io_ply, utils
from .render_trajectory import _find_ply


def prune_ply(ply_path, source_path, out_path, mode="sum", ratio=0.3, threshold=0.01, antialiased=False, images="images",
              resolution=1, eval=False, log=None, undistort=False, undistort_zoom=1.0):
    """-> (rows before, rows after).  `eval`: the scene's held-out split is left out of the scoring, as in training;
    `undistort`, `undistort_zoom`: as the model was trained (trainer --undistort), so that it is scored on the same cameras."""
    from .colmap_scene import load_colmap_scene
    if mode not in contribution.PRUNE_MODES:
        raise ValueError(f"--mode must be one of {contribution.PRUNE_MODES}, got {mode!r}")
    args = utils.default_args(rasterize_mode="antialiased" if antialiased else "classic")
    utils.set_args(args)
    scene = load_colmap_scene(source_path, images=images, eval=eval, resolution=resolution, device="cuda",
                              undistort=undistort, undistort_zoom=undistort_zoom)
    cams = scene.train_cameras
    sizes = {(c.image_height, c.image_width) for c in cams}
    assert len(sizes) == 1, f"all images must share one size: {sizes}"
    h, w = next(iter(sizes))
    utils.set_img_size(h, w)
    rows = io_ply.load_model(ply_path)
    model = contribution.tensors_model(rows["xyz"], rows["opacity"], rows["scaling"], rows["rotation"])
    t0 = time.perf_counter()
    stats = contribution.score_cameras(model, cams)
    mask = contribution.prune_mask(stats, mode, ratio, threshold)
    keep = (~mask).cpu()
    dt = time.perf_counter() - t0
    io_ply.save_ply(out_path, *(rows[k][keep] for k in ("xyz", "shs48", "opacity", "scaling", "rotation")))
    n0, n1 = int(keep.numel()), int(keep.sum())
    msg = "contribution prune: mode {} rows {} -> {} scoring pass {:.3f} s over {} cameras -> {}\n".format(
        mode, n0, n1, dt, len(cams), out_path)
    (log or sys.stdout).write(msg)
    return n0, n1


def main(argv=None):
    ap = argparse.ArgumentParser(description="prune a trained model by per-Gaussian blend weight over its training views")
    ap.add_argument("-m", "--model_path", required=True, help="model directory (point_cloud/iteration_*/point_cloud.ply) or a .ply")
    ap.add_argument("--iteration", type=int, default=-1)
    ap.add_argument("-s", "--source_path", required=True, help="the COLMAP directory the model was trained on")
    ap.add_argument("-i", "--images", default="images")
    ap.add_argument("-r", "--resolution", type=float, default=1)
    ap.add_argument("--eval", action="store_true", help="leave the held-out test split out of the scoring")
    ap.add_argument("--mode", choices=list(contribution.PRUNE_MODES), default="sum")
    ap.add_argument("--ratio", type=float, default=0.3, help="--mode sum: the fraction of rows pruned, lowest summed weight first")
    ap.add_argument("--threshold", type=float, default=0.01, help="--mode max: rows whose largest weight is below it are pruned")
    ap.add_argument("--antialiased", action="store_true", help="for a model trained with trainer --antialiased")
    ap.add_argument("--undistort", action="store_true", help="for a model trained with trainer --undistort")
    ap.add_argument("--undistort_zoom", type=float, default=1.0, help="--undistort: the trainer's --undistort_zoom")
    ap.add_argument("-o", "--output", required=True, help="the pruned .ply")
    a = ap.parse_args(argv)
    with torch.no_grad():
        prune_ply(_find_ply(a.model_path, a.iteration), a.source_path, a.output, a.mode, a.ratio, a.threshold,
                  a.antialiased, a.images, a.resolution, a.eval, undistort=a.undistort, undistort_zoom=a.undistort_zoom)
    return 0


if __name__ == "__main__":
    sys.exit(main())
