"""Compressed export of a finished model ("Compressed models"):

    python -m clm_gs_amd.compress_model -m <model dir | .ply> -o <out.vq.npz> [--codebook 65536 --iters 10
                                        --sample 4194304 --pos_bits 16 --scale_bits 8 --opacity_bits 8 --rot_bits 8
                                        --dc_bits 8] [--decompress <out.ply>]
                                        [-s <colmap dir> [--eval --antialiased --undistort --undistort_zoom Z]]

writes the .npz (compress.save_compressed) and logs one line: rows, bytes before and after, K, empty centroids, mean
distortion.  --decompress also writes the dequantised model back as a plain .ply (rows in Morton order).  With -s the
scene's cameras (the held-out split with --eval, else the training cameras) are rendered from the original and from the
decompressed model through the no_offload eval entry, and the line gains three PSNRs: original against ground truth,
compressed against ground truth, compressed against original.  Every tool that loads a model takes the .npz wherever
it takes a .ply (io_ply.load_model).
"""
import argparse
import os
import sys
import time

import torch

from . import compress, io_ply, utils
from .render_trajectory import _find_ply, eval_one_cam


def _psnr(a, b):
    mse = float(((a - b) ** 2).mean())
    return float("inf") if mse == 0 else -10.0 * torch.log10(torch.tensor(mse)).item()


@torch.no_grad()
def scene_psnr(rows_a, rows_b, source_path, images="images", resolution=1, eval=False, antialiased=False,
               undistort=False, undistort_zoom=1.0):
    """Mean PSNR over the scene's cameras of (model a vs ground truth, model b vs ground truth, b vs a); the models are
    built the way render_trajectory builds its model and rendered through the no_offload eval entry."""
    from .colmap_scene import load_colmap_scene
    from .strategies.no_offload import GaussianModelNoOffload as M
    args = utils.default_args(bsz=1, rasterize_mode="antialiased" if antialiased else "classic")
    args.no_offload, args.clm_offload, args.naive_offload = True, False, False
    utils.set_args(args)
    scene = load_colmap_scene(source_path, images=images, eval=eval, resolution=resolution, device="cuda",
                              undistort=undistort, undistort_zoom=undistort_zoom)
    cams = scene.test_cameras if eval and scene.test_cameras else scene.train_cameras
    sizes = {(c.image_height, c.image_width) for c in cams}
    assert len(sizes) == 1, f"all images must share one size: {sizes}"
    utils.set_img_size(*next(iter(sizes)))
    models = []
    for rows in (rows_a, rows_b):
        g = M(3, only_for_rendering=True)
        g.create_from_tensors(rows["xyz"], rows["shs48"], rows["scaling"], rows["rotation"], rows["opacity"], 1.0)
        g.active_sh_degree = g.max_sh_degree
        models.append(g)
    sums = [0.0, 0.0, 0.0]
    for cam in cams:
        gt = torch.clamp(cam.original_image.float() / 255.0, 0.0, 1.0)
        ia, ib = (torch.clamp(eval_one_cam(cam, g, None, args), 0.0, 1.0) for g in models)
        for k, (x, y) in enumerate(((ia, gt), (ib, gt), (ib, ia))):
            sums[k] += _psnr(x, y)
    return tuple(s / max(1, len(cams)) for s in sums)


def compress_file(model_file, out_path, K=65536, iters=10, sample=1 << 22, bits=None, decompress_to=None,
                  source_path=None, log=None, **scene_kw):
    """-> (meta, bytes after).  One log line (compress.size_line, plus the PSNRs with a scene)."""
    log = log or sys.stdout
    rows = io_ply.load_model(model_file)
    timings = {}
    arrays, meta = compress.compress(rows, K=K, iters=iters, sample=sample, bits=bits, timings=timings)
    t0 = time.perf_counter()
    compress.save_compressed(out_path, arrays, meta)
    timings["write_s"] = time.perf_counter() - t0
    after = os.path.getsize(out_path)
    line = compress.size_line(meta, after)
    back = None
    if decompress_to or source_path:
        back = compress.load_compressed(out_path)
    if decompress_to:
        io_ply.save_ply(decompress_to, *(back[k] for k in ("xyz", "shs48", "opacity", "scaling", "rotation")))
    if source_path:
        p = scene_psnr(rows, back, source_path, **scene_kw)
        line += " PSNR original/gt {:.3f} compressed/gt {:.3f} compressed/original {:.3f}".format(*p)
    line += " (fit {fit_s:.2f} s, assignment {assign_s:.2f} s, quantisation {quantise_s:.2f} s, write {write_s:.2f} s)".format(
        **timings)
    log.write(line + " -> " + out_path + "\n")
    return meta, after


def main(argv=None):
    ap = argparse.ArgumentParser(description="compress a trained model: SH vector quantisation + quantised attributes")
    ap.add_argument("-m", "--model_path", required=True, help="model directory (point_cloud/iteration_*/point_cloud.ply) or a .ply")
    ap.add_argument("--iteration", type=int, default=-1)
    ap.add_argument("-o", "--output", required=True, help="the compressed model (.vq.npz)")
    ap.add_argument("--codebook", type=int, default=65536, help="number of SH centroids K (<= 65536)")
    ap.add_argument("--iters", type=int, default=10, help="Lloyd iterations of the codebook fit")
    ap.add_argument("--sample", type=int, default=1 << 22, help="rows the codebook is fitted on")
    for k, v in compress.BITS.items():  # the trainer has the same knobs, prefixed compress_
        ap.add_argument(f"--{k}", type=int, default=v)
    ap.add_argument("--decompress", default=None, metavar="PLY", help="also write the dequantised model as a plain .ply")
    ap.add_argument("-s", "--source_path", default=None, help="a COLMAP directory: report PSNR before / after over its cameras")
    ap.add_argument("-i", "--images", default="images")
    ap.add_argument("-r", "--resolution", type=float, default=1)
    ap.add_argument("--eval", action="store_true", help="-s: measure on the held-out test split")
    ap.add_argument("--antialiased", action="store_true", help="for a model trained with trainer --antialiased")
    ap.add_argument("--undistort", action="store_true", help="for a model trained with trainer --undistort")
    ap.add_argument("--undistort_zoom", type=float, default=1.0, help="--undistort: the trainer's --undistort_zoom")
    a = ap.parse_args(argv)
    if not a.output.endswith(".npz"):
        raise SystemExit(f"-o {a.output}: a compressed model is a .npz (io_ply.load_model goes by the extension)")
    bits = compress.check_bits({k: getattr(a, k) for k in compress.BITS})
    compress_file(_find_ply(a.model_path, a.iteration), a.output, a.codebook, a.iters, a.sample, bits, a.decompress,
                  a.source_path, images=a.images, resolution=a.resolution, eval=a.eval, antialiased=a.antialiased,
                  undistort=a.undistort, undistort_zoom=a.undistort_zoom)
    return 0


if __name__ == "__main__":
    sys.exit(main())
