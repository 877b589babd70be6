"""Mesh export of a finished model ("Mesh export"):

    python -m clm_gs_amd.mesh_model -m <model dir | .ply | .vq.npz> -s <colmap dir> -o <mesh.ply> --voxel V
        [--trunc_voxels 4] [--bounds emin nmin umin emax nmax umax] [--up X Y Z] [--east X Y Z] [--every K] [-r R]
        [--alpha_min 0.5] [--depth_max D] [--min_weight 2] [--grid_gb 16] [--antialiased] [--undistort --undistort_zoom Z]
        [--depth_mode expected|median|ray] [--min_component_faces N] [--keep_components K] [--sparse] [--decimate_cell C]
        [--smooth_iterations N --smooth_lambda 0.5 --smooth_mu -0.53] [--normals] [--eval]
        [--reference REF.ply --eval_tau T [T ...] --eval_spacing S --eval_max_distance D]
        [--clm_offload | --naive_offload | --no_offload]

renders every selected training camera of the scene through the strategy's own eval entry (render_mode "RGB+ED":
expected depth and alpha), fuses the depth maps into a dense TSDF volume in the map frame of render_ortho (tsdf.TsdfVolume,
csrc/tsdf.hip), extracts the surface by naive Surface Nets and writes the coloured triangle mesh (io_ply.save_mesh_ply)
and, next to it, <mesh>.json: frame, bounds, voxel, truncation, grid, counts and the cameras used.  --bounds default: the
1st to 99th percentile box of the rows in the map frame.  A non-positive --voxel, inverted --bounds and a grid above
--grid_gb or 2^31 voxels are refused by name (with the voxel size that fits) before anything is loaded or written.
--depth_mode median fuses the median depth (render_mode "RGB+MD": the depth of the Gaussian at which the transmittance
falls through one half; DESIGN.md section 3, "Median depth") instead of the expected depth, which a translucent layer in
front of a surface pulls forward; the .json then carries "depth_mode": "median".  --depth_mode ray fuses the ray depth (render_mode
"RGB+RD": per pixel the depth at which that same Gaussian's 3-D density peaks along the pixel's ray, not the depth of its
centre, which turns an obliquely seen flat splat into a fronto-parallel step; DESIGN.md section 3, "Ray depth"); the .json
then carries "depth_mode": "ray".  An unknown mode is refused by name.
--min_component_faces N and --keep_components K drop the small connected components of the extracted mesh on the device
before it is written (mesh_clean.clean; DESIGN.md section 3, "Mesh cleanup"): those with fewer than N faces, and all but
the K with the most faces; the .json then carries "cleanup" (the options and the report) and the log line the component
counts.  Negative values are refused by name.  Without either flag nothing changes.
--sparse stores the volume in bricks of 8 x 8 x 8 voxels allocated only where some camera's depth map can put a surface
(tsdf.SparseTsdfVolume, csrc/tsdf_sparse.hip; DESIGN.md section 3, "Sparse volume"): the cameras are rendered twice, once to
mark the bricks and once to fuse, and mesh.ply is byte for byte the file the dense volume writes wherever that fits; the
dense limits (2^31 voxels, 24 B per voxel under --grid_gb) give way to a brick grid of at most 2^30 bricks, 2^31 STORED
voxels and marks + table + pool under --grid_gb.  The .json gains "sparse" and the log line the brick counts, the pool's GB
and the marking rate.  Without the flag every file is what it was.
--decimate_cell C merges, after the cleanup, the vertices of every cell of C world units into one, placed by the quadric of
the faces that touch the cell (mesh_decimate.decimate, csrc/mesh_decimate.hip; DESIGN.md section 3, "Mesh decimation"); the
.json gains "decimation" (the report) and the log line " decimated V -> V' vertices F -> F' faces cell C".  A negative or
non-finite value is refused by name; 0, the default, changes nothing.  The decimated mesh need not be a manifold.
--smooth_iterations N runs, between the cleanup and the decimation, N passes of Taubin's lambda | mu smoothing
(mesh_smooth.smooth, csrc/mesh_smooth.hip; DESIGN.md section 3, "Mesh smoothing and normals"): a step with --smooth_lambda
(0.5), then one with --smooth_mu (-0.53; 0 = plain Laplacian smoothing, which shrinks).  Vertex count, colours and faces
stay; the decimation's quadrics then see denoised faces.  --normals writes the area-weighted vertex normals of the FINAL
mesh into the file (x y z nx ny nz red green blue).  The .json gains "smoothing" (the report) and "normals": true, the
log line " smoothed N x (lam, mu)" and " normals", each only with its flag; without them every file is what it was.
--reference REF.ply --eval_tau T [T ...] evaluates the final mesh, after it is written, against a reference scan or mesh in
the same frame (mesh_eval.evaluate, csrc/mesh_distance.hip; DESIGN.md section 3, "Mesh evaluation"): accuracy, completeness,
chamfer distance and precision / recall / F-score per tau, with --eval_spacing (the smallest tau / 2) and
--eval_max_distance (10 x the largest tau).  The .json gains "evaluation" (the report) and the log line " F <F>@tau <T>" per
tau; mesh.ply is the file it was.  One of --reference and --eval_tau without the other, and a bad value, are refused by
name before anything is loaded.
"""
import argparse
import json
import os
import sys
import time

import torch

from . import io_ply, mesh_clean, mesh_decimate, mesh_eval, mesh_smooth, tsdf, utils
from .render_ortho import map_frame, percentile_sorted
from .render_trajectory import _find_ply, depth_render_mode, eval_one_cam


def percentile_box(means, frame, lo=1.0, hi=99.0):
    """(emin, nmin, umin, emax, nmax, umax): the lo-th to hi-th percentile of the rows along the three axes of the frame."""
    if means.shape[0] == 0:
        raise ValueError("percentile bounds of an empty model")
    los, his = [], []
    for axis in frame:
        coord = torch.sort(means.detach().float() @ torch.as_tensor(axis, dtype=torch.float32, device=means.device)).values
        los.append(percentile_sorted(coord, lo))
        his.append(percentile_sorted(coord, hi))
    return tuple(los + his)


def json_path(mesh_path):
    return os.path.splitext(mesh_path)[0] + ".json"


@torch.no_grad()
def build_mesh(gaussians, cameras, args, out_path, voxel, frame=None, bounds=None, trunc_voxels=4.0, every=1, alpha_min=0.5,
               depth_max=None, min_weight=2.0, grid_gb=16.0, near=0.01, background=None, log=None, depth_mode="expected",
               min_component_faces=0, keep_components=0, sparse=False, decimate_cell=0.0, smooth_iterations=0,
               smooth_lambda=0.5, smooth_mu=-0.53, normals=False, reference=None, eval_taus=None, eval_spacing=None,
               eval_max_distance=None):
    """Renders cameras[::every] from `gaussians` through the eval entry of the strategy `args` names, fuses them, extracts
    and writes out_path and its .json.  -> the dict written to the .json.  The global image size (utils.set_img_size)
    must be the cameras' size.  depth_mode "expected" fuses the "RGB+ED" depth, "median" the "RGB+MD" one, "ray" the "RGB+RD"
    one (the .json gains "depth_mode" only with these two).  min_component_faces / keep_components: mesh_clean.clean
    between the extraction and the file (the .json gains "cleanup" and the log line its component counts only when one of them is on).  sparse: the
    brick-allocated volume; every camera is rendered twice, to mark and to fuse (the eval forward is deterministic: see
    DESIGN.md section 3, "Sparse volume"), and the .json gains "sparse".  decimate_cell: mesh_decimate.decimate after the
    cleanup, which sees the full-resolution mesh (the .json gains "decimation" and the log line its counts only when it is
    on).  smooth_iterations / smooth_lambda / smooth_mu: mesh_smooth.smooth between the cleanup and the decimation;
    normals: the vertex normals of the final mesh in the file (the .json gains "smoothing" / "normals" and the log line
    its words only then).  reference (a .ply path) with eval_taus: mesh_eval.evaluate of the final mesh against it, after
    the mesh is written (the .json gains "evaluation" and the log line " F <F>@tau <T>" only then)."""
    check_eval_options(reference, eval_taus, eval_spacing, eval_max_distance)
    decimate_cell = mesh_decimate.check_cell(decimate_cell)
    smooth_iterations, smooth_lambda, smooth_mu = mesh_smooth.check_options(smooth_iterations, smooth_lambda, smooth_mu)
    min_component_faces, keep_components = mesh_clean.check_options(min_component_faces, keep_components,
                                                                    ("--min_component_faces", "--keep_components"))
    render_mode = depth_render_mode(depth_mode)
    log = log or sys.stdout
    frame = frame if frame is not None else map_frame()
    if bounds is None:
        bounds = percentile_box(gaussians.get_xyz.detach().to("cuda"), frame)
    cams = list(cameras)[::max(1, int(every))]
    if not cams:
        raise ValueError("mesh export: no camera selected")
    depth_max = float("inf") if depth_max is None else float(depth_max)
    t_render = t_fuse = t_mark = 0.0
    if sparse:  # pass 1: the union of the bricks every camera can put a surface into, before any sum is formed
        volume = tsdf.SparseTsdfVolume(frame, bounds, voxel, trunc_voxels, device="cuda", grid_gb=grid_gb)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for cam in cams:
            _, depth, alpha = eval_one_cam(cam, gaussians, background, args, None, render_mode=render_mode)
            volume.mark(cam, depth, alpha, near=near, depth_max=depth_max, alpha_min=alpha_min)
        volume.allocate()
        torch.cuda.synchronize()
        t_mark = time.perf_counter() - t0
    else:
        volume = tsdf.TsdfVolume(frame, bounds, voxel, trunc_voxels, device="cuda", grid_gb=grid_gb)
    for cam in cams:
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        image, depth, alpha = eval_one_cam(cam, gaussians, background, args, None, render_mode=render_mode)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        volume.add(cam, image, depth, alpha, near=near, depth_max=depth_max, alpha_min=alpha_min)
        torch.cuda.synchronize()
        t_render, t_fuse = t_render + (t1 - t0), t_fuse + (time.perf_counter() - t1)
    t1 = time.perf_counter()
    volume.flush()
    torch.cuda.synchronize()
    t_fuse += time.perf_counter() - t1
    t0 = time.perf_counter()
    verts, colours, faces = volume.extract(min_weight)
    torch.cuda.synchronize()
    t_extract = time.perf_counter() - t0
    verts, colours, faces, report = mesh_clean.clean(verts, colours, faces, min_component_faces, keep_components)
    verts, colours, faces, smoothing = mesh_smooth.smooth(verts, colours, faces, smooth_iterations, smooth_lambda, smooth_mu)
    verts, colours, faces, decimation = mesh_decimate.decimate(verts, colours, faces, decimate_cell)
    vertex_normals = mesh_smooth.vertex_normals(verts, faces) if normals else None
    d = os.path.dirname(out_path)
    if d:
        os.makedirs(d, exist_ok=True)
    io_ply.save_mesh_ply(out_path, verts, colours, faces, vertex_normals)
    e, n, u = volume.frame
    meta = dict(east=[float(v) for v in e], north=[float(v) for v in n], up=[float(v) for v in u],
                bounds=[float(v) for v in volume.bounds], voxel=volume.voxel, trunc=volume.trunc,
                grid=[volume.nx, volume.ny, volume.nz], min_weight=float(min_weight), alpha_min=float(alpha_min),
                depth_max=None if depth_max == float("inf") else depth_max, vertices=int(verts.shape[0]),
                faces=int(faces.shape[0]), cameras=len(cams), camera_names=[str(c.image_name) for c in cams])
    if depth_mode in ("median", "ray"):
        meta["depth_mode"] = depth_mode
    if sparse:
        meta["sparse"] = dict(bricks=volume.S, bricks_total=volume.bricks_total, pool_gb=volume.S * tsdf.BYTES_PER_BRICK / 1e9)
    if report is not None:
        meta = mesh_clean.json_record(meta, min_component_faces, keep_components, report, verts.shape[0], faces.shape[0])
    if decimation is not None:
        meta = mesh_decimate.json_record(meta, decimation, verts.shape[0], faces.shape[0])
    meta = mesh_smooth.json_record(meta, smoothing, bool(normals))
    evaluation = None
    if reference is not None:
        ref_points, ref_faces = mesh_eval.load_reference(reference, verts.device)
        evaluation = mesh_eval.evaluate(verts, faces, ref_points, ref_faces, eval_taus, eval_spacing, eval_max_distance,
                                        names=mesh_eval.MODEL_NAMES)
        meta = mesh_eval.json_record(meta, evaluation)
    with open(json_path(out_path), "w") as f:
        json.dump(meta, f, indent=1)
    log.write("mesh export: grid {} x {} x {} voxel {:g} cameras {} render {:.1f} cameras/s integration {:.1f} cameras/s "
              "extraction {:.3f} s vertices {} faces {}{}{}{}{}{} -> {}\n".format(
                  volume.nx, volume.ny, volume.nz, volume.voxel, len(cams), len(cams) / max(t_render, 1e-9),
                  len(cams) / max(t_fuse, 1e-9), t_extract, meta["vertices"], meta["faces"],
                  "" if report is None else " components {} kept {}".format(report["components"], report["components_kept"]),
                  "" if not sparse else " sparse bricks {} of {} pool {:.3f} GB marking {:.1f} cameras/s".format(
                      volume.S, volume.bricks_total, meta["sparse"]["pool_gb"], len(cams) / max(t_mark, 1e-9)),
                  "" if decimation is None else mesh_decimate.log_words(decimation),
                  mesh_smooth.log_words(smoothing, bool(normals)), mesh_eval.log_words(evaluation),
                  out_path))
    return meta


def check_eval_options(reference=None, eval_taus=None, eval_spacing=None, eval_max_distance=None):
    """--reference and --eval_tau come together; the values are mesh_eval.check_options' (ValueError by name)."""
    if reference is None and eval_taus is None:
        if eval_spacing is not None or eval_max_distance is not None:
            raise ValueError("--eval_spacing and --eval_max_distance have effect only with --reference and --eval_tau")
        return
    if reference is None or eval_taus is None:
        raise ValueError("--reference and --eval_tau come together: give both, or neither")
    mesh_eval.check_options(eval_taus, eval_spacing, eval_max_distance, names=mesh_eval.MODEL_NAMES)


def check_options(voxel, bounds=None, grid_gb=16.0, trunc_voxels=4.0, min_weight=2.0, every=1, depth_mode="expected",
                  min_component_faces=0, keep_components=0, sparse=False, decimate_cell=0.0, smooth_iterations=0,
                  smooth_lambda=0.5, smooth_mu=-0.53, reference=None, eval_taus=None, eval_spacing=None, eval_max_distance=None):
    """The refusals that need nothing loaded (ValueError by name); with sparse the brick-grid limits take the place of the
    dense ones."""
    mesh_clean.check_options(min_component_faces, keep_components, ("--min_component_faces", "--keep_components"))
    mesh_decimate.check_cell(decimate_cell)
    mesh_smooth.check_options(smooth_iterations, smooth_lambda, smooth_mu)
    check_eval_options(reference, eval_taus, eval_spacing, eval_max_distance)
    tsdf.grid_shape((0, 0, 0, 1, 1, 1), voxel)  # (--voxel alone)
    depth_render_mode(depth_mode)
    if not trunc_voxels > 0:
        raise ValueError(f"--trunc_voxels must be positive, got {trunc_voxels}")
    if not min_weight > 0:
        raise ValueError(f"--min_weight must be positive, got {min_weight}")
    if int(every) < 1:
        raise ValueError(f"--every must be >= 1, got {every}")
    if not grid_gb > 0:
        raise ValueError(f"--grid_gb must be positive, got {grid_gb}")
    if bounds is not None:
        (tsdf.check_brick_grid if sparse else tsdf.check_grid)(bounds, voxel, grid_gb)


def main(argv=None):
    ap = argparse.ArgumentParser(description="triangle mesh of a trained model: TSDF fusion of its rendered depth maps")
    ap.add_argument("-m", "--model_path", required=True, help="model directory (point_cloud/iteration_*/point_cloud.ply), a .ply or a compressed .npz")
    ap.add_argument("--iteration", type=int, default=-1)
    ap.add_argument("-s", "--source_path", required=True, help="the COLMAP directory whose training cameras are rendered")
    ap.add_argument("-i", "--images", default="images")
    ap.add_argument("-r", "--resolution", type=float, default=1)
    ap.add_argument("-o", "--output", required=True, help="the mesh (.ply); <output without .ply>.json is written next to it")
    ap.add_argument("--voxel", type=float, required=True, help="voxel size in world units")
    ap.add_argument("--trunc_voxels", type=float, default=4.0, help="truncation distance in voxels")
    ap.add_argument("--bounds", type=float, nargs=6, default=None, metavar=("EMIN", "NMIN", "UMIN", "EMAX", "NMAX", "UMAX"),
                    help="map coordinates; default: 1st to 99th percentile box of the rows")
    ap.add_argument("--up", type=float, nargs=3, default=(0.0, 0.0, 1.0), metavar=("X", "Y", "Z"))
    ap.add_argument("--east", type=float, nargs=3, default=(1.0, 0.0, 0.0), metavar=("X", "Y", "Z"))
    ap.add_argument("--every", type=int, default=1, metavar="K", help="use every K-th training camera")
    ap.add_argument("--alpha_min", type=float, default=0.5, help="pixels below this opacity are not fused")
    ap.add_argument("--depth_max", type=float, default=None, help="pixels deeper than this are not fused")
    ap.add_argument("--min_weight", type=float, default=2.0, help="a voxel counts when at least this many cameras observed it")
    ap.add_argument("--grid_gb", type=float, default=16.0, help="the largest grid allocated (24 B per voxel)")
    ap.add_argument("--depth_mode", default="expected", metavar="expected|median|ray",
                    help="the depth map fused: the expected depth D / alpha, the ray depth (where the median Gaussian's "
                         "density peaks along the pixel's ray), or the median depth (the Gaussian at which "
                         "the transmittance falls through one half)")
    ap.add_argument("--min_component_faces", type=int, default=0, metavar="N",
                    help="drop the connected components of the mesh with fewer than N faces")
    ap.add_argument("--keep_components", type=int, default=0, metavar="K",
                    help="keep only the K connected components with the most faces")
    ap.add_argument("--decimate_cell", type=float, default=0.0, metavar="C",
                    help="decimate the mesh before it is written: merge the vertices of every cell of C world units "
                         "(quadric vertex clustering, after the cleanup); 0 = off")
    ap.add_argument("--smooth_iterations", type=int, default=0, metavar="N",
                    help="smooth the mesh before the decimation: N passes of Taubin's lambda | mu smoothing; 0 = off")
    ap.add_argument("--smooth_lambda", type=float, default=0.5, metavar="L", help="the factor of a pass's first step, in (0, 1]")
    ap.add_argument("--smooth_mu", type=float, default=-0.53, metavar="M",
                    help="the factor of a pass's second step, in [-1, 0]; 0 = plain Laplacian smoothing")
    ap.add_argument("--normals", action="store_true",
                    help="write area-weighted vertex normals of the final mesh (nx ny nz) into the file")
    ap.add_argument("--reference", default=None, metavar="PLY",
                    help="evaluate the final mesh against this reference scan or mesh (same frame); needs --eval_tau")
    ap.add_argument("--eval_tau", type=float, nargs="+", default=None, metavar="T", help="the distance thresholds of the F-score")
    ap.add_argument("--eval_spacing", type=float, default=None, metavar="S",
                    help="the sampling distance of the evaluation (default: the smallest tau / 2)")
    ap.add_argument("--eval_max_distance", type=float, default=None, metavar="D",
                    help="distances are capped here (default: 10 x the largest tau)")
    ap.add_argument("--sparse", action="store_true",
                    help="a brick-allocated volume: the same mesh.ply, on boxes far beyond 2^31 voxels (renders every camera twice)")
    ap.add_argument("--antialiased", action="store_true", help="for a model trained with trainer --antialiased")
    ap.add_argument("--undistort", action="store_true", help="for a model trained with trainer --undistort")
    ap.add_argument("--undistort_zoom", type=float, default=1.0, help="--undistort: the trainer's --undistort_zoom")
    ap.add_argument("--eval", action="store_true", help="leave the held-out test split out, as in training")
    g = ap.add_mutually_exclusive_group()
    g.add_argument("--clm_offload", action="store_true")
    g.add_argument("--naive_offload", action="store_true")
    g.add_argument("--no_offload", action="store_true")
    a = ap.parse_args(argv)
    try:  # refusals before anything is loaded or written
        check_options(a.voxel, a.bounds, a.grid_gb, a.trunc_voxels, a.min_weight, a.every, a.depth_mode,
                      a.min_component_faces, a.keep_components, a.sparse, a.decimate_cell, a.smooth_iterations,
                      a.smooth_lambda, a.smooth_mu, a.reference, a.eval_tau, a.eval_spacing, a.eval_max_distance)
        frame = map_frame(a.up, a.east)
    except ValueError as e:
        raise SystemExit(str(e))
    if not (a.clm_offload or a.naive_offload or a.no_offload):
        a.clm_offload = True
    from .colmap_scene import load_colmap_scene
    args = utils.default_args(bsz=4, rasterize_mode="antialiased" if a.antialiased else "classic")
    for k in ("clm_offload", "naive_offload", "no_offload"):
        setattr(args, k, getattr(a, k))
    utils.set_args(args)
    scene = load_colmap_scene(a.source_path, images=a.images, eval=a.eval, resolution=a.resolution, device="cuda",
                              load_images=False, undistort=a.undistort, undistort_zoom=a.undistort_zoom)
    cams = scene.train_cameras
    sizes = {(c.image_height, c.image_width) for c in cams}
    if len(sizes) != 1:
        raise SystemExit(f"all images must share one size: {sizes}")
    utils.set_img_size(*next(iter(sizes)))
    if a.clm_offload:
        from .strategies.clm_offload import GaussianModelCLMOffload as M
    elif a.naive_offload:
        from .strategies.naive_offload import GaussianModelNaiveOffload as M
    else:
        from .strategies.no_offload import GaussianModelNoOffload as M
    gaussians = M(3, only_for_rendering=True)
    gaussians.load_ply(_find_ply(a.model_path, a.iteration))
    gaussians.active_sh_degree = gaussians.max_sh_degree
    try:
        build_mesh(gaussians, cams, args, a.output, a.voxel, frame, a.bounds, a.trunc_voxels, a.every, a.alpha_min,
                   a.depth_max, a.min_weight, a.grid_gb, depth_mode=a.depth_mode,
                   min_component_faces=a.min_component_faces, keep_components=a.keep_components, sparse=a.sparse,
                   decimate_cell=a.decimate_cell, smooth_iterations=a.smooth_iterations, smooth_lambda=a.smooth_lambda,
                   smooth_mu=a.smooth_mu, normals=a.normals, reference=a.reference, eval_taus=a.eval_tau,
                   eval_spacing=a.eval_spacing, eval_max_distance=a.eval_max_distance)
    except ValueError as e:  # (the size of a grid whose bounds come from the model)
        raise SystemExit(str(e))
    return 0


if __name__ == "__main__":
    sys.exit(main())
