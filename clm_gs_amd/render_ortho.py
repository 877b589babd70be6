"""Orthophoto and height-map export: a trained model (any of the three strategies) rendered top-down through
orthographic cameras (cameras.OrthoCamera, gsplat's camera_model="ortho") -- one ground-sampling distance everywhere, no
perspective lean -- with the matching elevation raster.

    python -m clm_gs_amd.render_ortho -m <model dir | .ply> --clm_offload --gsd 0.05 [--bounds emin nmin emax nmax]
        [--up X Y Z] [--east X Y Z] [--camera_height H] [--tile 4096] [--output_dir DIR] [--antialiased] [--white_background]
        [--depth_mode expected|median|ray]

Map frame: u = --up (default 0 0 1), e = --east projected onto the plane perpendicular to u (default 1 0 0; 0 1 0 if that
is parallel to u), n = u x e.  The camera's rows are x = e, y = -n, z = -u: it looks straight down and image row 0 is
north.  Pixel centre (c, r) is the world point  origin + (c + 0.5) gsd e - (r + 0.5) gsd n  (at height 0 along u).

The map is rendered in windows of at most --tile x --tile pixels whose origins are multiples of 16, each through the
strategy's own eval entry with render_mode "RGB+ED", and assembled on the host: every Gaussian meets the same 16x16
raster tiles as in a one-shot render, so seams differ by the rounding of sx * x + cx only.

Outputs in --output_dir: ortho.png (8-bit RGB), ortho_height.npy (float32 [H,W]: camera_height - expected depth, NaN
where alpha < 0.5), ortho_alpha.npy (float32 [H,W]) and ortho.json (origin, east, north, up, gsd, width, height,
camera_height).  --depth_mode median: the height map is camera_height - median depth (render_mode "RGB+MD": the depth of
the Gaussian at which the transmittance falls through one half, which a translucent layer above the ground does not pull
up) under the same alpha < 0.5 -> NaN rule, and ortho.json gains "depth_mode": "median".  --depth_mode ray: camera_height -
ray depth (render_mode "RGB+RD": the depth at which that same Gaussian's 3-D density peaks along the pixel's vertical ray,
so a tilted flat splat gives a slope, not a terrace) under the same rule; ortho.json gains "depth_mode": "ray"."""
import argparse
import json
import math
import os
import sys

import numpy as np
import torch

from . import utils
from .cameras import OrthoCamera
from .render_trajectory import _find_ply, depth_render_mode, eval_one_cam, write_png

RASTER_TILE = 16
JSON_FIELDS = ("origin", "east", "north", "up", "gsd", "width", "height", "camera_height")


# ------------------------------------------------------------------------------------------------ map frame
def map_frame(up=(0.0, 0.0, 1.0), east=(1.0, 0.0, 0.0)):
    """-> (e, n, u): float64 unit vectors, orthonormal and right-handed (e x n = u).  `east` is projected onto the plane
    perpendicular to `up`; one that is parallel to it is replaced by 0 1 0 (and that, if parallel too, by 1 0 0)."""
    u = np.asarray(up, dtype=np.float64)
    if not np.isfinite(u).all() or np.linalg.norm(u) == 0.0:
        raise ValueError(f"--up must be a non-zero vector, got {up}")
    u = u / np.linalg.norm(u)
    for cand in (east, (0.0, 1.0, 0.0), (1.0, 0.0, 0.0)):
        c = np.asarray(cand, dtype=np.float64)
        nc = np.linalg.norm(c)
        if not np.isfinite(c).all() or nc == 0.0:
            continue
        e = c / nc - np.dot(c / nc, u) * u
        if np.linalg.norm(e) > 1e-6:
            e = e / np.linalg.norm(e)
            return e, np.cross(u, e), u
    raise ValueError(f"no east direction perpendicular to up={up}")


def world_to_cam(frame, camera_height):
    """The 4x4 world->camera matrix of the map's camera: rows e, -n, -u, sitting camera_height up the u axis, so that
    p = (e.m, -n.m, camera_height - u.m)."""
    e, n, u = frame
    w2c = np.eye(4)
    w2c[:3, :3] = np.stack([e, -n, -u])
    w2c[:3, 3] = (0.0, 0.0, float(camera_height))
    return w2c


class MapGeometry:
    """The raster of a map: frame (e, n, u), bounds (emin, nmin, emax, nmax) in map coordinates, gsd (world units per
    pixel) and camera_height.  width / height cover the bounds; the top-left pixel corner is (emin, nmax)."""

    def __init__(self, frame, bounds, gsd, camera_height):
        self.frame = tuple(np.asarray(v, dtype=np.float64) for v in frame)
        emin, nmin, emax, nmax = (float(v) for v in bounds)
        if not (emax > emin and nmax > nmin):
            raise ValueError(f"--bounds must be emin nmin emax nmax with emax > emin and nmax > nmin, got {bounds}")
        if not (gsd > 0 and math.isfinite(gsd)):
            raise ValueError(f"--gsd must be positive, got {gsd}")
        self.bounds, self.gsd, self.camera_height = (emin, nmin, emax, nmax), float(gsd), float(camera_height)
        self.width = max(1, int(math.ceil((emax - emin) / self.gsd - 1e-9)))
        self.height = max(1, int(math.ceil((nmax - nmin) / self.gsd - 1e-9)))

    @property
    def origin(self):
        """World point of the top-left pixel corner at height 0."""
        e, n, _ = self.frame
        return self.bounds[0] * e + self.bounds[3] * n

    def principal_point(self):
        """(cx, cy) of the whole map's orthographic camera: px = e.m / gsd + cx, py = -n.m / gsd + cy."""
        return -self.bounds[0] / self.gsd, self.bounds[3] / self.gsd

    def pixel_to_world(self, c, r, height=0.0):
        e, n, u = self.frame
        return self.origin + (c + 0.5) * self.gsd * e - (r + 0.5) * self.gsd * n + height * u

    def camera(self, x0=0, y0=0, width=None, height=None, uid=0, device="cuda"):
        """The OrthoCamera of the window whose top-left pixel is (x0, y0): the map's camera with its principal point
        shifted by the window's origin."""
        cx, cy = self.principal_point()
        return OrthoCamera(uid, torch.from_numpy(world_to_cam(self.frame, self.camera_height)).float(), 1.0 / self.gsd,
                           self.width if width is None else width, self.height if height is None else height,
                           cx=cx - x0, cy=cy - y0, image_name=f"ortho_window_{x0}_{y0}", device=device)

    def to_json(self):
        e, n, u = self.frame
        return dict(origin=[float(v) for v in self.origin], east=[float(v) for v in e], north=[float(v) for v in n],
                    up=[float(v) for v in u], gsd=self.gsd, width=self.width, height=self.height,
                    camera_height=self.camera_height)

    @classmethod
    def from_json(cls, d):
        e, n, u = (np.asarray(d[k], dtype=np.float64) for k in ("east", "north", "up"))
        o = np.asarray(d["origin"], dtype=np.float64)
        emin, nmax = float(np.dot(o, e)), float(np.dot(o, n))
        g = cls((e, n, u), (emin, nmax - d["height"] * d["gsd"], emin + d["width"] * d["gsd"], nmax), d["gsd"],
                d["camera_height"])
        g.width, g.height = int(d["width"]), int(d["height"])
        return g


# ------------------------------------------------------------------------------------------------ extent
def percentile_sorted(xs, q):
    """numpy.percentile(x, q) (linear interpolation) read off the ascending 1-D tensor xs."""
    n = xs.numel()
    pos = (float(q) / 100.0) * (n - 1)
    k = min(int(math.floor(pos)), n - 1)
    lo = float(xs[k])
    return lo if k + 1 >= n else lo + (pos - k) * (float(xs[k + 1]) - lo)


def percentile_1d(x, q):
    """numpy.percentile(x, q) of a 1-D tensor by a sort: torch.quantile refuses inputs above 2^24 elements, and models
    here hold 28 M and 102 M rows (torch.kthvalue takes them, but its selection goes quadratic on ordered input)."""
    if x.numel() == 0:
        raise ValueError("percentile of an empty tensor")
    return percentile_sorted(torch.sort(x.detach().reshape(-1)).values, q)


def percentile_bounds(means, frame, lo=1.0, hi=99.0):
    """(emin, nmin, emax, nmax): the lo-th to hi-th percentile of the rows' e.mean and n.mean, so that floaters do not
    set the size of a city map.  One sort per axis."""
    if means.shape[0] == 0:
        raise ValueError("percentile bounds of an empty model")
    e, n, _ = frame
    out = []
    for axis in (e, n):
        coord = torch.sort(means.detach() @ torch.as_tensor(axis, dtype=means.dtype, device=means.device)).values
        out.append((percentile_sorted(coord, lo), percentile_sorted(coord, hi)))
    return out[0][0], out[1][0], out[0][1], out[1][1]


def default_camera_height(means, frame):
    """max(u . mean) + 1: above every row; a lower value doubles as a ceiling (rows above it are culled by the near plane)."""
    u = torch.as_tensor(frame[2], dtype=means.dtype, device=means.device)
    return float((means.detach() @ u).max()) + 1.0


# ------------------------------------------------------------------------------------------------ rendering
def check_tile(tile):
    tile = int(tile)
    if tile <= 0 or tile % RASTER_TILE:
        raise ValueError(f"--tile must be a positive multiple of {RASTER_TILE}, got {tile}")
    return tile


def _round_up(v, m):
    return (v + m - 1) // m * m


def _small_attributes(gaussians):
    """Activated means, quaternions and scales on the GPU (a naive_offload model keeps them in pinned host memory)."""
    put = lambda t: t.detach().to("cuda", non_blocking=True)
    return put(gaussians.get_xyz), put(gaussians.get_rotation), put(gaussians.get_scaling)


def window_sees_anything(camera, gaussians):
    """The eval entries' own cull (the cull-only orthographic projection) for one window: False when no Gaussian
    survives it.  The engines assert a non-empty filter (a training camera that sees nothing is an error); an empty
    window of a map is not, and is answered here, before the entry is called."""
    from .gsplat import visibility_radii
    xyz, rot, sca = _small_attributes(gaussians)
    radii = visibility_radii(xyz, rot, sca, camera.world_view_transform.t()[None].contiguous(), camera.K[None],
                             camera.image_width, camera.image_height,
                             radius_clip=float(getattr(utils.get_args(), "radius_clip", 0.0)), camera_model="ortho")
    return bool((radii > 0).any())


def render_window(camera, gaussians, background, args, depth_mode="expected"):
    """One OrthoCamera (the global image size must be its size) -> (image[3,h,w], expected depth[h,w], alpha[h,w]) on the
    GPU (depth_mode "median": the median depth, "ray": the ray depth); a window that sees no Gaussian is background, depth 0 and alpha 0."""
    h, w = camera.image_height, camera.image_width
    if not window_sees_anything(camera, gaussians):
        bg = background if background is not None else torch.zeros(3, device="cuda")
        return (bg.reshape(3, 1, 1).expand(3, h, w).float(), torch.zeros((h, w), device="cuda"),
                torch.zeros((h, w), device="cuda"))
    img, depth, alpha = eval_one_cam(camera, gaussians, background, args, None, render_mode=depth_render_mode(depth_mode))
    return img, depth[0], alpha[0]


def render_mosaic(gaussians, geometry, args, tile=4096, background=None, quantise=False, log=None, depth_mode="expected"):
    """The whole map, window by window, assembled on the host (depth_mode "median" / "ray": heights from the median / ray depth).
    -> (rgb [H,W,3]: float32 as rendered, or uint8 (clamped, x255) with quantise -- a 20 000^2 map is 1.2 GB of uint8 --,
        height float32 [H,W]: camera_height - expected depth, NaN where alpha < 0.5, alpha float32 [H,W]).
    Windows are min(tile, size rounded up to 16) pixels on a side; the last row and column are rendered whole and
    cropped.  Sets the global image size (utils.set_img_size) to the window."""
    tile = check_tile(tile)
    depth_render_mode(depth_mode)
    W, H = geometry.width, geometry.height
    tw, th = min(tile, _round_up(W, RASTER_TILE)), min(tile, _round_up(H, RASTER_TILE))
    rgb = np.empty((H, W, 3), dtype=np.uint8 if quantise else np.float32)
    height = np.empty((H, W), dtype=np.float32)
    alpha = np.empty((H, W), dtype=np.float32)
    utils.set_img_size(th, tw)
    with torch.no_grad():
        for y0 in range(0, H, th):
            for x0 in range(0, W, tw):
                cam = geometry.camera(x0, y0, tw, th, uid=(y0 // th) * ((W + tw - 1) // tw) + x0 // tw)
                img, depth, al = render_window(cam, gaussians, background, args, depth_mode)
                h, w = min(th, H - y0), min(tw, W - x0)
                img = img[:, :h, :w].permute(1, 2, 0)
                if quantise:
                    img = (torch.clamp(img, 0.0, 1.0) * 255).to(torch.uint8)
                hm = torch.where(al[:h, :w] >= 0.5, geometry.camera_height - depth[:h, :w],
                                 torch.full_like(depth[:h, :w], float("nan")))
                rgb[y0:y0 + h, x0:x0 + w] = img.cpu().numpy()
                height[y0:y0 + h, x0:x0 + w] = hm.cpu().numpy()
                alpha[y0:y0 + h, x0:x0 + w] = al[:h, :w].cpu().numpy()
                if log is not None:
                    log.write(f"window x0={x0} y0={y0} {w}x{h}\n")
    return rgb, height, alpha


def write_outputs(output_dir, geometry, rgb_u8, height, alpha, depth_mode="expected"):
    """(ortho.json carries "depth_mode" only when it is "median" or "ray")"""
    os.makedirs(output_dir, exist_ok=True)
    write_png(os.path.join(output_dir, "ortho.png"), rgb_u8)
    np.save(os.path.join(output_dir, "ortho_height.npy"), height.astype(np.float32))
    np.save(os.path.join(output_dir, "ortho_alpha.npy"), alpha.astype(np.float32))
    with open(os.path.join(output_dir, "ortho.json"), "w") as f:
        json.dump(dict(geometry.to_json(), **({"depth_mode": depth_mode} if depth_mode in ("median", "ray") else {})), f, indent=1)


def main(argv=None):
    ap = argparse.ArgumentParser(description="Orthophoto and height-map export")
    ap.add_argument("-m", "--model_path", required=True, help="model directory (point_cloud/iteration_*/point_cloud.ply) or a .ply")
    ap.add_argument("--iteration", type=int, default=-1)
    ap.add_argument("--output_dir", default=None)
    ap.add_argument("--up", type=float, nargs=3, default=(0.0, 0.0, 1.0), metavar=("X", "Y", "Z"))
    ap.add_argument("--east", type=float, nargs=3, default=(1.0, 0.0, 0.0), metavar=("X", "Y", "Z"))
    ap.add_argument("--bounds", type=float, nargs=4, default=None, metavar=("EMIN", "NMIN", "EMAX", "NMAX"),
                    help="map coordinates; default: 1st to 99th percentile of the rows")
    ap.add_argument("--gsd", type=float, default=None, help="world units per pixel")
    ap.add_argument("--width", type=int, default=None, help="map width in pixels (derives --gsd)")
    ap.add_argument("--camera_height", type=float, default=None, help="default: max(up . mean) + 1; lower = a ceiling")
    ap.add_argument("--tile", type=int, default=4096, help="window size in pixels, a multiple of 16")
    ap.add_argument("--white_background", action="store_true")
    ap.add_argument("--antialiased", action="store_true",
                    help="gsplat's rasterize_mode=\"antialiased\": for a model trained with trainer --antialiased")
    ap.add_argument("--depth_mode", default="expected", metavar="expected|median|ray",
                    help="the depth behind the height map: the expected depth D / alpha, the ray depth (where the median "
                         "Gaussian's density peaks along the pixel's ray), or the median depth (the Gaussian "
                         "at which the transmittance falls through one half)")
    g = ap.add_mutually_exclusive_group()
    g.add_argument("--clm_offload", action="store_true")
    g.add_argument("--naive_offload", action="store_true")
    g.add_argument("--no_offload", action="store_true")
    a = ap.parse_args(argv)
    try:  # refusals before anything is loaded
        tile = check_tile(a.tile)
        depth_render_mode(a.depth_mode)
    except ValueError as e:
        raise SystemExit(str(e))
    if (a.gsd is None) == (a.width is None):
        raise SystemExit("exactly one of --gsd and --width is needed")
    if a.width is not None and a.width <= 0:
        raise SystemExit(f"--width must be positive, got {a.width}")
    if not (a.clm_offload or a.naive_offload or a.no_offload):
        a.clm_offload = True
    frame = map_frame(a.up, a.east)
    args = utils.default_args(bsz=4, rasterize_mode="antialiased" if a.antialiased else "classic")
    for k in ("clm_offload", "naive_offload", "no_offload"):
        setattr(args, k, getattr(a, k))
    utils.set_args(args)
    utils.set_img_size(tile, tile)
    if a.clm_offload:
        from .strategies.clm_offload import GaussianModelCLMOffload as M
    elif a.naive_offload:
        from .strategies.naive_offload import GaussianModelNaiveOffload as M
    else:
        from .strategies.no_offload import GaussianModelNoOffload as M
    gaussians = M(3, only_for_rendering=True)
    gaussians.load_ply(_find_ply(a.model_path, a.iteration))
    gaussians.active_sh_degree = gaussians.max_sh_degree
    means = gaussians.get_xyz.detach()
    bounds = tuple(a.bounds) if a.bounds is not None else percentile_bounds(means, frame)
    gsd = a.gsd if a.gsd is not None else (bounds[2] - bounds[0]) / a.width
    cam_h = a.camera_height if a.camera_height is not None else default_camera_height(means, frame)
    geometry = MapGeometry(frame, bounds, gsd, cam_h)
    out = a.output_dir or os.path.join(a.model_path if os.path.isdir(a.model_path) else os.path.dirname(a.model_path),
                                       "render_ortho")
    os.makedirs(out, exist_ok=True)
    bg = torch.tensor([1.0, 1.0, 1.0], device="cuda") if a.white_background else None
    with open(os.path.join(out, "render_ortho.log"), "w") as log:
        log.write(f"Model path: {a.model_path}\nMap: {geometry.width}x{geometry.height} px, gsd {geometry.gsd}\n")
        rgb, height, alpha = render_mosaic(gaussians, geometry, args, tile=tile, background=bg, quantise=True, log=log,
                                           depth_mode=a.depth_mode)
    write_outputs(out, geometry, rgb, height, alpha, a.depth_mode)
    print(f"Orthophoto saved to: {out} ({geometry.width}x{geometry.height} px, gsd {geometry.gsd:g})")
    return 0


if __name__ == "__main__":
    sys.exit(main())
