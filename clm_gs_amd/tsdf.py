"""Mesh export ("Mesh export"): a dense TSDF volume in a map frame, fused from rendered depth maps
(csrc/tsdf.hip through clm_kernels.tsdf_integrate) and turned into a triangle mesh by naive Surface Nets
(clm_kernels.tsdf_extract).

The box: frame (e, n, u) as render_ortho.map_frame gives it, bounds (emin, nmin, umin, emax, nmax, umax) in that frame,
`voxel` world units per voxel.  Grid axis x runs along e, y along n, z along u; voxel (i, j, k) sits at the grid point
(i + 0.5, j + 0.5, k + 0.5), i.e. at the world point  e (emin + (i + 0.5) voxel) + n (nmin + ...) + u (umin + ...).  The
kernels see grid coordinates only: the host composes, in float64, grid_to_world (3x4) for the vertices and one matrix
M = world_to_camera . grid_to_world per camera."""
import math

import numpy as np
import torch

from . import clm_kernels

BYTES_PER_VOXEL = 24   # six float32 planes
MAX_VOXELS = 1 << 31   # exclusive
BATCH = clm_kernels.TSDF_MAX_B


def grid_shape(bounds, voxel):
    """(nx, ny, nz) of the box: ceil(extent / voxel) per axis, 2 at the least.  Refuses a non-positive voxel and inverted
    bounds by name."""
    if not (isinstance(voxel, (int, float)) and math.isfinite(voxel) and voxel > 0):
        raise ValueError(f"--voxel must be positive and finite, got {voxel}")
    b = [float(v) for v in bounds]
    if len(b) != 6 or not all(math.isfinite(v) for v in b):
        raise ValueError(f"--bounds must be six finite numbers emin nmin umin emax nmax umax, got {bounds}")
    if not (b[3] > b[0] and b[4] > b[1] and b[5] > b[2]):
        raise ValueError(f"--bounds must be emin nmin umin emax nmax umax with every max above its min, got {tuple(b)}")
    return tuple(max(2, int(math.ceil((b[3 + a] - b[a]) / float(voxel) - 1e-9))) for a in range(3))


def check_grid(bounds, voxel, grid_gb=16.0):
    """grid_shape, refused by name when the grid would hold 2^31 voxels or more or take more than grid_gb GB (24 B per
    voxel); the message states the voxel size that fits."""
    nx, ny, nz = grid_shape(bounds, voxel)
    n = nx * ny * nz
    cap = min(MAX_VOXELS - 1, int(float(grid_gb) * 1e9 / BYTES_PER_VOXEL))
    if cap < 8:
        raise ValueError(f"--grid_gb must allow at least 2 x 2 x 2 voxels, got {grid_gb}")
    if n > cap:
        fit = float(voxel) * (n / cap) ** (1.0 / 3.0)
        while True:  # (the cube root rounded up to three digits, then up in 1 % steps until the rounded-up sides fit)
            unit = 10.0 ** (math.floor(math.log10(fit)) - 2)
            fit = math.ceil(fit / unit) * unit
            s = grid_shape(bounds, fit)
            if s[0] * s[1] * s[2] <= cap:
                break
            fit *= 1.01
        what = "2^31 voxels" if cap == MAX_VOXELS - 1 else f"--grid_gb {grid_gb:g}"
        raise ValueError(f"--voxel {voxel:g} gives a grid of {nx} x {ny} x {nz} = {n} voxels ({n * BYTES_PER_VOXEL / 1e9:.2f} GB), "
                         f"above {what}; --voxel {fit:.3g} fits (or shrink --bounds)")
    return nx, ny, nz


def grid_to_world(frame, bounds, voxel):
    """float64 [3,4]: grid coordinates -> world."""
    e, n, u = (np.asarray(v, dtype=np.float64) for v in frame)
    g = np.empty((3, 4), dtype=np.float64)
    g[:, 0], g[:, 1], g[:, 2] = e * voxel, n * voxel, u * voxel
    g[:, 3] = e * float(bounds[0]) + n * float(bounds[1]) + u * float(bounds[2])
    return g


def camera_record(camera, g2w):
    """The 16 doubles csrc/tsdf.hip takes for a pinhole camera: M = world_to_camera . grid_to_world (3x4, float64), then
    fx, fy, cx, cy.  Orthographic cameras are refused."""
    from .cameras import camera_model
    if camera_model(camera) != "pinhole":
        raise ValueError(f"tsdf: camera {getattr(camera, 'image_name', camera)!r} is not a pinhole; orthographic cameras "
                         "are not supported as sources of a mesh")
    host = getattr(camera, "_clmgs_host", None)
    if host is not None:
        w2c, K = np.asarray(host[0], dtype=np.float64).reshape(4, 4), np.asarray(host[1], dtype=np.float64).reshape(3, 3)
    else:
        w2c = camera.world_view_transform.t().detach().cpu().double().numpy()
        K = camera.K.detach().cpu().double().numpy()
    g4 = np.vstack([g2w, [0.0, 0.0, 0.0, 1.0]])
    return np.concatenate([(w2c @ g4)[:3].reshape(12), [K[0, 0], K[1, 1], K[0, 2], K[1, 2]]])


class TsdfVolume:
    """The volume and its two operations.  integrate() may be called any number of times; the sums continue."""

    def __init__(self, frame, bounds, voxel, trunc_voxels=4.0, device="cuda", grid_gb=16.0):
        self.frame = tuple(np.asarray(v, dtype=np.float64) for v in frame)
        self.bounds = tuple(float(v) for v in bounds)
        self.nx, self.ny, self.nz = check_grid(self.bounds, voxel, grid_gb)
        self.voxel = float(voxel)
        if not (math.isfinite(trunc_voxels) and trunc_voxels > 0):
            raise ValueError(f"--trunc_voxels must be positive and finite, got {trunc_voxels}")
        self.trunc = float(trunc_voxels) * self.voxel
        self.grid_to_world = grid_to_world(self.frame, self.bounds, self.voxel)
        self.grid = torch.zeros((6, self.nz, self.ny, self.nx), dtype=torch.float32, device=device)
        self.cameras_used = 0
        self._ring, self._slot, self._fill, self._records = None, 0, 0, []
        self._gates = None

    # ------------------------------------------------------------------------------------------ fusion
    def _buffers(self, H, W):
        """Two slots of stacked batch inputs, allocated once per image size: a slot is filled while the launch that reads
        the other one may still be running."""
        if self._ring is None or self._ring[0][0].shape[1:] != (H, W):
            dev = self.grid.device
            self._ring = [(torch.empty((BATCH, H, W), dtype=torch.float32, device=dev),
                           torch.empty((BATCH, H, W), dtype=torch.float32, device=dev),
                           torch.empty((BATCH, 3, H, W), dtype=torch.float32, device=dev)) for _ in range(2)]
        return self._ring[self._slot]

    def add(self, camera, image, depth, alpha, near=0.01, depth_max=float("inf"), alpha_min=0.5):
        """Stages one camera's render (image [3,H,W], expected depth and alpha [H,W] or [1,H,W]) and launches the fusion
        when 16 are staged; flush() launches what is left.  The gates must not change inside a batch."""
        gates = (float(near), float(depth_max), float(alpha_min))
        H, W = (int(v) for v in image.shape[-2:])
        if self._fill and (self._gates != gates or self._ring[0][0].shape[1:] != (H, W)):
            self.flush()
        self._gates = gates
        d, a, c = self._buffers(H, W)
        d[self._fill].copy_(depth.reshape(H, W))
        a[self._fill].copy_(alpha.reshape(H, W))
        c[self._fill].copy_(image.reshape(3, H, W))
        self._records.append(camera_record(camera, self.grid_to_world))
        self._fill += 1
        if self._fill == BATCH:
            self.flush()

    def flush(self):
        if not self._fill:
            return
        d, a, c = self._ring[self._slot]
        near, depth_max, alpha_min = self._gates
        clm_kernels.tsdf_integrate(self.grid, d[:self._fill], a[:self._fill], c[:self._fill], np.stack(self._records),
                                   near=near, depth_max=depth_max, alpha_min=alpha_min, trunc=self.trunc)
        self.cameras_used += self._fill
        self._slot, self._fill, self._records = 1 - self._slot, 0, []

    def integrate(self, cameras, renders, near=0.01, depth_max=float("inf"), alpha_min=0.5):
        """cameras: pinhole cameras; renders: per camera (image [3,H,W], expected depth, alpha) as the eval entries return
        them with render_mode="RGB+ED".  In batches of 16, in order."""
        cameras, renders = list(cameras), list(renders)
        if len(cameras) != len(renders):
            raise ValueError(f"tsdf: {len(cameras)} cameras and {len(renders)} renders")
        for cam, (image, depth, alpha) in zip(cameras, renders):
            self.add(cam, image, depth, alpha, near, depth_max, alpha_min)
        self.flush()
        return self

    # ------------------------------------------------------------------------------------------ surface
    def extract(self, min_weight=2.0):
        """-> (verts float32 [V,3] in world coordinates, colours uint8 [V,3], faces int32 [F,3]) on the device; an empty
        result is V = F = 0, not an error."""
        self.flush()
        return clm_kernels.tsdf_extract(self.grid, min_weight, self.grid_to_world)
