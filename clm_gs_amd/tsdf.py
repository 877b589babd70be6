"""Mesh export ("Mesh export" and "Sparse volume"): a dense TSDF volume in a map frame, fused from rendered depth maps
(csrc/tsdf.hip through clm_kernels.tsdf_integrate) and turned into a triangle mesh by naive Surface Nets
(clm_kernels.tsdf_extract).

The box: frame (e, n, u) as render_ortho.map_frame gives it, bounds (emin, nmin, umin, emax, nmax, umax) in that frame,
`voxel` world units per voxel.  Grid axis x runs along e, y along n, z along u; voxel (i, j, k) sits at the grid point
(i + 0.5, j + 0.5, k + 0.5), i.e. at the world point  e (emin + (i + 0.5) voxel) + n (nmin + ...) + u (umin + ...).  The
kernels see grid coordinates only: the host composes, in float64, grid_to_world (3x4) for the vertices and one matrix
M = world_to_camera . grid_to_world per camera.

SparseTsdfVolume is the same volume stored in bricks of 8 x 8 x 8 voxels, allocated only where some camera's depth map can put
a surface (csrc/tsdf_sparse.hip): two passes over the cameras, mark then fuse, and the mesh of the dense volume bit for bit
on a box far beyond what the dense volume can hold."""
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


class _Staging:
    """Up to 16 cameras staged for one launch.  Two slots of stacked float32 planes [16, *lead, H, W], one per entry of
    `leads`, allocated once per image size: a slot is filled while the launch that reads the other one may still be running.
    launch(*planes[:fill], records [fill,16], *gates) runs at 16 cameras, before a camera whose gates or image size differ,
    and on flush().  (The owner passes `launch` with every call: a stored bound method would tie the volume into a cycle
    and keep its tensors until the collector runs.)"""

    def __init__(self, leads):
        self.leads = leads
        self.ring, self.size, self.slot, self.fill, self.records, self.gates = None, None, 0, 0, [], None

    def add(self, launch, device, record, planes, H, W, gates):
        if self.fill and (self.gates != gates or self.size != (H, W)):
            self.flush(launch)
        self.gates = gates
        if self.size != (H, W):
            self.ring = [tuple(torch.empty((BATCH,) + lead + (H, W), dtype=torch.float32, device=device) for lead in self.leads)
                         for _ in range(2)]
            self.size = (H, W)
        for dst, src in zip(self.ring[self.slot], planes):
            dst[self.fill].copy_(src.reshape(dst.shape[1:]))
        self.records.append(record)
        self.fill += 1
        if self.fill == BATCH:
            self.flush(launch)

    def flush(self, launch):
        if not self.fill:
            return
        launch(*(t[:self.fill] for t in self.ring[self.slot]), np.stack(self.records), *self.gates)
        self.slot, self.fill, self.records = 1 - self.slot, 0, []


class TsdfVolume:
    """The volume and its two operations.  integrate() may be called any number of times; the sums continue."""

    def __init__(self, frame, bounds, voxel, trunc_voxels=4.0, device="cuda", grid_gb=16.0):
        self.frame = tuple(np.asarray(v, dtype=np.float64) for v in frame)
        self.bounds = tuple(float(v) for v in bounds)
        self._size(voxel, grid_gb)
        self.voxel = float(voxel)
        if not (math.isfinite(trunc_voxels) and trunc_voxels > 0):
            raise ValueError(f"--trunc_voxels must be positive and finite, got {trunc_voxels}")
        self.trunc = float(trunc_voxels) * self.voxel
        self.grid_to_world = grid_to_world(self.frame, self.bounds, self.voxel)
        self.cameras_used = 0
        self._staged = _Staging(((), (), (3,)))
        self._allocate(device)

    def _size(self, voxel, grid_gb):
        self.nx, self.ny, self.nz = check_grid(self.bounds, voxel, grid_gb)

    def _allocate(self, device):
        self.grid = torch.zeros((6, self.nz, self.ny, self.nx), dtype=torch.float32, device=device)

    def _device(self):
        return self.grid.device

    # ------------------------------------------------------------------------------------------ fusion
    def _fuse(self, depth, alpha, rgb, records, near, depth_max, alpha_min):
        clm_kernels.tsdf_integrate(self.grid, depth, alpha, rgb, records, near=near, depth_max=depth_max, alpha_min=alpha_min,
                                   trunc=self.trunc)
        self.cameras_used += len(records)

    def add(self, camera, image, depth, alpha, near=0.01, depth_max=float("inf"), alpha_min=0.5):
        """Stages one camera's render (image [3,H,W], expected depth and alpha [H,W] or [1,H,W]) and launches the fusion
        when 16 are staged; flush() launches what is left.  The gates must not change inside a batch."""
        H, W = (int(v) for v in image.shape[-2:])
        self._staged.add(self._fuse, self._device(), camera_record(camera, self.grid_to_world), (depth, alpha, image), H, W,
                         (float(near), float(depth_max), float(alpha_min)))

    def flush(self):
        self._staged.flush(self._fuse)

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


# ---------------------------------------------------------------------------------------------- sparse volume
BRICK = clm_kernels.TSDF_BRICK
BYTES_PER_BRICK = BYTES_PER_VOXEL * BRICK ** 3   # 12 288: six float32 planes of 512 voxels
BYTES_PER_TABLE_ENTRY = 5                        # marks uint8 + table int32, per brick of the box
MAX_BRICK_GRID = clm_kernels.TSDF_MAX_BRICK_GRID  # inclusive
MAX_SPARSE_VOXELS = 1 << 31                      # S * 512, exclusive


def check_brick_grid(bounds, voxel, grid_gb=16.0):
    """grid_shape and the brick grid (nbx, nby, nbz) = ceil(n / 8) of the sparse volume, refused by name when a side reaches
    2^31 voxels, the brick grid holds more than 2^30 bricks, or marks + table alone (5 B per brick) exceed grid_gb: what can be
    refused from the bounds before anything is loaded.  -> ((nx, ny, nz), (nbx, nby, nbz))"""
    shape = grid_shape(bounds, voxel)
    if not (isinstance(grid_gb, (int, float)) and math.isfinite(grid_gb) and grid_gb > 0):
        raise ValueError(f"--grid_gb must be positive and finite, got {grid_gb}")
    if max(shape) >= 1 << 31:
        raise ValueError(f"--sparse: --voxel {voxel:g} gives a grid of {shape[0]} x {shape[1]} x {shape[2]} voxels, a side of "
                         "2^31 voxels or more; use a larger --voxel (or shrink --bounds)")
    nb = tuple(-(-v // BRICK) for v in shape)
    total = nb[0] * nb[1] * nb[2]
    if total > MAX_BRICK_GRID:
        fit = float(voxel) * (total / MAX_BRICK_GRID) ** (1.0 / 3.0)
        raise ValueError(f"--sparse: --voxel {voxel:g} gives a brick grid of {nb[0]} x {nb[1]} x {nb[2]} = {total} bricks, above "
                         f"2^30 bricks; about --voxel {fit:.3g} fits (an estimate; or shrink --bounds)")
    if total * BYTES_PER_TABLE_ENTRY > float(grid_gb) * 1e9:
        raise ValueError(f"--sparse: the brick table of {nb[0]} x {nb[1]} x {nb[2]} = {total} bricks takes "
                         f"{total * BYTES_PER_TABLE_ENTRY / 1e9:.2f} GB before any brick is allocated, above --grid_gb {grid_gb:g}")
    return shape, nb


def check_sparse_size(S, bricks_total, voxel, grid_gb=16.0):
    """The sizes of an allocation of S bricks out of bricks_total, refused by name: S * 512 < 2^31 and marks + table + pool
    <= grid_gb.  The message gives the brick count, the GB and an ESTIMATE of the voxel size that fits: a surface is
    two-dimensional, so the bytes go with voxel^-2 and the estimate is voxel sqrt(bytes / cap).  -> bytes"""
    S, bricks_total = int(S), int(bricks_total)
    nbytes = bricks_total * BYTES_PER_TABLE_ENTRY + S * BYTES_PER_BRICK
    cap_bytes = float(grid_gb) * 1e9
    cap_slots = (MAX_SPARSE_VOXELS - 1) // BRICK ** 3
    if S > cap_slots:
        fit = float(voxel) * math.sqrt(S / cap_slots)
        raise ValueError(f"--sparse: {S} of {bricks_total} bricks are marked ({nbytes / 1e9:.2f} GB), above 2^31 stored voxels "
                         f"({cap_slots} bricks); about --voxel {fit:.3g} fits (an estimate; or shrink --bounds)")
    if nbytes > cap_bytes:
        fit = float(voxel) * math.sqrt(nbytes / cap_bytes)
        raise ValueError(f"--sparse: {S} of {bricks_total} bricks are marked, marks + table + pool take {nbytes / 1e9:.2f} GB, "
                         f"above --grid_gb {grid_gb:g}; about --voxel {fit:.3g} fits (an estimate; or shrink --bounds)")
    return nbytes


def camera_mark_record(camera, g2w):
    """The 16 doubles clm_kernels.tsdf_mark takes: the inverse of camera_record's M (camera space -> grid coordinates, 3x4,
    float64), then fx, fy, cx, cy."""
    rec = camera_record(camera, g2w)
    inv = np.linalg.inv(np.vstack([rec[:12].reshape(3, 4), [0.0, 0.0, 0.0, 1.0]]))
    return np.concatenate([inv[:3].reshape(12), rec[12:]])


class SparseTsdfVolume(TsdfVolume):
    """TsdfVolume in bricks of 8 x 8 x 8 voxels, allocated where a surface can be.  First mark() every camera, then allocate(),
    then add() / integrate() the SAME cameras and depth maps, then extract(): the mesh is the dense volume's, bit for bit
    ("Sparse volume").  The dense limits do not apply; grid_gb bounds marks + table + pool."""

    def _size(self, voxel, grid_gb):
        (self.nx, self.ny, self.nz), (self.nbx, self.nby, self.nbz) = check_brick_grid(self.bounds, voxel, grid_gb)
        self.grid_gb = float(grid_gb)

    def _allocate(self, device):
        self.marks = torch.zeros((self.nbz, self.nby, self.nbx), dtype=torch.uint8, device=device)
        self.table = self.bricks = self.pool = None
        self.cameras_marked = 0
        self._marked = _Staging(((), ()))

    @property
    def shape(self):
        return self.nx, self.ny, self.nz

    @property
    def bricks_total(self):
        return self.nbx * self.nby * self.nbz

    @property
    def S(self):
        if self.pool is None:
            raise ValueError("SparseTsdfVolume: allocate() has not been called")
        return int(self.pool.shape[0])

    @property
    def nbytes(self):
        return self.bricks_total * BYTES_PER_TABLE_ENTRY + self.S * BYTES_PER_BRICK

    def _device(self):
        return self.marks.device

    # ------------------------------------------------------------------------------------------ pass 1: marking
    def mark(self, camera, depth, alpha, near=0.01, depth_max=float("inf"), alpha_min=0.5):
        """Stages one camera's depth and alpha ([H,W] or [1,H,W]) and launches the marking when 16 are staged, as add()
        does for the fusion; allocate() launches what is left."""
        if self.pool is not None:
            raise ValueError("SparseTsdfVolume: mark() after allocate(): a brick allocated late would lack the earlier "
                             "cameras' observations; mark every camera first")
        H, W = (int(v) for v in depth.shape[-2:])
        self._marked.add(self._mark, self._device(), camera_mark_record(camera, self.grid_to_world), (depth, alpha), H, W,
                         (float(near), float(depth_max), float(alpha_min)))

    def _mark(self, depth, alpha, records, near, depth_max, alpha_min):
        clm_kernels.tsdf_mark(self.marks, self.shape, depth, alpha, records, near=near, depth_max=depth_max,
                              alpha_min=alpha_min, trunc=self.trunc, voxel_cam=self.voxel)
        self.cameras_marked += len(records)

    def allocate(self):
        """Builds table, bricks and the zeroed pool from the marks; refuses by name S * 512 >= 2^31 and marks + table + pool
        above grid_gb.  -> S.  No marked brick is a result (S = 0), not an error."""
        if self.pool is not None:
            raise ValueError("SparseTsdfVolume: allocate() has been called already")
        self._marked.flush(self._mark)
        self._marked = _Staging(((), ()))  # (the staging buffers are free before the pool is allocated)
        flat = self.marks.reshape(-1) != 0
        S = int(flat.sum())
        check_sparse_size(S, self.bricks_total, self.voxel, self.grid_gb)
        scan = torch.cumsum(flat, 0, dtype=torch.int32)
        self.table = torch.where(flat, scan - 1, torch.full_like(scan, -1)).reshape(self.nbz, self.nby, self.nbx).contiguous()
        del scan
        self.bricks = torch.nonzero(flat).reshape(-1).to(torch.int32)
        self.pool = torch.zeros((S, 6, BRICK, BRICK, BRICK), dtype=torch.float32, device=self._device())
        return S

    # ------------------------------------------------------------------------------------------ pass 2: fusion
    def add(self, camera, image, depth, alpha, near=0.01, depth_max=float("inf"), alpha_min=0.5):
        if self.pool is None:
            raise ValueError("SparseTsdfVolume: add() before allocate(): mark() every camera, then allocate(), then add() them")
        if self.S:
            super().add(camera, image, depth, alpha, near, depth_max, alpha_min)
        else:
            camera_record(camera, self.grid_to_world)  # (an orthographic camera is refused all the same)
            self.cameras_used += 1

    def _fuse(self, depth, alpha, rgb, records, near, depth_max, alpha_min):
        clm_kernels.tsdf_sparse_integrate(self.pool, self.bricks, self.shape, depth, alpha, rgb, records, near=near,
                                          depth_max=depth_max, alpha_min=alpha_min, trunc=self.trunc)
        self.cameras_used += len(records)

    # ------------------------------------------------------------------------------------------ surface
    def extract(self, min_weight=2.0):
        """As TsdfVolume.extract, in the same order: vertices by cell index, faces by (owner voxel, axis)."""
        self.flush()
        if self.S == 0:
            dev = self._device()
            return (torch.empty((0, 3), dtype=torch.float32, device=dev), torch.empty((0, 3), dtype=torch.uint8, device=dev),
                    torch.empty((0, 3), dtype=torch.int32, device=dev))
        return clm_kernels.tsdf_sparse_extract(self.pool, self.bricks, self.table, self.shape, min_weight, self.grid_to_world)

    def to_dense(self):
        """float32 [6, nz, ny, nx] with zeros where nothing is stored: for tests and for boxes that fit."""
        self.flush()
        S = self.S
        n = self.nx * self.ny * self.nz
        if n >= MAX_VOXELS:
            raise ValueError(f"SparseTsdfVolume.to_dense: {self.nx} x {self.ny} x {self.nz} = {n} voxels, 2^31 or more")
        full = torch.zeros((self.bricks_total, 6, BRICK, BRICK, BRICK), dtype=torch.float32, device=self._device())
        if S:
            full[self.bricks.long()] = self.pool
        full = full.reshape(self.nbz, self.nby, self.nbx, 6, BRICK, BRICK, BRICK).permute(3, 0, 4, 1, 5, 2, 6)
        full = full.reshape(6, self.nbz * BRICK, self.nby * BRICK, self.nbx * BRICK)
        return full[:, :self.nz, :self.ny, :self.nx].contiguous()
