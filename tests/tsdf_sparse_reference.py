"""numpy restatement of the marking kernel of csrc/tsdf_sparse.hip ("Sparse volume"), operation for
operation in float64, with the band of pixel-slabs whose box edge sits within rounding of a voxel-centre threshold; the set
N of voxels some camera observes with a negative term, computed voxel-side from the update rule and independent of the
marking code; the restriction of a dense grid to a set of bricks; and the sphere scene the CPU and GPU tests share."""
import math

import numpy as np

from tests import tsdf_reference as R

F32, F64 = np.float32, np.float64
TAU = 2.0 ** -20
BRICK = 8
ZREL = 2.0 ** -20   # TS_MARK_ZREL
GEPS = 2.0 ** -16   # TS_MARK_GEPS
MAX_SLABS = 4096


def brick_grid(shape):
    """(nbx, nby, nbz) of (nx, ny, nz)."""
    return tuple(-(-int(v) // BRICK) for v in shape)


def invert_records(cams):
    """[B,16] grid -> camera records (3x4, fx, fy, cx, cy) -> the records of the marking: the inverse map, float64."""
    cams = np.asarray(cams, dtype=F64)
    out = cams.copy()
    for b in range(len(cams)):
        out[b, :12] = np.linalg.inv(np.vstack([cams[b, :12].reshape(3, 4), [0.0, 0.0, 0.0, 1.0]]))[:3].reshape(12)
    return out


def _store(marks, b0, b1, ok):
    """marks[bz, by, bx] = True over the brick ranges b0[e] .. b1[e] (arrays [3, P]) of the pixel-slabs `ok`."""
    rows = np.unique(np.concatenate([b0[:, ok], b1[:, ok]]).T, axis=0)
    for x0, y0, z0, x1, y1, z1 in rows:
        marks[z0:z1 + 1, y0:y1 + 1, x0:x1 + 1] = True


def mark(shape, cams_inv, depth, alpha, near, depth_max, alpha_min, trunc, voxel_cam):
    """-> (marks bool [nbz,nby,nbx], band, slabs, lo, hi): the marked brick set; band: how many pixel-slabs have a box
    edge (after the widening, less 0.5) within 2^-20 of an integer, i.e. whose first or last voxel index a rounding
    difference could move; slabs: the number of pixel-slabs; lo / hi: the sets with every box narrowed / widened by 2^-20,
    between which any implementation that differs only by rounding must lie (lo == hi == marks when band == 0)."""
    nx, ny, nz = (int(v) for v in shape)
    nbx, nby, nbz = brick_grid(shape)
    dim = np.array([nx, ny, nz], dtype=F64)
    sets = [np.zeros((nbz, nby, nbx), dtype=bool) for _ in range(3)]  # marks, lo, hi
    B, H, W = depth.shape
    near64, trunc64 = F64(F32(near)), F64(F32(trunc))
    depth_max, alpha_min = F32(depth_max), F32(alpha_min)
    voxel_cam = F64(voxel_cam)
    band = slabs = 0
    row, col = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    row, col = row.reshape(-1).astype(F64), col.reshape(-1).astype(F64)
    for b in range(B):
        m = np.asarray(cams_inv[b], dtype=F64)
        d, a = depth[b].reshape(-1), alpha[b].reshape(-1)
        with np.errstate(all="ignore"):
            gate = (a >= alpha_min) & (d > F32(0.0)) & (d <= depth_max) & np.isfinite(d)
            d64 = d.astype(F64)
            z0 = np.maximum(d64, near64) * (1.0 - ZREL)
            z1 = (d64 + trunc64) * (1.0 + ZREL)
            gate &= z1 > z0
            fn = np.ceil((z1 - z0) / (4.0 * voxel_cam))
        nslab = np.where(gate, np.clip(np.where(fn >= 1.0, fn, 1.0), 1.0, float(MAX_SLABS)), 0.0).astype(np.int64)
        fx, fy, cx, cy = m[12:]
        xf = [(col - cx) / fx, ((col + 1.0) - cx) / fx]
        yf = [(row - cy) / fy, ((row + 1.0) - cy) / fy]
        for s in range(int(nslab.max()) if nslab.size else 0):
            live = nslab > s
            ns = np.where(live, nslab, 1).astype(F64)
            with np.errstate(all="ignore"):
                zz = [z0 + (z1 - z0) * (F64(s) / ns), z0 + (z1 - z0) * (F64(s + 1) / ns)]
                lo = hi = None
                for c in range(8):
                    z = zz[c >> 2]
                    x, y = xf[c & 1] * z, yf[(c >> 1) & 1] * z
                    g = np.stack([((m[4 * e] * x + m[4 * e + 1] * y) + m[4 * e + 2] * z) + m[4 * e + 3] for e in range(3)])
                    lo = g if c == 0 else np.minimum(lo, g)
                    hi = g if c == 0 else np.maximum(hi, g)
                ea = (lo - (1.0 + GEPS)) - 0.5   # a voxel index i is covered iff ea <= i <= eb
                eb = (hi + (1.0 + GEPS)) - 0.5
                near_int = (np.abs(ea - np.rint(ea)) <= TAU) | (np.abs(eb - np.rint(eb)) <= TAU)
                band += int((live & near_int.any(axis=0)).sum())
                slabs += int(live.sum())
                for which, shift in enumerate((0.0, TAU, -TAU)):
                    first = np.maximum(np.ceil(ea + shift), 0.0)
                    last = np.minimum(np.floor(eb - shift), dim[:, None] - 1.0)
                    ok = live & (first <= last).all(axis=0)
                    if ok.any():
                        b0 = np.where(ok, first, 0.0).astype(np.int64) >> 3
                        b1 = np.where(ok, last, 0.0).astype(np.int64) >> 3
                        _store(sets[which], b0, b1, ok)
    return sets[0], band, slabs, sets[1], sets[2]


def negative_voxels(shape, cams, depth, alpha, near, depth_max, alpha_min, trunc):
    """The set N, bool [nz,ny,nx]: the voxels at least one camera observes with -trunc <= sdf < 0, by the update rule of
    csrc/tsdf_math.h applied voxel by voxel (the projection of tsdf_reference.integrate)."""
    nx, ny, nz = (int(v) for v in shape)
    B, H, W = depth.shape
    k, j, i = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    px, py, pz = i.astype(F64) + 0.5, j.astype(F64) + 0.5, k.astype(F64) + 0.5
    near64 = F64(F32(near))
    trunc, depth_max, alpha_min = F32(trunc), F32(depth_max), F32(alpha_min)
    neg = np.zeros((nz, ny, nx), dtype=bool)
    for b in range(B):
        c = np.asarray(cams[b], dtype=F64)
        rw = lambda r: ((c[r] * px + c[r + 1] * py) + c[r + 2] * pz) + c[r + 3]
        x, y, z = rw(0), rw(4), rw(8)
        with np.errstate(all="ignore"):
            fu, fv = np.floor(c[12] * x / z + c[14]), np.floor(c[13] * y / z + c[15])
            seen = (z > near64) & (fu >= 0.0) & (fu < float(W)) & (fv >= 0.0) & (fv < float(H))
            cc, rr = np.where(seen, fu, 0.0).astype(np.int64), np.where(seen, fv, 0.0).astype(np.int64)
            d, a = depth[b][rr, cc], alpha[b][rr, cc]
            sdf = d - z.astype(F32)
            neg |= seen & (a >= alpha_min) & (d > F32(0.0)) & (d <= depth_max) & ~(sdf < -trunc) & (sdf < F32(0.0))
    return neg


def dilate(mask, r=1):
    """The voxels within r of a voxel of the mask in infinity norm."""
    out = np.array(mask, dtype=bool, copy=True)
    for axis in range(3):
        acc = out.copy()
        for s in range(1, r + 1):
            lo = [slice(None)] * 3
            hi = [slice(None)] * 3
            lo[axis], hi[axis] = slice(0, -s), slice(s, None)
            acc[tuple(lo)] |= out[tuple(hi)]
            acc[tuple(hi)] |= out[tuple(lo)]
        out = acc
    return out


def voxels(marks, shape):
    """Brick marks [nbz,nby,nbx] -> the voxel mask [nz,ny,nx]."""
    nx, ny, nz = (int(v) for v in shape)
    m = np.repeat(np.repeat(np.repeat(np.asarray(marks, dtype=bool), BRICK, 0), BRICK, 1), BRICK, 2)
    return m[:nz, :ny, :nx]


def restrict(grid, marks):
    """The dense grid [6,nz,ny,nx] with zeros outside the marked bricks: what a sparse volume holds."""
    _, nz, ny, nx = grid.shape
    return np.where(voxels(marks, (nx, ny, nz))[None], grid, F32(0.0)).astype(F32)


# ------------------------------------------------------------------------------------------------ the sphere scene
SHAPE = (48, 40, 40)
ORIGIN = (-2.4, -2.0, -2.0)  # of the box, in world units: bounds (-2.4, -2, -2, 2.4, 2, 2)
VOXEL, TRUNC, NEAR, DEPTH_MAX, ALPHA_MIN = 0.1, 0.4, 0.01, float("inf"), 0.5
H, W, N_CAMS, RADIUS = 60, 80, 12, 0.9
_CACHE = {}


def look_at(C, target, up):
    f = target - C
    f = f / np.linalg.norm(f)
    r = np.cross(f, up)
    r = r / np.linalg.norm(r)
    d = np.cross(f, r)
    w2c = np.eye(4)
    w2c[:3, :3] = np.stack([r, d, f])
    w2c[:3, 3] = -w2c[:3, :3] @ C
    return w2c


def sphere_scene(centre=(0.0, 0.0, 0.0), seed=7):
    """dict: shape, g2w [3,4], cams [12,16] (grid -> camera), cams_inv, depth / alpha float32 [12,60,80], rgb [12,3,60,80]:
    a sphere of radius 0.9 at `centre` in a 4.8 x 4.0 x 4.0 box about the origin (voxel 0.1: 6 x 5 x 5 bricks), 12 seeded
    look-at cameras 3.5 to 4.5 from the origin with focal lengths 60 to 80; the depth of a pixel is the camera z of the near
    intersection of the ray through its centre, alpha 1 on a hit and 0 elsewhere, colours random."""
    key = (tuple(float(v) for v in centre), seed)
    if key in _CACHE:
        return _CACHE[key]
    rng = np.random.default_rng(seed)
    nx, ny, nz = SHAPE
    g2w = np.array([[VOXEL, 0, 0, ORIGIN[0]], [0, VOXEL, 0, ORIGIN[1]], [0, 0, VOXEL, ORIGIN[2]]], dtype=F64)
    g4 = np.vstack([g2w, [0, 0, 0, 1.0]])
    centre = np.asarray(centre, dtype=F64)
    cams = np.empty((N_CAMS, 16))
    depth = np.zeros((N_CAMS, H, W), dtype=F32)
    alpha = np.zeros((N_CAMS, H, W), dtype=F32)
    v, u = np.meshgrid(np.arange(H) + 0.5, np.arange(W) + 0.5, indexing="ij")
    for b in range(N_CAMS):
        d = rng.normal(size=3)
        C = d / np.linalg.norm(d) * rng.uniform(3.5, 4.5)
        w2c = look_at(C, rng.uniform(-0.2, 0.2, size=3), rng.normal(size=3))
        fx, fy = rng.uniform(60, 80, size=2)
        cx, cy = W / 2 + rng.uniform(-2, 2), H / 2 + rng.uniform(-2, 2)
        cams[b, :12] = (w2c @ g4)[:3].reshape(12)
        cams[b, 12:] = (fx, fy, cx, cy)
        dirs = np.stack([(u - cx) / fx, (v - cy) / fy, np.ones_like(u)], -1) @ w2c[:3, :3]  # world direction per unit camera z
        oc = C - centre
        qa, qb, qc = (dirs * dirs).sum(-1), 2.0 * (dirs @ oc), oc @ oc - RADIUS * RADIUS
        disc = qb * qb - 4 * qa * qc
        hit = disc > 0
        t = (-qb - np.sqrt(np.where(hit, disc, 0.0))) / (2 * qa)
        depth[b] = np.where(hit, t, 0.0).astype(F32)
        alpha[b] = hit.astype(F32)
    rgb = rng.uniform(0.0, 1.0, size=(N_CAMS, 3, H, W)).astype(F32)
    _CACHE[key] = dict(shape=SHAPE, g2w=g2w, cams=cams, cams_inv=invert_records(cams), depth=depth, alpha=alpha, rgb=rgb)
    return _CACHE[key]


def scene_marks(scene):
    """mark() of a scene with the scene's gates, cached on the scene."""
    if "marks" not in scene:
        scene["marks"] = mark(scene["shape"], scene["cams_inv"], scene["depth"], scene["alpha"], NEAR, DEPTH_MAX, ALPHA_MIN,
                              TRUNC, VOXEL)
    return scene["marks"]


def scene_dense(scene):
    """tsdf_reference.integrate of a scene from a zero grid -> (grid, band), cached on the scene."""
    if "dense" not in scene:
        nx, ny, nz = scene["shape"]
        scene["dense"] = R.integrate(np.zeros((6, nz, ny, nx), dtype=F32), scene["cams"], scene["depth"], scene["alpha"],
                                     scene["rgb"], NEAR, DEPTH_MAX, ALPHA_MIN, TRUNC)
    return scene["dense"]


def scene_negative(scene):
    if "neg" not in scene:
        scene["neg"] = negative_voxels(scene["shape"], scene["cams"], scene["depth"], scene["alpha"], NEAR, DEPTH_MAX,
                                       ALPHA_MIN, TRUNC)
    return scene["neg"]
