"""numpy restatement of csrc/tsdf_math.h / csrc/tsdf.hip ("Mesh export"): the TSDF fusion operation for
operation (float64 projection without contraction, float32 sums in camera order) with the band of voxels whose decision
sits within rounding of a threshold, naive Surface Nets as specified, two analytic grids, and the topology figures the
tests assert."""
import numpy as np

F32, F64 = np.float32, np.float64
TAU = 2.0 ** -20
PLANES = 6


# ------------------------------------------------------------------------------------------------ fusion
def integrate(grid, cams, depth, alpha, rgb, near, depth_max, alpha_min, trunc):
    """grid float32 [6,nz,ny,nx] (not modified), cams float64 [B,16], depth / alpha float32 [B,H,W], rgb [B,3,H,W].
    -> (new grid, band int32 [nz,ny,nx]: for how many cameras the voxel's decision is within rounding of a threshold:
    u or v within 2^-20 of an integer, z within 2^-20 (relative) of near, sdf within 2^-20 trunc of +-trunc)."""
    g = np.array(grid, dtype=F32, copy=True)
    _, nz, ny, nx = g.shape
    B, H, W = depth.shape
    k, j, i = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    px, py, pz = i.astype(F64) + 0.5, j.astype(F64) + 0.5, k.astype(F64) + 0.5
    near64 = F64(F32(near))
    trunc, depth_max, alpha_min = F32(trunc), F32(depth_max), F32(alpha_min)
    inv_trunc = F32(1.0) / trunc
    band = np.zeros((nz, ny, nx), dtype=np.int32)
    one = F32(1.0)
    for b in range(B):
        c = np.asarray(cams[b], dtype=F64)
        row = lambda r: ((c[r] * px + c[r + 1] * py) + c[r + 2] * pz) + c[r + 3]
        x, y, z = row(0), row(4), row(8)
        front = z > near64
        with np.errstate(all="ignore"):
            u = c[12] * x / z + c[14]
            v = c[13] * y / z + c[15]
            fu, fv = np.floor(u), np.floor(v)
            seen = front & (fu >= 0.0) & (fu < float(W)) & (fv >= 0.0) & (fv < float(H))
            col = np.where(seen, fu, 0.0).astype(np.int64)
            rw = np.where(seen, fv, 0.0).astype(np.int64)
            d, a = depth[b][rw, col], alpha[b][rw, col]
            gate = seen & (a >= alpha_min) & (d > F32(0.0)) & (d <= depth_max)
            sdf = d - z.astype(F32)
            assert sdf.dtype == F32
            obs = gate & ~(sdf < -trunc)
            term = np.minimum(sdf * inv_trunc, one)
            colour = obs & (sdf <= trunc)
            near_uv = front & ((np.abs(u - np.rint(u)) <= TAU) | (np.abs(v - np.rint(v)) <= TAU))
            near_z = np.abs(z - near64) <= TAU * np.maximum(np.abs(z), abs(near64))
            near_t = gate & (np.abs(np.abs(sdf.astype(F64)) - F64(trunc)) <= TAU * F64(trunc))
        band += (near_uv | near_z | near_t).astype(np.int32)
        g[0] = np.where(obs, g[0] + term, g[0])
        g[1] = np.where(obs, g[1] + one, g[1])
        for ch in range(3):
            pc = np.minimum(np.maximum(rgb[b, ch][rw, col], F32(0.0)), one)
            g[2 + ch] = np.where(colour, g[2 + ch] + pc, g[2 + ch])
        g[5] = np.where(colour, g[5] + one, g[5])
    assert g.dtype == F32
    return g, band


# ------------------------------------------------------------------------------------------------ extraction
def _corner(a, c):
    """The array of corner c of every cell: a[k + (c >> 2), j + ((c >> 1) & 1), i + (c & 1)] over the cells."""
    nz, ny, nx = a.shape[-3:]
    dx, dy, dz = c & 1, (c >> 1) & 1, c >> 2
    return a[..., dz:nz - 1 + dz, dy:ny - 1 + dy, dx:nx - 1 + dx]


def edge_corner(axis, r):
    s = 1 << axis
    return (r & (s - 1)) | ((r >> axis) << (axis + 1))


def active_cells(grid, min_weight):
    valid, inside = grid[1] >= F32(min_weight), grid[0] < F32(0.0)
    ok = np.ones(_corner(valid, 0).shape, dtype=bool)
    nin = np.zeros(ok.shape, dtype=np.int32)
    for c in range(8):
        ok &= _corner(valid, c)
        nin += _corner(inside, c)
    return ok & (nin > 0) & (nin < 8)


def extract(grid, min_weight, g2w):
    """-> (verts float32 [V,3], colours uint8 [V,3], faces int32 [F,3], cells int [V,3]: the (i, j, k) of each vertex's cell)."""
    grid = np.asarray(grid, dtype=F32)
    g2w = np.asarray(g2w, dtype=F64)
    _, nz, ny, nx = grid.shape
    active = active_cells(grid, min_weight)
    ks, js, is_ = np.nonzero(active)  # C order = cell linear index order
    V = len(ks)
    ids = np.full((nz, ny, nx), -1, dtype=np.int64)
    ids[ks, js, is_] = np.arange(V)
    with np.errstate(all="ignore"):
        vox = [[_corner(grid[p], c)[ks, js, is_] for c in range(8)] for p in range(PLANES)]
        val = [vox[0][c].astype(F64) / vox[1][c].astype(F64) for c in range(8)]
        col = [[np.where(vox[5][c] > 0, vox[2 + ch][c].astype(F64) / vox[5][c].astype(F64), 0.5) for c in range(8)]
               for ch in range(3)]
        sp, sc = [np.zeros(V) for _ in range(3)], [np.zeros(V) for _ in range(3)]
        n = np.zeros(V)
        for axis in range(3):
            for r in range(4):
                a = edge_corner(axis, r)
                b = a + (1 << axis)
                cross = (vox[0][a] < 0) != (vox[0][b] < 0)
                t = val[a] / (val[a] - val[b])
                for d in range(3):
                    sp[d] = sp[d] + np.where(cross, t if d == axis else float((a >> d) & 1), 0.0)
                for ch in range(3):
                    sc[ch] = sc[ch] + np.where(cross, col[ch][a] + t * (col[ch][b] - col[ch][a]), 0.0)
                n = n + cross
        gx = (is_.astype(F64) + 0.5) + sp[0] / n
        gy = (js.astype(F64) + 0.5) + sp[1] / n
        gz = (ks.astype(F64) + 0.5) + sp[2] / n
        verts = np.stack([(((g2w[d, 0] * gx + g2w[d, 1] * gy) + g2w[d, 2] * gz) + g2w[d, 3]).astype(F32) for d in range(3)],
                         axis=1).reshape(V, 3)
        colours = np.stack([np.clip(np.floor(255.0 * (sc[ch] / n) + 0.5), 0.0, 255.0).astype(np.uint8) for ch in range(3)],
                           axis=1).reshape(V, 3)
    # faces: every voxel owns its +x, +y, +z edges
    valid, inside = grid[1] >= F32(min_weight), grid[0] < F32(0.0)
    cell = np.zeros((nz, ny, nx), dtype=bool)
    cell[:nz - 1, :ny - 1, :nx - 1] = active
    tri = np.zeros((nz, ny, nx, 3, 2, 3), dtype=np.int64)
    has = np.zeros((nz, ny, nx, 3), dtype=bool)

    def shifted(a, axes):  # a[p - 1 along every axis of `axes`] (index 0 wraps: masked out below)
        for ax in axes:
            a = np.roll(a, 1, axis=2 - ax)  # array axes are (z, y, x)
        return a

    idx = np.indices((nz, ny, nx))  # [k, j, i]
    coord = {0: idx[2], 1: idx[1], 2: idx[0]}
    dim = {0: nx, 1: ny, 2: nz}
    for axis in range(3):
        a1, a2 = (axis + 1) % 3, (axis + 2) % 3
        nb = lambda a: np.roll(a, -1, axis=2 - axis)  # the +1 neighbour along the axis
        ok = (coord[axis] + 1 < dim[axis]) & (coord[a1] >= 1) & (coord[a1] + 1 < dim[a1]) & (coord[a2] >= 1) & \
             (coord[a2] + 1 < dim[a2])
        ok &= valid & nb(valid) & (inside != nb(inside))
        q = [shifted(ids, (a1, a2)), shifted(ids, (a2,)), ids, shifted(ids, (a1,))]
        for qq, cc in zip(q, [shifted(cell, (a1, a2)), shifted(cell, (a2,)), cell, shifted(cell, (a1,))]):
            ok &= cc
        has[..., axis] = ok
        fwd = np.stack([np.stack([q[0], q[1], q[2]], -1), np.stack([q[0], q[2], q[3]], -1)], -2)
        rev = np.stack([np.stack([q[0], q[2], q[1]], -1), np.stack([q[0], q[3], q[2]], -1)], -2)
        tri[..., axis, :, :] = np.where(inside[..., None, None], fwd, rev)
    faces = tri[has].reshape(-1, 3).astype(np.int32)
    return verts, colours, faces, np.stack([is_, js, ks], axis=1).reshape(V, 3)


# ------------------------------------------------------------------------------------------------ analytic grids
N, VOXEL, TRUNC = 20, 0.125, 0.5
G2W = np.array([[VOXEL, 0, 0, -N * VOXEL / 2], [0, VOXEL, 0, -N * VOXEL / 2], [0, 0, VOXEL, -N * VOXEL / 2]], dtype=F64)


def centres(n=N, voxel=VOXEL):
    c = (np.arange(n) + 0.5) * voxel - n * voxel / 2
    z, y, x = np.meshgrid(c, c, c, indexing="ij")
    return x, y, z


def sphere_sdf(r=0.8):
    x, y, z = centres()
    return np.sqrt(x * x + y * y + z * z) - r


def torus_sdf(R=0.75, r=0.3):
    x, y, z = centres()
    return np.sqrt((np.sqrt(x * x + y * y) - R) ** 2 + z * z) - r


def grid_from_sdf(sdf, weight=3.0, unseen_interior=False, colour=True, trunc=TRUNC):
    """What `weight` cameras that all saw the exact surface would have fused: tsum = weight clip(sdf / trunc, -1, 1) and
    wsum = weight; with unseen_interior wsum = tsum = 0 where sdf < -trunc (no camera sees behind a surface)."""
    n = sdf.shape[0]
    g = np.zeros((PLANES,) + sdf.shape, dtype=F32)
    g[0] = (weight * np.clip(sdf / trunc, -1.0, 1.0)).astype(F32)
    g[1] = weight
    if colour:
        x, y, z = centres(n)
        near = np.abs(sdf) <= trunc
        for ch, c in enumerate((x, y, z)):
            g[2 + ch] = np.where(near, weight * np.clip(0.5 + 0.4 * c, 0, 1), 0).astype(F32)
        g[5] = np.where(near, weight, 0).astype(F32)
    if unseen_interior:
        g[:, sdf < -trunc] = 0
    return g


# ------------------------------------------------------------------------------------------------ topology
def topology(verts, faces):
    """dict: V, F, E, euler, closed (every undirected edge in exactly two triangles), oriented (every directed edge exactly
    once), volume (signed, outward normals positive)."""
    f = np.asarray(faces, dtype=np.int64)
    v = np.asarray(verts, dtype=F64)
    d = np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]])
    key = d[:, 0] * (len(v) + 1) + d[:, 1]
    lo, hi = d.min(axis=1), d.max(axis=1)
    ukey, ucount = np.unique(lo * (len(v) + 1) + hi, return_counts=True)
    vol = float(np.einsum("ij,ij->i", v[f[:, 0]], np.cross(v[f[:, 1]], v[f[:, 2]])).sum() / 6.0) if len(f) else 0.0
    return dict(V=len(v), F=len(f), E=len(ukey), euler=len(v) - len(ukey) + len(f),
                closed=bool((ucount == 2).all()), oriented=len(np.unique(key)) == len(key) and bool((lo != hi).all()),
                volume=vol)


def check_closed_surface(verts, faces, cells, g2w, euler):
    """The topology assertions shared by the CPU test (on the reference) and the GPU test (on the kernel's output)."""
    t = topology(verts, faces)
    assert t["closed"] and t["oriented"], t
    assert t["euler"] == euler, t
    assert t["volume"] > 0, t
    ginv = np.linalg.inv(np.vstack([g2w, [0, 0, 0, 1]]))
    gpos = (np.concatenate([np.asarray(verts, dtype=F64), np.ones((len(verts), 1))], axis=1) @ ginv.T)[:, :3]
    lo = np.asarray(cells, dtype=F64) + 0.5
    assert (gpos >= lo - 1e-4).all() and (gpos <= lo + 1.0 + 1e-4).all()  # every vertex inside its own cell
    return t
