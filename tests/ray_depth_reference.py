"""The float64 restatement of clm_gs_amd/csrc/ray_math.h in numpy, over whole maps, and the tilted-plane scene both ray
depth test files use.

numpy's float64 ufuncs round every product, quotient, sum and square root on their own (no contraction), so writing the
header's expressions in the header's order gives the header's bits: the tests compare bit for bit.

The tilted plane and its bound
------------------------------
A Gaussian with local axes (t1, t2, n), scales (s, s, eps), eps << s, centre m.  A ray o + t d; r = m - o.  In the local
frame d = (d_t, d_n), r = (r_t, r_n).  The ray meets the Gaussian's own plane (through m, normal n) at t_p = r_n / d_n, at
the in-plane offset h = t_p d_t - r_t from the centre.  ray_math.h returns

    t* = (d_t.r_t / s^2 + d_n r_n / eps^2) / (|d_t|^2 / s^2 + d_n^2 / eps^2)

and therefore, exactly,

    t* - t_p = -(eps/s)^2  d_t.h / (d_n^2 + (eps/s)^2 |d_t|^2),        |t* - t_p| <= (eps/s)^2 |d_t| |h| / d_n^2.

"The footprint holds the pixel" is taken as |h| <= FOOT s with FOOT = 4: an entry the rasterizer accumulates has
alpha >= 1/255, i.e. a 2-D Mahalanobis distance <= sqrt(2 ln 255) = 3.33; the 0.3 px^2 low-pass on a variance of at least
4.6 px^2 widens that by < 4 %, the affine approximation of the projection over 0.7 units at depth 5 by about 6 %: 3.65.
So for every pixel and every Gaussian that can be its median entry

    |t* - t_p| <= GEOM = (eps/s)^2 FOOT s max|d_t| / min d_n^2                                           (1)

with the maximum and minimum over the camera's pixels.  The Gaussian's own plane is the analytic plane up to the float32
rounding of its parameters (and whatever float32 activation a model applies to them): a centre that lies off the analytic
plane by delta moves its plane by delta along the normal; a normal turned by the angle phi moves the plane at the offset
|h| <= FOOT s by <= FOOT s phi.  Both are measured in float64 on the float32 rows themselves -- inputs of the code under
test, not its results -- and along the ray both are divided by d_n:

    PLACE = (max_i |n.mu_i - c0| + FOOT s max_i phi_i) / min d_n                                          (2)

bound() returns GEOM + PLACE.  With eps/s = 1e-3, s = 0.2 and slope 0.5 it is about 2.2e-6 at depth 5, where the centre
depth misses the plane by up to 0.5 x (the in-plane offset along the slope): several cm.
"""
import math

import numpy as np

FOOT = 4.0
SLOPE = 0.5
PLANE_DEPTH = 5.0
S_TANGENT, S_NORMAL, SPACING = 0.2, 2e-4, 0.25
W, H, FOCAL = 64, 48, 60.0
ORTHO_PPU = 12.0  # pixels per world unit of the orthographic camera: the pinhole's f / depth


# ------------------------------------------------------------------------------------------------ ray_math.h
def quat_to_rotmat(q):
    """q [...,4] (w,x,y,z) float64 -> the nine entries R[0..8] of ray_quat_to_rotmat, each [...]."""
    n2 = ((q[..., 0] * q[..., 0] + q[..., 1] * q[..., 1]) + q[..., 2] * q[..., 2]) + q[..., 3] * q[..., 3]
    inv = 1.0 / np.sqrt(n2)
    w, x, y, z = q[..., 0] * inv, q[..., 1] * inv, q[..., 2] * inv, q[..., 3] * inv
    return [1.0 - 2.0 * (y * y + z * z), 2.0 * (x * y - w * z), 2.0 * (x * z + w * y),
            2.0 * (x * y + w * z), 1.0 - 2.0 * (x * x + z * z), 2.0 * (y * z - w * x),
            2.0 * (x * z - w * y), 2.0 * (y * z + w * x), 1.0 - 2.0 * (x * x + y * y)]


def _dot3(a, b, c, d, e, f):
    return (a * b + c * d) + e * f


def ray_tstar(mu, q, s, cam, px, py, ortho):
    """ray_tstar of ray_math.h: mu [...,3], q [...,4], s [...,3] float64 (broadcast against px, py [...]), cam float64 [16]."""
    with np.errstate(all="ignore"):
        R = quat_to_rotmat(q)
        B, m = [None] * 9, [None] * 3
        for i in range(3):
            rv = cam[4 * i:4 * i + 4]
            for j in range(3):
                B[3 * i + j] = _dot3(rv[0], R[j], rv[1], R[3 + j], rv[2], R[6 + j])
            m[i] = _dot3(rv[0], mu[..., 0], rv[1], mu[..., 1], rv[2], mu[..., 2]) + rv[3]
        u = ((px + 0.5) - cam[14]) / cam[12]
        v = ((py + 0.5) - cam[15]) / cam[13]
        zero = np.zeros_like(u)
        o = [u, v, zero] if ortho else [zero, zero, zero]
        d = [zero, zero, zero + 1.0] if ortho else [u, v, zero + 1.0]
        r = [m[0] - o[0], m[1] - o[1], m[2] - o[2]]
        g = [_dot3(B[j], d[0], B[3 + j], d[1], B[6 + j], d[2]) / s[..., j] for j in range(3)]
        p = [_dot3(B[j], r[0], B[3 + j], r[1], B[6 + j], r[2]) / s[..., j] for j in range(3)]
        num = _dot3(g[0], p[0], g[1], p[1], g[2], p[2])
        den = _dot3(g[0], g[0], g[1], g[1], g[2], g[2])
        return num / den


def ray_depth(mu, q, s, cam, px, py, ortho, near, centre):
    """ray_depth of ray_math.h -> float32: (float32) t* where t* is finite and > near, else `centre` (float32) as it is."""
    t = ray_tstar(mu, q, s, cam, px, py, ortho)
    with np.errstate(all="ignore"):
        ok = np.isfinite(t) & (t > near)
        return np.where(ok, t.astype(np.float32), np.broadcast_to(np.asarray(centre, dtype=np.float32), t.shape))


def camera_table(viewmats, Ks):
    """float32 viewmats [C,4,4], Ks [C,3,3] -> float64 [C,16], as gsplat.ray_camera_table."""
    viewmats, Ks = np.asarray(viewmats, dtype=np.float32), np.asarray(Ks, dtype=np.float32)
    C = viewmats.shape[0]
    return np.concatenate([viewmats[:, :3, :4].reshape(C, 12), Ks[:, 0, 0:1], Ks[:, 1, 1:2], Ks[:, 0, 2:3], Ks[:, 1, 2:3]],
                          axis=1).astype(np.float64)


def ray_depth_map(means, quats, scales, viewmats, Ks, median_depth, median_ids, near=0.01, camera_model="pinhole"):
    """gsplat.ray_gaussian_depth restated: float32 numpy inputs -> float32 [C,H,W]; 0.0 where the id lies outside [0, N)."""
    means, quats, scales = (np.asarray(a, dtype=np.float32).astype(np.float64) for a in (means, quats, scales))
    median_depth, median_ids = np.asarray(median_depth, dtype=np.float32), np.asarray(median_ids)
    N = means.shape[0]
    C, Hh, Ww = median_ids.shape
    cams = camera_table(viewmats, Ks)
    out = np.zeros((C, Hh, Ww), dtype=np.float32)
    py, px = np.meshgrid(np.arange(Hh, dtype=np.float64), np.arange(Ww, dtype=np.float64), indexing="ij")
    for c in range(C):
        ids = median_ids[c]
        ok = (ids >= 0) & (ids < N)
        if N == 0 or not ok.any():
            continue
        row = np.where(ok, ids, 0)
        val = ray_depth(means[row], quats[row], scales[row], cams[c], px, py, camera_model == "ortho", float(near),
                        median_depth[c])
        out[c] = np.where(ok, val, np.float32(0.0))
    return out


# ------------------------------------------------------------------------------------------------ the tilted plane
THETA = math.atan(SLOPE)


def plane_rows(a_half=5.0, b_half=3.5, world_from_cam=None):
    """Flat Gaussians (S_TANGENT, S_TANGENT, S_NORMAL) on a SPACING grid on the plane z = PLANE_DEPTH + SLOPE x of the
    camera frame (x right, y down, z forward), local z along the plane's normal.  world_from_cam (R [3,3], t [3]) moves
    them into a world frame (the quaternion is composed with R's, which must be a half turn about x or the identity).
    -> float32 (xyz [N,3], quats [N,4] (w,x,y,z), scales [N,3]) and float64 (n: the plane's unit normal, c0: n.x on it) in
    the frame the rows are in."""
    na, nb = int(round(a_half / SPACING)), int(round(b_half / SPACING))
    a = np.arange(-na, na + 1, dtype=np.float64) * SPACING
    b = np.arange(-nb, nb + 1, dtype=np.float64) * SPACING
    bb, aa = np.meshgrid(b, a, indexing="ij")
    aa, bb = aa.reshape(-1), bb.reshape(-1)
    c, s = math.cos(THETA), math.sin(THETA)
    t1, t2, n = np.array([c, 0.0, s]), np.array([0.0, 1.0, 0.0]), np.array([-s, 0.0, c])  # t1 x t2 = n
    xyz = np.array([0.0, 0.0, PLANE_DEPTH]) + aa[:, None] * t1 + bb[:, None] * t2
    # the rotation with columns (t1, t2, n) turns by -THETA about y: q = (cos(THETA/2), 0, -sin(THETA/2), 0)
    q = np.array([math.cos(THETA / 2), 0.0, -math.sin(THETA / 2), 0.0])
    if world_from_cam is not None:
        Rw, tw = (np.asarray(v, dtype=np.float64) for v in world_from_cam)
        xyz = xyz @ Rw.T + tw
        n = Rw @ n
        if np.allclose(Rw, np.diag([1.0, -1.0, -1.0])):  # half turn about x: (0,1,0,0) * q
            q = np.array([-q[1], q[0], -q[3], q[2]])
        else:
            assert np.allclose(Rw, np.eye(3))
    xyz32 = xyz.astype(np.float32)
    quats = np.broadcast_to(q.astype(np.float32), (xyz.shape[0], 4)).copy()
    scales = np.broadcast_to(np.array([S_TANGENT, S_TANGENT, S_NORMAL], dtype=np.float32), (xyz.shape[0], 3)).copy()
    return xyz32, quats, scales, n, float(n @ xyz[0])


def pixel_rays(cam, ortho, Hh=H, Ww=W):
    """float64 camera record [16] -> (o [H,W,3], d [H,W,3]) in camera axes."""
    py, px = np.meshgrid(np.arange(Hh, dtype=np.float64), np.arange(Ww, dtype=np.float64), indexing="ij")
    u, v = (px + 0.5 - cam[14]) / cam[12], (py + 0.5 - cam[15]) / cam[13]
    z, one = np.zeros_like(u), np.ones_like(u)
    return (np.stack([u, v, z], -1), np.stack([z, z, one], -1)) if ortho else (np.stack([z, z, z], -1), np.stack([u, v, one], -1))


def plane_hit(cam, ortho, n_cam, c0, Hh=H, Ww=W):
    """The depth at which each pixel's ray meets the plane n_cam.x = c0 (camera axes), float64 [H,W]."""
    o, d = pixel_rays(cam, ortho, Hh, Ww)
    return (c0 - o @ n_cam) / (d @ n_cam)


def bound(cam, ortho, n_cam, xyz, quats, scales, n_rows, c0_rows, Hh=H, Ww=W):
    """GEOM + PLACE of the module docstring for a camera record and the plane's normal in camera axes; the float32 rows
    (xyz, quats, ACTIVATED scales sorted (s, s, eps)) and the analytic plane n_rows.x = c0_rows in the rows' frame.
    -> (bound, GEOM, PLACE)"""
    _, d = pixel_rays(cam, ortho, Hh, Ww)
    dn = np.abs(d @ n_cam)
    dt = np.sqrt(np.maximum((d * d).sum(-1) - dn * dn, 0.0))
    xyz, quats, scales = (np.asarray(a, dtype=np.float32).astype(np.float64) for a in (xyz, quats, scales))
    s_max, ratio = float(scales[:, :2].max()), float((scales[:, 2] / scales[:, :2].min(-1)).max())
    geom = ratio ** 2 * FOOT * s_max * float(dt.max()) / float(dn.min()) ** 2
    Rq = quat_to_rotmat(quats)
    n_own = np.stack([Rq[2], Rq[5], Rq[8]], -1)  # the local z axis
    phi = np.arcsin(np.minimum(np.linalg.norm(np.cross(n_own, n_rows), axis=-1), 1.0))
    place = (float(np.abs(xyz @ n_rows - c0_rows).max()) + FOOT * s_max * float(phi.max())) / float(dn.min())
    return geom + place, geom, place


def pinhole_record():
    return np.array([1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, FOCAL, FOCAL, W / 2.0, H / 2.0], dtype=np.float64)


def ortho_record():
    return np.array([1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, ORTHO_PPU, ORTHO_PPU, W / 2.0, H / 2.0], dtype=np.float64)
