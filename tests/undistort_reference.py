"""Lens undistortion in numpy float64 ("Lens distortion"), written from the formulae, every product
and sum rounded on its own in the order written.  lens = (fx, fy, cx, cy, k1, k2, k3, k4, p1, p2), intrinsics in pixels
of the source image, COLMAP's convention (the centre of the top-left pixel is at (0.5, 0.5)).  For output pixel (i, j) of
the Ho x Wo centred pinhole with focal lengths fxo, fyo:

    x = (j + 0.5 - Wo/2) / fxo,   y = (i + 0.5 - Ho/2) / fyo,   r2 = x*x + y*y
    perspective:  rad  = 1 + r2*(k1 + r2*k2)
                  mono = 1 + r2*(3*k1 + r2*5*k2)
                  xd = x*rad + 2*p1*x*y + p2*(r2 + 2*x*x)
                  yd = y*rad + p1*(r2 + 2*y*y) + 2*p2*x*y
    fisheye:      r = sqrt(r2),  th = atan(r),  t2 = th*th
                  rad  = 1 + t2*(k1 + t2*(k2 + t2*(k3 + t2*k4)))
                  mono = 1 + t2*(3*k1 + t2*(5*k2 + t2*(7*k3 + t2*9*k4)))
                  s = th*rad/r   (s = 1 where r < 1e-12),   xd = x*s,  yd = y*s
    u = fx*xd + cx - 0.5,   v = fy*yd + cy - 0.5
    valid:  mono > 0,  -tau <= u <= Ws-1+tau,  -tau <= v <= Hs-1+tau          (tau = 2^-20)
            and, with a source mask, all four taps non-zero in it
    u, v clamped into the source;  x0 = min(floor(u), max(Ws-2, 0)),  x1 = min(x0+1, Ws-1),  a = u - x0;  y0, y1, b likewise
    val = (1-b)*((1-a)*p[y0,x0] + a*p[y0,x1]) + b*((1-a)*p[y1,x0] + a*p[y1,x1]);   out = floor(val + 0.5) where valid, else 0

Besides the image and the valid map, undistort() returns the BAND: the pixels where a last-ulp difference could
legitimately flip a result -- |mono| < 1e-9, u or v within 1e-6 of -tau or size-1+tau, val + 0.5 within 1e-9 of an integer
(in any plane of a valid pixel)."""
import numpy as np

TAU = 2.0 ** -20


def mapping(lens, fisheye, fxo, fyo, Ho, Wo):
    """(u, v, mono), float64 [Ho, Wo] each."""
    fx, fy, cx, cy, k1, k2, k3, k4, p1, p2 = (np.float64(t) for t in lens)
    fxo, fyo = np.float64(fxo), np.float64(fyo)
    j, i = np.meshgrid(np.arange(Wo, dtype=np.float64), np.arange(Ho, dtype=np.float64))
    x = (j + 0.5 - np.float64(Wo) / 2.0) / fxo
    y = (i + 0.5 - np.float64(Ho) / 2.0) / fyo
    r2 = x * x + y * y
    if fisheye:
        r = np.sqrt(r2)
        th = np.arctan(r)
        t2 = th * th
        rad = 1.0 + t2 * (k1 + t2 * (k2 + t2 * (k3 + t2 * k4)))
        mono = 1.0 + t2 * (3.0 * k1 + t2 * (5.0 * k2 + t2 * (7.0 * k3 + t2 * 9.0 * k4)))
        with np.errstate(divide="ignore", invalid="ignore"):
            s = np.where(r < 1e-12, 1.0, th * rad / r)
        xd, yd = x * s, y * s
    else:
        rad = 1.0 + r2 * (k1 + r2 * k2)
        mono = 1.0 + r2 * (3.0 * k1 + r2 * 5.0 * k2)
        xd = x * rad + 2.0 * p1 * x * y + p2 * (r2 + 2.0 * x * x)
        yd = y * rad + p1 * (r2 + 2.0 * y * y) + 2.0 * p2 * x * y
    return fx * xd + cx - 0.5, fy * yd + cy - 0.5, mono


def in_bounds(u, v, Hs, Ws):
    return (u >= -TAU) & (u <= Ws - 1 + TAU) & (v >= -TAU) & (v <= Hs - 1 + TAU)


def _taps(t, n):
    t = np.clip(t, 0.0, float(n - 1))
    i0 = np.minimum(np.floor(t).astype(np.int64), max(n - 2, 0))
    i1 = np.minimum(i0 + 1, n - 1)
    return i0, i1, t - i0.astype(np.float64)


def undistort(src, lens, fisheye, fxo, fyo, out_size=None, src_mask=None):
    """src uint8 / uint16 [P,Hs,Ws] or [Hs,Ws] -> (image of the same dtype and rank at out_size, valid uint8 [Ho,Wo] of
    255 / 0, band bool [Ho,Wo])."""
    src = np.asarray(src)
    planes = src if src.ndim == 3 else src[None]
    Hs, Ws = planes.shape[-2:]
    Ho, Wo = (Hs, Ws) if out_size is None else out_size
    u, v, mono = mapping(lens, fisheye, fxo, fyo, Ho, Wo)
    valid = (mono > 0) & in_bounds(u, v, Hs, Ws)
    band = np.abs(mono) < 1e-9
    for t, n in ((u, Ws), (v, Hs)):
        band |= (np.abs(t + TAU) < 1e-6) | (np.abs(t - (n - 1 + TAU)) < 1e-6)
    x0, x1, a = _taps(u, Ws)
    y0, y1, b = _taps(v, Hs)
    if src_mask is not None:
        m = np.asarray(src_mask) != 0
        valid &= m[y0, x0] & m[y0, x1] & m[y1, x0] & m[y1, x1]
    out = np.zeros((planes.shape[0], Ho, Wo), dtype=src.dtype)
    for k, p in enumerate(planes.astype(np.float64)):
        val = (1.0 - b) * ((1.0 - a) * p[y0, x0] + a * p[y0, x1]) + b * ((1.0 - a) * p[y1, x0] + a * p[y1, x1])
        band |= valid & (np.abs((val + 0.5) - np.rint(val + 0.5)) < 1e-9)   # (an invalid pixel is 0 whatever val is)
        out[k] = np.where(valid, np.floor(val + 0.5), 0.0).astype(src.dtype)
    return (out if src.ndim == 3 else out[0]), np.where(valid, 255, 0).astype(np.uint8), band


# ------------------------------------------------------------------------------- the cases of the GPU test, and their inputs
SIZES = ((1, 1), (2, 2), (3, 5), (7, 9), (16, 16), (17, 33), (65, 47), (5, 1031), (1031, 5))   # (H, W)
ZOOMS = (1.0, 0.8)
FOLDING_K1 = -2.5   # 1 + 3 k1 r2 <= 0 from r2 = 0.134: the corners of the larger frames fold back into the image
# name -> (COLMAP model, distortion parameters after the intrinsics)
LENSES = (
    ("pinhole", "PINHOLE", ()),
    ("simple_radial", "SIMPLE_RADIAL", (-0.12,)),
    ("radial", "RADIAL", (-0.12, 0.03)),
    ("opencv", "OPENCV", (-0.12, 0.03, 0.004, -0.003)),
    ("pincushion", "RADIAL", (0.15, 0.02)),
    ("folding", "SIMPLE_RADIAL", (FOLDING_K1,)),
    ("fisheye", "OPENCV_FISHEYE", (-0.04, 0.01, -0.003, 0.0007)),
)


def colmap_params(model, dist, H, W):
    """The COLMAP parameter list of a test lens on an H x W image: f = 1.2 max(W, H), fy = 1.07 f, an off-centre
    principal point."""
    f = 1.2 * max(W, H)
    cx, cy = W / 2 + 0.37, H / 2 - 0.23
    head = (f, cx, cy) if model in ("SIMPLE_RADIAL", "RADIAL") else (f, 1.07 * f, cx, cy)
    return head + tuple(dist)


def record(model, dist, H, W):
    """(lens record of ten doubles, fisheye) of a test lens, written out by hand (the product's Lens is held to it)."""
    f = 1.2 * max(W, H)
    cx, cy = W / 2 + 0.37, H / 2 - 0.23
    d = tuple(float(t) for t in dist)
    if model == "PINHOLE":
        fy, k = 1.07 * f, (0.0,) * 6                            # k1 k2 k3 k4 p1 p2
    elif model == "SIMPLE_RADIAL":
        fy, k = f, (d[0], 0.0, 0.0, 0.0, 0.0, 0.0)
    elif model == "RADIAL":
        fy, k = f, (d[0], d[1], 0.0, 0.0, 0.0, 0.0)
    elif model == "OPENCV":
        fy, k = 1.07 * f, (d[0], d[1], 0.0, 0.0, d[2], d[3])
    else:
        assert model == "OPENCV_FISHEYE", model
        fy, k = 1.07 * f, (d[0], d[1], d[2], d[3], 0.0, 0.0)
    return (f, fy, cx, cy) + k, model == "OPENCV_FISHEYE"


SEED = 2   # (chosen so that the band cap of tests/test_undistort_cpu.py holds: the cap is a condition on the inputs)


def inputs(H, W, lens_index, zoom_index):
    """Seeded random (uint8 [3,H,W], uint16 [H,W]) of a case."""
    rng = np.random.default_rng(SEED + 1000 * (H * 2048 + W) + 10 * lens_index + zoom_index)
    return (rng.integers(0, 256, size=(3, H, W)).astype(np.uint8), rng.integers(0, 65536, size=(H, W)).astype(np.uint16))
