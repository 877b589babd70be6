"""Float64 / Python-int restatement of the compressed-model format (clm_gs_amd/compress.py, csrc/vq.hip): no GPU, no
product code.  What the kernels and the host module are held to by tests/test_compress_cpu.py and
tests/test_gpu_compress.py.

Layout of an SH row [48]: coefficient-major, the DC in columns 0..2, the 45 higher-order coefficients in columns 3..47.
"""
import math

import numpy as np

CHUNK = 256
BITS = dict(pos_bits=16, scale_bits=8, opacity_bits=8, rot_bits=8, dc_bits=8)
RSQRT2 = 0.7071067811865476


# ---------------------------------------------------------------- vector quantisation
def dist64(rows, codebook):
    """[N,K] float64 squared distances over columns 3..47 (brute force, (x - c)^2 summed)."""
    x = np.asarray(rows, np.float64)[:, 3:]
    c = np.asarray(codebook, np.float64)[:, 3:]
    out = np.empty((x.shape[0], c.shape[0]), np.float64)
    step = max(1, (1 << 20) // max(1, c.shape[0]))  # about 2^20 x 45 doubles at a time
    for a in range(0, x.shape[0], step):
        d = x[a:a + step, None, :] - c[None, :, :]
        out[a:a + step] = (d * d).sum(-1)
    return out


def assign64(rows, codebook):
    """-> (idx int64 [N], dist float64 [N]): the nearest centroid, the lowest index on an exact tie."""
    d = dist64(rows, codebook)
    idx = d.argmin(1)  # numpy: the first minimum
    return idx, d[np.arange(d.shape[0]), idx]


def vq_scale(n, max_abs):
    """2^(61 - e), e the binary exponent of n * max_abs; 1 for an all-zero table."""
    prod = float(n) * float(max_abs)
    assert math.isfinite(prod)
    if prod <= 0.0:
        return 1.0
    return math.ldexp(1.0, max(-900, min(900, 61 - math.frexp(prod)[1])))


def update_int(rows, idx, codebook, scale):
    """The Lloyd update as the kernel defines it: per centroid the Python-int sum of rint(x * scale) over its rows,
    float32(float64(sum) / count / scale); a centroid without rows keeps columns 3..47; columns 0..2 are 0.
    -> (codebook float32 [K,48], counts int64 [K])."""
    rows = np.asarray(rows, np.float32)
    idx = np.asarray(idx).astype(np.int64)
    K = codebook.shape[0]
    q = np.rint(rows[:, 3:].astype(np.float64) * scale)
    assert np.abs(q).max(initial=0.0) < 2.0 ** 62
    q = q.astype(np.int64)
    out = np.array(codebook, np.float32, copy=True)
    out[:, :3] = 0.0
    counts = np.bincount(idx, minlength=K).astype(np.int64)
    order = np.argsort(idx, kind="stable")
    bounds = np.concatenate(([0], np.cumsum(counts)))
    for k in range(K):
        if counts[k] == 0:
            continue
        sel = q[order[bounds[k]:bounds[k + 1]]]
        for j in range(45):
            total = sum(int(v) for v in sel[:, j])  # Python ints: no overflow, no order
            out[k, 3 + j] = np.float32(float(total) / float(int(counts[k])) / scale)
    return out, counts


def fit_codebook64(shs48, K, iters, sample=1 << 22):
    """Lloyd on every ceil(N / sample)-th row, K clamped to the sample, the initial codebook K sample rows at an even
    stride; assignment in float64, update as update_int.  -> (codebook float32 [K,48], history)."""
    shs48 = np.asarray(shs48, np.float32)
    n = shs48.shape[0]
    stride = -(-n // int(sample))
    samp = shs48[::stride]
    m = samp.shape[0]
    K = min(int(K), m)
    cb = samp[(np.arange(K, dtype=np.int64) * m) // K].copy()
    cb[:, :3] = 0.0
    scale = vq_scale(m, float(np.abs(samp).max(initial=0.0)))
    history = []
    for _ in range(int(iters)):
        idx, d = assign64(samp, cb)
        history.append(float(d.sum()))
        cb, _ = update_int(samp, idx, cb, scale)
    return cb, history


# ---------------------------------------------------------------- scalar quantisers
def code_dtype(bits):
    return np.uint8 if bits <= 8 else np.uint16


def quantise(x, lo, hi, bits):
    """code = rint((x - lo) / (hi - lo) * (2^b - 1)), 0 where hi == lo; float64 arithmetic on float32 lo / hi."""
    x, lo, hi = (np.asarray(v, np.float64) for v in (x, lo, hi))
    span = hi - lo
    levels = float((1 << bits) - 1)
    t = np.where(span > 0, (x - lo) / np.where(span > 0, span, 1.0), 0.0)
    return np.rint(np.clip(t, 0.0, 1.0) * levels).astype(code_dtype(bits))


def dequantise(code, lo, hi, bits):
    lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
    return (lo + np.asarray(code, np.float64) / float((1 << bits) - 1) * (hi - lo)).astype(np.float32)


def chunk_bounds(x, chunk=CHUNK):
    """float32 min and max of every `chunk` consecutive rows: ([C,D], [C,D])."""
    x = np.asarray(x, np.float32)
    starts = np.arange(0, x.shape[0], chunk)
    return np.minimum.reduceat(x, starts, axis=0), np.maximum.reduceat(x, starts, axis=0)


def quat_encode(rot, bits):
    """-> (codes [N,3], largest [N] uint8): normalised, sign so that the largest |component| is positive (the first on a
    tie), the three others in order, each over [-1/sqrt 2, 1/sqrt 2]."""
    q = np.asarray(rot, np.float64)
    q = q / np.linalg.norm(q, axis=1, keepdims=True)
    big = np.abs(q).argmax(1)
    q = q * np.where(q[np.arange(len(q)), big] < 0, -1.0, 1.0)[:, None]
    rest = np.stack([np.delete(r, b) for r, b in zip(q, big)]) if len(q) else np.zeros((0, 3))
    lo, hi = np.float32(-RSQRT2), np.float32(RSQRT2)
    return quantise(rest, lo, hi, bits), big.astype(np.uint8)


def quat_decode(codes, big, bits):
    lo, hi = np.float32(-RSQRT2), np.float32(RSQRT2)
    rest = dequantise(codes, lo, hi, bits).astype(np.float64)
    w = np.sqrt(np.maximum(0.0, 1.0 - (rest * rest).sum(1)))
    out = np.empty((len(rest), 4), np.float64)
    for i in range(len(rest)):
        out[i] = np.insert(rest[i], int(big[i]), w[i])
    return out.astype(np.float32)


# ---------------------------------------------------------------- the whole pipeline
def morton_order64(xyz, bits=16):
    """Z-order of (x, y), `bits` per axis, ties in row order."""
    p = np.asarray(xyz, np.float64)[:, :2]
    lo, hi = p.min(0), p.max(0)
    q = np.rint((p - lo) / np.maximum(hi - lo, 1e-30) * ((1 << bits) - 1)).astype(np.uint64)
    code = np.zeros(len(p), np.uint64)
    for b in range(bits):
        code |= ((q[:, 0] >> np.uint64(b)) & np.uint64(1)) << np.uint64(2 * b)
        code |= ((q[:, 1] >> np.uint64(b)) & np.uint64(1)) << np.uint64(2 * b + 1)
    return np.argsort(code, kind="stable")


def pipeline64(rows, K, iters, sample=1 << 22, bits=BITS, order=None):
    """compress -> decompress of a load_ply-style dict of numpy arrays, everything in float64 / Python ints.
    -> (dict of float32 arrays in Morton order, order, codebook, idx)."""
    if order is None:
        order = morton_order64(rows["xyz"])
    r = {k: np.asarray(v, np.float32)[order] for k, v in rows.items()}
    cb, _ = fit_codebook64(r["shs48"], K, iters, sample)
    idx, _ = assign64(r["shs48"], cb)
    out = {}
    lo, hi = chunk_bounds(r["xyz"])
    rep = np.arange(len(order)) // CHUNK
    out["xyz"] = dequantise(quantise(r["xyz"], lo[rep], hi[rep], bits["pos_bits"]), lo[rep], hi[rep], bits["pos_bits"])
    lo, hi = chunk_bounds(r["scaling"])
    out["scaling"] = dequantise(quantise(r["scaling"], lo[rep], hi[rep], bits["scale_bits"]), lo[rep], hi[rep],
                                bits["scale_bits"])
    lo, hi = r["opacity"].min(), r["opacity"].max()
    out["opacity"] = dequantise(quantise(r["opacity"], lo, hi, bits["opacity_bits"]), lo, hi, bits["opacity_bits"])
    out["rotation"] = quat_decode(*quat_encode(r["rotation"], bits["rot_bits"]), bits["rot_bits"])
    dc = r["shs48"][:, :3]
    lo, hi = dc.min(0), dc.max(0)
    sh = cb[idx].copy()
    sh[:, :3] = dequantise(quantise(dc, lo, hi, bits["dc_bits"]), lo, hi, bits["dc_bits"])
    out["shs48"] = sh
    return out, order, cb, idx


# ---------------------------------------------------------------- the bounds a round trip is held to
def ulp32(v):
    return float(np.spacing(np.float32(abs(float(v)))))


def quantiser_bound(lo, hi, bits):
    """|x - dq(q(x))| <= half a step, (hi - lo) / (2^b - 1) / 2, plus one float32 ulp of max(|lo|, |hi|) (the cast of
    the dequantised value, which lies in [lo, hi], to float32; the float64 arithmetic in front of it is far below)."""
    lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
    big = np.maximum(np.abs(lo), np.abs(hi)).astype(np.float32)
    return (hi - lo) / float((1 << bits) - 1) / 2.0 + np.spacing(big).astype(np.float64)


def check_round_trip(orig, dec, bits=BITS, chunk=CHUNK):
    """orig: the rows in their stored order (numpy float32), dec: what decompress gave.  Asserts every scalar field
    inside quantiser_bound (per chunk or global, as the field is defined) and the quaternion, up to sign, inside
    e = quantiser_bound(-1/sqrt 2, 1/sqrt 2) for the three stored components and 5 e for the rebuilt largest one:
    w = sqrt(1 - s), s the sum of the three squares, |s - s'| <= sum |c - c'| (|c| + |c'|) <= 3 e (sqrt 2 + e) and
    w + w' >= 2 * 1/2 - 5 e (the largest of four components of a unit vector is >= 1/2), so |w - w'| <= 3 e (sqrt 2 + e) /
    (1 - 5 e) < 5 e for e < 0.02, i.e. from 6 bits up; the bound used is the un-simplified expression."""
    n = orig["xyz"].shape[0]
    rep = np.arange(n) // chunk
    for key, b in (("xyz", "pos_bits"), ("scaling", "scale_bits")):
        lo, hi = chunk_bounds(orig[key], chunk)
        err = np.abs(np.asarray(dec[key], np.float64) - orig[key].astype(np.float64))
        assert (err <= quantiser_bound(lo, hi, bits[b])[rep]).all(), key
    op = orig["opacity"].reshape(n)
    err = np.abs(np.asarray(dec["opacity"], np.float64).reshape(n) - op.astype(np.float64))
    assert (err <= quantiser_bound(op.min(), op.max(), bits["opacity_bits"])).all(), "opacity"
    dc = orig["shs48"][:, :3]
    err = np.abs(np.asarray(dec["shs48"], np.float64)[:, :3] - dc.astype(np.float64))
    assert (err <= quantiser_bound(dc.min(0), dc.max(0), bits["dc_bits"])[None]).all(), "dc"
    q = orig["rotation"].astype(np.float64)
    q = q / np.linalg.norm(q, axis=1, keepdims=True)
    big = np.abs(q).argmax(1)
    q = q * np.where(q[np.arange(n), big] < 0, -1.0, 1.0)[:, None]
    e = float(quantiser_bound(np.float32(-RSQRT2), np.float32(RSQRT2), bits["rot_bits"]))
    tol = np.full((n, 4), e)
    tol[np.arange(n), big] = 3 * e * (math.sqrt(2) + e) / (1 - 5 * e) + ulp32(1.0)
    assert (np.abs(np.asarray(dec["rotation"], np.float64) - q) <= tol).all(), "rotation"
