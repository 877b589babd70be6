"""Compressed model export ("Compressed models"): the 45 higher-order SH coefficients of a row are
replaced by a uint16 index into a k-means codebook (csrc/vq.hip: nearest-centroid search on the f32 MFMA, Lloyd update
in fixed point), the small attributes are quantised to a few bits per value against per-chunk or global bounds, and the
rows are stored in Morton order.  One .npz (numpy's deflate) holds the arrays and a JSON meta string.

    arrays, meta = compress(io_ply.load_ply(path))          # needs the GPU (fit_codebook, vq_assign)
    save_compressed("model.vq.npz", arrays, meta)
    rows = load_compressed("model.vq.npz")                  # the dict io_ply.load_ply returns (io_ply.load_model)

Everything but the codebook fit and the assignment is numpy plumbing on the host.
"""
import json
import time

import numpy as np
import torch

FORMAT_VERSION = 1
CHUNK = 256
KEYS = ("xyz", "shs48", "opacity", "scaling", "rotation")
BITS = dict(pos_bits=16, scale_bits=8, opacity_bits=8, rot_bits=8, dc_bits=8)
_RSQRT2 = np.float32(0.7071067811865476)  # a component that is not the largest lies in [-1/sqrt 2, 1/sqrt 2]


# ---------------------------------------------------------------- scalar quantisers
def _code_dtype(bits):
    return np.uint8 if bits <= 8 else np.uint16


def check_bits(bits):
    """The five bit widths as a dict (missing ones: BITS); each must be an integer in [1, 16]."""
    out = dict(BITS)
    for k, v in (bits or {}).items():
        if k not in BITS:
            raise ValueError(f"compress: unknown bit width {k!r}; known: {', '.join(BITS)}")
        if v is not None:
            out[k] = v
    for k, v in out.items():
        if int(v) != v or not 1 <= int(v) <= 16:
            raise ValueError(f"compress: --{k} must be an integer in [1, 16], got {v}")
        out[k] = int(v)
    return out


def quantise(x, lo, hi, bits):
    """code = rint((x - lo) / (hi - lo) * (2^bits - 1)) in float64, 0 where hi == lo; lo / hi broadcast against x."""
    x, lo, hi = (np.asarray(v, np.float64) for v in (x, lo, hi))
    span = hi - lo
    ok = span > 0
    t = np.where(ok, (x - lo) / np.where(ok, span, 1.0), 0.0)
    return np.rint(np.clip(t, 0.0, 1.0) * float((1 << bits) - 1)).astype(_code_dtype(bits))


def dequantise(code, lo, hi, bits):
    """float32(lo + code / (2^bits - 1) * (hi - lo)), in float64 up to the cast."""
    lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
    return (lo + np.asarray(code, np.float64) / float((1 << bits) - 1) * (hi - lo)).astype(np.float32)


def chunk_bounds(x, chunk=CHUNK):
    """float32 (min, max), each [ceil(N / chunk), D], of every `chunk` consecutive rows of x [N,D]."""
    x = np.asarray(x, np.float32)
    starts = np.arange(0, x.shape[0], chunk)
    return np.minimum.reduceat(x, starts, axis=0), np.maximum.reduceat(x, starts, axis=0)


def quat_encode(rot, bits):
    """-> (codes [N,3], largest uint8 [N]): the quaternion normalised, its sign fixed so that the component of largest
    magnitude (the first on a tie) is positive, and the three OTHER components, in order, quantised over
    [-1/sqrt 2, 1/sqrt 2]."""
    q = np.asarray(rot, np.float64)
    norm = np.linalg.norm(q, axis=1, keepdims=True)
    if not (np.isfinite(norm).all() and (norm > 0).all()):
        raise ValueError("compress: a rotation quaternion is zero or not finite")
    q = q / norm
    n = q.shape[0]
    big = np.abs(q).argmax(1)
    q = q * np.where(q[np.arange(n), big] < 0, -1.0, 1.0)[:, None]
    keep = np.ones((n, 4), bool)
    keep[np.arange(n), big] = False
    return quantise(q[keep].reshape(n, 3), -_RSQRT2, _RSQRT2, bits), big.astype(np.uint8)


def quat_decode(codes, big, bits):
    """float32 [N,4]: the three stored components and the largest as sqrt(1 - their squares)."""
    rest = dequantise(codes, -_RSQRT2, _RSQRT2, bits).astype(np.float64)
    n = rest.shape[0]
    keep = np.ones((n, 4), bool)
    keep[np.arange(n), np.asarray(big, np.int64)] = False
    out = np.empty((n, 4), np.float64)
    out[keep] = rest.reshape(-1)
    out[~keep] = np.sqrt(np.maximum(0.0, 1.0 - (rest * rest).sum(1)))
    return out.astype(np.float32)


# ---------------------------------------------------------------- codebook
def _check_degree3(shs48):
    if shs48.dim() != 2 or shs48.shape[1] != 48:
        raise ValueError(f"compress: SH degree 3 only (rows of 48 floats: 3 DC + 45 higher-order coefficients), got rows of "
                         f"{tuple(shs48.shape)[1:]} floats; SH degrees other than 3 are not supported")


@torch.no_grad()
def fit_codebook(shs48, K=65536, iters=10, sample=1 << 22, seed=0):
    """Lloyd's k-means on the higher-order SH coefficients -> (codebook float32 [K,48] on the device, columns 0..2 zero;
    history: the summed squared distance after each assignment).  shs48: float32 [N,48] on the device, in Morton order
    (a trained model's table is; sort a cold .ply with utils.morton_order first).  The fit runs on every
    ceil(N / sample)-th row; K is clamped to the number of those; the initial codebook is K of them at an even stride
    (duplicates allowed; a centroid that loses every row keeps its value).  Nothing is random: `seed` is accepted for
    the interface's sake and the same rows give the same bits (clm_kernels.vq_update)."""
    from . import clm_kernels as CK
    _check_degree3(shs48)
    n = int(shs48.shape[0])
    if n < 1:
        raise ValueError("compress: a model without rows cannot be compressed")
    sample, iters = int(sample), int(iters)
    if sample < 1 or iters < 0 or int(K) < 1:
        raise ValueError(f"compress: --codebook and --sample must be >= 1 and --iters >= 0, got {K}, {sample}, {iters}")
    stride = -(-n // sample)
    samp = shs48[::stride].contiguous()
    m = int(samp.shape[0])
    K = min(int(K), m, CK.VQ_MAX_K)
    pick = (torch.arange(K, dtype=torch.int64, device=samp.device) * m) // K
    cb = samp[pick].contiguous()
    cb[:, :3] = 0.0
    lo, hi = torch.aminmax(samp)
    scale = CK.vq_scale(m, max(-float(lo), float(hi)))
    history = []
    for _ in range(iters):
        idx, dist = CK.vq_assign(samp, cb, want_dist=True)
        history.append(float(dist.sum(dtype=torch.float64)))
        cb, _ = CK.vq_update(samp, idx, cb, scale=scale)
    return cb, history


# ---------------------------------------------------------------- encode / decode
def _np32(t):
    return np.ascontiguousarray(t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else t, dtype=np.float32)


def encode(rows, sh_idx, codebook, bits=None, chunk=CHUNK):
    """The file's arrays from rows ALREADY in their stored (Morton) order, the SH index of every row and the codebook
    [K,48] (or [K,45]): pure numpy.  -> (arrays, meta)."""
    bits = check_bits(bits)
    r = {k: _np32(rows[k]) for k in KEYS}
    n = r["xyz"].shape[0]
    if r["shs48"].ndim != 2 or r["shs48"].shape[1] != 48:
        raise ValueError(f"compress: SH degree 3 only (rows of 48 floats), got rows of {r['shs48'].shape[1:]} floats; "
                         "SH degrees other than 3 are not supported")
    cb = _np32(codebook)
    cb = cb[:, 3:] if cb.shape[1] == 48 else cb
    K = cb.shape[0]
    if cb.shape[1] != 45 or not 1 <= K <= 65536:
        raise ValueError(f"compress: the codebook must be [K,45] or [K,48] with 1 <= K <= 65536, got {cb.shape}")
    sh_idx = np.asarray(sh_idx.detach().cpu().numpy() if isinstance(sh_idx, torch.Tensor) else sh_idx)
    if sh_idx.shape != (n,) or (n and (sh_idx.min() < 0 or sh_idx.max() >= K)):
        raise ValueError(f"compress: {n} SH indices in [0, {K}) expected")
    for k in KEYS:
        if not np.isfinite(r[k]).all():
            raise ValueError(f"compress: {k} holds a value that is not finite")
    rep = np.arange(n) // chunk
    a = {}
    a["pos_lo"], a["pos_hi"] = chunk_bounds(r["xyz"], chunk)
    a["pos"] = quantise(r["xyz"], a["pos_lo"][rep], a["pos_hi"][rep], bits["pos_bits"])
    a["scale_lo"], a["scale_hi"] = chunk_bounds(r["scaling"], chunk)
    a["scale"] = quantise(r["scaling"], a["scale_lo"][rep], a["scale_hi"][rep], bits["scale_bits"])
    op = r["opacity"].reshape(n)
    a["opacity_lohi"] = np.array([op.min(), op.max()], np.float32)
    a["opacity"] = quantise(op, a["opacity_lohi"][0], a["opacity_lohi"][1], bits["opacity_bits"])
    a["rot"], a["rot_big"] = quat_encode(r["rotation"], bits["rot_bits"])
    dc = r["shs48"][:, :3]
    a["dc_lohi"] = np.stack([dc.min(0), dc.max(0)]).astype(np.float32)
    a["dc"] = quantise(dc, a["dc_lohi"][0], a["dc_lohi"][1], bits["dc_bits"])
    a["sh_idx"] = sh_idx.astype(np.uint16)
    a["codebook"] = np.ascontiguousarray(cb, np.float32)
    meta = dict(version=FORMAT_VERSION, N=int(n), K=int(K), chunk=int(chunk), sh_degree=3, **bits)
    return a, meta


def expected_nbytes(meta):
    """The summed nbytes of the arrays of a file with this meta: per row 3 position, 3 scale, 1 opacity, 3 rotation and
    3 DC codes (1 byte each up to 8 bits, 2 above), 1 byte for the largest quaternion component and 2 for the SH index;
    per chunk 2 x 3 float32 bounds for positions and for scales; 2 + 6 float32 global bounds; the codebook K x 45 x 4."""
    n, K, chunks = meta["N"], meta["K"], -(-meta["N"] // meta["chunk"])
    w = lambda b: 1 if meta[b] <= 8 else 2
    per_row = 3 * w("pos_bits") + 3 * w("scale_bits") + w("opacity_bits") + 3 * w("rot_bits") + 3 * w("dc_bits") + 1 + 2
    return n * per_row + chunks * 2 * (3 * 4 + 3 * 4) + (2 + 6) * 4 + K * 45 * 4


def check_meta(meta):
    if meta.get("version") != FORMAT_VERSION:
        raise ValueError(f"compressed model: format version {meta.get('version')!r} is unknown (this build reads version "
                         f"{FORMAT_VERSION})")
    if meta.get("sh_degree", 3) != 3:
        raise ValueError(f"compressed model: SH degree {meta.get('sh_degree')} is not supported (degree 3 only)")
    return meta


def decompress(arrays, meta):
    """-> the dict io_ply.load_ply returns (xyz [n,3], shs48 [n,48], opacity [n,1], scaling [n,3], rotation [n,4] float32
    host tensors), rows in the file's (Morton) order."""
    check_meta(meta)
    n, chunk = int(meta["N"]), int(meta["chunk"])
    rep = np.arange(n) // chunk
    a = arrays
    xyz = dequantise(a["pos"], a["pos_lo"][rep], a["pos_hi"][rep], meta["pos_bits"])
    scaling = dequantise(a["scale"], a["scale_lo"][rep], a["scale_hi"][rep], meta["scale_bits"])
    opacity = dequantise(a["opacity"], a["opacity_lohi"][0], a["opacity_lohi"][1], meta["opacity_bits"]).reshape(n, 1)
    rotation = quat_decode(a["rot"], a["rot_big"], meta["rot_bits"])
    sh = np.empty((n, 48), np.float32)
    sh[:, :3] = dequantise(a["dc"], a["dc_lohi"][0], a["dc_lohi"][1], meta["dc_bits"])
    sh[:, 3:] = np.asarray(a["codebook"], np.float32)[np.asarray(a["sh_idx"], np.int64)]
    t = lambda v: torch.from_numpy(np.ascontiguousarray(v, dtype=np.float32))
    return dict(xyz=t(xyz.reshape(n, 3)), shs48=t(sh), opacity=t(opacity), scaling=t(scaling.reshape(n, 3)),
                rotation=t(rotation))


@torch.no_grad()
def compress(rows, K=65536, iters=10, sample=1 << 22, bits=None, timings=None):
    """rows: the dict io_ply.load_ply returns (host or device tensors) -> (arrays, meta) as save_compressed takes them;
    meta also carries what the size line reports (`history`, `empty`, `distortion`).  The rows are put in Morton order
    (utils.morton_order: the library's clmgs_morton_order on the device), the codebook is fitted on a sample of them
    (fit_codebook) and every row is assigned once more against the final codebook.  `timings`: a dict that receives the
    wall time of the fit, the full assignment and the quantisation."""
    from . import clm_kernels as CK
    from . import utils
    bits = check_bits(bits)
    _check_degree3(rows["shs48"])
    dev = torch.device("cuda")
    t0 = time.perf_counter()
    order = utils.morton_order(rows["xyz"].detach().float().to(dev))
    shs = rows["shs48"].detach().to(dev, torch.float32)[order].contiguous()
    cb, history = fit_codebook(shs, K, iters, sample)
    torch.cuda.synchronize(dev)
    t1 = time.perf_counter()
    idx, dist = CK.vq_assign(shs, cb, want_dist=True)
    counts = torch.bincount(idx.long(), minlength=cb.shape[0])
    distortion = float(dist.sum(dtype=torch.float64)) / max(1, shs.shape[0])
    empty = int((counts == 0).sum())
    t2 = time.perf_counter()
    order_h = order.cpu()
    sorted_rows = {k: rows[k].detach().cpu()[order_h] for k in KEYS if k != "shs48"}
    sorted_rows["shs48"] = shs.cpu()
    arrays, meta = encode(sorted_rows, idx.cpu(), cb.cpu(), bits)
    t3 = time.perf_counter()
    meta.update(history=history, empty=empty, distortion=distortion)
    if timings is not None:
        timings.update(fit_s=t1 - t0, assign_s=t2 - t1, quantise_s=t3 - t2)
    return arrays, meta


# ---------------------------------------------------------------- the file
def save_compressed(path, arrays, meta):
    """One numpy .npz (deflate): the arrays under their names and the meta as a JSON string under "meta"."""
    check_meta(meta)
    with open(path, "wb") as f:  # (a file object: numpy does not append ".npz" to the name)
        np.savez_compressed(f, meta=np.array(json.dumps(meta)), **arrays)


def read_compressed(path):
    """-> (arrays, meta) as they were saved; an unknown format version is refused."""
    with np.load(path, allow_pickle=False) as z:
        if "meta" not in z.files:
            raise ValueError(f"{path}: not a compressed model (no meta entry)")
        meta = check_meta(json.loads(str(z["meta"][()])))
        arrays = {k: z[k] for k in z.files if k != "meta"}
    return arrays, meta


def load_compressed(path):
    """The decompressed rows of a .npz written by save_compressed: what io_ply.load_ply returns for a .ply."""
    return decompress(*read_compressed(path))


def size_line(meta, nbytes_after):
    """The one-line report of the CLI and the trainer."""
    n = meta["N"]
    return ("compressed model: rows {} bytes {} -> {} ({:.1f}x) K {} empty centroids {} mean distortion {:.6g}".format(
        n, n * 62 * 4, nbytes_after, n * 62 * 4 / max(1, nbytes_after), meta["K"], meta.get("empty", 0),
        meta.get("distortion", float("nan"))))
