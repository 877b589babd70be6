"""The resolution schedule's area filter in numpy int64, cell by cell ("Resolution schedule"):

    f = 2^L,  Ho = ceil(H / f),  Wo = ceil(W / f)
    wx(j, x) = max(0, min((x+1) Wo, (j+1) W) - max(x Wo, j W))        sum over x = W
    wy(i, y) = max(0, min((y+1) Ho, (i+1) H) - max(y Ho, i H))        sum over y = H
    S(i, j)  = sum_y sum_x wy(i, y) wx(j, x) p[y, x]
    out(i,j) = (2 S + W H) // (2 W H)                                  round half up
    mask:      p = [m != 0];  out = 255 if 2 S >= W H else 0

Explicit loops over the cells, nothing clever: this is what csrc/resample.hip is held to, bit for bit."""
import functools

import numpy as np


def level_size(H, W, level):
    f = 1 << int(level)
    return -(-int(H) // f), -(-int(W) // f)


@functools.lru_cache(maxsize=None)
def weights(n_src, n_dst):
    """w[j, x]: the overlap of destination cell j and source cell x, in units of 1 / (n_src * n_dst) of the extent."""
    w = np.zeros((n_dst, n_src), dtype=np.int64)
    for j in range(n_dst):
        for x in range(n_src):
            w[j, x] = max(0, min((x + 1) * n_dst, (j + 1) * n_src) - max(x * n_dst, j * n_src))
    return w


def weighted_sums(plane, level):
    """S[i, j] of one plane [H, W] (any integer dtype), int64."""
    H, W = plane.shape
    Ho, Wo = level_size(H, W, level)
    wy, wx = weights(H, Ho), weights(W, Wo)
    p = plane.astype(np.int64)
    S = np.zeros((Ho, Wo), dtype=np.int64)
    for i in range(Ho):
        ys = np.nonzero(wy[i])[0]
        for j in range(Wo):
            xs = np.nonzero(wx[j])[0]
            acc = 0
            for y in ys:
                for x in xs:
                    acc += int(wy[i, y]) * int(wx[j, x]) * int(p[y, x])
            S[i, j] = acc
    return S


def area_resample(a, level):
    """uint8 [P,H,W] / [H,W] or uint16 [H,W] -> the same dtype and rank at the level's size."""
    a = np.asarray(a)
    if level == 0:
        return a.copy()
    if a.ndim == 3:
        return np.stack([area_resample(p, level) for p in a])
    H, W = a.shape
    S = weighted_sums(a, level)
    return ((2 * S + W * H) // (2 * W * H)).astype(a.dtype)


def mask_resample(m, level):
    """uint8 [H,W], 0 = ignored -> (uint8 mask of 0 / 255 at the level's size, the number of counted cells)."""
    m = np.asarray(m)
    H, W = m.shape
    S = weighted_sums((m != 0).astype(np.int64), level)
    out = np.where(2 * S >= W * H, 255, 0).astype(np.uint8)
    return out, int(np.count_nonzero(out))
