"""Seeded synthetic inputs shared by the parity tests (CPU tensors)."""
import math

import torch


def small_scene(n=400, width=64, height=48, seed=0, spread=1.5, depth=6.0, log_scale=-1.5):
    g = torch.Generator().manual_seed(seed)
    means = torch.randn(n, 3, generator=g) * spread
    means[:, 2] += depth
    quats = torch.randn(n, 4, generator=g)
    scales = torch.exp(torch.randn(n, 3, generator=g) * 0.4 + log_scale)
    opac = torch.sigmoid(torch.randn(n, 1, generator=g) * 1.5)
    shs = torch.randn(n, 16, 3, generator=g) * 0.3
    shs[:, 0] += 0.5
    ang = 0.2
    R = torch.tensor([[math.cos(ang), 0, math.sin(ang)], [0, 1, 0], [-math.sin(ang), 0, math.cos(ang)]])
    viewmat = torch.eye(4)
    viewmat[:3, :3] = R
    viewmat[:3, 3] = torch.tensor([0.1, -0.05, 0.3])
    f = 0.9 * width
    K = torch.tensor([[f, 0, width / 2.0], [0, f, height / 2.0], [0, 0, 1.0]])
    gt = (torch.rand(3, height, width, generator=g) * 255).to(torch.uint8)
    return dict(means=means, quats=quats, scales=scales, opac=opac, shs=shs, viewmat=viewmat, K=K,
                width=width, height=height, gt=gt)


def rel_l2(a, b):
    a, b = a.double().flatten(), b.double().flatten()
    return ((a - b).norm() / (b.norm() + 1e-30)).item()


def psnr(a, b):
    mse = ((a.double() - b.double()) ** 2).mean().item()
    return 10 * math.log10(1.0 / max(mse, 1e-30))


# ---------------------------------------------------------------- hand-built rasterizer inputs
# A raster case: means2d m2 [C,N,2], conics cn [C,N,3], colours col [C,N,3], opacities op [C,N] (float32), image w x h,
# optional per-camera backgrounds bg [C,3], cotangents vi [C,H,W,3] / va [C,H,W], and the intersection lists
# (fids, off) built by the oracle's binning from radii and depths given directly (no projection).  `groups` maps a
# name to a bool mask over the C*N rows.

def conic_from_eig(l1, l2, theta):
    """Conic (a, b, c) with eigenvalues l1, l2 (either sign), l1's eigenvector at angle theta."""
    cs, sn = math.cos(theta), math.sin(theta)
    return (l1 * cs * cs + l2 * sn * sn, (l1 - l2) * sn * cs, l1 * sn * sn + l2 * cs * cs)


def _finish_case(m2, cn, col, op, radii, depths, w, h, bg=None, groups=None, seed=0):
    from oracle import gs_oracle as O
    C, N = op.shape
    tw, th = math.ceil(w / 16), math.ceil(h / 16)
    _, ids, fids = O.isect_tiles(m2, radii, depths, 16, tw, th)
    off = O.isect_offset_encode(ids, C, tw, th)
    g = torch.Generator().manual_seed(1000 + seed)
    return dict(m2=m2.float().contiguous(), cn=cn.float().contiguous(), col=col.float().contiguous(),
                op=op.float().contiguous(), w=w, h=h, bg=None if bg is None else bg.float().contiguous(),
                fids=fids, off=off, vi=torch.randn(C, h, w, 3, generator=g), va=torch.randn(C, h, w, generator=g),
                groups=groups or {"all": torch.ones(C * N, dtype=torch.bool)})


def special_entry_case(seed=0):
    """One camera, 64x48: plain rows, rows special by opacity (0.998 .. 1.0, some clamped at o G > 0.999), needle
    conics on both sides of det = 1e-5 (a+c)^2, non-positive-definite conics (det < 0, a <= 0, c <= 0), rows clamped at
    every valid pixel and rows that are never valid."""
    g = torch.Generator().manual_seed(seed)
    w, h = 64, 48
    rows = []  # (x, y, a, b, c, opacity, radius, group)

    def u(lo, hi):
        return lo + (hi - lo) * torch.rand(1, generator=g).item()

    for _ in range(70):  # plain: well-conditioned, opacity <= 0.998
        l1, l2 = u(0.02, 0.6), u(0.02, 0.6)
        a, b, c = conic_from_eig(l1, l2, u(0, math.pi))
        rows.append((u(-4, w + 4), u(-4, h + 4), a, b, c, u(0.05, 0.7), math.ceil(3.5 / math.sqrt(min(l1, l2))), "plain"))
    ops = [0.998, 0.998, 0.99805, 0.9985, 0.999, 0.999, 0.9991, 0.9995, 0.9999, 1 - 1e-6, 1.0, 1.0]
    for i in range(36):  # special by opacity; wide ones put o G > 0.999 on several pixels, some centred on a pixel
        l = [2e-4, 1e-3, 0.05, 0.2, 0.5, 2.0][i % 6]
        a, b, c = conic_from_eig(l, l * u(0.3, 1.0), u(0, math.pi))
        x, y = u(2, w - 2), u(2, h - 2)
        if i % 3 == 0:
            x, y = math.floor(x) + 0.5, math.floor(y) + 0.5
        rows.append((x, y, a, b, c, ops[i % len(ops)], min(200, math.ceil(3.5 / math.sqrt(l * 0.3))), "opacity"))
    for i in range(40):  # needles: det / (a+c)^2 on both sides of 1e-5 (well clear of fp32's rounding of det)
        ratio = [0.5e-5, 0.8e-5, 1.25e-5, 2e-5, 1e-4][i % 5]
        l1 = [0.003, 0.01, 0.03][i % 3]
        theta = [0.0, 0.2, 0.7, math.pi / 4, 1.2, 2.5][i % 6]
        a, b, c = conic_from_eig(l1, l1 * ratio, theta)
        rows.append((u(0, w), u(0, h), a, b, c, u(0.1, 0.9), 200, "needle"))
    for i in range(24):  # not positive definite: sigma < 0 somewhere, and gsplat's skip must fire there
        kind = i % 4
        if kind == 0:
            a, b, c = conic_from_eig(u(0.05, 0.5), -u(0.001, 0.05), u(0, math.pi))  # det < 0, a, c > 0 or not
        elif kind == 1:
            a, b, c = -u(0.01, 0.2), u(-0.05, 0.05), u(0.05, 0.5)                   # a < 0
        elif kind == 2:
            a, b, c = 0.0, u(-0.05, 0.05), u(0.05, 0.5)                              # a == 0
        else:
            a, b, c = u(0.05, 0.5), u(-0.05, 0.05), -u(0.0, 0.1)                     # c <= 0
        rows.append((u(0, w), u(0, h), a, b, c, u(0.1, 1.0), 200, "nonpd"))
    for i in range(6):  # one-pixel Gaussians at o = 1 centred on a pixel: the only valid pixel is clamped
        rows.append((8.5 + 9 * i, 20.5 + (i % 2) * 11, 50.0, 0.0, 50.0, 1.0, 2, "opacity"))
    for i in range(4):  # never valid: sigma < 0 at every pixel, or opacity below 1/255
        if i < 2:
            rows.append((10.3 + 20 * i, 30.7, -1.0, 0.0, -1.0, 0.8, 20, "nonpd"))
        else:
            rows.append((10.3 + 20 * i, 12.2, 0.2, 0.0, 0.2, 0.003, 20, "plain"))
    N = len(rows)
    perm = torch.randperm(N, generator=g)  # groups interleaved in row order and in depth
    rows = [rows[i] for i in perm.tolist()]
    m2 = torch.tensor([[r[0], r[1]] for r in rows])[None]
    cn = torch.tensor([[r[2], r[3], r[4]] for r in rows])[None]
    op = torch.tensor([r[5] for r in rows])[None]
    radii = torch.tensor([r[6] for r in rows], dtype=torch.int32)[None]
    depths = torch.rand(1, N, generator=g) * 10 + 1
    depths[0, [i for i, r in enumerate(rows) if r[2] == 50.0]] = 0.5  # the one-pixel ones in front of everything
    depths[0, [i for i, r in enumerate(rows) if r[7] == "opacity" and r[2] + r[4] < 3e-3]] += 10.0  # flat ones behind
    col = torch.rand(1, N, 3, generator=g)
    groups = {name: torch.tensor([r[7] == name for r in rows]) for name in ("plain", "opacity", "needle", "nonpd")}
    return _finish_case(m2, cn, col, op, radii, depths, w, h, groups=groups, seed=seed)


LIST_LENGTHS = (1, 63, 64, 65, 127, 128, 129, 191, 192, 193, 300)
# saturating lists: the deepest contributor of the tile (two clamped walls at D and D + 1 end every pixel there)
SATURATE_AT = {1: 0, 63: 61, 64: 62, 65: 63, 127: 64, 128: 126, 129: 127, 191: 128, 192: 190, 193: 191, 300: 192}


def list_case(K, saturating, layout):
    """Exactly K entries in one tile.  layout "single": a 16x16 image; "middle": a 48x16 image whose middle tile holds
    the list, between two empty tiles.  Translucent: broad entries with alpha in [0.0044, 0.008] everywhere (clear of
    1/255), every pixel reaches the end of the list.  Saturating: the same, plus two walls of clamped entries (o = 1,
    alpha = 0.999 on the whole tile) at D = SATURATE_AT[K] and D + 1, so every pixel still alive stops before D + 1
    with D as its last contributor; and sixteen o = 1 entries centred in quadrant 0 ending at D - 2, sixteen in
    quadrant 3 ending near D / 2, which end all of their quadrant's pixels mid-list while the far pixels of quadrants
    1 and 2 live on to D (T before D >= 0.2 there, so T after it is >= 2e-4, clear of 1e-4)."""
    g = torch.Generator().manual_seed(7 * K + (1 if saturating else 0))
    x0 = 16.0 if layout == "middle" else 0.0
    w, h = (48, 16) if layout == "middle" else (16, 16)

    def u(n, lo, hi):
        return lo + (hi - lo) * torch.rand(n, generator=g)

    m2 = torch.stack([x0 + u(K, 4, 12), u(K, 4, 12)], -1)
    l1, l2 = u(K, 1e-5, 1e-4), u(K, 1e-5, 1e-4)
    th = u(K, 0, math.pi)
    cn = torch.stack([l1 * th.cos() ** 2 + l2 * th.sin() ** 2, (l1 - l2) * th.sin() * th.cos(),
                      l1 * th.sin() ** 2 + l2 * th.cos() ** 2], -1)
    op = u(K, 0.0042, 0.0065)
    wall = torch.zeros(K, dtype=torch.bool)
    if saturating:
        D = SATURATE_AT[K]
        for i in (D, D + 1):
            if i < K:
                m2[i] = torch.tensor([x0 + 8.0, 8.0]); cn[i] = torch.tensor([1e-6, 0.0, 1e-6]); op[i] = 1.0; wall[i] = True
        for q, end in ((0, D - 2), (3, D // 2)):
            for i in range(max(0, end - 15), end + 1):
                if end >= 16 and not wall[i]:
                    m2[i] = torch.tensor([x0 + 4.0 + 8 * (q & 1), 4.0 + 8 * (q >> 1)]); cn[i] = torch.tensor([0.06, 0.0, 0.06])
                    op[i] = 1.0; wall[i] = True
    radii = torch.full((1, K), 4, dtype=torch.int32)  # each box covers exactly the one tile
    depths = torch.arange(K, dtype=torch.float32)[None] + 1.0  # list order = row order
    col = torch.rand(1, K, 3, generator=g)
    groups = {"walls": wall, "translucent": ~wall}
    return _finish_case(m2[None], cn[None], col, op[None], radii, depths, w, h, groups=groups, seed=K)


# (C, w, h): images of 1x1 .. 17x17 pixels, tile totals C * tw * th of 1, 7, 8, 9 and 15, several cameras
SHAPES = {
    "1x1": (1, 1, 1), "1x37": (1, 1, 37), "37x1": (1, 37, 1), "16x16": (1, 16, 16), "17x17": (1, 17, 17),
    "tiles1": (1, 13, 11), "tiles7": (1, 100, 10), "tiles8_C2": (2, 30, 20), "tiles9_C3": (3, 40, 16),
    "tiles15_C3": (3, 77, 9), "C2": (2, 40, 24), "C3": (3, 33, 29),
}


def shape_case(name, n=160):
    """Random Gaussians on C cameras (rows differ per camera) with a different background per camera."""
    C, w, h = SHAPES[name]
    g = torch.Generator().manual_seed(sum(map(ord, name)))

    def u(*s, lo=0.0, hi=1.0):
        return lo + (hi - lo) * torch.rand(*s, generator=g)

    m2 = torch.stack([u(C, n, lo=-3, hi=w + 3), u(C, n, lo=-3, hi=h + 3)], -1)
    l1, l2, th = u(C, n, lo=0.03, hi=0.8), u(C, n, lo=0.03, hi=0.8), u(C, n, hi=math.pi)
    cn = torch.stack([l1 * th.cos() ** 2 + l2 * th.sin() ** 2, (l1 - l2) * th.sin() * th.cos(),
                      l1 * th.sin() ** 2 + l2 * th.cos() ** 2], -1)
    op = u(C, n, lo=0.05, hi=0.95)
    radii = torch.ceil(3.5 / torch.minimum(l1, l2).sqrt()).to(torch.int32)
    depths = u(C, n, lo=1, hi=9)
    bg = torch.tensor([[0.2, 0.5, 0.9], [0.8, 0.1, 0.3], [0.05, 0.7, 0.4]])[:C]
    return _finish_case(m2, cn, u(C, n, 3), op, radii, depths, w, h, bg=bg, seed=C * 100 + w)


def nonfinite_case():
    """special_entry_case with NaN in means2d, conics and opacities and +-Inf in conics of a few rows, built on the
    clean lists.  -> (poisoned case, the same case with those rows at opacity 0, bool mask of the rows)."""
    clean = special_entry_case(seed=3)
    N = clean["op"].shape[1]
    nan, inf = float("nan"), float("inf")
    edits = [("m2", 0, nan), ("m2", 1, nan), ("cn", 0, nan), ("cn", 1, nan), ("cn", 2, nan), ("op", None, nan),
             ("cn", 0, inf), ("cn", 2, -inf), ("cn", 1, inf), ("cn", 1, -inf), ("cn", 0, -inf), ("cn", 2, inf)]
    rows = torch.linspace(3, N - 4, len(edits)).long().tolist()
    bad, zero = {k: clean[k].clone() for k in ("m2", "cn", "op")}, clean["op"].clone()
    for r, (k, j, v) in zip(rows, edits):
        if j is None:
            bad[k][0, r] = v
        else:
            bad[k][0, r, j] = v
        zero[0, r] = 0.0
    mask = torch.zeros(N, dtype=torch.bool)
    mask[rows] = True
    return dict(clean, **bad), dict(clean, op=zero), mask
