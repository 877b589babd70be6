"""float64 reference of the median depth (gsplat.rasterize_median_depth; csrc/median.hip), for the tests.

The per-tile dense blend of tests/contribution_reference.py with the same rules (sigma < 0 skip, 0.999 clamp, 1/255 cut).
The MEDIAN ENTRY of a pixel is the last accumulated entry whose transmittance before blending it is > 0.5: the entry at
which T crosses one half, or the pixel's last contributor where the final T stays above it; a pixel has one if and only
if it accumulates anything.

A float32 kernel can legitimately decide a near-tie the other way, so for every in-image pixel the reference returns an
admissible INTERVAL of list positions, not an answer: pos_hi and pos_lo are the positions of the median entry under the
thresholds 0.5 (1 + d) and 0.5 (1 - d), pos_hi <= pos_lo, with d = 5e-4.  d is derived, not tuned: the project's bound
on one pixel's alpha is 2e-4 relative (ALPHA_REL of contribution_reference, GRAD_TOL of the raster tests); while every
partial product exceeds about one half each a_i < 0.5, hence sum a_i / (1 - a_i) <= 2 sum a_i <= -2 sum ln(1 - a_i) =
2 ln(1 / T) <= 2 ln 2, which bounds the relative error of T that the alphas cause by 2 ln 2 x 2e-4 = 2.8e-4; 300 roundings
of 6e-8 each (the longest list of the cases) add 1.8e-5.  A kernel whose T is within d of the exact one picks a valid
entry between the two positions.

A pixel is *excluded* if, at an entry it looks at before T falls to 0.5 (1 - d), either
    * alpha is within 2e-4 relative of 1/255, or
    * |sigma| <= 1e-5 on a conic that fails special_entry's positive-definite test (rasterize.hip / raster_tile.h)
(the first and third fragility rules of contribution_reference): the kernel may accumulate such an entry or not.  The
cap on exclusions is a condition of the tests, not a measurement: at most EXCLUDED_CAP of the in-image pixels of a case.

The reference also asserts the fact the kernel rests on: no accumulated entry whose T before it is > 0.5 (1 - d) leaves
T <= 1e-4 (alpha <= 0.999 leaves T >= 0.5 (1 - d) x 0.001 = 5e-4), so the forward's "stop before T <= 1e-4" rule can
never fire at or before the median entry.
"""
import torch

from tests.contribution_reference import ALPHA_MIN, ALPHA_REL, SIGMA_ABS, T_EPS

D_REL = 5e-4
EXCLUDED_CAP = 0.005


def median_reference(m2, cn, op, w, h, off, fids, tile_size=16, d=D_REL):
    """m2 [C,N,2], cn [C,N,3], op [C,N]; off [C,th,tw], fids [I]: the lists.
    -> dict(has [C,H,W] bool: the pixel accumulates an entry; pos_hi, pos_lo [C,H,W] int64: the admissible interval of
    positions within the tile's list (-1 without an entry); pos [C,H,W]: the position under the threshold 0.5 itself;
    excluded [C,H,W] bool; tiles: per listed tile (c, ty, tx, s, e, valid [256,K] bool: the entries each of its pixels
    accumulates); inside: number of pixels; wide: pixels whose interval holds more than one entry; visited, listed: list
    entries up to the deepest median entry of each tile (the whole list where a pixel stays open), and all of them)."""
    dt = torch.float64
    C, N = op.shape
    th, tw = off.shape[1:]
    offs = off.flatten().tolist() + [int(fids.shape[0])]
    m2, cn, op = m2.reshape(C * N, 2).to(dt), cn.reshape(C * N, 3).to(dt), op.reshape(C * N).to(dt)
    fid = fids.to(torch.int64)
    has = torch.zeros((C, h, w), dtype=torch.bool)
    excluded = torch.zeros((C, h, w), dtype=torch.bool)
    pos_hi = torch.full((C, h, w), -1, dtype=torch.int64)
    pos_lo, pos_mid = pos_hi.clone(), pos_hi.clone()
    tiles, visited = [], 0
    ii, jj = torch.meshgrid(torch.arange(tile_size), torch.arange(tile_size), indexing="ij")
    ii, jj = ii.reshape(-1), jj.reshape(-1)
    a_all, b_all, c_all = cn.unbind(-1)
    tr = a_all + c_all
    not_pd = ~((a_all > 0) & (c_all > 0) & ((a_all * c_all - b_all * b_all) > 1e-5 * tr * tr))
    for c in range(C):
        for ty in range(th):
            for tx in range(tw):
                tid = (c * th + ty) * tw + tx
                s, e = offs[tid], offs[tid + 1]
                if e <= s:
                    continue
                K = e - s
                g = fid[s:e]
                y, x = ty * tile_size + ii, tx * tile_size + jj
                inside = (y < h) & (x < w)
                dx = m2[g, 0][None] - (x.to(dt) + 0.5)[:, None]
                dy = m2[g, 1][None] - (y.to(dt) + 0.5)[:, None]
                a_, b_, c_ = cn[g, 0][None], cn[g, 1][None], cn[g, 2][None]
                sigma = 0.5 * (a_ * dx * dx + c_ * dy * dy) + b_ * dx * dy
                neg = sigma < 0
                alpha = torch.clamp(op[g][None] * torch.exp(-torch.where(neg, torch.zeros_like(sigma), sigma)), max=0.999)
                valid = ~neg & (alpha >= ALPHA_MIN)
                a_eff = torch.where(valid, alpha, torch.zeros_like(alpha))
                incl = torch.cumprod(1.0 - a_eff, dim=1)
                T_before = torch.cat([torch.ones(tile_size * tile_size, 1, dtype=dt), incl[:, :-1]], dim=1)
                looked = T_before > 0.5 * (1 - d)
                # the fact the kernel rests on
                assert not bool((valid & looked & (incl <= T_EPS)).any()), "an entry at or before the median left T <= 1e-4"

                def last(cand):
                    p = K - 1 - torch.flip(cand, dims=(1,)).to(torch.int64).argmax(dim=1)
                    return torch.where(cand.any(dim=1), p, torch.full_like(p, -1))

                hi, mid, lo = (last(valid & (T_before > 0.5 * (1 + f))) for f in (d, 0.0, -d))
                any_valid = valid.any(dim=1)
                assert bool(((hi >= 0) == any_valid).all()) and bool((hi <= mid).all()) and bool((mid <= lo).all())
                near_alpha = ~neg & ((alpha * 255.0 - 1.0).abs() <= ALPHA_REL)
                near_sigma = (sigma.abs() <= SIGMA_ABS) & not_pd[g][None]
                frag = ((near_alpha | near_sigma) & looked).any(dim=1)
                yy, xx = y[inside], x[inside]
                has[c, yy, xx] = any_valid[inside]
                excluded[c, yy, xx] = frag[inside]
                pos_hi[c, yy, xx], pos_mid[c, yy, xx], pos_lo[c, yy, xx] = hi[inside], mid[inside], lo[inside]
                tiles.append((c, ty, tx, s, e, valid))
                open_ = (incl[:, -1] > 0.5)[inside]
                visited += K if bool(open_.any()) else int(mid[inside].max()) + 1
    return dict(has=has, pos_hi=pos_hi, pos_lo=pos_lo, pos=pos_mid, excluded=excluded, tiles=tiles, inside=C * w * h,
                wide=int((pos_lo > pos_hi).sum()), visited=visited, listed=int(fids.shape[0]), N=N, tile_size=tile_size)


def case_median(case, op=None):
    """median_reference on a raster case of tests/scenes.py (`op`: other opacities)."""
    return median_reference(case["m2"], case["cn"], case["op"] if op is None else op, case["w"], case["h"], case["off"],
                            case["fids"])


def reference_depth_and_id(ref, case, depths):
    """The maps under the threshold 0.5 itself, float32 depth [C,H,W] and int32 id [C,H,W], from depths [C,N]: what a
    kernel without rounding would return (for the hand-made pixels and for figures; the GPU tests use check_maps)."""
    C, H, W = ref["has"].shape
    N, ts = ref["N"], ref["tile_size"]
    ids = torch.full((C, H, W), -1, dtype=torch.int32)
    for c, ty, tx, s, e, _ in ref["tiles"]:
        y0, x0 = ty * ts, tx * ts
        p = ref["pos"][c, y0:y0 + ts, x0:x0 + ts]
        row = (case["fids"][s:e].to(torch.int64) - c * N)[p.clamp_min(0)]
        ids[c, y0:y0 + ts, x0:x0 + ts] = torch.where(p >= 0, row, torch.full_like(row, -1)).to(torch.int32)
    if N == 0:
        return torch.zeros((C, H, W)), ids
    flat = depths.reshape(C, N).float()
    dep = torch.stack([flat[c][ids[c].clamp_min(0).long()] for c in range(C)])
    return torch.where(ids >= 0, dep, torch.zeros_like(dep)), ids


def check_maps(ref, case, depths, median_depth, median_id):
    """The kernel's maps (CPU tensors) against the reference -> dict of counts; every `bad_*` must be zero.
    For every non-excluded pixel: the id is -1 exactly where the reference accumulates nothing (bad_none), otherwise it is
    an entry of the pixel's tile list (bad_listed) that the reference accumulates at that pixel (bad_entry) and whose
    position lies in [pos_hi, pos_lo] (bad_pos).  For EVERY pixel: the depth is bit-equal to depths[] at the kernel's own
    id, 0.0 for -1, and the id is -1 or a row of the camera (bad_depth, bad_range)."""
    C, H, W = ref["has"].shape
    N, ts = ref["N"], ref["tile_size"]
    assert median_depth.shape == median_id.shape == (C, H, W)
    assert median_depth.dtype == torch.float32 and median_id.dtype == torch.int32
    kid = median_id.to(torch.int64)
    flat = depths.reshape(C, N).float()
    in_range = (kid >= -1) & (kid < N)
    want = torch.stack([flat[c][kid[c].clamp(0, max(N - 1, 0))] for c in range(C)]) if N else torch.zeros((C, H, W))
    want = torch.where(kid >= 0, want, torch.zeros_like(want))
    out = dict(bad_range=int((~in_range).sum()), bad_depth=int((want.view(torch.int32) != median_depth.view(torch.int32)).sum()),
               bad_none=0, bad_listed=0, bad_entry=0, bad_pos=0, excluded=int(ref["excluded"].sum()), inside=ref["inside"])
    sure = ~ref["excluded"]
    out["bad_none"] = int((sure & ((kid == -1) != ~ref["has"])).sum())
    for c, ty, tx, s, e, valid in ref["tiles"]:
        y0, x0 = ty * ts, tx * ts
        k = kid[c, y0:y0 + ts, x0:x0 + ts]
        hh, ww = k.shape
        v = valid.reshape(ts, ts, -1)[:hh, :ww]
        sel = sure[c, y0:y0 + ts, x0:x0 + ts] & ref["has"][c, y0:y0 + ts, x0:x0 + ts] & (k >= 0)
        rows = case["fids"][s:e].to(torch.int64) - c * N
        match = k[..., None] == rows[None, None, :]  # (a row is listed once per tile)
        found, p = match.any(-1), match.to(torch.int64).argmax(-1)
        accumulated = torch.gather(v, 2, p[..., None])[..., 0]
        lo, hi = ref["pos_lo"][c, y0:y0 + ts, x0:x0 + ts], ref["pos_hi"][c, y0:y0 + ts, x0:x0 + ts]
        out["bad_listed"] += int((sel & ~found).sum())
        out["bad_entry"] += int((sel & found & ~accumulated).sum())
        out["bad_pos"] += int((sel & found & accumulated & ((p < hi) | (p > lo))).sum())
    return out


# the cases of tests/test_median_depth_cpu.py and tests/test_gpu_median_depth.py, by name
LIST_KS = (1, 64, 65, 129, 300)
CPU_SHAPES = ("1x1", "17x17", "tiles7", "tiles9_C3", "C3", "tiles15_C3", "1x37", "37x1")
GPU_SHAPES = ("1x1", "17x17", "tiles7", "tiles9_C3", "C3")


def list_names():
    return [f"list{K}_{'sat' if sat else 'trans'}" for K in LIST_KS for sat in (False, True)]


def make_case(name):
    from tests import scenes as S
    if name == "special":
        return S.special_entry_case()
    if name == "list65_sat_middle":
        return S.list_case(65, True, "middle")
    if name.startswith("list"):
        k, kind = name[4:].split("_")
        return S.list_case(int(k), kind == "sat", "single")
    return S.shape_case(name)


def list_order_rank(case):
    """A rank per row of the C*N rows that increases along every tile list of the case: the lists are subsequences of one
    depth order per camera, which a topological sort of their consecutive pairs recovers (smallest row first among the
    free ones; rows that no list holds come where their number puts them)."""
    import heapq
    C, N = case["op"].shape
    offs = case["off"].flatten().tolist() + [int(case["fids"].shape[0])]
    fid = case["fids"].tolist()
    succ, indeg = [set() for _ in range(C * N)], [0] * (C * N)
    for s, e in zip(offs[:-1], offs[1:]):
        for a, b in zip(fid[s:e - 1], fid[s + 1:e]):
            if b not in succ[a]:
                succ[a].add(b)
                indeg[b] += 1
    free = [r for r in range(C * N) if indeg[r] == 0]
    heapq.heapify(free)
    rank, n = torch.zeros(C * N, dtype=torch.int64), 0
    while free:
        r = heapq.heappop(free)
        rank[r], n = n, n + 1
        for b in succ[r]:
            indeg[b] -= 1
            if indeg[b] == 0:
                heapq.heappush(free, b)
    assert n == C * N, "the lists of the case are not subsequences of one order"
    return rank.reshape(C, N)


def case_depths(case, kind):
    """depths [C,N] for a case: "increasing" in list order (list_order_rank), or "permuted": a seeded permutation of
    those values, not monotone in list order -- a kernel that returned a minimum, a maximum or a blend of the depths it
    met would fail on it."""
    C, N = case["op"].shape
    inc = list_order_rank(case).float() * 0.25 + 1.0
    if kind == "increasing":
        return inc
    g = torch.Generator().manual_seed(11 + N)
    return inc.reshape(-1)[torch.randperm(C * N, generator=g)].reshape(C, N).contiguous()


_CACHE = {}


def cached(name):
    """(case, reference) computed once per process and shared by the tests that need it; treat both as read-only."""
    if name not in _CACHE:
        case = make_case(name)
        _CACHE[name] = (case, case_median(case))
    return _CACHE[name]
