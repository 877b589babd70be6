"""float64 reference of the per-Gaussian blend weights (gsplat.rasterize_contributions; csrc/contrib.hip), for the tests.

The per-tile dense blend of oracle.gs_oracle.rasterize_to_pixels / tests/absgrad_reference.py with the same rules (sigma < 0
skip, 0.999 clamp, 1/255 cut, stop before T <= 1e-4).  With w = alpha * T at the pixels where the forward accumulates an
entry, per row of the C*N rows:

    wsum = sum of w,    wmax = max of w,    pixels = number of such in-image pixels

and an ALLOWANCE.  A pixel is *fragile* if, at an entry it reaches (every entry up to and including the one it stops at),
    * alpha is within 2e-4 relative of 1/255 (GRAD_TOL, the existing bound on one pixel's alpha), or
    * the running transmittance after the entry is within 1e-2 relative of 1e-4 (10 x SAT_TOL: products of up to 300
      factors), or
    * |sigma| <= 1e-5 on a conic that fails special_entry's positive-definite test (rasterize.hip / raster_tile.h):
a float32 kernel may decide such a pixel the other way, and then every later entry of that pixel changes too.  A row's
allowance is the number of fragile in-image pixels of the tiles that list it.
"""
import torch

ALPHA_MIN = 1.0 / 255.0
T_EPS = 1e-4
ALPHA_REL, T_REL, SIGMA_ABS = 2e-4, 1e-2, 1e-5


def contribution_reference(m2, cn, op, w, h, off, fids, tile_size=16):
    """m2 [C,N,2], cn [C,N,3], op [C,N]; off [C,th,tw], fids [I]: the lists.
    -> dict(wsum [C*N] f64, wmax [C*N] f64, pixels [C*N] i64, allowance [C*N] i64, fragile: number of fragile in-image
    pixels, inside: number of in-image pixels, alpha_sum: sum over the image of 1 - T_final)."""
    dt = torch.float64
    C, N = op.shape
    th, tw = off.shape[1:]
    offs = off.flatten().tolist() + [int(fids.shape[0])]
    m2, cn, op = m2.reshape(C * N, 2).to(dt), cn.reshape(C * N, 3).to(dt), op.reshape(C * N).to(dt)
    fid = fids.to(torch.int64)
    wsum, wmax = torch.zeros(C * N, dtype=dt), torch.zeros(C * N, dtype=dt)
    pixels, allowance = torch.zeros(C * N, dtype=torch.int64), torch.zeros(C * N, dtype=torch.int64)
    fragile_total, alpha_sum = 0, 0.0
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
                done = (incl <= T_EPS) & valid
                anyd = done.any(dim=1)
                first = torch.where(anyd, done.to(torch.int64).argmax(dim=1), torch.full_like(anyd, K, dtype=torch.int64))
                ar = torch.arange(K)[None, :]
                keep = ar < first[:, None]
                reached = ar <= first[:, None]  # the entry a pixel stops at is still looked at
                acc = valid & keep & inside[:, None]
                a_eff = a_eff * keep
                incl_k = torch.cumprod(1.0 - a_eff, dim=1)
                T_before = torch.cat([torch.ones(256, 1, dtype=dt), incl_k[:, :-1]], dim=1)
                wgt = torch.where(acc, a_eff * T_before, torch.zeros_like(a_eff))
                wsum.index_add_(0, g, wgt.sum(0))
                wmax[g] = torch.maximum(wmax[g], wgt.max(0).values)  # (a row is listed once per tile)
                pixels.index_add_(0, g, acc.sum(0))
                alpha_sum += float((1.0 - incl_k[:, -1])[inside].sum())
                near_alpha = ~neg & ((alpha * 255.0 - 1.0).abs() <= ALPHA_REL)
                near_T = valid & ((incl / T_EPS - 1.0).abs() <= T_REL)
                near_sigma = (sigma.abs() <= SIGMA_ABS) & not_pd[g][None]
                frag = ((near_alpha | near_T | near_sigma) & reached).any(dim=1) & inside
                nf = int(frag.sum())
                fragile_total += nf
                if nf:
                    allowance.index_add_(0, torch.unique(g), torch.full((torch.unique(g).numel(),), nf, dtype=torch.int64))
    inside_total = C * w * h
    return dict(wsum=wsum, wmax=wmax, pixels=pixels, allowance=allowance, fragile=fragile_total, inside=inside_total,
                alpha_sum=alpha_sum)


def case_contribution(case, op=None):
    """contribution_reference on a raster case of tests/scenes.py (`op`: other opacities, e.g. x compensation)."""
    return contribution_reference(case["m2"], case["cn"], case["op"] if op is None else op, case["w"], case["h"],
                                  case["off"], case["fids"])


# the cases of tests/test_contribution_cpu.py and tests/test_gpu_contribution.py, by name
LIST_KS = (1, 64, 65, 129, 300)
SHAPE_NAMES = ("1x1", "17x17", "tiles7", "tiles9_C3")


def case_names():
    return ["special"] + [f"list{K}_{'sat' if sat else 'trans'}" for K in LIST_KS for sat in (False, True)] + list(SHAPE_NAMES)


def make_case(name):
    from tests import scenes as S
    if name == "special":
        return S.special_entry_case()
    if name.startswith("list"):
        k, kind = name[4:].split("_")
        return S.list_case(int(k), kind == "sat", "single")
    return S.shape_case(name)


def row_tolerances(name, case):
    """Per group of rows: GRAD_TOL 2e-4, SAT_TOL 1e-3 for opacity-special rows and every row of a saturating list
    (tests/test_gpu_raster_edges.py)."""
    GRAD_TOL, SAT_TOL = 2e-4, 1e-3
    if name == "special":
        return {"plain": GRAD_TOL, "needle": GRAD_TOL, "nonpd": GRAD_TOL, "opacity": SAT_TOL}
    if name.startswith("list"):
        tol = SAT_TOL if name.endswith("_sat") else GRAD_TOL
        return {"walls": SAT_TOL, "translucent": tol}
    return {"all": GRAD_TOL}


_CACHE = {}


def cached(name):
    """(case, reference) computed once per process and shared by the tests that need it; treat both as read-only."""
    if name not in _CACHE:
        case = make_case(name)
        _CACHE[name] = (case, case_contribution(case))
    return _CACHE[name]
