"""-m gpu: the rasterizer's tile kernels (rasterize.hip) at their edges, against the float64 oracle.

Hand-built inputs (tests/scenes.py, no projection): special entries (opacity above 0.998, needle and non-positive-
definite conics), list lengths around the 64-entry staging rounds, small and multi-camera shapes, non-finite rows, and
the A/B builds of rasterize.hip's compile-time switches.  Both backward routes are checked: float atomics
(clmgs_rasterize_bwd without slots) and emit slots + partial lines + the per-row sum.

Gradients are compared per GROUP of rows (a global relative L2 would let the bulk hide a wrong minority), and wherever
the oracle's gradient of a row is exactly zero the kernel's must be exactly zero too.

Tolerances.  Forward and plain rows: those of tests/test_gpu_ops.py (max-abs 2e-4, PSNR 60 dB, GRAD_TOL = 2e-4).
SAT_TOL = 1e-3 for rows special by opacity and for every row of a saturating list.  Derivation, per pixel: the backward
recovers T from the stored alpha, T_final = 1 - fl(1 - T_final); fl(.) of a value in [0.5, 1) errs by <= 2^-25, and a
pixel stops with T_final > 1e-4, so T (and every contribution of the pixel, all proportional to T) carries a relative
error of up to 2^-25 / 1e-4 = 3.0e-4.  Each entry with alpha near 0.999 adds: v_exp_f32 (1 ulp) errs by 2^-23 alpha,
which is 2^-23 alpha / (1 - alpha) <= 1.2e-4 of 1 - alpha, and each clamped entry adds
|(1 - 0.999f) / (1 - 0.999) - 1| = 1.3e-5 against the float64 clamp.  Five such entries in a pixel's path:
3.0e-4 + 5 * 1.2e-4 + 5 * 1.3e-5 = 9.7e-4 < 1e-3.
"""
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from oracle import gs_oracle as O
from tests import scenes as S
from tests.raster_edge_worker import GRAD_NAMES, run
from tests.scenes import psnr, rel_l2

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GRAD_TOL = 2e-4
SAT_TOL = 1e-3
ROUTES = ("atomic", "slot")


def oracle(case):
    """float64 forward (image, alpha, last_ids) and autograd gradients of sum(img * vi) + sum(alpha * va)."""
    a = [case[k].double().requires_grad_() for k in ("m2", "cn", "col", "op")]
    bg = case["bg"].double() if case["bg"] is not None else None
    img, al, last = O.rasterize_to_pixels(*a, case["w"], case["h"], 16, case["off"], case["fids"], backgrounds=bg,
                                          return_last_ids=True)
    ((img * case["vi"].double()).sum() + (al[..., 0] * case["va"].double()).sum()).backward()
    return dict(img=img.detach(), alpha=al[..., 0].detach(), last=last, grads=[x.grad for x in a])


def pixel_trace(case, c, i, j):
    """float64 walk of pixel (i, j) of camera c down its tile's list: (list index, sigma, alpha, T after) per entry."""
    tw = math.ceil(case["w"] / 16)
    off = case["off"].flatten().tolist() + [case["fids"].numel()]
    t = (c * case["off"].shape[1] + i // 16) * tw + j // 16
    N = case["op"].shape[1]
    T, rows = 1.0, []
    for idx in range(off[t], off[t + 1]):
        r = int(case["fids"][idx])
        x, y = case["m2"].reshape(-1, 2)[r].double().tolist()
        a, b, cc = case["cn"].reshape(-1, 3)[r].double().tolist()
        dx, dy = x - (j + 0.5), y - (i + 0.5)
        sig = 0.5 * (a * dx * dx + cc * dy * dy) + b * dx * dy
        scale = 0.5 * (abs(a) * dx * dx + abs(cc) * dy * dy) + abs(b * dx * dy)
        al = min(0.999, float(case["op"].reshape(-1)[r]) * math.exp(-max(sig, -700.0)))
        if sig >= 0 and al >= 1 / 255:
            T *= 1 - al
        rows.append((idx, sig, scale, al, T))
    assert N > 0
    return rows


def is_tie(case, c, i, j, k1, k2):
    """A last_ids mismatch is a genuine tie when a decision between the two candidates sits on its threshold: T after
    an entry within 2e-3 of 1e-4 (SAT_TOL's per-pixel floor, doubled), alpha within 1e-5 of 1/255, or sigma within
    fp32's rounding of 0."""
    lo, hi = min(k1, k2), max(k1, k2) + 1
    for idx, sig, scale, al, T in pixel_trace(case, c, i, j):
        if lo <= idx <= hi and (abs(T / 1e-4 - 1) < 2e-3 or abs(al * 255 - 1) < 1e-5 or abs(sig) <= 1e-6 * scale):
            return True
    return False


def check_forward(case, got, ref):
    for name in ("img", "alpha"):
        x, y = got[name], ref[name]
        assert torch.isfinite(x).all(), name
        assert (x - y.float()).abs().max() < 2e-4, name
        assert psnr(x, y) > 60, name
    mism = torch.nonzero(got["last"] != ref["last"]).tolist()
    assert len(mism) <= 0.01 * got["last"].numel(), f"{len(mism)} last_ids mismatches"
    for c, i, j in mism:
        k1, k2 = int(got["last"][c, i, j]), int(ref["last"][c, i, j])
        assert is_tie(case, c, i, j, k1, k2), f"last_ids ({c},{i},{j}): kernel {k1}, oracle {k2}, not a threshold tie"


def check_grads(case, got, ref, tols, routes=ROUTES):
    """Per group of rows and per parameter: relative L2 within the group's tolerance, exact zeros kept."""
    C, N = case["op"].shape
    for route in routes:
        for pname, y in zip(GRAD_NAMES, ref["grads"]):
            x = got[f"{route}_{pname}"].reshape(C * N, -1)
            y = y.reshape(C * N, -1)
            assert torch.isfinite(y).all(), f"oracle {pname}: not finite"  # a NaN norm would skip the group below
            assert torch.isfinite(x).all(), (route, pname)
            zero = (y == 0).all(dim=1)
            bad = torch.nonzero(zero & (x != 0).any(dim=1)).flatten().tolist()
            assert not bad, f"{route} {pname}: rows {bad[:8]} have a zero oracle gradient but a nonzero one here"
            for gname, rows in case["groups"].items():
                if gname in ("nonpd", "needle", "opacity"):
                    assert float(y[rows].norm()) > 0, (pname, gname)  # the group is really compared
                if float(y[rows].norm()) > 0:
                    e = rel_l2(x[rows], y[rows])
                    assert e < tols[gname], f"{route} {pname} group {gname}: rel_l2 {e:.3g} >= {tols[gname]}"


def special_flags(case):
    """special_entry() of rasterize.hip restated in fp32: opacity > 0.998 or a conic that is not well inside PD."""
    op = case["op"].reshape(-1)
    a, b, c = case["cn"].reshape(-1, 3).unbind(-1)
    tr = a + c
    plain = (op <= 0.998) & (a > 0) & (c > 0) & ((a * c - b * b) > 1e-5 * tr * tr)
    return ~plain


def test_special_entries_match_float64(dev):
    case = S.special_entry_case()
    got, ref = run(case, dev), oracle(case)
    # the scene reaches what it is for: both sides of the special test in every group that straddles it, clamped
    # pixels, sigma < 0 on listed pixels, rows never valid and rows valid only where clamped
    sp = special_flags(case)
    gr = case["groups"]
    op = case["op"].reshape(-1)
    assert not sp[gr["plain"]].any() and sp[gr["nonpd"]].all() and torch.equal(sp[gr["opacity"]], op[gr["opacity"]] > 0.998)
    for g in ("opacity", "needle"):  # both sides of the test: opacity 0.998 itself is not special
        assert 0 < int(sp[gr[g]].sum()) < int(gr[g].sum()), g
    assert int(((op > 0.998) & (op < 0.999)).sum()) > 0 and int((op == 1.0).sum()) > 0
    clamped = neg = 0
    for c, i, j in [(0, i, j) for i in range(case["h"]) for j in range(case["w"])]:
        for idx, sig, scale, al, T in pixel_trace(case, c, i, j):
            r = int(case["fids"][idx])
            clamped += al == 0.999 and sig >= 0
            neg += sig < 0 and bool(gr["nonpd"][r])
    assert clamped > 20 and neg > 1000, (clamped, neg)
    gz = [g.reshape(len(op), -1) for g in ref["grads"]]
    never = torch.stack([(g == 0).all(dim=1) for g in gz]).all(dim=0)
    clamp_only = (gz[1] == 0).all(dim=1) & (gz[3] == 0).all(dim=1) & ~never
    assert int(never.sum()) >= 4 and int(clamp_only.sum()) >= 6
    check_forward(case, got, ref)
    check_grads(case, got, ref, {"plain": GRAD_TOL, "needle": GRAD_TOL, "nonpd": GRAD_TOL, "opacity": SAT_TOL})


@pytest.mark.parametrize("layout", ["single", "middle"])
@pytest.mark.parametrize("saturating", [False, True], ids=["translucent", "saturating"])
@pytest.mark.parametrize("K", S.LIST_LENGTHS)
def test_list_length_and_round_boundaries(dev, K, saturating, layout):
    case = S.list_case(K, saturating, layout)
    got, ref = run(case, dev), oracle(case)
    tile = ref["last"][0, :, 16:32] if layout == "middle" else ref["last"][0]
    if not saturating:
        assert int(tile.min()) == K - 1, "every pixel reaches the end of the list"
    else:
        D = S.SATURATE_AT[K]
        assert int(tile.max()) == D, "the deepest contributor of the tile"
        qmax = [int(tile[8 * (q >> 1):8 * (q >> 1) + 8, 8 * (q & 1):8 * (q & 1) + 8].max()) for q in range(4)]
        if D >= 10:  # the walled quadrants end mid-list, the others go on to D
            assert qmax[0] < D and qmax[3] < D and qmax[1] == D and qmax[2] == D, qmax
    if layout == "middle":
        assert float(ref["alpha"][0, :, :16].abs().max()) == 0 and float(ref["alpha"][0, :, 32:].abs().max()) == 0
    check_forward(case, got, ref)
    tol = SAT_TOL if saturating else GRAD_TOL
    check_grads(case, got, ref, {"walls": SAT_TOL, "translucent": tol})


@pytest.mark.parametrize("name", list(S.SHAPES))
def test_shapes_and_cameras(dev, name):
    case = S.shape_case(name)
    got, ref = run(case, dev), oracle(case)
    C = case["op"].shape[0]
    assert got["img"].shape == (C, case["h"], case["w"], 3)
    check_forward(case, got, ref)
    check_grads(case, got, ref, {"all": GRAD_TOL})


def test_nonfinite_rows_change_nothing_else(dev):
    """Rows with NaN in means2d / conics / opacities or +-Inf in conics are never valid (quadrant_mask drops NaN
    opacities and NaN offsets; a staged NaN / Inf conic fails `sigma >= 0` or `alpha >= 1/255`, in the forward and in
    both branches of the backward): the forward is bitwise that of the same rows at opacity 0, the slot route's
    gradients of every other row are bitwise those of that run, and the poisoned rows' gradients are finite."""
    bad, zero, rows = S.nonfinite_case()
    gb, gz = run(bad, dev), run(zero, dev)
    for k in ("img", "alpha", "last"):
        assert torch.equal(gb[k], gz[k]), k
    for pname in GRAD_NAMES:
        for route in ROUTES:
            x = gb[f"{route}_{pname}"][0]
            assert torch.isfinite(x).all(), (route, pname)
        x, y = gb[f"slot_{pname}"][0], gz[f"slot_{pname}"][0]
        assert torch.equal(x[~rows], y[~rows]), pname
        assert rel_l2(gb[f"atomic_{pname}"][0][~rows], gz[f"atomic_{pname}"][0][~rows]) < 1e-5, pname


# ------------------------------------------------------------------------------------------- build variants
PRODUCT_LIB = os.path.join(ROOT, "clm_gs_amd", "libclmgs_hip.so")
VARIANT_TIMEOUT_S = 600
# float atomics land in a different order from run to run: each sum is reordered, a relative difference of a few ulp of
# the summands, so the bound of the existing route-to-route comparison (slot vs atomic, also a reordering) applies
REORDER_TOL = 1e-5


def _worker(lib, outdir):
    assert os.path.exists(lib), f"{lib} is missing: build() makes it (python -c 'import __graft_entry__ as g; g.build()')"
    env = dict(os.environ, CLMGS_LIB_PATH=lib)
    p = subprocess.run([sys.executable, "-m", "tests.raster_edge_worker", str(outdir)], cwd=ROOT, env=env,
                       capture_output=True, text=True, timeout=VARIANT_TIMEOUT_S)
    assert p.returncode == 0, f"worker on {os.path.basename(lib)} exited {p.returncode}:\n{p.stdout[-2000:]}\n{p.stderr[-4000:]}"
    return {f[:-4]: np.load(os.path.join(outdir, f)) for f in sorted(os.listdir(outdir)) if f.endswith(".npy")}


@pytest.fixture(scope="module")
def product_outputs(tmp_path_factory):
    return _worker(PRODUCT_LIB, tmp_path_factory.mktemp("product"))


@pytest.mark.parametrize("variant", ["special0"])
def test_build_variant_matches_product(dev, variant, product_outputs, tmp_path):
    """CLMGS_SPECIAL_ENTRIES=0 (every entry takes the special branch) is claimed bit for bit: forward, last_ids and
    slot-route gradients must be identical.  Float-atomic gradients are order-nondeterministic: REORDER_TOL."""
    got = _worker(os.path.join(ROOT, "clm_gs_amd", f"libclmgs_hip_ab_{variant}.so"), tmp_path)
    assert sorted(got) == sorted(product_outputs) and len(got) > 100
    for key, want in product_outputs.items():
        x = got[key]
        out = key.split(".")[1]
        if out in ("img", "alpha", "last") or out.startswith("slot_"):
            assert x.dtype == want.dtype and x.tobytes() == want.tobytes(), key
        else:
            assert np.isfinite(x).all(), key
            e = rel_l2(torch.from_numpy(x), torch.from_numpy(want))
            assert e < REORDER_TOL, (key, e)
