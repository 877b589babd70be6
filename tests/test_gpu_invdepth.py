"""-m gpu: depth regularisation ("Depth regularisation"): the kernels of csrc/invdepth.hip on their
own, the 4-channel tile kernels on the slot route and in the device-count forms, the engines and the trainer, against the
float64 restatement in tests/invdepth_reference.py."""
import ctypes
import functools
import json
import math
import os
import re

import numpy as np
import pytest
import torch

from tests import invdepth_reference as R
from tests import masked_loss_reference as M
from tests import scenes as S
from tests import test_gpu_engines as GE
from tests import test_gpu_exposure as EX
from tests import test_gpu_masked_loss as ML
from tests import test_gpu_raster_depth as RD
from tests.raster_edge_worker import GRAD_NAMES, slots_of
from tests.scenes import rel_l2
from tests.test_gpu_raster_edges import GRAD_TOL

pytestmark = pytest.mark.gpu

U = 2.0 ** -24  # unit roundoff of float32
SENT = 123.25
EINVAL = 10001
# 1 pixel; width below one vector; width no multiple of 4; 9100 pixels: more than one workgroup (8192 pixels each)
SHAPES = [(1, 1), (5, 7), (13, 67), (70, 130)]
# channel 3 of [H,W,4] (the engine's layout: the flat path) | the same, base moved by one pixel | the same, base moved by
# one float (not 16-byte aligned) | planar (generic path) | planar, base moved by one element
LAYOUTS = ["hwc4", "hwc4_offset", "hwc4_unaligned", "planar", "planar_offset"]
# prior = raw * 1.75 / 65536 - 0.125 = (7 raw - 32768) / 2^18: an integer below 2^19 over a power of two, so the prior is a
# float32 EXACTLY, on the device as in float64.  Then I - prior is one float32 rounding of the exact difference, its sign is
# exact, and the kernel's sum differs from the float64 sum of the n terms by that rounding and the roundings of fewer than
# n additions: at most n * 2^-24 * sum|terms|, the bound the comparison uses.
SCALE, OFFSET = 1.75, -0.125
WEIGHT = float(np.float32(0.37))


def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _alloc(layout, h, w, dev, dtype=torch.float32, fill=SENT):
    """-> (whole buffer, [h,w] view of it) in the given layout."""
    n = h * w
    if layout == "hwc4":
        buf = torch.full((n * 4,), fill, dtype=dtype, device=dev)
        view = buf.view(h, w, 4)[..., 3]
    elif layout == "hwc4_offset":
        buf = torch.full(((n + 1) * 4,), fill, dtype=dtype, device=dev)
        view = buf[4:].view(h, w, 4)[..., 3]
    elif layout == "hwc4_unaligned":
        buf = torch.full((n * 4 + 1,), fill, dtype=dtype, device=dev)
        view = buf[1:].view(h, w, 4)[..., 3]
    elif layout == "planar":
        buf = torch.full((n,), fill, dtype=dtype, device=dev)
        view = buf.view(h, w)
    else:
        buf = torch.full((n + 2,), fill, dtype=dtype, device=dev)
        view = buf[1:1 + n].view(h, w)
    return buf, view


def _untouched(layout, h, w, buf):
    """Every element of the buffer that is not a pixel's own word still holds the sentinel."""
    own, view = _alloc(layout, h, w, buf.device, torch.bool, False)
    view.fill_(True)
    return bool((buf[~own] == SENT).all())


@functools.lru_cache(maxsize=None)
def _case(h, w):
    """Inputs and the float64 reference, once per shape."""
    gen = torch.Generator().manual_seed(1000 * h + w)
    n = h * w
    raw = torch.randint(0, 65536, (h, w), generator=gen, dtype=torch.int32)
    raw.view(-1)[n - 1] = 65535
    if n > 1:
        raw.view(-1)[0] = 0
    prior = R.prior_of(raw, SCALE, OFFSET)
    assert torch.equal(prior.float().double(), prior), "the prior is a float32 exactly"
    delta = (0.01 + 0.5 * torch.rand(h, w, generator=gen, dtype=torch.float64)) * \
        (torch.randint(0, 2, (h, w), generator=gen) * 2 - 1)
    tie = torch.rand(h, w, generator=gen) < 0.1 if n > 1 else torch.zeros(h, w, dtype=torch.bool)
    I = torch.where(tie, prior, prior + delta).float()
    mask = torch.randint(0, 3, (h, w), generator=gen).to(torch.uint8) * 127  # 0, 127, 254
    if n > 1:
        mask.view(-1)[1] = 0
    return I, raw.to(torch.uint16), mask, int(tie.sum())


def _run_loss(layout, h, w, dev, I, raw, mask, weight=WEIGHT, scale=SCALE, offset=OFFSET):
    from clm_gs_amd import _lib
    L = _lib.lib()
    ibuf, iv = _alloc(layout, h, w, dev)
    vbuf, vv = _alloc(layout, h, w, dev)
    iv.copy_(I.to(dev))
    rows = int(L.clmgs_invdepth_partials_rows(h, w))
    partials = torch.full((rows,), float("nan"), device=dev)
    total = torch.full((1,), float("nan"), device=dev)
    rd, md = raw.to(dev).contiguous(), (mask.to(dev).contiguous() if mask is not None else None)
    _lib.check(L.clmgs_invdepth_l1_fwd_bwd(_lib.stream(), h, w, _p(iv), *iv.stride(), _p(rd), scale, offset, _p(md), weight,
                                           _p(vv), *vv.stride(), _p(partials)))
    _lib.check(L.clmgs_invdepth_finish(_lib.stream(), rows, _p(partials), _p(total)))
    torch.cuda.synchronize()
    return vbuf, vv, partials, total


@pytest.mark.parametrize("masked", [False, True], ids=["unmasked", "masked"])
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("hw", SHAPES)
def test_loss_kernel_against_float64(dev, hw, layout, masked):
    h, w = hw
    n = h * w
    I, raw, mask, ties = _case(h, w)
    mask = mask if masked else None
    assert int(raw.to(torch.int32).max()) == 65535 and (n == 1 or int(raw.to(torch.int32).min()) == 0)
    assert n == 1 or ties > 0
    vbuf, vv, partials, total = _run_loss(layout, h, w, dev, I, raw, mask)
    # the cotangent, exactly: +-float32(weight / n), 0 at a tie and at an ignored pixel
    coef = float(np.float32(np.float64(WEIGHT) / n))
    d = I.double() - R.prior_of(raw, SCALE, OFFSET)
    want_v = (R.counted(mask, d) * torch.sign(d) * coef).float()  # +-coef itself: no further rounding
    got_v = vv.cpu()
    assert torch.equal(got_v, want_v), float((got_v - want_v).abs().max())
    assert n == 1 or int((want_v == 0).sum()) >= ties
    assert _untouched(layout, h, w, vbuf), "words 0..2 of a pixel (and the padding) keep the sentinel"
    # the sum of m |I - prior|
    terms = R.counted(mask, I.double()) * (I.double() - R.prior_of(raw, SCALE, OFFSET)).abs()
    ref, bound = float(terms.sum()), n * U * float(terms.sum())
    assert bool(torch.isfinite(partials).all()), "every partial row is written"
    got = float(total.double().item())
    print(f"invdepth loss {hw} {layout} masked={masked}: sum {got:.9g} vs {ref:.9g}, error / bound "
          f"{abs(got - ref) / bound if bound else 0.0:.3f}")
    assert abs(got - ref) <= bound
    # the term as the operator reports it
    want_l = float(R.depth_term(I.double(), raw, SCALE, OFFSET, WEIGHT, mask))
    assert abs(got * WEIGHT / n - want_l) <= 2 * bound * WEIGHT / n + 1e-12


@pytest.mark.parametrize("layout", ["hwc4", "planar_offset"])
def test_loss_kernel_is_deterministic(dev, layout):
    h, w = 70, 130
    I, raw, mask, _ = _case(h, w)
    a = _run_loss(layout, h, w, dev, I, raw, mask)
    b = _run_loss(layout, h, w, dev, I, raw, mask)
    assert torch.equal(a[0], b[0]) and torch.equal(a[2], b[2]) and torch.equal(a[3], b[3])


def test_loss_kernel_general_scale_and_offset(dev):
    """A scale and an offset that are no short dyadic numbers: the prior is rounded to float32 once on the device (one fused
    multiply-add), so next to the n * 2^-24 * sum|terms| of the exact-prior case every term carries up to 2^-24 |prior|.
    Signs are kept away from that rounding by |I - prior| >= 0.01."""
    h, w = 13, 67
    n = h * w
    I0, raw, mask, _ = _case(h, w)
    scale, offset = float(np.float32(0.8371)), float(np.float32(0.0123))
    prior = R.prior_of(raw, scale, offset)
    gen = torch.Generator().manual_seed(5)
    sgn = torch.randint(0, 2, (h, w), generator=gen) * 2 - 1
    I = (prior + sgn * (0.01 + torch.rand(h, w, generator=gen, dtype=torch.float64))).float()
    _, vv, _, total = _run_loss("hwc4", h, w, dev, I, raw, mask, scale=scale, offset=offset)
    coef = float(np.float32(np.float64(WEIGHT) / n))
    cnt = R.counted(mask, prior)
    want_v = (cnt * torch.sign(I.double() - prior) * coef).float()
    assert torch.equal(vv.cpu(), want_v)
    terms = cnt * (I.double() - prior).abs()
    bound = n * U * float(terms.sum()) + U * float((cnt * prior.abs()).sum())
    assert abs(float(total.double().item()) - float(terms.sum())) <= bound


def test_loss_kernel_rejects_bad_arguments(dev):
    from clm_gs_amd import _lib
    L = _lib.lib()
    h, w = 5, 7
    I, raw, mask, _ = _case(h, w)
    _, iv = _alloc("hwc4", h, w, dev)
    iv.copy_(I.to(dev))
    vbuf, vv = _alloc("hwc4", h, w, dev)
    rows = int(L.clmgs_invdepth_partials_rows(h, w))
    partials = torch.full((rows,), SENT, device=dev)
    rd = raw.to(dev)
    st = _lib.stream()
    good = dict(H=h, W=w, I=_p(iv), sy=iv.stride(0), sx=iv.stride(1), prior=_p(rd), mask=None, weight=WEIGHT, v=_p(vv),
                vsy=vv.stride(0), vsx=vv.stride(1), partials=_p(partials))
    bad = [dict(H=0), dict(W=0), dict(I=None), dict(prior=None), dict(v=None), dict(partials=None), dict(v=_p(iv)),
           dict(vsx=0), dict(vsy=1), dict(weight=float("nan"))]
    for change in bad:
        a = {**good, **change}
        rc = L.clmgs_invdepth_l1_fwd_bwd(st, a["H"], a["W"], a["I"], a["sy"], a["sx"], a["prior"], SCALE, OFFSET, a["mask"],
                                         a["weight"], a["v"], a["vsy"], a["vsx"], a["partials"])
        assert rc == EINVAL, (change, rc)
    assert L.clmgs_invdepth_partials_rows(0, 5) == 0
    torch.cuda.synchronize()
    assert bool((vbuf == SENT).all()) and bool((partials == SENT).all()) and torch.equal(iv.cpu(), I)
    with pytest.raises(_lib.ClmgsError):
        _lib.check(rc)


def test_operator(dev):
    """clm_kernels.invdepth_l1_loss on channel 3 of a [1,H,W,4] leaf: value and gradient of the restatement; the other three
    channels receive zeros."""
    from clm_gs_amd import clm_kernels as K
    h, w = 13, 67
    I, raw, mask, _ = _case(h, w)
    for m in (None, mask):
        leaf = torch.zeros(1, h, w, 4, device=dev)
        leaf[0, ..., 3] = I.to(dev)
        leaf.requires_grad_()
        l = K.invdepth_l1_loss(leaf[0, ..., 3], raw.to(dev), SCALE, OFFSET, WEIGHT, m.to(dev) if m is not None else None)
        (2.0 * l).backward()
        want = float(R.depth_term(I.double(), raw, SCALE, OFFSET, WEIGHT, m))
        assert abs(l.item() - want) < 1e-6 * max(1.0, abs(want))
        want_v = R.cotangent(I, raw, SCALE, OFFSET, WEIGHT, m) * 2.0
        assert rel_l2(leaf.grad[0, ..., 3].cpu(), want_v) < 1e-6
        assert float(leaf.grad[0, ..., :3].abs().max()) == 0.0


# ------------------------------------------------------------------------------------------- pack kernel
@pytest.mark.parametrize("V", [1, 63, 64, 65, 1000])
def test_pack_kernel(dev, V):
    from clm_gs_amd import _lib
    gen = torch.Generator().manual_seed(V)
    radii = torch.randint(-2, 40, (V,), generator=gen, dtype=torch.int32)
    radii[V - 1] = 3
    if V > 1:
        radii[0] = 0
    depths = 0.1 + 50.0 * torch.rand(V, generator=gen)
    packed = torch.full((V, 16), SENT, device=dev)
    rd, dd = radii.to(dev), depths.to(dev)  # (named: a temporary's memory would be reused by the next upload)
    _lib.check(_lib.lib().clmgs_invdepth_pack(_lib.stream(), V, _p(rd), _p(dd), _p(packed)))
    torch.cuda.synchronize()
    got = packed.cpu()
    want = torch.where(radii > 0, 1.0 / depths, torch.zeros(V))  # float32 division, correctly rounded on both sides
    assert torch.equal(got[:, 9], want)
    keep = torch.ones(16, dtype=torch.bool)
    keep[9] = False
    assert bool((got[:, keep] == SENT).all())


# ------------------------------------------------------------------------------------------- four channels, slot route
def _projected_case(w, h):
    """The projected scene of tests/test_gpu_raster_depth.py as a raster case, fourth colour 1/z."""
    s, radii, m2, d, cn, off, fids = RD._projected(w, h)
    g = torch.Generator().manual_seed(9)
    n = m2.shape[1]
    case = dict(m2=m2.float().contiguous(), cn=cn.float().contiguous(), col=torch.rand(1, n, 3, generator=g),
                op=s["opac"].reshape(1, -1).contiguous(), w=w, h=h, bg=None, fids=fids, off=off,
                vi=torch.randn(1, h, w, 3, generator=g), va=torch.randn(1, h, w, generator=g),
                groups={"all": torch.ones(n, dtype=torch.bool)})
    z = torch.where(radii > 0, 1.0 / torch.where(radii > 0, d, torch.ones_like(d)), torch.zeros_like(d)).float()
    return case, z, None, torch.randn(1, h, w, generator=g)


SLOT_CASES = ["small64x48", "small70x37", "special", "list65_sat_single", "list129_sat_middle", "list300_tr_single"]


@functools.lru_cache(maxsize=None)
def _slot_case(name):
    if name.startswith("small"):
        w, h = (64, 48) if name == "small64x48" else (70, 37)  # 70x37: no multiple of the tile
        return _projected_case(w, h)
    if name == "special":
        case = S.special_entry_case()
    else:
        K, sat, layout = re.match(r"list(\d+)_(sat|tr)_(\w+)", name).groups()
        case = S.list_case(int(K), sat == "sat", layout)
    z, bgd, vd = RD.fourth_channel(case, 7)
    return case, 1.0 / z, bgd, vd


def _slot_backward(case, fw, v_cot, dev, nch=4, dev_capacity=None, unpack=True):
    """The slot route on the forward `fw` (RD.run4's): clmgs_rasterize4_slot_bwd (nch = 4) / clmgs_rasterize_bwd (nch = 3),
    or with dev_capacity the _dev forms.  -> partial lines [capacity,16], the summed lines [N,16] and the unpacked gradients
    (exact forms), on the CPU.  Every buffer starts as NaN / the sentinel."""
    from clm_gs_amd import _lib
    L = _lib.lib()
    C, N = case["op"].shape
    assert C == 1
    w, h = case["w"], case["h"]
    tw, th = math.ceil(w / 16), math.ceil(h / 16)
    I = case["fids"].numel()
    slot, row_cum = slots_of(case["fids"], N)
    cap = I if dev_capacity is None else dev_capacity
    pad = torch.zeros(cap - I, dtype=torch.int32)
    fids, sd = torch.cat([case["fids"].to(torch.int32), pad]).to(dev), torch.cat([slot, pad]).to(dev)
    rd, off = row_cum.to(dev), case["off"].to(dev).contiguous()
    packed, al, last = (fw[k].to(dev).contiguous() for k in ("packed", "alpha", "last"))
    bg = RD.bg4_of(case, fw["bgd"])
    if bg is not None:
        bg = (bg if nch == 4 else bg[:, :3]).to(dev).contiguous()
    v = v_cot.to(dev).contiguous()
    va = case["va"].to(dev).contiguous()  # the alpha cotangent of the case, as RD.run4 passes it to the atomic route
    assert v.shape[-1] == nch
    parts = torch.full((max(cap, 1), 16), SENT, device=dev)
    st = _lib.stream()
    res = {}
    if dev_capacity is None:
        pg = torch.full((N, 16), float("nan"), device=dev)
        outs = [torch.full(s, float("nan"), device=dev) for s in ((1, N, 2), (1, N, 3), (1, N, nch), (1, N))]
        fn = L.clmgs_rasterize4_slot_bwd if nch == 4 else L.clmgs_rasterize_bwd
        _lib.check(fn(st, 1, N, I, _p(packed), _p(bg), w, h, 16, tw, th, _p(off), _p(fids), _p(al), _p(last), _p(v), _p(va),
                      _p(pg) if unpack else None, *[_p(x) if unpack else None for x in outs], _p(sd), _p(rd), _p(parts)))
        if unpack:
            res.update({f"slot_{n}": x for n, x in zip(GRAD_NAMES, outs)})
            res["lines"] = pg
    else:
        n_dev = torch.tensor([I, I], dtype=torch.int64, device=dev)
        fn = L.clmgs_rasterize4_bwd_dev if nch == 4 else L.clmgs_rasterize_bwd_dev
        _lib.check(fn(st, 1, N, cap, _p(n_dev), _p(packed), _p(bg), w, h, 16, tw, th, _p(off), _p(fids), _p(al), _p(last),
                      _p(v), _p(va), _p(sd), _p(rd), _p(parts)))
    torch.cuda.synchronize()
    res["parts"] = parts
    res["row_of_slot"] = torch.empty(I, dtype=torch.long).scatter_(0, slot.long(), case["fids"].long())
    return {k: t.cpu() for k, t in res.items()}


@functools.lru_cache(maxsize=None)
def _slot_runs(name):
    dev = torch.device("cuda:0")
    case, z, bgd, vd = _slot_case(name)
    atomic = RD.run4(case, z, bgd, vd, dev)  # forward + the atomic route
    atomic["bgd"] = bgd
    v4 = torch.cat([case["vi"], vd[..., None]], -1)
    slot = _slot_backward(case, atomic, v4, dev)
    return case, atomic, slot, v4


@pytest.mark.parametrize("name", SLOT_CASES)
def test_slot_route_sums_to_the_atomic_line(dev, name):
    """Per row, the sum of the slot lines against the atomic 4-channel line: GRAD_TOL of tests/test_gpu_raster_edges.py (the
    same per-tile sums, added in another order), per parameter and for the fourth colour's column on its own; and the
    library's per-row sum (word 9 included) against a float64 sum of the lines it read."""
    case, atomic, slot, _ = _slot_runs(name)
    N, I = case["op"].shape[1], case["fids"].numel()
    assert bool(torch.isfinite(slot["parts"][:I]).all()) and not bool((slot["parts"][:I] == SENT).any()), \
        "every line is written"
    for n in GRAD_NAMES:
        x, y = slot[f"slot_{n}"], atomic[f"atomic_{n}"]
        e = rel_l2(x, y)
        print(f"{name} {n}: slot vs atomic rel_l2 {e:.3g}")
        assert e < GRAD_TOL, (name, n, e)
    x, y = slot["slot_colors"][..., 3], atomic["atomic_colors"][..., 3]
    assert float(y.abs().max()) > 0
    e = rel_l2(x, y)
    print(f"{name} colors[..., 3]: slot vs atomic rel_l2 {e:.3g}")
    assert e < GRAD_TOL, (name, e)
    sums = torch.zeros(N, 16, dtype=torch.float64).index_add_(0, slot["row_of_slot"], slot["parts"][:I].double())
    assert rel_l2(slot["lines"][:, :10], sums[:, :10]) < 1e-6
    assert rel_l2(slot["lines"][:, 9], sums[:, 9]) < 1e-6
    assert float(slot["lines"][:, 10:12].abs().max()) == 0.0 and float(slot["parts"][:I, 10:].abs().max()) == 0.0
    untouched = torch.ones(N, dtype=torch.bool)
    untouched[case["fids"].long()] = False
    assert float(slot["lines"][untouched, :12].abs().max() if bool(untouched.any()) else 0.0) == 0.0


@pytest.mark.parametrize("name", SLOT_CASES)
def test_zero_fourth_cotangent_gives_the_three_channel_lines(dev, name):
    case, atomic, _, v4 = _slot_runs(name)
    I = case["fids"].numel()
    v0 = v4.clone()
    v0[..., 3] = 0.0
    four = _slot_backward(case, atomic, v0, dev, unpack=False)["parts"][:I]
    three = _slot_backward(case, atomic, case["vi"], dev, nch=3, unpack=False)["parts"][:I]
    assert not bool((three == SENT).any()) and float(three.abs().max()) > 0
    assert bool((four[:, :9] == three[:, :9]).all())
    assert float(four[:, 9:].abs().max()) == 0.0


@pytest.mark.parametrize("name", ["small70x37", "special", "list129_sat_middle"])
@pytest.mark.parametrize("extra", [0, 37], ids=["capacity=count", "capacity>count"])
def test_dev_forms_equal_the_exact_forms(dev, name, extra):
    from clm_gs_amd import _lib
    L = _lib.lib()
    case, atomic, slot, v4 = _slot_runs(name)
    N, I = case["op"].shape[1], case["fids"].numel()
    w, h = case["w"], case["h"]
    cap = I + extra
    fids = torch.cat([case["fids"].to(torch.int32), torch.zeros(extra, dtype=torch.int32)]).to(dev)
    n_dev = torch.tensor([I, I], dtype=torch.int64, device=dev)
    bg = RD.bg4_of(case, atomic["bgd"])
    bg = bg.to(dev).contiguous() if bg is not None else None
    out = torch.full((1, h, w, 4), float("nan"), device=dev)
    al = torch.full((1, h, w), float("nan"), device=dev)
    last = torch.full((1, h, w), -7, dtype=torch.int32, device=dev)
    packed, off = atomic["packed"].to(dev).contiguous(), case["off"].to(dev).contiguous()
    _lib.check(L.clmgs_rasterize4_fwd_dev(_lib.stream(), 1, N, cap, _p(n_dev), _p(bg), w, h, 16, math.ceil(w / 16),
                                          math.ceil(h / 16), _p(off), _p(fids), _p(packed), _p(out), _p(al), _p(last)))
    torch.cuda.synchronize()
    assert torch.equal(out[..., :3].cpu(), atomic["img"]) and torch.equal(out[..., 3].cpu(), atomic["depth"])
    assert torch.equal(al.cpu(), atomic["alpha"]) and torch.equal(last.cpu(), atomic["last"])
    got = _slot_backward(case, atomic, v4, dev, dev_capacity=cap)["parts"]
    assert torch.equal(got[:I], slot["parts"][:I])
    assert bool((got[I:] == SENT).all()), "lines past the count are not written"


# ------------------------------------------------------------------------------------------- row kernel
ROW_COUNTS = (0, 1, 4, 5, 9, 2)


@pytest.mark.parametrize("table", ["n3", "n12"])
@pytest.mark.parametrize("filtered", [False, True], ids=["all_rows", "filter"])
@pytest.mark.parametrize("source", ["partials", "atomic_line"])
def test_row_kernel_against_float64(dev, table, filtered, source):
    from clm_gs_amd import _lib
    L = _lib.lib()
    V = 333
    gen = torch.Generator().manual_seed(17)
    N = 500 if filtered else V
    filt = torch.randperm(N, generator=gen)[:V].contiguous() if filtered else None
    radii = torch.randint(-1, 30, (V,), generator=gen, dtype=torch.int32)
    radii[:12] = 5  # every count of ROW_COUNTS on visible rows
    depths = 0.5 + 20.0 * torch.rand(V, generator=gen)
    cnt = torch.tensor([ROW_COUNTS[i % len(ROW_COUNTS)] for i in range(V)])
    row_cum = torch.cumsum(cnt, 0)
    n_lines = int(row_cum[-1])
    parts = torch.randn(n_lines, 16, generator=gen)
    lines = torch.randn(V, 16, generator=gen)
    vm = np.ascontiguousarray(torch.randn(4, 4, generator=gen).numpy().astype(np.float32).reshape(16))
    pitch = 3 if table == "n3" else 12
    before = torch.randn(N, pitch, generator=gen)
    g = before.clone().to(dev)
    pd, ld = parts.to(dev), lines.to(dev)
    fd, rd, dd, cd = (filt.to(dev) if filtered else None), radii.to(dev), depths.to(dev), row_cum.to(dev)
    _lib.check(L.clmgs_invdepth_rows_bwd(
        _lib.stream(), V, _p(fd), _p(rd), _p(dd), vm.ctypes.data_as(ctypes.c_void_p),
        _p(pd) if source == "partials" else None, _p(cd) if source == "partials" else None,
        _p(ld) if source == "atomic_line" else None, _p(g), 1 if table == "n12" else 0))
    torch.cuda.synchronize()
    got = g.cpu()
    # float64: g_d = the row's sum of word 9, dL/dz = -g_d / z^2, xyz += dL/dz * R[2,:]
    if source == "partials":
        row_of = torch.repeat_interleave(torch.arange(V), cnt)
        g_d = torch.zeros(V, dtype=torch.float64).index_add_(0, row_of, parts[:, 9].double())
        mag = torch.zeros(V, dtype=torch.float64).index_add_(0, row_of, parts[:, 9].double().abs())
    else:
        g_d, mag = lines[:, 9].double(), lines[:, 9].double().abs()
    vis = radii > 0
    r2 = torch.from_numpy(vm.reshape(4, 4)[2, :3].copy()).double()
    add = (-g_d / depths.double() ** 2)[:, None] * r2[None, :]
    add_mag = (mag / depths.double() ** 2)[:, None] * r2.abs()[None, :]
    rows = filt if filtered else torch.arange(V)
    want = before.double().clone()
    want[rows[vis], :3] += add[vis]
    err = (got.double() - want).abs()
    bound = torch.zeros_like(want)
    bound[rows[vis], :3] = 16 * U * (before.double()[rows[vis], :3].abs() + add_mag[vis])  # <= 9 sums, z^2, /, fma
    assert bool((err <= bound).all()), float((err - bound).max())
    assert float(add[vis].abs().max()) > 0.1
    # exactly untouched: rows that are not visible or not in the filter, and words 3..11 of a packed row
    keep = torch.ones(N, dtype=torch.bool)
    keep[rows[vis]] = False
    assert torch.equal(got[keep], before[keep])
    assert torch.equal(got[:, 3:], before[:, 3:])
    zero_rows = rows[vis & (cnt == 0)] if source == "partials" else rows[:0]
    assert torch.equal(got[zero_rows], before[zero_rows]), "a visible row without a line adds -0 / z^2 = 0"


def test_row_kernel_rejects_bad_arguments(dev):
    from clm_gs_amd import _lib
    L = _lib.lib()
    V = 8
    radii, depths = torch.ones(V, dtype=torch.int32, device=dev), torch.ones(V, device=dev)
    parts, lines = torch.zeros(V, 16, device=dev), torch.zeros(V, 16, device=dev)
    cum = torch.arange(1, V + 1, dtype=torch.int64, device=dev)
    g = torch.full((V, 3), SENT, device=dev)
    vm = np.eye(4, dtype=np.float32).reshape(16)
    vp = vm.ctypes.data_as(ctypes.c_void_p)
    st = _lib.stream()
    for args in [(V, None, _p(radii), _p(depths), vp, None, None, None, _p(g), 0),               # no source
                 (V, None, _p(radii), _p(depths), vp, _p(parts), _p(cum), _p(lines), _p(g), 0),  # both sources
                 (V, None, _p(radii), _p(depths), vp, _p(parts), None, None, _p(g), 0),          # partials without row_cum
                 (V, None, _p(radii), _p(depths), None, _p(parts), _p(cum), None, _p(g), 0),     # no viewmat
                 (V, None, _p(radii), _p(depths), vp, _p(parts), _p(cum), None, None, 0),        # no table
                 (V, None, _p(radii), _p(depths), vp, _p(parts), _p(cum), None, _p(g), 2),
                 (-1, None, _p(radii), _p(depths), vp, _p(parts), _p(cum), None, _p(g), 0)]:
        assert L.clmgs_invdepth_rows_bwd(st, *args) == EINVAL
    torch.cuda.synchronize()
    assert bool((g == SENT).all())


# ------------------------------------------------------------------------------------------- engines
W, H, N, BSZ = ML.W, ML.H, ML.N, ML.BSZ
PRIOR = (0, 1, 2)   # these cameras carry a prior,
MASKED = (1, 2)     # these a loss mask as well,
EXPOSED = 2         # this one an exposure too; camera 3 carries nothing
DELTA = 2e-3        # the priors lie DELTA off the float64 render, + / - on a checkerboard of 8x8-pixel cells
CELL = 8


def _mask():
    return ML._camera_masks()[0]


def _exposure_row():
    return EX._exposures()[EXPOSED]


def _render64(P, c):
    vm = c.world_view_transform.t().cpu().double()
    return R.render_with_inverse_depth(P["xyz"], torch.sigmoid(P["opacity"]), torch.exp(P["scaling"]),
                                       torch.nn.functional.normalize(P["rotation"]), P["shs48"].reshape(-1, 16, 3), 3, vm,
                                       c.K.cpu().double(), W, H)


@functools.lru_cache(maxsize=None)
def _float64_batch(priors=True):
    """The float64 render (image, I) of every camera, the priors built from it, the restated losses and their gradients.
    -> (losses, gradients, priors [(raw, scale, offset)], depth weight)"""
    from clm_gs_amd import utils
    _, sc, cams = ML._setup("no_offload", masks="none")
    weight = utils.depth_l1_weight()
    P = {k: sc[k].detach().cpu().double().requires_grad_() for k in ("xyz", "opacity", "scaling", "rotation", "shs48")}
    E = _exposure_row().double()
    yy, xx = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
    board = (((yy // CELL) + (xx // CELL)) % 2 * 2 - 1).double()
    losses, pri = [], []
    for i, c in enumerate(cams):
        img, I = _render64(P, c)
        mask = _mask() if i in MASKED else None
        if i == EXPOSED:
            img = EX.R.apply(img, E)
        l = M.masked_loss(img, c.original_image.cpu(), mask, 0.2)
        if i in PRIOR:
            I0 = I.detach()
            scale = float(np.float32(float(I0.max()) + 8 * DELTA))
            offset = float(np.float32(-4 * DELTA))
            assert scale / 65536 < DELTA / 4, "the uint16 grid is finer than DELTA / 4"
            raw = torch.round((I0 + board * DELTA - offset) / scale * 65536)
            assert float(raw.min()) >= 0 and float(raw.max()) <= 65535
            raw = raw.to(torch.int32).to(torch.uint16)
            gap = (I0 - R.prior_of(raw, scale, offset)).abs()
            counted = gap if mask is None else gap[mask != 0]
            # no counted pixel is excluded, and no sign can flip between the float32 and the float64 render
            assert float(counted.min()) >= 1e-4, float(counted.min())
            assert float(I0.max()) > 0.01, float(I0.max())
            pri.append((raw, scale, offset))
            if priors:
                l = l + R.depth_term(I, raw, scale, offset, weight, mask)
        else:
            pri.append(None)
        l.backward()
        losses.append(l.item())
    grads = {"xyz": P["xyz"].grad, "opacity": P["opacity"].grad.reshape(N, -1), "scaling": P["scaling"].grad,
             "rotation": P["rotation"].grad, "shs": P["shs48"].grad.reshape(N, 48)}
    return losses, grads, pri, weight


def _attach(cams, priors=True):
    from clm_gs_amd.exposure import ExposureModel
    model = ExposureModel(BSZ, "cuda")
    with torch.no_grad():
        model.param[EXPOSED].copy_(_exposure_row())
    model.attach(cams)
    for i, c in enumerate(cams):
        if i != EXPOSED:
            c.exposure, c.exposure_grad = None, None
        if i in MASKED:
            c.loss_mask, c.loss_mask_count = _mask().cuda(), int((_mask() != 0).sum())
        if priors and i in PRIOR:
            raw, scale, offset = _float64_batch()[2][i]
            c.invdepth, c.invdepth_scale, c.invdepth_offset = raw.cuda(), scale, offset
    return model


_RUNS = {}


def _batch(strategy, residency="hbm", fused=True, priors=True, **over):
    """tests/test_gpu_exposure.py's _batch with the priors (and the masks and the one exposure) on the cameras."""
    key = (strategy, residency, fused, priors, tuple(sorted(over.items())))
    if key in _RUNS:
        return _RUNS[key]
    if priors:
        _float64_batch()  # (sets the process-wide args itself: before this batch's own)
    args, sc, cams = ML._setup(strategy, residency, "none", fused, debug_skip_optimizer=True,
                               stop_update_param=strategy == "naive_offload", **over)
    _attach(cams, priors)
    m = ML._make(strategy, sc, args)
    if strategy == "no_offload":
        from clm_gs_amd.strategies.no_offload import baseline_accumGrads_impl
        losses, _ = baseline_accumGrads_impl(m, ML._Scene, cams, None)
        order = list(range(BSZ))
        gsh = torch.cat((m._features_dc.grad, m._features_rest.grad), dim=1).reshape(-1, 48)
        small = [m._xyz.grad, m._opacity.grad, m._scaling.grad, m._rotation.grad]
    elif strategy == "naive_offload":
        from clm_gs_amd.strategies.naive_offload import naive_offload_train_one_batch
        m.optimizer.zero_grad = lambda *a, **k: None  # the engine ends by dropping the gradients this test reads
        losses, _ = naive_offload_train_one_batch(m, ML._Scene, cams, None)
        order = list(range(BSZ))
        gk, gsh = m._small.grad, m._parameters.grad
        small = [gk[:, 0:3], gk[:, 3:4], gk[:, 4:7], gk[:, 7:11]]
    else:
        from clm_gs_amd.strategies.clm_offload import clm_offload_train_one_batch
        comm = torch.cuda.Stream()
        gen = torch.Generator(device="cuda").manual_seed(1)
        losses, order, _ = clm_offload_train_one_batch(m, ML._Scene, cams, m.parameters_grad_buffer, None, None, comm, gen)
        torch.cuda.synchronize()
        gsh = m.parameters_grad_buffer[:N]
        if residency == "hbm" and fused:
            gk = m.small_grad()
            small = [gk[:, 0:3], gk[:, 3:4], gk[:, 4:7], gk[:, 7:11]]
        else:
            small = [m._xyz.grad, m._opacity.grad, m._scaling.grad, m._rotation.grad]
    torch.cuda.synchronize()
    lo = [0.0] * BSZ
    for k, l in zip(order, losses):
        lo[k] = l.item()
    names = ("xyz", "opacity", "scaling", "rotation")
    r = dict(losses=lo, grads={**{n: t.detach().cpu().reshape(N, -1).clone() for n, t in zip(names, small)},
                               "shs": gsh.detach().cpu().reshape(N, 48).clone()})
    _RUNS[key] = r
    return r


@pytest.mark.parametrize("mode", EX.ENGINE_MODES, ids=lambda m: f"{m[0]}-{m[1]}-{'fused' if m[2] else 'op_by_op'}")
def test_engines_with_priors_match_the_float64_composition(dev, mode):
    want_l, want_g, _, weight = _float64_batch()
    plain_l, plain_g, _, _ = _float64_batch(False)
    b = _batch(*mode)
    for i, (u, v) in enumerate(zip(b["losses"], want_l)):
        print(f"{mode} camera {i}: loss {u:.7f} vs {v:.7f} (float64 without the depth term {plain_l[i]:.7f}, weight {weight:.6f})")
        assert abs(u - v) < 2e-5, (mode, i)
        if i in PRIOR:
            assert v - plain_l[i] > 20 * 2e-5, "the depth term is well above the gate it is held to"
    for k in b["grads"]:
        e = rel_l2(b["grads"][k], want_g[k])
        share = rel_l2(plain_g[k], want_g[k])
        print(f"{mode}: {k} gradient rel_l2 {e:.3g} (the depth term's share of the float64 gradient: {share:.3g})")
        assert e < 1e-3, (mode, k, e)
    # the depth term's own part of the gradient: this batch minus the same batch without priors, against the same
    # difference in float64.  Each run is within 1e-3 of its float64 gradient, so the difference is known to 2e-3 / share;
    # compared wherever that still says something (a missing or sign-flipped part reads 1 or 2).
    plain = _batch(*mode, priors=False)
    for k in b["grads"]:
        share = rel_l2(plain_g[k], want_g[k])
        if share == 0.0:  # the SH rows: colours receive nothing from the fourth channel
            continue
        tol = 2e-3 / share
        e = rel_l2(b["grads"][k] - plain["grads"][k], want_g[k] - plain_g[k])
        print(f"{mode}: {k} depth part rel_l2 {e:.3g} (known to {tol:.3g})")
        if tol < 0.5:
            assert e < tol, (mode, k, e, tol)


def test_camera_without_a_prior_reports_the_plain_loss(dev):
    """Against the same batch without any prior: the camera that carries nothing reports the same loss, the others
    another; and against tests/test_gpu_masked_loss.py's plain batch, where that camera carries nothing either."""
    for mode in (("clm_offload", "hbm", True), ("no_offload", "hbm", True), ("no_offload", "hbm", False)):
        a, b = _batch(*mode), _batch(*mode, priors=False)
        for i, (u, v) in enumerate(zip(a["losses"], b["losses"])):
            if i in PRIOR:
                assert u - v > 4e-4, (mode, i, u, v)
            else:
                assert u == v, (mode, i, u, v)
    assert _batch("clm_offload")["losses"][3] == ML._batch("clm_offload", masks="none")["losses"][3]


@pytest.mark.parametrize("mode", [("clm_offload", "hbm", True), ("clm_offload", "host", True), ("no_offload", "hbm", True),
                                  ("naive_offload", "hbm", True)],
                         ids=lambda m: f"{m[0]}-{m[1]}")
def test_weight_zero_gives_the_gradients_of_the_batch_without_priors(dev, mode):
    """Weight 0: the fourth cotangent is +-0, every product it enters is a zero that is added to a sum -- the gradients
    compare equal (==) to those of the batch without priors, whose cameras run the 3-channel kernels."""
    a = _batch(*mode, depth_l1_weight_init=0.0, depth_l1_weight_final=0.0)
    b = _batch(*mode, priors=False)
    for k in a["grads"]:
        assert bool((a["grads"][k] == b["grads"][k]).all()), (mode, k)
    for i, (u, v) in enumerate(zip(a["losses"], b["losses"])):
        print(f"{mode} camera {i}: loss {u!r} at weight 0, {v!r} without priors")
        assert abs(u - v) < 1e-6, (mode, i, u, v)


def test_capacity_redo_counts_the_depth_term_once(dev):
    """tests/test_gpu_exposure.py's capacity pattern: every camera of the second batch is found over capacity and redone
    exactly; losses (the term from the partial rows of the accepted forward) and the trained model have the bits of the
    exact-size run."""
    def attach(cams):
        gen = torch.Generator().manual_seed(3)
        for c in cams:
            c.invdepth = torch.randint(0, 65536, (GE.H, GE.W), generator=gen, dtype=torch.int32).to(torch.uint16).cuda()
            c.invdepth_scale, c.invdepth_offset = 0.5, 0.01
        return None
    l_plain, t_plain, _, _ = EX._two_batches(None, dict(device_side_counts=False))
    l_exact, t_exact, _, redo_exact = EX._two_batches(attach, dict(device_side_counts=False))
    l_over, t_over, _, redo_over = EX._two_batches(attach, dict(device_side_counts=True, isect_capacity_margin=0.5,
                                                                 isect_capacity_floor=0))
    assert redo_exact == 0 and redo_over >= GE.BSZ, (redo_exact, redo_over)
    assert l_over == l_exact
    assert all(a - b > 1e-3 for a, b in zip(l_exact, l_plain)), "the term is in the loss"
    for a, b in zip(t_over, t_exact):
        assert torch.equal(a, b)
    assert not torch.equal(t_exact[0], t_plain[0]), "the term moves the positions"


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "op_by_op"])
def test_absgrad_with_a_prior_raises(dev, fused):
    from clm_gs_amd.strategies.no_offload import baseline_accumGrads_impl
    _float64_batch()
    args, sc, cams = ML._setup("no_offload", "hbm", "none", fused, debug_skip_optimizer=True, absgrad=True)
    _attach(cams)
    m = ML._make("no_offload", sc, args)
    with pytest.raises(ValueError, match="absgrad"):
        baseline_accumGrads_impl(m, ML._Scene, cams, None)
    torch.cuda.synchronize()
    assert m._xyz.grad is None or float(m._xyz.grad.abs().max()) == 0.0, "nothing ran"


@pytest.mark.parametrize("strategy,fused", [("clm_offload", True), ("clm_offload", False), ("no_offload", True),
                                            ("no_offload", False), ("naive_offload", True)])
def test_absgrad_refusal_covers_the_whole_batch(dev, strategy, fused):
    """The prior sits on the LAST camera only: the engines check the batch at their entry, so the cameras in front of it
    have not run when the ValueError comes (no gradient anywhere)."""
    args, sc, cams = ML._setup(strategy, "hbm", "none", fused, debug_skip_optimizer=True, absgrad=True,
                               stop_update_param=strategy == "naive_offload")
    cams[-1].invdepth = torch.zeros((H, W), dtype=torch.int32).to(torch.uint16).cuda()
    cams[-1].invdepth_scale, cams[-1].invdepth_offset = 1.0, 0.0
    m = ML._make(strategy, sc, args)
    with pytest.raises(ValueError, match="absgrad"):
        if strategy == "no_offload":
            from clm_gs_amd.strategies.no_offload import baseline_accumGrads_impl
            baseline_accumGrads_impl(m, ML._Scene, cams, None)
        elif strategy == "naive_offload":
            from clm_gs_amd.strategies.naive_offload import naive_offload_train_one_batch
            naive_offload_train_one_batch(m, ML._Scene, cams, None)
        else:
            from clm_gs_amd.strategies.clm_offload import clm_offload_train_one_batch
            clm_offload_train_one_batch(m, ML._Scene, cams, m.parameters_grad_buffer, None, None, torch.cuda.Stream(),
                                        torch.Generator(device="cuda").manual_seed(1))
    torch.cuda.synchronize()
    for t in (m._xyz, m._opacity, m._scaling, m._rotation):
        assert t.grad is None or float(t.grad.abs().max()) == 0.0, "a camera ran before the refusal"


# ------------------------------------------------------------------------------------------- trainer
def _losses_of(log):
    return [float(x) for line in re.findall(r"loss: (.*?) (?:depth_l1_weight|image)", log) for x in line.split()]


@pytest.mark.parametrize("strategy", ["clm_offload", "no_offload", "naive_offload"])
def test_trainer_with_depths(dev, tmp_path, strategy):
    from PIL import Image
    from clm_gs_amd import trainer
    from clm_gs_amd.cameras import camera_invdepth
    from clm_gs_amd.io_ply import load_ply
    work = EX._tiny_scene(tmp_path)
    from clm_gs_amd.colmap_scene import load_colmap_scene
    cams = load_colmap_scene(str(work), device="cuda", load_images=False).train_cameras
    os.makedirs(work / "depths")
    g = np.random.default_rng(1)
    for c in cams:
        raw = g.integers(0, 65536, size=(c.image_height, c.image_width), dtype=np.uint16)
        Image.fromarray(raw).save(work / "depths" / f"{c.image_name}.png")
    with open(work / "sparse" / "0" / "depth_params.json", "w") as f:
        json.dump({c.image_name: {"scale": 0.4, "offset": 0.05} for c in cams}, f)
    logs = {}
    for tag, extra in (("with", dict(depths="depths")), ("without", {})):
        out = tmp_path / f"out_{tag}"
        gaussians, scene, _ = trainer.train_from_colmap(str(work), str(out), strategy=strategy, iterations=8, bsz=4,
                                                        disable_auto_densification=True, **extra)
        assert all((camera_invdepth(c) is not None) == (tag == "with") for c in scene.train_cameras)
        logs[tag] = open(out / "python_ws=1_rk=0.log").read()
        ply = out / "point_cloud" / "iteration_8" / "point_cloud.ply"
        assert os.path.exists(ply)
        for k, t in load_ply(str(ply)).items():
            assert bool(torch.isfinite(t).all()), f"the written model is finite: {k}"
    a, b = _losses_of(logs["with"]), _losses_of(logs["without"])
    print(f"{strategy}: logged losses with --depths {a}, without {b}")
    assert len(a) == len(b) == 8 and all(math.isfinite(x) for x in a)
    assert all(x - y > 1e-3 for x, y in zip(a[:4], b[:4])), "the first batch sees the same model: the term is the difference"
    assert "depth_l1_weight: " in logs["with"] and "depth_l1_weight" not in logs["without"]
    w = [float(x) for x in re.findall(r"depth_l1_weight: ([0-9.]+)", logs["with"])]
    assert len(w) == 2 and 0.0 < w[1] < w[0] <= 1.0
