"""-m gpu: every form of the Adam kernels (clm_ops.hip) against the float64 restatement of the step in
tests/adam_reference.py, element by element under its error budget, on the input classes of tests/adam_cases.py (every
class in every test).  eps 1e-15, betas (0.9, 0.999) and (0.9^4, 0.999^4), learning rate 2.5e-3 for 3 columns and
1.25e-4 for the rest, grad_scale 0.25.  Every test prints its largest error / bound per quantity and input class."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from tests import adam_cases as C
from tests import adam_reference as R

pytestmark = pytest.mark.gpu

N_ROWS = 2048
FORMS = {"48": (48, 0), "3": (3, 0), "8": (8, 0), "48 unaligned": (48, 1)}


def _table(x, off=0):
    """Device copy of a host [n, cols] table, `off` floats past an allocation's (aligned) start."""
    n, cols = x.shape
    t = torch.empty(n * cols + off, device="cuda", dtype=torch.float32)[off:].view(n, cols)
    t.copy_(torch.from_numpy(np.array(x)))
    return t


def _bits(t):
    return (t.cpu().numpy() if isinstance(t, torch.Tensor) else t).view(np.uint32)


def _same_bits(a, b, rows=None):
    a, b = _bits(a), _bits(b)
    return np.array_equal(a, b) if rows is None else np.array_equal(a[rows], b[rows])


@functools.lru_cache(maxsize=None)
def _inputs(cols, seed=21):
    p, m, v, g, cls = C.input_classes(N_ROWS, cols, seed)
    for x in (p, m, v, g):
        x.setflags(write=False)
    return p, m, v, g, cls


# ------------------------------------------------------------------------------------------------ clmgs_adam_rows
def _kept(store, group, key, make):
    """make() once per key while `group` (a step count, a (last, to_step) pair) stays the same: the forms of one group
    share their references whatever the order of the tests, and those of the groups before it are dropped."""
    if store.get("group") != group:
        store.clear()
        store["group"] = group
    if key not in store:
        store[key] = make()
    return store[key]


_EAGER, _LAZY = {}, {}


def _eager_ref(cols, betas, step, with_g, bias):
    """step64 (+ the rounding of p) of the whole table, after the float32 emulation of the same step has come back
    finite."""
    def make():
        p, m, v, g, _ = _inputs(cols)
        args = (g if with_g else None, C.col_lr(cols), betas[0], betas[1], C.EPS, step, bias, C.GRAD_SCALE)
        assert all(np.isfinite(x).all() for x in C.emulate_rows(p, m, v, *args)), "non-finite on the CPU: not launched"
        return C.one_step(p, m, v, *args)
    return _kept(_EAGER, step, (cols, betas, with_g, bias), make)


@pytest.mark.parametrize("form", ["48", "3", "48 unaligned"])
@pytest.mark.parametrize("step", [1, 2, 7, 1000, 30000])
def test_adam_rows_within_the_bounds(dev, form, step):
    """adam_rows_kernel, float4 form (48 columns), scalar forms (3 columns; 48 columns one float off alignment): 1024
    listed rows of 2048 as int32 and int64 lists, rows = None, g = None, the mask route of selective_adam_update (no bias
    correction), zero_grad 0 and 1, both betas, against step64.  Rows not listed or masked out are bit-identical in every
    table; g is cleared on the stepped rows with zero_grad and kept exactly without.
    Largest error / bound measured on an MI355X, the same at every step count: 48 columns (aligned = unaligned)
    p 1.000 m 0.500 v 0.433; 3 columns p 0.998 m 0.444 v 0.359; selective_adam_update p 0.998 m 0.425 v 0.358.  The 1.000
    of p is the rounding of p itself where |p| ~ 1 (classes a, e, g: half an ulp of p is the whole bound there); where
    the step is resolved p reaches 0.828 (class b) and 0.180 (class d)."""
    from clm_gs_amd import clm_kernels as K
    cols, off = FORMS[form]
    p0, m0, v0, g0, cls = _inputs(cols)
    lr = torch.from_numpy(C.col_lr(cols)).cuda()
    gen = torch.Generator().manual_seed(4)
    listed = np.zeros(N_ROWS, dtype=bool)
    listed[torch.randperm(N_ROWS, generator=gen)[:1024].numpy()] = True
    order = torch.from_numpy(np.nonzero(listed)[0])[torch.randperm(1024, generator=gen)]
    mask = torch.rand(N_ROWS, generator=gen) > 0.5
    everyone = np.ones(N_ROWS, dtype=bool)
    # (rows, mask, with_g, bias, zero_grad, rows stepped)
    variants = (("int32", order.int().cuda(), None, True, True, 1, listed),
                ("int64", order.long().cuda(), None, True, True, 0, listed),
                ("all rows", None, None, True, True, 1, everyone),
                ("g = None", order.int().cuda(), None, False, True, 0, listed),
                ("mask", None, mask.cuda(), True, False, 0, mask.numpy()))
    worst = dict(p=0.0, m=0.0, v=0.0)
    for betas in C.BETAS:
        for name, rows, msk, with_g, bias, zero_grad, stepped in variants:
            want = _eager_ref(cols, betas, step, with_g, bias)  # (and the CPU emulation: finite before the launch)
            p, m, v, g = (_table(x, off) for x in (p0, m0, v0, g0))
            K.adam_rows(p, g if with_g else None, m, v, rows, lr, betas[0], betas[1], C.EPS, step, bias, C.GRAD_SCALE,
                        bool(zero_grad), mask=msk)
            got = [x.cpu().numpy() for x in (p, m, v)]
            w = C.report(f"adam_rows {form} step {step} betas {betas[0]:.4f} {name}", cls, p0, got, want,
                         rows=np.nonzero(stepped)[0])
            worst = {q: max(worst[q], w[q]) for q in worst}
            for x, x0 in zip(got, (p0, m0, v0)):
                assert _same_bits(x, x0, ~stepped), name
            assert _same_bits(g, g0, ~stepped)
            if zero_grad and with_g:
                assert not g.cpu().numpy()[stepped].any()
            else:
                assert _same_bits(g, g0)
            is_c = stepped & (cls == C.CLASSES.index("c"))
            assert _same_bits(got[0], p0, is_c) and not got[1][is_c].any() and not got[2][is_c].any()
    if cols == 3:  # selective_adam_update itself: one learning rate, step 1, no bias correction, unscaled gradients
        sel_args = (g0, np.float32(1e-3), 0.9, 0.999, C.EPS, 1, False, 1.0)
        assert all(np.isfinite(x).all() for x in C.emulate_rows(p0, m0, v0, *sel_args))
        p, m, v, g = (_table(x) for x in (p0, m0, v0, g0))
        K.selective_adam_update(p, g, m, v, mask.cuda(), 1e-3, 0.9, 0.999, C.EPS, N_ROWS, cols)
        want = C.one_step(p0, m0, v0, *sel_args)
        C.report("selective_adam_update", cls, p0, [x.cpu().numpy() for x in (p, m, v)], want,
                 rows=np.nonzero(mask.numpy())[0])
        assert _same_bits(p, p0, ~mask.numpy()) and _same_bits(g, g0)
    print(f"adam_rows {form} step {step}: largest error / bound over all variants  p {worst['p']:.3f} "
          f"m {worst['m']:.3f} v {worst['v']:.3f}")


# ------------------------------------------------------------------------------------------------ clmgs_adam_catch_up
# name -> (last low, last high (inclusive), to_step, max_replay)
PAIRS = {"0 to 1": (0, 0, 1, 256), "0 to 2": (0, 0, 2, 256), "0 to 14": (0, 0, 14, 256),
         "3..11 to 14": (3, 11, 14, 256), "990..1010 to 1014": (990, 1010, 1014, 256), "10 to 310": (10, 10, 310, 256),
         "10 to 30, max_replay 4": (10, 10, 30, 4)}


@functools.lru_cache(maxsize=None)
def _lazy_state(pair):
    """last [n], g_step [n] and the listed rows of one (last, to_step) pair: three quarters of the rows listed (an
    eighth for the pair 300 steps apart); a third of the rows with a gradient due, some stamps <= last (consumed
    leftovers), some > to_step (not due yet)."""
    lo, hi, to_step, _ = PAIRS[pair]
    rng = np.random.default_rng(6)
    last = rng.integers(lo, hi + 1, N_ROWS).astype(np.int32)
    kind = rng.integers(0, 9, N_ROWS)  # 0-2 waiting, 3 consumed, 4 not due, else none
    u = rng.random(N_ROWS)
    waiting = np.minimum(last + 1 + (u * (to_step - last)).astype(np.int32), to_step)
    g_step = np.where(kind < 3, waiting, 0)
    g_step = np.where(kind == 3, np.minimum((u * (last + 1)).astype(np.int32), last), g_step)
    g_step = np.where(kind == 4, to_step + 1 + (u * 3).astype(np.int32), g_step).astype(np.int32)
    listed = np.zeros(N_ROWS, dtype=bool)
    # (300 steps of float64 reference on 1536 x 48 elements take seconds on the host: that pair lists 256 rows)
    listed[rng.permutation(N_ROWS)[:N_ROWS * 3 // 4 if to_step - lo <= 64 else 256]] = True
    pending = (g_step > last) & (g_step <= to_step)
    assert 0.25 < pending.mean() < 0.42 and ((g_step > 0) & (g_step <= last)).sum() + (lo == 0) > 0
    return last, g_step, listed


def _lazy_ref(pair, cols, betas, with_g, bias):
    """replay64 of the listed rows, after the float32 emulation of the same replay has come back finite."""
    return _kept(_LAZY, pair, (cols, betas, with_g, bias), lambda: _lazy_make(pair, cols, betas, with_g, bias))


def _lazy_make(pair, cols, betas, with_g, bias):
    p, m, v, g, _ = _inputs(cols)
    last, g_step, listed = _lazy_state(pair)
    _, _, to_step, max_replay = PAIRS[pair]
    rows = np.nonzero(listed)[0]
    emu = C.emulate_replay(p[rows], m[rows], v[rows], g[rows] if with_g else None, last[rows], g_step[rows], to_step,
                           C.col_lr(cols), betas[0], betas[1], C.EPS, bias, C.GRAD_SCALE, max_replay)
    assert all(np.isfinite(x).all() for x in emu), "non-finite on the CPU: not launched"
    return R.replay64(p[rows], m[rows], v[rows], g[rows] if with_g else None, last[rows],
                      g_step[rows] if with_g else None, to_step, C.col_lr(cols), betas[0], betas[1], C.EPS, bias,
                      C.GRAD_SCALE, max_replay)


@pytest.mark.parametrize("form", ["48", "8", "48 unaligned"])
@pytest.mark.parametrize("pair", list(PAIRS))
def test_adam_catch_up_within_the_bounds(dev, form, pair):
    """adam_catch_up48_kernel (48 columns), adam_catch_up_kernel float4 (8 columns) and scalar (48 columns one float off
    alignment) against replay64: 2048 rows, 1536 listed (256 for the pair 300 steps apart); rows never stepped
    (last = 0), step counts of 14 and of a thousand, 300 steps behind with max_replay 256 and 20 behind with
    max_replay 4; with and without waiting gradients (keep_grad 0 and 1), bias_correction 1 and 0, both betas (int64
    row lists, int32 with keep_grad).  Rows outside the list, gradient lines not consumed and
    all-zero rows are bit-identical.  Also printed: the relative error of the whole displacement of the rows whose step is
    (lr / bc1) m / eps (class d: v = 0, p = 0) and of the p = 0 elements of class b (lr / bc1 m sqrt(bc2) / sqrt(v)),
    without gradients: what the device's 1 / bc1 and 1 / sqrt(bc2) are off by, to within the few roundings of the rest.
    Largest error / bound measured on an MI355X over all pairs: 48 columns (aligned = unaligned) p 1.000 m 0.611
    v 0.433, 8 columns p 0.999 m 0.528 v 0.385; p where the step is resolved: 0.632 (class b), 0.173 (class d).
    Relative error of the displacement, betas (0.9, 0.999) / (0.9^4, 0.999^4), where it is lr/bc1 m/eps and where it is
    lr/bc1 m sqrt(bc2)/sqrt(v):
      0 to 1              2.3e-7 / 1.4e-7    6.9e-6 / 2.2e-6
      0 to 2              2.1e-7 / 1.3e-7    8.2e-6 / 2.8e-6
      0 to 14             5.0e-7 / 1.9e-7    9.2e-6 / 3.0e-6
      3..11 to 14         3.0e-7 / 2.1e-7    8.7e-6 / 2.6e-6
      990..1010 to 1014   3.9e-7 / 3.2e-7    4.3e-6 / 6.9e-7
      10 to 310           5.4e-7 / 2.9e-7    7.7e-6 / 3.0e-6
      10 to 30 (4 exact)  2.0e-7 / 9.2e-8    7.3e-6 / 2.6e-6
    (1 / bc1 is good to a few roundings; 1 / sqrt(bc2) carries the float rounding of beta2, 1.3e-8 for 0.999, divided by
    1 - beta2^step: 1e-3 at step 1.)"""
    from clm_gs_amd import clm_kernels as K
    cols, off = FORMS[form]
    _, _, to_step, max_replay = PAIRS[pair]
    p0, m0, v0, g0, cls = _inputs(cols)
    last, g_step, listed = _lazy_state(pair)
    rows_np = np.nonzero(listed)[0]
    rows = torch.from_numpy(rows_np).cuda()
    lr = torch.from_numpy(C.col_lr(cols)).cuda()
    worst = dict(p=0.0, m=0.0, v=0.0)
    for betas in C.BETAS:
        for with_g in (False, True):
            for bias in (True, False):
                ref = _lazy_ref(pair, cols, betas, with_g, bias)
                consumed = np.zeros(N_ROWS, dtype=bool)
                consumed[rows_np] = ref[6]
                for keep_grad in ((0, 1) if with_g else (0,)):
                    p, m, v, g = (_table(x, off) for x in (p0, m0, v0, g0))
                    K.adam_catch_up(p, m, v, torch.from_numpy(last.copy()).cuda(),
                                    rows.int() if keep_grad else rows, lr, betas[0], betas[1], C.EPS, to_step, bias,
                                    max_replay=max_replay, g=g if with_g else None,
                                    g_step=torch.from_numpy(g_step).cuda() if with_g else None,
                                    grad_scale=C.GRAD_SCALE, keep_grad=bool(keep_grad))
                    got = [x.cpu().numpy() for x in (p, m, v)]
                    name = (f"catch_up {form}, {pair}, betas {betas[0]:.4f} gradients {int(with_g)} bias {int(bias)} "
                            f"keep_grad {keep_grad}")
                    w = C.report(name, cls[rows_np], p0[rows_np], [x[rows_np] for x in got], ref[:6])
                    worst = {q: max(worst[q], w[q]) for q in worst}
                    for x, x0 in zip(got, (p0, m0, v0)):
                        assert _same_bits(x, x0, ~listed), "rows outside the list"
                    assert _same_bits(g, g0, ~consumed), "gradient lines that were not consumed"
                    if with_g and not keep_grad:
                        assert not g.cpu().numpy()[consumed].any()
                    else:
                        assert _same_bits(g, g0)
                    is_c = cls == C.CLASSES.index("c")
                    assert _same_bits(got[0], p0, is_c) and not got[1][is_c].any() and not got[2][is_c].any()
                    if bias and not with_g:
                        dp = got[0][rows_np].astype(np.float64) - p0[rows_np].astype(np.float64)
                        cl = cls[rows_np]
                        rel = lambda sel: float(np.max(np.abs(dp[sel] - ref[0][sel]) / np.abs(ref[0][sel])))
                        even = np.broadcast_to((np.arange(cols) % 2 == 0)[None, :], dp.shape)
                        d_rows = (cl == C.CLASSES.index("d"))[:, None] & (ref[0] != 0)
                        b_el = (cl == C.CLASSES.index("b"))[:, None] & even & (ref[0] != 0)
                        print(f"{name}: displacement off by at most {rel(d_rows):.2e} relative where it is lr/bc1 m/eps, "
                              f"{rel(b_el):.2e} where it is lr/bc1 m sqrt(bc2)/sqrt(v)")
    print(f"catch_up {form}, {pair}: largest error / bound over all variants  p {worst['p']:.3f} m {worst['m']:.3f} "
          f"v {worst['v']:.3f}")


# ------------------------------------------------------------------------------------------------ the small attributes
N_SMALL = 256 * 2 + 77
WIDTHS = (3, 1, 3, 4)
LR4 = tuple(float(np.float32(x)) for x in (1.6e-4, 5e-2, 5e-3, 1e-3))  # (the library rounds them to float)


@functools.lru_cache(maxsize=None)
def _small_inputs():
    """The class table cut into the four tensors (xyz 3 | opacity 1 | scaling 3 | rotation 4) and a packed [n, 12]
    gradient table (pad column 0)."""
    p, m, v, g, cls = C.input_classes(N_SMALL, 11, seed=31)
    cut = lambda x: [np.ascontiguousarray(x[:, a:a + w]) for a, w in zip((0, 3, 4, 7), WIDTHS)]
    pg = np.concatenate([g, np.zeros((N_SMALL, 1), np.float32)], axis=1)
    return cut(p), cut(m), cut(v), pg, cls


def _small_device():
    ps, ms, vs, pg, _ = _small_inputs()
    d = [[torch.from_numpy(x).cuda() for x in t] for t in (ps, ms, vs)]
    pk = torch.cat(d[0] + [torch.zeros(N_SMALL, 1, device="cuda")], dim=1).contiguous()
    return d[0], d[1], d[2], pk, torch.from_numpy(pg).cuda()


_arr = lambda xs: (ctypes.c_void_p * 4)(*[x.data_ptr() for x in xs])


@pytest.mark.parametrize("stamped", [False, True])
@pytest.mark.parametrize("step", [1, 7, 1000])
def test_adam_small_packed_within_the_bounds(dev, step, stamped):
    """adam_small_packed_kernel, plain (the clmgs_adam_small_packed entry and the range (0, -1)) and RANGE ((255, 257)
    and (100, 589)), on 2 * 256 + 77 rows: the four tensors and their moments against step64 on the rows of the range,
    every other row bit for bit; the mirror equals the four tensors with a zero pad column.  g_stamp NULL: every line
    counts, and the lines of the range come back cleared while those of every row outside it are bit-identical (the
    ranged kernel used to clear the lines of all rows of the two blocks its borders cut: rows 0..254 and 257..511 for
    the range (255, 257)); g_stamp given with half the rows at cur_step: the other rows take a zero gradient and no
    line is written.
    Largest error / bound measured on an MI355X over steps 1, 7 and 1000: p 0.998 (0.281 on class b, 0.199 on class
    d) m 0.408 v 0.435."""
    from clm_gs_amd import _lib
    L = _lib.lib()
    ps0, ms0, vs0, pg0, cls = _small_inputs()
    cur = 9
    stamp = np.where(np.random.default_rng(8).random(N_SMALL) < 0.5, cur, 3).astype(np.int32)
    lrs = (ctypes.c_double * 4)(*LR4)
    worst = dict(p=0.0, m=0.0, v=0.0)
    for betas in C.BETAS:
        want, co = [], 0
        for ti, w in enumerate(WIDTHS):
            g = pg0[:, co:co + w] * (stamp == cur)[:, None] if stamped else pg0[:, co:co + w]
            args = (g, np.float32(LR4[ti]), betas[0], betas[1], C.EPS, step, True, C.GRAD_SCALE)
            assert all(np.isfinite(x).all() for x in C.emulate_rows(ps0[ti], ms0[ti], vs0[ti], *args))  # before the launch
            want.append(C.one_step(ps0[ti], ms0[ti], vs0[ti], *args))
            co += w
        for entry, lo, hi in (("plain", 0, -1), ("range", 0, -1), ("range", 255, 257), ("range", 100, N_SMALL)):
            ps, ms, vs, pk, pg = _small_device()
            st = torch.from_numpy(stamp).cuda() if stamped else None
            tail = (lrs, _lib.dptr(pk), _lib.dptr(pg), betas[0], betas[1], C.EPS, step, 1, C.GRAD_SCALE,
                    _lib.dptr(st, torch.int32, True), cur)
            if entry == "plain":
                _lib.check(L.clmgs_adam_small_packed(_lib.stream(), N_SMALL, _arr(ps), _arr(ms), _arr(vs), *tail))
                name = "plain entry"
            else:
                _lib.check(L.clmgs_adam_small_packed_range(_lib.stream(), N_SMALL, lo, hi, _arr(ps), _arr(ms), _arr(vs),
                                                           *tail))
                name = f"range ({lo}, {hi})"
            inside = np.zeros(N_SMALL, dtype=bool)
            inside[lo:(N_SMALL if hi < 0 else hi)] = True
            for ti in range(4):
                got = [x[ti].cpu().numpy() for x in (ps, ms, vs)]
                w_ = C.report(f"small_packed step {step} stamped {int(stamped)} betas {betas[0]:.4f} {name} tensor {ti}",
                              cls, ps0[ti], got, want[ti], rows=np.nonzero(inside)[0])
                worst = {q: max(worst[q], w_[q]) for q in worst}
                for x, x0 in zip(got, (ps0[ti], ms0[ti], vs0[ti])):
                    assert _same_bits(x, x0, ~inside), "rows outside the range"
            mirror = torch.cat(ps + [torch.zeros(N_SMALL, 1, device="cuda")], dim=1)
            assert _same_bits(pk, mirror), "the mirror"
            if stamped:
                assert _same_bits(pg, pg0)
            else:
                assert not pg.cpu().numpy()[inside].any()
                assert _same_bits(pg, pg0, ~inside), "gradient lines of the rows outside the range"
    print(f"small_packed step {step} stamped {int(stamped)}: largest error / bound  p {worst['p']:.3f} "
          f"m {worst['m']:.3f} v {worst['v']:.3f}")


@pytest.mark.parametrize("betas", C.BETAS)
def test_adam_small_deferred_within_the_bounds(dev, betas):
    """adam_small_deferred_kernel with flush_all = 1 (no cameras) on 2 * 256 + 77 rows: block 0 current, block 1 five
    steps behind, block 2 kmax steps behind; every step of history with its own learning rates and its own Adam step
    count; stamps spread over 0 .. to_step + 1; against small_deferred64.  The current block is bit-identical, blk_last is
    to_step everywhere afterwards, the device error word stays 0, the mirror equals the tensors, and the _sel entry with
    both optional arguments NULL gives the bits of the plain entry (it launches the same <false> form: the <SEL> form
    needs cameras, and tests/test_gpu_head_overlap.py holds it to the plain form bit for bit).
    Largest error / bound measured on an MI355X: p 0.884 (0.158 on class b, 0.115 on class d) m 0.304 v 0.276."""
    from clm_gs_amd import _lib
    L = _lib.lib()
    kmax = int(L.clmgs_small_deferred_kmax())
    to_step = kmax + 4
    ps0, ms0, vs0, pg0, cls = _small_inputs()
    stamp = np.random.default_rng(9).integers(0, to_step + 2, N_SMALL).astype(np.int32)
    blk_last0 = np.array([to_step, to_step - 5, to_step - kmax], dtype=np.int32)
    lr_hist = np.array([[float(np.float32(x * (1.0 + 0.01 * j))) for x in LR4] for j in range(kmax)])
    sidx = np.array([to_step + 3 - j for j in range(kmax)], dtype=np.int32)
    want = R.small_deferred64(ps0, ms0, vs0, pg0, stamp, blk_last0, to_step, lr_hist, sidx, betas[0], betas[1], C.EPS,
                              C.GRAD_SCALE)
    row_last, co = np.repeat(blk_last0, 256)[:N_SMALL], 0
    for ti, w in enumerate(WIDTHS):  # the same replay in float32 on the CPU first: finite
        emu = C.emulate_replay(ps0[ti], ms0[ti], vs0[ti], pg0[:, co:co + w], row_last, stamp, to_step, None, betas[0],
                               betas[1], C.EPS, True, C.GRAD_SCALE, kmax,
                               lr_of_step=lambda s: np.float32(lr_hist[to_step - s, ti]),
                               step_count=lambda s: int(sidx[to_step - s]))
        assert all(np.isfinite(x).all() for x in emu), "non-finite on the CPU: not launched"
        co += w
    pm = (ctypes.c_float * (kmax + 1))(*[1e-12 + 0.002 * k for k in range(kmax + 1)])
    sg = (ctypes.c_float * (kmax + 1))(*[1.001 + 0.01 * k for k in range(kmax + 1)])
    bits = ctypes.c_uint32(0)
    _lib.check(L.clmgs_device_errors(ctypes.byref(bits), 1))
    results = []
    for entry in ("plain", "sel"):
        ps, ms, vs, pk, pg = _small_device()
        blk = torch.from_numpy(blk_last0.copy()).cuda()
        args = (_lib.stream(), N_SMALL, _arr(ps), _arr(ms), _arr(vs), _lib.dptr(pk), _lib.dptr(pg),
                _lib.dptr(torch.from_numpy(stamp).cuda(), torch.int32), _lib.dptr(blk, torch.int32), to_step, kmax,
                (ctypes.c_double * (4 * kmax))(*lr_hist.flatten()), (ctypes.c_int32 * kmax)(*sidx.tolist()), pm, sg,
                betas[0], betas[1], C.EPS, C.GRAD_SCALE, 0, None, None, 160, 128, 0.3, 0.01, 1e10, 1, None)
        if entry == "plain":
            _lib.check(L.clmgs_adam_small_deferred(*args))
        else:
            _lib.check(L.clmgs_adam_small_deferred_sel(*args, None, None, 0, 0))
        _lib.check(L.clmgs_device_errors(ctypes.byref(bits), 1))
        assert bits.value == 0
        assert blk.cpu().tolist() == [to_step] * 3
        assert _same_bits(pg, pg0)
        assert _same_bits(pk, torch.cat(ps + [torch.zeros(N_SMALL, 1, device="cuda")], dim=1)), "the mirror"
        results.append([x.cpu().numpy() for t in (ps, ms, vs) for x in t])
    assert all(_same_bits(a, b) for a, b in zip(*results)), "the _sel entry without its optional arguments"
    worst = dict(p=0.0, m=0.0, v=0.0)
    current = np.arange(N_SMALL) < 256
    for ti in range(4):
        got = [results[0][k * 4 + ti] for k in range(3)]
        w = C.report(f"small_deferred betas {betas[0]:.4f} tensor {ti}", cls, ps0[ti], got, want[ti])
        worst = {q: max(worst[q], w[q]) for q in worst}
        for x, x0 in zip(got, (ps0[ti], ms0[ti], vs0[ti])):
            assert _same_bits(x, x0, current), "the block that is current"
        assert not _same_bits(got[0], ps0[ti], ~current)
    print(f"small_deferred betas {betas[0]:.4f}: largest error / bound  p {worst['p']:.3f} m {worst['m']:.3f} "
          f"v {worst['v']:.3f}")
