"""No GPU: tests/adam_reference.py is pinned on torch.optim.Adam in float64, its error budget on a float32 emulation of
adam_elem (which must stay inside it, and leave it when the step is made slightly wrong), and the two host routines of
the library (clmgs_host_adam_rows, clmgs_host_rows_prepare) are held to it element by element."""
import ctypes

import numpy as np
import pytest
import torch

from tests import adam_cases as C
from tests import adam_reference as R

STEPS = (1, 2, 7, 1000, 30000)


# ------------------------------------------------------------------------------- 1. the reference against torch
def _torch_adam(p, m, v, betas, eps):
    pt = torch.nn.Parameter(torch.from_numpy(p.copy()))
    opt = torch.optim.Adam([pt], lr=1.0, betas=betas, eps=eps, foreach=False)
    opt.state[pt] = dict(step=torch.tensor(0.0), exp_avg=torch.from_numpy(m.copy()), exp_avg_sq=torch.from_numpy(v.copy()))
    return pt, opt


def _rel(a, b):
    return float(np.max(np.abs(a - b) / np.maximum(np.abs(b), 1e-300)))


def test_step64_and_replay64_equal_torch_adam():
    """20 steps of torch.optim.Adam (float64, foreach=False, betas (0.9^4, 0.999^4), eps 5e-16) with a learning rate
    that changes every step: step64 with random gradients, and replay64 with all-zero gradients (in runs of 3, 1, 7 and
    9 steps, the learning rate changing between the runs), agree to 1e-13 relative in p - p0 (p0 = 0: nothing hides the
    step), m and v."""
    rng = np.random.default_rng(0)
    n, cols, betas, eps = 50, 6, (0.9 ** 4, 0.999 ** 4), 5e-16
    p0 = np.zeros((n, cols))
    m0, v0 = rng.standard_normal((n, cols)) * 1e-3, (rng.random((n, cols)) + 0.1) * 1e-6
    lrs = [1e-3 * (1.0 + 0.37 * k) / (1.0 + 0.05 * k * k) for k in range(20)]
    # with gradients
    pt, opt = _torch_adam(p0, m0, v0, betas, eps)
    p, m, v = p0.copy(), m0.copy(), v0.copy()
    for s in range(1, 21):
        g = rng.standard_normal((n, cols)) * 4e-3
        opt.param_groups[0]["lr"] = lrs[s - 1]
        pt.grad = torch.from_numpy(g * 0.25)
        opt.step()
        dp, m, v, *_ = R.step64(p, m, v, g, lrs[s - 1], betas[0], betas[1], eps, s, True, 0.25)
        p = p + dp
    st = opt.state[pt]
    figures = (_rel(p, pt.detach().numpy()), _rel(m, st["exp_avg"].numpy()), _rel(v, st["exp_avg_sq"].numpy()))
    print("step64 against torch.optim.Adam, 20 steps: largest relative difference p %.2e m %.2e v %.2e" % figures)
    assert max(figures) < 1e-13
    # zero gradients, replayed in runs
    pt, opt = _torch_adam(p0, m0, v0, betas, eps)
    p, m, v = p0.copy(), m0.copy(), v0.copy()
    for (a, b), lr in zip(((0, 3), (3, 4), (4, 11), (11, 20)), lrs):
        opt.param_groups[0]["lr"] = lr
        for _ in range(a, b):
            pt.grad = torch.zeros(n, cols, dtype=torch.float64)
            opt.step()
        dp, m, v, *_ = R.replay64(p, m, v, None, np.full(n, a), None, b, lr, betas[0], betas[1], eps, True, 1.0, 256)
        p = p + dp
    st = opt.state[pt]
    figures = (_rel(p, pt.detach().numpy()), _rel(m, st["exp_avg"].numpy()), _rel(v, st["exp_avg_sq"].numpy()))
    print("replay64 against torch.optim.Adam, 20 zero-gradient steps: p %.2e m %.2e v %.2e" % figures)
    assert max(figures) < 1e-13


def test_replay64_waiting_gradient_and_max_replay_against_torch_adam():
    """replay64's other two rules, against torch.optim.Adam too: a waiting gradient enters at its own step between
    zero-gradient steps (stamps <= last and > to_step are ignored, rows with to_step <= last untouched), and past
    max_replay steps of a run only the moments move."""
    rng = np.random.default_rng(1)
    n, cols, betas, eps, lr, to_step = 40, 5, (0.9, 0.999), 1e-15, 2e-3, 12
    p0 = np.zeros((n, cols))
    m0, v0 = rng.standard_normal((n, cols)) * 1e-3, (rng.random((n, cols)) + 0.1) * 1e-6
    g = rng.standard_normal((n, cols)) * 4e-3
    last = rng.integers(0, 15, n)
    g_step = rng.integers(0, 16, n)
    dp, m, v, _, _, _, consumed = R.replay64(p0, m0, v0, g, last, g_step, to_step, lr, *betas, eps, True, 0.25, 256)
    dp4, m4, v4, *_ = R.replay64(p0, m0, v0, None, last, None, to_step, lr, *betas, eps, True, 1.0, 4)
    for r in range(n):
        pt, opt = _torch_adam(p0[r:r + 1], m0[r:r + 1], v0[r:r + 1], betas, eps)
        opt.param_groups[0]["lr"] = lr
        opt.state[pt]["step"] = torch.tensor(float(last[r]))
        due = last[r] < g_step[r] <= to_step
        assert bool(consumed[r]) == bool(due)
        for s in range(last[r] + 1, to_step + 1):
            pt.grad = torch.from_numpy(g[r:r + 1] * 0.25 if (due and s == g_step[r]) else np.zeros((1, cols)))
            opt.step()
        st = opt.state[pt]
        if last[r] >= to_step:
            assert np.array_equal(dp[r], np.zeros(cols)) and np.array_equal(m[r], m0[r]) and np.array_equal(v[r], v0[r])
        assert _rel(dp[r:r + 1], pt.detach().numpy()) < 1e-13 or not np.any(dp[r])
        assert _rel(m[r:r + 1], st["exp_avg"].numpy()) < 1e-13 and _rel(v[r:r + 1], st["exp_avg_sq"].numpy()) < 1e-13
        # max_replay = 4, no gradients: the moments are those of every step, p those of the first four
        pt, opt = _torch_adam(p0[r:r + 1], m0[r:r + 1], v0[r:r + 1], betas, eps)
        opt.param_groups[0]["lr"] = lr
        opt.state[pt]["step"] = torch.tensor(float(last[r]))
        p_first4 = np.zeros((1, cols))
        for s in range(last[r] + 1, to_step + 1):
            pt.grad = torch.zeros(1, cols, dtype=torch.float64)
            opt.step()
            if s == last[r] + 4:
                p_first4 = pt.detach().numpy().copy()
        if to_step - last[r] <= 4:
            p_first4 = pt.detach().numpy().copy()
        st = opt.state[pt]
        assert _rel(dp4[r:r + 1], p_first4) < 1e-13 or not np.any(dp4[r])
        assert _rel(m4[r:r + 1], st["exp_avg"].numpy()) < 1e-13 and _rel(v4[r:r + 1], st["exp_avg_sq"].numpy()) < 1e-13


def test_small_deferred64_equals_16_dense_steps():
    """small_deferred64 == 16 dense float64 Adam steps (written out here with torch, not through step64) in which rows
    without a due line get g = 0 and a block joins at the step after its blk_last; every step of history has its own
    learning rates and its own Adam step count."""
    rng = np.random.default_rng(2)
    n, widths, kmax, to_step, b1, b2, eps, scale = 256 * 2 + 77, (3, 1, 3, 4), 16, 20, 0.9, 0.999, 1e-15, 0.25
    ps = [rng.standard_normal((n, w)) for w in widths]
    ms = [rng.standard_normal((n, w)) * 1e-3 for w in widths]
    vs = [(rng.random((n, w)) + 0.1) * 1e-6 for w in widths]
    pg = rng.standard_normal((n, 12)) * 4e-3
    stamp = rng.integers(0, to_step + 2, n)
    blk_last = np.array([to_step, to_step - 5, to_step - kmax])
    lr_hist = np.array([[x * (1.0 + 0.01 * j) for x in (1.6e-4, 5e-2, 5e-3, 1e-3)] for j in range(kmax)])
    sidx = np.array([to_step + 3 - j for j in range(kmax)])
    got = R.small_deferred64(ps, ms, vs, pg, stamp, blk_last, to_step, lr_hist, sidx, b1, b2, eps, scale)
    row_last = torch.from_numpy(np.repeat(blk_last, 256)[:n])
    co = 0
    for ti, w in enumerate(widths):
        p, m, v = (torch.from_numpy(x[ti].copy()) for x in (ps, ms, vs))
        for s in range(to_step - kmax + 1, to_step + 1):
            j = to_step - s
            on = (row_last < s)[:, None].double()
            has = ((torch.from_numpy(stamp) == s) & (row_last < s))[:, None].double()
            g = torch.from_numpy(pg[:, co:co + w]) * scale * has
            m2 = b1 * m + (1 - b1) * g
            v2 = b2 * v + (1 - b2) * g * g
            bc1, bc2 = 1 - b1 ** int(sidx[j]), 1 - b2 ** int(sidx[j])
            p2 = p - (lr_hist[j, ti] / bc1) * m2 / (v2.sqrt() / bc2 ** 0.5 + eps)
            p, m, v = torch.where(on > 0, p2, p), torch.where(on > 0, m2, m), torch.where(on > 0, v2, v)
        co += w
        dp, m_r, v_r = got[ti][:3]
        assert np.array_equal(dp[:256], np.zeros((256, w)))  # the block that is current
        assert _rel(ps[ti] + dp, p.numpy()) < 1e-13 and _rel(m_r, m.numpy()) < 1e-13 and _rel(v_r, v.numpy()) < 1e-13
        assert np.any(dp[256:] != 0)


# ------------------------------------------------------------------------------- 2. the budget against an emulation
def _eager_cases():
    for betas in C.BETAS:
        for step in STEPS:
            for cols in (48, 3):
                for with_g in (True, False):
                    yield betas, step, cols, with_g


def test_float32_emulation_stays_inside_the_budget_and_wrong_steps_leave_it():
    """The float32 numpy emulation of adam_elem (IEEE sqrt and divide) on every input class, both betas, steps 1, 2, 7,
    1000 and 30000, with and without gradients, with and without bias correction, both roundings of the moments:
    finite everywhere, every element within the bounds of step64.  Measured, largest error / bound over all of it:
    p 1.000 (the rounding of p itself where |p| ~ 1), m 0.605, v 0.435 (the correct step).  The same emulation with every
    learning rate scaled by 1 + 1e-5 leaves the bound of p on class b (measured 9.7 to 11.1 over the settings) and so
    does bc2 in place of sqrt(bc2) (measured 8.8e3 to 9.4e5 at steps 1 to 1000; at step 30000 bc2 is 1 to float precision
    and nothing differs, so that step is left out of this check)."""
    worst = dict(p=0.0, m=0.0, v=0.0)
    worst_lr, worst_bc2 = [], []
    for betas, step, cols, with_g in _eager_cases():
        p, m, v, g, cls = C.input_classes(700, cols, seed=step + cols)
        lr = C.col_lr(cols)
        for bias in (True, False):
            args = (lr, betas[0], betas[1], C.EPS, step, bias, C.GRAD_SCALE)
            want = C.one_step(p, m, v, g if with_g else None, *args)
            for fused in (False, True):
                got = C.emulate_rows(p, m, v, g if with_g else None, *args, grad_fused=fused)
                assert all(np.isfinite(x).all() for x in got)
                rs = C.ratios(p, got, want)
                for q, r in zip("pmv", rs):
                    worst[q] = max(worst[q], float(r.max()))
                    assert r.max() <= 1.0, (q, betas, step, cols, with_g, bias, fused, float(r.max()))
            is_b = cls == C.CLASSES.index("b")
            bad = C.emulate_rows(p, m, v, g if with_g else None, *args, lr_mul=1.0 + 1e-5)
            worst_lr.append(float(C.ratios(p, bad, want)[0][is_b].max()))
            if bias and step <= 1000:
                bad = C.emulate_rows(p, m, v, g if with_g else None, *args, bc2_plain=True)
                worst_bc2.append(float(C.ratios(p, bad, want)[0][is_b].max()))
    print("emulation: largest error / bound  p %.3f m %.3f v %.3f" % (worst["p"], worst["m"], worst["v"]))
    print("learning rate x (1 + 1e-5), class b: error / bound between %.1f and %.1f" % (min(worst_lr), max(worst_lr)))
    print("bc2 for sqrt(bc2), class b: error / bound between %.3g and %.3g" % (min(worst_bc2), max(worst_bc2)))
    assert min(worst_lr) > 1.0 and min(worst_bc2) > 1.0


# ------------------------------------------------------------------------------- 3. the host routines
P = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None


@pytest.mark.parametrize("betas", C.BETAS)
@pytest.mark.parametrize("step", [1, 3, 1000])
def test_host_adam_rows_within_the_bounds(betas, step):
    """clmgs_host_adam_rows on the shape of test_abi.py::test_tsp_and_host_adam_run_on_cpu (5000 x 48, 2500 listed
    rows, two threads, behind a signal) and the input classes: every listed element within the bounds of step64, the
    gradient lines of the listed rows cleared, every other row bit for bit.  Largest error / bound measured: p 1.000
    (class a: the rounding of p; 0.396 on class b, 0.135 on class d), m 0.473, v 0.421."""
    from clm_gs_amd import _lib
    N, cols = 5000, 48
    p0, m0, v0, g0, cls = C.input_classes(N, cols, seed=11)
    rows = torch.randperm(N, generator=torch.Generator().manual_seed(0))[:2500].to(torch.int32).contiguous()
    lr = C.col_lr(cols)
    p, m, v, g = (torch.from_numpy(x.copy()) for x in (p0, m0, v0, g0))
    sig = torch.ones(1, dtype=torch.int32)
    _lib.check(_lib.lib().clmgs_host_adam_rows(P(p), P(g), P(m), P(v), P(rows), rows.numel(), cols,
                                               P(torch.from_numpy(lr)), betas[0], betas[1], C.EPS, step, 1,
                                               C.GRAD_SCALE, 1, P(sig), 2))
    want = C.one_step(p0, m0, v0, g0, lr, betas[0], betas[1], C.EPS, step, True, C.GRAD_SCALE)
    listed = np.zeros(N, dtype=bool)
    listed[rows.numpy()] = True
    C.report(f"host_adam_rows step {step} betas {betas[0]:.4f}", cls, p0, (p.numpy(), m.numpy(), v.numpy()), want,
             rows=np.nonzero(listed)[0])
    for x, x0 in ((p, p0), (m, m0), (v, v0), (g, g0)):
        assert np.array_equal(x.numpy()[~listed].view(np.uint32), x0[~listed].view(np.uint32))
    assert not g.numpy()[listed].any()


@pytest.mark.parametrize("betas", C.BETAS)
@pytest.mark.parametrize("sparse", [0, 1])
@pytest.mark.parametrize("to_step,max_replay,last_hi", [(7, 256, 4), (30, 4, 12), (1014, 256, 1011)])
def test_host_rows_prepare_within_the_bounds(sparse, to_step, max_replay, last_hi, betas):
    """clmgs_host_rows_prepare, dense and sparse, on the shape of test_abi.py's deferred test (6000 x 48, staleness 0 to
    3 of 7 steps, half the rows with a gradient waiting) and two more (the max_replay cut; step counts in the
    thousands), on the input classes: every element within the bounds of replay64 (bias corrections computed in double,
    rounded once), stamps advanced, the staged copy is the row.  Both betas.  Largest error / bound
    measured, dense: p 0.922 (0.555 on class b) m 0.348 v 0.219; sparse: p 1.000 (0.579 on class b) m 0.510 v 0.443."""
    from clm_gs_amd import _lib
    L = _lib.lib()
    N, cols = 6000, 48
    b1, b2 = betas
    p0, m0, v0, g0, cls = C.input_classes(N, cols, seed=12)
    rng = np.random.default_rng(3)
    last0 = rng.integers(max(0, last_hi - 24) if to_step > 100 else 0, last_hi, N).astype(np.int32)
    gstep0 = np.where(rng.random(N) < 0.5, last0 + 1 + rng.integers(0, 2, N), 0).astype(np.int32)
    gstep0[rng.random(N) < 0.05] = to_step + 1  # not due yet
    lr = C.col_lr(cols)
    p, m, v, g, last, gstep = (torch.from_numpy(x.copy()) for x in (p0, m0, v0, g0, last0, gstep0))
    rows = torch.randperm(N, generator=torch.Generator().manual_seed(1)).to(torch.int32).contiguous()
    stage = torch.empty(N, cols)
    assert L.clmgs_host_pool_start(3) == 3
    _lib.check(L.clmgs_host_rows_prepare(P(p), P(g), P(m), P(v), P(last), P(gstep), P(rows), N, cols,
                                         P(torch.from_numpy(lr)), b1, b2, C.EPS, to_step, to_step + 1, 1, C.GRAD_SCALE,
                                         max_replay, P(stage), sparse))
    ref = R.replay64(p0, m0, v0, g0, last0, gstep0, to_step, lr, b1, b2, C.EPS, True, C.GRAD_SCALE, max_replay,
                     lazy=False, sparse=bool(sparse))
    C.report(f"host_rows_prepare betas {b1:.4f} sparse={sparse} to_step {to_step} max_replay {max_replay}", cls, p0,
             (p.numpy(), m.numpy(), v.numpy()), ref[:6])
    assert torch.equal(stage, p[rows.long()])
    assert int(last.min()) == to_step == int(last.max()) and int(gstep.min()) == to_step + 1 == int(gstep.max())
    assert np.array_equal(g.numpy().view(np.uint32), g0.view(np.uint32))  # (const in the ABI)
    is_c = cls == C.CLASSES.index("c")
    assert np.array_equal(p.numpy()[is_c], p0[is_c]) and not m.numpy()[is_c].any() and not v.numpy()[is_c].any()
