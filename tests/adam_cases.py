"""What tests/test_adam_cpu.py and tests/test_gpu_adam.py share: the input classes, a float32 numpy emulation of
adam_elem (clm_ops.hip) with correctly rounded sqrt and divide, and the element-by-element comparison with
tests/adam_reference.py.  Plain numpy; imports nothing from the package."""
import numpy as np

from tests import adam_reference as R

F32 = np.float32
CLASSES = "abcdefg"
EPS = 1e-15
BETAS = ((0.9, 0.999), (0.9 ** 4, 0.999 ** 4))
GRAD_SCALE = 0.25


def col_lr(cols):
    """2.5e-3 for 3 columns, 1.25e-4 for the rest (float32)."""
    return np.concatenate([np.full(3, 2.5e-3), np.full(max(cols - 3, 0), 1.25e-4)])[:cols].astype(F32)


def input_classes(n, cols, seed):
    """-> p, m, v, g float32 [n, cols] and cls [n] (index into CLASSES): row r is of class r % 7, so that every class
    lies in every block of 256 rows and on both sides of every range border.
      a  p ~ N(0,1), m ~ 1e-3 N(0,1), v in [1, 2] 1e-6, g ~ 4e-3 N(0,1)  (moments as Adam leaves them: |m| / sqrt(v) ~ 1)
      b  as a with p = 0 (even columns) and |p| in [1, 2] 1e-6 (odd): the step is resolved to float precision
      c  m = v = g = 0
      d  v = 0, m = +-1e-20, g = 0, p = 0  (the step is m / eps)
      e  as a with m = -0.0 in even columns and v = -0.0 in odd ones
      f  v log-uniform in [1e-44, 1e-38], m = +-sqrt(v), g = 0, p = 0 (even columns) or N(0,1)
      g  as a with |g| = 1e-12 (even columns) and 1e+12 (odd), p = 0 in the first half of the columns"""
    rng = np.random.default_rng(seed)
    cls = (np.arange(n) % 7).astype(np.int64)
    sign = lambda: np.where(rng.random((n, cols)) < 0.5, -1.0, 1.0)
    p = rng.standard_normal((n, cols))
    m = rng.standard_normal((n, cols)) * 1e-3
    v = (rng.random((n, cols)) + 1.0) * 1e-6
    g = rng.standard_normal((n, cols)) * 4e-3
    even = (np.arange(cols) % 2 == 0)[None, :]
    is_ = lambda c: (cls == CLASSES.index(c))[:, None]
    p = np.where(is_("b"), np.where(even, 0.0, sign() * (rng.random((n, cols)) + 1.0) * 1e-6), p)
    for t in (m, v, g):
        t[cls == CLASSES.index("c")] = 0.0
    m = np.where(is_("d"), sign() * 1e-20, m)
    v = np.where(is_("d"), 0.0, v)
    p = np.where(is_("d"), 0.0, p)
    m = np.where(is_("e") & even, -0.0, m)
    v = np.where(is_("e") & ~even, -0.0, v)
    vf = 10.0 ** (-44.0 + 6.0 * rng.random((n, cols)))
    v = np.where(is_("f"), vf, v)
    m = np.where(is_("f"), sign() * np.sqrt(vf), m)
    p = np.where(is_("f") & even, 0.0, p)
    g = np.where(is_("d") | is_("f"), 0.0, g)
    g = np.where(is_("g"), sign() * np.where(even, 1e-12, 1e12), g)
    p = np.where(is_("g") & (np.arange(cols) < (cols + 1) // 2)[None, :], 0.0, p)
    return p.astype(F32), m.astype(F32), v.astype(F32), g.astype(F32), cls


# ------------------------------------------------------------------------------- float32 emulation of adam_elem
def fma32(a, b, c):
    """float32 fused multiply-add: the product of two float32 is exact in float64 (48 bits); the sum is rounded to 53
    bits and then to 24 (a double rounding that moves the result by 2^-29 ulp at the most)."""
    return (np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(F32)


def emulate_rows(p, m, v, g, lr, beta1, beta2, eps, step, bias_correction, grad_scale, lr_mul=1.0, bc2_plain=False,
                 grad_fused=False):
    """clmgs_adam_rows in float32 numpy: the host's scalars as adam_bias_host makes them, then adam_elem on every
    element with IEEE sqrt and divide in place of the hardware instructions.  lr_mul and bc2_plain are the two
    deliberately wrong forms (every learning rate scaled; bc2 where sqrt(bc2) belongs).  -> p', m', v' (float32)."""
    inv_bc1 = inv_sqrt_bc2 = F32(1.0)
    if bias_correction:
        inv_bc1 = F32(1.0 / (1.0 - beta1 ** step))
        bc2 = 1.0 - beta2 ** step
        inv_sqrt_bc2 = F32(1.0 / (bc2 if bc2_plain else np.sqrt(bc2)))
    b1, b2, e = F32(beta1), F32(beta2), F32(eps)
    ob1, ob2 = F32(1.0 - beta1), F32(1.0 - beta2)
    lr_bc = (np.asarray(lr, F32) * F32(lr_mul)) * inv_bc1 if lr_mul != 1.0 else np.asarray(lr, F32) * inv_bc1
    with np.errstate(all="ignore"):
        gs = np.zeros_like(m) if g is None else g * F32(grad_scale)
        if grad_fused:
            m2 = fma32(ob1, gs, b1 * m)
            v2 = fma32(ob2 * gs, gs, b2 * v)
        else:
            m2 = fma32(b1, m, ob1 * gs)
            v2 = fma32(b2, v, (ob2 * gs) * gs)
        ratio = m2 * (F32(1.0) / fma32(np.sqrt(v2), inv_sqrt_bc2, e))
        p2 = fma32(-lr_bc, ratio, p)
    return p2, m2, v2


def emulate_replay(p, m, v, g, last, g_step, to_step, lr, beta1, beta2, eps, bias_correction, grad_scale, max_replay,
                   lr_of_step=None, step_count=None):
    """A replay in float32 numpy, emulate_rows step by step: row r takes steps last[r] + 1 .. to_step, its gradient line
    (g None / g_step None: none) at g_step[r] when that lies among them and zero gradients otherwise; past max_replay
    steps of a run of zero-gradient steps p stands still and the moments go on decaying (step by step here, in one
    product in the kernels).  lr_of_step(s) / step_count(s): the learning rates and the Adam step count of step s
    (default lr and s: the catch-up kernels; the deferred small-attribute kernel has its own per step).  What the
    tests launch on the device is run through this first and must be finite.  -> p', m', v' (float32)."""
    p, m, v = (np.array(x, F32) for x in (p, m, v))
    last = np.asarray(last, np.int64)
    gst = np.zeros_like(last) if g is None or g_step is None else np.asarray(g_step, np.int64)
    due = (gst > last) & (gst <= to_step)
    run_from = last.copy()
    for s in range(int(last.min()) + 1, int(to_step) + 1):
        active = last < s
        wait = active & due & (gst == s)
        gs = None if g is None else np.where(wait[:, None], g, F32(0.0)).astype(F32)
        p2, m2, v2 = emulate_rows(p, m, v, gs, lr if lr_of_step is None else lr_of_step(s), beta1, beta2, eps,
                                  s if step_count is None else step_count(s), bias_correction, grad_scale)
        moves = active & (wait | (s - run_from <= max_replay))
        p = np.where(moves[:, None], p2, p)
        m, v = np.where(active[:, None], m2, m), np.where(active[:, None], v2, v)
        run_from = np.where(wait, s, run_from)
    return p, m, v


# ------------------------------------------------------------------------------------------------ the comparison
def ratios(p_old, got, want):
    """got = (p', m', v') float32 of an implementation; want = (dp, m', v', b_p, b_m, b_v) of the reference, b_p
    INCLUDING the rounding of p.  -> error / bound per element for p, m, v."""
    out = []
    dp_got = np.asarray(got[0], np.float64) - np.asarray(p_old, np.float64)
    for x, ref, b in ((dp_got, want[0], want[3]), (got[1], want[1], want[4]), (got[2], want[2], want[5])):
        err = np.abs(np.asarray(x, np.float64) - ref)
        with np.errstate(divide="ignore", invalid="ignore"):  # a bound of 0 (an element no step touches) allows 0
            r = np.where(b > 0, err / b, np.where(err == 0, 0.0, np.inf))
        assert not np.isnan(r).any()
        out.append(r)
    return out


def one_step(p, m, v, g, lr, beta1, beta2, eps, step, bias_correction, grad_scale):
    """step64 with the rounding of p added to b_dp: the `want` of ratios() for one step."""
    dp, m2, v2, b_dp, b_m, b_v = R.step64(p, m, v, g, lr, beta1, beta2, eps, step, bias_correction, grad_scale)
    p64 = np.asarray(p, np.float64)
    return dp, m2, v2, b_dp + R.round_p(p64, p64 + dp, b_dp), b_m, b_v


def report(name, cls, p_old, got, want, rows=None):
    """Prints the largest error / bound per quantity and input class, names the worst element, and asserts that every
    output is finite and every element within its bound.  rows: the rows compared (default all).  -> {quantity: worst}."""
    sel = np.arange(len(cls)) if rows is None else np.asarray(rows)
    got = [np.asarray(x)[sel] for x in got]
    want = [np.asarray(x)[sel] for x in want]
    p_old, cls = np.asarray(p_old)[sel], np.asarray(cls)[sel]
    for x in got:
        assert np.isfinite(x).all(), f"{name}: non-finite output"
    rs = ratios(p_old, got, want)
    worst, lines = {}, []
    for q, r in zip("pmv", rs):
        worst[q] = float(r.max()) if r.size else 0.0
        per = " ".join(f"{c}={float(r[cls == i].max()) if (cls == i).any() else 0.0:.3f}" for i, c in enumerate(CLASSES))
        lines.append(f"{q}: {worst[q]:.3f} ({per})")
    print(f"{name}: largest error / bound  " + "  ".join(lines))
    for qi, (q, r) in enumerate(zip("pmv", rs)):
        if worst[q] > 1.0:
            i, k = np.unravel_index(int(np.argmax(r)), r.shape)
            gq = (np.asarray(got[0], np.float64) - p_old)[i, k] if q == "p" else got[qi][i, k]
            raise AssertionError(
                f"{name}: {q} of row {sel[i]} (class {CLASSES[cls[i]]}) column {k}: p {p_old[i, k]!r} got {gq!r} "
                f"want {want[qi][i, k]!r} error / bound {worst[q]:.3f}")
    return worst
