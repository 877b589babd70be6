"""Float64 restatement of the Adam step every kernel and host routine of this project applies, with a per-element
bound on what a float32 implementation of it may differ by.  Plain numpy; imports nothing from the package.

Convention (DeepSpeed's FusedAdam and torch.optim.Adam): with gs = g * grad_scale,
    m' = beta1 m + (1 - beta1) gs          v' = beta2 v + (1 - beta2) gs^2
    bc1 = 1 - beta1^step, bc2 = 1 - beta2^step   (both 1 without bias correction)
    dp = -(lr / bc1) * m' / (sqrt(v') / sqrt(bc2) + eps)
The inputs are the float32 values the kernel receives, widened to float64; beta1, beta2 and eps are the doubles the C
ABI takes (the implementations round them to float: counted below).

THE BUDGET.  u = 2^-24 is the relative error of one float32 rounding; "1 ulp" of a hardware instruction is at most
2u relative.  One line per operation of adam_elem / adam_update (clm_ops.hip); every count is first order.

  m' = fma(beta1, m, ob1 * gs)                          term beta1 m     term (1-beta1) gs
    beta1 -> float                                            u
    ob1 = float(1 - beta1)                                                      u
    gs = g * grad_scale                                                         u
    ob1 * gs                                                                    u
    the fma's one rounding                                    u                 u
                                                             2u                4u     b_m = 4u (|beta1 m| + |(1-beta1) gs|)
  v' = fma(beta2, v, (ob2 * gs) * gs)                   term beta2 v     term (1-beta2) gs^2
    beta2 -> float                                            u
    ob2 = float(1 - beta2)                                                      u
    gs, twice                                                                  2u
    ob2 * gs, then * gs                                                        2u
    the fma's one rounding                                    u                 u
                                                             2u                6u     b_v = 6u (beta2 v + (1-beta2) gs^2)
  (the other rounding of the moments -- the catch-up kernels' waiting step rounds the decay and fuses the gradient
  term -- moves one rounding from the right column to the left: 3u / 3u and 3u / 5u, inside the same bounds.  The
  host routines write the same expressions with plain operators: the same counts with or without contraction.)
  Results below FLT_MIN are rounded to a multiple of 2^-149, not to 24 bits: every counted rounding also adds 2^-150
  (not where every term is exactly 0: products and sums of zeros are exact, so b_v = 0 where v' = 0).
  Errors already in m and v (b_m_in, b_v_in: earlier steps of a replay) come through multiplied by beta1 and beta2.

  dp = -lr_bc * ratio,  ratio = m' * rcp(fma(sqrt(v'), inv_sqrt_bc2, eps)),  lr_bc = lr * inv_bc1
    inv_bc1 -> float (computed in double on the host)         u      = rel_ibc1 (larger for the lazy kernels, below)
    lr * inv_bc1                                              u
    inv_sqrt_bc2 -> float                                     u      = rel_isbc2 (larger for the lazy kernels, below)
    hardware sqrt, 1 ulp                                     2u
    eps -> float                                              u
    the fma's one rounding                                    u
    hardware rcp, 1 ulp                                      2u
    m' * rcp                                                  u
                                                            10u      = 8u + rel_ibc1 + rel_isbc2
    p' = fma(-lr_bc, ratio, p): the product is exact inside the fma and p' is rounded once: half an ulp of p', which
    the comparison adds on its own (round_p).
  The host routines (libm sqrtf and IEEE division, correctly rounded: u each instead of 2u; one more rounding for the
  product sqrtf * inv_sqrt_bc2 and one for step_lr * quotient when they are not contracted) come to 10u as well.
  The error of m' reaches dp through the factor (lr / bc1) / denom; the error of v' through sqrt: |d sqrt(v')| <=
  b_v / (2 sqrt(v')), and never more than sqrt(b_v) (|sqrt a - sqrt b| <= sqrt |a - b|), divided by sqrt(bc2), relative
  to denom.  Where v' is below FLT_MIN the hardware sqrt may take its input for anything in [0, FLT_MIN]: sqrt(FLT_MIN)
  more on sqrt(v') there (v' = 0 exactly is not such an input).
    b_dp = |dp| (8u + rel_ibc1 + rel_isbc2 + d_sqrt / (sqrt(bc2) denom)) + (lr / bc1) / denom * b_m

THE LAZY KERNELS (clmgs_adam_catch_up) make their bias corrections on the device (pow_beta, adam_bias, adam_replay):
  pw = exp2(x0 * log2(beta)) at the first step x0 of a replay run, then j products pw *= beta.  Relative error of pw
  at step s = x0 + j against beta^s with the double beta:
    beta -> float, s factors                                s u
    hardware log2, 1 ulp, and the product x0 * log2(beta): 3u relative on the exponent x0 log2(beta), which is an
      absolute error of the exponent; through exp2          3u x0 |ln beta|
    hardware exp2, 1 ulp                                    2u
    j roundings of the running product                      j u
    (a result below FLT_MIN may be flushed: FLT_MIN absolute)
  1 / bc1 = 1 / (1 - pw): d(1/bc) = d pw / (1 - pw)^2, relative to 1/bc: d pw / (1 - pw); the IEEE subtraction and
  division round once each: rel_ibc1 = d pw / (1 - pw) + 2u.  1 / sqrt(bc2): half of that through the square root,
  half of the subtraction's rounding, the IEEE sqrt and division: rel_isbc2 = d pw / (2 (1 - pw)) + 2.5u.
  Steps past max_replay of a run only decay the moments, by f = pow_beta(beta, d) in one product: the error of f as
  above with s = x0 = d, j = 0, and one rounding for the product (host: powf, inside the same figure).

Nothing here is fitted to what an implementation returns.
"""
import math

import numpy as np

U = 2.0 ** -24
FLT_MIN = 2.0 ** -126
HALF_DENORM = 2.0 ** -150  # half of the smallest float32 step


def _f64(x):
    return np.asarray(x, dtype=np.float64)


def ulp32(x):
    """Spacing of float32 at |x| (float64 in, float64 out): 2^(e-23) for 2^e <= |x| < 2^(e+1), 2^-149 below FLT_MIN."""
    a = np.abs(_f64(x))
    _, e = np.frexp(a)  # a = f 2^e, 0.5 <= f < 1
    return np.ldexp(1.0, np.maximum(e, -125) - 24)


def _bias(beta1, beta2, step, bias_correction):
    step = _f64(step)
    if not bias_correction:
        one = np.ones_like(step)
        return one, one
    return 1.0 - np.power(float(beta1), step), 1.0 - np.power(float(beta2), step)


def step64(p, m, v, g, lr, beta1, beta2, eps, step, bias_correction, grad_scale, *, b_m_in=0.0, b_v_in=0.0,
           rel_ibc1=None, rel_isbc2=None):
    """One Adam step.  -> dp, m', v', b_dp, b_m, b_v (float64; b_dp does NOT contain the rounding of p', see round_p).
    g None = zero gradient; lr and step broadcast against the tables (step per row: shape [n, 1]).  rel_ibc1 /
    rel_isbc2: relative error of the implementation's 1/bc1 and 1/sqrt(bc2) (default: one rounding to float, none
    without bias correction)."""
    p, m, v, lr = _f64(p), _f64(m), _f64(v), _f64(lr)
    gs = np.zeros_like(m) if g is None else _f64(g) * float(grad_scale)
    b1, b2, eps = float(beta1), float(beta2), float(eps)
    bc1, bc2 = _bias(b1, b2, step, bias_correction)
    if rel_ibc1 is None:
        rel_ibc1 = U if bias_correction else 0.0
    if rel_isbc2 is None:
        rel_isbc2 = U if bias_correction else 0.0
    m2 = b1 * m + (1.0 - b1) * gs
    v2 = b2 * np.abs(v) + (1.0 - b2) * gs * gs  # (|v|: a second moment of -0 is 0)
    mag_m = np.abs(b1 * m) + np.abs((1.0 - b1) * gs)
    b_m = b1 * _f64(b_m_in) + 4 * U * mag_m + np.where(mag_m > 0, 4 * HALF_DENORM, 0.0)  # (all terms 0: exact)
    b_v = b2 * _f64(b_v_in) + 6 * U * v2 + np.where(v2 > 0, 6 * HALF_DENORM, 0.0)
    sq = np.sqrt(v2)
    denom = sq / np.sqrt(bc2) + eps
    step_size = lr / bc1
    dp = -step_size * m2 / denom
    with np.errstate(divide="ignore", invalid="ignore"):
        d_sqrt = np.where(v2 > 0, np.minimum(b_v / (2.0 * sq), np.sqrt(b_v)), np.sqrt(b_v))
    d_sqrt = d_sqrt + np.where((v2 > 0) & (v2 - b_v < FLT_MIN), math.sqrt(FLT_MIN), 0.0)
    b_dp = np.abs(dp) * (8 * U + rel_ibc1 + rel_isbc2 + d_sqrt / (np.sqrt(bc2) * denom)) + step_size / denom * b_m
    return dp, m2, v2, b_dp, b_m, b_v


def round_p(p_old, p_new, slack=0.0):
    """What the one rounding of p' = fma(-lr_bc, ratio, p) may cost: half an ulp of the larger of |p_old|, |p_new|
    (slack: what is already uncertain about them, so that the binade is not misjudged at a power of two)."""
    return 0.5 * ulp32(np.maximum(np.abs(_f64(p_old)), np.abs(_f64(p_new))) + slack)


def pow_rel(beta, x0, j):
    """Relative error of the lazy kernels' beta^(x0 + j) (module docstring), FLT_MIN absolute not included."""
    x0, j = _f64(x0), _f64(j)
    return (x0 + j) * U + 3 * U * x0 * abs(math.log(float(beta))) + 2 * U + j * U


def lazy_bias_rel(beta1, beta2, x0, j, bias_correction=True):
    """-> rel_ibc1, rel_isbc2 of the lazy kernels at step x0 + j of a replay run that began at step x0."""
    x0, j = _f64(x0), _f64(j)
    if not bias_correction:
        z = np.zeros(np.broadcast(x0, j).shape)
        return z, z
    out = []
    for beta, half, fixed in ((beta1, 1.0, 2.0 * U), (beta2, 0.5, 2.5 * U)):
        pw = np.power(float(beta), x0 + j)
        d_pw = pw * pow_rel(beta, x0, j) + FLT_MIN
        out.append(half * d_pw / (1.0 - pw) + fixed)
    return out[0], out[1]


def replay64(p, m, v, g, last, g_step, to_step, lr, beta1, beta2, eps, bias_correction, grad_scale, max_replay,
             lazy=True, sparse=False):
    """The documented semantics of clmgs_adam_catch_up (and clmgs_host_rows_prepare) applied step by step to every
    row of the tables: zero-gradient steps last+1 .. g_step-1, the waiting gradient g (None / g_step None: no gradients)
    at g_step when last < g_step <= to_step, zero-gradient steps up to to_step.  Of each run of zero-gradient steps the
    first max_replay are exact; the rest only decay the moments, by beta^d.  Rows with to_step <= last are untouched.
    lazy: bias corrections made on the device (lazy_bias_rel); else computed in double and rounded once (the host).
    sparse: zero-gradient steps do not exist (clmgs_host_rows_prepare with sparse != 0).
    -> dp (the whole displacement), m', v', b_dp (with every step's rounding of p), b_m, b_v, consumed [n] bool."""
    p0, m, v = _f64(p).copy(), _f64(m).copy(), np.abs(_f64(v))
    n = p0.shape[0]
    last = np.asarray(last, dtype=np.int64).reshape(n)
    gst = np.zeros(n, dtype=np.int64) if g_step is None or g is None else np.asarray(g_step, dtype=np.int64).reshape(n)
    to_step, max_replay = int(to_step), int(max_replay)
    pending = (gst > last) & (gst <= to_step)
    pc = p0.copy()
    b_p, b_m, b_v = np.zeros_like(p0), np.zeros_like(p0), np.zeros_like(p0)
    lr = np.broadcast_to(_f64(lr), p0.shape)
    gg = None if g is None else _f64(g)

    def apply(rows, s, grad, x0, j):
        if rows.size == 0:
            return
        if lazy:
            r1, r2 = lazy_bias_rel(beta1, beta2, x0[:, None], j[:, None], bias_correction)
        else:
            r1 = r2 = None
        dp, m2, v2, b_dp, bm, bv = step64(pc[rows], m[rows], v[rows], gg[rows] if grad else None, lr[rows], beta1,
                                          beta2, eps, s, bias_correction, grad_scale if grad else 1.0,
                                          b_m_in=b_m[rows], b_v_in=b_v[rows], rel_ibc1=r1, rel_isbc2=r2)
        new = pc[rows] + dp
        b_p[rows] += b_dp + round_p(pc[rows], new, b_p[rows] + b_dp)
        pc[rows], m[rows], v[rows], b_m[rows], b_v[rows] = new, m2, v2, bm, bv

    def fold(rows, d):  # d [rows] steps of decay only
        if rows.size == 0:
            return
        for t, b, beta in ((m, b_m, beta1), (v, b_v, beta2)):
            f = np.power(float(beta), _f64(d))[:, None]
            d_f = f * pow_rel(beta, d, 0)[:, None] + FLT_MIN
            old = t[rows]
            t[rows] = old * f
            b[rows] = f * b[rows] + np.abs(old) * d_f + np.abs(old * f) * U + np.where(old != 0, HALF_DENORM, 0.0)

    start = int(last.min()) + 1 if n else to_step + 1
    run_from = last.copy()  # the step each row's current run of zero-gradient steps began after
    for s in range(start, to_step + 1):
        active = last < s
        wait = active & pending & (gst == s)
        zero = active & ~wait
        if sparse:
            zero[:] = False
        age = s - run_from  # 1 = first step of the run
        exact = np.nonzero(zero & (age <= max_replay))[0]
        apply(exact, s, False, (run_from[exact] + 1).astype(np.float64), (age[exact] - 1).astype(np.float64))
        # a run ends at its row's g_step - 1 or at to_step: fold what lies past max_replay there, in one product
        ends = zero & (((pending) & (s == gst - 1)) | (s == to_step))
        fo = np.nonzero(ends & (age > max_replay))[0]
        fold(fo, age[fo] - max_replay)
        w = np.nonzero(wait)[0]
        apply(w, s, True, np.full(w.size, float(s)), np.zeros(w.size))
        run_from[w] = s
    return pc - p0, m, v, b_p, b_m, b_v, pending & (last < to_step)


def small_deferred64(params, moms, vars_, packed_g, g_stamp, blk_last, to_step, lr4_hist, step_index, beta1, beta2, eps,
                     grad_scale, block=256):
    """The documented semantics of clmgs_adam_small_deferred with flush_all = 1: the four small-attribute tensors
    (params / moms / vars_: lists of [n, w] with w = 3, 1, 3, 4; packed_g [n, 12] holds their gradient lines in that
    order of columns) are brought, block of 256 rows by block, from blk_last[block] to to_step; step s uses
    lr4_hist[to_step - s] and the bias corrections of Adam step count step_index[to_step - s]; a row's line enters at
    g_stamp[row] when blk_last < g_stamp <= to_step, zero gradients at every other step.
    -> per tensor (dp, m', v', b_dp, b_m, b_v), b_dp with every step's rounding of p."""
    n = _f64(params[0]).shape[0]
    row_last = np.repeat(np.asarray(blk_last, dtype=np.int64), block)[:n]
    gst = np.asarray(g_stamp, dtype=np.int64).reshape(n)
    due = (gst > row_last) & (gst <= int(to_step))
    lr4_hist = _f64(lr4_hist).reshape(-1, 4)
    out, co = [], 0
    for ti, (p, m, v) in enumerate(zip(params, moms, vars_)):
        p0, m, v = _f64(p).copy(), _f64(m).copy(), np.abs(_f64(v))
        w = p0.shape[1]
        gg = _f64(packed_g)[:, co:co + w]
        co += w
        pc, b_p, b_m, b_v = p0.copy(), np.zeros_like(p0), np.zeros_like(p0), np.zeros_like(p0)
        for s in range(int(row_last.min()) + 1, int(to_step) + 1):
            j = int(to_step) - s
            rows = np.nonzero(row_last < s)[0]
            gs = np.where((due & (gst == s))[rows, None], gg[rows], 0.0)
            dp, m2, v2, b_dp, bm, bv = step64(pc[rows], m[rows], v[rows], gs, lr4_hist[j, ti], beta1, beta2, eps,
                                              int(step_index[j]), True, grad_scale, b_m_in=b_m[rows], b_v_in=b_v[rows])
            new = pc[rows] + dp
            b_p[rows] += b_dp + round_p(pc[rows], new, b_p[rows] + b_dp)
            pc[rows], m[rows], v[rows], b_m[rows], b_v[rows] = new, m2, v2, bm, bv
        out.append((pc - p0, m, v, b_p, b_m, b_v))
    return out
