"""-m gpu: MCMC densification ("MCMC") -- the three kernels of csrc/mcmc.hip against the float64
restatement (tests/mcmc_reference.py), relocate_gs / add_new_gs of both models, the engines and the trainer."""
import io
import math

import numpy as np
import pytest
import torch

from tests import mcmc_reference as R
from tests.scenes import rel_l2

pytestmark = pytest.mark.gpu

ROWS = (1, 63, 64, 65, 255, 256, 257, 1000)


def _logit(p):
    return math.log(p / (1.0 - p))


# ====================================================================== kernels
@pytest.mark.parametrize("n", ROWS)
def test_relocation_kernel(dev, n):
    """Relative 1e-6 (double arithmetic rounded once to float32: 2^-24 plus margin) on every element whose alternating
    sum has kappa <= 1e6; at most 10 % of the elements may be excluded by that rule (the CPU suite shows the restatement
    excludes none of these inputs)."""
    from clm_gs_amd import clm_kernels as K
    o, s, ratios = R.relocation_inputs(n)
    ref_o, ref_s, kappa = R.relocation(o.numpy(), s.numpy(), ratios.numpy())
    new_o, new_s = K.mcmc_relocation(o.to(dev), s.to(dev), ratios.to(dev))
    assert new_o.shape == o.shape and new_s.shape == s.shape and new_o.dtype == torch.float32
    ok = kappa <= 1e6
    assert float((~ok).mean()) <= 0.10
    eo = np.abs(new_o.cpu().double().numpy() - ref_o) / np.abs(ref_o)
    es = np.abs(new_s.cpu().double().numpy() - ref_s) / np.abs(ref_s)
    print(f"relocation n={n}: max rel err opacity {eo[ok].max():.3e} scales {es[ok].max():.3e} kappa max {kappa.max():.3e}")
    assert eo[ok].max() <= 1e-6 and es[ok].max() <= 1e-6
    # [n,1] opacities (the models' layout) give the same bits
    o1, s1 = K.mcmc_relocation(o.to(dev)[:, None].contiguous(), s.to(dev), ratios.to(dev))
    assert o1.shape == (n, 1) and torch.equal(o1[:, 0], new_o) and torch.equal(s1, new_s)


def test_relocation_clamps_the_ratio(dev):
    from clm_gs_amd import clm_kernels as K
    o = torch.tensor([0.3, 0.3, 0.3, 0.3], device=dev)
    s = torch.ones(4, 3, device=dev)
    a = K.mcmc_relocation(o, s, torch.tensor([0, 1, 51, 200], dtype=torch.int32, device=dev))
    assert torch.equal(a[0][0], a[0][1]) and torch.equal(a[1][0], a[1][1])   # 0 -> 1
    assert torch.equal(a[0][2], a[0][3]) and torch.equal(a[1][2], a[1][3])   # 200 -> 51
    assert float(a[0][1]) == pytest.approx(0.3, rel=1e-6) and float(a[1][1, 0]) == pytest.approx(1.0, rel=1e-6)


def _reg_inputs(n, dev):
    g = torch.Generator().manual_seed(2000 + n)
    o = torch.randn(n, 1, generator=g) * 2.5
    o[0], o[-1] = 12.0, (-12.0 if n > 1 else 12.0)  # saturated opacities: s (1 - s) must not cancel
    s = torch.randn(n, 3, generator=g) * 1.5 - 1.0
    w_o, w_s = 0.01, 0.02
    c_o, c_s = w_o * 4.0 / n, w_s * 4.0 / (3 * n)  # (a batch scale of 4 folded in, as the engines do)
    # a NON-ZERO gradient of the increments' own magnitude to start from: the test proves the kernel adds, and an error
    # of the increment is not hidden behind a large starting value
    g_o = torch.randn(n, 1, generator=g) * c_o * 0.25
    g_s = torch.randn(n, 3, generator=g) * c_s
    od, sd = o.double().requires_grad_(), s.double().requires_grad_()
    (4.0 * R.reg_loss(od, sd, w_o, w_s)).backward()  # autograd of the two means
    return o, s, g_o, g_s, c_o, c_s, od.grad, sd.grad


def _assert_added(got, start, inc, what):
    """got = start + inc at relative 1e-5 of the sum's operands."""
    err = (got.cpu().double() - (start.double() + inc)).abs()
    tol = 1e-5 * (start.double().abs() + inc.abs())
    print(f"reg {what}: max err / tol {float((err / tol).max()):.3e}")
    assert bool((err <= tol).all()), what


@pytest.mark.parametrize("n", ROWS)
def test_reg_grad_kernel_separate_tensors(dev, n):
    from clm_gs_amd import clm_kernels as K
    o, s, g_o, g_s, c_o, c_s, inc_o, inc_s = _reg_inputs(n, dev)
    od, sd, god, gsd = o.to(dev), s.to(dev), g_o.to(dev), g_s.to(dev)
    K.mcmc_reg_grad_(c_o, c_s, od, sd, god, gsd)
    assert torch.equal(od.cpu(), o) and torch.equal(sd.cpu(), s)
    _assert_added(god, g_o, inc_o, "opacity")
    _assert_added(gsd, g_s, inc_s, "scaling")


@pytest.mark.parametrize("n", ROWS)
def test_reg_grad_kernel_packed_tables(dev, n):
    from clm_gs_amd import clm_kernels as K
    o, s, g_o, g_s, c_o, c_s, inc_o, inc_s = _reg_inputs(n, dev)
    g = torch.Generator().manual_seed(n)
    pk, gk = torch.randn(n, 12, generator=g), torch.randn(n, 12, generator=g)
    pk[:, 3:4], pk[:, 4:7], gk[:, 3:4], gk[:, 4:7] = o, s, g_o, g_s
    pkd, gkd = pk.to(dev), gk.to(dev)
    K.mcmc_reg_grad_(c_o, c_s, packed=pkd, packed_grad=gkd)
    assert torch.equal(pkd.cpu(), pk)
    out = gkd.cpu()
    _assert_added(out[:, 3:4], g_o, inc_o, "packed opacity")
    _assert_added(out[:, 4:7], g_s, inc_s, "packed scaling")
    keep = [0, 1, 2, 7, 8, 9, 10, 11]
    assert torch.equal(out[:, keep], gk[:, keep])  # every other column bit-identical
    # the same values as the separate-tensor form, bit for bit
    god, gsd = g_o.to(dev), g_s.to(dev)
    K.mcmc_reg_grad_(c_o, c_s, o.to(dev), s.to(dev), god, gsd)
    assert torch.equal(god.cpu(), out[:, 3:4]) and torch.equal(gsd.cpu(), out[:, 4:7])
    # an offset view of a larger table (rows not 16 B aligned as a whole): the strided form
    if n > 1:
        big_p, big_g = torch.zeros(n * 12 + 1), torch.zeros(n * 12 + 1)
        big_p[1:], big_g[1:] = pk.flatten(), gk.flatten()
        bp, bg = big_p.to(dev), big_g.to(dev)
        K.mcmc_reg_grad_(c_o, c_s, packed=bp[1:].view(n, 12), packed_grad=bg[1:].view(n, 12))
        assert torch.equal(bg.cpu()[1:].view(n, 12), out) and float(bg[0]) == 0.0


OPACITIES = (0.001, 0.004, 0.006, 0.5, 0.999)


def _noise_inputs(n, seed=0):
    g = torch.Generator().manual_seed(3000 + 10 * n + seed)
    xyz = torch.randn(n, 3, generator=g) * 5.0
    o = torch.tensor([_logit(OPACITIES[i % len(OPACITIES)]) for i in range(n)], dtype=torch.float32)[:, None]
    o = o[torch.randperm(n, generator=g)].contiguous()
    s = torch.rand(n, 3, generator=g) * math.log(1e4) + math.log(1e-3)          # scales 1e-3 .. 1e1, per axis
    q = torch.randn(n, 4, generator=g) * torch.exp(torch.randn(n, 1, generator=g))  # un-normalised
    e = torch.randn(n, 3, generator=g)
    return xyz, o, s, q, e


SCALER = 5e5 * 1.6e-4  # mcmc_noise_lr x the initial xyz learning rate


def _check_noise(xyz0, new_xyz, o, s, q, e, scaler, what):
    dx_ref, mag = R.noise_delta(o, s, q, e, scaler)
    dx = new_xyz.cpu().double() - xyz0.double()
    bound = 1e-5 * mag + 2.0 ** -23 * xyz0.double().abs()
    ratio = ((dx - dx_ref).abs() / bound).max()
    print(f"noise {what}: max |dx - dx_ref| / bound {float(ratio):.3e}; max |dx| {float(dx.abs().max()):.3e}")
    assert bool(((dx - dx_ref).abs() <= bound).all()), what
    assert float(dx.abs().max()) > 0


@pytest.mark.parametrize("n", ROWS)
def test_noise_kernel(dev, n):
    from clm_gs_amd import clm_kernels as K
    xyz, o, s, q, e = _noise_inputs(n)
    xd = xyz.to(dev)
    od, sd, qd, ed = o.to(dev), s.to(dev), q.to(dev), e.to(dev)
    K.mcmc_inject_noise_(xd, od, sd, qd, ed, SCALER)
    for a, b in ((od, o), (sd, s), (qd, q), (ed, e)):
        assert torch.equal(a.cpu(), b)
    _check_noise(xyz, xd, o, s, q, e, SCALER, f"n={n}")
    # zero noise: bit-identical positions (signed zeros included)
    x0 = xyz.clone()
    x0[0, 0] = -0.0
    xz = x0.to(dev)
    K.mcmc_inject_noise_(xz, od, sd, qd, torch.zeros_like(ed), SCALER)
    assert torch.equal(xz.cpu().view(torch.int32), x0.view(torch.int32))
    # with the mirror: columns 0..2 are the xyz tensor bit for bit, columns 3..11 untouched; same positions as without
    g = torch.Generator().manual_seed(n)
    pk = torch.randn(n, 12, generator=g)
    pkd, xm = pk.to(dev), xyz.to(dev)
    K.mcmc_inject_noise_(xm, od, sd, qd, ed, SCALER, packed=pkd)
    assert torch.equal(xm, xd)
    assert torch.equal(pkd[:, :3].contiguous().view(torch.int32), xm.view(torch.int32))
    assert torch.equal(pkd[:, 3:].cpu(), pk[:, 3:])


@pytest.mark.parametrize("n", (5, 257))
def test_noise_kernel_unaligned_views_and_isotropic_rows(dev, n):
    """Tensors that are offset views (not 16 B aligned: the rotation is then read as four dwords) give the same bits; rows
    with equal scales (Sigma's off-diagonal terms cancel exactly) stay inside the bound."""
    from clm_gs_amd import clm_kernels as K
    xyz, o, s, q, e = _noise_inputs(n, seed=1)
    s[::2] = s[::2, :1]  # every second row isotropic
    xa = xyz.to(dev)
    K.mcmc_inject_noise_(xa, o.to(dev), s.to(dev), q.to(dev), e.to(dev), SCALER)
    _check_noise(xyz, xa, o, s, q, e, SCALER, f"isotropic n={n}")

    def off(t):  # the same values one float into a larger allocation
        big = torch.zeros(t.numel() + 1, device=dev)
        big[1:] = t.flatten().to(dev)
        return big[1:].view(t.shape)
    xb = off(xyz)
    K.mcmc_inject_noise_(xb, off(o), off(s), off(q), off(e), SCALER)
    assert torch.equal(xb, xa)


def test_operators_refuse_wrong_tensors(dev):
    from clm_gs_amd import clm_kernels as K
    n = 8
    z = lambda *s: torch.zeros(*s, device=dev)
    with pytest.raises(Exception):
        K.mcmc_inject_noise_(z(n, 3).double(), z(n, 1), z(n, 3), z(n, 4), z(n, 3), 1.0)
    with pytest.raises(Exception):
        K.mcmc_inject_noise_(z(n, 4)[:, :3], z(n, 1), z(n, 3), z(n, 4), z(n, 3), 1.0)  # not contiguous
    with pytest.raises(Exception):
        K.mcmc_inject_noise_(torch.zeros(n, 3), z(n, 1), z(n, 3), z(n, 4), z(n, 3), 1.0)  # host tensor
    with pytest.raises(Exception):
        K.mcmc_reg_grad_(1.0, 1.0, z(n, 1), z(n, 3), z(n, 1), z(n, 4))
    with pytest.raises(Exception):
        K.mcmc_relocation(z(n), z(n, 3), torch.zeros(n, dtype=torch.int64, device=dev))


# ====================================================================== models
N_MODEL, N_DEAD, MIN_OPACITY = 300, 40, 0.005


def _args(strategy, **over):
    from clm_gs_amd import utils
    args = utils.default_args(bsz=4, mcmc=True, **over)
    setattr(args, strategy, True)
    utils.set_args(args)
    return args


def _model(strategy, args, n=N_MODEL, n_dead=N_DEAD, seed=0):
    """A model of n rows with degree-3 SH, n_dead of them forced dead (opacity 0.001 .. 0.005), random non-zero moments
    in every group."""
    from clm_gs_amd.synthetic import synth_gaussians
    if strategy == "no_offload":
        from clm_gs_amd.strategies.no_offload import GaussianModelNoOffload as M
    else:
        from clm_gs_amd.strategies.clm_offload import GaussianModelCLMOffload as M
    sc = synth_gaussians(n, seed=seed, device="cuda")
    g = torch.Generator().manual_seed(seed + 1)
    op = sc["opacity"].clone().clamp_(min=_logit(0.02))          # everybody alive ...
    dead = torch.randperm(n, generator=g)[:n_dead].cuda()
    op[dead, 0] = torch.tensor([_logit(0.001 + 0.004 * i / max(n_dead - 1, 1)) for i in range(n_dead)], device="cuda")
    op[dead[-1:], 0] = _logit(MIN_OPACITY) - 1e-3              # ... but these; the last one just below the threshold
    m = M(3)
    m.create_from_tensors(sc["xyz"].clone(), sc["shs48"].clone(), sc["scaling"].clone(), sc["rotation"].clone(), op,
                          spatial_lr_scale=1.0)
    m.active_sh_degree = 3
    m.training_setup(args)
    gd = torch.Generator(device="cuda").manual_seed(seed + 2)
    if strategy == "no_offload":
        for grp in m.optimizer.param_groups:
            p = grp["params"][0]
            m.optimizer.state[p] = {"step": torch.tensor(3.0, device=p.device),
                                    "exp_avg": torch.randn(p.shape, device=p.device, generator=gd),
                                    "exp_avg_sq": torch.rand(p.shape, device=p.device, generator=gd)}
    else:
        for grp in m.optimizer.small_groups():
            st = m.optimizer.gpu_adam.state[grp["params"][0]]
            st["exp_avg"].copy_(torch.randn(st["exp_avg"].shape, device="cuda", generator=gd))
            st["exp_avg_sq"].copy_(torch.rand(st["exp_avg_sq"].shape, device="cuda", generator=gd))
        st = m.optimizer.cpu_adam.state[m._parameters]
        st["exp_avg"].copy_(torch.randn(st["exp_avg"].shape, device="cuda", generator=gd))
        st["exp_avg_sq"].copy_(torch.rand(st["exp_avg_sq"].shape, device="cuda", generator=gd))
    return m, torch.sort(dead).values


def _state(m, strategy):
    """float32 CPU tables of the model and both moments, keyed as tests/mcmc_reference.TABLES."""
    n = m._xyz.shape[0]
    out = {}
    if strategy == "no_offload":
        st = {g["name"]: m.optimizer.state[g["params"][0]] for g in m.optimizer.param_groups}
        cat = lambda a, b: torch.cat((a, b), dim=1).reshape(n, 48)
        out["shs48"] = cat(m._features_dc.detach(), m._features_rest.detach())
        out["m_shs48"] = cat(st["f_dc"]["exp_avg"], st["f_rest"]["exp_avg"])
        out["v_shs48"] = cat(st["f_dc"]["exp_avg_sq"], st["f_rest"]["exp_avg_sq"])
        small = {k: (getattr(m, "_" + k), st[k]) for k in ("xyz", "opacity", "scaling", "rotation")}
    else:
        m.flush_lazy_rows()
        st = m.optimizer.cpu_adam.state[m._parameters]
        out["shs48"], out["m_shs48"], out["v_shs48"] = m._parameters.detach(), st["exp_avg"], st["exp_avg_sq"]
        small = {k: (getattr(m, "_" + k), m.optimizer.gpu_adam.state[getattr(m, "_" + k)])
                 for k in ("xyz", "opacity", "scaling", "rotation")}
    for k, (p, s) in small.items():
        out[k], out["m_" + k], out["v_" + k] = p.detach(), s["exp_avg"], s["exp_avg_sq"]
    return {k: v.detach().cpu().clone() for k, v in out.items()}


def _compare_with_restatement(got, want, exact_rows, moved_rows, what):
    """`want` (float64) is the restatement applied to the state before.  Rows in exact_rows must carry the bits of the
    state before (want holds them exactly); rows in moved_rows took relocated values: opacity logit and log scale of
    float32 quantities, compared at 1e-5 relative + 1e-6 absolute (float32 log / logit of O(1..10) values)."""
    for k, w in want.items():
        g = got[k]
        assert g.shape == w.shape, (what, k, g.shape, w.shape)
        assert torch.equal(g[exact_rows].double(), w[exact_rows]), (what, k, "untouched rows")
        if k in ("opacity", "scaling"):
            torch.testing.assert_close(g[moved_rows].double(), w[moved_rows], rtol=1e-5, atol=1e-6)
        else:
            assert torch.equal(g[moved_rows].double(), w[moved_rows]), (what, k, "moved rows")


@pytest.mark.parametrize("strategy", ["no_offload", "clm_offload"])
def test_relocate_gs(dev, strategy):
    args = _args(strategy)
    m, forced_dead = _model(strategy, args)
    before = _state(m, strategy)
    dead_idx, src_idx = m.relocate_gs(MIN_OPACITY, torch.Generator(device="cuda").manual_seed(9))
    assert m._xyz.shape[0] == N_MODEL                                        # the row count is unchanged
    assert torch.equal(dead_idx, forced_dead) and src_idx.shape == dead_idx.shape
    assert not bool(torch.isin(src_idx, dead_idx).any())                      # sources are alive
    assert src_idx.unique().numel() < src_idx.numel()                         # (40 draws from 260 rows by opacity: repeats)
    after = _state(m, strategy)
    want = R.relocate({k: v.double() for k, v in before.items()}, dead_idx.cpu(), src_idx.cpu(), MIN_OPACITY)
    touched = torch.zeros(N_MODEL, dtype=torch.bool)
    touched[dead_idx.cpu()] = True
    touched[src_idx.cpu()] = True
    _compare_with_restatement(after, want, ~touched, touched, strategy)
    # rows that are neither dead nor sources: bit-identical to the state before, in every table and both moments
    for k in before:
        assert torch.equal(after[k][~touched], before[k][~touched]), k
    # a dead row IS its source, bit for bit, in every attribute; the sources' moments are zero, the dead rows' kept
    for k in R.TABLES:
        assert torch.equal(after[k][dead_idx.cpu()], after[k][src_idx.cpu()]), k
        assert float(after["m_" + k][src_idx.cpu()].abs().max()) == 0.0 and float(after["v_" + k][src_idx.cpu()].abs().max()) == 0.0
        assert torch.equal(after["m_" + k][dead_idx.cpu()], before["m_" + k][dead_idx.cpu()])
    assert float(torch.sigmoid(after["opacity"]).min()) >= MIN_OPACITY * (1 - 1e-5)  # nobody is dead any more
    if strategy == "clm_offload":  # the deferred-step stamps say "current, nothing waiting"; the mirror is rebuilt
        step = int(m.optimizer.cpu_adam.global_step)
        assert bool((m._row_last_step[:N_MODEL] == step).all()) and int(m._row_g_step[:N_MODEL].max()) <= step
        pk = m.small_packed()
        assert torch.equal(pk[:, :3], m._xyz.detach()) and torch.equal(pk[:, 3:4], m._opacity.detach())
    # nothing dead: nothing happens
    d2, s2 = m.relocate_gs(MIN_OPACITY, None)
    assert d2.numel() == 0 and s2.numel() == 0
    again = _state(m, strategy)
    for k in after:
        assert torch.equal(again[k], after[k]), k


@pytest.mark.parametrize("strategy", ["no_offload", "clm_offload"])
def test_add_new_gs(dev, strategy):
    args = _args(strategy)
    m, _ = _model(strategy, args, n_dead=0)
    N = N_MODEL
    before = _state(m, strategy)
    src = m.add_new_gs(10 ** 6, torch.Generator(device="cuda").manual_seed(4))
    n1 = int(1.05 * N)
    assert m._xyz.shape[0] == n1 and src.numel() == n1 - N == 15
    after = _state(m, strategy)
    want = R.add_new({k: v.double() for k, v in before.items()}, src.cpu(), MIN_OPACITY)
    moved = torch.zeros(n1, dtype=torch.bool)
    moved[src.cpu()] = True
    moved[N:] = True
    _compare_with_restatement(after, want, ~moved, moved, strategy)
    for k in R.TABLES:  # the copies are their sources, with zero moments on both sides
        assert torch.equal(after[k][N:], after[k][src.cpu()]), k
        assert float(after["m_" + k][N:].abs().max()) == 0.0 and float(after["m_" + k][src.cpu()].abs().max()) == 0.0
        assert float(after["v_" + k][N:].abs().max()) == 0.0 and float(after["v_" + k][src.cpu()].abs().max()) == 0.0
    assert m.xyz_gradient_accum.shape[0] == n1 and m.denom.shape[0] == n1 and m.max_radii2D.shape[0] == n1
    # the cap: min(cap, int(1.05 N)); one row short of the cap adds exactly one; at the cap nothing happens
    src = m.add_new_gs(n1 + 7, None)
    assert m._xyz.shape[0] == n1 + 7 and src.numel() == 7
    src = m.add_new_gs(n1 + 8, None)
    assert m._xyz.shape[0] == n1 + 8 and src.numel() == 1
    at_cap = _state(m, strategy)
    src = m.add_new_gs(n1 + 8, None)
    assert m._xyz.shape[0] == n1 + 8 and src.numel() == 0
    src = m.add_new_gs(n1, None)  # a cap below the row count: nothing either
    assert m._xyz.shape[0] == n1 + 8 and src.numel() == 0
    same = _state(m, strategy)
    for k in at_cap:
        assert torch.equal(same[k], at_cap[k]), k
    for t in (m._xyz, m._opacity, m._scaling, m._rotation):
        assert bool(torch.isfinite(t).all())


def test_add_new_gs_resorts_where_densify_and_prune_does(dev):
    """clm_offload under the trainer (fuse_sort_into_prune): the rows are left in Z-order, and the trainer's own
    spatial_sort() afterwards finds nothing to do."""
    from clm_gs_amd import utils
    args = _args("clm_offload")
    m, _ = _model("clm_offload", args, n_dead=0)
    m.spatial_sort()
    m.fuse_sort_into_prune = True
    m.add_new_gs(10 ** 6, torch.Generator(device="cuda").manual_seed(4))
    order = utils.morton_order(m._xyz.detach())
    assert torch.equal(order, torch.arange(m._xyz.shape[0], device=order.device))
    tag = m._mutations
    m.spatial_sort()
    assert m._mutations == tag  # the shortcut: already sorted


# ====================================================================== engines
W, H, N_ENG, BSZ = 96, 64, 3000, 4  # (clm_offload takes batches of 4, 8, ...: 4 is its smallest)


class _Scene:
    cameras_extent = 30.0


def _engine_setup(strategy, seed=0, **over):
    from clm_gs_amd import utils
    from clm_gs_amd.synthetic import nadir_cameras, synth_gaussians
    args = utils.default_args(bsz=BSZ, **over)
    setattr(args, strategy, True)
    utils.set_args(args)
    utils.set_img_size(H, W)
    utils.set_cur_iter(1)
    sc = synth_gaussians(N_ENG, seed=seed, device="cuda")
    sc["opacity"].clamp_(min=_logit(0.3))  # the noise gate is closed (e^-29) on every row ...
    sc["opacity"][::7] = _logit(0.003)     # ... but open on every seventh: dead Gaussians
    cams = nadir_cameras(2 * BSZ, N_ENG, W, H, 0.35, seed=seed, device="cuda")
    g = torch.Generator().manual_seed(5)
    for c in cams:
        c.original_image = (torch.rand(3, H, W, generator=g) * 255).to(torch.uint8).cuda()
    if strategy == "no_offload":
        from clm_gs_amd.strategies.no_offload import GaussianModelNoOffload as M
    else:
        from clm_gs_amd.strategies.clm_offload import GaussianModelCLMOffload as M
    m = M(3)
    m.create_from_tensors(sc["xyz"].clone(), sc["shs48"].clone(), sc["scaling"].clone(), sc["rotation"].clone(),
                          sc["opacity"].clone(), spatial_lr_scale=1.0)
    m.active_sh_degree = 3
    m.training_setup(args)
    return args, sc, cams, m


def _two_batches(strategy, m, args, cams):
    """Two batches of BSZ cameras through the engine and its optimizer epilogue, as trainer.training runs them."""
    from clm_gs_amd import trainer
    losses = []
    for b in range(2):
        batch = cams[b * BSZ:(b + 1) * BSZ]
        if strategy == "no_offload":
            from clm_gs_amd.strategies.no_offload import baseline_accumGrads_impl
            ls, vis = baseline_accumGrads_impl(m, _Scene, batch, None)
            trainer.no_offload_optimizer_step(m, args, BSZ, vis)
            order = list(range(BSZ))
        else:
            from clm_gs_amd.strategies.clm_offload import clm_offload_train_one_batch
            if b == 0:
                m._test_comm = torch.cuda.Stream()
            ls, order, _ = clm_offload_train_one_batch(m, _Scene, batch, m.parameters_grad_buffer, None, None, m._test_comm,
                                                       torch.Generator(device="cuda").manual_seed(1))
        lo = [0.0] * BSZ
        for k, l in zip(order, ls):
            lo[k] = l.item()
        losses += lo
    if strategy != "no_offload":
        m.flush_lazy_rows()
        shs = m._parameters.detach().clone()
    else:
        shs = torch.cat((m._features_dc, m._features_rest), dim=1).reshape(-1, 48).detach().clone()
    torch.cuda.synchronize()
    return dict(xyz=m._xyz.detach().clone(), opacity=m._opacity.detach().clone(), scaling=m._scaling.detach().clone(),
                rotation=m._rotation.detach().clone(), shs48=shs, losses=losses)


KEYS = ("xyz", "opacity", "scaling", "rotation", "shs48")


@pytest.mark.parametrize("strategy", ["no_offload", "clm_offload"])
def test_mcmc_mode_with_everything_off_is_the_undeferred_engine(dev, strategy):
    """Noise and both regularisers at 0, outside the refinement window: bit for bit the same engine run with
    deferred_small_adam=False, first_touch_grads=False (the model sets both in MCMC mode)."""
    args, sc, cams, m = _engine_setup(strategy, mcmc=True, mcmc_noise_lr=0.0, mcmc_opacity_reg=0.0, mcmc_scale_reg=0.0,
                                      mcmc_refine_start_iter=10 ** 9)
    if strategy == "clm_offload":
        assert not m.small_deferred and not m.first_touch_grads
    a = _two_batches(strategy, m, args, cams)
    args, sc, cams, m = _engine_setup(strategy, deferred_small_adam=False, first_touch_grads=False)
    b = _two_batches(strategy, m, args, cams)
    assert a["losses"] == b["losses"]
    for k in KEYS:
        assert torch.equal(a[k], b[k]), k
    assert float((a["xyz"] - sc["xyz"]).abs().max()) > 0


def _frac_differs(a, b, init, lr_tol):
    """tests/test_gpu_engines.py's measure for this pair: the share of elements whose step differs noticeably."""
    da, db = (a - init).cpu(), (b - init).cpu()
    scale = db.abs().max().item() + 1e-30
    return ((da - db).abs() > lr_tol * scale).float().mean().item()


def test_no_offload_and_clm_offload_agree_with_noise_and_regularisers(dev):
    """The tolerance tests/test_gpu_engines.py uses for this pair (losses 1e-5; fewer than 1 % of the elements of a
    tensor differ by more than 2 % of the largest step).  The positions are compared in two parts: rows whose gate is
    closed by that measure, rows whose gate is open (every seventh) against the noise increment, which is far larger."""
    over = dict(mcmc=True, mcmc_opacity_reg=0.01, mcmc_scale_reg=0.01)
    args, sc, cams, m = _engine_setup("no_offload", **over)
    a = _two_batches("no_offload", m, args, cams)
    args, sc, cams, m = _engine_setup("clm_offload", **over)
    b = _two_batches("clm_offload", m, args, cams)
    for u, v in zip(a["losses"], b["losses"]):
        assert abs(u - v) < 1e-5
    open_gate = torch.zeros(N_ENG, dtype=torch.bool, device="cuda")
    open_gate[::7] = True
    for k in KEYS:
        x, y, init = a[k], b[k], sc[k]
        if k == "xyz":
            moved = (x[open_gate] - init[open_gate]).abs().max().item()
            assert moved > 100 * (x[~open_gate] - init[~open_gate]).abs().max().item(), "the noise did not act"
            assert rel_l2(x[open_gate] - init[open_gate], y[open_gate] - init[open_gate]) < 1e-3
            x, y, init = x[~open_gate], y[~open_gate], init[~open_gate]
        frac = _frac_differs(x, y, init, 0.02)
        assert frac < 0.01, (k, frac)


# what test_no_offload_agrees_with_a_torch_restatement measured on an MI355X ("MCMC"): the
# relative L2 distance of the two runs' parameter UPDATES after two batches, per tensor.  The test asserts 4x these.
# "xyz" is measured on the rows whose gate is closed (Adam's step alone), "xyz_noise" on the rows whose gate is open (the
# noise increment, five orders of magnitude larger).
MEASURED_GAP = {"xyz": 1.21e-5, "xyz_noise": 7.8e-8, "opacity": 1.09e-6, "scaling": 8.2e-7, "rotation": 2.98e-6,
                "shs48": 1.27e-6}


def test_no_offload_agrees_with_a_torch_restatement(dev):
    """no_offload in MCMC mode (fused front end, the three kernels) against the same two batches spelled out in torch: the
    op-by-op gsplat.py operators under autograd, the two regulariser terms added to the loss of the step, torch.optim.Adam,
    and the reference noise (tests/mcmc_reference.noise_delta, float64) on the same noise tensors."""
    from clm_gs_amd import mcmc
    from clm_gs_amd.strategies.no_offload import baseline_accumGrads_impl
    w_o, w_s = 0.01, 0.01
    args, sc, cams, m = _engine_setup("no_offload", mcmc=True, mcmc_opacity_reg=w_o, mcmc_scale_reg=w_s)
    a = _two_batches("no_offload", m, args, cams)
    # the restatement: a plain no_offload model, op-by-op route, nothing of the MCMC code path
    args, sc, cams, m = _engine_setup("no_offload", fused_front_end=False)
    assert isinstance(m.optimizer, torch.optim.Adam)
    gen = torch.Generator(device="cuda").manual_seed(mcmc.NOISE_SEED)
    lr_xyz = [g["lr"] for g in m.optimizer.param_groups if g["name"] == "xyz"][0]
    losses = []
    for b in range(2):
        ls, _ = baseline_accumGrads_impl(m, _Scene, cams[b * BSZ:(b + 1) * BSZ], None)
        losses += [l.item() for l in ls]
        for p in m.all_parameters():
            p.grad /= BSZ
        R.reg_loss(m._opacity, m._scaling, w_o, w_s).backward()  # accumulates into .grad
        m.optimizer.step()
        m.optimizer.zero_grad(set_to_none=True)
        noise = torch.randn((N_ENG, 3), dtype=torch.float32, device="cuda", generator=gen)
        with torch.no_grad():
            dx, _ = R.noise_delta(m._opacity.detach(), m._scaling.detach(), m._rotation.detach(), noise, 5e5 * lr_xyz)
            m._xyz.data.copy_((m._xyz.detach().double() + dx).float())
    ref = dict(xyz=m._xyz.detach(), opacity=m._opacity.detach(), scaling=m._scaling.detach(), rotation=m._rotation.detach(),
               shs48=torch.cat((m._features_dc, m._features_rest), dim=1).reshape(-1, 48).detach())
    for u, v in zip(a["losses"], losses):
        assert abs(u - v) < 1e-5
    gaps = {k: rel_l2(a[k] - sc[k], ref[k] - sc[k]) for k in KEYS if k != "xyz"}
    open_gate = torch.zeros(N_ENG, dtype=torch.bool, device="cuda")
    open_gate[::7] = True
    for name, rows in (("xyz", ~open_gate), ("xyz_noise", open_gate)):
        gaps[name] = rel_l2(a["xyz"][rows] - sc["xyz"][rows], ref["xyz"][rows] - sc["xyz"][rows])
    print("restatement gap (rel L2 of the updates): " + " ".join(f"{k} {v:.3e}" for k, v in gaps.items()))
    for k in gaps:
        assert gaps[k] <= 4 * MEASURED_GAP[k], (k, gaps[k])


# ====================================================================== trainer
@pytest.mark.parametrize("strategy", ["clm_offload", "no_offload"])
def test_trainer_grows_to_the_cap_and_trains(dev, strategy):
    from clm_gs_amd import trainer, utils
    from clm_gs_amd.strategies.clm_offload import GaussianModelCLMOffload, clm_offload_eval_one_cam
    from clm_gs_amd.strategies.no_offload import GaussianModelNoOffload
    from clm_gs_amd.synthetic import nadir_cameras, synth_gaussians
    N, Wt, Ht, bsz = 20000, 160, 128, 4
    cap = int(1.3 * N)
    args = utils.default_args(bsz=bsz, mcmc=True, mcmc_cap_max=cap, mcmc_refine_every=20, mcmc_refine_start_iter=40,
                              mcmc_refine_stop_iter=10 ** 6)
    setattr(args, strategy, True)
    utils.set_args(args)
    utils.set_img_size(Ht, Wt)
    utils.set_cur_iter(1)
    truth = synth_gaussians(N, seed=7, device="cuda")
    cams = nadir_cameras(24, N, Wt, Ht, 0.3, seed=7, device="cuda")
    gt_model = GaussianModelCLMOffload(3, only_for_rendering=True)
    gt_model.args = utils.default_args(bsz=bsz, sh_residency="hbm")
    gt_model.create_from_tensors(truth["xyz"], truth["shs48"], truth["scaling"], truth["rotation"], truth["opacity"])
    gt_model.active_sh_degree = 3
    for c in cams:
        c.original_image = (clm_offload_eval_one_cam(c, gt_model, None, None).clamp(0, 1) * 255).round().to(torch.uint8)
    g = torch.Generator(device="cuda").manual_seed(1)
    noisy_sh = truth["shs48"].clone()
    noisy_sh[:, :3] += torch.randn((N, 3), generator=g, device="cuda") * 0.6
    model = {"clm_offload": GaussianModelCLMOffload, "no_offload": GaussianModelNoOffload}[strategy](3)
    model.create_from_tensors(truth["xyz"] + torch.randn((N, 3), generator=g, device="cuda") * 0.05, noisy_sh,
                              truth["scaling"], truth["rotation"], truth["opacity"], spatial_lr_scale=truth["extent"])
    model.training_setup(args)
    model.split_generator = torch.Generator(device="cuda").manual_seed(5)

    class Scene:
        cameras_extent = truth["extent"]

    sizes = []
    log = io.StringIO()
    trainer.training(model, Scene, cams, [], log, iterations=400,
                     phase_times={"iter_hook": lambda it: sizes.append(int(model.get_xyz.shape[0]))})
    text = log.getvalue()
    assert len(sizes) == 100 and max(sizes) <= cap, max(sizes)            # N never exceeds the cap
    assert sizes[-1] == cap == int(model.get_xyz.shape[0])                # ... and equals it at the end
    assert sizes[0] == N and sorted(sizes) == sizes and len(set(sizes)) >= 6
    assert "MCMC refinement" in text and "Number of split gaussians" not in text
    if hasattr(model, "flush_lazy_rows"):
        model.flush_lazy_rows()
    params = [model._xyz, model._opacity, model._scaling, model._rotation, model._features_dc, model._features_rest]
    for t in params:
        assert t.shape[0] == cap and bool(torch.isfinite(t).all())
    losses = [float(x) for l in text.splitlines() if " loss: " in l for x in l.split(" loss: ")[1].split(" image:")[0].split()]
    assert len(losses) == 400 and all(math.isfinite(x) for x in losses)
    first, last = sum(losses[:24]) / 24, sum(losses[-24:]) / 24  # one pass over the cameras each
    print(f"trainer {strategy}: loss {first:.5f} -> {last:.5f}; sizes {sorted(set(sizes))}")
    assert last < first
