"""Not GPU: the float64 restatement of MCMC densification (tests/mcmc_reference.py) against the identities it must
satisfy, the inverse-CDF sampler, the refinement schedule, the refused combinations and the arguments."""
import math

import numpy as np
import pytest
import torch

from tests import mcmc_reference as R


# ------------------------------------------------------------------ relocation restatement
def test_relocation_at_ratio_one_returns_its_inputs():
    g = torch.Generator().manual_seed(0)
    o = (0.005 + 0.985 * torch.rand(200, generator=g, dtype=torch.float64)).numpy()
    s = torch.exp(torch.randn(200, 3, generator=g, dtype=torch.float64)).numpy()
    new_o, new_s, kappa = R.relocation(o, s, np.ones(200, dtype=np.int32))
    np.testing.assert_allclose(new_o, o, rtol=1e-13)     # D = o' = o
    np.testing.assert_allclose(new_s, s, rtol=1e-13)
    np.testing.assert_allclose(kappa, 1.0, rtol=1e-13)   # a single term


@pytest.mark.parametrize("ratio", [0, 1, 2, 3, 8, 51, 200])
def test_relocated_copies_compose_to_the_original_opacity(ratio):
    g = torch.Generator().manual_seed(ratio)
    o = (0.005 + 0.985 * torch.rand(300, generator=g, dtype=torch.float64)).numpy()
    new_o, _, _ = R.relocation(o, np.ones((300, 3)), np.full(300, ratio, dtype=np.int32))
    r = min(max(ratio, 1), 51)  # 0 and 200 exercise the clamp
    np.testing.assert_allclose(1.0 - (1.0 - new_o) ** r, o, rtol=1e-11)
    assert np.all(new_o > 0) and np.all(new_o <= o * (1 + 1e-12))


def test_relocation_shrinks_scales_of_repeated_gaussians():
    """D > o for r > 1 (the copies overlap), so the factor o / D is below 1 and falls with the ratio."""
    o = np.full(4, 0.6)
    _, s, _ = R.relocation(o, np.ones((4, 3)), np.array([1, 2, 8, 51], dtype=np.int32))
    assert s[0, 0] == pytest.approx(1.0, rel=1e-13) and np.all(np.diff(s[:, 0]) < 0) and np.all(s > 0)


def test_the_gpu_test_inputs_are_well_conditioned():
    """tests/test_gpu_mcmc.py compares the kernel at relative 1e-6 where kappa <= 1e6 and may exclude at most 10 % of
    its elements by that rule: the restatement alone keeps the chosen inputs within it (here: excludes none)."""
    for n in (1, 63, 64, 65, 255, 256, 257, 1000):
        o, s, ratios = R.relocation_inputs(n)
        assert o.dtype == torch.float32 and bool((o >= torch.tensor(0.005)).all()) and bool((o <= torch.tensor(0.99)).all())
        assert set(ratios.tolist()) <= {0, 1, 2, 3, 8, 51, 200}
        _, new_s, kappa = R.relocation(o.numpy(), s.numpy(), ratios.numpy())
        assert np.all(np.isfinite(new_s)) and np.all(np.isfinite(kappa))
        assert float((kappa > 1e6).mean()) <= 0.10, (n, float(kappa.max()))
    o, s, ratios = R.relocation_inputs(1000)
    assert set(ratios.tolist()) == {0, 1, 2, 3, 8, 51, 200}


# ------------------------------------------------------------------ reg / noise restatement
def test_reg_grads_are_the_gradients_of_the_two_means():
    g = torch.Generator().manual_seed(1)
    o = torch.randn(37, 1, generator=g, dtype=torch.float64, requires_grad=True)
    s = torch.randn(37, 3, generator=g, dtype=torch.float64, requires_grad=True)
    R.reg_loss(o, s, 0.01, 0.02).backward()
    go, gs = R.reg_grads(o.detach(), s.detach(), 0.01 / 37, 0.02 / (3 * 37))
    torch.testing.assert_close(go, o.grad, rtol=1e-12, atol=0)
    torch.testing.assert_close(gs, s.grad, rtol=1e-12, atol=0)


def test_noise_gate_and_covariance():
    """The gate is ~1 for dead Gaussians and vanishes for live ones; an isotropic Gaussian moves along its noise."""
    logit = lambda p: math.log(p / (1 - p))
    o = torch.tensor([[logit(0.001)], [logit(0.005)], [logit(0.5)]], dtype=torch.float64)
    s = torch.full((3, 3), math.log(0.5), dtype=torch.float64)
    q = torch.tensor([[2.0, 0.3, -0.7, 0.1]] * 3, dtype=torch.float64)  # not normalised
    e = torch.tensor([[1.0, -2.0, 0.5]] * 3, dtype=torch.float64)
    dx, mag = R.noise_delta(o, s, q, e, 2.0)
    gate = [1 / (1 + math.exp(-100 * ((1 - p) - 0.995))) for p in (0.001, 0.005, 0.5)]
    assert gate[0] > 0.59 and gate[1] == pytest.approx(0.5) and gate[2] < 1e-20
    for i in range(3):
        torch.testing.assert_close(dx[i], 0.25 * e[i] * gate[i] * 2.0, rtol=1e-9, atol=1e-30)
    assert bool((mag >= dx.abs() * (1 - 1e-12)).all())


# ------------------------------------------------------------------ sampler
def test_sampler_is_reproducible_and_multinomial():
    from clm_gs_amd.strategies.base_gaussian_model import mcmc_sample
    p = torch.tensor([0.1, 0.0, 2.0, 0.7, 1.2])
    n = 200_000
    a = mcmc_sample(p, n, torch.Generator().manual_seed(3))
    b = mcmc_sample(p, n, torch.Generator().manual_seed(3))
    c = mcmc_sample(p, n, torch.Generator().manual_seed(4))
    assert a.dtype == torch.int64 and torch.equal(a, b) and not torch.equal(a, c)
    assert torch.equal(a, R.sample(p, n, torch.Generator().manual_seed(3)))
    counts = torch.bincount(a, minlength=5).double()
    prob = (p / p.sum()).double()
    sd = torch.sqrt(n * prob * (1 - prob))
    assert bool(((counts - n * prob).abs() <= 5 * sd).all()), counts.tolist()
    assert counts[1] == 0  # a category of weight 0 is never drawn


def test_sampler_works_beyond_torch_multinomial():
    from clm_gs_amd.strategies.base_gaussian_model import mcmc_sample
    n_cat = 2 ** 24 + 1
    p = torch.ones(n_cat)
    p[-1] = 1000.0
    with pytest.raises(RuntimeError):
        torch.multinomial(p, 16, replacement=True)
    idx = mcmc_sample(p, 100_000, torch.Generator().manual_seed(0))
    assert int(idx.min()) >= 0 and int(idx.max()) <= n_cat - 1
    assert int((idx == n_cat - 1).sum()) > 0           # the heavy last category is reachable
    assert int((idx >= 2 ** 24 - 4096).sum()) > 0 and int((idx < 2 ** 23).sum()) > 40_000


# ------------------------------------------------------------------ schedule
class _FakeModel:
    split_generator = None

    def __init__(self):
        self.calls = []

    def relocate_gs(self, min_opacity, generator):
        self.calls.append("relocate")
        return torch.zeros(3, dtype=torch.int64), torch.zeros(3, dtype=torch.int64)

    def add_new_gs(self, cap_max, generator):
        self.calls.append(("add", cap_max))
        return torch.zeros(2, dtype=torch.int64)

    def densify_and_prune(self, *a, **k):
        raise AssertionError("densify_and_prune in MCMC mode")

    def reset_opacity(self, *a, **k):
        raise AssertionError("opacity reset in MCMC mode")


@pytest.mark.parametrize("bsz,expected", [
    (1, [60, 80, 100, 120, 140, 160, 180]),
    # image counters 1, 5, 9, ...: the batch [57, 61) crosses 60, ..., [197, 201) crosses 200 and starts inside the window;
    # [37, 41) crosses 40 but starts at or before mcmc_refine_start_iter
    (4, [57, 77, 97, 117, 137, 157, 177, 197]),
])
def test_refinement_schedule(bsz, expected):
    from clm_gs_amd import densification, utils
    args = utils.default_args(bsz=bsz, mcmc=True, mcmc_refine_start_iter=40, mcmc_refine_stop_iter=200,
                              mcmc_refine_every=20, mcmc_cap_max=1234, no_offload=True)
    utils.set_args(args)
    try:
        m, refined = _FakeModel(), []
        for it in range(1, 3300, bsz):  # past densify_from_iter and the opacity reset at 3000: neither exists in the mode
            n0 = len(m.calls)
            if densification.mcmc_refinement(it, None, m):
                refined.append(it)
                assert m.calls[n0:] == ["relocate", ("add", 1234)]  # relocation first, then growth
            else:
                assert len(m.calls) == n0
        assert refined == expected
    finally:
        utils.set_args(None)


# ------------------------------------------------------------------ refusals
@pytest.mark.parametrize("over,names", [
    (dict(clm_offload=True, sh_residency="host"), "sh_residency"),
    (dict(clm_offload=True, sh_hbm_budget_gb=1.0), "sh_hbm_budget_gb"),
    (dict(naive_offload=True), "naive_offload"),
    (dict(clm_offload=True, sparse_adam=True), "sparse_adam"),
    (dict(no_offload=True, sparse_adam=True), "sparse_adam"),
    (dict(no_offload=True, stop_update_param=True), "stop_update_param"),
])
def test_refused_combinations_name_the_flag(over, names):
    from clm_gs_amd import densification, utils
    with pytest.raises(ValueError, match=names):
        densification.check_mcmc_args(utils.default_args(mcmc=True, **over))
    densification.check_mcmc_args(utils.default_args(mcmc=False, **over))  # the mode off: nothing is refused


def test_camera_dp_is_refused(monkeypatch):
    from clm_gs_amd import densification, dp, utils
    monkeypatch.setattr(dp, "world_size", lambda: 2)
    with pytest.raises(ValueError, match="camera-DP"):
        densification.check_mcmc_args(utils.default_args(mcmc=True, clm_offload=True))


def test_supported_combinations_pass():
    from clm_gs_amd import densification, utils
    densification.check_mcmc_args(utils.default_args(mcmc=True, no_offload=True))
    densification.check_mcmc_args(utils.default_args(mcmc=True, clm_offload=True, sh_residency="hbm"))


# ------------------------------------------------------------------ arguments
def test_argument_names_and_defaults():
    from clm_gs_amd import trainer, utils
    a = utils.default_args()
    want = dict(mcmc=False, mcmc_cap_max=1_000_000, mcmc_noise_lr=5e5, mcmc_refine_start_iter=500,
                mcmc_refine_stop_iter=25_000, mcmc_refine_every=100, mcmc_min_opacity=0.005, mcmc_opacity_reg=0.01,
                mcmc_scale_reg=0.01)
    for k, v in want.items():
        assert getattr(a, k) == v and type(getattr(a, k)) is type(v), k
    ns = trainer.build_arg_parser().parse_args(["-s", "x", "-m", "y"])
    assert ns.mcmc is False and ns.cap_max == 1_000_000 and ns.mcmc_noise_lr == 5e5
    assert (ns.mcmc_refine_start_iter, ns.mcmc_refine_stop_iter, ns.mcmc_refine_every) == (500, 25_000, 100)
    assert (ns.mcmc_min_opacity, ns.mcmc_opacity_reg, ns.mcmc_scale_reg) == (0.005, 0.01, 0.01)
    ns = trainer.build_arg_parser().parse_args(["-s", "x", "-m", "y", "--mcmc", "--cap_max", "2000000"])
    assert ns.mcmc is True and ns.cap_max == 2_000_000
