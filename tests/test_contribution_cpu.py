"""CPU: the float64 reference of the blend-weight pass against the oracle's rasterizer, the fragile-pixel condition its
allowances rest on, the two prune policies and the refused flag combinations of contribution pruning."""
import math

import pytest
import torch

from oracle import gs_oracle as O
from tests import contribution_reference as R

# fragile in-image pixels of the cases that have any (tests/contribution_reference.py: its definition); every other
# case has none
FRAGILE_LIMIT = 0.08


@pytest.mark.parametrize("name", R.case_names())
def test_reference_sums_to_the_oracle_alpha_image_and_few_pixels_are_fragile(name):
    case, ref = R.cached(name)
    _, alpha = O.rasterize_to_pixels(case["m2"].double(), case["cn"].double(), case["col"].double(), case["op"].double(),
                                     case["w"], case["h"], 16, case["off"], case["fids"])
    want = float(alpha.sum())
    got = float(ref["wsum"].sum())
    print(f"{name}: sum(wsum) {got:.17g} oracle alpha sum {want:.17g} rel {abs(got - want) / max(abs(want), 1e-300):.3g}; "
          f"fragile {ref['fragile']} / {ref['inside']}")
    assert abs(got - want) <= 1e-12 * abs(want)
    assert abs(ref["alpha_sum"] - want) <= 1e-12 * abs(want)
    assert ref["inside"] == case["op"].shape[0] * case["w"] * case["h"]
    assert ref["fragile"] <= FRAGILE_LIMIT * ref["inside"], (ref["fragile"], ref["inside"])
    # consistency of the three arrays: a row has pixels exactly where it has weight, wmax <= wsum <= pixels * wmax
    assert torch.equal(ref["pixels"] > 0, ref["wsum"] > 0) and torch.equal(ref["pixels"] > 0, ref["wmax"] > 0)
    assert bool((ref["wmax"] <= ref["wsum"] * (1 + 1e-15)).all())
    assert bool((ref["wsum"] <= ref["pixels"].double() * ref["wmax"] * (1 + 1e-12)).all())
    assert bool((ref["allowance"] >= 0).all()) and int(ref["allowance"].max()) <= ref["fragile"]


def test_lowest_fraction_mask_counts_and_ties():
    from clm_gs_amd.contribution import lowest_fraction_mask
    g = torch.Generator().manual_seed(0)
    for n in (1, 7, 10, 1000, 4097):
        w = torch.rand(n, generator=g, dtype=torch.float64)
        for ratio in (0.0, 0.1, 0.29, 0.3, 0.5, 0.999, 1.0):
            m = lowest_fraction_mask(w, ratio)
            k = int(math.floor(ratio * n))
            assert m.dtype == torch.bool and m.shape == (n,) and int(m.sum()) == k, (n, ratio)
            if 0 < k < n:
                assert float(w[m].max()) <= float(w[~m].min())
    assert int(lowest_fraction_mask(torch.rand(50, generator=g), 0.0).sum()) == 0
    assert bool(lowest_fraction_mask(torch.rand(50, generator=g), 1.0).all())
    # ties: the lower row index goes first -- all equal, and a tie that straddles the cut
    m = lowest_fraction_mask(torch.zeros(10, dtype=torch.float64), 0.35)
    assert m.tolist() == [True] * 3 + [False] * 7
    w = torch.tensor([5.0, 1.0, 2.0, 1.0, 2.0, 2.0, 0.0, 2.0])
    assert torch.nonzero(lowest_fraction_mask(w, 0.5)).flatten().tolist() == [1, 2, 3, 6]
    assert torch.nonzero(lowest_fraction_mask(w, 0.625)).flatten().tolist() == [1, 2, 3, 4, 6]
    assert lowest_fraction_mask(torch.zeros(0), 0.3).numel() == 0
    for bad in (-0.1, 1.5, float("nan")):
        with pytest.raises(ValueError, match="contrib_prune_ratio"):
            lowest_fraction_mask(w, bad)


def test_below_max_mask_threshold_edges():
    from clm_gs_amd.contribution import below_max_mask
    w = torch.tensor([0.0, 0.0099999, 0.01, 0.0100001, 0.5, 0.999], dtype=torch.float32)
    assert below_max_mask(w, 0.01).tolist() == [True, True, False, False, False, False]  # strictly below
    assert below_max_mask(w, 0.0).tolist() == [False] * 6
    assert below_max_mask(w, 1.0).tolist() == [True] * 6
    assert below_max_mask(w.reshape(6, 1), 0.01).shape == (6,)


def test_stats_units_without_a_device():
    from clm_gs_amd.contribution import ContributionStats, prune_mask
    st = ContributionStats(4, "cpu")
    assert st.wsum_q.dtype == torch.int64 and st.wmax_bits.dtype == torch.int32 and st.pixels.dtype == torch.int64
    st.wsum_q += torch.tensor([0, 1, 2 ** 28, 3 * 2 ** 27])
    st.wmax_bits.copy_(torch.tensor([0.0, 0.25, 0.999, 0.005]).view(torch.int32))
    assert st.wsum.dtype == torch.float64 and st.wsum.tolist() == [0.0, 2.0 ** -28, 1.0, 1.5]
    assert st.wmax.dtype == torch.float32 and st.wmax.tolist() == torch.tensor([0.0, 0.25, 0.999, 0.005]).tolist()
    assert prune_mask(st, "sum", ratio=0.5).tolist() == [True, True, False, False]
    assert prune_mask(st, "max", threshold=0.01).tolist() == [True, False, False, True]
    with pytest.raises(ValueError, match="contrib_prune_mode"):
        prune_mask(st, "median")
    assert int(st.zero_().wsum_q.sum()) == 0 and int(st.wmax_bits.abs().sum()) == 0


def _args(**over):
    from clm_gs_amd import utils
    a = utils.default_args(clm_offload=True, contrib_prune_iterations=(20000,), **over)
    return a


def test_refused_flag_combinations_raise_by_name(monkeypatch):
    from clm_gs_amd import contribution, dp, utils
    chk = contribution.check_contrib_prune_args
    chk(utils.default_args())                       # flags off: nothing to refuse, whatever else is set
    chk(utils.default_args(naive_offload=True, mcmc=True))
    chk(_args())                                    # after densify_until_iter = 15000
    chk(_args(sh_residency="host"))
    chk(utils.default_args(no_offload=True, contrib_prune_iterations=(40,), disable_auto_densification=True))
    with pytest.raises(ValueError, match="contrib_prune_iterations .*15000.* densification window"):
        chk(utils.default_args(clm_offload=True, contrib_prune_iterations=(20000, 15000)))
    with pytest.raises(ValueError, match="contrib_prune_iterations is not supported with naive_offload"):
        chk(utils.default_args(naive_offload=True, contrib_prune_iterations=(20000,)))
    with pytest.raises(ValueError, match="contrib_prune_iterations is not supported with mcmc"):
        chk(_args(mcmc=True))
    with pytest.raises(ValueError, match="contrib_prune_mode"):
        chk(_args(contrib_prune_mode="median"))
    with pytest.raises(ValueError, match="contrib_prune_ratio"):
        chk(_args(contrib_prune_ratio=1.5))
    monkeypatch.setattr(dp, "world_size", lambda: 2)
    with pytest.raises(ValueError, match="contrib_prune_iterations is not supported with camera-DP"):
        chk(_args())


def test_command_lines_carry_the_flags():
    from clm_gs_amd import trainer
    a = trainer.build_arg_parser().parse_args(["-s", "x", "-m", "y"])
    assert a.contrib_prune_iterations == [] and a.contrib_prune_mode == "sum" and a.contrib_prune_ratio == 0.3
    assert a.contrib_prune_threshold == 0.01
    a = trainer.build_arg_parser().parse_args(["-s", "x", "-m", "y", "--contrib_prune_iterations", "20000", "25000",
                                               "--contrib_prune_mode", "max", "--contrib_prune_threshold", "0.02"])
    assert a.contrib_prune_iterations == [20000, 25000] and a.contrib_prune_mode == "max" and a.contrib_prune_threshold == 0.02
