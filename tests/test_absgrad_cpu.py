"""CPU-only: the float64 absgrad reference (tests/absgrad_reference.py) is sound on the inputs the GPU tests use, and the
absgrad entries are part of the C ABI, the binding table and the argument set.

The first three tests guard the reference and the inputs (they hold with or without the feature): the reference's plain
sum of per-pixel gradients is the oracle's autograd v_means2d, the absolute sum dominates it componentwise, and on
every multi-pixel case the two are far apart, so a kernel that returned |signed sum| cannot pass the GPU tests."""
import ctypes
import os
import re

import pytest
import torch

from tests import scenes as S
from tests.absgrad_reference import case_absgrad, oracle_v_means2d
from tests.scenes import rel_l2

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("clmgs_rasterize_abs_bwd", "clmgs_rasterize_abs_bwd_dev", "clmgs_preprocess_abs_bwd")
CASES = {
    "special": lambda: S.special_entry_case(),
    "tiles9_C3": lambda: S.shape_case("tiles9_C3"),
    "1x1": lambda: S.shape_case("1x1"),
    "list300_sat_single": lambda: S.list_case(300, True, "single"),
    "list65_tr_middle": lambda: S.list_case(65, False, "middle"),
}


@pytest.fixture(scope="module")
def refs():
    out = {}
    for name, make in CASES.items():
        case = make()
        a, s = case_absgrad(case)
        out[name] = (a, s, oracle_v_means2d(case))
    return out


@pytest.mark.parametrize("name", list(CASES))
def test_plain_sum_of_per_pixel_gradients_is_the_oracles_v_means2d(refs, name):
    a, s, v = refs[name]
    assert float(v.norm()) > 0
    assert rel_l2(s, v) < 1e-12


@pytest.mark.parametrize("name", list(CASES))
def test_absgrad_dominates_the_signed_sum(refs, name):
    a, s, _ = refs[name]
    assert bool((a >= s.abs() * (1 - 1e-12)).all())
    if name == "1x1":  # one pixel: nothing to cancel
        assert rel_l2(a, s.abs()) < 1e-14
    else:  # measured 17.6 / 4.4 / 19.1 / 15.1
        assert float(a.norm()) > 2 * float(s.norm()), float(a.norm()) / float(s.norm())


def test_exact_zero_rows_of_the_reference(refs):
    """Rows that are never valid, or clamped at every valid pixel, have an exactly zero absgrad; the GPU tests hold the
    kernels to exact zeros there."""
    assert int((refs["special"][0] == 0).all(dim=1).sum()) == 26
    assert int((refs["list300_sat_single"][0] == 0).all(dim=1).sum()) == 108


def test_library_header_and_bindings_carry_the_abs_entries():
    from clm_gs_amd import _lib
    l = ctypes.CDLL(_lib.LIB_PATH)
    header = open(os.path.join(ROOT, "include", "clmgs.h")).read()
    for name in NEW_SYMBOLS:
        assert name in _lib.SIGNATURES, name
        assert hasattr(l, name), name
        assert re.search(r"\bint %s\(" % name, header), name
    sig = _lib.SIGNATURES
    vp = sig["clmgs_rasterize_bwd"][1][-1]
    # the plain entries' arguments, plus one trailing optional output where the plain entry has an unpacked neighbour
    assert sig["clmgs_rasterize_abs_bwd"] == (sig["clmgs_rasterize_bwd"][0], sig["clmgs_rasterize_bwd"][1] + [vp])
    assert sig["clmgs_rasterize_abs_bwd_dev"] == sig["clmgs_rasterize_bwd_dev"]
    assert sig["clmgs_preprocess_abs_bwd"] == (sig["clmgs_preprocess_bwd"][0], sig["clmgs_preprocess_bwd"][1] + [vp])


def test_absgrad_is_an_argument_and_off_by_default():
    from clm_gs_amd import utils
    assert utils.default_args().absgrad is False
    assert utils.default_args(absgrad=True).absgrad is True


def test_absgrad_with_a_fourth_channel_is_not_implemented():
    from clm_gs_amd import gsplat
    n = 5
    inputs = (torch.zeros(1, n, 2), torch.ones(1, n, 3), torch.zeros(1, n, 4), torch.ones(1, n), 16, 16, 16,
              torch.zeros(1, 1, 1, dtype=torch.int32), torch.zeros(0, dtype=torch.int32))
    with pytest.raises(NotImplementedError):
        gsplat.rasterize_to_pixels(*inputs, absgrad=True)
