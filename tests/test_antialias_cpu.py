"""CPU-only: gsplat's antialiased mode (Mip-Splatting opacity compensation).  The float64 reference of
tests/antialias_reference.py is held to the oracle, its guarded square-root derivative to plain autograd, and the
product's fp32 formulas (clm_gs_amd/csrc/gs_math.h project_fwd_aa / project_bwd_aa, compiled with plain g++) to the
reference.  Scene A = small_scene() (compensation 0.68-0.99), scene B = small_scene(log_scale=-3.5) (0.043-0.63, median
0.21: the regime the mode exists for), extremes = small_scene(log_scale=-5.0) (0.002-0.08)."""
import ctypes
import os
import re
import subprocess

import pytest
import torch

from oracle import gs_oracle as O
from tests import antialias_reference as R
from tests.scenes import rel_l2, small_scene

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GRAD_TOL = 2e-4   # tests/test_gpu_raster_edges.py
COMP_TOL = 1e-5   # the conics' bound of tests/test_gpu_ops.py::test_projection_fwd_bwd
SCENES = {"A": {}, "B": {"log_scale": -3.5}}
NEW_SYMBOLS = ("clmgs_projection_aa_fwd", "clmgs_projection_aa_bwd", "clmgs_preprocess_aa_fwd",
               "clmgs_preprocess_aa_bwd", "clmgs_preprocess_aa_abs_bwd")


@pytest.fixture(scope="module")
def shim():
    out = os.path.join("/tmp", f"gs_math_aa_shim_{os.getpid()}.so")
    subprocess.check_call(["g++", "-O2", "-shared", "-fPIC", "-I", os.path.join(ROOT, "clm_gs_amd", "csrc"),
                           os.path.join(ROOT, "tests", "host_shim", "gs_math_aa_shim.cpp"), "-o", out])
    return ctypes.CDLL(out)


def _P(t):
    return ctypes.c_void_p(t.data_ptr())


def _shim_fwd(shim, s):
    N, f = s["means"].shape[0], ctypes.c_float
    means, quats, scales = s["means"].contiguous(), s["quats"].contiguous(), s["scales"].contiguous()
    vm, K = s["viewmat"].contiguous(), s["K"].contiguous()
    radii = torch.zeros(N, dtype=torch.int32)
    m2, d, cn, comp = torch.zeros(N, 2), torch.zeros(N), torch.zeros(N, 3), torch.full((N,), float("nan"))
    shim.shim_project_aa_fwd(N, _P(means), _P(quats), _P(scales), _P(vm), _P(K), f(s["width"]), f(s["height"]), f(0.3),
                             f(0.01), f(1e10), f(0.0), _P(radii), _P(m2), _P(d), _P(cn), _P(comp))
    return radii, m2, d, cn, comp


def _shim_bwd(shim, s, radii, vm2, vd, vc, vk):
    N, f = s["means"].shape[0], ctypes.c_float
    means, quats, scales = s["means"].contiguous(), s["quats"].contiguous(), s["scales"].contiguous()
    vm, K = s["viewmat"].contiguous(), s["K"].contiguous()
    vmn, vq, vs, comp = torch.zeros(N, 3), torch.zeros(N, 4), torch.zeros(N, 3), torch.zeros(N)
    shim.shim_project_aa_bwd(N, _P(means), _P(quats), _P(scales), _P(vm), _P(K), f(s["width"]), f(s["height"]), f(0.3),
                             _P(radii), _P(vm2.contiguous()), _P(vd.contiguous()), _P(vc.contiguous()), _P(vk.contiguous()),
                             _P(vmn), _P(vq), _P(vs), _P(comp))
    return vmn, vq, vs, comp


@pytest.mark.parametrize("name", ["A", "B"])
def test_reference_is_the_oracles_projection(name):
    s = small_scene(**SCENES[name])
    (m, q, sc), vm, K = R.scene_f64(s)
    with torch.no_grad():
        r0, m0, d0, c0, _ = O.fully_fused_projection(m, None, q, sc, vm, K, s["width"], s["height"])
        r1, m1, d1, c1, comp = R.projection(m, q, sc, vm, K, s["width"], s["height"])
    assert torch.equal(r0, r1)
    for a, b in ((m0, m1), (d0, d1), (c0, c1)):
        assert float((a - b).abs().max()) <= 1e-12
    vis = r1[0] > 0
    lo, hi = float(comp[0][vis].min()), float(comp[0][vis].max())
    print(f"scene {name}: {int(vis.sum())} visible rows, compensation {lo:.3g} .. {hi:.3g}, median {float(comp[0][vis].median()):.3g}")
    assert float(comp[0][~vis].abs().max()) == 0.0 and 0.0 < lo and hi < 1.0
    if name == "A":
        assert int(vis.sum()) == 373 and lo > 0.6
    else:
        assert int(vis.sum()) == 341 and float(comp[0][vis].median()) < 0.3


@pytest.mark.parametrize("name", ["A", "B"])
def test_guarded_derivative_is_the_plain_one_up_to_the_guard(name):
    """d sqrt(x) = 0.5 / (comp + 1e-6) against 0.5 / comp: a relative difference of 1e-6 / (comp + 1e-6) < 1e-6 / min(comp)
    in every row's contribution, hence in the whole gradient."""
    s = small_scene(**SCENES[name])
    g = torch.Generator().manual_seed(3)
    vk = torch.randn(1, s["means"].shape[0], generator=g).double()
    grads, cmin = {}, None
    for guarded in (True, False):
        (m, q, sc), vm, K = R.scene_f64(s)
        r, _, _, _, comp = R.projection(m, q, sc, vm, K, s["width"], s["height"], guarded=guarded)
        (comp * vk).sum().backward()
        grads[guarded] = (m.grad, q.grad, sc.grad)
        cmin = float(comp.detach()[0][r[0] > 0].min())
    for a, b in zip(grads[True], grads[False]):
        e = rel_l2(a, b)
        print(f"scene {name}: guarded vs plain derivative rel_l2 {e:.3g} (bound {1e-6 / cmin:.3g})")
        assert 0.0 < e < 1e-6 / cmin


@pytest.mark.parametrize("name", ["A", "B"])
def test_product_formulas_against_the_reference(shim, name):
    """fp32 product (g++ shim) against the float64 reference.  Measured: compensation rel-L2 4.5e-8 on scene A and
    1.8e-7 on scene B (fp32 cancellation in det_orig does not show: the bound stays 1e-5 on both), gradients <= 1.1e-6
    with v_compensation alone and <= 6.3e-7 with all cotangents ("Antialiased")."""
    s = small_scene(**SCENES[name])
    N = s["means"].shape[0]
    radii, m2, d, cn, comp = _shim_fwd(shim, s)
    (m, q, sc), vm, K = R.scene_f64(s)
    r0, m0, d0, c0, k0 = R.projection(m, q, sc, vm, K, s["width"], s["height"])
    assert torch.equal(r0[0], radii)
    ok = radii > 0
    assert float(comp[~ok].abs().max()) == 0.0
    e = rel_l2(comp[ok], k0[0][ok])
    print(f"scene {name}: compensation rel_l2 {e:.3g}")
    assert e < COMP_TOL
    assert rel_l2(cn[ok], c0[0][ok]) < 1e-5 and rel_l2(m2[ok], m0[0][ok]) < 1e-6
    g = torch.Generator().manual_seed(1)
    vm2, vd, vc, vk = (torch.randn(N, 2, generator=g), torch.randn(N, generator=g), torch.randn(N, 3, generator=g),
                       torch.randn(N, generator=g))
    zero = lambda t: torch.zeros_like(t)
    for what, (a2, ad, ac) in (("v_compensation alone", (zero(vm2), zero(vd), zero(vc))), ("all cotangents", (vm2, vd, vc))):
        for t in (m, q, sc):
            t.grad = None
        ((m0[0] * a2.double()).sum() + (d0[0] * ad.double()).sum() + (c0[0] * ac.double()).sum()
         + (k0[0] * vk.double()).sum()).backward(retain_graph=True)
        vmn, vq, vs, comp_b = _shim_bwd(shim, s, radii, a2, ad, ac, vk)
        assert torch.equal(comp_b[ok], comp[ok])  # the backward recomputes the forward's factor
        for pname, x, y in (("means", vmn, m.grad), ("quats", vq, q.grad), ("scales", vs, sc.grad)):
            e = rel_l2(x[ok], y[ok])
            print(f"scene {name}, {what}: v_{pname} rel_l2 {e:.3g}")
            assert e < GRAD_TOL, (what, pname, e)
        assert float(vmn[~ok].abs().max()) == 0.0


def test_extremes_stay_finite(shim):
    """Compensation 0.002-0.08: the guard dominates the derivative, so no accuracy claim; finite and in [0, 1]."""
    s = small_scene(log_scale=-5.0)
    N = s["means"].shape[0]
    radii, _, _, _, comp = _shim_fwd(shim, s)
    ok = radii > 0
    assert int(ok.sum()) > 100
    assert torch.isfinite(comp).all() and float(comp.min()) >= 0.0 and float(comp.max()) <= 1.0
    assert float(comp[ok].max()) < 0.2
    g = torch.Generator().manual_seed(2)
    vm2, vd, vc, vk = (torch.randn(N, 2, generator=g), torch.randn(N, generator=g), torch.randn(N, 3, generator=g),
                       torch.randn(N, generator=g))
    for x in _shim_bwd(shim, s, radii, vm2, vd, vc, vk):
        assert torch.isfinite(x).all()


def test_abi_and_default():
    from clm_gs_amd import _lib, utils
    src = open(os.path.join(ROOT, "include", "clmgs.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for name in NEW_SYMBOLS:
        assert re.search(r"\b" + name + r"\s*\(", src), name
        assert name in _lib.SIGNATURES, name
    fwd, bwd = _lib.SIGNATURES["clmgs_preprocess_fwd"], _lib.SIGNATURES["clmgs_preprocess_bwd"]
    assert _lib.SIGNATURES["clmgs_preprocess_aa_fwd"] == fwd and _lib.SIGNATURES["clmgs_preprocess_aa_bwd"] == bwd
    assert _lib.SIGNATURES["clmgs_preprocess_aa_abs_bwd"] == _lib.SIGNATURES["clmgs_preprocess_abs_bwd"]
    l = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert hasattr(l, name), name
    assert utils.default_args().rasterize_mode == "classic"
    utils.set_args(utils.default_args(rasterize_mode="bogus"))
    with pytest.raises(ValueError):
        utils.antialiased()
    utils.set_args(utils.default_args(rasterize_mode="antialiased"))
    assert utils.antialiased()
    utils.set_args(utils.default_args())
    assert not utils.antialiased()
