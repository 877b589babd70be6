"""-m gpu: bilateral-grid colour correction ("Bilateral grid"): the kernels of csrc/bilagrid.hip on
their own, through clm_kernels.apply_bilagrid, through the engines and through the trainer, against the float64
restatement in tests/bilagrid_reference.py."""
import ctypes
import functools
import os

import numpy as np
import pytest
import torch

from tests import bilagrid_reference as R
from tests import masked_loss_reference as M
from tests import test_gpu_engines as GE
from tests import test_gpu_exposure as EX
from tests import test_gpu_invdepth as ID
from tests import test_gpu_masked_loss as ML
from tests.scenes import rel_l2

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
SENT = 123.25
# 1 pixel (W = 1); fewer pixels than cells; cells with no pixel under (16,16,8); several workgroups per cell under (2,2,2)
SHAPES = [(1, 1), (5, 7), (13, 67), (70, 130)]
GRIDS = [(2, 2, 2), (5, 3, 4), (16, 16, 8)]  # (Wg, Hg, L)
LAYOUTS = ["hwc3", "hwc4", "chw"]  # the engine's interleaved buffer | its [H,W,4] buffer of a camera with a depth prior | planar
# csrc/bilagrid.hip: BG_P (a lane's fused multiply-adds), the DPP steps of wave_sum, the add into the wave's LDS block,
# BG_WAVES, and per node at most 4 cells x the slab rows of a cell in clmgs_bilagrid_grad_finish, plus its add into grad
LANE_PIXELS, WAVE_STEPS, WAVES = 4, 6, 4


def _chain(rows, Wg, Hg):
    chunks = rows // ((Wg - 1) * (Hg - 1))
    return LANE_PIXELS + WAVE_STEPS + 1 + WAVES + 4 * chunks + 1


def _p(t):
    return ctypes.c_void_p(t.data_ptr())


def _alloc(layout, h, w, dev, fill=None):
    """-> (a [3,H,W] float32 view on the device in the given memory layout, NaN where nothing is copied in; its buffer)"""
    if layout == "chw":
        buf = torch.full((3, h, w), float("nan"), device=dev)
        t = buf
    elif layout == "hwc3":
        buf = torch.full((h, w, 3), float("nan"), device=dev)
        t = buf.permute(2, 0, 1)
    else:
        buf = torch.full((h, w, 4), float("nan"), device=dev)
        buf[..., 3] = SENT
        t = buf[..., :3].permute(2, 0, 1)
        assert t.stride() == (1, 4 * w, 4)
    if fill is not None:
        t.copy_(fill.to(dev))
    return t, buf


def _fourth_word_untouched(layout, buf):
    return layout != "hwc4" or bool((buf[..., 3] == SENT).all())


def _raw_fwd(x, G, y):
    from clm_gs_amd import _lib
    _, h, w = x.shape
    _lib.check(_lib.lib().clmgs_bilagrid_fwd(_lib.stream(), h, w, _p(x), *x.stride(), _p(G), *G.shape[:3], _p(y), *y.stride()))


def _raw_bwd(x, G, g, v):
    """-> the slab [rows, L * 48], every row written by the kernel (NaN before)."""
    from clm_gs_amd import _lib
    L = _lib.lib()
    _, h, w = x.shape
    Lz, Hg, Wg = G.shape[:3]
    rows = int(L.clmgs_bilagrid_partials_rows(h, w, Hg, Wg))
    partials = torch.full((rows, Lz * 48), float("nan"), device=x.device)
    _lib.check(L.clmgs_bilagrid_bwd(_lib.stream(), h, w, _p(x), *x.stride(), _p(G), Lz, Hg, Wg, _p(g), *g.stride(), _p(v),
                                    *v.stride(), _p(partials)))
    return partials


def _raw_finish(h, w, partials, grad):
    from clm_gs_amd import _lib
    Lz, Hg, Wg = grad.shape[:3]
    _lib.check(_lib.lib().clmgs_bilagrid_grad_finish(_lib.stream(), h, w, Lz, Hg, Wg, _p(partials), _p(grad)))


def _colours(h, w, L, gen):
    """Colours in [-0.3, 1.3] (both clamped sides occur in all but the smallest image), re-drawn until every pixel's
    s (L - 1) is at least 1e-3 from every integer and s at least 1e-3 from 0 and 1: the guidance gradient is discontinuous
    there and float32 and float64 may take different sides.  No pixel is excluded from any comparison."""
    x = torch.rand(3, h, w, generator=gen) * 1.6 - 0.3
    for _ in range(100):
        s = R.luminance(x.double())
        fz = s * (L - 1)
        bad = ((fz - fz.round()).abs() < 1e-3) | (s.abs() < 1e-3) | ((s - 1).abs() < 1e-3)
        if not bool(bad.any()):
            return x
        fresh = torch.rand(3, h, w, generator=gen) * 1.6 - 0.3
        x = torch.where(bad[None], fresh, x)
    raise AssertionError("no admissible colours")


@functools.lru_cache(maxsize=None)
def _case(h, w, grid):
    """Inputs and the float64 reference, computed once per (shape, grid) and shared by the layouts and tests."""
    Wg, Hg, L = grid
    gen = torch.Generator().manual_seed(1000 * h + 10 * w + L)
    x = _colours(h, w, L, gen)
    g = torch.randn(3, h, w, generator=gen) * 1e-3
    G = torch.randn(L, Hg, Wg, 12, generator=gen)
    xd, gd, Gd = x.double(), g.double(), G.double()
    y0 = R.apply(xd, Gd).detach()
    v0, dG0 = R.vjp(xd, Gd, gd)
    return x, g, G, y0, v0, dG0


@functools.lru_cache(maxsize=None)
def _bounds(h, w, grid, chain):
    x, g, G, *_ = _case(h, w, grid)
    return R.bounds(x.double(), G.double(), g.double(), chain)


def _worst(err, bound):
    """Largest error / bound over the elements with a non-zero bound; an element whose bound is zero must be exact."""
    nz = bound > 0
    assert bool((err[~nz] == 0).all())
    return float((err[nz] / bound[nz]).max()) if bool(nz.any()) else 0.0


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("grid", GRIDS, ids=lambda g: "x".join(map(str, g)))
@pytest.mark.parametrize("hw", SHAPES)
def test_forward_against_float64(dev, hw, grid, layout):
    h, w = hw
    x, _, G, y0, *_ = _case(h, w, grid)
    b_y = _bounds(h, w, grid, 0)[0]
    (xv, _), (yv, ybuf) = _alloc(layout, h, w, dev, x), _alloc(layout, h, w, dev)
    _raw_fwd(xv, G.to(dev), yv)
    y = yv.cpu().double()
    assert bool(torch.isfinite(y).all()), "every element of y must be written"
    assert _fourth_word_untouched(layout, ybuf)
    worst = _worst((y - y0).abs(), b_y)
    print(f"bilagrid fwd {hw} {grid} {layout}: largest error / bound {worst:.3f}")
    assert worst <= 1.0


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("grid", GRIDS, ids=lambda g: "x".join(map(str, g)))
@pytest.mark.parametrize("hw", SHAPES)
def test_identity_is_exact(dev, hw, grid, layout):
    h, w = hw
    Wg, Hg, L = grid
    x, g, *_ = _case(h, w, grid)
    G = R.identity(L, Hg, Wg, torch.float32).to(dev)
    (xv, _), (yv, _), (gv, _), (vv, _) = (_alloc(layout, h, w, dev, x), _alloc(layout, h, w, dev),
                                          _alloc(layout, h, w, dev, g), _alloc(layout, h, w, dev))
    _raw_fwd(xv, G, yv)
    assert torch.equal(yv, xv)
    _raw_bwd(xv, G, gv, vv)
    assert torch.equal(vv, gv)


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("grid", GRIDS, ids=lambda g: "x".join(map(str, g)))
@pytest.mark.parametrize("hw", SHAPES)
def test_backward_against_float64(dev, hw, grid, layout):
    from clm_gs_amd import _lib
    h, w = hw
    Wg, Hg, L = grid
    x, g, G, _, v0, dG0 = _case(h, w, grid)
    rows = int(_lib.lib().clmgs_bilagrid_partials_rows(h, w, Hg, Wg))
    assert rows >= (Wg - 1) * (Hg - 1) and rows % ((Wg - 1) * (Hg - 1)) == 0
    n = _chain(rows, Wg, Hg)
    if (hw, grid) == ((70, 130), (2, 2, 2)):
        assert rows >= 2, "several workgroups per cell"
    _, b_v, b_G = _bounds(h, w, grid, n)
    Gd = G.to(dev)
    (xv, _), (gv, _), (vv, vbuf) = _alloc(layout, h, w, dev, x), _alloc(layout, h, w, dev, g), _alloc(layout, h, w, dev)
    partials = _raw_bwd(xv, Gd, gv, vv)
    assert bool(torch.isfinite(partials).all()), "every slab row must be written"
    dG = torch.zeros(L, Hg, Wg, 12, device=dev)
    _raw_finish(h, w, partials, dG)
    v, dG_h = vv.cpu().double(), dG.cpu().double()
    assert bool(torch.isfinite(v).all()), "every element of v_x must be written"
    assert _fourth_word_untouched(layout, vbuf)
    w_v, w_G = _worst((v - v0).abs(), b_v), _worst((dG_h - dG0).abs(), b_G)
    print(f"bilagrid bwd {hw} {grid} {layout}: {rows} rows, n = {n}; v_x error / bound {w_v:.3f}, dG error / bound {w_G:.4f}")
    assert w_v <= 1.0
    assert w_G <= 1.0
    # in place (v_x is g) gives the same bits as out of place
    g2, g2buf = _alloc(layout, h, w, dev, g)
    p2 = _raw_bwd(xv, Gd, g2, g2)
    assert torch.equal(g2, vv) and torch.equal(p2, partials) and _fourth_word_untouched(layout, g2buf)
    # a second run gives the same bits: slab, total and v_x
    v3, _ = _alloc(layout, h, w, dev)
    p3 = _raw_bwd(xv, Gd, gv, v3)
    dG3 = torch.zeros_like(dG)
    _raw_finish(h, w, p3, dG3)
    assert torch.equal(p3, partials) and torch.equal(dG3, dG) and torch.equal(v3, vv)
    # grad_finish ADDS: twice, onto a grid that is not zero
    start = torch.randn(L, Hg, Wg, 12, generator=torch.Generator().manual_seed(4)) * float(dG0.abs().max())
    acc = start.to(dev)
    _raw_finish(h, w, partials, acc)
    _raw_finish(h, w, partials, acc)
    want = start.double() + 2 * dG0
    b_add = 2 * b_G + 2 * U * (start.double().abs() + 2 * dG0.abs())  # + the two roundings of the adds themselves
    assert bool(((acc.cpu().double() - want).abs() <= b_add).all())


@pytest.mark.parametrize("grid", GRIDS, ids=lambda g: "x".join(map(str, g)))
def test_guidance_term_in_isolation(dev, grid):
    """Every column sum over c of A[c][k], k < 3, made zero at every node and the cotangent equal in the three channels: the
    first term of dL/dx, sum_c A[c][k] g[c], vanishes and what is left is the gradient through the luminance alone (carried by
    the bias column A[c][3], whose sums are left as drawn)."""
    h, w = 13, 67
    Wg, Hg, L = grid
    x = _case(h, w, grid)[0]
    gen = torch.Generator().manual_seed(77)
    G = torch.randn(L, Hg, Wg, 3, 4, generator=gen).double()
    G[..., :3] -= G[..., :3].mean(dim=3, keepdim=True)
    G = G.float()  # rounded to float32: the sums are zero to rounding, the reference sees the same
    G = G.reshape(L, Hg, Wg, 12)
    g = (torch.randn(1, h, w, generator=gen) * 1e-3).expand(3, h, w).contiguous()
    v0, _ = R.vjp(x.double(), G.double(), g.double())
    P = R.parts(x.double(), G.double())
    first = torch.einsum("hwck,chw->khw", P["A"].reshape(h, w, 3, 4)[..., :3], g.double())
    assert float(first.abs().max()) < 1e-6 * float(v0.abs().max()), "the first term is gone"
    assert float(v0[:, P["inside"]].abs().min()) > 0 and not bool(v0[:, ~P["inside"]].abs().gt(1e-9).any())
    b_v = R.bounds(x.double(), G.double(), g.double(), 0)[1]
    (xv, _), (gv, _), (vv, _) = _alloc("hwc3", h, w, dev, x), _alloc("hwc3", h, w, dev, g), _alloc("hwc3", h, w, dev)
    _raw_bwd(xv, G.to(dev), gv, vv)
    v = vv.cpu().double()
    worst = _worst((v - v0).abs(), b_v)
    share = float((v - v0).abs().max() / v0.abs().max())
    print(f"bilagrid guidance term {grid}: error / bound {worst:.3f}, largest error / largest value {share:.3g}")
    assert worst <= 1.0
    assert share < 1e-4, "a missing guidance term reads 1"


def test_slab_rows(dev):
    """The row count every layout writes: cells x the chunks that cover the largest cell."""
    from clm_gs_amd import _lib
    L = _lib.lib()
    assert int(L.clmgs_bilagrid_partials_rows(1, 1, 2, 2)) == 1
    assert int(L.clmgs_bilagrid_partials_rows(3456, 4608, 16, 16)) == 225 * 71  # 24.5 MB at L = 8
    for bad in ((0, 5, 2, 2), (5, 0, 2, 2), (5, 5, 1, 2), (5, 5, 2, 65)):
        assert int(L.clmgs_bilagrid_partials_rows(*bad)) == 0


def test_entries_reject_bad_arguments(dev):
    from clm_gs_amd import _lib
    L = _lib.lib()
    x, _ = _alloc("hwc3", 4, 4, dev, torch.zeros(3, 4, 4))
    y, _ = _alloc("hwc3", 4, 4, dev)
    G = R.identity(2, 2, 2, torch.float32).to(dev)
    with pytest.raises(_lib.ClmgsError):
        _raw_fwd(x, G, x)  # the forward is not in place
    with pytest.raises(_lib.ClmgsError):
        _raw_bwd(x, G, x, x)  # v_x must not be x
    g, _ = _alloc("chw", 4, 4, dev, torch.zeros(3, 4, 4))
    slab = torch.empty(64, 32 * 48, device=dev)
    with pytest.raises(_lib.ClmgsError):  # in place only as the same view
        _lib.check(L.clmgs_bilagrid_bwd(_lib.stream(), 4, 4, _p(x), *x.stride(), _p(G), 2, 2, 2, _p(g), *g.stride(), _p(g),
                                        1, 12, 3, _p(slab)))
    big = torch.zeros(33 * 65 * 65 * 12, device=dev)
    # the out-of-range shapes, (L, Hg, Wg): refused by every entry that takes them
    for Lz, Hg, Wg in ((1, 2, 2), (33, 2, 2), (2, 1, 2), (2, 65, 2), (2, 2, 1), (2, 2, 65)):
        with pytest.raises(_lib.ClmgsError):
            _lib.check(L.clmgs_bilagrid_fwd(_lib.stream(), 4, 4, _p(x), *x.stride(), _p(big), Lz, Hg, Wg, _p(y), *y.stride()))
        with pytest.raises(_lib.ClmgsError):
            _lib.check(L.clmgs_bilagrid_bwd(_lib.stream(), 4, 4, _p(x), *x.stride(), _p(big), Lz, Hg, Wg, _p(g), *g.stride(),
                                            _p(y), *y.stride(), _p(slab)))
        with pytest.raises(_lib.ClmgsError):
            _lib.check(L.clmgs_bilagrid_grad_finish(_lib.stream(), 4, 4, Lz, Hg, Wg, _p(slab), _p(big)))
        with pytest.raises(_lib.ClmgsError):
            _lib.check(L.clmgs_bilagrid_tv_grad(_lib.stream(), _p(big), 1, Lz, Hg, Wg, 1.0, _p(slab)))
    torch.cuda.synchronize()


@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("grid", [(2, 2, 2), (5, 3, 4), (16, 16, 8)], ids=lambda g: "x".join(map(str, g)))
def test_tv_grad_against_float64(dev, grid, n):
    """Per element and axis a = (G - G_prev) - (G_next - G): three subtractions, |error| <= 2 U m with m = 2 |G| + |G_prev| +
    |G_next| (absent neighbours left out); the coefficient c_axis is a rounded float (U), the three axes are joined by fused
    multiply-adds (3 roundings): 6 U sum_axis c_axis m_axis; and the add into the gradient table: U |result|."""
    from clm_gs_amd import _lib
    Wg, Hg, L = grid
    weight = 10.0
    gen = torch.Generator().manual_seed(12 + n)
    T = torch.randn(n, L, Hg, Wg, 12, generator=gen)
    start = torch.randn(n, L, Hg, Wg, 12, generator=gen) * 0.1
    want = start.double() + R.tv_grad(T.double(), weight)
    Ta = T.double().abs()
    mag = torch.zeros_like(Ta)
    for dim, count in ((1, 12 * (L - 1) * Hg * Wg), (2, 12 * L * (Hg - 1) * Wg), (3, 12 * L * Hg * (Wg - 1))):
        c, k = 2.0 * weight / (n * count), Ta.shape[dim] - 1
        pair = Ta.narrow(dim, 1, k) + Ta.narrow(dim, 0, k)  # |G| + |neighbour| of every difference
        mag.narrow(dim, 1, k).add_(pair, alpha=c)
        mag.narrow(dim, 0, k).add_(pair, alpha=c)
    bound = U * (6 * mag + want.abs())
    Td, grad = T.to(dev), start.to(dev)
    _lib.check(_lib.lib().clmgs_bilagrid_tv_grad(_lib.stream(), _p(Td), n, L, Hg, Wg, weight, _p(grad)))
    err = (grad.cpu().double() - want).abs()
    worst = _worst(err, bound)
    moved = float((grad.cpu() - start).abs().max())
    print(f"bilagrid tv_grad {grid} n={n}: error / bound {worst:.3f}, largest |gradient| {moved:.3g}")
    assert moved > 0 and worst <= 1.0
    # the model's step reaches the same kernel
    from clm_gs_amd.bilagrid import BilagridModel
    m = BilagridModel(n, dev, grid=grid, tv_weight=weight)
    with torch.no_grad():
        m.param.copy_(Td)
        m.grad.copy_(start)
    m.tv_grad()
    assert torch.equal(m.grad, grad)
    assert abs(float(m.tv()) - float(R.tv(T.double()))) < 1e-5 * float(R.tv(T.double()))


# ------------------------------------------------------------------------------------------ operator
@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("layout", ["chw", "hwc_view"])
@pytest.mark.parametrize("hw", [(13, 67), (70, 130)])
def test_apply_bilagrid_then_loss_matches_autograd_of_the_restatement(dev, hw, layout, masked):
    from clm_gs_amd import clm_kernels as K
    h, w = hw
    img, gt, mask, _, _ = ML._case(h, w, "bernoulli")
    if not masked:
        mask = None
    G = R.identity(4, 3, 5, torch.float32) + 0.2 * torch.randn(4, 3, 5, 12, generator=torch.Generator().manual_seed(9))
    xr, Gr = img.double().requires_grad_(), G.double().requires_grad_()
    l0 = R.loss(xr, Gr, gt, mask, 0.2)
    l0.backward()
    if layout == "chw":
        leaf = img.to(dev).requires_grad_()
        view = leaf
    else:
        leaf = img.permute(1, 2, 0).contiguous().to(dev).requires_grad_()
        view = leaf.permute(2, 0, 1)
    Gl = G.to(dev).requires_grad_()
    y = K.apply_bilagrid(view, Gl)
    assert y.stride() == view.stride() and y.shape == view.shape
    if mask is None:
        l = K.fused_l1_ssim_loss(y, gt.to(dev), 0.2)
    else:
        l = K.fused_l1_ssim_loss(y, gt.to(dev), 0.2, mask=mask.to(dev), mask_count=int((mask != 0).sum()))
    l.backward()
    gi = leaf.grad.cpu() if layout == "chw" else leaf.grad.permute(2, 0, 1).cpu()
    e_l, e_i, e_G = abs(l.item() - l0.item()), rel_l2(gi, xr.grad), rel_l2(Gl.grad.cpu(), Gr.grad)
    print(f"apply_bilagrid + loss {hw} {layout} masked={masked}: loss error {e_l:.3g}, image gradient rel_l2 {e_i:.3g}, "
          f"grid gradient rel_l2 {e_G:.3g}")
    assert e_l < 1e-5
    assert e_i < 1e-4
    assert e_G < 1e-4


def test_apply_camera_bilagrid(dev):
    """The engines' and the evaluation's entry: the camera's grid, its gradient ADDED to the camera's gradient grid; the image
    itself for a camera without a grid; a camera with an exposure row as well is refused."""
    from clm_gs_amd import clm_kernels as K
    from clm_gs_amd.bilagrid import BilagridModel

    class Cam:
        image_name = "a"
    cam, img = Cam(), torch.rand(3, 6, 10, device=dev)
    assert K.apply_camera_colour(img, cam) is img
    m = BilagridModel(1, dev, grid=(3, 2, 2))
    m.attach([cam])
    with torch.no_grad():
        m.param[0, ..., 3] = 0.25  # A[0][3] at every node: red + 0.25
        m.grad[0] += 1.0
    leaf = img.clone().requires_grad_()
    y = K.apply_camera_colour(leaf, cam)
    assert torch.equal(y.detach()[0], img[0] + 0.25) and torch.equal(y.detach()[1:], img[1:])
    y.sum().backward()
    # the gradient of sum(y) over all nodes: per coefficient 4c + k, sum_p x_k (x_3 = 1), on top of the 1 that was there
    got = (m.grad[0] - 1.0).sum(dim=(0, 1, 2)).cpu()
    want = torch.cat([img.sum(dim=(1, 2)).cpu(), torch.tensor([60.0])]).repeat(3)
    assert rel_l2(got, want) < 1e-5 and torch.equal(leaf.grad, torch.ones_like(img))
    with torch.no_grad():  # evaluation: no tape, nothing added
        before = m.grad.clone()
        y2 = K.apply_camera_colour(img, cam)
    assert torch.equal(y2, y.detach()) and torch.equal(m.grad, before)
    cam.exposure = torch.eye(3, 4, device=dev)
    with pytest.raises(ValueError, match="both an exposure row and a bilateral grid"):
        K.apply_camera_colour(img, cam)


# ------------------------------------------------------------------------------------------- engines
W, H, N, BSZ = ML.W, ML.H, ML.N, ML.BSZ
GRID = (5, 3, 4)  # (Wg, Hg, L) of the engine tests
NO_GRID = 3       # this camera of the batch carries none: its gradient grid stays zero
MASKED = 1        # this one a loss mask as well
PRIOR = 0         # and this one an inverse-depth prior (the [H,W,4] buffer)


def _grids():
    Wg, Hg, L = GRID
    gen = torch.Generator().manual_seed(41)
    return R.identity(L, Hg, Wg, torch.float32).repeat(BSZ, 1, 1, 1, 1) + 0.1 * torch.randn(BSZ, L, Hg, Wg, 12, generator=gen)


def _attach(cams, dev="cuda"):
    from clm_gs_amd.bilagrid import BilagridModel
    model = BilagridModel(BSZ, dev, grid=GRID)
    with torch.no_grad():
        model.param.copy_(_grids())
    model.attach(cams)
    cams[NO_GRID].bilagrid, cams[NO_GRID].bilagrid_grad = None, None
    mask = ML._camera_masks()[0]
    cams[MASKED].loss_mask, cams[MASKED].loss_mask_count = mask.cuda(), int((mask != 0).sum())
    raw, scale, offset = ID._float64_batch()[2][PRIOR]
    cams[PRIOR].invdepth, cams[PRIOR].invdepth_scale, cams[PRIOR].invdepth_offset = raw.cuda(), scale, offset
    return model


_RUNS = {}


def _batch(strategy, residency="hbm", fused=True):
    """tests/test_gpu_exposure.py's _batch with grids (and the mask and the prior) on the cameras -> losses by camera, model
    gradients and the grid gradient table, on the CPU."""
    key = (strategy, residency, fused)
    if key in _RUNS:
        return _RUNS[key]
    ID._float64_batch()  # (sets the process-wide args itself: before this batch's own)
    args, sc, cams = ML._setup(strategy, residency, "none", fused, debug_skip_optimizer=True,
                               stop_update_param=strategy == "naive_offload")
    model = _attach(cams)
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
                               "shs": gsh.detach().cpu().reshape(N, 48).clone()},
             grid_grad=model.grad.detach().cpu().clone(), grids=model.param.detach().cpu().clone())
    _RUNS[key] = r
    return r


@functools.lru_cache(maxsize=None)
def _float64_batch():
    """The oracle's float64 render of every camera, the restated slice, the restated (masked) loss and the depth term."""
    from clm_gs_amd import utils
    pri = ID._float64_batch()[2][PRIOR]
    _, sc, cams = ML._setup("no_offload", masks="none")
    weight = utils.depth_l1_weight()
    P = {k: sc[k].detach().cpu().double().requires_grad_() for k in ("xyz", "opacity", "scaling", "rotation", "shs48")}
    Gs = [g.double().requires_grad_() for g in _grids()]
    losses = []
    for i, c in enumerate(cams):
        img, inv = ID._render64(P, c)
        if i != NO_GRID:
            img = R.apply(img, Gs[i])
        mask = ML._camera_masks()[0] if i == MASKED else None
        l = M.masked_loss(img, c.original_image.cpu(), mask, 0.2)
        if i == PRIOR:
            l = l + ID.R.depth_term(inv, *pri, weight, mask)
        l.backward()
        losses.append(l.item())
    grads = {"xyz": P["xyz"].grad, "opacity": P["opacity"].grad.reshape(N, -1), "scaling": P["scaling"].grad,
             "rotation": P["rotation"].grad, "shs": P["shs48"].grad.reshape(N, 48)}
    dG = torch.stack([g.grad if g.grad is not None else torch.zeros_like(g) for g in Gs])
    return losses, grads, dG


@pytest.mark.parametrize("mode", EX.ENGINE_MODES, ids=lambda m: f"{m[0]}-{m[1]}-{'fused' if m[2] else 'op_by_op'}")
def test_engines_with_grids_match_the_float64_composition(dev, mode):
    want_l, want_g, want_G = _float64_batch()
    b = _batch(*mode)
    assert torch.equal(b["grids"], _grids()), "a batch without an optimizer step leaves the table alone"
    for i, (u, v) in enumerate(zip(b["losses"], want_l)):
        print(f"{mode} camera {i}: loss {u:.7f} vs {v:.7f}")
        assert abs(u - v) < 2e-5, (mode, i)
    for k in b["grads"]:
        e = rel_l2(b["grads"][k], want_g[k])
        print(f"{mode}: {k} gradient rel_l2 {e:.3g}")
        assert e < 1e-3, (mode, k, e)
    for i in range(BSZ):
        if i == NO_GRID:  # no trace in the table
            assert not bool(b["grid_grad"][i].any()) and not bool(want_G[i].any())
            continue
        e = rel_l2(b["grid_grad"][i], want_G[i])
        print(f"{mode} camera {i}: grid gradient rel_l2 {e:.3g}")
        assert e < 1e-3, (mode, i, e)


def test_grids_change_the_loss_and_nothing_in_front_of_it(dev):
    """Against the plain batch of tests/test_gpu_masked_loss.py: the camera that carries nothing sees the same loss, a camera
    with a grid another; and the op-by-op and fused engines agree on the gradient table."""
    a, b = _batch("clm_offload"), ML._batch("clm_offload", masks="none")
    assert a["losses"][NO_GRID] == b["losses"][NO_GRID]
    assert abs(a["losses"][2] - b["losses"][2]) > 1e-6
    e = rel_l2(_batch("clm_offload", fused=True)["grid_grad"], _batch("clm_offload", fused=False)["grid_grad"])
    assert e < 1e-4, e


def _model_for(lr=None):
    def attach(cams):
        from clm_gs_amd.bilagrid import BilagridModel
        if lr is None:
            model = BilagridModel(GE.BSZ, "cuda", grid=GRID)
            gen = torch.Generator().manual_seed(43)
            with torch.no_grad():
                model.param.add_((0.1 * torch.randn(model.param.shape, generator=gen)).cuda())
        else:
            model = BilagridModel(GE.BSZ, "cuda", lr_init=lr, lr_final=lr, max_steps=100)
            model.step_in_test = True
        model.attach(cams)
        return model
    return attach


def test_capacity_redo_adds_the_grid_gradient_once(dev):
    """A forward repeated for capacity (isect_capacity_margin 0.5: every camera of the second batch is found over capacity
    and redone exactly) adds the gradient of the exact forward, once: the table, accumulated over both batches, has the bits
    of the exact-size run."""
    _, t_exact, m_exact, redo_exact = EX._two_batches(_model_for(), dict(device_side_counts=False))
    _, t_over, m_over, redo_over = EX._two_batches(_model_for(), dict(device_side_counts=True, isect_capacity_margin=0.5,
                                                                      isect_capacity_floor=0))
    assert redo_exact == 0 and redo_over >= GE.BSZ, (redo_exact, redo_over)
    assert bool(m_exact.grad.any())
    assert torch.equal(m_over.grad, m_exact.grad)
    for a, b in zip(t_over, t_exact):
        assert torch.equal(a, b)


def test_identity_grids_at_zero_learning_rate_train_the_same_model(dev):
    """Off means off: identity grids (16, 16, 8), stepped at learning rate 0 after each of two batches.  The slice and its
    VJP are exact at the identity, so every model tensor ends with the values of the run without grids."""
    l_plain, t_plain, _, _ = EX._two_batches(None)
    l_grid, t_grid, model, _ = EX._two_batches(_model_for(lr=0.0))
    assert l_grid == l_plain
    assert torch.equal(model.param.detach(), R.identity(8, 16, 16, torch.float32).cuda().expand(GE.BSZ, 8, 16, 16, 12))
    for name, a, b in zip(("xyz", "opacity", "scaling", "rotation", "shs"), t_grid, t_plain):
        assert torch.equal(a, b), name


# ------------------------------------------------------------------------------------------- trainer
def test_trainer_with_bilagrid(dev, tmp_path):
    from clm_gs_amd import trainer
    from clm_gs_amd.bilagrid import BilagridModel
    from clm_gs_amd.cameras import camera_bilagrid
    work = EX._tiny_scene(tmp_path)
    out = tmp_path / "out"
    gaussians, scene, _ = trainer.train_from_colmap(
        str(work), str(out), strategy="clm_offload", iterations=8, test_iterations=(5,), bsz=4, eval=True,
        disable_auto_densification=True, bilagrid=True, bilagrid_shape=(6, 4, 3))
    assert scene.test_cameras and all(camera_bilagrid(c) == (None, None) for c in scene.test_cameras)
    assert all(camera_bilagrid(c)[0] is not None for c in scene.train_cameras)
    with np.load(out / "bilagrid.npz") as f:
        grids, names = f["grids"], [str(s) for s in f["image_names"]]
    assert names == [c.image_name for c in scene.train_cameras] and grids.shape == (len(names), 12, 3, 4, 6)
    log = open(out / "python_ws=1_rk=0.log").read()
    # two batches of 4 out of 10 training cameras: the grids of the 8 cameras the loss lines name have moved; a grid whose
    # camera was never drawn has zero gradients (its total-variation gradient is zero at the identity) and zero moments,
    # which dense Adam does not move -- it is still the identity, exactly
    import re
    trained = set(re.findall(r"'([^']+)'", " ".join(re.findall(r" image: \[(.*?)\]", log))))
    assert len(trained) == 8 and trained <= set(names)
    eye = R.identity(3, 4, 6, torch.float32).permute(3, 0, 1, 2).numpy()
    moved = {k: float(np.abs(g - eye).max()) for k, g in zip(names, grids)}
    print("bilagrid.npz after 8 images: max |G - I| per camera", {k: round(v, 7) for k, v in moved.items()})
    for k, v in moved.items():
        assert (v > 1e-6) if k in trained else (v == 0.0), (k, v)
    fresh = BilagridModel(len(scene.train_cameras), "cuda", grid=(6, 4, 3))
    fresh.load(str(out / "bilagrid.npz"), scene.train_cameras)
    assert torch.equal(fresh.param.detach(), scene.bilagrid.param.detach())
    assert "Evaluating train:" in log and "Evaluating test:" in log and "end2end total_time:" in log
    assert os.path.exists(out / "point_cloud" / "iteration_8" / "point_cloud.ply")
    # without the flag: no table, no file
    out2 = tmp_path / "out2"
    _, scene2, _ = trainer.train_from_colmap(str(work), str(out2), strategy="clm_offload", iterations=8, bsz=4,
                                             disable_auto_densification=True)
    assert scene2.bilagrid is None and not os.path.exists(out2 / "bilagrid.npz")
    assert all(camera_bilagrid(c) == (None, None) for c in scene2.train_cameras)
