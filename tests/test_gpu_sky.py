"""-m gpu: the learnable sky ("Sky"): the kernels of csrc/sky.hip on their own, through
clm_kernels.apply_sky, through the rasterizer, the engines and the trainer, against the float64 restatement in
tests/sky_reference.py."""
import ctypes
import functools
import math
import os

import numpy as np
import pytest
import torch

from oracle import gs_oracle as O
from tests import exposure_reference as XR
from tests import masked_loss_reference as M
from tests import sky_reference as R
from tests import test_gpu_engines as GE
from tests import test_gpu_exposure as GX
from tests import test_gpu_masked_loss as ML
from tests.scenes import rel_l2

pytestmark = pytest.mark.gpu

U = 2.0 ** -24      # unit roundoff of float32
UNIT = 2.0 ** -48   # the accumulator's unit
# The texel weights go through the device's atan2f / asinf, whose accuracy is the library's: what depends on them is
# bounded with the project's operator tolerance (tests/test_gpu_exposure.py: 1e-4), per unit of what multiplies the sample.
TOL_S = 1e-4
SHAPES = [(1, 1), (5, 7), (13, 67), (70, 130)]
LAYOUTS = GX.LAYOUTS  # interleaved | planar | interleaved with the base moved by one pixel
TILE, WIN_TEXELS = 16, 256  # csrc/sky.hip: SKY_TILE, SKY_WIN_TEXELS


def _K(w, h, fov, fy_ratio=1.0, dcx=0.0, dcy=0.0):
    """cx, cy multiples of 0.5: pixel coordinates relative to the principal point are formed exactly in float32."""
    return R.intrinsics(w, h, fov, fy_ratio, math.floor(w) / 2.0 + dcx, math.floor(h) / 2.0 + dcy)


# name -> (Hs, Ws, world->camera, (fov_x degrees, fy / fx, principal point offset)); what each one exercises
CASES = {
    "one_texel_map": (1, 1, R.look_at_camera((0.3, -0.5, 0.8), roll=0.4), (80.0, 1.0, 0.0, 0.0)),
    # 45-degree texels behind a 3-degree camera: every pixel in one bilinear cell -- the LDS window, maximal contention
    "inside_one_cell": (4, 8, R.look_at_camera((0.05, -0.02, 1.0)), (3.0, 1.0, 0.0, 0.0)),
    "several_texels": (64, 128, R.look_at_camera((0.4, -0.3, 1.0)), (90.0, 1.0, 0.0, 0.0)),
    # a pole inside a tile: its window spans all 128 columns (129 unwrapped) and two rows or more -- over the budget
    "up": (64, 128, R.look_at_camera((0.0, -1.0, 0.0)), (90.0, 1.0, 0.0, 0.0)),
    "down": (64, 128, R.look_at_camera((0.0, 1.0, 0.0)), (90.0, 1.0, 0.0, 0.0)),
    # the u seam crosses the image: the unwrapped columns of a tile on it run from -1 to 127
    "seam": (64, 128, R.look_at_camera((0.0, 0.1, -1.0)), (60.0, 1.0, 0.0, 0.0)),
    "rotated": (32, 64, R.look_at_camera((-0.7, 0.2, 0.5), roll=0.7), (75.0, 1.3, 3.5, -2.0)),
    # texels finer than pixels: the direct path (run at 13x67 only: one size is enough for a path that has no tiling)
    "fine_map": (512, 1024, R.look_at_camera((0.1, -0.2, 1.0)), (120.0, 1.0, 0.0, 0.0)),
    # about one texel per pixel at 130 columns: a 16x16 tile's window is 17x17 or more (direct), an 8-row tile's fits
    "pixel_sized": (256, 512, R.look_at_camera((0.3, 0.2, 1.0)), (90.0, 1.0, 0.0, 0.0)),
}
GRID = [(hw, c) for hw in SHAPES for c in CASES if c not in ("fine_map", "pixel_sized")] + [((13, 67), "fine_map")]


def _p(t):
    return ctypes.c_void_p(t.data_ptr())


def _host(m, n):
    a = np.ascontiguousarray(m.numpy().astype(np.float32).reshape(-1))
    assert a.size == n
    return a


def _raw_fwd(x, a, vm, K, S, y):
    from clm_gs_amd import _lib
    _, h, w = x.shape
    vmh, Kh = _host(vm, 16), _host(K, 9)
    _lib.check(_lib.lib().clmgs_sky_fwd(_lib.stream(), h, w, _p(x), *x.stride(), _p(a), vmh.ctypes.data_as(ctypes.c_void_p),
                                        Kh.ctypes.data_as(ctypes.c_void_p), _p(S), S.shape[0], S.shape[1], _p(y), *y.stride()))


def _raw_bwd(g, a, vm, K, S, v_a, acc, h=None, w=None):
    from clm_gs_amd import _lib
    if h is None:
        _, h, w = g.shape
    vmh, Kh = _host(vm, 16), _host(K, 9)
    _lib.check(_lib.lib().clmgs_sky_bwd(_lib.stream(), h, w, _p(g), *g.stride(), _p(a), vmh.ctypes.data_as(ctypes.c_void_p),
                                        Kh.ctypes.data_as(ctypes.c_void_p), _p(S), S.shape[0], S.shape[1], _p(v_a), _p(acc)))


def _f32(t):
    """A float64 matrix as the kernels see it (float32), back in float64: the reference is stated on the same camera."""
    return t.float().double()


@functools.lru_cache(maxsize=None)
def _case(h, w, name):
    """Inputs and the float64 reference, computed once per (shape, case) and shared by the layouts and tests."""
    Hs, Ws, vm, (fov, ratio, dcx, dcy) = CASES[name]
    vm, K = _f32(vm), _f32(_K(w, h, fov, ratio, dcx, dcy))
    gen = torch.Generator().manual_seed(1000 * h + w + len(name))
    x = torch.rand(3, h, w, generator=gen) * 1.2 - 0.1
    a = torch.rand(h, w, generator=gen)
    a[torch.rand(h, w, generator=gen) < 0.15] = 1.0  # opaque pixels add nothing
    a[torch.rand(h, w, generator=gen) < 0.15] = 0.0  # pure sky
    g = torch.randn(3, h, w, generator=gen)          # O(1) cotangents
    S = torch.rand(Hs, Ws, 3, generator=gen)
    xd, ad, gd, Sd = x.double(), a.double(), g.double(), S.double()
    y0 = R.apply(xd, ad, Sd, vm, K)
    v_a0, v_S0 = R.vjp(ad, Sd, vm, K, gd)
    rows, cols, _ = R.taps(vm, K, h, w, Hs, Ws)
    # per texel and channel: sum over the pixels that touch it of (1 - alpha) |g[c]| -- what an error of a weight scales with
    mass = torch.zeros(Hs * Ws, 3, dtype=torch.float64)
    add = ((1 - ad)[..., None] * gd.abs().permute(1, 2, 0))[:, :, None, :].expand(h, w, 4, 3)
    mass.index_add_(0, (rows * Ws + cols).reshape(-1), add.reshape(-1, 3))
    return dict(x=x, a=a, g=g, S=S, vm=vm, K=K, y0=y0, v_a0=v_a0, v_S0=v_S0, mass=mass.reshape(Hs, Ws, 3))


def _paths(vm, K, h, w, Hs, Ws, y0=0, rows_=None):
    """(tiles through the LDS window, tiles adding directly) as csrc/sky.hip's window rule decides, predicted from the
    float64 taps for the rows [y0, y0 + rows_) handed over as one call."""
    rows, cols, _ = R.taps(vm, K, h, w, Hs, Ws)
    u, _ = R.coordinates(vm, K, h, w, Hs, Ws)
    iu = torch.floor(u).long()
    rows_ = h - y0 if rows_ is None else rows_
    lds = direct = 0
    _paths.windowed = torch.zeros(h, w, dtype=torch.bool) if y0 == 0 else _paths.windowed  # per pixel, for the caller
    for ty in range(y0, y0 + rows_, TILE):
        for tx in range(0, w, TILE):
            sl = (slice(ty, min(ty + TILE, y0 + rows_)), slice(tx, min(tx + TILE, w)))
            wc = int(iu[sl].max()) + 1 - int(iu[sl].min()) + 1
            wr = int(rows[sl].max()) - int(rows[sl].min()) + 1
            _paths.windowed[sl] = wc * wr <= WIN_TEXELS
            if wc * wr <= WIN_TEXELS:
                lds += 1
            else:
                direct += 1
    return lds, direct


# ------------------------------------------------------------------------------------------ kernels
@pytest.mark.parametrize("hw,name", GRID, ids=lambda v: v if isinstance(v, str) else f"{v[0]}x{v[1]}")
def test_forward_and_backward_against_float64(dev, hw, name):
    h, w = hw
    c = _case(h, w, name)
    Sd, n = c["S"].to(dev), h * w
    lds, direct = _paths(c["vm"], c["K"], h, w, *c["S"].shape[:2])
    ref = None
    for layout in LAYOUTS:
        xv, yv = GX._alloc(layout, h, w, dev, c["x"]), GX._alloc(layout, h, w, dev)
        av = c["a"].to(dev)
        _raw_fwd(xv, av, c["vm"], c["K"], Sd, yv)
        y = yv.cpu().double()
        assert bool(torch.isfinite(y).all()), "every element of y must be written"
        # y = x + (1 - a) s: the sample's tolerance times what multiplies it, plus the blend's two roundings
        b_y = TOL_S * (1 - c["a"].double()) + 2 * U * (c["x"].double().abs() + 1.0)
        e_y = (y - c["y0"]).abs()
        x2 = GX._alloc(layout, h, w, dev, c["x"])
        _raw_fwd(x2, av, c["vm"], c["K"], Sd, x2)  # in place
        assert torch.equal(x2, yv), "in place equals out of place"
        gv = GX._alloc(layout, h, w, dev, c["g"])
        v_a = torch.full((h, w), float("nan"), device=dev)
        acc = torch.zeros(c["S"].shape, dtype=torch.int64, device=dev)
        _raw_bwd(gv, av, c["vm"], c["K"], Sd, v_a, acc)
        va = v_a.cpu().double()
        assert bool(torch.isfinite(va).all()), "every element of v_alphas must be written"
        b_a = (TOL_S + 3 * U) * c["g"].double().abs().sum(dim=0)  # -(g . s): the sample's tolerance per unit of |g|
        e_a = (va - c["v_a0"]).abs()
        dS = acc.cpu().double() * UNIT
        # fixed point: n * 2^-49 at most; three fp32 roundings per addend and the weights' tolerance, per unit of mass
        b_S = n * 2.0 ** -49 + (TOL_S + 5 * U) * c["mass"]
        e_S = (dS - c["v_S0"]).abs()
        r_S = rel_l2(dS, c["v_S0"]) if bool(c["v_S0"].any()) else float(e_S.max())
        if layout == LAYOUTS[0]:
            print(f"sky {hw} {name}: tiles lds/direct {lds}/{direct}; y max error {float(e_y.max()):.3g} (share of bound "
                  f"{float((e_y / b_y).max()):.3f}), v_alphas {float(e_a.max()):.3g} ({float((e_a / b_a.clamp(min=1e-30)).max()):.3f}), "
                  f"map gradient rel_l2 {r_S:.3g}, max abs {float(e_S.max()):.3g} ({float((e_S / b_S).max()):.3f})")
        assert bool((e_y <= b_y).all())
        assert bool((e_a <= b_a).all())
        assert bool((e_S <= b_S).all())
        assert r_S < TOL_S
        # a second run gives the same bits
        v_a2 = torch.empty_like(v_a)
        acc2 = torch.zeros_like(acc)
        _raw_bwd(gv, av, c["vm"], c["K"], Sd, v_a2, acc2)
        assert torch.equal(acc2, acc) and torch.equal(v_a2, v_a)
        # and so does every layout
        if ref is None:
            ref = (yv.contiguous().clone(), v_a, acc)
        else:
            assert torch.equal(yv.contiguous(), ref[0]) and torch.equal(v_a, ref[1]) and torch.equal(acc, ref[2])
    if name == "fine_map":
        assert lds == 0 and direct > 0
    if name == "inside_one_cell":
        assert direct == 0 and lds > 0
    if name in ("up", "down", "seam") and hw == (70, 130):
        assert direct > 0 and lds > 0, "a tile with a pole or the seam adds directly, the others through the window"


@pytest.mark.parametrize("name", ["several_texels", "fine_map", "up"])
def test_opaque_pixels_leave_no_trace(dev, name):
    """alphas == 1 everywhere: y has the bits of x and the accumulator stays all zero."""
    h, w = 13, 67
    c = _case(h, w, name)
    Sd, ones = c["S"].to(dev), torch.ones(h, w, device=dev)
    for layout in LAYOUTS:
        xv, yv = GX._alloc(layout, h, w, dev, c["x"]), GX._alloc(layout, h, w, dev)
        _raw_fwd(xv, ones, c["vm"], c["K"], Sd, yv)
        assert torch.equal(yv, xv)
        acc = torch.zeros(c["S"].shape, dtype=torch.int64, device=dev)
        _raw_bwd(GX._alloc(layout, h, w, dev, c["g"]), ones, c["vm"], c["K"], Sd, torch.empty(h, w, device=dev), acc)
        assert not bool(acc.any())


@pytest.mark.parametrize("split", [32, 24])
@pytest.mark.parametrize("name", ["several_texels", "rotated", "seam", "down", "inside_one_cell", "pixel_sized"])
def test_accumulator_bits_do_not_depend_on_the_order(dev, name, split):
    """The backward of a 70x130 image against the same image handed over as two calls into one accumulator: the top `split`
    rows, then the rest with cy lowered by `split` (cx, cy are multiples of 0.5: the pixel coordinates are formed exactly
    either way).  split 32 keeps the tiles; split 24 moves them (16 + 8 rows, then 16 + 16 + 14 from row 24), so tiles
    change their windows and -- for `pixel_sized`, whose 16-row tiles exceed the window and add directly while the 8-row
    tiles fit -- their path.  The integers agree."""
    h, w = 70, 130
    c = _case(h, w, name)
    Hs, Ws = c["S"].shape[:2]
    Sd, av = c["S"].to(dev), c["a"].to(dev)
    gv = GX._alloc("hwc", h, w, dev, c["g"])
    whole, va = torch.zeros(c["S"].shape, dtype=torch.int64, device=dev), torch.empty(h, w, device=dev)
    _raw_bwd(gv, av, c["vm"], c["K"], Sd, va, whole)
    K2 = c["K"].clone()
    K2[1, 2] -= split
    parts, va2 = torch.zeros_like(whole), torch.empty(h, w, device=dev)
    _raw_bwd(gv[:, :split], av[:split], c["vm"], c["K"], Sd, va2[:split], parts)
    _raw_bwd(gv[:, split:], av[split:].contiguous(), c["vm"], K2, Sd, va2[split:], parts)
    p_whole = _paths(c["vm"], c["K"], h, w, Hs, Ws)
    win_whole = _paths.windowed.clone()
    p_parts = tuple(x + y for x, y in zip(_paths(c["vm"], c["K"], h, w, Hs, Ws, 0, split),
                                          _paths(c["vm"], c["K"], h, w, Hs, Ws, split, h - split)))
    moved = int((_paths.windowed & ~win_whole).sum()), int((~_paths.windowed & win_whole).sum())
    print(f"sky order {name} split {split}: pixels direct -> window {moved[0]}, window -> direct {moved[1]}")
    print(f"sky order {name} split {split}: tiles lds/direct, one call {p_whole}, two calls {p_parts}")
    assert bool(whole.any())
    assert torch.equal(parts, whole)
    assert torch.equal(va2, va)
    if name == "pixel_sized" and split == 24:
        assert moved[0] > 0, "pixels of a direct 16-row tile lie in an 8-row tile of the split calls, which fits the window"
        assert p_whole[1] > 0 and p_whole[0] > 0


def test_conservation(dev):
    """Per channel, the sum of the accumulator is sum_p (1 - alpha) g[c]: the weights of a pixel sum to 1.  Bound: every
    addend is rounded to the unit once (4 n addends per channel, 2^-49 each); in fp32 the complements 1 - fu, 1 - fv, the
    weight product, t * w and tw * g round once each and the four weights then sum to 1 within 3 U: 8 U per unit of
    sum_p |(1 - alpha) g[c]| covers the fp32 part."""
    for (h, w), name in [((70, 130), "several_texels"), ((70, 130), "seam"), ((13, 67), "fine_map"), ((70, 130), "down")]:
        c = _case(h, w, name)
        acc = torch.zeros(c["S"].shape, dtype=torch.int64, device=dev)
        _raw_bwd(GX._alloc("hwc", h, w, dev, c["g"]), c["a"].to(dev), c["vm"], c["K"], c["S"].to(dev), torch.empty(h, w, device=dev), acc)
        got = acc.cpu().sum(dim=(0, 1)).double() * UNIT  # integer sum: exact
        t = (1 - c["a"].double())[None] * c["g"].double()
        want, mag = t.sum(dim=(1, 2)), t.abs().sum(dim=(1, 2))
        bound = 4 * h * w * 2.0 ** -49 + 8 * U * mag
        share = float(((got - want).abs() / bound).max())
        print(f"sky conservation {name} {h}x{w}: error {float((got - want).abs().max()):.3g}, share of the bound {share:.3f}")
        assert share <= 1.0


def test_acc_add_and_grad_convert(dev):
    from clm_gs_amd import _lib
    from clm_gs_amd import clm_kernels as K
    gen = torch.Generator().manual_seed(5)
    q = torch.randint(-2 ** 50, 2 ** 50, (7, 11, 3), generator=gen, dtype=torch.int64)
    q[0] = 0
    src, dst = q.to(dev), torch.zeros(7, 11, 3, dtype=torch.int64, device=dev)
    K.sky_acc_add(_lib.stream(), src, dst)
    K.sky_acc_add(_lib.stream(), src, dst)
    assert torch.equal(dst.cpu(), 2 * q)
    g0 = torch.randn(7, 11, 3, generator=gen)
    grad = g0.to(dev)
    K.sky_grad_convert(_lib.stream(), dst, grad)
    assert not bool(dst.any()), "grad_convert zeroes the accumulator"
    assert torch.equal(grad.cpu(), g0 + ((2 * q).double() * UNIT).float()), "and ADDS the float of the exact sum"


def test_entries_reject_bad_arguments(dev):
    from clm_gs_amd import _lib
    L = _lib.lib()
    x = GX._alloc("hwc", 4, 4, dev, torch.zeros(3, 4, 4))
    a, S = torch.zeros(4, 4, device=dev), torch.zeros(2, 4, 3, device=dev)
    acc, va = torch.zeros(2, 4, 3, dtype=torch.int64, device=dev), torch.zeros(4, 4, device=dev)
    vm = np.eye(4, dtype=np.float32).reshape(-1)
    Kh = np.array([5, 0, 2, 0, 5, 2, 0, 0, 1], dtype=np.float32)
    vp, kp = vm.ctypes.data_as(ctypes.c_void_p), Kh.ctypes.data_as(ctypes.c_void_p)

    def fwd(h=4, w=4, sky=_p(S), hs=2, ws=4, y=_p(x), ys=x.stride(), alphas=_p(a)):
        return L.clmgs_sky_fwd(_lib.stream(), h, w, _p(x), *x.stride(), alphas, vp, kp, sky, hs, ws, y, *ys)

    def bwd(h=4, w=4, sky=_p(S), hs=2, ws=4, acc_=_p(acc), v=_p(va)):
        return L.clmgs_sky_bwd(_lib.stream(), h, w, _p(x), *x.stride(), _p(a), vp, kp, sky, hs, ws, v, acc_)

    assert fwd() == 0 and bwd() == 0
    for bad in (dict(sky=None), dict(hs=0), dict(ws=0), dict(h=0), dict(w=0)):
        assert fwd(**bad) != 0, bad
        assert bwd(**bad) != 0, bad
    assert fwd(alphas=None) != 0 and fwd(y=None) != 0
    assert fwd(ys=(16, 1, 4)) != 0, "in place only as the same view"
    assert bwd(acc_=None) != 0 and bwd(v=None) != 0
    assert L.clmgs_sky_acc_add(_lib.stream(), 4, None, _p(acc)) != 0
    assert L.clmgs_sky_grad_convert(_lib.stream(), 4, _p(acc), None) != 0
    with pytest.raises(_lib.ClmgsError):
        _lib.check(fwd(sky=None))
    torch.cuda.synchronize()
    assert not bool(acc.any()) and not bool(x.any())


# ------------------------------------------------------------------------------------------ operator
@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("layout", ["chw", "hwc_view"])
@pytest.mark.parametrize("hw", [(13, 67), (70, 130)])
def test_apply_sky_then_loss_matches_autograd_of_the_restatement(dev, hw, layout, masked):
    from clm_gs_amd import clm_kernels as K
    h, w = hw
    img, gt, mask, _, _ = ML._case(h, w, "bernoulli")
    if not masked:
        mask = None
    c = _case(h, w, "rotated")
    xr, ar, Sr = img.double().requires_grad_(), c["a"].double().requires_grad_(), c["S"].double().requires_grad_()
    l0 = M.masked_loss(R.apply(xr, ar, Sr, c["vm"], c["K"]), gt, mask, 0.2)
    l0.backward()
    if layout == "chw":
        leaf = img.to(dev).requires_grad_()
        view = leaf
    else:
        leaf = img.permute(1, 2, 0).contiguous().to(dev).requires_grad_()
        view = leaf.permute(2, 0, 1)
    al, Sl = c["a"].to(dev).reshape(1, h, w).requires_grad_(), c["S"].to(dev).requires_grad_()
    y = K.apply_sky(view, al, Sl, c["vm"], c["K"])
    assert y.stride() == view.stride() and y.shape == view.shape
    if mask is None:
        l = K.fused_l1_ssim_loss(y, gt.to(dev), 0.2)
    else:
        l = K.fused_l1_ssim_loss(y, gt.to(dev), 0.2, mask=mask.to(dev), mask_count=int((mask != 0).sum()))
    l.backward()
    gi = leaf.grad.cpu() if layout == "chw" else leaf.grad.permute(2, 0, 1).cpu()
    e_l, e_i = abs(l.item() - l0.item()), rel_l2(gi, xr.grad)
    e_a, e_S = rel_l2(al.grad.cpu().reshape(h, w), ar.grad), rel_l2(Sl.grad.cpu(), Sr.grad)
    print(f"apply_sky + loss {hw} {layout} masked={masked}: loss error {e_l:.3g}, gradient rel_l2: image {e_i:.3g}, "
          f"alpha {e_a:.3g}, map {e_S:.3g}")
    assert e_l < 1e-5
    assert e_i < 1e-4 and e_a < 1e-4 and e_S < 1e-4


def test_apply_camera_sky(dev):
    """The engines' and the evaluation's entry: the image itself without a sky; with one, the map's gradient ADDED in fixed
    point to the accumulator the camera carries; no tape, nothing added."""
    from clm_gs_amd import clm_kernels as K
    from clm_gs_amd.cameras import Camera
    from clm_gs_amd.sky import SkyModel
    h, w = 6, 10
    cam = Camera(0, torch.eye(4), 1.0, 0.7, w, h, device=dev)
    img, a = torch.rand(3, h, w, device=dev), torch.rand(h, w, device=dev)
    assert K.apply_camera_sky(img, a, cam) is img
    m = SkyModel((4, 8), dev, init=(0.25, 0.5, 0.75))
    m.attach([cam])
    leaf, al = img.clone().requires_grad_(), a.clone().requires_grad_()
    y = K.apply_camera_sky(leaf, al, cam)
    want = img + (1 - a)[None] * torch.tensor([0.25, 0.5, 0.75], device=dev)[:, None, None]
    assert float((y.detach() - want).abs().max()) < 1e-6  # a constant map: the weights sum to 1 to rounding
    y.sum().backward()
    assert torch.equal(leaf.grad, torch.ones_like(img))
    assert float((al.grad + 1.5).abs().max()) < 1e-5
    got = m.acc.sum(dim=(0, 1)).double().cpu() * UNIT
    assert float((got - float((1 - a).double().sum())).abs().max()) < 1e-4
    m.before_step()
    assert not bool(m.acc.any()) and abs(float(m.grad.double().sum()) - 3 * float((1 - a).double().sum())) < 1e-3
    with torch.no_grad():
        y2 = K.apply_camera_sky(img, a, cam)
    assert torch.equal(y2, y.detach()) and not bool(m.acc.any())


def test_v_alphas_reaches_the_tile_backward(dev):
    """gsplat.rasterize_to_pixels -> apply_sky -> sum of y * r: the opacities, means2d and conics gradients against the
    same graph with the restatement (its sample s computed in float64 on the host) in place of the operator."""
    from clm_gs_amd import clm_kernels as K
    from clm_gs_amd import gsplat
    from clm_gs_amd.synthetic import nadir_cameras, synth_gaussians
    W_, H_, N_ = 64, 48, 400
    sc = synth_gaussians(N_, seed=3, device=dev)
    cam = nadir_cameras(1, N_, W_, H_, 0.5, seed=3, device=dev)[0]
    vm = cam.world_view_transform.t().contiguous()
    with torch.no_grad():
        radii, m2, depths, conics, _ = gsplat.fully_fused_projection(
            sc["xyz"], None, torch.nn.functional.normalize(sc["rotation"]), torch.exp(sc["scaling"]), vm[None], cam.K[None],
            W_, H_, packed=False)
        tw, th = math.ceil(W_ / 16.0), math.ceil(H_ / 16.0)
        _, ids, fids = gsplat.isect_tiles(m2, radii, depths, 16, tw, th, packed=False)
        offs = gsplat.isect_offset_encode(ids, 1, tw, th)
    gen = torch.Generator().manual_seed(8)
    colors = torch.rand(1, N_, 3, generator=gen).to(dev)
    opac = torch.sigmoid(sc["opacity"]).reshape(1, N_)
    S = torch.rand(16, 32, 3, generator=gen)
    r = torch.randn(3, H_, W_, generator=gen).to(dev)
    s_ref = R.sample(S.double(), _f32(vm.cpu().double()), _f32(cam.K.cpu().double()), H_, W_).float().to(dev)
    out = []
    for use_op in (True, False):
        leaves = [t.detach().clone().requires_grad_() for t in (m2, conics, colors, opac)]
        img, alpha = gsplat.rasterize_to_pixels(leaves[0], leaves[1], leaves[2], leaves[3], W_, H_, 16, offs, fids)
        x, a = img[0].permute(2, 0, 1), alpha[0, ..., 0]
        y = K.apply_sky(x, a, S.to(dev), vm, cam.K) if use_op else x + (1 - a)[None] * s_ref
        (y * r).sum().backward()
        out.append([t.grad.clone() for t in leaves])
        if use_op:
            cover = float((a > 0.5).float().mean())
            assert 0.05 < cover < 0.98, cover
    for name, u, v in zip(("means2d", "conics", "colors", "opacities"), *out):
        e = rel_l2(u.cpu(), v.cpu())
        print(f"rasterizer + apply_sky: {name} gradient rel_l2 {e:.3g}")
        assert bool(v.any()) and e < 1e-4, (name, e)
    # without v_alphas the opacity gradient is another one: the term is not small here
    leaves = [t.detach().clone().requires_grad_() for t in (m2, conics, colors, opac)]
    img, alpha = gsplat.rasterize_to_pixels(leaves[0], leaves[1], leaves[2], leaves[3], W_, H_, 16, offs, fids)
    ((img[0].permute(2, 0, 1) + (1 - alpha[0, ..., 0].detach())[None] * s_ref) * r).sum().backward()
    assert rel_l2(leaves[3].grad.cpu(), out[1][3].cpu()) > 1e-2


# ------------------------------------------------------------------------------------------- engines
W, H, N, BSZ = ML.W, ML.H, ML.N, ML.BSZ
NO_SKY, MASKED, EXPOSED = 3, 1, 2   # this camera of the batch carries no sky; this one a loss mask; this one an exposure row
SKY_SHAPE = (64, 128)


def _sky_map():
    return torch.rand(*SKY_SHAPE, 3, generator=torch.Generator().manual_seed(77))


def _attach(cams, sky=True, constant=None):
    from clm_gs_amd.sky import SkyModel
    model = SkyModel(SKY_SHAPE, "cuda")
    with torch.no_grad():
        model.param.copy_(_sky_map() if constant is None else torch.tensor(constant).expand(*SKY_SHAPE, 3))
    if sky:
        model.attach(cams)
    if constant is None:
        cams[NO_SKY].sky, cams[NO_SKY].sky_acc = None, None
        mask = ML._camera_masks()[0]
        cams[MASKED].loss_mask, cams[MASKED].loss_mask_count = mask.cuda(), int((mask != 0).sum())
        cams[EXPOSED].exposure = GX._exposures()[EXPOSED].cuda()
        cams[EXPOSED].exposure_grad = torch.zeros(3, 4, device="cuda")
    return model


_RUNS = {}


def _batch(strategy, residency="hbm", fused=True, variant="sky", background=None):
    """One batch with the sky on the cameras, the optimizer left out (tests/test_gpu_exposure.py's _batch with the sky model
    next to it) -> losses by camera, model gradients, the accumulator's bits and the converted map gradient, on the CPU.
    variant: "sky" | "detached" (the model exists, no camera carries it) | "constant" (map == 0.25 0.5 0.75 everywhere on
    every camera) | "background" (no sky model, the parent's route with that constant background)."""
    key = (strategy, residency, fused, variant)
    if key in _RUNS:
        return _RUNS[key]
    args, sc, cams = ML._setup(strategy, residency, "none", fused, debug_skip_optimizer=True,
                               stop_update_param=strategy == "naive_offload")
    model = None
    if variant == "sky":
        model = _attach(cams)
    elif variant == "detached":
        model = _attach(cams, sky=False, constant=(0.5, 0.5, 0.5))
    elif variant == "constant":
        model = _attach(cams, constant=(0.25, 0.5, 0.75))
    bg = torch.tensor([0.25, 0.5, 0.75], device="cuda") if variant == "background" else None
    m = ML._make(strategy, sc, args)
    if strategy == "no_offload":
        from clm_gs_amd.strategies.no_offload import baseline_accumGrads_impl
        losses, _ = baseline_accumGrads_impl(m, ML._Scene, cams, bg)
        order = list(range(BSZ))
        gsh = torch.cat((m._features_dc.grad, m._features_rest.grad), dim=1).reshape(-1, 48)
        small = [m._xyz.grad, m._opacity.grad, m._scaling.grad, m._rotation.grad]
    elif strategy == "naive_offload":
        from clm_gs_amd.strategies.naive_offload import naive_offload_train_one_batch
        m.optimizer.zero_grad = lambda *a, **k: None  # the engine ends by dropping the gradients this test reads
        losses, _ = naive_offload_train_one_batch(m, ML._Scene, cams, bg)
        order = list(range(BSZ))
        gk, gsh = m._small.grad, m._parameters.grad
        small = [gk[:, 0:3], gk[:, 3:4], gk[:, 4:7], gk[:, 7:11]]
    else:
        from clm_gs_amd.strategies.clm_offload import clm_offload_train_one_batch
        comm = torch.cuda.Stream()
        gen = torch.Generator(device="cuda").manual_seed(1)
        losses, order, _ = clm_offload_train_one_batch(m, ML._Scene, cams, m.parameters_grad_buffer, bg, None, comm, gen)
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
                               "shs": gsh.detach().cpu().reshape(N, 48).clone()})
    if model is not None:
        r["acc"] = model.acc.cpu().clone()
        model.before_step()
        torch.cuda.synchronize()
        r["sky_grad"], r["sky"] = model.grad.detach().cpu().clone(), model.param.detach().cpu().clone()
        assert not bool(model.acc.any())
    _RUNS[key] = r
    return r


@functools.lru_cache(maxsize=None)
def _float64_batch():
    """The oracle's float64 render of every camera with background None and its alpha, the restated sky, the restated
    exposure transform and the restated (masked) loss; the same once more with the alpha of the sky term detached, for the
    share of the opacity gradient that travels through v_alphas."""
    _, sc, cams = ML._setup("no_offload", masks="none")
    S0 = _sky_map().double()
    res = {}
    for with_v_alpha in (True, False):
        P = {k: sc[k].detach().cpu().double().requires_grad_() for k in ("xyz", "opacity", "scaling", "rotation", "shs48")}
        S = S0.clone().requires_grad_()
        losses, cover = [], []
        for i, c in enumerate(cams):
            vm, K = c.world_view_transform.t().cpu().double(), c.K.cpu().double()
            img, _, _, d = O.render_one_camera(P["xyz"], torch.sigmoid(P["opacity"]), torch.exp(P["scaling"]),
                                               torch.nn.functional.normalize(P["rotation"]),
                                               P["shs48"].reshape(-1, 16, 3), 3, vm, K, W, H)
            alpha = d["alpha"].reshape(H, W)
            if i != NO_SKY:
                img = R.apply(img, alpha if with_v_alpha else alpha.detach(), S, vm, K)
                cover.append((float(((1 - alpha) > 0.1).double().mean()), float((alpha > 0.9).double().mean())))
            if i == EXPOSED:
                img = XR.apply(img, GX._exposures()[EXPOSED].double())
            l = M.masked_loss(img, c.original_image.cpu(), ML._camera_masks()[0] if i == MASKED else None, 0.2)
            l.backward()
            losses.append(l.item())
        grads = {"xyz": P["xyz"].grad, "opacity": P["opacity"].grad.reshape(N, -1), "scaling": P["scaling"].grad,
                 "rotation": P["rotation"].grad, "shs": P["shs48"].grad.reshape(N, 48)}
        res[with_v_alpha] = (losses, grads, S.grad, cover)
    return res


def test_the_engine_scene_exercises_the_sky():
    """The condition on the scene, asserted on the float64 composition."""
    res = _float64_batch()
    _, grads, dS, cover = res[True]
    for sky_share, opaque_share in cover:
        assert sky_share >= 0.10 and opaque_share >= 0.10, cover
    texels = int((dS.abs().sum(dim=2) > 0).sum())
    share = float((grads["opacity"] - res[False][1]["opacity"]).norm() / grads["opacity"].norm())
    print(f"sky engine scene: (1 - alpha > 0.1, alpha > 0.9) shares per camera {[(round(a, 3), round(b, 3)) for a, b in cover]}, "
          f"{texels} texels with a gradient, sky term's share of the opacity gradient {share:.3f}")
    assert texels >= 8
    assert share >= 0.01


@pytest.mark.parametrize("mode", GX.ENGINE_MODES, ids=lambda m: f"{m[0]}-{m[1]}-{'fused' if m[2] else 'op_by_op'}")
def test_engines_with_a_sky_match_the_float64_composition(dev, mode):
    want_l, want_g, want_S, _ = _float64_batch()[True]
    b = _batch(*mode)
    assert torch.equal(b["sky"], _sky_map()), "a batch without an optimizer step leaves the map alone"
    for i, (u, v) in enumerate(zip(b["losses"], want_l)):
        print(f"{mode} camera {i}: loss {u:.7f} vs {v:.7f}")
        assert abs(u - v) < 2e-5, (mode, i)
    for k in b["grads"]:
        e = rel_l2(b["grads"][k], want_g[k])
        print(f"{mode}: {k} gradient rel_l2 {e:.3g}")
        assert e < 1e-3, (mode, k, e)
    e = rel_l2(b["sky_grad"], want_S)
    print(f"{mode}: map gradient rel_l2 {e:.3g}")
    assert e < 1e-3, (mode, e)


def test_fused_modes_agree_on_the_accumulator_bits(dev):
    """Every fused mode runs the same kernels on the same tile outputs: the integers agree whatever the order of the cameras."""
    ref = _batch("clm_offload")["acc"]
    assert bool(ref.any())
    for mode in GX.ENGINE_MODES:
        if mode[2]:
            assert torch.equal(_batch(*mode)["acc"], ref), mode


def test_cameras_without_a_sky_run_the_parent(dev):
    """A sky model exists, no camera carries it: the accumulator stays zero, losses and gradients have the bits of the same
    batch on a run with no sky model at all.  (The op-by-op route's tile backward accumulates with float atomics -- the
    atomic mode of clmgs_rasterize_bwd -- so its gradients do not repeat their own bits from run to run: there the losses
    are compared bit for bit and the gradients to the last few bits.)"""
    for mode in (("clm_offload", "hbm", True), ("no_offload", "hbm", True), ("no_offload", "hbm", False)):
        a = _batch(*mode, variant="detached")
        b = ML._batch(mode[0], mode[1], "none", mode[2])
        assert not bool(a["acc"].any()) and not bool(a["sky_grad"].any())
        assert a["losses"] == b["losses"]
        for k in a["grads"]:
            if mode[2]:
                assert torch.equal(a["grads"][k], b["grads"][k]), (mode, k)
            else:
                assert rel_l2(a["grads"][k], b["grads"][k]) < 1e-6, (mode, k)


@pytest.mark.parametrize("mode", [("clm_offload", "hbm", True), ("no_offload", "hbm", False)],
                         ids=lambda m: f"{m[0]}-{'fused' if m[2] else 'op_by_op'}")
def test_a_constant_map_is_a_constant_background(dev, mode):
    """S == b everywhere against the parent's route with background b and no sky: the same losses and model gradients
    within the engines' tolerance (not bitwise: the weights sum to 1 only to rounding)."""
    a, b = _batch(*mode, variant="constant"), _batch(*mode, variant="background")
    for i, (u, v) in enumerate(zip(a["losses"], b["losses"])):
        assert abs(u - v) < 2e-5, (i, u, v)
    for k in a["grads"]:
        e = rel_l2(a["grads"][k], b["grads"][k])
        print(f"constant map vs background {mode}: {k} gradient rel_l2 {e:.3g}")
        assert e < 1e-3, (k, e)
    assert bool(a["acc"].any())


def test_a_background_on_a_camera_with_a_sky_is_refused(dev):
    from clm_gs_amd.strategies.no_offload import baseline_accumGrads_impl
    for fused in (True, False):
        args, sc, cams = ML._setup("no_offload", "hbm", "none", fused, debug_skip_optimizer=True)
        model = _attach(cams)
        m = ML._make("no_offload", sc, args)
        with pytest.raises(ValueError, match="non-zero background"):
            baseline_accumGrads_impl(m, ML._Scene, cams, torch.tensor([1.0, 1.0, 1.0], device="cuda"))
        torch.cuda.synchronize()
        assert not bool(model.acc.any())


def test_capacity_redo_adds_the_map_gradient_once(dev):
    """A forward repeated for capacity (tests/test_gpu_exposure.py's way of forcing it) adds the gradient of the exact
    forward, once: the accumulator, summed over both batches, has the bits of the exact-size run."""
    def attach(cams):
        from clm_gs_amd.sky import SkyModel
        model = SkyModel(SKY_SHAPE, "cuda")
        with torch.no_grad():
            model.param.copy_(_sky_map())
        model.attach(cams)
        return model
    _, t_exact, m_exact, redo_exact = GX._two_batches(attach, dict(device_side_counts=False))
    _, t_over, m_over, redo_over = GX._two_batches(attach, dict(device_side_counts=True, isect_capacity_margin=0.5,
                                                                isect_capacity_floor=0))
    assert redo_exact == 0 and redo_over >= GE.BSZ, (redo_exact, redo_over)
    assert bool(m_exact.acc.any())
    assert torch.equal(m_over.acc, m_exact.acc)
    for a, b in zip(t_over, t_exact):
        assert torch.equal(a, b)


# ------------------------------------------------------------------------------------------- trainer
def test_trainer_with_sky(dev, tmp_path, monkeypatch):
    from clm_gs_amd import render_trajectory, sky, trainer, utils
    from clm_gs_amd.cameras import camera_sky
    from clm_gs_amd.strategies.clm_offload import clm_offload_eval_one_cam
    work = GX._tiny_scene(tmp_path)
    out = tmp_path / "out"
    gaussians, scene, _ = trainer.train_from_colmap(
        str(work), str(out), strategy="clm_offload", iterations=8, test_iterations=(5,), bsz=4, eval=True,
        disable_auto_densification=True, sky=True, sky_shape=(16, 32), sky_init=(0.2, 0.4, 0.6))
    assert scene.test_cameras and all(camera_sky(c)[1] is None for c in scene.test_cameras)
    assert all(camera_sky(c)[1] is scene.sky.acc for c in scene.train_cameras)
    assert os.path.exists(out / "sky.npz") and os.path.exists(out / "point_cloud" / "iteration_8" / "point_cloud.ply")
    fresh = sky.SkyModel.from_file(str(out), "cuda")
    assert torch.equal(fresh.param.detach(), scene.sky.param.detach())
    moved = (fresh.param.detach().cpu() - torch.tensor([0.2, 0.4, 0.6])).abs().amax(dim=2)
    print(f"sky.npz after 8 images: {int((moved > 1e-4).sum())} of {moved.numel()} texels moved, the farthest by {float(moved.max()):.4f}")
    assert int((moved > 1e-4).sum()) >= 1, "the map moved where it was seen"
    assert int((moved == 0).sum()) >= 1, "a texel no camera saw has zero moments and stays where it was, exactly"
    log = open(out / "python_ws=1_rk=0.log").read()
    assert "Evaluating train:" in log and "Evaluating test:" in log and "end2end total_time:" in log
    # evaluation of a test camera uses the map: another map gives another image wherever alpha < 1
    cam = scene.test_cameras[0]
    with_sky = clm_offload_eval_one_cam(cam, gaussians, None, scene).clone()
    held = cam.sky
    cam.sky = None
    without = clm_offload_eval_one_cam(cam, gaussians, None, scene).clone()
    cam.sky = held
    assert float((with_sky - without).abs().max()) > 0.05
    # render_trajectory --sky reads the map back; without the flag the frames differ
    # (the path: the poses of two test cameras, as fresh camera objects, in place of the built-in city polyline)
    from clm_gs_amd.cameras import Camera
    w_, h_ = cam.image_width, cam.image_height
    frames = {}
    for flag in (["--sky"], []):
        path = [Camera(i, c.world_view_transform.t().cpu(), c.FoVx, c.FoVy, w_, h_, device="cuda")
                for i, c in enumerate(scene.test_cameras[:2])]
        monkeypatch.setattr(render_trajectory, "polyline_trajectory", lambda *a, **k: path)
        d = tmp_path / ("traj_sky" if flag else "traj")
        assert render_trajectory.main(["-m", str(out), "--width", str(w_), "--height", str(h_), "--n_frames", "2",
                                       "--output_dir", str(d)] + flag) == 0
        frames[bool(flag)] = open(d / "frame_00000.png", "rb").read()  # the encoder is deterministic: other bytes, other pixels
    assert frames[True] != frames[False]
    utils.set_img_size(H, W)
