"""-m gpu: per-camera exposure compensation ("Exposure"): the kernels of csrc/exposure.hip on their
own, through clm_kernels.apply_exposure, through the engines and through the trainer, against the float64 restatement in
tests/exposure_reference.py."""
import ctypes
import functools
import json
import os
import shutil

import numpy as np
import pytest
import torch

from oracle import gs_oracle as O
from tests import exposure_reference as R
from tests import masked_loss_reference as M
from tests import test_gpu_engines as GE
from tests import test_gpu_masked_loss as ML
from tests.scenes import rel_l2

pytestmark = pytest.mark.gpu

U = 2.0 ** -24  # unit roundoff of float32
# 1 pixel; 35 = 8 groups of 4 + a tail of 3; 871 = 4 * 217 + 3; 9100: several forward workgroups (4096 pixels each), a partial last one
SHAPES = [(1, 1), (5, 7), (13, 67), (70, 130)]
LAYOUTS = ["hwc", "chw", "hwc_offset"]  # the engine's interleaved buffer (fast path) | planar | interleaved, base moved by one pixel
# csrc/exposure.hip: EXP_LANE_PIXELS, the DPP steps of wave_sum, EXP_WAVES, the four slices of rows_finish_kernel<16> (+ its two-step tree)
LANE_PIXELS, WAVE_STEPS, WAVES, FINISH_SLICES, FINISH_TREE = 64, 6, 4, 4, 2


def _chain(rows):
    """The longest serial chain of float32 additions behind one element of dE: a lane's pixels, the wave reduction, the
    waves of a workgroup, the rows one lane of the finish kernel sums plus its tree, and the add into the gradient row."""
    return LANE_PIXELS + WAVE_STEPS + WAVES + (-(-rows // FINISH_SLICES) + FINISH_TREE) + 1


def _alloc(layout, h, w, dev, fill=None):
    """A [3,H,W] float32 view on the device in the given memory layout, NaN where nothing is copied in."""
    if layout == "chw":
        t = torch.full((3, h, w), float("nan"), device=dev)
    elif layout == "hwc":
        t = torch.full((h, w, 3), float("nan"), device=dev).permute(2, 0, 1)
    else:
        buf = torch.full(((h * w + 1) * 3,), float("nan"), device=dev)
        t = buf[3:].view(h, w, 3).permute(2, 0, 1)
        assert t.data_ptr() % 16 == 12
    if fill is not None:
        t.copy_(fill.to(dev))
    return t


def _p(t):
    return ctypes.c_void_p(t.data_ptr())


def _raw_fwd(x, E, y):
    from clm_gs_amd import _lib
    _, h, w = x.shape
    _lib.check(_lib.lib().clmgs_exposure_fwd(_lib.stream(), h, w, _p(x), *x.stride(), _p(E), _p(y), *y.stride()))


def _raw_bwd(x, E, g, v):
    """-> partial rows [rows,12], every row written by the kernel (NaN before)."""
    from clm_gs_amd import _lib
    L = _lib.lib()
    _, h, w = x.shape
    rows = int(L.clmgs_exposure_partials_rows(h, w))
    partials = torch.full((rows, 12), float("nan"), device=x.device)
    _lib.check(L.clmgs_exposure_bwd(_lib.stream(), h, w, _p(x), *x.stride(), _p(E), _p(g), *g.stride(), _p(v), *v.stride(),
                                    _p(partials)))
    return partials


def _raw_finish(partials, grad12):
    from clm_gs_amd import _lib
    _lib.check(_lib.lib().clmgs_exposure_grad_finish(_lib.stream(), int(partials.shape[0]), _p(partials), _p(grad12)))


@functools.lru_cache(maxsize=None)
def _case(h, w):
    """Inputs and the float64 reference, computed once per shape and shared by the layouts and tests."""
    gen = torch.Generator().manual_seed(100 * h + w)
    x = torch.rand(3, h, w, generator=gen) * 1.2 - 0.1
    g = torch.randn(3, h, w, generator=gen) * 1e-3
    E = torch.rand(3, 4, generator=gen) * 3.0 - 1.5
    xd, gd, Ed = x.double(), g.double(), E.double()
    v_x, v_E = R.vjp(xd, Ed, gd)
    m_x, m_E = R.magnitude_vjp(xd, Ed, gd)
    return x, g, E, R.apply(xd, Ed), R.magnitude_fwd(xd, Ed), v_x, v_E, m_x, m_E


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("hw", SHAPES)
def test_forward_against_float64(dev, hw, layout):
    h, w = hw
    x, _, E, y0, mag, *_ = _case(h, w)
    xv, yv = _alloc(layout, h, w, dev, x), _alloc(layout, h, w, dev)
    _raw_fwd(xv, E.to(dev), yv)
    y = yv.cpu().double()
    assert bool(torch.isfinite(y).all()), "every element of y must be written"
    bound = 4 * U * mag  # one product, two fused multiply-adds, one addition
    worst = float(((y - y0).abs() / bound).max())
    print(f"exposure fwd {hw} {layout}: largest error / bound {worst:.3f}")
    assert bool(((y - y0).abs() <= bound).all()), worst


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("hw", SHAPES)
def test_identity_is_exact(dev, hw, layout):
    h, w = hw
    x = _case(h, w)[0]
    xv, yv = _alloc(layout, h, w, dev, x), _alloc(layout, h, w, dev)
    _raw_fwd(xv, torch.eye(3, 4, device=dev), yv)
    assert torch.equal(yv, xv)


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("hw", SHAPES)
def test_backward_against_float64(dev, hw, layout):
    from clm_gs_amd import _lib
    h, w = hw
    x, g, E, _, _, v0, dE0, m_x, m_E = _case(h, w)
    rows = int(_lib.lib().clmgs_exposure_partials_rows(h, w))
    n = _chain(rows)
    if hw == (70, 130):
        assert n <= 128, n
    Ed = E.to(dev)
    xv, gv, vv = _alloc(layout, h, w, dev, x), _alloc(layout, h, w, dev, g), _alloc(layout, h, w, dev)
    partials = _raw_bwd(xv, Ed, gv, vv)
    assert bool(torch.isfinite(partials).all()), "every partial row must be written"
    dE = torch.zeros(12, device=dev)
    _raw_finish(partials, dE)
    v, dE_h = vv.cpu().double(), dE.cpu().double().reshape(3, 4)
    assert bool(torch.isfinite(v).all()), "every element of v_x must be written"
    b_v, b_E = 3 * U * m_x, n * U * m_E  # v_x: one product, two fused multiply-adds
    print(f"exposure bwd {hw} {layout}: {rows} rows, n = {n}; v_x error / bound {float(((v - v0).abs() / b_v).max()):.3f}, "
          f"dE error / bound {float(((dE_h - dE0).abs() / b_E).max()):.4f}")
    assert bool(((v - v0).abs() <= b_v).all())
    assert bool(((dE_h - dE0).abs() <= b_E).all())
    # in place (v_x is g) gives the same bits as out of place
    g2 = _alloc(layout, h, w, dev, g)
    p2 = _raw_bwd(xv, Ed, g2, g2)
    assert torch.equal(g2, vv) and torch.equal(p2, partials)
    # a second run gives the same bits, partial rows and total
    v3 = _alloc(layout, h, w, dev)
    p3 = _raw_bwd(xv, Ed, gv, v3)
    dE3 = torch.zeros(12, device=dev)
    _raw_finish(p3, dE3)
    assert torch.equal(p3, partials) and torch.equal(dE3, dE) and torch.equal(v3, vv)
    # grad_finish ADDS: twice, onto a row that is not zero
    row0 = torch.randn(12, generator=torch.Generator().manual_seed(4)) * float(dE0.abs().max())
    row = row0.to(dev)
    _raw_finish(partials, row)
    _raw_finish(partials, row)
    want = row0.double().reshape(3, 4) + 2 * dE0
    b_add = 2 * b_E + 2 * U * (row0.double().abs().reshape(3, 4) + 2 * dE0.abs())  # + the two roundings of the adds themselves
    assert bool(((row.cpu().double().reshape(3, 4) - want).abs() <= b_add).all())


def test_partial_rows_cover_every_layout():
    """Host only (needs the library, no device): the row count is the eligible layout's split and never below the generic one."""
    from clm_gs_amd import _lib
    L = _lib.lib()
    block = 256 * LANE_PIXELS
    for h, w in [(1, 1), (1, 3), (2, 2), (1, block), (1, block + 1), (1, block + 3), (3, block + 1), (4608, 3456)]:
        n = h * w
        rows = int(L.clmgs_exposure_partials_rows(h, w))
        assert rows == -(-(n - n % 4) // block) + (1 if n % 4 else 0), (h, w, rows)
        assert rows >= -(-n // block)
    assert int(L.clmgs_exposure_partials_rows(4608, 3456)) == 972  # n = 64 + 6 + 4 + 243 + 2 + 1 = 320 at 4608x3456


def test_entries_reject_bad_arguments(dev):
    from clm_gs_amd import _lib
    x = _alloc("hwc", 4, 4, dev, torch.zeros(3, 4, 4))
    E = torch.eye(3, 4, device=dev)
    with pytest.raises(_lib.ClmgsError):
        _raw_fwd(x, E, x)  # the forward is not in place
    with pytest.raises(_lib.ClmgsError):
        _raw_bwd(x, E, x, x)  # v_x must not be x
    g = _alloc("chw", 4, 4, dev, torch.zeros(3, 4, 4))
    with pytest.raises(_lib.ClmgsError):  # in place only as the same view
        _lib.check(_lib.lib().clmgs_exposure_bwd(_lib.stream(), 4, 4, _p(x), *x.stride(), _p(E), _p(g), *g.stride(), _p(g), 1, 12, 3,
                                                 _p(torch.empty(1, 12, device=dev))))


# ------------------------------------------------------------------------------------------ operator
@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("layout", ["chw", "hwc_view"])
@pytest.mark.parametrize("hw", [(13, 67), (70, 130)])
def test_apply_exposure_then_loss_matches_autograd_of_the_restatement(dev, hw, layout, masked):
    from clm_gs_amd import clm_kernels as K
    h, w = hw
    img, gt, mask, _, _ = ML._case(h, w, "bernoulli")
    if not masked:
        mask = None
    E = torch.eye(3, 4) + 0.3 * torch.randn(3, 4, generator=torch.Generator().manual_seed(9))
    xr, Er = img.double().requires_grad_(), E.double().requires_grad_()
    l0 = R.loss(xr, Er, gt, mask, 0.2)
    l0.backward()
    if layout == "chw":
        leaf = img.to(dev).requires_grad_()
        view = leaf
    else:
        leaf = img.permute(1, 2, 0).contiguous().to(dev).requires_grad_()
        view = leaf.permute(2, 0, 1)
    El = E.to(dev).requires_grad_()
    y = K.apply_exposure(view, El)
    assert y.stride() == view.stride() and y.shape == view.shape
    if mask is None:
        l = K.fused_l1_ssim_loss(y, gt.to(dev), 0.2)
    else:
        l = K.fused_l1_ssim_loss(y, gt.to(dev), 0.2, mask=mask.to(dev), mask_count=int((mask != 0).sum()))
    l.backward()
    gi = leaf.grad.cpu() if layout == "chw" else leaf.grad.permute(2, 0, 1).cpu()
    e_l, e_i, e_E = abs(l.item() - l0.item()), rel_l2(gi, xr.grad), rel_l2(El.grad.cpu(), Er.grad)
    print(f"apply_exposure + loss {hw} {layout} masked={masked}: loss error {e_l:.3g}, image gradient rel_l2 {e_i:.3g}, "
          f"E gradient rel_l2 {e_E:.3g}")
    assert e_l < 1e-5
    assert e_i < 1e-4
    assert e_E < 1e-4


def test_apply_camera_exposure(dev):
    """The engines' and the evaluation's entry: the camera's row, its gradient ADDED to the camera's gradient row; the image
    itself for a camera without an exposure."""
    from clm_gs_amd import clm_kernels as K
    from clm_gs_amd.exposure import ExposureModel

    class Cam:
        image_name = "a"
    cam, img = Cam(), torch.rand(3, 6, 10, device=dev)
    assert K.apply_camera_colour(img, cam) is img
    m = ExposureModel(1, dev)
    m.attach([cam])
    with torch.no_grad():
        m.param[0, 0, 3] = 0.25
        m.grad[0] += 1.0
    leaf = img.clone().requires_grad_()
    y = K.apply_camera_colour(leaf, cam)
    assert torch.equal(y.detach()[0], img[0] + 0.25) and torch.equal(y.detach()[1:], img[1:])
    y.sum().backward()
    want = torch.ones(3, 4, device=dev)
    want[:, :3] += img.sum(dim=(1, 2))[:, None]
    want[:, 3] += 60.0
    assert rel_l2(m.grad[0].cpu(), want.cpu()) < 1e-6 and torch.equal(leaf.grad, torch.ones_like(img))
    with torch.no_grad():  # evaluation: no tape, nothing added
        before = m.grad.clone()
        y2 = K.apply_camera_colour(img, cam)
    assert torch.equal(y2, y.detach()) and torch.equal(m.grad, before)


# ------------------------------------------------------------------------------------------- engines
W, H, N, BSZ = ML.W, ML.H, ML.N, ML.BSZ
NO_EXPOSURE = 3   # this camera of the batch carries none
MASKED = 1        # and this one a loss mask as well


def _exposures():
    gen = torch.Generator().manual_seed(31)
    E = torch.eye(3, 4).repeat(BSZ, 1, 1) + 0.15 * torch.randn(BSZ, 3, 4, generator=gen)
    E[:, :, 3] *= 0.3
    return E


def _attach(cams, dev="cuda"):
    from clm_gs_amd.exposure import ExposureModel
    model = ExposureModel(BSZ, dev)
    with torch.no_grad():
        model.param.copy_(_exposures())
    model.attach(cams)
    cams[NO_EXPOSURE].exposure, cams[NO_EXPOSURE].exposure_grad = None, None
    mask = ML._camera_masks()[0]
    cams[MASKED].loss_mask, cams[MASKED].loss_mask_count = mask.cuda(), int((mask != 0).sum())
    return model


_RUNS = {}


def _batch(strategy, residency="hbm", fused=True):
    """One batch with exposures on the cameras, the optimizer left out (tests/test_gpu_masked_loss.py's _batch with the
    exposure table next to it) -> losses by camera, model gradients and the exposure gradient table, on the CPU."""
    key = (strategy, residency, fused)
    if key in _RUNS:
        return _RUNS[key]
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
             exposure_grad=model.grad.detach().cpu().clone(), exposure=model.param.detach().cpu().clone())
    _RUNS[key] = r
    return r


@functools.lru_cache(maxsize=None)
def _float64_batch():
    """The oracle's float64 render of every camera, the restated transform and the restated (masked) loss."""
    _, sc, cams = ML._setup("no_offload", masks="none")
    P = {k: sc[k].detach().cpu().double().requires_grad_() for k in ("xyz", "opacity", "scaling", "rotation", "shs48")}
    Es = [e.double().requires_grad_() for e in _exposures()]
    losses = []
    for i, c in enumerate(cams):
        vm = c.world_view_transform.t().cpu().double()
        img, _, _, _ = O.render_one_camera(P["xyz"], torch.sigmoid(P["opacity"]), torch.exp(P["scaling"]),
                                           torch.nn.functional.normalize(P["rotation"]),
                                           P["shs48"].reshape(-1, 16, 3), 3, vm, c.K.cpu().double(), W, H)
        if i != NO_EXPOSURE:
            img = R.apply(img, Es[i])
        l = M.masked_loss(img, c.original_image.cpu(), ML._camera_masks()[0] if i == MASKED else None, 0.2)
        l.backward()
        losses.append(l.item())
    grads = {"xyz": P["xyz"].grad, "opacity": P["opacity"].grad.reshape(N, -1), "scaling": P["scaling"].grad,
             "rotation": P["rotation"].grad, "shs": P["shs48"].grad.reshape(N, 48)}
    dE = torch.stack([e.grad if e.grad is not None else torch.zeros(3, 4, dtype=torch.float64) for e in Es])
    return losses, grads, dE


ENGINE_MODES = [("no_offload", "hbm", True), ("no_offload", "hbm", False), ("clm_offload", "hbm", True),
                ("clm_offload", "hbm", False), ("clm_offload", "host", True), ("clm_offload", "host_batch", True),
                ("naive_offload", "hbm", True)]


@pytest.mark.parametrize("mode", ENGINE_MODES, ids=lambda m: f"{m[0]}-{m[1]}-{'fused' if m[2] else 'op_by_op'}")
def test_engines_with_exposures_match_the_float64_composition(dev, mode):
    want_l, want_g, want_E = _float64_batch()
    b = _batch(*mode)
    assert torch.equal(b["exposure"], _exposures()), "a batch without an optimizer step leaves the table alone"
    for i, (u, v) in enumerate(zip(b["losses"], want_l)):
        print(f"{mode} camera {i}: loss {u:.7f} vs {v:.7f}")
        assert abs(u - v) < 2e-5, (mode, i)
    for k in b["grads"]:
        e = rel_l2(b["grads"][k], want_g[k])
        print(f"{mode}: {k} gradient rel_l2 {e:.3g}")
        assert e < 1e-3, (mode, k, e)
    for i in range(BSZ):
        if i == NO_EXPOSURE:  # no trace in the table
            assert not bool(b["exposure_grad"][i].any()) and not bool(want_E[i].any())
            continue
        e = rel_l2(b["exposure_grad"][i], want_E[i])
        print(f"{mode} camera {i}: exposure gradient rel_l2 {e:.3g}")
        assert e < 1e-3, (mode, i, e)


def test_exposures_change_the_loss_and_nothing_in_front_of_it(dev):
    """Against the same batch without exposures (tests/test_gpu_masked_loss.py's, unmasked): the cameras that carry one see
    another loss, the one that carries none sees the same; and the op-by-op and fused engines agree on the table."""
    a, b = _batch("clm_offload"), ML._batch("clm_offload", masks="none")
    for i, (u, v) in enumerate(zip(a["losses"], b["losses"])):
        if i == NO_EXPOSURE:
            assert u == v, (u, v)
        else:
            assert abs(u - v) > 1e-6, (i, u, v)
    e = rel_l2(_batch("clm_offload", fused=True)["exposure_grad"], _batch("clm_offload", fused=False)["exposure_grad"])
    assert e < 1e-4, e


def _two_batches(exposure_model_for, overrides=None):
    """tests/test_gpu_engines.py's two-batch loop (test_device_side_counts_equal_exact_sizes_and_survive_overflow) with an
    optional exposure model made by `exposure_model_for(cams)` -> (losses, model tensors, exposure model)."""
    from clm_gs_amd import _lib, fused, utils
    from clm_gs_amd.strategies.clm_offload import clm_offload_train_one_batch
    args, sc, cams = GE._setup("clm_offload")
    for k, v in (overrides or {}).items():
        setattr(args, k, v)
    fused._CAPACITY.clear(); fused._CAP_HELD.clear()
    _lib.STATS["isect_capacity_redo"] = 0
    model = exposure_model_for(cams) if exposure_model_for is not None else None
    m = GE._make("clm_offload", sc, args)
    comm, gen = torch.cuda.Stream(), torch.Generator(device="cuda").manual_seed(1)
    it, losses = 1, []
    for _ in range(2):
        utils.set_cur_iter(it)
        m.update_learning_rate(it)
        l, _, _ = clm_offload_train_one_batch(m, GE._Scene, cams, m.parameters_grad_buffer, None, None, comm, gen)
        losses += [x.item() for x in l]
        if model is not None and getattr(model, "step_in_test", False):
            model.step(it)
            model.zero_grad()
        it += GE.BSZ
    torch.cuda.synchronize()
    m.flush_lazy_rows()
    tensors = [t.detach().clone() for t in (m._xyz, m._opacity, m._scaling, m._rotation, m._parameters)]
    redo = _lib.STATS["isect_capacity_redo"]
    fused._CAPACITY.clear(); fused._CAP_HELD.clear()
    return losses, tensors, model, redo


def test_capacity_redo_adds_the_exposure_gradient_once(dev):
    """A forward repeated for capacity (isect_capacity_margin 0.5: every camera of the second batch is found over capacity
    and redone exactly) adds the gradient of the exact forward, once: the table, accumulated over both batches, has the bits
    of the exact-size run."""
    def attach(cams):
        from clm_gs_amd.exposure import ExposureModel
        model = ExposureModel(GE.BSZ, "cuda")
        with torch.no_grad():
            model.param.copy_(_exposures())
        model.attach(cams)
        return model
    _, t_exact, m_exact, redo_exact = _two_batches(attach, dict(device_side_counts=False))
    _, t_over, m_over, redo_over = _two_batches(attach, dict(device_side_counts=True, isect_capacity_margin=0.5,
                                                             isect_capacity_floor=0))
    assert redo_exact == 0 and redo_over >= GE.BSZ, (redo_exact, redo_over)
    assert bool(m_exact.grad.any())
    assert torch.equal(m_over.grad, m_exact.grad)
    for a, b in zip(t_over, t_exact):
        assert torch.equal(a, b)


def test_identity_exposures_at_zero_learning_rate_train_the_same_model(dev):
    """Off means off: identity rows, stepped at learning rate 0 after each of two batches.  The transform and its VJP are
    exact at the identity (1 * x + 0 * .. + 0), so every model tensor ends with the values of the run without exposures
    (torch.equal compares values: a -0.0 against a 0.0 would pass, and would be harmless)."""
    def attach(cams):
        from clm_gs_amd.exposure import ExposureModel
        model = ExposureModel(GE.BSZ, "cuda", lr_init=0.0, lr_final=0.0, max_steps=100)
        model.attach(cams)
        model.step_in_test = True
        return model
    l_plain, t_plain, _, _ = _two_batches(None)
    l_exp, t_exp, model, _ = _two_batches(attach)
    assert l_exp == l_plain
    assert torch.equal(model.param.detach(), torch.eye(3, 4, device="cuda").expand(GE.BSZ, 3, 4))
    for name, a, b in zip(("xyz", "opacity", "scaling", "rotation", "shs"), t_exp, t_plain):
        assert torch.equal(a, b), name


# ------------------------------------------------------------------------------------------- trainer
def _tiny_scene(tmp_path):
    """The tiny COLMAP scene of tests/test_gpu_masked_loss.py's trainer test: a blob of points in front of every camera."""
    from clm_gs_amd.colmap_scene import load_colmap_scene
    work = tmp_path / "scene"
    shutil.copytree(ML.SRC, work)
    poses = load_colmap_scene(str(work), device="cuda", load_images=False)
    g = torch.Generator().manual_seed(11)
    pts = []
    for c in poses.train_cameras:
        c2w = c.camtoworlds[0].cpu()
        local = torch.cat([torch.randn(150, 2, generator=g) * 0.6, 4.0 + torch.rand(150, 1, generator=g)], 1)
        pts.append(local @ c2w[:3, :3].T + c2w[:3, 3])
    pts = torch.cat(pts).numpy().astype(np.float64)
    rgb = (torch.rand(len(pts), 3, generator=g) * 255).to(torch.uint8).numpy()
    with open(work / "sparse" / "0" / "points3D.txt", "w") as f:
        for i, (p, cc) in enumerate(zip(pts, rgb)):
            f.write(f"{i + 1} {float(p[0])!r} {float(p[1])!r} {float(p[2])!r} {int(cc[0])} {int(cc[1])} {int(cc[2])} 0.5 1 0\n")
    os.remove(work / "sparse" / "0" / "points3D.bin")
    return work


def test_trainer_with_exposure(dev, tmp_path):
    from clm_gs_amd import trainer
    from clm_gs_amd.cameras import camera_exposure
    from clm_gs_amd.exposure import ExposureModel
    work = _tiny_scene(tmp_path)
    out = tmp_path / "out"
    gaussians, scene, _ = trainer.train_from_colmap(
        str(work), str(out), strategy="clm_offload", iterations=8, test_iterations=(5,), bsz=4, eval=True,
        disable_auto_densification=True, exposure=True)
    assert scene.test_cameras and all(camera_exposure(c) == (None, None) for c in scene.test_cameras)
    assert all(camera_exposure(c)[0] is not None for c in scene.train_cameras)
    table = json.load(open(out / "exposure.json"))
    assert sorted(table) == sorted(c.image_name for c in scene.train_cameras)
    eye = torch.eye(3, 4)
    rows = {k: torch.tensor(v, dtype=torch.float64).to(torch.float32) for k, v in table.items()}
    assert all(r.shape == (3, 4) for r in rows.values())
    log = open(out / "python_ws=1_rk=0.log").read()
    # 10 training cameras, two batches of 4: the rows of the 8 cameras the loss lines name have moved; a row whose camera
    # was never drawn has zero moments, which dense Adam does not move -- it is still the identity, exactly
    import re
    trained = set(re.findall(r"'([^']+)'", " ".join(re.findall(r" image: \[(.*?)\]", log))))
    assert len(trained) == 8 and trained <= set(table)
    moved = {k: float((r - eye).abs().max()) for k, r in rows.items()}
    print("exposure.json after 8 images: max |E - I| per camera", {k: round(v, 5) for k, v in moved.items()})
    for k, v in moved.items():
        assert (v > 1e-4) if k in trained else (v == 0.0), (k, v)
    fresh = ExposureModel(len(scene.train_cameras), "cuda")
    fresh.load_json(str(out / "exposure.json"), scene.train_cameras)
    assert torch.equal(fresh.param.detach(), scene.exposure.param.detach())
    assert "Evaluating train:" in log and "Evaluating test:" in log and "end2end total_time:" in log
    assert os.path.exists(out / "point_cloud" / "iteration_8" / "point_cloud.ply")
    # without the flag: no table, no file
    out2 = tmp_path / "out2"
    _, scene2, _ = trainer.train_from_colmap(str(work), str(out2), strategy="clm_offload", iterations=8, bsz=4,
                                             disable_auto_densification=True)
    assert scene2.exposure is None and not os.path.exists(out2 / "exposure.json")
    assert os.path.exists(out2 / "point_cloud" / "iteration_8" / "point_cloud.ply")
    assert all(camera_exposure(c) == (None, None) for c in scene2.train_cameras)
