"""-m gpu: the masked training loss ("Masked loss"): clmgs_l1_ssim_loss_masked_fwd/_bwd through the
operator, the engines and the trainer, against the float64 restatement in tests/masked_loss_reference.py."""
import functools
import os
import shutil

import numpy as np
import pytest
import torch

from oracle import gs_oracle as O
from tests import masked_loss_reference as M
from tests.scenes import rel_l2

pytestmark = pytest.mark.gpu

SRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "colmap_tiny")
SHAPES = [(37, 70), (70, 130)]  # the 64-column seam + a ragged last strip; two strip rows (62 rows each), three strip columns
MASKS = ["bernoulli", "rectangle", "first_pixel", "last_pixel"]


def _mask(kind, h, w):
    m = torch.zeros(h, w, dtype=torch.uint8)
    if kind == "bernoulli":
        g = torch.Generator().manual_seed(23)
        keep = torch.rand(h, w, generator=g) < 0.5
        vals = torch.tensor([0, 1, 255], dtype=torch.uint8)[torch.randint(0, 3, (h, w), generator=g)]
        m = torch.where(keep, vals, m)
    elif kind == "rectangle":
        m[20:62, 40:64] = 255  # edges on the strip seams: rows 61 / 62, columns 63 / 64
    elif kind == "first_pixel":
        m[0, 0] = 1
    elif kind == "last_pixel":
        m[h - 1, w - 1] = 1
    elif kind == "ones":
        m[:] = 1
    elif kind != "zeros":
        raise ValueError(kind)
    return m


@functools.lru_cache(maxsize=None)
def _case(h, w, kind):
    """Inputs and the float64 reference, computed once per (shape, mask) and shared by the layouts."""
    g = torch.Generator().manual_seed(17)
    img = torch.rand(3, h, w, generator=g)
    gt = (torch.rand(3, h, w, generator=g) * 255).to(torch.uint8)
    mask = _mask(kind, h, w)
    x = img.double().requires_grad_()
    loss = M.masked_loss(x, gt, mask, 0.2)
    loss.backward()
    return img, gt, mask, loss.item(), x.grad


def _run(img, gt, mask, layout, dev, count=None, poison=False):
    """The operator on `img` in the given memory layout -> (loss as a Python float, gradient [3,H,W] on the CPU)."""
    from clm_gs_amd import clm_kernels as K
    if layout == "chw":
        leaf = img.to(dev).requires_grad_()
        view = leaf
    else:
        leaf = img.permute(1, 2, 0).contiguous().to(dev).requires_grad_()  # [H,W,3] memory, as the rasterizer leaves it
        view = leaf.permute(2, 0, 1)
    if poison:  # the gradient buffer is torch.empty: hand the allocator blocks full of NaN to reuse
        junk = [torch.full((img.numel(),), float("nan"), device=dev) for _ in range(4)]
        del junk
    if mask is None:
        l = K.fused_l1_ssim_loss(view, gt.to(dev), 0.2)
    else:
        l = K.fused_l1_ssim_loss(view, gt.to(dev), 0.2, mask=mask.to(dev), mask_count=count)
    l.backward()
    got = leaf.grad.cpu() if layout == "chw" else leaf.grad.permute(2, 0, 1).contiguous().cpu()
    return l.item(), got


@pytest.mark.parametrize("kind", MASKS)
@pytest.mark.parametrize("layout", ["chw", "hwc_view"])
@pytest.mark.parametrize("hw", SHAPES)
def test_masked_operator_matches_the_restatement(dev, hw, layout, kind):
    img, gt, mask, l0, g0 = _case(hw[0], hw[1], kind)
    count = int((mask != 0).sum())
    l1, g1 = _run(img, gt, mask, layout, dev, count=count)
    e_loss, e_grad = abs(l1 - l0), rel_l2(g1, g0)
    print(f"masked loss {hw} {layout} {kind} ({count} counted): loss error {e_loss:.3g}, gradient rel_l2 {e_grad:.3g}")
    assert e_loss < 1e-5
    assert e_grad < 1e-4
    l2, g2 = _run(img, gt, mask, layout, dev, count=None)  # the operator counts for itself when not given the count
    assert l2 == l1 and torch.equal(g2, g1)


@pytest.mark.parametrize("layout", ["chw", "hwc_view"])
def test_locality_on_the_rectangle_mask(dev, layout):
    h, w = 70, 130
    img, gt, mask, _, g0 = _case(h, w, "rectangle")
    far = M.far_from_counted(mask)  # farther than 5 pixels (Chebyshev) from every counted pixel
    ring = (~far) & (mask == 0)
    assert bool(far.any()) and bool(ring.any())
    assert bool((g0[:, far] == 0).all())  # the float64 reference itself: exactly 0 there
    l1, g1 = _run(img, gt, mask, layout, dev)
    assert bool((g1[:, far] == 0).all()), float(g1[:, far].abs().max())
    print(f"rectangle {layout}: largest |gradient| at ignored pixels inside the ring {float(g1[:, ring].abs().max()):.3g}, "
          f"reference {float(g0[:, ring].abs().max()):.3g}")
    assert float(g1[:, ring].abs().max()) > 0
    # neither the ground-truth bytes nor the rendered values of the far pixels influence anything
    gen = torch.Generator().manual_seed(99)
    img2, gt2 = img.clone(), gt.clone()
    img2[:, far] = torch.rand(3, int(far.sum()), generator=gen) * 3.0 - 1.0
    gt2[:, far] = (torch.rand(3, int(far.sum()), generator=gen) * 255).to(torch.uint8)
    assert not torch.equal(gt2, gt)
    l2, g2 = _run(img2, gt2, mask, layout, dev)
    assert l2 == l1
    assert torch.equal(g2[:, ~far], g1[:, ~far]) and bool((g2[:, far] == 0).all())


@pytest.mark.parametrize("layout", ["chw", "hwc_view"])
@pytest.mark.parametrize("hw", SHAPES)
def test_all_zero_mask(dev, hw, layout):
    img, gt, mask, l0, g0 = _case(hw[0], hw[1], "zeros")
    assert l0 == 0.0 and not bool(g0.any())
    l1, g1 = _run(img, gt, mask, layout, dev, count=0, poison=True)
    assert l1 == 0.0
    assert bool((g1 == 0).all()), "every element of the gradient buffer must be written"


@pytest.mark.parametrize("layout", ["chw", "hwc_view"])
@pytest.mark.parametrize("hw", SHAPES)
def test_all_ones_mask_is_the_unmasked_operator(dev, hw, layout):
    img, gt, mask, _, _ = _case(hw[0], hw[1], "ones")
    lu, gu = _run(img, gt, None, layout, dev)
    lm, gm = _run(img, gt, mask, layout, dev)
    print(f"all-ones mask {hw} {layout}: loss difference {abs(lm - lu):.3g}, gradient rel_l2 {rel_l2(gm, gu):.3g}, "
          f"gradient bit-equal: {torch.equal(gm, gu)}")
    assert abs(lm - lu) < 1e-6
    assert rel_l2(gm, gu) < 1e-6


def test_operator_rejects_a_wrong_mask(dev):
    from clm_gs_amd import clm_kernels as K
    img = torch.rand(3, 8, 12, device=dev)
    gt = torch.zeros(3, 8, 12, dtype=torch.uint8, device=dev)
    with pytest.raises(AssertionError):
        K.fused_l1_ssim_loss(img, gt, 0.2, mask=torch.ones(12, 8, dtype=torch.uint8, device=dev))
    with pytest.raises(AssertionError):
        K.fused_l1_ssim_loss(img, gt, 0.2, mask=torch.ones(8, 12, device=dev))


# ------------------------------------------------------------------------------------------- engines
W, H, N, BSZ = 96, 64, 3000, 4  # tests/test_gpu_antialias.py
RECTS = [(10, 50, 20, 70), (0, 30, 0, 96), (33, 64, 60, 96), None]  # (y0, y1, x0, x1) per camera; the last stays unmasked


def _camera_masks():
    out = []
    for r in RECTS:
        if r is None:
            out.append(None)
            continue
        m = torch.zeros(H, W, dtype=torch.uint8)
        m[r[0]:r[1], r[2]:r[3]] = 255
        out.append(m)
    return out


def _setup(strategy, residency="hbm", masks="rects", fused=True, seed=0, **over):
    from clm_gs_amd import utils
    from clm_gs_amd.synthetic import nadir_cameras, synth_gaussians
    extra = dict(over)
    if residency == "host_batch":
        residency, extra["host_staging"] = "host", "batch"
    if residency == "host_budget":  # about half of the rows resident in HBM (768 B per row)
        residency, extra["sh_hbm_budget_gb"] = "host", 1500 * 768 / 1e9
    args = utils.default_args(bsz=BSZ, sh_residency=residency, fused_front_end=fused, **extra)
    setattr(args, strategy, True)
    utils.set_args(args)
    utils.set_img_size(H, W)
    utils.set_cur_iter(1)
    sc = synth_gaussians(N, seed=seed, device="cuda")
    cams = nadir_cameras(BSZ, N, W, H, 0.35, seed=seed, device="cuda")
    g = torch.Generator().manual_seed(5)
    for c in cams:
        c.original_image = (torch.rand(3, H, W, generator=g) * 255).to(torch.uint8).cuda()
    if masks == "rects":
        for c, m in zip(cams, _camera_masks()):
            if m is not None:
                c.loss_mask, c.loss_mask_count = m.cuda(), int((m != 0).sum())
    elif masks == "never":  # camera objects from before the attribute existed
        for c in cams:
            del c.loss_mask, c.loss_mask_count
    else:
        assert masks == "none" and all(c.loss_mask is None for c in cams)
    return args, sc, cams


def _make(strategy, sc, args):
    if strategy == "no_offload":
        from clm_gs_amd.strategies.no_offload import GaussianModelNoOffload as Mo
    elif strategy == "naive_offload":
        from clm_gs_amd.strategies.naive_offload import GaussianModelNaiveOffload as Mo
    else:
        from clm_gs_amd.strategies.clm_offload import GaussianModelCLMOffload as Mo
    m = Mo(3)
    m.create_from_tensors(sc["xyz"].clone(), sc["shs48"].clone(), sc["scaling"].clone(),
                          sc["rotation"].clone(), sc["opacity"].clone(), spatial_lr_scale=1.0)
    m.active_sh_degree = 3
    m.training_setup(args)
    return m


class _Scene:
    cameras_extent = 30.0


_BATCHES = {}


def _batch(strategy, residency="hbm", masks="rects", fused=True):
    """One batch, the optimizer left out -> losses by camera, the five gradients (sums over the cameras), statistics
    and intersection counts, on the CPU."""
    from clm_gs_amd import _lib
    key = (strategy, residency, masks, fused)
    if key in _BATCHES:
        return _BATCHES[key]
    args, sc, cams = _setup(strategy, residency, masks, fused, debug_skip_optimizer=True,
                            stop_update_param=strategy == "naive_offload")
    m = _make(strategy, sc, args)
    n0 = len(_lib.STATS["n_isects"])
    if strategy == "no_offload":
        from clm_gs_amd.strategies.no_offload import baseline_accumGrads_impl
        losses, _ = baseline_accumGrads_impl(m, _Scene, cams, None)
        order = list(range(BSZ))
        gsh = torch.cat((m._features_dc.grad, m._features_rest.grad), dim=1).reshape(-1, 48)
        small = [m._xyz.grad, m._opacity.grad, m._scaling.grad, m._rotation.grad]
    elif strategy == "naive_offload":
        from clm_gs_amd.strategies.naive_offload import naive_offload_train_one_batch
        m.optimizer.zero_grad = lambda *a, **k: None  # the engine ends by dropping the gradients this test reads
        losses, _ = naive_offload_train_one_batch(m, _Scene, cams, None)
        order = list(range(BSZ))
        gk, gsh = m._small.grad, m._parameters.grad
        small = [gk[:, 0:3], gk[:, 3:4], gk[:, 4:7], gk[:, 7:11]]
    else:
        from clm_gs_amd.strategies.clm_offload import clm_offload_train_one_batch
        comm = torch.cuda.Stream()
        gen = torch.Generator(device="cuda").manual_seed(1)
        losses, order, _ = clm_offload_train_one_batch(m, _Scene, cams, m.parameters_grad_buffer, None, None, comm, gen)
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
             accum=m.xyz_gradient_accum.detach().cpu().reshape(-1).clone(), denom=m.denom.detach().cpu().reshape(-1).clone(),
             maxr=m.max_radii2D.detach().cpu().reshape(-1).clone(), n_isects=list(_lib.STATS["n_isects"][n0:]))
    _BATCHES[key] = r
    return r


def _close(a, b, tol, what):
    for u, v in zip(a["losses"], b["losses"]):
        assert abs(u - v) < tol, (what, "loss", u, v)
    for k in a["grads"]:
        e = rel_l2(a["grads"][k], b["grads"][k])
        print(f"{what}: {k} gradient rel_l2 {e:.3g}")
        assert e < tol, (what, k, e)


@pytest.mark.parametrize("strategy", ["clm_offload", "no_offload"])
def test_fused_equals_op_by_op_masked(dev, strategy):
    _close(_batch(strategy, fused=True), _batch(strategy, fused=False), 1e-4, f"{strategy} masked, fused vs op-by-op")


def test_strategies_and_residencies_agree_with_no_offload_masked(dev):
    ref = _batch("no_offload")
    for residency in ("hbm", "host", "host_batch", "host_budget"):
        _close(_batch("clm_offload", residency), ref, 1e-4, f"clm_offload {residency} vs no_offload, masked")
    _close(_batch("naive_offload"), ref, 1e-4, "naive_offload vs no_offload, masked")


def test_no_offload_matches_the_float64_composition_masked(dev):
    """The oracle's float64 render of every camera + the restated masked loss."""
    _, sc, cams = _setup("no_offload")
    P = {k: sc[k].detach().cpu().double().requires_grad_() for k in ("xyz", "opacity", "scaling", "rotation", "shs48")}
    want = []
    for c, mask in zip(cams, _camera_masks()):
        vm = c.world_view_transform.t().cpu().double()
        img, _, _, _ = O.render_one_camera(P["xyz"], torch.sigmoid(P["opacity"]), torch.exp(P["scaling"]),
                                           torch.nn.functional.normalize(P["rotation"]),
                                           P["shs48"].reshape(-1, 16, 3), 3, vm, c.K.cpu().double(), W, H)
        l = M.masked_loss(img, c.original_image.cpu(), mask, 0.2)
        l.backward()
        want.append(l.item())
    grads = {"xyz": P["xyz"].grad, "opacity": P["opacity"].grad.reshape(N, -1), "scaling": P["scaling"].grad,
             "rotation": P["rotation"].grad, "shs": P["shs48"].grad.reshape(N, 48)}
    b = _batch("no_offload")
    for u, v in zip(b["losses"], want):
        print(f"no_offload masked vs float64: loss {u:.7f} vs {v:.7f}")
        assert abs(u - v) < 2e-5
    for k in b["grads"]:
        e = rel_l2(b["grads"][k], grads[k])
        print(f"no_offload masked vs float64: {k} gradient rel_l2 {e:.3g}")
        assert e < 1e-3, (k, e)


def test_masked_against_unmasked_batch(dev):
    """The mask changes the loss of the cameras that carry one and nothing in front of the loss: radii, the visibility
    counts and the intersection lists are those of the unmasked batch."""
    for strategy in ("no_offload", "clm_offload"):
        a, b = _batch(strategy), _batch(strategy, masks="none")
        for u, v, r in zip(a["losses"], b["losses"], RECTS):
            if r is not None:
                assert abs(u - v) > 1e-6, (strategy, u, v)
            else:
                assert u == v, (strategy, "the unmasked camera of a mixed batch", u, v)
        assert torch.equal(a["maxr"], b["maxr"]) and torch.equal(a["denom"], b["denom"]), strategy
        assert a["n_isects"] == b["n_isects"] and len(a["n_isects"]) >= BSZ and min(a["n_isects"]) > 0, strategy
        assert not torch.equal(a["accum"], b["accum"]), strategy


def test_no_mask_is_the_parent(dev):
    """Guards the dispatch: cameras whose loss_mask is None train bit-identically to camera objects that never had
    the attribute."""
    for strategy in ("clm_offload", "no_offload"):
        a, b = _batch(strategy, masks="none"), _batch(strategy, masks="never")
        assert a["losses"] == b["losses"], strategy
        for k in a["grads"]:
            assert torch.equal(a["grads"][k], b["grads"][k]), (strategy, k)
        assert torch.equal(a["accum"], b["accum"]) and torch.equal(a["denom"], b["denom"]), strategy


def test_engine_rejects_a_mask_of_another_size(dev):
    from clm_gs_amd import _lib
    from clm_gs_amd.strategies.no_offload import baseline_accumGrads_impl
    args, sc, cams = _setup("no_offload", masks="none")
    cams[0].loss_mask, cams[0].loss_mask_count = torch.ones(W, H, dtype=torch.uint8, device="cuda"), W * H
    with pytest.raises(_lib.ClmgsError):
        baseline_accumGrads_impl(_make("no_offload", sc, args), _Scene, cams, None)
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------- trainer
def test_trainer_with_mask_directory(dev, tmp_path):
    """A few batches of trainer.train_from_colmap on the tiny COLMAP scene with a mask per image; the evaluation line
    is the mean, over the first five training cameras, of L1 / PSNR over the counted pixels of the final render."""
    from PIL import Image
    from clm_gs_amd import trainer
    from clm_gs_amd.colmap_scene import load_colmap_scene
    from clm_gs_amd.strategies.clm_offload import clm_offload_eval_one_cam
    work = tmp_path / "scene"
    shutil.copytree(SRC, work)
    poses = load_colmap_scene(str(work), device="cuda", load_images=False)
    g = torch.Generator().manual_seed(11)
    pts = []
    for c in poses.train_cameras:  # the fixture's poses are random: a blob in front of every camera (tests/test_colmap_scene.py)
        c2w = c.camtoworlds[0].cpu()
        local = torch.cat([torch.randn(150, 2, generator=g) * 0.6, 4.0 + torch.rand(150, 1, generator=g)], 1)
        pts.append(local @ c2w[:3, :3].T + c2w[:3, 3])
    pts = torch.cat(pts).numpy().astype(np.float64)
    rgb = (torch.rand(len(pts), 3, generator=g) * 255).to(torch.uint8).numpy()
    with open(work / "sparse" / "0" / "points3D.txt", "w") as f:
        for i, (p, cc) in enumerate(zip(pts, rgb)):
            f.write(f"{i + 1} {float(p[0])!r} {float(p[1])!r} {float(p[2])!r} {int(cc[0])} {int(cc[1])} {int(cc[2])} 0.5 1 0\n")
    os.remove(work / "sparse" / "0" / "points3D.bin")
    os.makedirs(work / "masks")
    names = sorted(os.listdir(work / "images"))
    for i, name in enumerate(names):
        m = np.zeros((16, 24), dtype=np.uint8)
        m[2 + i % 3:12, 3:16 + i % 5] = 255
        Image.fromarray(m).save(work / "masks" / (name + ".png"))
    out = tmp_path / "out"
    gaussians, scene, _ = trainer.train_from_colmap(
        str(work), str(out), strategy="clm_offload", iterations=8, test_iterations=(5,), bsz=4,
        disable_auto_densification=True, masks="masks", save=False)
    assert all(c.loss_mask is not None and 0 < c.loss_mask_count < 16 * 24 for c in scene.train_cameras)
    log = open(out / "python_ws=1_rk=0.log").read()
    assert "end2end total_time:" in log and log.count(" loss: ") == 2
    line = [ln for ln in log.splitlines() if "Evaluating train:" in ln]
    assert len(line) == 1 and line[0].startswith("[ITER 5] Evaluating train: L1 ")
    l1 = float(line[0].split("L1 ")[1].split(" PSNR")[0])
    ps = float(line[0].split("PSNR ")[1])
    # clm_offload steps inside the engine: the model after the run is the model the evaluation rendered
    want, plain = [], []
    for c in scene.train_cameras[:5]:
        img = clm_offload_eval_one_cam(c, gaussians, None, scene).detach().cpu()
        want.append(M.masked_eval_metrics(img, c.original_image.cpu(), c.loss_mask.cpu()))
        plain.append(M.masked_eval_metrics(img, c.original_image.cpu(), torch.ones(16, 24, dtype=torch.uint8)))
    w_l1, w_ps = sum(a for a, _ in want) / 5, sum(b for _, b in want) / 5
    print(f"evaluation line: L1 {l1:.7f} PSNR {ps:.5f}; restated over counted pixels {w_l1:.7f} {w_ps:.5f}; "
          f"over all pixels {sum(a for a, _ in plain) / 5:.7f}")
    assert abs(l1 - w_l1) < 1e-6 and abs(ps - w_ps) < 1e-3
    assert abs(l1 - sum(a for a, _ in plain) / 5) > 1e-4
