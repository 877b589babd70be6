"""CPU-only: the masked training loss ("Masked loss").  The float64 restatement
(tests/masked_loss_reference.py) against what the reference's own pixelwise masked losses produced
(tests/golden/masked_loss.npz, made by tests/golden/make_masked_loss_golden.py) and against the oracle's unmasked loss;
the COLMAP loader's mask options; trainer.evaluate over counted pixels."""
import io
import os
import shutil
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from oracle import gs_oracle as O
from tests import masked_loss_reference as M
from tests.scenes import rel_l2

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SRC = os.path.join(G, "colmap_tiny")


def test_restatement_reproduces_the_reference_fixture():
    z = np.load(os.path.join(G, "masked_loss.npz"))
    assert os.path.getsize(os.path.join(G, "masked_loss.npz")) <= 100 * 1024
    img, gt, mask = torch.from_numpy(z["img"]), torch.from_numpy(z["gt"]), torch.from_numpy(z["mask"])
    assert tuple(img.shape) == (3, 24, 40) and 0 < int((mask != 0).sum()) < mask.numel()
    x = img.double().requires_grad_()
    loss = M.masked_loss(x, gt, mask, float(z["lambda_dssim"]))
    loss.backward()
    d_loss, d_grad = abs(loss.item() - float(z["loss"])), rel_l2(x.grad, torch.from_numpy(z["grad"]))
    d_l1 = float((M.masked_l1_map(x.detach(), gt, mask) - torch.from_numpy(z["l1_map"])).abs().max())
    d_ss = float((M.masked_ssim_map(x.detach(), gt, mask) - torch.from_numpy(z["ssim_map"])).abs().max())
    print(f"restatement vs fixture: loss {d_loss:.3g}, gradient rel_l2 {d_grad:.3g}, l1 map {d_l1:.3g}, ssim map {d_ss:.3g}")
    assert d_loss < 1e-10 and d_grad < 1e-10
    assert d_l1 < 1e-12 and d_ss < 1e-10
    # what the semantics promise, on the reference's numbers: exact zeros far from every counted pixel
    far = M.far_from_counted(mask)
    assert bool(far.any()) and bool((torch.from_numpy(z["grad"])[:, far] == 0).all())


def test_all_ones_mask_is_the_unmasked_loss():
    g = torch.Generator().manual_seed(3)
    H, W = 70, 130
    img = torch.rand(3, H, W, generator=g).double()
    gt = (torch.rand(3, H, W, generator=g) * 255).to(torch.uint8)
    ones = torch.ones(H, W, dtype=torch.uint8)
    a, b = M.masked_loss(img, gt, ones).item(), O.training_loss(img, gt).item()
    print(f"all-ones mask vs oracle.training_loss: {a - b:.3g}")
    assert abs(a - b) < 1e-6
    assert M.masked_loss(img, gt, None).item() == a
    assert M.masked_loss(img, gt, torch.zeros(H, W, dtype=torch.uint8)).item() == 0.0


# ------------------------------------------------------------------------------------------------ loader
def _scene_copy(tmp_path):
    work = tmp_path / "scene"
    shutil.copytree(SRC, work)
    os.makedirs(work / "masks")
    return work


def _write_mask(path, arr):
    from PIL import Image
    Image.fromarray(arr).save(path)


def test_loader_without_options_is_unchanged(tmp_path):
    from PIL import Image
    from clm_gs_amd.colmap_scene import load_colmap_scene
    work = _scene_copy(tmp_path)
    _write_mask(work / "masks" / "view_001.png.png", np.zeros((16, 24), dtype=np.uint8))  # present, but not asked for
    scene = load_colmap_scene(str(work), device="cpu")
    for c in scene.train_cameras:
        assert c.loss_mask is None and c.loss_mask_count is None
        ref = np.asarray(Image.open(os.path.join(SRC, "images", c.image_name + ".png")).convert("RGB"))
        assert np.array_equal(c.original_image.permute(1, 2, 0).numpy(), ref)


def test_loader_finds_both_namings_counts_and_leaves_the_rest_unmasked(tmp_path):
    from clm_gs_amd.colmap_scene import load_colmap_scene
    work = _scene_copy(tmp_path)
    g = np.random.default_rng(0)
    m1 = (g.random((16, 24)) < 0.5).astype(np.uint8) * g.integers(1, 256, (16, 24)).astype(np.uint8)
    m2 = np.zeros((16, 24), dtype=np.uint8)
    m2[2:9, 5:20] = 255
    _write_mask(work / "masks" / "view_001.png.png", m1)    # COLMAP's convention: NAME.EXT.png
    _write_mask(work / "masks" / "view_002.png", m2)        # the fallback: NAME.png
    m3 = np.full((16, 24), 7, dtype=np.uint8)
    _write_mask(work / "masks" / "view_003.png.png", m3)    # both present: COLMAP's convention wins
    _write_mask(work / "masks" / "view_003.png", np.zeros((16, 24), dtype=np.uint8))
    plain = load_colmap_scene(str(work), device="cpu")
    for masks in ("masks", str(work / "masks")):            # relative to the source path, or absolute
        scene = load_colmap_scene(str(work), device="cpu", masks=masks)
        cams = {c.image_name: c for c in scene.train_cameras}
        for name, want in (("view_001", m1), ("view_002", m2), ("view_003", m3)):
            c = cams[name]
            assert c.loss_mask.dtype == torch.uint8 and tuple(c.loss_mask.shape) == (16, 24) and c.loss_mask.is_contiguous()
            assert np.array_equal(c.loss_mask.numpy() != 0, want != 0), name
            assert c.loss_mask_count == int((want != 0).sum()) and isinstance(c.loss_mask_count, int), name
        for name, c in cams.items():
            if name not in ("view_001", "view_002", "view_003"):
                assert c.loss_mask is None and c.loss_mask_count is None, name
        for a, b in zip(scene.train_cameras, plain.train_cameras):
            assert torch.equal(a.original_image, b.original_image)
    with pytest.raises(FileNotFoundError):
        load_colmap_scene(str(work), device="cpu", masks="no_such_directory")


def test_loader_resizes_masks_with_nearest_neighbour_and_rejects_other_sizes(tmp_path):
    from PIL import Image
    from clm_gs_amd.colmap_scene import load_colmap_scene
    work = _scene_copy(tmp_path)
    g = np.random.default_rng(1)
    m = (g.random((16, 24)) < 0.5).astype(np.uint8) * 200
    _write_mask(work / "masks" / "view_001.png.png", m)
    half = load_colmap_scene(str(work), device="cpu", resolution=2, masks="masks")
    c = half.train_cameras[0]
    assert (c.image_width, c.image_height) == (12, 8) and tuple(c.loss_mask.shape) == (8, 12)
    want = np.asarray(Image.fromarray(m).resize((12, 8), Image.NEAREST))
    assert np.array_equal(c.loss_mask.numpy(), want) and set(np.unique(c.loss_mask.numpy())) <= {0, 200}
    assert c.loss_mask_count == int((want != 0).sum())
    _write_mask(work / "masks" / "view_002.png.png", np.ones((15, 24), dtype=np.uint8))
    with pytest.raises(ValueError, match="mask"):
        load_colmap_scene(str(work), device="cpu", masks="masks")


def test_loader_alpha_channel(tmp_path):
    from PIL import Image
    from clm_gs_amd.colmap_scene import load_colmap_scene
    work = _scene_copy(tmp_path)
    p = work / "images" / "view_001.png"
    rgb = np.asarray(Image.open(p).convert("RGB"))
    alpha = np.zeros((16, 24), dtype=np.uint8)
    alpha[4:12, 3:15] = 1
    alpha[0, 0] = 255
    Image.fromarray(np.dstack([rgb, alpha])).save(p)
    off = load_colmap_scene(str(work), device="cpu")
    assert off.train_cameras[0].loss_mask is None
    assert np.array_equal(off.train_cameras[0].original_image.permute(1, 2, 0).numpy(), rgb)
    on = load_colmap_scene(str(work), device="cpu", alpha_mask=True)
    c = on.train_cameras[0]
    assert np.array_equal(c.loss_mask.numpy() != 0, alpha > 0) and c.loss_mask_count == int((alpha > 0).sum())
    assert torch.equal(c.original_image, off.train_cameras[0].original_image)
    assert on.train_cameras[1].loss_mask is None  # an RGB image has no alpha to take
    file_mask = np.full((16, 24), 9, dtype=np.uint8)
    _write_mask(work / "masks" / "view_001.png.png", file_mask)  # a mask file applies: it wins over the alpha channel
    both = load_colmap_scene(str(work), device="cpu", masks="masks", alpha_mask=True)
    assert both.train_cameras[0].loss_mask_count == 16 * 24
    # transparency without an A band: a palette PNG whose tRNS chunk makes one colour transparent
    idx = np.ones((16, 24), dtype=np.uint8)
    idx[5:9, 2:20] = 0
    pal = Image.fromarray(idx, mode="P")
    pal.putpalette([10, 20, 30, 200, 100, 50] + [0] * (3 * 254))
    pal.save(work / "images" / "view_002.png", transparency=0)
    assert "A" not in Image.open(work / "images" / "view_002.png").getbands()
    trns = load_colmap_scene(str(work), device="cpu", alpha_mask=True).train_cameras[1]
    assert np.array_equal(trns.loss_mask.numpy() != 0, idx != 0) and trns.loss_mask_count == int((idx != 0).sum())
    assert tuple(trns.original_image[:, 0, 0].tolist()) == (200, 100, 50)


def test_camera_takes_the_count_on_the_host_and_checks_the_shape():
    from clm_gs_amd.cameras import Camera, camera_loss_mask
    m = torch.zeros(6, 8, dtype=torch.uint8)
    m[1:3, 2:7] = 3
    c = Camera(0, torch.eye(4), 0.8, 0.6, 8, 6, device="cpu", loss_mask=m)
    assert c.loss_mask_count == 10 and torch.equal(c.loss_mask, m) and camera_loss_mask(c) == (c.loss_mask, 10)
    assert camera_loss_mask(Camera(0, torch.eye(4), 0.8, 0.6, 8, 6, device="cpu")) == (None, None)
    assert camera_loss_mask(SimpleNamespace()) == (None, None)  # camera objects from before the attribute
    with pytest.raises(ValueError):
        Camera(0, torch.eye(4), 0.8, 0.6, 8, 6, device="cpu", loss_mask=torch.zeros(8, 6, dtype=torch.uint8))


# ---------------------------------------------------------------------------------------------- evaluate
def test_evaluate_counts_only_counted_pixels():
    from clm_gs_amd import trainer
    g = torch.Generator().manual_seed(2)
    H, W = 12, 20
    gt = (torch.rand(3, H, W, generator=g) * 255).to(torch.uint8)
    render = torch.rand(3, H, W, generator=g) * 1.2 - 0.1
    mask = torch.zeros(H, W, dtype=torch.uint8)
    mask[2:9, 4:15] = 255
    render_bad = render.clone()
    render_bad[:, mask == 0] = 5.0  # rubbish where the mask ignores: must not move the metrics
    masked = SimpleNamespace(original_image=gt, loss_mask=mask, loss_mask_count=int((mask != 0).sum()))
    plain = SimpleNamespace(original_image=gt)
    log = io.StringIO()
    l1, ps = trainer.evaluate("train", 7, [masked], lambda cam: render_bad, log)
    want_l1, want_ps = M.masked_eval_metrics(render, gt, mask)
    assert abs(l1 - want_l1) < 1e-6 and abs(ps - want_ps) < 1e-4
    assert log.getvalue() == "[ITER 7] Evaluating train: L1 {} PSNR {}\n".format(l1, ps)
    l1u, psu = trainer.evaluate("train", 7, [plain], lambda cam: render, io.StringIO())
    x, y = render.clamp(0, 1), gt.float() / 255.0
    assert abs(l1u - float((x - y).abs().mean())) < 1e-7 and abs(l1u - l1) > 1e-4
    # a mixed set: the mean of the per-camera figures; a camera whose mask counts nothing has nothing to measure and
    # stays out of the means (it would contribute L1 0 and an infinite PSNR)
    empty = SimpleNamespace(original_image=gt, loss_mask=torch.zeros(H, W, dtype=torch.uint8), loss_mask_count=0)
    l1m, psm = trainer.evaluate("test", 7, [masked, empty, plain], lambda cam: render, io.StringIO())
    assert abs(l1m - 0.5 * (l1 + l1u)) < 1e-7 and abs(psm - 0.5 * (ps + psu)) < 1e-5
