"""The resolution schedule on the CPU: the integer reference of the area filter (tests/resample_reference.py), the
geometry of cameras.level_view, the schedule and its refusals, and the three entries in the header, the binding table and
the built library."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from clm_gs_amd import _lib, cameras, trainer, utils
from oracle import gs_oracle as O
from tests import resample_reference as R

ENTRIES = ("clmgs_area_resample_u8", "clmgs_area_resample_u16", "clmgs_area_resample_mask")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------- the reference itself
@pytest.mark.parametrize("n", [1, 2, 3, 5, 7, 16, 17, 33, 47, 65, 1031])
@pytest.mark.parametrize("level", [1, 2, 3])
def test_weights_of_every_row_sum_to_the_source_size(n, level):
    n_dst = R.level_size(n, n, level)[0]
    w = R.weights(n, n_dst)
    assert (w.sum(axis=1) == n).all()        # every destination cell has the same area ...
    assert (w.sum(axis=0) == n_dst).all()    # ... and every source cell is used up exactly
    assert ((w > 0).sum(axis=1) <= (1 << level) + 1).all()


@pytest.mark.parametrize("dtype,top", [(np.uint8, 255), (np.uint16, 65535)])
@pytest.mark.parametrize("level", [1, 2])
def test_divisible_sizes_give_the_rounded_block_mean(dtype, top, level):
    f = 1 << level
    a = np.random.default_rng(level).integers(0, top + 1, size=(3 * f, 5 * f)).astype(dtype)
    blocks = a.astype(np.int64).reshape(3, f, 5, f).sum(axis=(1, 3))
    assert np.array_equal(R.area_resample(a, level), ((2 * blocks + f * f) // (2 * f * f)).astype(dtype))


@pytest.mark.parametrize("dtype,top", [(np.uint8, 255), (np.uint16, 65535)])
@pytest.mark.parametrize("hw", [(1, 1), (3, 5), (17, 33), (16, 16)])
@pytest.mark.parametrize("level", [1, 2])
def test_a_constant_image_stays_the_constant(dtype, top, hw, level):
    out = R.area_resample(np.full(hw, top, dtype=dtype), level)
    assert out.shape == R.level_size(*hw, level) and (out == top).all()


def test_a_mask_cell_with_exactly_half_its_area_counted_is_counted():
    m = np.array([[1, 1, 0, 0], [0, 0, 7, 0]], dtype=np.uint8)   # level 1: cell 0 has 2 of 4, cell 1 has 1 of 4
    out, n = R.mask_resample(m, 1)
    assert out.tolist() == [[255, 0]] and n == 1
    # an inexact pitch: 3 columns -> 2 with weights (2, 1 | 1, 2) of 3.  Left: (2*0 + 1*1) / 3 < 1/2, right: 3 / 3
    out, n = R.mask_resample(np.array([[0, 1, 1]], dtype=np.uint8), 1)
    assert out.tolist() == [[0, 255]] and n == 1
    # ... and 2 x 3 -> 1 x 2: the left cell's weights are (2, 1) in both rows, 6 in all; 2 + 1 is exactly half of it
    out, n = R.mask_resample(np.array([[1, 0, 0], [0, 1, 0]], dtype=np.uint8), 1)
    assert out.tolist() == [[255, 0]] and n == 1
    # 2 x 2 with one diagonal is exactly half
    out, n = R.mask_resample(np.array([[1, 0], [0, 1]], dtype=np.uint8), 1)
    assert out.tolist() == [[255]] and n == 1


# ------------------------------------------------------------------------------------------------------ geometry
def _camera(w=67, h=45, cls=cameras.Camera, **kw):
    w2c = torch.eye(4)
    w2c[:3, :3] = O.quat_to_rotmat(torch.tensor([[0.96, 0.1, -0.2, 0.15]]))[0]
    w2c[:3, 3] = torch.tensor([0.2, -0.1, 4.0])
    return cls(3, w2c, 1.1, 0.8, w, h, device="cpu", **kw)


@pytest.mark.parametrize("level", [1, 2])
def test_a_view_projects_to_the_scaled_pixels(level):
    cam = _camera()
    view = cameras.level_view(cam, level)
    W, H = cam.image_width, cam.image_height
    Ho, Wo = R.level_size(H, W, level)
    assert (view.image_width, view.image_height) == (Wo, Ho)
    assert (view.uid, view.image_name, view.FoVx, view.FoVy) == (cam.uid, cam.image_name, cam.FoVx, cam.FoVy)
    g = torch.Generator().manual_seed(level)
    means = (torch.rand((100, 3), generator=g, dtype=torch.float64) - 0.5) * torch.tensor([2.0, 1.5, 1.0], dtype=torch.float64)
    quats = torch.randn((100, 4), generator=g, dtype=torch.float64)
    scales = torch.full((100, 3), 0.05, dtype=torch.float64)
    vm = cam.world_view_transform.t().double()[None]
    full = O.fully_fused_projection(means, None, quats, scales, vm, cam.K.double()[None], W, H)
    lvl = O.fully_fused_projection(means, None, quats, scales, vm, view.K.double()[None], Wo, Ho)
    seen = (full[0] > 0) & (lvl[0] > 0)
    assert int(seen.sum()) >= 90
    scale = torch.tensor([Wo / W, Ho / H], dtype=torch.float64)
    err = ((lvl[1] - full[1] * scale).abs() * seen[..., None]).max().item()
    assert err < 1e-5, err
    # the host triple the fused front end reads carries the view's K and the camera's pose
    assert np.array_equal(view._clmgs_host[1], view.K.numpy().reshape(9))
    assert np.array_equal(view._clmgs_host[0], cam._clmgs_host[0]) and np.array_equal(view._clmgs_host[2], cam._clmgs_host[2])
    assert not np.array_equal(view._clmgs_host[1], cam._clmgs_host[1])


def test_level_zero_is_the_camera_and_views_share_the_side_models():
    cam = _camera()
    assert cameras.level_view(cam, 0) is cam
    cam.exposure, cam.exposure_grad = torch.zeros(3, 4), torch.zeros(3, 4)
    cam.sky, cam.sky_acc = torch.zeros(4, 8, 3), torch.zeros(4, 8, 3, dtype=torch.int64)
    cam.invdepth_scale, cam.invdepth_offset = 2.5, 0.25
    view = cameras.level_view(cam, 1)
    for name in ("exposure", "exposure_grad", "sky", "sky_acc", "world_view_transform", "camtoworlds"):
        assert getattr(view, name) is getattr(cam, name), name
    assert (view.invdepth_scale, view.invdepth_offset) == (2.5, 0.25)
    assert view.original_image is None and view.loss_mask is None and view.invdepth is None
    grid = _camera()
    grid.bilagrid, grid.bilagrid_grad = torch.zeros(2, 2, 2, 12), torch.zeros(2, 2, 2, 12)
    v2 = cameras.level_view(grid, 2)
    assert v2.bilagrid is grid.bilagrid and v2.bilagrid_grad is grid.bilagrid_grad
    assert cameras.camera_colour(v2)[1] is grid.bilagrid and cameras.camera_sky(view) == (cam.sky, cam.sky_acc)


def test_an_orthographic_camera_is_refused_by_name():
    ortho = cameras.OrthoCamera(0, torch.eye(4), 10.0, 32, 32, image_name="map_tile", device="cpu")
    with pytest.raises(ValueError, match="map_tile.*orthographic"):
        cameras.level_view(ortho, 1)
    with pytest.raises(ValueError, match="orthographic"):
        cameras.level_view(ortho, 0)


# ------------------------------------------------------------------------------------- the schedule, the refusals
def test_the_schedule():
    D, R_, bsz = 2, 8, 4
    firsts = list(range(1, 41, bsz))
    got = [trainer.schedule_level(it, 1, D, R_) for it in firsts]
    assert got == [2, 2, 1, 1, 0, 0, 0, 0, 0, 0]
    assert trainer.schedule_level(9, 1, D, R_) == 1 and trainer.schedule_level(8, 1, D, R_) == 2   # exactly at a boundary
    assert trainer.schedule_level(17, 1, D, R_) == 0 and trainer.schedule_level(16, 1, D, R_) == 1
    assert [trainer.schedule_level(it, 5, 1, 3) for it in (5, 7, 8, 100)] == [1, 1, 0, 0]
    assert trainer.schedule_level(10 ** 6, 1, 0, 3000) == 0


@pytest.mark.parametrize("over,name", [
    (dict(num_downscales=1, pose_opt=True), "--pose_opt"),
    (dict(num_downscales=-1), "--num_downscales"),
    (dict(num_downscales=1, resolution_schedule=0), "--resolution_schedule"),
    (dict(num_downscales=1, resolution_schedule=-5), "--resolution_schedule"),
])
def test_refusals_name_the_option(over, name):
    args = utils.default_args(clm_offload=True, **over)
    with pytest.raises(ValueError, match=re.escape(name)) as e:
        trainer.check_training(args)
    assert "--num_downscales" in str(e.value) or "--resolution_schedule" in str(e.value)


def test_a_schedule_too_deep_for_the_images_is_refused():
    args = utils.default_args(clm_offload=True, num_downscales=3)
    trainer.check_training(args)                              # the size is not known yet: nothing to refuse
    trainer.check_training(args, image_size=(128, 200))       # 16 x 25
    with pytest.raises(ValueError, match=re.escape("--num_downscales 3")):
        trainer.check_training(args, image_size=(64, 96))     # 8 x 12
    with pytest.raises(ValueError, match=re.escape("--num_downscales 2")):
        trainer.check_training(utils.default_args(), num_downscales=2, image_size=(200, 60))


def test_camera_dp_is_refused(monkeypatch):
    monkeypatch.setattr(trainer.dp, "world_size", lambda: 2)
    with pytest.raises(ValueError, match="--num_downscales.*camera-DP"):
        trainer.check_training(utils.default_args(clm_offload=True, num_downscales=1))
    trainer.check_training(utils.default_args(clm_offload=True))


def test_the_options_and_their_defaults():
    d = utils.default_args()
    assert (d.num_downscales, d.resolution_schedule) == (0, 3000)
    ap = trainer.build_arg_parser()
    base = trainer.train_kwargs(ap.parse_args(["-s", "a", "-m", "b"]))
    assert (base["num_downscales"], base["resolution_schedule"]) == (0, 3000)
    out = trainer.train_kwargs(ap.parse_args(["-s", "a", "-m", "b", "--num_downscales", "2", "--resolution_schedule", "500"]))
    assert (out["num_downscales"], out["resolution_schedule"]) == (2, 500)
    import inspect
    for fn in (trainer.training, trainer.train_from_colmap):
        assert {"num_downscales", "resolution_schedule"} <= set(inspect.signature(fn).parameters), fn


# ------------------------------------------------------------------------------------------------- the three entries
def test_the_entries_are_declared_bound_and_built():
    header = open(os.path.join(ROOT, "include", "clmgs.h")).read()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in ENTRIES:
        assert re.search(r"\bint\s+%s\s*\(" % name, header), name
        assert name in _lib.SIGNATURES and name not in _lib._NO_STREAM, name
        assert hasattr(lib, name), name
    makefile = open(os.path.join(ROOT, "clm_gs_amd", "csrc", "Makefile")).read()
    assert "resample.hip" in makefile
