"""CPU-only: depth regularisation -- the float64 restatement against hand-computed cases, the weight schedule, the
loader's convention and reliability rule on files the tests write themselves, Camera validation, the refusals and the
library's new symbols."""
import ctypes
import json
import os
import shutil

import numpy as np
import pytest
import torch

from tests import invdepth_reference as R

SRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "colmap_tiny")
NEW_SYMBOLS = ("clmgs_invdepth_pack", "clmgs_invdepth_l1_fwd_bwd", "clmgs_invdepth_finish", "clmgs_invdepth_rows_bwd",
               "clmgs_invdepth_partials_rows", "clmgs_rasterize4_slot_bwd", "clmgs_rasterize4_fwd_dev",
               "clmgs_rasterize4_bwd_dev")


# ------------------------------------------------------------------------------------------- the restatement
# prior = raw / 65536 * 2 + 0.5 = [[0.5, 1.5], [1.0, 2.0]];  I - prior = [[0 (a tie), 0.5], [-0.75, 1.0]]
RAW = torch.tensor([[0, 32768], [16384, 49152]], dtype=torch.int32).to(torch.uint16)
I22 = torch.tensor([[0.5, 2.0], [0.25, 3.0]], dtype=torch.float64)


def test_restatement_on_a_hand_computed_case():
    assert torch.equal(R.prior_of(RAW, 2.0, 0.5), torch.tensor([[0.5, 1.5], [1.0, 2.0]], dtype=torch.float64))
    leaf = I22.clone().requires_grad_()
    loss = R.depth_term(leaf, RAW, 2.0, 0.5, 0.5)
    assert loss.item() == 0.5 * (0.0 + 0.5 + 0.75 + 1.0) / 4
    loss.backward()
    want = torch.tensor([[0.0, 0.125], [-0.125, 0.125]], dtype=torch.float64)  # the tie passes no gradient
    assert torch.equal(leaf.grad, want)
    assert torch.equal(R.cotangent(I22, RAW, 2.0, 0.5, 0.5), want)


def test_restatement_with_a_masked_pixel():
    """A masked-out pixel adds nothing and receives nothing; the divisor stays H*W."""
    mask = torch.tensor([[255, 1], [1, 0]], dtype=torch.uint8)
    leaf = I22.clone().requires_grad_()
    loss = R.depth_term(leaf, RAW, 2.0, 0.5, 0.5, mask)
    assert loss.item() == 0.5 * (0.0 + 0.5 + 0.75) / 4
    loss.backward()
    want = torch.tensor([[0.0, 0.125], [-0.125, 0.0]], dtype=torch.float64)
    assert torch.equal(leaf.grad, want) and torch.equal(R.cotangent(I22, RAW, 2.0, 0.5, 0.5, mask), want)


def test_weight_schedule_endpoints():
    from clm_gs_amd import utils
    prev = utils.ARGS
    try:
        utils.set_args(utils.default_args(iterations=200))
        assert utils.depth_l1_weight(0) == pytest.approx(1.0, rel=1e-12)
        assert utils.depth_l1_weight(200) == pytest.approx(0.01, rel=1e-12)
        assert utils.depth_l1_weight(100) == pytest.approx(0.1, rel=1e-12)  # log-linear in between
        assert utils.depth_l1_weight(5000) == pytest.approx(0.01, rel=1e-12)
        utils.set_args(utils.default_args(iterations=200, depth_l1_weight_init=0.5, depth_l1_weight_final=0.25))
        assert utils.depth_l1_weight(0) == pytest.approx(0.5) and utils.depth_l1_weight(200) == pytest.approx(0.25)
        utils.set_args(utils.default_args(iterations=200, depth_l1_weight_init=0.0, depth_l1_weight_final=0.0))
        assert utils.depth_l1_weight(7) == 0.0
        a = utils.default_args()
        assert (a.depths, a.depth_l1_weight_init, a.depth_l1_weight_final) == ("", 1.0, 0.01)
    finally:
        utils.set_args(prev)


# ------------------------------------------------------------------------------------------- the loader
def _scene_with_depths(tmp_path, names_to_skip=(), params=None, size=None, folder="depths"):
    """tests/golden/colmap_tiny copied under tmp_path with a depth directory and a depth_params.json written here.
    -> (work dir, {NAME: raw uint16 [h,w]})"""
    from PIL import Image
    from clm_gs_amd.colmap_scene import load_colmap_scene
    work = tmp_path / "scene"
    shutil.copytree(SRC, work)
    cams = load_colmap_scene(str(work), device="cpu", load_images=False).train_cameras
    os.makedirs(work / folder)
    g = np.random.default_rng(3)
    raws = {}
    for c in cams:
        h, w = size or (c.image_height, c.image_width)
        raw = g.integers(0, 65536, size=(h, w), dtype=np.uint16)
        raw[0, 0], raw[-1, -1] = 0, 65535
        raws[c.image_name] = raw
        if c.image_name not in names_to_skip:
            Image.fromarray(raw).save(work / folder / f"{c.image_name}.png")
    if params is None:
        params = {c.image_name: {"scale": 1.0 + 0.01 * i, "offset": 0.001 * i} for i, c in enumerate(cams)}
    with open(work / "sparse" / "0" / "depth_params.json", "w") as f:
        json.dump(params, f)
    return work, raws, [c.image_name for c in cams]


def test_loader_convention_and_training_cameras_only(tmp_path):
    from clm_gs_amd.cameras import camera_invdepth
    from clm_gs_amd.colmap_scene import load_colmap_scene
    work, raws, names = _scene_with_depths(tmp_path)
    sc = load_colmap_scene(str(work), device="cpu", eval=True, depths="depths")
    assert sc.test_cameras and all(camera_invdepth(c) is None for c in sc.test_cameras)
    assert len(sc.train_cameras) + len(sc.test_cameras) == len(names)
    for c in sc.train_cameras:
        raw, scale, offset = camera_invdepth(c)
        i = names.index(c.image_name)
        assert raw.dtype == torch.uint16 and tuple(raw.shape) == (c.image_height, c.image_width)
        assert np.array_equal(raw.numpy(), raws[c.image_name])  # 16 bits, untouched (0 and 65535 included)
        assert (scale, offset) == (1.0 + 0.01 * i, 0.001 * i)
    # an absolute directory is taken as it is; without the argument nothing is attached
    sc2 = load_colmap_scene(str(work), device="cpu", depths=str(work / "depths"))
    assert all(camera_invdepth(c) is not None for c in sc2.train_cameras)
    assert all(camera_invdepth(c) is None for c in load_colmap_scene(str(work), device="cpu").train_cameras)
    with pytest.raises(FileNotFoundError):
        load_colmap_scene(str(work), device="cpu", depths="no_such_dir")


def test_loader_resamples_to_the_training_size(tmp_path):
    """-r 2: the map is resampled to the training size, bilinear on float32, rounded back to uint16: a constant map keeps
    its value, a horizontal ramp stays a monotone ramp within its range; a map already at the training size is untouched."""
    from PIL import Image
    from clm_gs_amd.cameras import camera_invdepth
    from clm_gs_amd.colmap_scene import load_colmap_scene
    work, raws, names = _scene_with_depths(tmp_path)
    full = load_colmap_scene(str(work), device="cpu", load_images=False).train_cameras[0]
    H, W = full.image_height, full.image_width
    const = np.full((H, W), 40000, dtype=np.uint16)
    ramp = np.tile(np.linspace(1000, 60000, W).round().astype(np.uint16), (H, 1))
    Image.fromarray(const).save(work / "depths" / f"{names[0]}.png")
    Image.fromarray(ramp).save(work / "depths" / f"{names[1]}.png")
    sc = load_colmap_scene(str(work), device="cpu", resolution=2, depths="depths")
    c0, c1 = sc.train_cameras[0], sc.train_cameras[1]
    h, w = c0.image_height, c0.image_width
    assert (h, w) == (round(H / 2), round(W / 2))
    r0, r1 = camera_invdepth(c0)[0], camera_invdepth(c1)[0]
    assert r0.dtype == torch.uint16 and tuple(r0.shape) == (h, w) and tuple(r1.shape) == (h, w)
    assert bool((r0.to(torch.int32) == 40000).all())
    r1 = r1.to(torch.int32)
    assert bool((r1[:, 1:] >= r1[:, :-1]).all()) and 1000 <= int(r1.min()) < 3000 and 58000 < int(r1.max()) <= 60000
    assert bool((r1 == r1[:1]).all())
    # written at the training size: the bits of the file
    half = np.ascontiguousarray(raws[names[2]][:h, :w])
    Image.fromarray(half).save(work / "depths" / f"{names[2]}.png")
    sc = load_colmap_scene(str(work), device="cpu", resolution=2, depths="depths")
    assert np.array_equal(camera_invdepth(sc.train_cameras[2])[0].numpy(), half)


def test_loader_reliability_rule(tmp_path, capsys):
    """No prior for: a missing PNG, a missing json entry, scale <= 0, a scale outside [0.2, 5] x the median scale."""
    from clm_gs_amd.cameras import camera_invdepth
    from clm_gs_amd.colmap_scene import load_colmap_scene, read_depth_params, reliable_depth_params
    work, _, names = _scene_with_depths(tmp_path)
    assert len(names) >= 10
    params = {n: {"scale": 2.0, "offset": 0.1} for n in names}
    del params[names[1]]                   # no json entry
    params[names[2]]["scale"] = 0.0        # scale <= 0
    params[names[3]]["scale"] = -1.0
    params[names[4]]["scale"] = 0.39       # below 0.2 x median (0.4)
    params[names[5]]["scale"] = 10.01      # above 5 x median (10)
    params[names[6]]["scale"] = 0.4        # the bounds themselves are kept
    params[names[7]]["scale"] = 10.0
    with open(work / "sparse" / "0" / "depth_params.json", "w") as f:
        json.dump(params, f)
    os.remove(work / "depths" / f"{names[0]}.png")  # no PNG
    table, med = read_depth_params(str(work / "sparse" / "0" / "depth_params.json"))
    assert med == 2.0  # median of the POSITIVE scales
    sc = load_colmap_scene(str(work), device="cpu", depths="depths")
    assert f"depth priors: {len(names) - 6} of {len(names)} training cameras" in capsys.readouterr().out
    got = {c.image_name: camera_invdepth(c) for c in sc.train_cameras}
    for i, n in enumerate(names):
        if i in (0, 1, 2, 3, 4, 5):
            assert got[n] is None, (i, n)
        else:
            assert got[n] is not None and got[n][1:] == (params[n]["scale"], 0.1), (i, n)
    assert reliable_depth_params(table, med, "no_such_image") is None
    # every scale rejected: the run would train without a single prior -> refused, not silent
    with open(work / "sparse" / "0" / "depth_params.json", "w") as f:
        json.dump({n: {"scale": -1.0, "offset": 0.0} for n in names}, f)
    with pytest.raises(ValueError, match="no training camera"):
        load_colmap_scene(str(work), device="cpu", depths="depths")
    # a depth directory without its depth_params.json: refused as well
    os.remove(work / "sparse" / "0" / "depth_params.json")
    with pytest.raises(FileNotFoundError, match="depth_params.json"):
        load_colmap_scene(str(work), device="cpu", depths="depths")


# ------------------------------------------------------------------------------------------- Camera
def test_camera_validates_the_prior():
    from clm_gs_amd.cameras import Camera, camera_invdepth
    w2c = torch.eye(4)
    raw = torch.zeros(6, 8, dtype=torch.uint16)
    c = Camera(0, w2c, 1.0, 0.8, 8, 6, device="cpu", invdepth=raw, invdepth_scale=2.5, invdepth_offset=-0.25)
    got = camera_invdepth(c)
    assert got[0].dtype == torch.uint16 and tuple(got[0].shape) == (6, 8) and got[1:] == (2.5, -0.25)
    assert camera_invdepth(Camera(0, w2c, 1.0, 0.8, 8, 6, device="cpu")) is None

    class Old:  # a camera object from before the attribute existed
        pass
    assert camera_invdepth(Old()) is None
    for bad in (torch.zeros(6, 8, dtype=torch.int16), torch.zeros(6, 8, dtype=torch.float32),
                torch.zeros(8, 6, dtype=torch.uint16), torch.zeros(1, 6, 8, dtype=torch.uint16)):
        with pytest.raises(ValueError, match="invdepth"):
            Camera(0, w2c, 1.0, 0.8, 8, 6, device="cpu", invdepth=bad)
    with pytest.raises(ValueError, match="finite"):
        Camera(0, w2c, 1.0, 0.8, 8, 6, device="cpu", invdepth=raw, invdepth_scale=float("nan"))


# ------------------------------------------------------------------------------------------- refusals, flags, symbols
def test_absgrad_with_depths_is_refused_before_anything_is_loaded(tmp_path):
    from clm_gs_amd import clm_kernels, trainer, utils
    before = utils.ARGS
    with pytest.raises(ValueError, match="absgrad"):  # the source directory does not even exist
        trainer.train_from_colmap(str(tmp_path / "no_such_scene"), str(tmp_path / "out"), absgrad=True, depths="depths")
    assert not (tmp_path / "out").exists() and utils.ARGS is before
    # ... and the engines' own check, for cameras that got their prior some other way

    class Cam:
        invdepth = torch.zeros(2, 2, dtype=torch.uint16)
    try:
        utils.set_args(utils.default_args(absgrad=True))
        with pytest.raises(ValueError, match="absgrad"):
            clm_kernels.check_depth_prior_args(Cam())
        Cam.invdepth = None
        assert clm_kernels.check_depth_prior_args(Cam()) is False
        utils.set_args(utils.default_args())
        Cam.invdepth = torch.zeros(2, 2, dtype=torch.uint16)
        assert clm_kernels.check_depth_prior_args(Cam()) is True
    finally:
        utils.set_args(before)


def test_trainer_parses_the_depth_flags():
    from clm_gs_amd import trainer
    ap = trainer.build_arg_parser()
    a = ap.parse_args(["-s", "x", "-m", "y"])
    assert (a.depths, a.depth_l1_weight_init, a.depth_l1_weight_final) == (None, 1.0, 0.01)
    a = ap.parse_args(["-s", "x", "-m", "y", "--depths", "d", "--depth_l1_weight_init", "0.5", "--depth_l1_weight_final",
                       "0.05"])
    assert (a.depths, a.depth_l1_weight_init, a.depth_l1_weight_final) == ("d", 0.5, 0.05)


def test_library_exports_the_new_symbols():
    from clm_gs_amd import _lib
    l = ctypes.CDLL(_lib.LIB_PATH)
    for n in NEW_SYMBOLS:
        assert hasattr(l, n), n
        assert n in _lib.SIGNATURES, n
    assert _lib.SIGNATURES["clmgs_rasterize4_slot_bwd"] == _lib.SIGNATURES["clmgs_rasterize_bwd"]
    assert _lib.SIGNATURES["clmgs_rasterize4_fwd_dev"] == _lib.SIGNATURES["clmgs_rasterize_fwd_dev"]
    assert _lib.SIGNATURES["clmgs_rasterize4_bwd_dev"] == _lib.SIGNATURES["clmgs_rasterize_bwd_dev"]


def test_render_mode_is_listed():
    from clm_gs_amd.strategies import base_engine as B
    assert "RGB+ID" in B.RENDER_MODES
    col, d = torch.rand(1, 5, 3), torch.tensor([[2.0, 4.0, 0.0, -1.0, 0.5]], requires_grad=True)
    c4, bg = B.colors_with_depth(col, d, torch.tensor([[0.1, 0.2, 0.3]]), "RGB+ID")
    assert torch.equal(c4[..., 3].detach(), torch.tensor([[0.5, 0.25, 0.0, 0.0, 2.0]])) and torch.equal(c4[..., :3], col)
    assert torch.equal(bg, torch.tensor([[0.1, 0.2, 0.3, 0.0]]))
    c4[..., 3].sum().backward()  # d(1/z) = -1/z^2; nothing (and no NaN) at or behind the camera plane
    assert torch.equal(d.grad, torch.tensor([[-0.25, -0.0625, 0.0, 0.0, -4.0]]))
