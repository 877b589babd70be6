"""Lens distortion on the CPU: the lens records of clm_kernels.Lens, the two entries in the header, the binding table and
the built library, the float64 reference itself (tests/undistort_reference.py), the band cap that keeps the GPU test's
inputs honest, the loader's geometry with undistort=True, and the options."""
import ctypes
import inspect
import math
import os
import re
import shutil

import numpy as np
import pytest

from clm_gs_amd import _lib, trainer, utils
from clm_gs_amd import colmap_scene as C
from clm_gs_amd.clm_kernels import Lens
from tests import undistort_reference as R

ENTRIES = ("clmgs_undistort_u8", "clmgs_undistort_u16")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "golden", "colmap_tiny")


# ------------------------------------------------------------------------------------------------ the lens records
#                 model, COLMAP's parameters -> fx, fy, cx, cy, k1, k2, k3, k4, p1, p2 | fisheye
RECORDS = [
    ("SIMPLE_PINHOLE", (500.0, 320.5, 239.25), (500.0, 500.0, 320.5, 239.25, 0, 0, 0, 0, 0, 0), False),
    ("PINHOLE", (500.0, 510.0, 320.5, 239.25), (500.0, 510.0, 320.5, 239.25, 0, 0, 0, 0, 0, 0), False),
    ("SIMPLE_RADIAL", (500.0, 320.5, 239.25, -0.11), (500.0, 500.0, 320.5, 239.25, -0.11, 0, 0, 0, 0, 0), False),
    ("RADIAL", (500.0, 320.5, 239.25, -0.11, 0.02), (500.0, 500.0, 320.5, 239.25, -0.11, 0.02, 0, 0, 0, 0), False),
    ("OPENCV", (500.0, 510.0, 320.5, 239.25, -0.11, 0.02, 0.003, -0.004),
     (500.0, 510.0, 320.5, 239.25, -0.11, 0.02, 0, 0, 0.003, -0.004), False),
    ("OPENCV_FISHEYE", (500.0, 510.0, 320.5, 239.25, -0.04, 0.01, -0.003, 0.0007),
     (500.0, 510.0, 320.5, 239.25, -0.04, 0.01, -0.003, 0.0007, 0, 0), True),
]


@pytest.mark.parametrize("model,params,record,fisheye", RECORDS, ids=[r[0] for r in RECORDS])
def test_the_record_of_each_model(model, params, record, fisheye):
    lens = Lens(model, params, 640, 480)
    assert lens.record() == tuple(float(v) for v in record) and lens.fisheye is fisheye
    assert (lens.width, lens.height, lens.model) == (640, 480, model)
    with pytest.raises(ValueError, match=model):
        Lens(model, params[:-1], 640, 480)


@pytest.mark.parametrize("lens_index", range(len(R.LENSES)))
def test_the_gpu_tests_hand_written_records_are_what_lens_builds(lens_index):
    _, model, dist = R.LENSES[lens_index]
    rec, fisheye = R.record(model, dist, 65, 47)
    lens = Lens(model, R.colmap_params(model, dist, 65, 47), 47, 65)
    assert lens.record() == rec and lens.fisheye == fisheye


def test_a_decoded_image_of_another_size_rescales_the_intrinsics():
    lens = Lens("OPENCV", (500.0, 510.0, 320.5, 239.25, -0.11, 0.02, 0.003, -0.004), 640, 480)
    assert lens.at(640, 480) is lens
    half = lens.at(320, 160)   # -r 2 on the width, 3 on the height
    assert half.record() == (250.0, 170.0, 160.25, 239.25 / 3.0, -0.11, 0.02, 0.0, 0.0, 0.003, -0.004)
    assert (half.width, half.height, half.model, half.fisheye) == (320, 160, "OPENCV", False)
    assert lens.record()[0] == 500.0   # the original is not touched


@pytest.mark.parametrize("model", ["FULL_OPENCV", "FOV", "SIMPLE_RADIAL_FISHEYE", "RADIAL_FISHEYE", "THIN_PRISM_FISHEYE"])
def test_the_other_models_are_refused_by_name(model):
    n = C._MODEL_BY_NAME[model][1]
    with pytest.raises(ValueError, match=model):
        Lens(model, [1.0] * n, 64, 48)
    with pytest.raises(ValueError, match="finite"):
        Lens("PINHOLE", (float("nan"), 1.0, 2.0, 2.0), 4, 4)


def test_is_identity():
    centred = Lens("PINHOLE", (30.0, 28.0, 12.0, 8.0), 24, 16)
    assert centred.is_identity() and centred.is_identity((16, 24), 1.0)
    assert not centred.is_identity((16, 24), 0.9) and not centred.is_identity((16, 25), 1.0)
    assert not Lens("PINHOLE", (30.0, 28.0, 12.5, 8.0), 24, 16).is_identity()
    assert not Lens("PINHOLE", (30.0, 28.0, 12.0, 8.0 + 2.0 ** -40), 24, 16).is_identity()   # exactly, or not at all
    assert Lens("OPENCV", (30.0, 28.0, 12.0, 8.0, 0, 0, 0, 0), 24, 16).is_identity()
    assert not Lens("OPENCV", (30.0, 28.0, 12.0, 8.0, 0, 0, 0, 1e-9), 24, 16).is_identity()
    assert not Lens("SIMPLE_RADIAL", (30.0, 12.0, 8.0, 1e-9), 24, 16).is_identity()
    assert not Lens("OPENCV_FISHEYE", (30.0, 28.0, 12.0, 8.0, 0, 0, 0, 0), 24, 16).is_identity()   # equidistant, no pinhole
    assert centred.at(12, 8).is_identity() and Lens("SIMPLE_PINHOLE", (26.0, 12.0, 8.0), 24, 16).is_identity()


# ----------------------------------------------------------------------------------------- the header and the bindings
def test_the_entries_are_declared_bound_and_built():
    header = open(os.path.join(ROOT, "include", "clmgs.h")).read()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in ENTRIES:
        assert re.search(r"\bint\s+%s\s*\(" % name, header), name
        assert name in _lib.SIGNATURES and name not in _lib._NO_STREAM, name
        assert hasattr(lib, name), name
    makefile = open(os.path.join(ROOT, "clm_gs_amd", "csrc", "Makefile")).read()
    assert "undistort.hip" in makefile and "lens_math.h" in makefile


# ------------------------------------------------------------------------------------------------ the reference itself
IDENTITY = (30.0, 28.0, 12.0, 8.0, 0, 0, 0, 0, 0, 0)   # of a 16 x 24 image


def test_an_identity_lens_returns_the_input():
    rng = np.random.default_rng(0)
    for src in (rng.integers(0, 256, size=(3, 16, 24)).astype(np.uint8), rng.integers(0, 65536, size=(16, 24)).astype(np.uint16)):
        out, valid, _ = R.undistort(src, IDENTITY, False, 30.0, 28.0)
        assert np.array_equal(out, src) and (valid == 255).all() and out.dtype == src.dtype


def test_a_whole_pixel_principal_point_shift_is_a_shifted_copy_with_an_invalid_rim():
    src = np.random.default_rng(1).integers(0, 256, size=(3, 16, 24)).astype(np.uint8)
    lens = (30.0, 28.0, 12.0 + 3.0, 8.0 - 2.0) + (0,) * 6      # output (i, j) looks at source (i - 2, j + 3)
    out, valid, _ = R.undistort(src, lens, False, 30.0, 28.0)
    want_valid = np.zeros((16, 24), dtype=bool)
    want_valid[2:, :21] = True
    assert np.array_equal(valid != 0, want_valid)
    assert np.array_equal(out[:, 2:, :21], src[:, :14, 3:]) and not out[:, ~want_valid].any()


def test_a_folding_k1_is_rejected_by_mono_alone():
    H, W = 65, 47
    rec, fisheye = R.record("SIMPLE_RADIAL", (R.FOLDING_K1,), H, W)
    u, v, mono = R.mapping(rec, fisheye, rec[0], rec[1], H, W)
    inside = R.in_bounds(u, v, H, W)
    assert int((inside & (mono <= 0)).sum()) >= 1        # a second image of a ray that is not there: only mono says so
    assert int((inside & (mono > 0)).sum()) >= 1
    src = np.full((H, W), 200, dtype=np.uint8)
    out, valid, _ = R.undistort(src, rec, fisheye, rec[0], rec[1])
    assert np.array_equal(valid != 0, inside & (mono > 0)) and not out[inside & (mono <= 0)].any()


def test_the_fisheye_branch_at_the_centre():
    # a 1 x 1 pinhole looks along the axis: r = 0 exactly, s = 1, no division by zero
    lens = (30.0, 28.0, 12.0, 8.0, -0.04, 0.01, -0.003, 0.0007, 0, 0)
    u, v, mono = R.mapping(lens, True, 30.0, 28.0, 1, 1)
    assert (u[0, 0], v[0, 0], mono[0, 0]) == (11.5, 7.5, 1.0)
    # r -> 0: theta / r -> 1, the map tends to the pinhole's and stays finite and monotone along a row through the axis
    u, v, mono = R.mapping(lens, True, 3e13, 3e13, 1, 4)
    assert np.isfinite(u).all() and np.isfinite(v).all() and (np.diff(u[0]) > 0).all() and (mono == 1.0).all()
    assert np.abs(u[0] - 11.5).max() < 1e-11
    # with all k zero a fisheye is the equidistant projection: u - cx + 0.5 = fx * atan(r) on the x axis
    u, _, _ = R.mapping((30.0, 28.0, 12.0, 8.0) + (0,) * 6, True, 30.0, 28.0, 1, 24)
    x = (np.arange(24) + 0.5 - 12.0) / 30.0
    assert np.allclose(u[0] - 11.5, 30.0 * np.arctan(x), rtol=0, atol=1e-12)


# ------------------------------------------------------------------------------- the band cap of the GPU test's inputs
@pytest.mark.parametrize("size", R.SIZES, ids=lambda s: "%dx%d" % s)
def test_the_band_of_the_gpu_tests_inputs_is_all_but_empty(size):
    """The GPU test allows a difference inside the band only, so the band has to be (all but) empty: at most 0.1 % of the
    pixels and never more than 2, for every (size, lens, zoom) case and both dtypes."""
    H, W = size
    for li, (name, model, dist) in enumerate(R.LENSES):
        rec, fisheye = R.record(model, dist, H, W)
        for zi, zoom in enumerate(R.ZOOMS):
            for src in R.inputs(H, W, li, zi):
                band = R.undistort(src, rec, fisheye, rec[0] * zoom, rec[1] * zoom)[2]
                n = int(band.sum())
                assert n <= 2 and n <= 0.001 * H * W, (size, name, zoom, src.dtype, n)


# ------------------------------------------------------------------------------------------------------- the loader
CAMERAS = """# three distorted cameras with off-centre principal points
1 SIMPLE_RADIAL 24 16 30.0 12.4 7.7 -0.11
2 OPENCV 24 16 26.0 25.0 11.5 8.25 -0.1 0.02 0.001 0.002
3 OPENCV_FISHEYE 24 16 31.0 29.0 12.25 8.5 -0.04 0.01 -0.003 0.0007
"""
FOCALS = {1: (30.0, 30.0), 2: (26.0, 25.0), 3: (31.0, 29.0)}


def distorted_scene(tmp_path, cameras=CAMERAS):
    """A copy of golden/colmap_tiny (text model) whose cameras.txt is rewritten."""
    work = tmp_path / "scene"
    os.makedirs(work / "sparse")
    shutil.copytree(os.path.join(SRC, "sparse_txt", "0"), work / "sparse" / "0")
    shutil.copytree(os.path.join(SRC, "images"), work / "images")
    with open(work / "sparse" / "0" / "cameras.txt", "w") as f:
        f.write(cameras)
    return str(work)


@pytest.mark.parametrize("zoom", [1.0, 0.8])
def test_the_loader_builds_centred_pinholes(tmp_path, zoom, capsys):
    work = distorted_scene(tmp_path)
    scene = C.load_colmap_scene(work, load_images=False, device="cpu", undistort=True, undistort_zoom=zoom)
    cams = scene.train_cameras
    assert len(cams) == 12 and {c.uid for c in cams} == {1, 2, 3}
    for c in cams:
        fx, fy = FOCALS[c.uid]
        assert (c.image_width, c.image_height) == (24, 16) and c.original_image is None and c.loss_mask is None
        assert c.FoVx == 2.0 * math.atan(24 / (2.0 * fx * zoom)) and c.FoVy == 2.0 * math.atan(16 / (2.0 * fy * zoom))
        K = c.K.numpy()
        assert abs(K[0, 0] - fx * zoom) < 1e-4 and abs(K[1, 1] - fy * zoom) < 1e-4 and (K[0, 2], K[1, 2]) == (12.0, 8.0)
    assert len(scene.undistort_log) == 3 and "SIMPLE_RADIAL" in scene.undistort_log[0]
    assert all("zoom %g" % zoom in ln for ln in scene.undistort_log) and "OPENCV_FISHEYE" in capsys.readouterr().out
    half = C.load_colmap_scene(work, load_images=False, device="cpu", resolution=2, undistort=True, undistort_zoom=zoom)
    c = half.train_cameras[0]
    fx = FOCALS[c.uid][0]
    assert (c.image_width, c.image_height) == (12, 8) and c.FoVx == 2.0 * math.atan(12 / (2.0 * (fx * 0.5) * zoom))


def test_the_loader_without_undistort_is_what_it_was(tmp_path):
    work = distorted_scene(tmp_path)
    with pytest.raises(ValueError, match="not handled"):
        C.load_colmap_scene(work, load_images=False, device="cpu")
    plain = C.load_colmap_scene(SRC, device="cpu")
    assert plain.undistort_log == [] and plain.train_cameras[0].loss_mask is None


def test_the_loader_refusals(tmp_path):
    work = distorted_scene(tmp_path)
    with pytest.raises(ValueError, match=r"device='cpu'.*(SIMPLE_RADIAL|OPENCV|OPENCV_FISHEYE)"):
        C.load_colmap_scene(work, device="cpu", undistort=True)      # images on a CPU device: the remap is a device kernel
    for bad in (0.0, -1.0, float("inf"), float("nan")):
        with pytest.raises(ValueError, match="--undistort_zoom"):
            C.load_colmap_scene(work, load_images=False, device="cpu", undistort=True, undistort_zoom=bad)
    other = distorted_scene(tmp_path / "b", "1 PINHOLE 24 16 30 28 12 8\n2 FULL_OPENCV 24 16 30 28 12 8 0 0 0 0 0 0 0 0\n"
                            "3 SIMPLE_PINHOLE 24 16 26 12 8\n")
    with pytest.raises(ValueError, match="FULL_OPENCV"):
        C.load_colmap_scene(other, load_images=False, device="cpu", undistort=True)
    # an identity lens has nothing to remap: images load on a CPU device, bit for bit, without a mask
    centred = distorted_scene(tmp_path / "c", "1 PINHOLE 24 16 30 28 12 8\n2 SIMPLE_PINHOLE 24 16 26 12 8\n"
                              "3 OPENCV 24 16 31 29 12 8 0 0 0 0\n")
    same = C.load_colmap_scene(centred, device="cpu", undistort=True)
    plain = C.load_colmap_scene(centred, device="cpu")
    for a, b in zip(same.train_cameras, plain.train_cameras):
        assert a.loss_mask is None and np.array_equal(a.original_image.numpy(), b.original_image.numpy())
        assert (a.FoVx, a.FoVy) == (b.FoVx, b.FoVy)
    assert all("0.00% of the pixels have no source" in ln for ln in same.undistort_log)


# ------------------------------------------------------------------------------------------------------ the options
def test_the_options_and_their_defaults():
    d = utils.default_args()
    assert (d.undistort, d.undistort_zoom) == (False, 1.0)
    ap = trainer.build_arg_parser()
    base = trainer.train_kwargs(ap.parse_args(["-s", "a", "-m", "b"]))
    assert (base["undistort"], base["undistort_zoom"]) == (False, 1.0)
    out = trainer.train_kwargs(ap.parse_args(["-s", "a", "-m", "b", "--undistort", "--undistort_zoom", "0.8"]))
    assert (out["undistort"], out["undistort_zoom"]) == (True, 0.8)
    assert {"undistort", "undistort_zoom"} <= set(inspect.signature(trainer.train_from_colmap).parameters)
    assert {"undistort", "undistort_zoom"} <= set(inspect.signature(C.load_colmap_scene).parameters)
    from clm_gs_amd import prune_model
    assert {"undistort", "undistort_zoom"} <= set(inspect.signature(prune_model.prune_ply).parameters)


@pytest.mark.parametrize("zoom", [0.0, -0.5, float("inf"), float("nan")])
def test_a_bad_zoom_is_refused_before_anything_is_loaded(tmp_path, zoom):
    with pytest.raises(ValueError, match=re.escape("--undistort_zoom")):
        trainer.check_training(utils.default_args(clm_offload=True, undistort=True, undistort_zoom=zoom))
    with pytest.raises(ValueError, match=re.escape("--undistort_zoom")):
        trainer.train_from_colmap(str(tmp_path / "no_such_scene"), str(tmp_path / "out"), undistort=True, undistort_zoom=zoom)
    assert not (tmp_path / "out").exists()
    trainer.check_training(utils.default_args(clm_offload=True, undistort_zoom=zoom))   # not asked for: not looked at
