"""Lens distortion on the device: csrc/undistort.hip through clm_kernels.undistort against the float64 reference
(tests/undistort_reference.py), pixel for pixel outside the reference's band; the source mask's four-tap rule; `out=`;
an identity lens at full size; the entries' refusals; and a distorted COLMAP directory end to end through the trainer."""
import ctypes
import os
import shutil

import numpy as np
import pytest
import torch

from tests import undistort_reference as R

pytestmark = pytest.mark.gpu

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SRC = os.path.join(G, "colmap_tiny")
DEV = "cuda"


def _lens(model, dist, H, W):
    from clm_gs_amd.clm_kernels import Lens
    return Lens(model, R.colmap_params(model, dist, H, W), W, H)


def _hold_to_reference(got, got_valid, got_count, ref, ref_valid, band, what):
    """Outside the band: the image, the valid map (hence the count) equal the reference's.  Inside: a value may differ by
    at most 1, a validity either way; the count lies within the band's size of the reference's."""
    got, ref = np.asarray(got).astype(np.int64), np.asarray(ref).astype(np.int64)
    planes = (got if got.ndim == 3 else got[None]), (ref if ref.ndim == 3 else ref[None])
    out = ~band
    assert np.array_equal(planes[0][:, out], planes[1][:, out]), (what, int((planes[0] != planes[1])[:, out].sum()))
    if got_valid is not None:
        got_valid = np.asarray(got_valid)
        assert set(np.unique(got_valid)) <= {0, 255}, what
        assert np.array_equal(got_valid[out], ref_valid[out]), (what, int((got_valid != ref_valid)[out].sum()))
        agree = band & (got_valid == ref_valid)
        assert (np.abs(planes[0] - planes[1])[:, agree] <= 1).all(), what
        assert int(np.count_nonzero(got_valid)) == got_count, what       # the kernel's count is the count of its own map
        assert abs(got_count - int(np.count_nonzero(ref_valid))) <= int(band.sum()), what
    else:
        assert (np.abs(planes[0] - planes[1])[:, band & (ref_valid != 0)] <= 1).all(), what


# ------------------------------------------------------------------------------------- the entries against the reference
@pytest.mark.parametrize("lens_index", range(len(R.LENSES)), ids=[l[0] for l in R.LENSES])
@pytest.mark.parametrize("size", R.SIZES, ids=lambda s: "%dx%d" % s)
def test_the_entries_match_the_float64_reference(size, lens_index):
    from clm_gs_amd.clm_kernels import undistort
    H, W = size
    name, model, dist = R.LENSES[lens_index]
    lens = _lens(model, dist, H, W)
    rec, fisheye = R.record(model, dist, H, W)
    for zi, zoom in enumerate(R.ZOOMS):
        u8, u16 = R.inputs(H, W, lens_index, zi)
        ref, ref_valid, band = R.undistort(u8, rec, fisheye, rec[0] * zoom, rec[1] * zoom)
        out, valid, count = undistort(torch.from_numpy(u8).to(DEV), lens, zoom=zoom, want_valid=True)
        assert out.dtype == torch.uint8 and tuple(out.shape) == (3, H, W) and tuple(valid.shape) == (H, W)
        assert count.dtype == torch.int64 and tuple(count.shape) == (1,)
        _hold_to_reference(out.cpu().numpy(), valid.cpu().numpy(), int(count.item()), ref, ref_valid, band, (name, zoom, "u8"))
        ref, ref_valid, band = R.undistort(u16, rec, fisheye, rec[0] * zoom, rec[1] * zoom)
        out = undistort(torch.from_numpy(u16).to(DEV), lens, zoom=zoom)
        assert out.dtype == torch.uint16 and tuple(out.shape) == (H, W)
        _hold_to_reference(out.cpu().numpy(), None, None, ref, ref_valid, band, (name, zoom, "u16"))


@pytest.mark.parametrize("out_size", [(40, 70), (9, 7)], ids=lambda s: "to%dx%d" % s)
def test_another_output_size(out_size):
    from clm_gs_amd.clm_kernels import undistort
    H, W = 17, 33
    _, model, dist = R.LENSES[3]
    rec, fisheye = R.record(model, dist, H, W)
    u8, _ = R.inputs(H, W, 3, 0)
    ref, ref_valid, band = R.undistort(u8, rec, fisheye, rec[0] * 0.9, rec[1] * 0.9, out_size=out_size)
    assert int(band.sum()) == 0 and 0 < np.count_nonzero(ref_valid)
    out, valid, count = undistort(torch.from_numpy(u8).to(DEV), _lens(model, dist, H, W), out_size=out_size, zoom=0.9,
                                  want_valid=True)
    assert tuple(out.shape) == (3,) + out_size
    _hold_to_reference(out.cpu().numpy(), valid.cpu().numpy(), int(count.item()), ref, ref_valid, band, out_size)


# ---------------------------------------------------------------------------------------------------- the source mask
@pytest.mark.parametrize("density", [0.1, 0.5, 0.9])
@pytest.mark.parametrize("size,lens_index", [((17, 33), 3), ((65, 47), 6), ((5, 1031), 1)],
                         ids=["17x33-opencv", "65x47-fisheye", "5x1031-simple_radial"])
def test_a_pixel_blended_from_an_ignored_pixel_is_ignored(size, lens_index, density):
    from clm_gs_amd.clm_kernels import undistort
    H, W = size
    name, model, dist = R.LENSES[lens_index]
    rec, fisheye = R.record(model, dist, H, W)
    u8, _ = R.inputs(H, W, lens_index, 1)
    rng = np.random.default_rng(int(density * 10) + 100 * lens_index)
    mask = np.where(rng.random((H, W)) < density, rng.integers(1, 256, size=(H, W)), 0).astype(np.uint8)
    ref, ref_valid, band = R.undistort(u8, rec, fisheye, rec[0] * 0.8, rec[1] * 0.8, src_mask=mask)
    no_mask_valid = R.undistort(u8, rec, fisheye, rec[0] * 0.8, rec[1] * 0.8)[1]
    assert np.count_nonzero(ref_valid) < np.count_nonzero(no_mask_valid) and int(band.sum()) <= 2
    out, valid, count = undistort(torch.from_numpy(u8).to(DEV), _lens(model, dist, H, W), zoom=0.8,
                                  src_mask=torch.from_numpy(mask).to(DEV), want_valid=True)
    _hold_to_reference(out.cpu().numpy(), valid.cpu().numpy(), int(count.item()), ref, ref_valid, band, (name, density))
    assert not out.cpu().numpy()[:, valid.cpu().numpy() == 0].any()


# ------------------------------------------------------------------------------------------ out=, a single plane, refusals
def test_out_is_written_and_returned_and_a_single_plane_is_a_plane():
    from clm_gs_amd import _lib
    from clm_gs_amd.clm_kernels import undistort
    H, W = 65, 47
    _, model, dist = R.LENSES[2]
    lens = _lens(model, dist, H, W)
    rec, fisheye = R.record(model, dist, H, W)
    u8, u16 = R.inputs(H, W, 2, 0)
    ref, ref_valid, band = R.undistort(u8, rec, fisheye, rec[0], rec[1])
    assert int(band.sum()) == 0
    src = torch.from_numpy(u8).to(DEV)
    buf = torch.full((3, H, W), 7, dtype=torch.uint8, device=DEV)
    ptr = buf.data_ptr()
    for _ in range(2):  # reuse: the second call overwrites the first one's result
        got = undistort(src, lens, out=buf)
        assert got is buf and buf.data_ptr() == ptr and np.array_equal(buf.cpu().numpy(), ref)
    plane, valid, count = undistort(src[1].contiguous(), lens, want_valid=True)
    assert tuple(plane.shape) == (H, W) and np.array_equal(plane.cpu().numpy(), ref[1])
    assert np.array_equal(valid.cpu().numpy(), ref_valid) and int(count.item()) == np.count_nonzero(ref_valid)
    buf16 = torch.zeros((H, W), dtype=torch.uint16, device=DEV)
    assert undistort(torch.from_numpy(u16).to(DEV), lens, out=buf16) is buf16
    assert np.array_equal(buf16.cpu().numpy(), R.undistort(u16, rec, fisheye, rec[0], rec[1])[0])
    for bad in (torch.zeros((3, H, W + 1), dtype=torch.uint8, device=DEV), torch.zeros((3, H, W), dtype=torch.int32, device=DEV)):
        with pytest.raises(_lib.ClmgsError, match="out must be"):
            undistort(src, lens, out=bad)
    with pytest.raises(_lib.ClmgsError, match="device tensor expected"):
        undistort(torch.from_numpy(u8), lens)
    with pytest.raises(_lib.ClmgsError, match="src_mask must be"):
        undistort(src, lens, src_mask=torch.zeros((H, W + 1), dtype=torch.uint8, device=DEV))
    with pytest.raises(_lib.ClmgsError, match="uint16"):
        undistort(torch.from_numpy(u16).to(DEV), lens, want_valid=True)
    with pytest.raises(ValueError, match="--undistort_zoom"):
        undistort(src, lens, zoom=0.0)


def test_an_identity_lens_at_full_size_returns_the_input_bit_for_bit():
    """Through the kernel (the operator launches for any lens; it is the callers that ask is_identity): u = j and v = i up
    to the last ulp, which is what the tau slack of the bounds test is for.  Needs no CPU reference."""
    from clm_gs_amd.clm_kernels import Lens, undistort
    H, W = 3456, 4608
    lens = Lens("PINHOLE", (3900.0, 3850.0, W / 2.0, H / 2.0), W, H)
    assert lens.is_identity((H, W), 1.0)
    gen = torch.Generator(device=DEV).manual_seed(3)
    src = torch.randint(0, 256, (3, H, W), dtype=torch.uint8, device=DEV, generator=gen)
    out, valid, count = undistort(src, lens, want_valid=True)
    assert out.data_ptr() != src.data_ptr()
    assert torch.equal(out, src) and bool((valid == 255).all()) and int(count.item()) == H * W
    raw = torch.randint(0, 65536, (H, W), dtype=torch.int32, device=DEV, generator=gen).to(torch.uint16)
    assert torch.equal(undistort(raw, lens).view(torch.int16), raw.view(torch.int16))


def test_bad_arguments_return_einval_before_anything_is_written():
    from clm_gs_amd import _lib
    L = _lib.lib()
    H, W = 6, 10
    src = torch.full((3, H, W), 9, dtype=torch.uint8, device=DEV)
    dst = torch.full((3, H, W), 77, dtype=torch.uint8, device=DEV)
    valid = torch.full((H, W), 77, dtype=torch.uint8, device=DEV)
    count = torch.full((1,), 77, dtype=torch.int64, device=DEV)
    src16, dst16 = src[0].to(torch.uint16), torch.full((H, W), 77, dtype=torch.int32, device=DEV).to(torch.uint16)
    good = [20.0, 20.0, 5.0, 3.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0]
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    rec = lambda v: (ctypes.c_double * 10)(*v)

    def u8(planes=3, Hs=H, Ws=W, Ho=H, Wo=W, lens=good, fisheye=0, fxo=20.0, fyo=20.0, s=p(src), d=p(dst)):
        return L.clmgs_undistort_u8(_lib.stream(), planes, Hs, Ws, Ho, Wo, None if lens is None else rec(lens), fisheye,
                                    fxo, fyo, s, None, d, p(valid), p(count))

    def u16(Hs=H, Ws=W, Ho=H, Wo=W, lens=good, fxo=20.0, fyo=20.0, s=p(src16), d=p(dst16)):
        return L.clmgs_undistort_u16(_lib.stream(), Hs, Ws, Ho, Wo, None if lens is None else rec(lens), 0, fxo, fyo, s, d)

    nan, inf = float("nan"), float("inf")
    bad = [dict(Hs=0), dict(Ws=0), dict(Ho=0), dict(Wo=0), dict(s=None), dict(d=None), dict(lens=None),
           dict(lens=good[:4] + [nan] + good[5:]), dict(lens=[inf] + good[1:]), dict(lens=good[:9] + [-inf]),
           dict(fxo=nan), dict(fyo=inf), dict(fxo=0.0)]
    for kw in bad + [dict(planes=0), dict(planes=-1), dict(fisheye=2), dict(d=p(src))]:
        assert u8(**kw) == 10001, kw
    for kw in bad:
        assert u16(**kw) == 10001, kw
    torch.cuda.synchronize()
    assert bool((dst == 77).all()) and bool((valid == 77).all()) and int(count.item()) == 77
    assert bool((dst16.view(torch.int16) == 77).all())
    with pytest.raises(_lib.ClmgsError, match="invalid argument"):
        _lib.check(u8(planes=0))
    assert u8() == 0 and u16() == 0   # and the good call goes through: an identity lens
    torch.cuda.synchronize()
    assert torch.equal(dst, src) and int(count.item()) == H * W and torch.equal(dst16.view(torch.int16), src16.view(torch.int16))


# ---------------------------------------------------------------------------------------------------------- end to end
CAMERAS = """1 SIMPLE_RADIAL 24 16 30.0 12.4 7.7 -0.11
2 SIMPLE_RADIAL 24 16 26.0 11.6 8.3 -0.09
3 SIMPLE_RADIAL 24 16 31.0 12.3 8.2 -0.12
"""
LENS_OF = {1: (30.0, 12.4, 7.7, -0.11), 2: (26.0, 11.6, 8.3, -0.09), 3: (31.0, 12.3, 8.2, -0.12)}


def _distort(ideal, f_r, lens, H, W):
    """The forward model on the CPU: the H x W image a SIMPLE_RADIAL lens (f, cx, cy, k) makes of the scene that the
    centred pinhole `ideal` [3,Hr,Wr] (focal length f_r) shows.  A distorted pixel's ray is found by inverting
    xd = x (1 + k r^2) with a fixed-point iteration, then looked up bilinearly."""
    f, cx, cy, k = lens
    Hr, Wr = ideal.shape[1:]
    jd, id_ = np.meshgrid(np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64))
    xd, yd = (jd + 0.5 - cx) / f, (id_ + 0.5 - cy) / f
    x, y = xd.copy(), yd.copy()
    for _ in range(50):
        s = 1.0 + k * (x * x + y * y)
        x, y = xd / s, yd / s
    u, v = x * f_r + Wr / 2.0 - 0.5, y * f_r + Hr / 2.0 - 0.5
    assert u.min() >= 0 and u.max() <= Wr - 1 and v.min() >= 0 and v.max() <= Hr - 1
    x0, y0 = np.minimum(np.floor(u).astype(int), Wr - 2), np.minimum(np.floor(v).astype(int), Hr - 2)
    a, b = u - x0, v - y0
    p = ideal.astype(np.float64)
    val = (1 - b) * ((1 - a) * p[:, y0, x0] + a * p[:, y0, x0 + 1]) + b * ((1 - a) * p[:, y0 + 1, x0] + a * p[:, y0 + 1, x0 + 1])
    return np.clip(np.rint(val), 0, 255).astype(np.uint8)


@pytest.fixture(scope="module")
def distorted_scene(tmp_path_factory):
    """colmap_tiny with SIMPLE_RADIAL cameras (off-centre principal points), a blob of points in front of every camera and
    images RENDERED by the engine from a hidden model through wide pinholes, then distorted by the forward model."""
    from PIL import Image
    from clm_gs_amd import utils
    from clm_gs_amd.cameras import Camera
    from clm_gs_amd.colmap_scene import focal_to_fov, load_colmap_scene
    from clm_gs_amd.strategies.clm_offload import GaussianModelCLMOffload, clm_offload_eval_one_cam
    work = tmp_path_factory.mktemp("undistort") / "scene"
    shutil.copytree(SRC, work)
    shutil.rmtree(work / "sparse_txt")
    os.remove(work / "sparse" / "0" / "cameras.bin")
    with open(work / "sparse" / "0" / "cameras.txt", "w") as f:
        f.write(CAMERAS)
    poses = load_colmap_scene(str(work), device=DEV, load_images=False, undistort=True)
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
    args = utils.default_args(bsz=4, clm_offload=True)
    utils.set_args(args)
    Hr, Wr = 64, 80   # the wide pinhole: twice the lens' focal length, a margin of 8 source pixels on every side
    utils.set_img_size(Hr, Wr)
    utils.set_cur_iter(1)
    scene = load_colmap_scene(str(work), device=DEV, load_images=False, undistort=True)
    truth = GaussianModelCLMOffload(3, only_for_rendering=True)
    truth.args = args
    truth.create_from_pcd(scene.point_cloud, scene.cameras_extent)
    truth.active_sh_degree = 0
    with torch.no_grad():
        truth._scaling += 0.7
        truth._opacity += 2.0
    for c in scene.train_cameras:
        f_r = 2.0 * LENS_OF[c.uid][0]
        wide = Camera(c.uid, c.world_view_transform.t().cpu(), focal_to_fov(f_r, Wr), focal_to_fov(f_r, Hr), Wr, Hr, device=DEV)
        img = (clm_offload_eval_one_cam(wide, truth, None, None).clamp(0, 1) * 255).round().to(torch.uint8)
        assert int(img.max()) > 0, "every camera sees the blob in front of it"
        Image.fromarray(_distort(img.cpu().numpy(), f_r, LENS_OF[c.uid], 16, 24).transpose(1, 2, 0)).save(
            work / "images" / (c.image_name + ".png"))
    utils.set_img_size(16, 24)
    return work, len(pts)


@pytest.mark.parametrize("strategy", ["no_offload", "clm_offload"])
def test_training_from_a_distorted_colmap_directory(distorted_scene, tmp_path, strategy):
    from PIL import Image
    from clm_gs_amd import trainer
    from clm_gs_amd.io_ply import load_ply
    work, n_pts = distorted_scene
    with pytest.raises(ValueError, match="not handled"):
        trainer.train_from_colmap(str(work), str(tmp_path / "plain"), strategy=strategy, iterations=8, bsz=4)
    out = tmp_path / "out"
    gaussians, sc, timer = trainer.train_from_colmap(
        str(work), str(out), strategy=strategy, iterations=160, eval=True, test_iterations=(1, 157), bsz=4,
        disable_auto_densification=True, undistort=True)
    log = open(out / "python_ws=1_rk=0.log").read()
    for cid, (f, cx, cy, k) in LENS_OF.items():   # the per-camera line
        line = next(ln for ln in log.splitlines() if ln.startswith(f"undistort: camera {cid} SIMPLE_RADIAL"))
        assert "%.6g" % k in line and "of the pixels have no source" in line and "24x16" in line, line
    assert len(sc.train_cameras) == 10 and len(sc.test_cameras) == 2
    for c in sc.train_cameras + sc.test_cameras:   # centred pinholes with the kernel's masks and counts
        f, cx, cy, k = LENS_OF[c.uid]
        rec = (f, f, cx, cy, k, 0, 0, 0, 0, 0)
        png = np.asarray(Image.open(work / "images" / (c.image_name + ".png")).convert("RGB")).transpose(2, 0, 1)
        ref, ref_valid, band = R.undistort(png, rec, False, f, f)
        assert 0 < np.count_nonzero(ref_valid) < 16 * 24   # (a rendered image is no seeded input: its band is what it is)
        assert c.loss_mask is not None and c.loss_mask.is_cuda and c.loss_mask.dtype == torch.uint8
        assert c.loss_mask_count == int(torch.count_nonzero(c.loss_mask))
        _hold_to_reference(c.original_image.cpu().numpy(), c.loss_mask.cpu().numpy(), c.loss_mask_count, ref, ref_valid,
                           band, c.image_name)
        assert c.K[0, 2].item() == 12.0 and c.K[1, 2].item() == 8.0 and abs(c.K[0, 0].item() - f) < 1e-4
    psnr = [float(ln.split("PSNR ")[1]) for ln in log.splitlines() if "Evaluating train:" in ln]
    print("training PSNR over the counted pixels, first and last evaluation:", psnr)
    assert len(psnr) == 2 and psnr[1] > psnr[0], psnr
    assert "Evaluating test:" in log and "end2end total_time:" in log
    saved = load_ply(str(out / "point_cloud" / "iteration_160" / "point_cloud.ply"))
    assert saved["xyz"].shape[0] == gaussians.get_xyz.shape[0] == n_pts
