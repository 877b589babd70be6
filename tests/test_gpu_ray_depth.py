"""-m gpu: the ray depth -- the per-pixel pass (csrc/ray_depth.hip) against the float64 restatement of
tests/ray_depth_reference.py bit for bit, the C entry's refusals and bounds, render mode "RGB+RD" on the engines against the
analytic tilted plane, and the mesh, trajectory and orthophoto command lines.

No tolerance is tuned here: the operator is compared bit for bit; the engines' maps with the bound derived in the
reference's docstring (GEOM + PLACE, computed from the rows the model hands the kernels) plus one float32 ulp of the
depth.  Every test prints the figures it asserts on.
"""
import ctypes
import functools
import json
import math
import os

import numpy as np
import pytest
import torch

from tests import ray_depth_reference as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(1, 1), (17, 17), (48, 64)]  # (H, W)
ROWS = [1, 65, 300]
CANARY, PAD = -7.5, 64
CLMGS_EINVAL = 10001  # include/clmgs.h


def _bits(t):
    return t.view(torch.int32)


# ------------------------------------------------------------------------------------------- 1. the operator
@functools.lru_cache(maxsize=None)
def op_case(Hh, Ww, N, ortho, C=2):
    """Seeded rows (scales 1e-6 .. 1e2 and, from 65 rows on, a zero and a denormal scale; unnormalised quaternions), C rigid
    cameras, ids uniform over [-1, N) with every tenth pixel >= N, centre depths: float32 numpy, and the reference map."""
    rng = np.random.default_rng(1000 * N + 10 * Hh + int(ortho))
    viewmats = np.zeros((C, 4, 4), dtype=np.float32)
    Ks = np.zeros((C, 3, 3), dtype=np.float32)
    for c in range(C):
        q = rng.normal(size=4) * np.array([3.0, 0.4, 0.4, 0.4])  # a moderate turn away from the identity
        viewmats[c, :3, :3] = np.stack(R.quat_to_rotmat(q)).reshape(3, 3)
        viewmats[c, :3, 3] = rng.normal(size=3) * 0.5 + np.array([0.0, 0.0, 6.0])
        viewmats[c, 3, 3] = 1.0
        f = rng.uniform(20.0, 200.0, 2)
        Ks[c] = np.array([[f[0], 0, Ww / 2 + rng.normal()], [0, f[1], Hh / 2 + rng.normal()], [0, 0, 1]])
    means = (rng.normal(size=(N, 3)) * 2.0).astype(np.float32)
    quats = (rng.normal(size=(N, 4)) * 10.0 ** rng.uniform(-1, 1, (N, 1))).astype(np.float32)
    scales = (10.0 ** rng.uniform(-6, 2, (N, 3))).astype(np.float32)
    if N >= 65:
        scales[3, 1] = 0.0
        scales[7, 2] = 1e-42
    ids = rng.integers(-1, N, (C, Hh, Ww)).astype(np.int32)
    wild = rng.random((C, Hh, Ww)) < 0.1
    ids[wild] = rng.choice(np.array([N, N + 5, 2 ** 31 - 1, -2 ** 31, -7], dtype=np.int64), int(wild.sum())).astype(np.int32)
    md = rng.uniform(0.5, 10.0, (C, Hh, Ww)).astype(np.float32)
    model = "ortho" if ortho else "pinhole"
    ref = R.ray_depth_map(means, quats, scales, viewmats, Ks, md, ids, 0.01, model)
    return dict(means=means, quats=quats, scales=scales, viewmats=viewmats, Ks=Ks, ids=ids, md=md, model=model, ref=ref)


def _operator(case, dev, cams=slice(None)):
    from clm_gs_amd import gsplat as G
    t = {k: torch.from_numpy(case[k]).to(dev) for k in ("means", "quats", "scales", "viewmats", "Ks", "ids", "md")}
    out = G.ray_gaussian_depth(t["means"], t["quats"], t["scales"], t["viewmats"][cams], t["Ks"][cams], t["md"][cams].contiguous(),
                               t["ids"][cams].contiguous(), near_plane=0.01, camera_model=case["model"])
    torch.cuda.synchronize()
    return out.cpu()


def _entry(case, dev, **over):
    """The C entry on a canary-padded output -> (status, the whole buffer on the CPU, C, H, W)."""
    from clm_gs_amd import _lib, gsplat as G
    from clm_gs_amd._lib import dptr, stream
    L = _lib.lib()
    t = {k: torch.from_numpy(case[k]).to(dev) for k in ("means", "quats", "scales", "viewmats", "Ks", "ids", "md")}
    C, Hh, Ww = case["ids"].shape
    cams = G.ray_camera_table(t["viewmats"], t["Ks"])
    buf = torch.full((C * Hh * Ww + 2 * PAD,), CANARY, dtype=torch.float32, device=dev)
    out = buf[PAD:PAD + C * Hh * Ww]
    a = dict(C=C, N=case["means"].shape[0], H=Hh, W=Ww, means=dptr(t["means"]), quats=dptr(t["quats"]), scales=dptr(t["scales"]),
             cams=dptr(cams), ids=dptr(t["ids"]), md=dptr(t["md"]), near=0.01, model=G.RAY_CAMERA_MODELS[case["model"]],
             out=ctypes.c_void_p(out.data_ptr()))
    for k, v in over.items():
        a[k] = v(t, cams) if callable(v) else v
    status = L.clmgs_ray_depth(stream(), a["C"], a["N"], a["H"], a["W"], a["means"], a["quats"], a["scales"], a["cams"], a["ids"],
                               a["md"], a["near"], a["model"], a["out"])
    torch.cuda.synchronize()
    return status, buf.cpu(), C, Hh, Ww


@pytest.mark.parametrize("ortho", [False, True], ids=["pinhole", "ortho"])
@pytest.mark.parametrize("N", ROWS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[1]}x{s[0]}")
def test_operator_matches_the_reference_bit_for_bit(dev, shape, N, ortho):
    case = op_case(shape[0], shape[1], N, ortho)
    ref = torch.from_numpy(case["ref"])
    got = _operator(case, dev)
    assert got.dtype == torch.float32 and got.shape == ref.shape and not got.requires_grad
    outside = torch.from_numpy((case["ids"] < 0) | (case["ids"] >= N))
    differ = int((_bits(got) != _bits(ref)).sum())
    fell_back = int(((_bits(got) == _bits(torch.from_numpy(case["md"]))) & ~outside).sum())
    print(f"{shape[1]}x{shape[0]} N={N} {case['model']}: {differ} of {got.numel()} pixels differ in bits; {int(outside.sum())} ids "
          f"outside [0, N), {fell_back} fallbacks to the centre depth")
    assert differ == 0
    assert bool((_bits(got)[outside] == 0).all())  # +0.0 exactly
    again = _operator(case, dev)                   # two calls: the same bits
    assert torch.equal(_bits(got), _bits(again))
    for c in range(case["ids"].shape[0]):          # each camera alone
        one = _operator(case, dev, cams=slice(c, c + 1))
        assert torch.equal(_bits(one[0]), _bits(got[c]))
    status, buf, C, Hh, Ww = _entry(case, dev)     # the entry itself, between canaries
    n = C * Hh * Ww
    assert status == 0 and bool((buf[:PAD] == CANARY).all()) and bool((buf[PAD + n:] == CANARY).all())
    assert torch.equal(_bits(buf[PAD:PAD + n].reshape(C, Hh, Ww)), _bits(ref))


def test_operator_uses_the_formula_on_most_pixels():
    """(CPU-side property of the cases: they exercise t*, not the fallback or the id test)"""
    case = op_case(48, 64, 300, False)
    inside = (case["ids"] >= 0) & (case["ids"] < 300)
    used = inside & (case["ref"] != case["md"])
    print(f"{int(used.sum())} of {used.size} pixels carry a ray depth")
    assert used.sum() > 0.5 * used.size


def test_entry_refusals_write_nothing_and_no_rows_fill_zeros(dev):
    case = op_case(17, 17, 65, False)
    big = 2 ** 16
    refusals = dict(
        null_out=dict(out=None), null_ids=dict(ids=None), null_centre_depth=dict(md=None), null_cameras=dict(cams=None),
        null_means=dict(means=None), null_quats=dict(quats=None), null_scales=dict(scales=None),
        negative_C=dict(C=-1), negative_N=dict(N=-1), negative_H=dict(H=-1), negative_W=dict(W=-1),
        pixels_32bit=dict(C=big, H=big, W=1), image_32bit=dict(C=1, H=big, W=big), model_2=dict(model=2), model_negative=dict(model=-1),
        cameras_misaligned=dict(cams=lambda t, cams: ctypes.c_void_p(cams.data_ptr() + 4)))
    for what, kw in refusals.items():
        status, buf, *_ = _entry(case, dev, **kw)
        assert status == CLMGS_EINVAL, (what, status)
        assert bool((buf == CANARY).all()), what  # refused before anything is written
    # nothing to do: no pixel is written, no pointer is needed
    for kw in (dict(C=0), dict(H=0), dict(W=0)):
        status, buf, *_ = _entry(case, dev, out=None, ids=None, md=None, cams=None, means=None, quats=None, scales=None, **kw)
        assert status == 0 and bool((buf == CANARY).all())
    # no rows: zeros to every pixel, no row pointer is read
    status, buf, C, Hh, Ww = _entry(case, dev, N=0, means=None, quats=None, scales=None)
    n = C * Hh * Ww
    assert status == 0 and bool((_bits(buf[PAD:PAD + n]) == 0).all())
    assert bool((buf[:PAD] == CANARY).all()) and bool((buf[PAD + n:] == CANARY).all())


def test_operator_detaches_and_refuses_an_unknown_model(dev):
    from clm_gs_amd import gsplat as G
    case = op_case(17, 17, 65, False)
    t = {k: torch.from_numpy(case[k]).to(dev) for k in ("means", "quats", "scales", "viewmats", "Ks", "ids", "md")}
    out = G.ray_gaussian_depth(t["means"].requires_grad_(), t["quats"].requires_grad_(), t["scales"].requires_grad_(),
                               t["viewmats"], t["Ks"], t["md"], t["ids"], camera_model="pinhole")
    assert not out.requires_grad and torch.equal(_bits(out.cpu()), _bits(torch.from_numpy(case["ref"])))
    with pytest.raises(ValueError, match="camera_model"):
        G.ray_gaussian_depth(t["means"], t["quats"], t["scales"], t["viewmats"], t["Ks"], t["md"], t["ids"], camera_model="fisheye")
    empty = G.ray_gaussian_depth(t["means"][:0], t["quats"][:0], t["scales"][:0], t["viewmats"], t["Ks"], t["md"], t["ids"])
    assert bool((_bits(empty) == 0).all())


# ------------------------------------------------------------------------------------------- 2. the engines
W, H = R.W, R.H
FOVX, FOVY = 2 * math.atan(W / (2 * R.FOCAL)), 2 * math.atan(H / (2 * R.FOCAL))
CAM_HEIGHT = R.PLANE_DEPTH
RM = np.diag([1.0, -1.0, -1.0])  # the nadir camera's rotation, its own inverse
B_HALF = 1.25  # the plane's half width along y: with the 4 s footprint it reaches |y| = 2.05, the view's rim at depth 5
ENGINES = [("no_offload", "hbm"), ("naive_offload", "hbm"), ("clm_offload", "hbm"), ("clm_offload", "host")]


class _Scene:
    cameras_extent = 5.0


def _plane_rows_world():
    """The tilted plane in the world of a nadir camera at (0, 0, CAM_HEIGHT): z_w = -SLOPE x_w."""
    return R.plane_rows(a_half=5.0, b_half=B_HALF, world_from_cam=(RM, np.array([0.0, 0.0, CAM_HEIGHT])))


def _camera(kind, uid, x, y, dev):
    from clm_gs_amd.cameras import Camera, OrthoCamera
    Rm = torch.tensor(RM, dtype=torch.float32)
    w2c = torch.eye(4)
    w2c[:3, :3] = Rm
    w2c[:3, 3] = -Rm @ torch.tensor([x, y, CAM_HEIGHT])
    if kind == "ortho":
        return OrthoCamera(uid, w2c, R.ORTHO_PPU, W, H, image_name=f"ortho_{uid}")
    return Camera(uid, w2c, FOVX, FOVY, W, H, device=dev)


def _model(strategy, residency, dev, mode="classic"):
    from clm_gs_amd import utils
    args = utils.default_args(bsz=4, sh_residency=residency, rasterize_mode=mode)
    setattr(args, strategy, True)
    utils.set_args(args)
    utils.set_img_size(H, W)
    utils.set_cur_iter(1)
    if strategy == "no_offload":
        from clm_gs_amd.strategies.no_offload import GaussianModelNoOffload as M
    elif strategy == "naive_offload":
        from clm_gs_amd.strategies.naive_offload import GaussianModelNaiveOffload as M
    else:
        from clm_gs_amd.strategies.clm_offload import GaussianModelCLMOffload as M
    xyz, quats, scales, _, _ = _plane_rows_world()
    n = xyz.shape[0]
    shs = torch.zeros(n, 16, 3)
    shs[:, 0, :] = torch.from_numpy(np.stack([xyz[:, 0] * 0.2, xyz[:, 1] * 0.3, np.full(n, 0.5)], 1)).float()
    m = M(3)
    m.create_from_tensors(torch.from_numpy(xyz).to(dev), shs.reshape(n, 48).to(dev), torch.log(torch.from_numpy(scales)).to(dev),
                          torch.from_numpy(quats).to(dev), torch.full((n, 1), 6.0, device=dev), spatial_lr_scale=1.0)
    m.active_sh_degree = 3
    m.training_setup(args)
    return args, m


def _plane_in_camera(cam, m, dev):
    """For a camera and the model's activated rows: the camera record the engine's K and view matrix give, the plane's
    analytic depth per pixel and the derived bound."""
    from clm_gs_amd.cameras import camera_model
    from clm_gs_amd.strategies.base_engine import fov_camera
    ortho = camera_model(cam) == "ortho"
    viewmat, K, _ = fov_camera(cam, dev)
    rec = R.camera_table(viewmat.detach().cpu().numpy()[None], K.detach().cpu().numpy()[None])[0]
    _, _, _, n_w, c0_w = _plane_rows_world()
    Rv, t = rec[:12].reshape(3, 4)[:, :3], rec[:12].reshape(3, 4)[:, 3]
    n_cam = Rv @ n_w
    hit = R.plane_hit(rec, ortho, n_cam, c0_w + float(n_cam @ t))
    rows = [x.detach().cpu().numpy() for x in (m.get_xyz, m.get_rotation, m.get_scaling)]
    bnd, geom, place = R.bound(rec, ortho, n_cam, rows[0], rows[1], rows[2], n_w, c0_w)
    return hit, bnd, geom, place


def _operator_on_the_engine_ids(cam, m, args, dev, antialiased=False):
    """What camera_forward_ops runs, op by op, on all rows -> (median depth, ray depth), [1,H,W] on the device."""
    from clm_gs_amd import gsplat as G
    from clm_gs_amd.cameras import camera_model
    from clm_gs_amd.strategies.base_engine import fov_camera
    model = camera_model(cam)
    viewmat, K, _ = fov_camera(cam, dev)
    radii, m2, depths, conics, comps = G.fully_fused_projection(
        m.get_xyz, None, m.get_rotation, m.get_scaling, viewmat[None], K[None], W, H, radius_clip=args.radius_clip,
        calc_compensations=antialiased, **({"camera_model": "ortho"} if model == "ortho" else {}))
    tw, th = math.ceil(W / 16), math.ceil(H / 16)
    _, isect_ids, fids = G.isect_tiles(m2, radii, depths, 16, tw, th)
    off = G.isect_offset_encode(isect_ids, 1, tw, th)
    op = m.get_opacity.squeeze(1).unsqueeze(0)
    md, ids = G.rasterize_median_depth(m2, conics, op * comps if antialiased else op, depths, W, H, 16, off, fids)
    rd = G.ray_gaussian_depth(m.get_xyz, m.get_rotation, m.get_scaling, viewmat[None], K[None], md, ids, camera_model=model)
    return md, rd


@pytest.fixture(scope="module")
def engine_maps(dev):
    """The tilted plane through the four eval entries, pinhole and orthographic: (image, depth, alpha) of "RGB+RD" and of
    "RGB+MD" on the CPU; per camera kind the analytic depth, the bound and the operator's own map on the engine's ids."""
    from clm_gs_amd import utils
    from clm_gs_amd.render_trajectory import eval_one_cam
    out = {}
    try:
        for strategy, residency in ENGINES:
            args, m = _model(strategy, residency, dev)
            for kind in ("pinhole", "ortho"):
                cam = _camera(kind, 0, 0.0, 0.0, dev)
                with torch.no_grad():
                    rd = tuple(t.clone().cpu() for t in eval_one_cam(cam, m, None, args, _Scene, render_mode="RGB+RD"))
                    md = tuple(t.clone().cpu() for t in eval_one_cam(cam, m, None, args, _Scene, render_mode="RGB+MD"))
                    if kind not in out:
                        out[kind] = _plane_in_camera(cam, m, dev) + tuple(
                            t.cpu() for t in _operator_on_the_engine_ids(cam, m, args, dev))
                torch.cuda.synchronize()
                out[(strategy, residency, kind)] = dict(rd=rd, md=md)
    finally:
        utils.set_args(utils.default_args())
    return out


@pytest.mark.parametrize("kind", ["pinhole", "ortho"])
@pytest.mark.parametrize("strategy,residency", ENGINES)
def test_engines_put_the_depth_on_the_plane(dev, engine_maps, strategy, residency, kind):
    r = engine_maps[(strategy, residency, kind)]
    hit, bnd, geom, place, op_md, op_rd = engine_maps[kind]
    (img, depth, alpha), (img_m, depth_m, alpha_m) = r["rd"], r["md"]
    assert depth.shape == alpha.shape == (1, H, W) and depth.dtype == torch.float32
    # image and alpha are those of "RGB+MD"; the depth is 0.0 exactly where the median depth is
    assert torch.equal(_bits(img), _bits(img_m)) and torch.equal(_bits(alpha), _bits(alpha_m))
    empty = _bits(depth_m[0]) == 0
    assert torch.equal(_bits(depth[0]) == 0, empty)
    seen = (~empty).numpy()
    assert 0.5 * W * H < seen.sum() < W * H  # the plane fills most of the view and leaves some of it empty
    d, dm = depth[0].numpy().astype(np.float64), depth_m[0].numpy().astype(np.float64)
    ulp = np.spacing(hit.astype(np.float32)).astype(np.float64)
    err, err_m = np.abs(d - hit)[seen], np.abs(dm - hit)[seen]
    print(f"{strategy}/{residency}/{kind}: {int(seen.sum())} pixels; bound {bnd:.3e} (GEOM {geom:.3e} + PLACE {place:.3e}) + ulp "
          f"{ulp[seen].max():.2e}; ray depth misses the plane by {err.max():.3e}, the median depth by {err_m.max():.3e}")
    assert bool((np.abs(d - hit) <= bnd + ulp)[seen].all())
    assert err_m.max() > 100 * bnd
    # the operator on rasterize_median_depth's ids for the same rows gives the engine's map, and the engines agree
    assert torch.equal(_bits(depth_m), _bits(op_md)) and torch.equal(_bits(depth), _bits(op_rd))


def test_training_entries_refuse_the_mode(dev):
    from clm_gs_amd import utils
    from clm_gs_amd.strategies.base_engine import pipeline_forward_one_step
    from clm_gs_amd.strategies.clm_offload.engine import pipeline_forward_one_step_shs_inplace
    from clm_gs_amd.strategies.no_offload import baseline_accumGrads_micro_step
    try:
        args, m = _model("no_offload", "hbm", dev)
        cam = _camera("pinhole", 0, 0.0, 0.0, dev)
        tensors = (m.get_xyz, m.get_opacity, m.get_scaling, m.get_rotation, m.get_features)
        with pytest.raises(ValueError, match="RGB\\+RD"):
            baseline_accumGrads_micro_step(*tensors, 3, cam, None, mode="train", render_mode="RGB+RD")
        xyz, opa, sca, rot, shs = tensors
        with pytest.raises(ValueError, match="RGB\\+RD"):
            pipeline_forward_one_step(opa, sca, rot, xyz, shs.reshape(-1, 48), cam, _Scene, m, None, None, eval=False,
                                      render_mode="RGB+RD")
        with pytest.raises(ValueError, match="RGB\\+RD"):
            pipeline_forward_one_step_shs_inplace(opa, sca, rot, xyz, shs.reshape(-1, 48), cam, _Scene, m, None, None,
                                                  render_mode="RGB+RD")
        with pytest.raises(ValueError, match="render_mode must be one of"):
            baseline_accumGrads_micro_step(*tensors, 3, cam, None, mode="eval", render_mode="RGB+XD")
    finally:
        utils.set_args(utils.default_args())


def test_antialiased_agrees_with_the_operator_on_the_same_ids(dev):
    from clm_gs_amd import utils
    from clm_gs_amd.render_trajectory import eval_one_cam
    try:
        args, m = _model("no_offload", "hbm", dev, mode="antialiased")
        cam = _camera("pinhole", 0, 0.0, 0.0, dev)
        with torch.no_grad():
            _, depth, _ = eval_one_cam(cam, m, None, args, _Scene, render_mode="RGB+RD")
            _, depth_m, _ = eval_one_cam(cam, m, None, args, _Scene, render_mode="RGB+MD")
            md, rd = _operator_on_the_engine_ids(cam, m, args, dev, antialiased=True)
            _, plain = _operator_on_the_engine_ids(cam, m, args, dev, antialiased=False)
        torch.cuda.synchronize()
        assert torch.equal(_bits(depth_m), _bits(md)) and torch.equal(_bits(depth), _bits(rd))
        print(f"antialiased: {int((rd != plain).sum())} of {W * H} pixels differ from the classic ray depth")
    finally:
        utils.set_args(utils.default_args())


# ------------------------------------------------------------------------------------------- 3. the mesh
PLANE_VOXEL = 0.05
MESH_BOUNDS = (-1.0, -0.9, -0.9, 1.0, 0.9, 0.9)
MESH_CAM_XY = ((0.03, -0.05), (-0.08, 0.06), (0.07, 0.04), (-0.05, -0.07), (0.0, 0.01))


def test_build_mesh_ray_against_median(dev, tmp_path):
    from clm_gs_amd import io_ply, mesh_model, utils
    from clm_gs_amd.render_ortho import map_frame
    try:
        args, m = _model("no_offload", "hbm", dev)
        cams = [_camera("pinhole", i, x, y, dev) for i, (x, y) in enumerate(MESH_CAM_XY)]
        _, _, _, n_w, c0_w = _plane_rows_world()
        metas, dist = {}, {}
        for mode in ("ray", "median"):
            path = str(tmp_path / mode / "mesh.ply")
            with open(os.devnull, "w") as log:
                metas[mode] = mesh_model.build_mesh(m, cams, args, path, PLANE_VOXEL, frame=map_frame(), bounds=MESH_BOUNDS,
                                                    log=log, depth_mode=mode)
            verts, _, faces = io_ply.load_mesh_ply(path)
            assert metas[mode] == json.load(open(mesh_model.json_path(path)))
            dist[mode] = np.abs(verts.astype(np.float64) @ n_w - c0_w)
            print(f"mesh/{mode}: V {len(verts)} F {len(faces)}; largest vertex-to-plane distance {dist[mode].max():.5f} "
                  f"(mean {dist[mode].mean():.5f}), voxel {PLANE_VOXEL}")
            assert len(verts) > 500 and len(faces) > 500
        assert float(dist["ray"].max()) <= PLANE_VOXEL         # every vertex within one voxel of the plane
        assert float(dist["ray"].max()) < float(dist["median"].max())
        assert metas["ray"]["depth_mode"] == "ray" and metas["median"]["depth_mode"] == "median"
        # the sparse volume writes the dense path's bytes in this mode too
        sparse = str(tmp_path / "sparse" / "mesh.ply")
        with open(os.devnull, "w") as log:
            meta_s = mesh_model.build_mesh(m, cams, args, sparse, PLANE_VOXEL, frame=map_frame(), bounds=MESH_BOUNDS, log=log,
                                           depth_mode="ray", sparse=True)
        assert meta_s["depth_mode"] == "ray" and "sparse" in meta_s
        assert open(sparse, "rb").read() == open(str(tmp_path / "ray" / "mesh.ply"), "rb").read()
    finally:
        utils.set_args(utils.default_args())


def test_mesh_cli_with_ray_depth(dev, tmp_path, capsys):
    from clm_gs_amd import io_ply, mesh_model, utils
    from tests.test_gpu_tsdf import _shell_rows
    scene = os.path.join(ROOT, "tests", "golden", "colmap_tiny")
    rows = _shell_rows()
    ply = str(tmp_path / "shell.ply")
    io_ply.save_ply(ply, rows["xyz"], rows["shs48"], rows["opacity"], rows["scaling"], rows["rotation"])
    try:
        mesh = str(tmp_path / "out" / "mesh.ply")
        assert mesh_model.main(["-m", ply, "-s", scene, "-o", mesh, "--voxel", "1", "--min_weight", "1", "--no_offload",
                                "--depth_mode", "ray", "--bounds", "-14", "-14", "-14", "14", "14", "14"]) == 0
        line = capsys.readouterr().out
        assert "render" in line and "integration" in line, line
        verts, colours, faces = io_ply.load_mesh_ply(mesh)
        meta = json.load(open(mesh[:-4] + ".json"))
        assert meta["depth_mode"] == "ray" and meta["vertices"] == len(verts) > 0 and meta["faces"] == len(faces) > 0
        r = np.linalg.norm(verts.astype(np.float64), axis=1)  # the surface found is the shell
        assert float(np.abs(r - 12.0).max()) < 4.0, (float(r.min()), float(r.max()))
    finally:
        utils.set_args(utils.default_args())


# ------------------------------------------------------------------------------------------- 4. trajectory and orthophoto
def _save_plane(path):
    from clm_gs_amd import io_ply
    xyz, quats, scales, _, _ = _plane_rows_world()
    n = xyz.shape[0]
    shs = torch.zeros(n, 16, 3)
    shs[:, 0, 2] = 0.5
    io_ply.save_ply(path, torch.from_numpy(xyz), shs.reshape(n, 48), torch.full((n, 1), 6.0), torch.log(torch.from_numpy(scales)),
                    torch.from_numpy(quats))


def test_render_trajectory_writes_the_ray_depth(dev, tmp_path):
    from clm_gs_amd import render_trajectory as RT, utils
    from clm_gs_amd.strategies.no_offload import GaussianModelNoOffload as M
    ply, out = str(tmp_path / "plane.ply"), tmp_path / "frames"
    _save_plane(ply)
    try:
        common = ["-m", ply, "--no_offload", "--n_frames", "1", "--manual_height", str(CAM_HEIGHT), "--width", str(W),
                  "--height", str(H), "--fovx", str(FOVX), "--hull", "0,0", "0.5,0", "0,0", "--render_depth"]
        assert RT.main(common + ["--output_dir", str(out), "--depth_mode", "ray"]) == 0
        got = np.load(out / "depth_00000.npy")
        assert (out / "depth_00000.png").exists() and (out / "frame_00000.png").exists()
        args = utils.default_args(bsz=4)
        args.no_offload = True
        utils.set_args(args)
        utils.set_img_size(H, W)
        m = M(3, only_for_rendering=True)
        m.load_ply(ply)
        m.active_sh_degree = m.max_sh_degree
        cam = RT.polyline_trajectory(RT.R_LOOK_DOWN, CAM_HEIGHT, 1, FOVX, FOVY, W, H, ((0.0, 0.0), (0.5, 0.0), (0.0, 0.0)))[0]
        with torch.no_grad():
            _, depth, _ = RT.eval_one_cam(cam, m, None, args, None, render_mode="RGB+RD")
            _, depth_m, _ = RT.eval_one_cam(cam, m, None, args, None, render_mode="RGB+MD")
        assert got.dtype == np.float32 and np.array_equal(got, depth[0].cpu().numpy())
        assert not np.array_equal(got, depth_m[0].cpu().numpy())
    finally:
        utils.set_args(utils.default_args())


def test_render_ortho_height_from_the_ray_depth(dev, tmp_path):
    from clm_gs_amd import render_ortho, utils
    ply = str(tmp_path / "plane.ply")
    _save_plane(ply)
    try:
        common = ["-m", ply, "--no_offload", "--gsd", "0.05", "--bounds", "-1.0", "-0.8", "1.0", "0.8", "--camera_height",
                  str(CAM_HEIGHT), "--tile", "64"]
        assert render_ortho.main(common + ["--output_dir", str(tmp_path / "rd"), "--depth_mode", "ray"]) == 0
        assert render_ortho.main(common + ["--output_dir", str(tmp_path / "md"), "--depth_mode", "median"]) == 0
        h_rd, h_md = np.load(tmp_path / "rd" / "ortho_height.npy"), np.load(tmp_path / "md" / "ortho_height.npy")
        meta_rd, meta_md = json.load(open(tmp_path / "rd" / "ortho.json")), json.load(open(tmp_path / "md" / "ortho.json"))
        assert meta_rd.pop("depth_mode") == "ray" and meta_md.pop("depth_mode") == "median" and meta_rd == meta_md
        assert np.array_equal(np.load(tmp_path / "rd" / "ortho_alpha.npy"), np.load(tmp_path / "md" / "ortho_alpha.npy"))
        assert h_rd.shape == h_md.shape == (32, 40) and np.isfinite(h_rd).all()
        # map pixel (row, col) looks down at x_w = -1 + (col + 0.5) gsd: the plane's height there is -SLOPE x_w
        x_w = -1.0 + (np.arange(40) + 0.5) * 0.05
        want = np.broadcast_to(-R.SLOPE * x_w, h_rd.shape)
        e_rd, e_md = np.abs(h_rd - want).max(), np.abs(h_md - want).max()
        print(f"ortho: the height from the ray depth misses the plane by {e_rd:.3e}, from the median depth by {e_md:.3e}")
        # the derived bound for the rows as the .ply holds them under a camera that looks straight down (rays along -z_w),
        # plus one float32 ulp of a depth in [4, 8); camera_height - depth is then exact (Sterbenz)
        xyz, quats, scales, n_w, c0_w = _plane_rows_world()
        bnd, _, _ = R.bound(R.ortho_record(), True, RM @ n_w, xyz, quats, np.exp(np.log(scales)), n_w, c0_w)
        assert e_rd <= bnd + 2.0 ** -21
        assert e_md > 100 * bnd
    finally:
        utils.set_args(utils.default_args())
