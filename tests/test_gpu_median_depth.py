"""-m gpu: the median depth -- the tile pass (csrc/median.hip) against the float64 intervals of
tests/median_depth_reference.py, its bit reproducibility and its independence from what lies behind the surface, the C
entry's refusals and bounds, render mode "RGB+MD" on the engines, and the mesh, trajectory and orthophoto command lines.

No tolerance is tuned here: ids are compared with the reference's admissible interval (d = 5e-4, derived in the
reference's docstring), depths bit for bit with the inputs.  Every test prints the figures it asserts on.

The image of "RGB+MD" is compared bit for bit with that of "RGB"; its alpha with that of "RGB+ED", which the eval
entries return and which the C ABI documents as bit-identical to the 3-channel forward's ("RGB" itself returns no alpha).
"""
import json
import math
import os

import numpy as np
import pytest
import torch

from tests import median_depth_reference as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = ["special"] + R.list_names() + ["list65_sat_middle"] + list(R.GPU_SHAPES)


def _run(case, depths, dev):
    from clm_gs_amd import gsplat as G
    dep, ids = G.rasterize_median_depth(case["m2"].to(dev), case["cn"].to(dev), case["op"].to(dev), depths.to(dev),
                                        case["w"], case["h"], 16, case["off"].to(dev), case["fids"].to(dev))
    torch.cuda.synchronize()
    return dep.cpu(), ids.cpu()


def _assert_clean(res, what):
    print(f"{what}: {res}")
    assert res["excluded"] <= R.EXCLUDED_CAP * res["inside"]
    bad = {k: v for k, v in res.items() if k.startswith("bad_") and v}
    assert not bad, (what, bad)


# ------------------------------------------------------------------------------------------- 1. operator against float64
@pytest.mark.parametrize("kind", ["increasing", "permuted"])
@pytest.mark.parametrize("name", CASES)
def test_operator_matches_the_reference(dev, name, kind):
    case, ref = R.cached(name)
    depths = R.case_depths(case, kind)
    dep, ids = _run(case, depths, dev)
    C, N = case["op"].shape
    assert dep.shape == ids.shape == (C, case["h"], case["w"])
    _assert_clean(R.check_maps(ref, case, depths, dep, ids), f"{name}/{kind}")
    dep2, ids2 = _run(case, depths, dev)  # two calls: the same bits
    assert torch.equal(dep.view(torch.int32), dep2.view(torch.int32)) and torch.equal(ids, ids2)
    if kind == "increasing" and bool(ref["has"].any()):  # no pixel without an entry is hidden behind a lucky 0
        assert bool((dep[ref["has"] & ~ref["excluded"]] >= 1.0).all())


def test_cameras_one_at_a_time_give_the_same_maps(dev):
    case, _ = R.cached("tiles9_C3")
    depths = R.case_depths(case, "permuted")
    dep, ids = _run(case, depths, dev)
    C, N = case["op"].shape
    starts = [int(case["off"][c].flatten()[0]) for c in range(C)] + [int(case["fids"].shape[0])]
    for c in range(C):
        one = dict(case, m2=case["m2"][c:c + 1], cn=case["cn"][c:c + 1], op=case["op"][c:c + 1],
                   off=(case["off"][c:c + 1] - starts[c]).contiguous(),
                   fids=(case["fids"][starts[c]:starts[c + 1]] - c * N).contiguous())
        assert starts[c + 1] > starts[c]
        d1, i1 = _run(one, depths[c:c + 1], dev)
        assert torch.equal(d1[0].view(torch.int32), dep[c].view(torch.int32)) and torch.equal(i1[0], ids[c])


def test_nothing_behind_the_surface_changes_the_maps(dev):
    """list129_sat: every pixel has crossed one half by the wall at D = 127.  Twenty more entries appended behind the walls,
    and the wall at D + 1 made translucent, leave both maps bit-identical."""
    from tests.scenes import SATURATE_AT
    case, ref = R.cached("list129_sat")
    K, D = 129, SATURATE_AT[129]
    assert case["fids"].tolist() == list(range(K)) and int(ref["pos_lo"].max()) <= D
    depths = R.case_depths(case, "permuted")
    base = _run(case, depths, dev)
    g = torch.Generator().manual_seed(5)
    extra = 20
    m2 = torch.cat([case["m2"], 4 + 8 * torch.rand(1, extra, 2, generator=g)], 1)
    cn = torch.cat([case["cn"], torch.tensor([0.05, 0.0, 0.05]).expand(1, extra, 3)], 1)
    op = torch.cat([case["op"], 0.2 + 0.8 * torch.rand(1, extra, generator=g)], 1)
    op[0, D + 1] = 0.3
    more = dict(case, m2=m2.contiguous(), cn=cn.contiguous(), op=op.contiguous(),
                fids=torch.arange(K + extra, dtype=torch.int32))
    deeper = torch.cat([depths, torch.rand(1, extra, generator=g) + 0.01], 1)  # (values a minimum would pick up)
    got = _run(more, deeper, dev)
    assert torch.equal(got[0].view(torch.int32), base[0].view(torch.int32)) and torch.equal(got[1], base[1])
    assert int(base[1].min()) >= 0 and int(base[1].max()) <= D


# ------------------------------------------------------------------------------------------- 2. the C entry
def test_entry_refusals_fill_and_bounds(dev):
    from clm_gs_amd import _lib
    from clm_gs_amd._lib import check, dptr, stream
    case, ref = R.cached("17x17")
    C, N = case["op"].shape
    w, h = case["w"], case["h"]
    L = _lib.lib()
    m2, cn, op = case["m2"].to(dev), case["cn"].to(dev), case["op"].to(dev)
    depths = R.case_depths(case, "permuted").to(dev)
    off, fids = case["off"].to(dev), case["fids"].to(dev)
    th, tw = off.shape[1:]
    pad, n = 64, C * h * w
    buf_d = torch.full((n + 2 * pad,), -7.5, dtype=torch.float32, device=dev)  # canaries on both sides of [C,H,W]
    buf_i = torch.full((n + 2 * pad,), 12345, dtype=torch.int32, device=dev)
    out_d, out_i = buf_d[pad:pad + n], buf_i[pad:pad + n]
    packed = torch.empty(L.clmgs_rasterize_median_pack_bytes(C, N) + 64, dtype=torch.uint8, device=dev)
    assert L.clmgs_rasterize_median_pack_bytes(C, N) == 32 * C * N and packed.data_ptr() % 32 == 0

    def args(**kw):
        a = dict(C=C, N=N, n=fids.numel(), m2=dptr(m2), cn=dptr(cn), op=dptr(op), dep=dptr(depths), w=w, h=h, ts=16, tw=tw,
                 th=th, off=dptr(off), fids=dptr(fids), packed=dptr(packed), od=dptr(out_d), oi=dptr(out_i))
        a.update(kw)
        return (stream(), a["C"], a["N"], a["n"], a["m2"], a["cn"], a["op"], a["dep"], a["w"], a["h"], a["ts"], a["tw"],
                a["th"], a["off"], a["fids"], a["packed"], a["od"], a["oi"])

    import ctypes
    refusals = dict(tile_size=dict(ts=8), tiles_x=dict(tw=tw - 1), tiles_y=dict(th=th - 1), count_32bit=dict(n=2 ** 31),
                    negative_count=dict(n=-1), rows_32bit=dict(C=2 ** 16, N=2 ** 16), no_camera=dict(C=0),
                    null_depth_out=dict(od=None), null_id_out=dict(oi=None), null_offsets=dict(off=None),
                    count_without_list=dict(fids=None), null_means=dict(m2=None), null_conics=dict(cn=None),
                    null_opacities=dict(op=None), null_depths=dict(dep=None), null_packed=dict(packed=None),
                    packed_misaligned=dict(packed=ctypes.c_void_p(packed.data_ptr() + 16)))
    for what, kw in refusals.items():
        assert L.clmgs_rasterize_median(*args(**kw)) != 0, what
    torch.cuda.synchronize()
    assert bool((buf_d == -7.5).all()) and bool((buf_i == 12345).all())  # refused before anything is written
    # nothing listed: every pixel is filled, no list or input is read
    check(L.clmgs_rasterize_median(*args(n=0, fids=None, m2=None, cn=None, op=None, dep=None, packed=None)))
    torch.cuda.synchronize()
    assert bool((out_d == 0).all()) and bool((out_i == -1).all())
    assert bool((buf_d[:pad] == -7.5).all()) and bool((buf_d[pad + n:] == -7.5).all())
    assert bool((buf_i[:pad] == 12345).all()) and bool((buf_i[pad + n:] == 12345).all())
    buf_d.fill_(-7.5); buf_i.fill_(12345)
    check(L.clmgs_rasterize_median(*args(N=0, n=0)))  # no rows
    torch.cuda.synchronize()
    assert bool((out_d == 0).all()) and bool((out_i == -1).all())
    # a full call on a 17x17 image (tiles of which only one row or column lies inside): [C,H,W] and nothing beyond it
    buf_d.fill_(-7.5); buf_i.fill_(12345)
    check(L.clmgs_rasterize_median(*args()))
    torch.cuda.synchronize()
    assert bool((buf_d[:pad] == -7.5).all()) and bool((buf_d[pad + n:] == -7.5).all())
    assert bool((buf_i[:pad] == 12345).all()) and bool((buf_i[pad + n:] == 12345).all())
    assert not bool((out_i == 12345).any()) and not bool((out_d == -7.5).any())  # every pixel was written
    _assert_clean(R.check_maps(ref, case, depths.cpu(), out_d.reshape(C, h, w).cpu(), out_i.reshape(C, h, w).cpu()), "entry")
    # ids outside the camera's rows read and write nothing: those entries are as if not listed
    wild = fids.clone()
    sel = torch.arange(wild.numel(), device=dev) % 3 == 0
    wild[sel] = torch.where(torch.arange(wild.numel(), device=dev)[sel] % 2 == 0, -5, C * N + 1000).to(torch.int32)
    check(L.clmgs_rasterize_median(*args(fids=dptr(wild))))
    torch.cuda.synchronize()
    kept = ~sel.cpu()
    rows_kept = set(case["fids"][kept].tolist())
    assert set(out_i.cpu().tolist()) <= rows_kept | {-1}


def test_operator_detaches_and_runs_without_grad(dev):
    from clm_gs_amd import gsplat as G
    case, _ = R.cached("17x17")
    depths = R.case_depths(case, "permuted").to(dev)
    m2 = case["m2"].to(dev).requires_grad_()
    dep, ids = G.rasterize_median_depth(m2, case["cn"].to(dev), case["op"].to(dev).requires_grad_(), depths, case["w"],
                                        case["h"], 16, case["off"].to(dev), case["fids"].to(dev))
    assert not dep.requires_grad and dep.dtype == torch.float32 and ids.dtype == torch.int32
    base = _run(case, depths.cpu(), dev)
    assert torch.equal(dep.cpu(), base[0]) and torch.equal(ids.cpu(), base[1])


# ------------------------------------------------------------------------------------------- 3. the engines
W, H = 64, 48
FOVX = 0.7
FOCAL = W / (2 * math.tan(FOVX / 2))
FOVY = 2 * math.atan(H / (2 * FOCAL))
CAM_HEIGHT, FRONT_Z = 5.0, 3.0  # camera depths: the back plane 5, the front sheet 2
SEAM, BORDER = 10, 4            # pixels left out on either side of the seam and along the image border
ENGINES = [("no_offload", "hbm"), ("clm_offload", "hbm"), ("clm_offload", "host")]


class _Scene:
    cameras_extent = 5.0


def _grid(x_half, y_half, step):
    xs = torch.arange(-round(x_half / step), round(x_half / step) + 1, dtype=torch.float32) * step
    ys = torch.arange(-round(y_half / step), round(y_half / step) + 1, dtype=torch.float32) * step
    y, x = torch.meshgrid(ys, xs, indexing="ij")
    return x.reshape(-1), y.reshape(-1)


def _two_layer_rows():
    """Back: opaque flat Gaussians 0.04 apart and 0.04 wide on z = 0 (the sheet of tests/test_gpu_tsdf.py).  Front: flat
    Gaussians 0.06 apart and 0.06 wide on z = 3, whose overlapping sum gives a per-pixel alpha of about 0.3 where x < 0 and
    about 0.7 where x > 0.  Every centre is moved along z by up to 2e-3 (seeded) so that the rows' depths differ.
    -> (xyz, shs48, log scales, quats, opacity logits, bool mask of the front rows), CPU."""
    g = torch.Generator().manual_seed(21)
    bx, by = _grid(2.4, 2.4, 0.04)
    fx, fy = _grid(1.5, 1.2, 0.06)
    nb, nf = bx.numel(), fx.numel()
    z = torch.cat([torch.zeros(nb), torch.full((nf,), FRONT_Z)]) + (torch.rand(nb + nf, generator=g) - 0.5) * 4e-3
    xyz = torch.stack([torch.cat([bx, fx]), torch.cat([by, fy]), z], 1)
    shs = torch.zeros(nb + nf, 16, 3)
    shs[:nb, 0, :] = torch.stack([bx * 0.3, by * 0.3, torch.full((nb,), 0.5)], 1)
    shs[nb:, 0, 0] = 1.0
    scaling = torch.log(torch.cat([torch.tensor([0.04, 0.04, 1e-4]).expand(nb, 3), torch.tensor([0.06, 0.06, 1e-4]).expand(nf, 3)]))
    rotation = torch.tensor([1.0, 0.0, 0.0, 0.0]).expand(nb + nf, 4)
    # alpha = 1 - prod(1 - o G): with the width equal to the spacing, sum G = 2 pi, so o ~ -ln(1 - alpha) / (2 pi)
    o_front = torch.where(fx < 0, torch.tensor(0.058), torch.tensor(0.20))
    opacity = torch.cat([torch.full((nb,), 6.0), torch.logit(o_front)]).reshape(-1, 1)
    front = torch.cat([torch.zeros(nb, dtype=torch.bool), torch.ones(nf, dtype=torch.bool)])
    return [t.contiguous() for t in (xyz, shs.reshape(-1, 48), scaling, rotation, opacity)] + [front]


def _nadir_camera(uid, x, y, dev):
    from clm_gs_amd.cameras import Camera
    Rm = torch.tensor([[1.0, 0, 0], [0, -1.0, 0], [0, 0, -1.0]])
    w2c = torch.eye(4)
    w2c[:3, :3] = Rm
    w2c[:3, 3] = -Rm @ torch.tensor([x, y, CAM_HEIGHT])
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
    else:
        from clm_gs_amd.strategies.clm_offload import GaussianModelCLMOffload as M
    xyz, shs, scaling, rotation, opacity, front = _two_layer_rows()
    m = M(3)
    m.create_from_tensors(xyz.to(dev), shs.to(dev), scaling.to(dev), rotation.to(dev), opacity.to(dev), spatial_lr_scale=1.0)
    m.active_sh_degree = 3
    m.training_setup(args)
    return args, m, front


def _layer_depth_bits(cam, dev):
    """The bit patterns of fully_fused_projection's depths of the back rows and of the front rows for a camera."""
    from clm_gs_amd import gsplat as G
    from clm_gs_amd.strategies.base_engine import fov_camera
    xyz, _, scaling, rotation, _, front = _two_layer_rows()
    viewmat, K, _ = fov_camera(cam, dev)
    _, _, depths, _, _ = G.fully_fused_projection(xyz.to(dev), None, rotation.to(dev), torch.exp(scaling).to(dev),
                                                  viewmat[None], K[None], W, H)
    bits = depths[0].view(torch.int32).cpu()
    return bits[~front], bits[front]


def _halves():
    cols = torch.arange(W)
    rows = torch.arange(H)
    inner = ((rows >= BORDER) & (rows < H - BORDER))[:, None]
    left = inner & ((cols >= BORDER) & (cols < W // 2 - SEAM))[None, :]
    right = inner & ((cols >= W // 2 + SEAM) & (cols < W - BORDER))[None, :]
    return left, right


@pytest.fixture(scope="module")
def engine_maps(dev):
    """The two-layer scene through the three eval entries: per engine the (image, depth, alpha) of "RGB+MD" and "RGB+ED"
    and the image of "RGB", on the CPU."""
    from clm_gs_amd import utils
    from clm_gs_amd.render_trajectory import eval_one_cam
    out = {}
    try:
        for strategy, residency in ENGINES:
            args, m, _ = _model(strategy, residency, dev)
            cam = _nadir_camera(0, 0.0, 0.0, dev)
            with torch.no_grad():
                md = tuple(t.clone().cpu() for t in eval_one_cam(cam, m, None, args, _Scene, render_mode="RGB+MD"))
                ed = tuple(t.clone().cpu() for t in eval_one_cam(cam, m, None, args, _Scene, render_mode="RGB+ED"))
                rgb = eval_one_cam(cam, m, None, args, _Scene).clone().cpu()
            torch.cuda.synchronize()
            out[(strategy, residency)] = dict(md=md, ed=ed, rgb=rgb)
        out["bits"] = _layer_depth_bits(_nadir_camera(0, 0.0, 0.0, dev), dev)
    finally:
        utils.set_args(utils.default_args())
    return out


@pytest.mark.parametrize("strategy,residency", ENGINES)
def test_engines_return_the_surface_not_the_blend(dev, engine_maps, strategy, residency):
    r = engine_maps[(strategy, residency)]
    back, front = engine_maps["bits"]
    (img, depth, alpha), (img_e, depth_e, alpha_e) = r["md"], r["ed"]
    assert depth.shape == alpha.shape == (1, H, W) and depth.dtype == torch.float32
    left, right = _halves()
    assert int(left.sum()) > 500 and int(right.sum()) > 500
    # the scene is what it claims: the sheet's own alpha is alpha_total - T_front * alpha_back; with an opaque back layer
    # the expected depth gives it back as (5 - ED) / 3 up to the 2e-3 jitter
    a_front = (CAM_HEIGHT - depth_e[0]) / (CAM_HEIGHT - (CAM_HEIGHT - FRONT_Z))
    print(f"{strategy}/{residency}: front alpha left [{float(a_front[left].min()):.3f}, {float(a_front[left].max()):.3f}] "
          f"right [{float(a_front[right].min()):.3f}, {float(a_front[right].max()):.3f}], total alpha min "
          f"{float(alpha[0][left | right].min()):.4f}")
    assert 0.2 < float(a_front[left].min()) and float(a_front[left].max()) < 0.4
    assert 0.6 < float(a_front[right].min()) and float(a_front[right].max()) < 0.8
    assert float(alpha[0][left | right].min()) > 0.9  # (the bound tests/test_gpu_tsdf.py holds the same back sheet to)
    d_bits = depth[0].view(torch.int32)
    assert bool(torch.isin(d_bits[left], back).all()), "a left-half pixel is not a back-layer row's depth"
    assert bool(torch.isin(d_bits[right], front).all()), "a right-half pixel is not a front-layer row's depth"
    assert not bool(torch.isin(d_bits[left], front).any()) and not bool(torch.isin(d_bits[right], back).any())
    # the bias the feature removes: the expected depth lies strictly between the layers on both halves
    lo, hi = CAM_HEIGHT - FRONT_Z + 2e-3, CAM_HEIGHT - 2e-3
    for half in (left, right):
        assert bool(((depth_e[0][half] > lo) & (depth_e[0][half] < hi)).all())
    print(f"{strategy}/{residency}: expected depth left {float(depth_e[0][left].mean()):.3f} right "
          f"{float(depth_e[0][right].mean()):.3f}; median depth left {float(depth[0][left].mean()):.3f} right "
          f"{float(depth[0][right].mean()):.3f}")
    # image and alpha are the 3-channel forward's
    assert torch.equal(img.view(torch.int32), r["rgb"].view(torch.int32))
    assert torch.equal(alpha.view(torch.int32), alpha_e.view(torch.int32))
    # the three engines agree bit for bit
    first = engine_maps[ENGINES[0]]["md"]
    assert torch.equal(depth.view(torch.int32), first[1].view(torch.int32))


def test_training_entries_refuse_the_mode(dev):
    from clm_gs_amd import utils
    from clm_gs_amd.strategies.base_engine import pipeline_forward_one_step
    from clm_gs_amd.strategies.clm_offload.engine import pipeline_forward_one_step_shs_inplace
    from clm_gs_amd.strategies.no_offload import baseline_accumGrads_micro_step
    try:
        args, m, _ = _model("no_offload", "hbm", dev)
        cam = _nadir_camera(0, 0.0, 0.0, dev)
        tensors = (m.get_xyz, m.get_opacity, m.get_scaling, m.get_rotation, m.get_features)
        with pytest.raises(ValueError, match="RGB\\+MD"):
            baseline_accumGrads_micro_step(*tensors, 3, cam, None, mode="train", render_mode="RGB+MD")
        xyz, opa, sca, rot, shs = tensors
        with pytest.raises(ValueError, match="RGB\\+MD"):
            pipeline_forward_one_step(opa, sca, rot, xyz, shs.reshape(-1, 48), cam, _Scene, m, None, None, eval=False,
                                      render_mode="RGB+MD")
        with pytest.raises(ValueError, match="RGB\\+MD"):
            pipeline_forward_one_step_shs_inplace(opa, sca, rot, xyz, shs.reshape(-1, 48), cam, _Scene, m, None, None,
                                                  render_mode="RGB+MD")
        with pytest.raises(ValueError, match="render_mode must be one of"):
            baseline_accumGrads_micro_step(*tensors, 3, cam, None, mode="eval", render_mode="RGB+XD")
    finally:
        utils.set_args(utils.default_args())


def test_antialiased_agrees_with_the_operator_on_compensated_opacities(dev):
    from clm_gs_amd import gsplat as G, utils
    from clm_gs_amd.render_trajectory import eval_one_cam
    from clm_gs_amd.strategies.base_engine import fov_camera
    try:
        args, m, _ = _model("no_offload", "hbm", dev, mode="antialiased")
        cam = _nadir_camera(0, 0.0, 0.0, dev)
        with torch.no_grad():
            _, depth, _ = eval_one_cam(cam, m, None, args, _Scene, render_mode="RGB+MD")
            viewmat, K, _ = fov_camera(cam, dev)
            radii, m2, depths, conics, comps = G.fully_fused_projection(
                m.get_xyz, None, m.get_rotation, m.get_scaling, viewmat[None], K[None], W, H, radius_clip=args.radius_clip,
                calc_compensations=True)
            tw, th = math.ceil(W / 16), math.ceil(H / 16)
            _, isect_ids, fids = G.isect_tiles(m2, radii, depths, 16, tw, th)
            off = G.isect_offset_encode(isect_ids, 1, tw, th)
            op = m.get_opacity.squeeze(1).unsqueeze(0)
            want, _ = G.rasterize_median_depth(m2, conics, op * comps, depths, W, H, 16, off, fids)
            plain, _ = G.rasterize_median_depth(m2, conics, op, depths, W, H, 16, off, fids)
        torch.cuda.synchronize()
        assert float(comps.min()) < 0.9  # the compensation is not the identity on this scene
        assert torch.equal(depth.view(torch.int32), want.view(torch.int32))
        print(f"antialiased: {int((want != plain).sum())} of {W * H} pixels differ from the uncompensated median")
    finally:
        utils.set_args(utils.default_args())


# ------------------------------------------------------------------------------------------- 4. the mesh
PLANE_VOXEL = 0.05  # tests/test_gpu_tsdf.py: every vertex of its sheet lies within one voxel of the plane
MESH_BOUNDS = (-1.0, -0.9, -0.5, 1.0, 0.9, 1.5)
# small offsets: seen from x = c the seam of the front sheet falls on the back plane at x = -1.5 c
MESH_CAM_XY = ((0.03, -0.05), (-0.08, 0.06), (0.07, 0.04), (-0.05, -0.07), (0.0, 0.01))
UNDER_LEFT = -0.7  # back-plane x below which every camera looks through the alpha 0.3 half (seam 0.12 + its blur 0.45)


def test_build_mesh_median_against_expected(dev, tmp_path):
    from clm_gs_amd import io_ply, mesh_model, utils
    from clm_gs_amd.render_ortho import map_frame
    try:
        args, m, _ = _model("no_offload", "hbm", dev)
        cams = [_nadir_camera(i, x, y, dev) for i, (x, y) in enumerate(MESH_CAM_XY)]
        metas, zs = {}, {}
        for mode in ("median", "expected"):
            path = str(tmp_path / mode / "mesh.ply")
            with open(os.devnull, "w") as log:
                metas[mode] = mesh_model.build_mesh(m, cams, args, path, PLANE_VOXEL, frame=map_frame(), bounds=MESH_BOUNDS,
                                                    log=log, depth_mode=mode)
            verts, _, faces = io_ply.load_mesh_ply(path)
            assert metas[mode] == json.load(open(mesh_model.json_path(path)))
            z = verts[verts[:, 0] < UNDER_LEFT][:, 2].astype(np.float64)
            print(f"mesh/{mode}: V {len(verts)} F {len(faces)}; under the left half {len(z)} vertices, z in "
                  f"[{z.min():.4f}, {z.max():.4f}]")
            assert len(z) > 50
            zs[mode] = z
        assert float(np.abs(zs["median"]).max()) <= PLANE_VOXEL  # on the back plane
        assert float(zs["expected"].min()) > PLANE_VOXEL         # in front of it by more than a voxel
        assert metas["median"]["depth_mode"] == "median" and "depth_mode" not in metas["expected"]
        with pytest.raises(ValueError, match="depth_mode"):
            mesh_model.build_mesh(m, cams, args, str(tmp_path / "bad" / "mesh.ply"), PLANE_VOXEL, depth_mode="mode7")
        assert not (tmp_path / "bad").exists()
    finally:
        utils.set_args(utils.default_args())


def test_mesh_cli_with_median_depth(dev, tmp_path, capsys):
    from clm_gs_amd import io_ply, mesh_model, utils
    from tests.test_gpu_tsdf import _shell_rows
    scene = os.path.join(ROOT, "tests", "golden", "colmap_tiny")
    rows = _shell_rows()
    ply = str(tmp_path / "shell.ply")
    io_ply.save_ply(ply, rows["xyz"], rows["shs48"], rows["opacity"], rows["scaling"], rows["rotation"])
    try:
        mesh = str(tmp_path / "out" / "mesh.ply")
        assert mesh_model.main(["-m", ply, "-s", scene, "-o", mesh, "--voxel", "1", "--min_weight", "1", "--no_offload",
                                "--depth_mode", "median", "--bounds", "-14", "-14", "-14", "14", "14", "14"]) == 0
        line = capsys.readouterr().out
        assert "render" in line and "integration" in line, line
        verts, colours, faces = io_ply.load_mesh_ply(mesh)
        meta = json.load(open(mesh[:-4] + ".json"))
        assert meta["depth_mode"] == "median" and meta["vertices"] == len(verts) > 0 and meta["faces"] == len(faces) > 0
        r = np.linalg.norm(verts.astype(np.float64), axis=1)  # the surface found is the shell
        assert float(np.abs(r - 12.0).max()) < 4.0, (float(r.min()), float(r.max()))
    finally:
        utils.set_args(utils.default_args())


# ------------------------------------------------------------------------------------------- 5. trajectory and orthophoto
def _save_two_layers(path):
    from clm_gs_amd import io_ply
    xyz, shs, scaling, rotation, opacity, _ = _two_layer_rows()
    io_ply.save_ply(path, xyz, shs, opacity, scaling, rotation)


def test_render_trajectory_writes_the_median_depth(dev, tmp_path):
    from clm_gs_amd import render_trajectory as RT, utils
    from clm_gs_amd.strategies.no_offload import GaussianModelNoOffload as M
    ply, out = str(tmp_path / "layers.ply"), tmp_path / "frames"
    _save_two_layers(ply)
    try:
        common = ["-m", ply, "--no_offload", "--n_frames", "1", "--manual_height", str(CAM_HEIGHT), "--width", str(W),
                  "--height", str(H), "--fovx", str(FOVX), "--hull", "0,0", "0.5,0", "0,0", "--render_depth"]
        assert RT.main(common + ["--output_dir", str(out), "--depth_mode", "median"]) == 0
        assert RT.main(common + ["--output_dir", str(tmp_path / "frames_ed")]) == 0
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
            _, depth, _ = RT.eval_one_cam(cam, m, None, args, None, render_mode="RGB+MD")
            _, depth_e, _ = RT.eval_one_cam(cam, m, None, args, None, render_mode="RGB+ED")
        assert got.dtype == np.float32 and np.array_equal(got, depth[0].cpu().numpy())
        assert np.array_equal(np.load(tmp_path / "frames_ed" / "depth_00000.npy"), depth_e[0].cpu().numpy())
        assert not np.array_equal(got, depth_e[0].cpu().numpy())
        # two layers and nothing between them
        near_a_layer = (np.abs(got - CAM_HEIGHT) < 3e-3) | (np.abs(got - (CAM_HEIGHT - FRONT_Z)) < 3e-3)
        assert near_a_layer.all()
    finally:
        utils.set_args(utils.default_args())


def test_render_ortho_height_from_the_median_depth(dev, tmp_path):
    from clm_gs_amd import render_ortho, utils
    ply = str(tmp_path / "layers.ply")
    _save_two_layers(ply)
    try:
        common = ["-m", ply, "--no_offload", "--gsd", "0.04", "--bounds", "-1.0", "-0.8", "1.0", "0.8", "--camera_height",
                  str(CAM_HEIGHT), "--tile", "64"]
        assert render_ortho.main(common + ["--output_dir", str(tmp_path / "md"), "--depth_mode", "median"]) == 0
        assert render_ortho.main(common + ["--output_dir", str(tmp_path / "ed")]) == 0
        h_md, h_ed = np.load(tmp_path / "md" / "ortho_height.npy"), np.load(tmp_path / "ed" / "ortho_height.npy")
        meta_md, meta_ed = json.load(open(tmp_path / "md" / "ortho.json")), json.load(open(tmp_path / "ed" / "ortho.json"))
        assert meta_md.pop("depth_mode") == "median" and meta_md == meta_ed and "depth_mode" not in meta_ed
        assert np.array_equal(np.load(tmp_path / "md" / "ortho_alpha.npy"), np.load(tmp_path / "ed" / "ortho_alpha.npy"))
        width = h_md.shape[1]
        assert h_md.shape == h_ed.shape == (40, 50)
        left = np.zeros_like(h_md, dtype=bool)
        left[2:-2, 2:width // 2 - 8] = True  # world x < -0.32: clear of the seam's blur (3 x 0.06)
        right = np.zeros_like(left)
        right[2:-2, width // 2 + 8:-2] = True
        print(f"ortho: median height left [{h_md[left].min():.4f}, {h_md[left].max():.4f}] right "
              f"[{h_md[right].min():.4f}, {h_md[right].max():.4f}]; expected-depth height left "
              f"[{h_ed[left].min():.4f}, {h_ed[left].max():.4f}]")
        assert np.isfinite(h_md[left | right]).all()
        assert np.abs(h_md[left]).max() < 3e-3                 # the back plane (z = 0 +- 2e-3)
        assert np.abs(h_md[right] - FRONT_Z).max() < 3e-3      # the sheet itself where it is the surface
        assert h_ed[left].min() > 0.5 and h_ed[left].max() < FRONT_Z - 0.5  # the blend: a height at which nothing is
    finally:
        utils.set_args(utils.default_args())
