"""Mesh export on the device ("Mesh export"): csrc/tsdf.hip through clm_kernels.tsdf_integrate /
tsdf_extract, tsdf.TsdfVolume and the command line against the numpy restatement (tests/tsdf_reference.py): the fused
grid bit for bit outside the band of near-tie voxels, batch invariance, the extraction (faces exactly, vertices to one
float32 ulp, colours to one level, the topology of the kernel's own output), a rendered plane end to end, the CLI and the
refusals of the entries."""
import ctypes
import json
import math
import os

import numpy as np
import pytest
import torch

from tests import tsdf_reference as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_CACHE = {}

# ------------------------------------------------------------------------------------------------ 1. fusion
NX, NY, NZ = 20, 18, 16          # three different sides: a swapped index shows
H, W = 33, 47
VOXEL = 0.1
NEAR, DEPTH_MAX, ALPHA_MIN, TRUNC = 2.2, 4.2, 0.5, 0.4
N_CAMS = 17


def _look_at(C, target, roll, rng):
    f = target - C
    f = f / np.linalg.norm(f)
    up = rng.normal(size=3)
    r = np.cross(f, up)
    r = r / np.linalg.norm(r)
    d = np.cross(f, r)
    c, s = math.cos(roll), math.sin(roll)
    r, d = c * r + s * d, -s * r + c * d
    w2c = np.eye(4)
    w2c[:3, :3] = np.stack([r, d, f])
    w2c[:3, 3] = -w2c[:3, :3] @ C
    return w2c


def _fusion_case():
    """17 random float64 poses about a 2.0 x 1.8 x 1.6 box: most look at a point near it from 2.5 to 4 away (so part of the
    box is nearer than `near` for some, and outside the image for others), two look away (the box behind them); depth
    maps scattered about the distance to the box so that every branch of the rule is taken; alpha on both sides of the
    gate; colours outside [0, 1]."""
    if "fusion" in _CACHE:
        return _CACHE["fusion"]
    rng = np.random.default_rng(20)
    g2w = np.array([[VOXEL, 0, 0, -NX * VOXEL / 2], [0, VOXEL, 0, -NY * VOXEL / 2], [0, 0, VOXEL, -NZ * VOXEL / 2]])
    g4 = np.vstack([g2w, [0, 0, 0, 1.0]])
    cams = np.empty((N_CAMS, 16))
    for b in range(N_CAMS):
        d = rng.normal(size=3)
        C = d / np.linalg.norm(d) * rng.uniform(2.5, 4.0)
        target = rng.uniform(-1.2, 1.2, size=3) if b % 6 != 5 else 2.0 * C
        w2c = _look_at(C, target, rng.uniform(0, 2 * math.pi), rng)
        cams[b, :12] = (w2c @ g4)[:3].reshape(12)
        cams[b, 12:] = (rng.uniform(35, 70), rng.uniform(35, 70), W / 2 + rng.uniform(-3, 3), H / 2 + rng.uniform(-3, 3))
    depth = rng.uniform(1.8, 4.6, size=(N_CAMS, H, W)).astype(np.float32)
    depth[rng.random(depth.shape) < 0.05] = 0.0
    alpha = rng.uniform(0.2, 1.0, size=(N_CAMS, H, W)).astype(np.float32)
    rgb = rng.uniform(-0.3, 1.3, size=(N_CAMS, 3, H, W)).astype(np.float32)
    start = np.zeros((6, NZ, NY, NX), dtype=np.float32)
    _CACHE["fusion"] = (cams, depth, alpha, rgb, start)
    return _CACHE["fusion"]


def _reference(B):
    key = ("ref", B)
    if key not in _CACHE:
        cams, depth, alpha, rgb, start = _fusion_case()
        _CACHE[key] = R.integrate(start, cams[:B], depth[:B], alpha[:B], rgb[:B], NEAR, DEPTH_MAX, ALPHA_MIN, TRUNC)
    return _CACHE[key]


def _fuse(dev, sel, grid=None, cull=True):
    from clm_gs_amd import clm_kernels
    cams, depth, alpha, rgb, start = _fusion_case()
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a[sel])).to(dev)
    if grid is None:
        grid = torch.from_numpy(start).to(dev)
    return clm_kernels.tsdf_integrate(grid, t(depth), t(alpha), t(rgb), cams[sel], near=NEAR, depth_max=DEPTH_MAX,
                                      alpha_min=ALPHA_MIN, trunc=TRUNC, cull=cull)


def check_against_reference(got, ref, band, what=""):
    """All six planes bit-equal outside the band; inside it wsum and cw differ by at most the voxel's band cameras.  The
    band holds at most 0.1 % of the voxels (asserted: the seeds are chosen so)."""
    got = np.asarray(got)
    n_band = int((band > 0).sum())
    print(f"{what}: band voxels {n_band} of {band.size}; observed voxels {int((ref[1] > 0).sum())}, coloured "
          f"{int((ref[5] > 0).sum())}, max wsum {float(ref[1].max()):g}")
    assert n_band <= 1e-3 * band.size
    out = band == 0
    for p, name in enumerate(("tsum", "wsum", "cr", "cg", "cb", "cw")):
        a, b = got[p][out].view(np.int32), ref[p][out].view(np.int32)
        assert np.array_equal(a, b), f"{what}: plane {name} differs in {int((a != b).sum())} voxels outside the band"
    for p in (1, 5):
        assert (np.abs(got[p] - ref[p]) <= band).all(), what


@pytest.mark.parametrize("B", [1, 5, 16])
def test_integration_equals_the_reference_bit_for_bit(dev, B):
    ref, band = _reference(B)
    if B == 16:  # every branch of the rule is taken by the inputs
        cams, depth, alpha, rgb, start = _fusion_case()
        assert 0 < int((ref[1] > 0).sum()) < ref[1].size and 0 < int((ref[5] > 0).sum()) < int((ref[1] > 0).sum())
        assert float(ref[0].min()) < 0 < float(ref[0].max()) and float(ref[1].max()) >= 3
        assert float(ref[2:5].max()) > 1.0  # (sums of clamped colours)
        for kw in (dict(near=0.01), dict(depth_max=100.0), dict(alpha_min=0.0)):  # ... each gate included
            args = dict(near=NEAR, depth_max=DEPTH_MAX, alpha_min=ALPHA_MIN, trunc=TRUNC)
            args.update(kw)
            other, _ = R.integrate(start, cams[:4], depth[:4], alpha[:4], rgb[:4], **args)
            assert not np.array_equal(other[1], _reference_first4()[1]), kw
    for cull in (True, False):
        got = _fuse(dev, slice(0, B), cull=cull).cpu().numpy()
        check_against_reference(got, ref, band, f"B={B} cull={cull}")
        if cull:
            culled = got
    assert np.array_equal(culled.view(np.int32), got.view(np.int32))  # the brick cull changes no bit


def _reference_first4():
    if "ref4" not in _CACHE:
        cams, depth, alpha, rgb, start = _fusion_case()
        _CACHE["ref4"] = R.integrate(start, cams[:4], depth[:4], alpha[:4], rgb[:4], NEAR, DEPTH_MAX, ALPHA_MIN, TRUNC)[0]
    return _CACHE["ref4"]


def test_batches_split_differently_give_the_same_bits(dev):
    whole = _fuse(dev, slice(0, 17))  # two launches: 16 + 1
    one_by_one = None
    for b in range(17):
        one_by_one = _fuse(dev, slice(b, b + 1), one_by_one)
    split = _fuse(dev, slice(5, 17), _fuse(dev, slice(0, 5)))  # a second call on the same volume continues the sums
    assert torch.equal(whole.view(torch.int32), one_by_one.view(torch.int32))
    assert torch.equal(whole.view(torch.int32), split.view(torch.int32))
    assert float(whole[1].max()) >= 3
    again = _fuse(dev, slice(0, 17), whole.clone())
    assert torch.equal(again[1], 2 * whole[1]) and torch.equal(again[5], 2 * whole[5])


# ------------------------------------------------------------------------------------------------ 2. extraction
def _random_grid():
    """31 x 27 x 23, a smooth random field plus noise (crossings everywhere, the border included), 20 % of the voxels below
    min_weight (so a sixth of the cells has eight valid voxels and few edges all four cells), a tenth without colour."""
    rng = np.random.default_rng(5)
    nz, ny, nx = 23, 27, 31
    z, y, x = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    field = np.sin(0.7 * x + 0.3) + np.cos(0.9 * y) + np.sin(0.8 * z + 1.0) + 0.3 * rng.normal(size=(nz, ny, nx))
    g = np.zeros((6, nz, ny, nx), dtype=np.float32)
    w = rng.integers(2, 7, size=(nz, ny, nx)).astype(np.float32)
    low = rng.random(w.shape) < 0.2
    w[low] = rng.integers(0, 2, size=int(low.sum()))
    g[0] = (w * np.clip(field, -1, 1)).astype(np.float32)
    g[1] = w
    cw = np.where(rng.random(w.shape) < 0.1, 0, w).astype(np.float32)
    for ch in range(3):
        g[2 + ch] = (cw * rng.random(w.shape)).astype(np.float32)
    g[5] = cw
    g2w = np.array([[0.3, 0.01, -0.02, 5.0], [0.02, 0.31, 0.0, -70.0], [0.0, 0.015, 0.29, 1000.0]])
    return g, g2w


def _all_outside():
    g = R.grid_from_sdf(R.sphere_sdf())
    g[0] = np.abs(g[0]) + 1
    return g, R.G2W


def _one_voxel():
    """3 x 3 x 3, every voxel valid and outside but the middle one: the smallest grid that can hold a quad at all (a quad needs
    a neighbour on both sides of its two cross axes).  The eight cells are active and the six edges out of the middle voxel
    have a quad each: V = 8, F = 12."""
    g = np.zeros((6, 3, 3, 3), dtype=np.float32)
    g[0] = g[1] = g[5] = 2.0
    g[0, 1, 1, 1] = -2.0
    return g, np.hstack([np.eye(3), np.zeros((3, 1))])


EXTRACT_CASES = {
    "sphere": lambda: (R.grid_from_sdf(R.sphere_sdf()), R.G2W), "torus": lambda: (R.grid_from_sdf(R.torus_sdf()), R.G2W),
    "sphere_unseen_interior": lambda: (R.grid_from_sdf(R.sphere_sdf(), unseen_interior=True), R.G2W),
    "random": _random_grid, "all_outside": _all_outside, "one_voxel": _one_voxel,
}


def _ulp_close(a, b):
    a, b = np.asarray(a, dtype=np.float32), np.asarray(b, dtype=np.float32)
    return np.abs(a.astype(np.float64) - b.astype(np.float64)) <= np.spacing(np.maximum(np.abs(a), np.abs(b)))


@pytest.mark.parametrize("name", sorted(EXTRACT_CASES))
def test_extraction_equals_the_reference(dev, name):
    from clm_gs_amd import clm_kernels
    grid, g2w = EXTRACT_CASES[name]()
    rv, rc, rf, cells = R.extract(grid, 2.0, g2w)
    verts, colours, faces = clm_kernels.tsdf_extract(torch.from_numpy(grid).to(dev), 2.0, g2w)
    assert verts.dtype == torch.float32 and colours.dtype == torch.uint8 and faces.dtype == torch.int32
    assert verts.shape == (len(rv), 3) and colours.shape == (len(rv), 3) and faces.shape == (len(rf), 3)
    verts, colours, faces = verts.cpu().numpy(), colours.cpu().numpy(), faces.cpu().numpy()
    print(f"{name}: V {len(rv)} F {len(rf)}")
    if name == "all_outside":
        assert len(rv) == 0 and len(rf) == 0
        return
    if name == "one_voxel":
        assert len(rv) == 8 and len(rf) == 12
    else:
        assert len(rv) > 100 and len(rf) > (20 if name == "random" else 100)
    assert np.array_equal(faces, rf)
    assert _ulp_close(verts, rv).all()
    assert int(np.abs(colours.astype(np.int32) - rc.astype(np.int32)).max()) <= 1
    if name == "random":
        assert 0 < int((grid[1] < 2).sum()) and len(rf) < 2 * 3 * grid[0].size
    else:  # the topology assertions of the CPU test on the kernel's own output
        t = R.check_closed_surface(verts, faces, cells, g2w, 0 if name == "torus" else 2)
        assert (t["V"], t["F"]) == {"torus": (728, 1456), "one_voxel": (8, 12)}.get(name, (746, 1488))


# ------------------------------------------------------------------------------------------------ 3. a rendered plane
PW = PH = 64
PLANE_VOXEL = 0.05
PLANE_BOUNDS = (-1.0, -0.9, -0.5, 1.0, 0.9, 0.5)
CAM_HEIGHT = 3.0
CAM_XY = ((0.137, -0.211), (-0.413, 0.322), (0.391, 0.289), (-0.277, -0.341), (0.013, 0.047))


def _plane_rows(dev):
    """A dense sheet of opaque flat Gaussians on z = 0: 0.04 apart over [-2.4, 2.4]^2, 0.04 wide, 1e-4 thick."""
    c = torch.arange(-60, 61, dtype=torch.float32) * 0.04
    y, x = torch.meshgrid(c, c, indexing="ij")
    n = x.numel()
    xyz = torch.stack([x.reshape(-1), y.reshape(-1), torch.zeros(n)], 1)
    shs = torch.zeros(n, 16, 3)
    shs[:, 0, :] = torch.stack([xyz[:, 0] * 0.3, xyz[:, 1] * 0.3, torch.full((n,), 0.5)], 1)  # colour varies over the sheet
    scaling = torch.log(torch.tensor([0.04, 0.04, 1e-4])).expand(n, 3)
    rotation = torch.tensor([1.0, 0.0, 0.0, 0.0]).expand(n, 4)
    opacity = torch.full((n, 1), 6.0)
    return [t.contiguous().to(dev) for t in (xyz, shs.reshape(n, 48), scaling, rotation, opacity)]


def _nadir_camera(uid, x, y, dev):
    from clm_gs_amd.cameras import Camera
    Rm = torch.tensor([[1.0, 0, 0], [0, -1.0, 0], [0, 0, -1.0]])
    w2c = torch.eye(4)
    w2c[:3, :3] = Rm
    w2c[:3, 3] = -Rm @ torch.tensor([x, y, CAM_HEIGHT])
    return Camera(uid, w2c, 0.7, 0.7, PW, PH, device=dev)


@pytest.mark.parametrize("strategy", ["no_offload", "clm_offload"])
def test_plane_end_to_end(dev, strategy):
    from clm_gs_amd import tsdf, utils
    from clm_gs_amd.render_ortho import map_frame
    from clm_gs_amd.render_trajectory import eval_one_cam
    try:
        args = utils.default_args(bsz=4)
        setattr(args, strategy, True)
        utils.set_args(args)
        utils.set_img_size(PH, PW)
        utils.set_cur_iter(1)
        if strategy == "clm_offload":
            from clm_gs_amd.strategies.clm_offload import GaussianModelCLMOffload as M
        else:
            from clm_gs_amd.strategies.no_offload import GaussianModelNoOffload as M
        xyz, shs, scaling, rotation, opacity = _plane_rows(dev)
        m = M(3, only_for_rendering=True)
        m.create_from_tensors(xyz, shs, scaling, rotation, opacity, spatial_lr_scale=1.0)
        m.active_sh_degree = 3
        cams = [_nadir_camera(i, x, y, dev) for i, (x, y) in enumerate(CAM_XY)]
        with torch.no_grad():
            renders = [tuple(t.clone() for t in eval_one_cam(c, m, None, args, render_mode="RGB+ED")) for c in cams]
        for image, depth, alpha in renders:  # the sheet is opaque and every centre has camera depth 3
            print(f"plane/{strategy}: alpha min {float(alpha.min()):.4f}, max |depth - 3| {float((depth - CAM_HEIGHT).abs().max()):.2e}")
            assert float(alpha.min()) > 0.9 and float((depth - CAM_HEIGHT).abs().max()) < 1e-4
        volume = tsdf.TsdfVolume(map_frame(), PLANE_BOUNDS, PLANE_VOXEL, trunc_voxels=4.0, device=dev)
        assert (volume.nx, volume.ny, volume.nz) == (40, 36, 20)
        volume.integrate(cams, renders)
        assert volume.cameras_used == len(cams)
        # the kernel's grid == the reference integration of the very depth maps that were rendered
        rec = np.stack([tsdf.camera_record(c, volume.grid_to_world) for c in cams])
        st = lambda k, shape: np.stack([r[k].reshape(shape).cpu().numpy() for r in renders])
        ref, band = R.integrate(np.zeros((6, 20, 36, 40), dtype=np.float32), rec, st(1, (PH, PW)), st(2, (PH, PW)),
                                st(0, (3, PH, PW)), 0.01, float("inf"), 0.5, volume.trunc)
        check_against_reference(volume.grid.cpu().numpy(), ref, band, f"plane/{strategy}")
        verts, colours, faces = (t.cpu().numpy() for t in volume.extract(min_weight=2.0))
        assert len(verts) > 500 and len(faces) > 1000
        assert float(np.abs(verts[:, 2]).max()) <= PLANE_VOXEL  # every vertex within one voxel of the plane
        v = verts.astype(np.float64)
        nrm = np.cross(v[faces[:, 1]] - v[faces[:, 0]], v[faces[:, 2]] - v[faces[:, 0]])
        assert (nrm[:, 2] > 0).all()  # the faces' normals point up, towards the cameras
        area = float(0.5 * np.linalg.norm(nrm, axis=1).sum())
        print(f"plane/{strategy}: V {len(verts)} F {len(faces)} area {area:.3f} max |z| {float(np.abs(verts[:, 2]).max()):.2e}")
        assert 1.0 < area <= 2.0 * 1.8 * 1.05  # at least two cameras see the middle; never more than the box's footprint
        # colours follow the sheet's (SH DC c -> 0.5 + 0.2821 c)
        want = np.clip(0.5 + 0.28209479 * np.stack([0.3 * v[:, 0], 0.3 * v[:, 1], np.full(len(v), 0.5)], 1), 0, 1)
        assert float(np.abs(colours / 255.0 - want).max()) < 0.03
        rv, rc, rf, _ = R.extract(volume.grid.cpu().numpy(), 2.0, volume.grid_to_world)
        assert np.array_equal(faces, rf) and _ulp_close(verts, rv).all()
    finally:
        utils.set_args(utils.default_args())


# ------------------------------------------------------------------------------------------------ 4. CLI
def _shell_rows(n=12000, radius=12.0):
    """An opaque shell of flat Gaussians around every camera of tests/golden/colmap_tiny (they sit within 9 of the origin
    and look in all directions): each camera sees a patch of its inside."""
    k = torch.arange(n, dtype=torch.float64) + 0.5
    zc = 1 - 2 * k / n
    phi = k * math.pi * (3 - math.sqrt(5))
    s = torch.sqrt(1 - zc * zc)
    d = torch.stack([s * torch.cos(phi), s * torch.sin(phi), zc], 1)
    q = torch.nn.functional.normalize(torch.stack([1 + d[:, 2], -d[:, 1], d[:, 0], torch.zeros(n, dtype=torch.float64)], 1))
    shs = torch.zeros(n, 16, 3)
    shs[:, 0, :] = d.float()
    return dict(xyz=(radius * d).float(), shs48=shs.reshape(n, 48), opacity=torch.full((n, 1), 6.0),
                scaling=torch.log(torch.tensor([0.35, 0.35, 0.01])).expand(n, 3).contiguous(), rotation=q.float())


def test_cli_on_a_ply_and_a_compressed_model(dev, tmp_path, capsys):
    from clm_gs_amd import compress_model, io_ply, mesh_model, utils
    scene = os.path.join(ROOT, "tests", "golden", "colmap_tiny")
    rows = _shell_rows()
    ply, npz = str(tmp_path / "shell.ply"), str(tmp_path / "shell.vq.npz")
    io_ply.save_ply(ply, rows["xyz"], rows["shs48"], rows["opacity"], rows["scaling"], rows["rotation"])
    try:
        assert compress_model.main(["-m", ply, "-o", npz, "--codebook", "16", "--iters", "1"]) == 0
        box = ["--bounds", "-14", "-14", "-14", "14", "14", "14"]
        out = tmp_path / "refused"
        for extra, match in ((["--voxel", "0"], "--voxel must be positive"),
                             (["--voxel", "1", "--bounds", "0", "0", "0", "1", "1", "-1"], "--bounds"),
                             (["--voxel", "0.01", "--grid_gb", "1"] + box, "--grid_gb 1; --voxel")):
            with pytest.raises(SystemExit, match=match):
                mesh_model.main(["-m", ply, "-s", scene, "-o", str(out / "mesh.ply"), "--no_offload"] + extra)
            assert not out.exists()  # a refusal leaves no output directory
        for model, strategy, every in ((ply, "--no_offload", 1), (npz, "--clm_offload", 2)):
            mesh = str(tmp_path / ("out_" + strategy[2:]) / "mesh.ply")
            capsys.readouterr()
            assert mesh_model.main(["-m", model, "-s", scene, "-o", mesh, "--voxel", "1", "--min_weight", "1",
                                    "--every", str(every), strategy] + box) == 0
            line = capsys.readouterr().out
            assert "render" in line and "integration" in line and "cameras/s" in line, line
            verts, colours, faces = io_ply.load_mesh_ply(mesh)
            meta = json.load(open(mesh[:-4] + ".json"))
            print(line.strip())
            assert meta["vertices"] == len(verts) == len(colours) and meta["faces"] == len(faces)
            assert meta["grid"] == [28, 28, 28] and meta["voxel"] == 1.0 and meta["bounds"] == [-14.0] * 3 + [14.0] * 3
            assert meta["cameras"] == len(meta["camera_names"]) == 12 // every and meta["up"] == [0.0, 0.0, 1.0]
            assert len(verts) > 0 and len(faces) > 0
            assert int(faces.min()) >= 0 and int(faces.max()) < len(verts)
            r = np.linalg.norm(verts.astype(np.float64), axis=1)  # the surface found is the shell
            assert float(np.abs(r - 12.0).max()) < 4.0, (float(r.min()), float(r.max()))  # inside the truncation band (4 voxels)
    finally:
        utils.set_args(utils.default_args())


def test_trainer_mesh_voxel(dev, tmp_path):
    """trainer --mesh_voxel writes <model>/mesh.ply and mesh.json after the final .ply and logs the line."""
    from clm_gs_amd import io_ply, trainer
    from tests.test_gpu_exposure import _tiny_scene
    work, out = _tiny_scene(tmp_path), tmp_path / "out"
    trainer.train_from_colmap(str(work), str(out), strategy="clm_offload", iterations=8, bsz=4,
                              disable_auto_densification=True, mesh_voxel=0.5, mesh_min_weight=1.0)
    assert (out / "point_cloud" / "iteration_8" / "point_cloud.ply").exists()
    verts, colours, faces = io_ply.load_mesh_ply(str(out / "mesh.ply"))
    meta = json.load(open(out / "mesh.json"))
    assert meta["vertices"] == len(verts) and meta["faces"] == len(faces) and meta["voxel"] == 0.5 and meta["cameras"] > 0
    assert len(faces) == 0 or int(faces.max()) < len(verts)
    assert "mesh export: grid" in open(out / "python_ws=1_rk=0.log").read()


# ------------------------------------------------------------------------------------------------ 5. entries
def test_entries_refuse_bad_arguments(dev):
    """CLMGS_EINVAL before anything is launched: null and misaligned pointers, overlapping outputs, B outside 1..16,
    non-finite or non-positive trunc / fx / fy / min_weight, sizes beyond the limits."""
    from clm_gs_amd import _lib, clm_kernels
    L, EINVAL = _lib.lib(), 10001  # CLMGS_EINVAL (include/clmgs.h)
    nx, ny, nz, B, h, w = 4, 3, 2, 2, 5, 6
    n = nx * ny * nz
    grid = torch.zeros((6, nz, ny, nx), device=dev)
    depth, alpha, rgb = torch.full((B, h, w), 2.5, device=dev), torch.ones((B, h, w), device=dev), torch.ones((B, 3, h, w), device=dev)
    cams = np.tile(np.array([1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 1, 10, 10, 3, 2.5], dtype=np.float64), (16, 1))
    P = lambda t, off=0: ctypes.c_void_p(t.data_ptr() + off)
    rec = lambda c: (ctypes.c_double * c.size)(*c.reshape(-1))
    s = _lib.stream

    def integrate(nx=nx, ny=ny, nz=nz, grid=P(grid), B=B, h=h, w=w, depth=P(depth), alpha=P(alpha), rgb=P(rgb), cams=cams,
                  trunc=0.5, inv_trunc=2.0, cull=1):
        return L.clmgs_tsdf_integrate(s(), nx, ny, nz, grid, B, h, w, depth, alpha, rgb, None if cams is None else rec(cams),
                                      0.01, 10.0, 0.5, trunc, inv_trunc, cull)

    assert integrate() == 0
    bad_fx, bad_fy, bad_m = cams.copy(), cams.copy(), cams.copy()
    bad_fx[1, 12], bad_fy[0, 13], bad_m[1, 3] = 0.0, float("nan"), float("inf")
    for kw in (dict(grid=None), dict(depth=None), dict(alpha=None), dict(rgb=None), dict(cams=None),
               dict(grid=P(grid, 2)), dict(depth=P(depth, 1)), dict(rgb=P(rgb, 2)),
               dict(depth=P(grid)), dict(rgb=P(grid, 4 * n)), dict(alpha=P(grid, 24 * n - 4)),
               dict(B=0), dict(B=17), dict(B=-1),
               dict(trunc=0.0), dict(trunc=-1.0), dict(trunc=float("nan")), dict(trunc=float("inf")), dict(inv_trunc=0.0),
               dict(inv_trunc=float("nan")), dict(cams=bad_fx), dict(cams=bad_fy), dict(cams=bad_m),
               dict(nx=1), dict(nz=0), dict(nx=2048, ny=2048, nz=512), dict(nx=1 << 16, ny=1 << 16, nz=2),
               dict(h=0), dict(w=32769), dict(cull=2)):
        assert integrate(**kw) == EINVAL, kw
    assert torch.count_nonzero(grid[1]).item() > 0  # (the one good call ran: the voxels at z = 2.5 meet the surface)
    count, scan = torch.zeros(n, dtype=torch.int32, device=dev), torch.ones(n, dtype=torch.int32, device=dev).cumsum(0, dtype=torch.int32)
    verts, colours = torch.zeros((n, 3), device=dev), torch.zeros((n, 3), dtype=torch.uint8, device=dev)
    faces = torch.zeros((6 * n, 3), dtype=torch.int32, device=dev)
    g2w = np.array([[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, 0]], dtype=np.float64)
    g2w_bad = g2w.copy()
    g2w_bad[2, 3] = float("nan")
    cells = lambda grid=P(grid), mw=1.0, out=P(count), nx=nx: L.clmgs_tsdf_cells(s(), nx, ny, nz, grid, mw, out)
    assert cells() == 0
    for kw in (dict(grid=None), dict(out=None), dict(out=P(count, 2)), dict(out=P(grid, 8)), dict(mw=0.0), dict(mw=-1.0),
               dict(mw=float("nan")), dict(mw=float("inf")), dict(nx=1)):
        assert cells(**kw) == EINVAL, kw
    vertices = lambda grid=P(grid), scan=P(scan), V=n, g=g2w, verts=P(verts), colours=P(colours): \
        L.clmgs_tsdf_vertices(s(), nx, ny, nz, grid, scan, V, None if g is None else rec(g), verts, colours)
    for kw in (dict(grid=None), dict(scan=None), dict(g=None), dict(verts=None), dict(colours=None), dict(V=0), dict(V=n + 1),
               dict(g=g2w_bad), dict(verts=P(verts, 2)), dict(colours=P(verts, 4)), dict(verts=P(grid)), dict(colours=P(scan)),
               dict(verts=P(scan))):
        assert vertices(**kw) == EINVAL, kw
    quad_count = lambda grid=P(grid), mw=1.0, scan=P(scan), out=P(count): L.clmgs_tsdf_quad_count(s(), nx, ny, nz, grid, mw, scan, out)
    for kw in (dict(grid=None), dict(scan=None), dict(out=None), dict(out=P(scan)), dict(out=P(grid, 4)), dict(mw=0.0),
               dict(out=P(count, 1))):
        assert quad_count(**kw) == EINVAL, kw
    quads = lambda grid=P(grid), mw=1.0, scan=P(scan), qscan=P(scan), V=n, Q=n, out=P(faces): \
        L.clmgs_tsdf_quads(s(), nx, ny, nz, grid, mw, scan, qscan, V, Q, out)
    for kw in (dict(grid=None), dict(scan=None), dict(qscan=None), dict(out=None), dict(V=0), dict(Q=0), dict(Q=1 << 30),
               dict(out=P(scan)), dict(out=P(grid, 16)), dict(mw=float("nan")), dict(out=P(faces, 2))):
        assert quads(**kw) == EINVAL, kw
    torch.cuda.synchronize()
    # the operators refuse what they can name
    with pytest.raises(_lib.ClmgsError, match="volume"):
        clm_kernels.tsdf_extract(grid[:5], 2.0, g2w)
    with pytest.raises(_lib.ClmgsError, match="volume"):
        clm_kernels.tsdf_extract(grid.cpu(), 2.0, g2w)
    with pytest.raises(ValueError, match="min_weight"):
        clm_kernels.tsdf_extract(grid, 0.0, g2w)
    with pytest.raises(ValueError, match="trunc"):
        clm_kernels.tsdf_integrate(grid, depth, alpha, rgb, cams[:B], trunc=0.0)
    with pytest.raises(_lib.ClmgsError, match="alpha"):
        clm_kernels.tsdf_integrate(grid, depth, alpha[:, :4], rgb, cams[:B], trunc=1.0)
    with pytest.raises(_lib.ClmgsError, match="cams"):
        clm_kernels.tsdf_integrate(grid, depth, alpha, rgb, cams[:1], trunc=1.0)
