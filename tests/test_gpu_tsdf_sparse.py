"""Sparse volume on the device ("Sparse volume"): csrc/tsdf_sparse.hip through clm_kernels.tsdf_mark /
tsdf_sparse_integrate / tsdf_sparse_extract, tsdf.SparseTsdfVolume and mesh_model --sparse.  The marks against the numpy
restatement (tests/tsdf_sparse_reference.py), the stored sums against the dense kernel bit for bit, and the acceptance
test: the sparse volume extracts the tensors the dense volume extracts -- vertices by bit pattern, colours, faces -- up to
mesh.ply byte for byte through the command line, and on a box of 2^33 voxels that the dense volume refuses."""
import ctypes
import json
import math
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from tests import tsdf_reference as R
from tests import tsdf_sparse_reference as SR

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_CACHE = {}
FRAME = (np.eye(3)[0], np.eye(3)[1], np.eye(3)[2])
SPHERE_BOUNDS = (-2.4, -2.0, -2.0, 2.4, 2.0, 2.0)
GATES = dict(near=SR.NEAR, depth_max=SR.DEPTH_MAX, alpha_min=SR.ALPHA_MIN)
CORNER_CENTRE = tuple(c + 0.9 / math.sqrt(3.0) for c in (0.0, -0.4, -0.4))  # the sphere passes through the brick corner (24, 16, 16)


def _dev(scene, dev, key, sel=slice(None)):
    return torch.from_numpy(np.ascontiguousarray(scene[key][sel])).to(dev)


def _mark(scene, dev, splits, gates=GATES, trunc=SR.TRUNC, voxel=SR.VOXEL):
    from clm_gs_amd import clm_kernels
    nbx, nby, nbz = SR.brick_grid(scene["shape"])
    marks = torch.zeros((nbz, nby, nbx), dtype=torch.uint8, device=dev)
    for sel in splits:
        clm_kernels.tsdf_mark(marks, scene["shape"], _dev(scene, dev, "depth", sel), _dev(scene, dev, "alpha", sel),
                              scene["cams_inv"][sel], trunc=trunc, voxel_cam=voxel, **gates)
    return marks


def _volume(scene, dev, bounds=SPHERE_BOUNDS, voxel=SR.VOXEL, gates=GATES, trunc=SR.TRUNC):
    """A SparseTsdfVolume of the scene's box, marked by the kernel and allocated."""
    from clm_gs_amd import tsdf
    v = tsdf.SparseTsdfVolume(FRAME, bounds, voxel, trunc_voxels=trunc / voxel, device=dev)
    assert v.shape == tuple(scene["shape"]) and np.array_equal(v.grid_to_world, scene["g2w"])
    v.marks.copy_(_mark(scene, dev, [slice(None)], gates, trunc, voxel))
    v.allocate()
    return v


def _fuse_sparse(scene, dev, v, splits, cull=True, gates=GATES, trunc=SR.TRUNC):
    from clm_gs_amd import clm_kernels
    for sel in splits:
        clm_kernels.tsdf_sparse_integrate(v.pool, v.bricks, v.shape, _dev(scene, dev, "depth", sel), _dev(scene, dev, "alpha", sel),
                                          _dev(scene, dev, "rgb", sel), scene["cams"][sel], trunc=trunc, cull=cull, **gates)
    return v


def _fuse_dense(scene, dev, gates=GATES, trunc=SR.TRUNC):
    from clm_gs_amd import clm_kernels
    nx, ny, nz = scene["shape"]
    grid = torch.zeros((6, nz, ny, nx), dtype=torch.float32, device=dev)
    return clm_kernels.tsdf_integrate(grid, _dev(scene, dev, "depth"), _dev(scene, dev, "alpha"), _dev(scene, dev, "rgb"),
                                      scene["cams"], trunc=trunc, **gates)


def _bits(t):
    return t.contiguous().view(torch.int32)


def _same_mesh(a, b, what=""):
    (av, ac, af), (bv, bc, bf) = a, b
    assert av.shape == bv.shape and af.shape == bf.shape, (what, av.shape, bv.shape, af.shape, bf.shape)
    assert av.dtype == torch.float32 and ac.dtype == torch.uint8 and af.dtype == torch.int32
    assert torch.equal(_bits(av), _bits(bv)), what
    assert torch.equal(ac, bc) and torch.equal(af, bf), what


# ------------------------------------------------------------------------------------------------ 1. marks
def test_marks_equal_the_reference_and_do_not_depend_on_the_split(dev):
    sc = SR.sphere_scene()
    ref, band, slabs, lo, hi = SR.scene_marks(sc)
    whole = _mark(sc, dev, [slice(0, 12)])
    got = whole.cpu().numpy().astype(bool)
    print(f"marks: {int(got.sum())} of {got.size} bricks, reference {int(ref.sum())}, band {band} of {slabs} pixel-slabs")
    assert band <= 1e-3 * slabs
    assert (got | ~lo).all() and (hi | ~got).all()  # exactly the reference outside the band (lo == hi == ref when band == 0)
    if band == 0:
        assert np.array_equal(got, ref)
    need = SR.dilate(SR.scene_negative(sc), 1)  # ... and inside it still a superset of the minimal coverage
    assert (SR.voxels(got, sc["shape"]) | ~need).all()
    assert 0 < int(got.sum()) < got.size / 2
    one_by_one = _mark(sc, dev, [slice(b, b + 1) for b in range(12)])
    split = _mark(sc, dev, [slice(5, 12), slice(0, 5)])
    assert torch.equal(whole, one_by_one) and torch.equal(whole, split)
    assert set(torch.unique(whole).tolist()) == {0, 1}


# ------------------------------------------------------------------------------------------------ 2. fusion
def test_stored_voxels_carry_the_dense_sums(dev):
    sc = SR.sphere_scene()
    v = _fuse_sparse(sc, dev, _volume(sc, dev), [slice(0, 12)])
    marks = v.marks.cpu().numpy().astype(bool)
    assert v.S == int(marks.sum()) and v.pool.shape == (v.S, 6, 8, 8, 8)
    got = v.to_dense()
    dense = _fuse_dense(sc, dev)
    want = torch.from_numpy(SR.restrict(dense.cpu().numpy(), marks)).to(dev)
    assert torch.equal(_bits(got), _bits(want))  # the dense kernel's bits wherever a brick is stored, zero elsewhere
    assert float(got[1].max()) >= 3 and float(got[0].min()) < 0 < float(got[0].max())
    # the numpy fusion outside tsdf_reference's band
    ref, band = SR.scene_dense(sc)
    ref = SR.restrict(ref, marks)
    n_band = int((band > 0).sum())
    print(f"fusion: S {v.S}, band voxels {n_band} of {band.size}")
    assert n_band <= 1e-3 * band.size
    g = got.cpu().numpy()
    for p, name in enumerate(("tsum", "wsum", "cr", "cg", "cb", "cw")):
        a, b = g[p][band == 0].view(np.int32), ref[p][band == 0].view(np.int32)
        assert np.array_equal(a, b), f"plane {name} differs in {int((a != b).sum())} voxels outside the band"
    for p in (1, 5):
        assert (np.abs(g[p] - ref[p]) <= band).all()
    # split invariance, the cull, and a second integrate on the same volume
    one_by_one = _fuse_sparse(sc, dev, _volume(sc, dev), [slice(b, b + 1) for b in range(12)])
    split = _fuse_sparse(sc, dev, _volume(sc, dev), [slice(0, 5), slice(5, 12)])
    no_cull = _fuse_sparse(sc, dev, _volume(sc, dev), [slice(0, 12)], cull=False)
    for other in (one_by_one, split, no_cull):
        assert torch.equal(_bits(other.pool), _bits(v.pool))
    again = _fuse_sparse(sc, dev, v, [slice(0, 12)])
    assert torch.equal(again.to_dense()[1], 2 * want[1]) and torch.equal(again.to_dense()[5], 2 * want[5])


# ------------------------------------------------------------------------------------------------ 3. mesh equality
NX, NY, NZ = 20, 18, 16
NOISY_GATES = dict(near=2.2, depth_max=4.2, alpha_min=0.5)


def _noisy_scene():
    """The fusion case of tests/test_gpu_tsdf.py rebuilt: 17 random poses about a 2.0 x 1.8 x 1.6 box (sides that are no
    multiples of 8: border bricks), depth maps scattered about the distance to the box, alpha on both sides of the gate."""
    if "noisy" in _CACHE:
        return _CACHE["noisy"]
    Hn, Wn, n_cams = 33, 47, 17
    rng = np.random.default_rng(20)
    g2w = np.array([[0.1, 0, 0, -1.0], [0, 0.1, 0, -0.9], [0, 0, 0.1, -0.8]])
    g4 = np.vstack([g2w, [0, 0, 0, 1.0]])
    cams = np.empty((n_cams, 16))
    for b in range(n_cams):
        d = rng.normal(size=3)
        C = d / np.linalg.norm(d) * rng.uniform(2.5, 4.0)
        target = rng.uniform(-1.2, 1.2, size=3) if b % 6 != 5 else 2.0 * C
        w2c = SR.look_at(C, target, rng.normal(size=3))
        cams[b, :12] = (w2c @ g4)[:3].reshape(12)
        cams[b, 12:] = (rng.uniform(35, 70), rng.uniform(35, 70), Wn / 2 + rng.uniform(-3, 3), Hn / 2 + rng.uniform(-3, 3))
    depth = rng.uniform(1.8, 4.6, size=(n_cams, Hn, Wn)).astype(np.float32)
    depth[rng.random(depth.shape) < 0.05] = 0.0
    alpha = rng.uniform(0.2, 1.0, size=(n_cams, Hn, Wn)).astype(np.float32)
    rgb = rng.uniform(-0.3, 1.3, size=(n_cams, 3, Hn, Wn)).astype(np.float32)
    _CACHE["noisy"] = dict(shape=(NX, NY, NZ), g2w=g2w, cams=cams, cams_inv=SR.invert_records(cams), depth=depth, alpha=alpha,
                           rgb=rgb)
    return _CACHE["noisy"]


MESH_CASES = {
    "sphere": lambda: (SR.sphere_scene(), SPHERE_BOUNDS, GATES),
    "corner": lambda: (SR.sphere_scene(centre=CORNER_CENTRE), SPHERE_BOUNDS, GATES),
    "noisy": lambda: (_noisy_scene(), (-1.0, -0.9, -0.8, 1.0, 0.9, 0.8), NOISY_GATES),
}


@pytest.mark.parametrize("name", sorted(MESH_CASES))
def test_sparse_mesh_equals_the_dense_mesh(dev, name):
    """The acceptance test.  "corner": the sphere shifted so that its surface passes through a corner of the brick grid and
    crosses the faces and edges that meet there; at least one quad has its four cells in four different bricks."""
    from clm_gs_amd import clm_kernels
    sc, bounds, gates = MESH_CASES[name]()
    nx, ny, nz = sc["shape"]
    splits = [slice(0, 16), slice(16, None)] if name == "noisy" else [slice(None)]
    v = _fuse_sparse(sc, dev, _volume(sc, dev, bounds, gates=gates), splits, gates=gates)
    dense = _fuse_dense(sc, dev, gates=gates)
    if name == "noisy":  # every brick is marked: the border bricks of a 20 x 18 x 16 grid hold voxels beyond it
        assert bool(v.marks.all()) and v.S == 3 * 3 * 2
        assert torch.equal(_bits(v.to_dense()), _bits(dense))
    else:
        assert 0 < v.S < v.bricks_total / 2
    for min_weight in (1.0, 2.0):
        want = clm_kernels.tsdf_extract(dense, min_weight, sc["g2w"])
        got = v.extract(min_weight)
        print(f"{name} min_weight {min_weight:g}: S {v.S} of {v.bricks_total}, V {want[0].shape[0]} F {want[2].shape[0]}")
        assert want[0].shape[0] > 100 and want[2].shape[0] > (20 if name == "noisy" else 100)
        _same_mesh(got, want, f"{name} {min_weight}")
    if name != "corner":
        return
    verts, colours, faces, vkeys, qkeys = (t.cpu().numpy() for t in clm_kernels.tsdf_sparse_extract(
        v.pool, v.bricks, v.table, v.shape, 2.0, sc["g2w"], want_keys=True))
    assert (np.diff(vkeys) > 0).all() and (np.diff(qkeys) > 0).all() and len(qkeys) * 2 == len(faces)
    owner, axis = qkeys // 3, qkeys % 3
    p = np.stack([owner % nx, (owner // nx) % ny, owner // (nx * ny)], 1)
    four = 0
    for q in range(len(qkeys)):
        a1, a2 = (axis[q] + 1) % 3, (axis[q] + 2) % 3
        cells = []
        for d1, d2 in ((-1, -1), (0, -1), (0, 0), (-1, 0)):
            c = p[q].copy()
            c[a1] += d1
            c[a2] += d2
            cells.append(tuple(c // 8))
        four += len(set(cells)) == 4
    print(f"corner: {four} of {len(qkeys)} quads have their cells in four bricks")
    assert four >= 1


def _pack(grid, marks, dev):
    """A dense grid [6,nz,ny,nx] -> (pool, bricks, table) of the marked bricks: the inverse of SparseTsdfVolume.to_dense."""
    _, nz, ny, nx = grid.shape
    nbz, nby, nbx = marks.shape
    full = torch.zeros((6, nbz * 8, nby * 8, nbx * 8), dtype=torch.float32)
    full[:, :nz, :ny, :nx] = torch.from_numpy(grid)
    full = full.reshape(6, nbz, 8, nby, 8, nbx, 8).permute(1, 3, 5, 0, 2, 4, 6).reshape(-1, 6, 8, 8, 8)
    flat = torch.from_numpy(np.ascontiguousarray(marks)).reshape(-1)
    scan = torch.cumsum(flat, 0, dtype=torch.int32)
    table = torch.where(flat, scan - 1, torch.full_like(scan, -1)).reshape(nbz, nby, nbx)
    bricks = torch.nonzero(flat).reshape(-1)
    return full[bricks].contiguous().to(dev), bricks.to(torch.int32).to(dev), table.contiguous().to(dev)


def test_missing_bricks_next_to_the_surface(dev):
    """tsdf_sparse_extract on a pool packed from a dense grid, where -- unlike in a fused volume -- bricks are missing right
    next to active cells: the "not stored" branch of the neighbour lookup decides cells and quads.  The result must be the
    dense extraction of the grid restricted to the stored bricks.  The counts (the numpy reference) show that the missing
    bricks matter on this input.  And the smallest grid with a quad, as one brick."""
    from clm_gs_amd import clm_kernels
    from tests.test_gpu_tsdf import EXTRACT_CASES
    grid, g2w = EXTRACT_CASES["random"]()  # 31 x 27 x 23 voxels: 4 x 4 x 3 bricks, border bricks on every axis
    marks = np.random.default_rng(7).random((3, 4, 4)) < 0.7
    restricted = SR.restrict(grid, marks)
    assert int(marks.sum()) == 35
    (rv, _, rf, _), (fv, _, ff, _) = R.extract(restricted, 2.0, g2w), R.extract(grid, 2.0, g2w)
    assert (len(rv), len(rf)) == (1012, 224) and (len(fv), len(ff)) == (1534, 332)
    want = clm_kernels.tsdf_extract(torch.from_numpy(restricted).to(dev), 2.0, g2w)
    got = clm_kernels.tsdf_sparse_extract(*_pack(grid, marks, dev), (31, 27, 23), 2.0, g2w)
    assert want[0].shape[0] == 1012 and want[2].shape[0] == 224
    _same_mesh(got, want, "random, 35 of 48 bricks")
    grid, g2w = EXTRACT_CASES["one_voxel"]()
    want = clm_kernels.tsdf_extract(torch.from_numpy(grid).to(dev), 2.0, g2w)
    got = clm_kernels.tsdf_sparse_extract(*_pack(grid, np.ones((1, 1, 1), dtype=bool), dev), (3, 3, 3), 2.0, g2w)
    assert got[0].shape[0] == 8 and got[2].shape[0] == 12
    _same_mesh(got, want, "one voxel")


def test_no_observation_is_an_empty_result(dev):
    from clm_gs_amd import tsdf
    sc = dict(SR.sphere_scene())
    sc["alpha"] = np.zeros_like(sc["alpha"])
    v = _volume(sc, dev)
    assert v.S == 0 and not bool(v.marks.any()) and int((v.table != -1).sum()) == 0
    cam = SimpleNamespace(_clmgs_host=(np.eye(4).reshape(16), np.array([[70.0, 0, 40], [0, 70, 30], [0, 0, 1]]).reshape(9), None),
                          image_name="c")
    v.add(cam, _dev(sc, dev, "rgb")[0], _dev(sc, dev, "depth")[0], _dev(sc, dev, "alpha")[0])
    verts, colours, faces = v.extract(1.0)
    assert verts.shape == (0, 3) and colours.shape == (0, 3) and faces.shape == (0, 3) and v.cameras_used == 1
    assert not bool(v.to_dense().any())
    with pytest.raises(ValueError, match="add\\(\\) before allocate"):
        tsdf.SparseTsdfVolume(FRAME, SPHERE_BOUNDS, 0.1, device=dev).add(cam, None, None, None)


# ------------------------------------------------------------------------------------------------ 4. end to end
def _json_without_sparse(path):
    meta = json.load(open(path))
    return meta, {k: v for k, v in meta.items() if k != "sparse"}


@pytest.mark.parametrize("strategy", ["no_offload", "clm_offload"])
def test_plane_end_to_end_sparse_equals_dense(dev, strategy, tmp_path):
    """The rendered plane of tests/test_gpu_tsdf.py through build_mesh with and without sparse: the same mesh.ply byte for
    byte, mesh.json differing by "sparse" only -- which needs the second pass to render the depth maps of the first."""
    from clm_gs_amd import mesh_model, utils
    from clm_gs_amd.render_ortho import map_frame
    from clm_gs_amd.render_trajectory import eval_one_cam
    from tests.test_gpu_tsdf import CAM_XY, PH, PLANE_BOUNDS, PLANE_VOXEL, PW, _nadir_camera, _plane_rows
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
        m = M(3, only_for_rendering=True)
        m.create_from_tensors(*_plane_rows(dev), spatial_lr_scale=1.0)
        m.active_sh_degree = 3
        cams = [_nadir_camera(i, x, y, dev) for i, (x, y) in enumerate(CAM_XY)]
        with torch.no_grad():  # two renders of one camera are bit-equal
            first = [t.clone() for t in eval_one_cam(cams[1], m, None, args, render_mode="RGB+ED")]
            other = [t.clone() for t in eval_one_cam(cams[3], m, None, args, render_mode="RGB+ED")]
            second = [t.clone() for t in eval_one_cam(cams[1], m, None, args, render_mode="RGB+ED")]
        for a, b in zip(first, second):
            assert torch.equal(_bits(a), _bits(b))
        assert not torch.equal(first[0], other[0])
        paths = {}
        for sparse in (False, True):
            paths[sparse] = str(tmp_path / ("sparse" if sparse else "dense") / "mesh.ply")
            log = open(str(tmp_path / "log.txt"), "w")
            meta = mesh_model.build_mesh(m, cams, args, paths[sparse], PLANE_VOXEL, frame=map_frame(), bounds=PLANE_BOUNDS,
                                         log=log, sparse=sparse)
            log.close()
            line = open(str(tmp_path / "log.txt")).read()
            assert ("sparse bricks" in line and "marking" in line) == sparse, line
        assert open(paths[True], "rb").read() == open(paths[False], "rb").read()
        sparse_meta, rest = _json_without_sparse(mesh_model.json_path(paths[True]))
        dense_meta, _ = _json_without_sparse(mesh_model.json_path(paths[False]))
        assert rest == dense_meta and "sparse" not in dense_meta and dense_meta["vertices"] > 500
        s = sparse_meta["sparse"]
        print(f"plane/{strategy}: {s}")
        assert s["bricks_total"] == 5 * 5 * 3 and 0 < s["bricks"] < s["bricks_total"] and s["pool_gb"] == s["bricks"] * 12288 / 1e9
    finally:
        utils.set_args(utils.default_args())


def test_cli_sparse_writes_the_same_bytes(dev, tmp_path, capsys):
    from clm_gs_amd import io_ply, mesh_model, utils
    from tests.test_gpu_tsdf import _shell_rows
    scene = os.path.join(ROOT, "tests", "golden", "colmap_tiny")
    rows = _shell_rows()
    ply = str(tmp_path / "shell.ply")
    io_ply.save_ply(ply, rows["xyz"], rows["shs48"], rows["opacity"], rows["scaling"], rows["rotation"])
    box = ["--bounds", "-14", "-14", "-14", "14", "14", "14"]
    try:
        for extra in ([], ["--min_component_faces", "8"]):  # the cleanup composes
            out = {}
            for flag in ([], ["--sparse"]):
                out[bool(flag)] = str(tmp_path / ("s" if flag else "d") / ("c" if extra else "p") / "mesh.ply")
                capsys.readouterr()
                assert mesh_model.main(["-m", ply, "-s", scene, "-o", out[bool(flag)], "--voxel", "1", "--min_weight", "1",
                                        "--no_offload"] + box + extra + flag) == 0
                line = capsys.readouterr().out
                assert ("sparse bricks" in line) == bool(flag), line
            assert open(out[True], "rb").read() == open(out[False], "rb").read()
            sparse_meta, rest = _json_without_sparse(mesh_model.json_path(out[True]))
            assert rest == json.load(open(mesh_model.json_path(out[False]))) and rest["faces"] > 0
            assert sparse_meta["sparse"]["bricks_total"] == 64 and ("cleanup" in rest) == bool(extra)
    finally:
        utils.set_args(utils.default_args())


# ------------------------------------------------------------------------------------------------ 5. capacity
def test_a_box_the_dense_volume_refuses(dev):
    """4096 x 4096 x 512 voxels = 2^33, four times the dense index limit: 512 x 512 x 64 = 16.8 M bricks, of which one
    64 x 64 nadir camera over the plane u = 0 allocates a handful.  Voxel, bounds and the camera position are dyadic, so
    the camera records of the big box and of a dense 64 x 64 x 32 sub-box about the patch are exact and both volumes
    compute the same sums: the faces are equal, and the vertices' cell indices after translation."""
    from clm_gs_amd import clm_kernels, tsdf
    voxel, big = 1.0 / 16, (-128.0, -128.0, -16.0, 128.0, 128.0, 16.0)
    with pytest.raises(ValueError, match="2\\^31 voxels"):
        tsdf.TsdfVolume(FRAME, big, voxel, device=dev, grid_gb=1000.0)
    cam_xy, height, hw, focal = (10.25, -7.75), 3.0, 64, 100.0
    Rm = np.diag([1.0, -1.0, -1.0])
    w2c = np.eye(4)
    w2c[:3, :3] = Rm
    w2c[:3, 3] = -Rm @ np.array([cam_xy[0], cam_xy[1], height])
    K = np.array([[focal, 0, hw / 2], [0, focal, hw / 2], [0, 0, 1.0]])
    cam = SimpleNamespace(_clmgs_host=(w2c.reshape(16), K.reshape(9), None), image_name="nadir")
    rng = np.random.default_rng(3)
    depth = torch.full((hw, hw), height, device=dev)
    alpha = torch.ones((hw, hw), device=dev)
    image = torch.from_numpy(rng.uniform(0, 1, size=(3, hw, hw)).astype(np.float32)).to(dev)
    v = tsdf.SparseTsdfVolume(FRAME, big, voxel, device=dev)
    assert v.shape == (4096, 4096, 512) and (v.nbx, v.nby, v.nbz) == (512, 512, 64)
    v.mark(cam, depth, alpha)
    S = v.allocate()
    print(f"capacity: {S} of {v.bricks_total} bricks, {v.nbytes / 1e9:.3f} GB")
    assert 8 <= S <= 400 and v.cameras_marked == 1
    v.add(cam, image, depth, alpha)
    v.flush()
    verts, colours, faces, vkeys, qkeys = clm_kernels.tsdf_sparse_extract(v.pool, v.bricks, v.table, v.shape, 1.0, v.grid_to_world,
                                                                          want_keys=True)
    _same_mesh(v.extract(1.0), (verts, colours, faces))
    assert verts.shape[0] > 300 and faces.shape[0] > 600
    assert float(verts[:, 2].abs().max()) <= voxel  # every vertex within one voxel of the plane
    # the dense volume over a sub-box about the patch: voxels (2180.., 1892.., 240..) of the big box, not brick-aligned
    origin = (2180, 1892, 240)
    lo = [big[a] + origin[a] * voxel for a in range(3)]
    sub = tsdf.TsdfVolume(FRAME, tuple(lo) + (lo[0] + 64 * voxel, lo[1] + 64 * voxel, lo[2] + 32 * voxel), voxel, device=dev)
    assert (sub.nx, sub.ny, sub.nz) == (64, 64, 32)
    sub.add(cam, image, depth, alpha)
    sv, sc, sf = sub.extract(1.0)
    assert torch.equal(faces, sf) and torch.equal(colours, sc)
    assert float((verts - sv).abs().max()) <= 1e-5
    k = vkeys.cpu().numpy()
    cell = np.stack([k % 4096, (k // 4096) % 4096, k // (4096 * 4096)], 1) - np.array(origin)
    _, _, rf, cells = R.extract(sub.grid.cpu().numpy(), 1.0, sub.grid_to_world)
    assert np.array_equal(cell, cells) and np.array_equal(rf, sf.cpu().numpy())
    assert int(qkeys.max()) >= 1 << 31  # the keys need their 64 bits


# ------------------------------------------------------------------------------------------------ 6. entries
def test_sparse_entries_refuse_bad_arguments(dev):
    """CLMGS_EINVAL before anything is launched: null and misaligned pointers, overlaps, B outside 1..16, non-finite
    records, sizes beyond the limits; and the operators refuse what they can name, a table that does not belong to the
    pool among it."""
    from clm_gs_amd import _lib, clm_kernels
    L, EINVAL = _lib.lib(), 10001  # CLMGS_EINVAL (include/clmgs.h)
    nx, ny, nz, B, h, w = 12, 9, 10, 2, 5, 6   # 2 x 2 x 2 bricks
    S = 3
    marks = torch.zeros((2, 2, 2), dtype=torch.uint8, device=dev)
    depth, alpha, rgb = torch.full((B, h, w), 2.5, device=dev), torch.ones((B, h, w), device=dev), torch.ones((B, 3, h, w), device=dev)
    cams = np.tile(np.array([1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 1, 10, 10, 3, 2.5], dtype=np.float64), (17, 1))
    inv = SR.invert_records(cams)
    bricks = torch.tensor([0, 3, 6], dtype=torch.int32, device=dev)
    table = torch.full((2, 2, 2), -1, dtype=torch.int32, device=dev)
    table.view(-1)[bricks.long()] = torch.arange(S, dtype=torch.int32, device=dev)
    pool = torch.zeros((S, 6, 8, 8, 8), device=dev)
    P = lambda t, off=0: ctypes.c_void_p(t.data_ptr() + off)
    rec = lambda c: (ctypes.c_double * c.size)(*c.reshape(-1))
    s = _lib.stream

    def mark(nx=nx, ny=ny, nz=nz, marks=P(marks), B=B, h=h, w=w, depth=P(depth), alpha=P(alpha), cams=inv[:2], trunc=0.5,
             voxel=1.0):
        return L.clmgs_tsdf_mark(s(), nx, ny, nz, marks, B, h, w, depth, alpha, None if cams is None else rec(cams), 0.01, 10.0,
                                 0.5, trunc, voxel)

    assert mark() == 0
    bad_fx, bad_m, huge = inv.copy(), inv.copy(), inv.copy()
    bad_fx[1, 12], bad_m[0, 3], huge[1, 7] = 0.0, float("nan"), 1e31
    for kw in (dict(marks=None), dict(depth=None), dict(alpha=None), dict(cams=None), dict(depth=P(depth, 2)),
               dict(alpha=P(marks)), dict(marks=P(depth, 8)), dict(B=0), dict(B=17, cams=inv), dict(B=-1),
               dict(trunc=0.0), dict(trunc=float("nan")), dict(voxel=0.0), dict(voxel=float("inf")), dict(voxel=1e-4),
               dict(cams=bad_fx[:2]), dict(cams=bad_m[:2]), dict(cams=huge[:2]), dict(nx=1), dict(nz=0),
               dict(nx=1 << 14, ny=1 << 14, nz=1 << 14), dict(h=0), dict(w=32769)):
        assert mark(**kw) == EINVAL, kw
    assert int(marks.sum()) > 0  # (the one good call ran)

    def integrate(nx=nx, S=S, bricks=P(bricks), pool=P(pool), B=B, h=h, depth=P(depth), alpha=P(alpha), rgb=P(rgb), cams=cams[:2],
                  trunc=0.5, inv_trunc=2.0, cull=1):
        return L.clmgs_tsdf_sparse_integrate(s(), nx, ny, nz, S, bricks, pool, B, h, w, depth, alpha, rgb,
                                             None if cams is None else rec(cams), 0.01, 10.0, 0.5, trunc, inv_trunc, cull)

    assert integrate() == 0
    bad_fy, bad_c = cams.copy(), cams.copy()
    bad_fy[0, 13], bad_c[1, 11] = -1.0, float("inf")
    for kw in (dict(bricks=None), dict(pool=None), dict(depth=None), dict(alpha=None), dict(rgb=None), dict(cams=None),
               dict(pool=P(pool, 2)), dict(bricks=P(bricks, 1)), dict(depth=P(pool)), dict(rgb=P(pool, 4096)),
               dict(bricks=P(pool, 64)), dict(B=0), dict(B=17, cams=cams), dict(S=0), dict(S=9), dict(S=1 << 22),
               dict(trunc=-1.0), dict(inv_trunc=float("nan")), dict(cams=bad_fy[:2]), dict(cams=bad_c[:2]), dict(nx=1),
               dict(h=0), dict(cull=2)):
        assert integrate(**kw) == EINVAL, kw
    assert torch.count_nonzero(pool[:, 1]).item() > 0
    n = S * 512
    count = torch.zeros(n, dtype=torch.int32, device=dev)
    scan = torch.ones(n, dtype=torch.int32, device=dev).cumsum(0, dtype=torch.int32)
    verts, colours = torch.zeros((n, 3), device=dev), torch.zeros((n, 3), dtype=torch.uint8, device=dev)
    vkeys, qkeys = torch.zeros(n, dtype=torch.int64, device=dev), torch.zeros(n, dtype=torch.int64, device=dev)
    faces = torch.zeros((2 * n, 3), dtype=torch.int32, device=dev)
    g2w = np.array([[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, 0]], dtype=np.float64)
    g2w_bad = g2w.copy()
    g2w_bad[1, 1] = float("nan")

    def extract(ps, S=S, bricks=P(bricks), table=P(table), pool=P(pool), mw=1.0, count=P(count), cscan=P(scan), qscan=P(scan), V=n,
                Q=n, g=g2w, verts=P(verts), colours=P(colours), vkeys=P(vkeys), faces=P(faces), qkeys=P(qkeys)):
        return L.clmgs_tsdf_sparse_extract(s(), ps, nx, ny, nz, S, bricks, table, pool, mw, count, cscan, qscan, V, Q,
                                           None if g is None else rec(g), verts, colours, vkeys, faces, qkeys)

    assert extract(0) == 0
    for ps in (-1, 4):
        assert extract(ps) == EINVAL
    for ps in range(4):
        for kw in (dict(bricks=None), dict(table=None), dict(pool=None), dict(S=0), dict(S=9), dict(pool=P(pool, 1))):
            assert extract(ps, **kw) == EINVAL, (ps, kw)
    for ps in (0, 2):
        for kw in (dict(count=None), dict(count=P(count, 2)), dict(count=P(pool, 8)), dict(count=P(table)), dict(mw=0.0),
                   dict(mw=float("nan"))) + ((dict(cscan=None), dict(count=P(scan))) if ps == 2 else ()):
            assert extract(ps, **kw) == EINVAL, (ps, kw)
    for kw in (dict(cscan=None), dict(g=None), dict(g=g2w_bad), dict(verts=None), dict(colours=None), dict(vkeys=None),
               dict(V=0), dict(V=n + 1), dict(verts=P(verts, 2)), dict(vkeys=P(vkeys, 4)), dict(verts=P(pool)),
               dict(colours=P(scan)), dict(vkeys=P(verts)), dict(colours=P(verts, 4)), dict(verts=P(table))):
        assert extract(1, **kw) == EINVAL, kw
    for kw in (dict(cscan=None), dict(qscan=None), dict(faces=None), dict(qkeys=None), dict(V=0), dict(Q=0), dict(Q=1 << 30),
               dict(mw=-1.0), dict(faces=P(scan)), dict(faces=P(pool, 16)), dict(qkeys=P(faces)), dict(faces=P(faces, 2)),
               dict(qkeys=P(qkeys, 4)), dict(qkeys=P(bricks))):
        assert extract(3, **kw) == EINVAL, kw
    torch.cuda.synchronize()
    # the operators refuse what they can name
    shape = (nx, ny, nz)
    with pytest.raises(_lib.ClmgsError, match="marks"):
        clm_kernels.tsdf_mark(marks[:1], shape, depth, alpha, inv[:2])
    with pytest.raises(_lib.ClmgsError, match="alpha"):
        clm_kernels.tsdf_mark(marks, shape, depth, alpha[:, :4], inv[:2])
    with pytest.raises(ValueError, match="voxel_cam"):
        clm_kernels.tsdf_mark(marks, shape, depth, alpha, inv[:2], voxel_cam=0.0)
    with pytest.raises(_lib.ClmgsError, match="pool"):
        clm_kernels.tsdf_sparse_integrate(pool[:, :5], bricks, shape, depth, alpha, rgb, cams[:2])
    with pytest.raises(_lib.ClmgsError, match="bricks must be"):
        clm_kernels.tsdf_sparse_integrate(pool, bricks[:2], shape, depth, alpha, rgb, cams[:2])
    with pytest.raises(_lib.ClmgsError, match="ascending"):
        clm_kernels.tsdf_sparse_integrate(pool, bricks.flip(0).contiguous(), shape, depth, alpha, rgb, cams[:2])
    with pytest.raises(_lib.ClmgsError, match="ascending"):
        clm_kernels.tsdf_sparse_integrate(pool, bricks + 6, shape, depth, alpha, rgb, cams[:2])
    with pytest.raises(ValueError, match="trunc"):
        clm_kernels.tsdf_sparse_integrate(pool, bricks, shape, depth, alpha, rgb, cams[:2], trunc=0.0)
    with pytest.raises(_lib.ClmgsError, match="does not belong to a pool of 2 bricks"):
        clm_kernels.tsdf_sparse_extract(pool[:2], bricks[:2], table, shape, 1.0, g2w)
    other = table.clone()
    other.view(-1)[3], other.view(-1)[4] = -1, 1  # the right slots at the wrong bricks
    with pytest.raises(_lib.ClmgsError, match="does not belong"):
        clm_kernels.tsdf_sparse_extract(pool, bricks, other, shape, 1.0, g2w)
    with pytest.raises(_lib.ClmgsError, match="table must be"):
        clm_kernels.tsdf_sparse_extract(pool, bricks, table[:1], shape, 1.0, g2w)
    with pytest.raises(ValueError, match="min_weight"):
        clm_kernels.tsdf_sparse_extract(pool, bricks, table, shape, 0.0, g2w)
    with pytest.raises(_lib.ClmgsError, match="2\\^30 bricks"):
        clm_kernels.tsdf_brick_grid(1 << 14, 1 << 14, 1 << 14)


def test_trainer_mesh_sparse(dev, tmp_path):
    """trainer --mesh_voxel V --mesh_sparse writes <model>/mesh.ply through the sparse volume: mesh.json carries "sparse",
    the log line the brick counts, and the file is the one mesh_model writes from the saved model without --sparse."""
    from clm_gs_amd import io_ply, mesh_model, trainer, utils
    from tests.test_gpu_exposure import _tiny_scene
    work, out = _tiny_scene(tmp_path), tmp_path / "out"
    try:
        trainer.train_from_colmap(str(work), str(out), strategy="clm_offload", iterations=8, bsz=4,
                                  disable_auto_densification=True, mesh_voxel=0.5, mesh_min_weight=1.0, mesh_sparse=True)
        verts, colours, faces = io_ply.load_mesh_ply(str(out / "mesh.ply"))
        meta = json.load(open(out / "mesh.json"))
        assert meta["vertices"] == len(verts) and meta["faces"] == len(faces) and meta["voxel"] == 0.5
        assert 0 < meta["sparse"]["bricks"] <= meta["sparse"]["bricks_total"]
        assert "sparse bricks" in open(out / "python_ws=1_rk=0.log").read()
        dense = str(tmp_path / "dense" / "mesh.ply")
        assert mesh_model.main(["-m", str(out), "-s", str(work), "-o", dense, "--voxel", "0.5", "--min_weight", "1",
                                "--clm_offload"]) == 0
        assert open(dense, "rb").read() == open(out / "mesh.ply", "rb").read()
    finally:
        utils.set_args(utils.default_args())
