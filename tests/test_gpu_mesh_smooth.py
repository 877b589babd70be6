"""Mesh smoothing and vertex normals on the device ("Mesh smoothing and normals"):
csrc/mesh_smooth.hip through clm_kernels.mesh_incidence / mesh_smooth_step / mesh_vertex_normals, mesh_smooth.smooth, the
mesh export, the clean_mesh tool and the trainer, against the numpy restatement of the contract
(tests/mesh_smooth_reference.py).  Every comparison is exact: array_equal on the float32 positions and normals."""
import json

import numpy as np
import pytest
import torch

from tests import mesh_smooth_reference as S
from tests import tsdf_reference as R
from tests.test_mesh_decimate_cpu import box_sdf

pytestmark = pytest.mark.gpu


def _dev(dev, verts, faces):
    return (torch.from_numpy(np.ascontiguousarray(verts, dtype=np.float32)).to(dev),
            torch.from_numpy(np.ascontiguousarray(faces, dtype=np.int32).reshape(-1, 3)).to(dev))


def _same(got, want, what):
    got = got.cpu().numpy()
    assert got.dtype == want.dtype and got.shape == want.shape, what
    bad = np.nonzero((got != want).any(axis=1))[0]
    assert np.array_equal(got, want), f"{what}: {len(bad)} of {len(want)} rows differ, first {bad[:1]}: {got[bad[:1]]} != {want[bad[:1]]}"


def _check(dev, verts, faces, what, factors=(0.5, -0.53)):
    """The lists, one step per factor and the normals on (verts, faces) == the reference, bit for bit.  -> the device
    tensors (verts, faces, order, start)."""
    from clm_gs_amd import clm_kernels
    v, f = _dev(dev, verts, faces)
    order, start = clm_kernels.mesh_incidence(f, len(verts))
    worder, wstart = S.incidence(faces, len(verts))
    assert order.dtype == torch.int64 and start.dtype == torch.int64 and order.is_contiguous() and start.is_contiguous()
    assert np.array_equal(order.cpu().numpy(), worder) and np.array_equal(start.cpu().numpy(), wstart), what
    for c in factors:
        out = clm_kernels.mesh_smooth_step(v, f, order, start, c)
        assert out.data_ptr() != v.data_ptr() and out.is_contiguous() and out.is_cuda
        _same(out, S.smooth_step(verts, faces, c, (worder, wstart)), f"{what}, step {c}")
    _same(v, np.ascontiguousarray(verts, dtype=np.float32), what + ", the input is not written")
    _same(clm_kernels.mesh_vertex_normals(v, f, order, start), S.vertex_normals(verts, faces, (worder, wstart)), what + ", normals")
    return v, f, order, start


def _extract(dev, sdf):
    from clm_gs_amd import clm_kernels
    return tuple(t.cpu().numpy() for t in clm_kernels.tsdf_extract(torch.from_numpy(R.grid_from_sdf(sdf)).to(dev), 2.0, R.G2W))


# ------------------------------------------------------------------------------------------------ 1. analytic grids
@pytest.mark.parametrize("name", ["sphere", "torus", "box", "two_spheres"])
def test_analytic_grids_through_the_extraction(dev, name):
    from clm_gs_amd import mesh_smooth
    x, y, z = R.centres()
    ball = lambda c, r: np.sqrt((x - c) ** 2 + (y - c) ** 2 + (z - c) ** 2) - r
    sdf = dict(sphere=R.sphere_sdf, torus=R.torus_sdf, box=box_sdf,
               two_spheres=lambda: np.minimum(ball(-0.3, 0.7), ball(0.8, 0.25)))[name]()
    verts, colours, faces = _extract(dev, sdf)
    assert (len(verts), len(faces)) == dict(sphere=(746, 1488), torus=(728, 1456), box=(602, 1200), two_spheres=(658, 1308))[name]
    verts = (verts.astype(np.float64) + np.random.default_rng(7).normal(0.0, 0.02, size=verts.shape)).astype(np.float32)
    v, f, order, start = _check(dev, verts, faces, name)
    c = torch.from_numpy(colours).to(dev)
    sv, sc, sf, rep = mesh_smooth.smooth(v, c, f, 3)
    wv, _, _, wrep = S.smooth(verts, colours, faces, 3)
    assert sc is c and sf is f and sv.data_ptr() != v.data_ptr() and rep == wrep and tuple(rep) == S.REPORT_KEYS
    _same(sv, wv, name + ", smooth(N=3)")
    _same(v, verts, name + ", the input is not written")
    _same(mesh_smooth.vertex_normals(sv, f), S.vertex_normals(wv, faces), name + ", normals after smoothing")
    one = mesh_smooth.smooth(v, c, f, 1, 0.5, 0)  # one step in all: a single buffer
    _same(one[0], S.smooth(verts, colours, faces, 1, 0.5, 0)[0], name + ", one plain step")
    assert one[3]["mu"] == 0.0 and one[3]["iterations"] == 1


# ------------------------------------------------------------------------------------------------ 2. segment lengths
def _fans(sizes, seed):
    """A fan of n faces around a hub for every n of sizes: the hub's segment has exactly n entries."""
    rng = np.random.default_rng(seed)
    verts, faces = [], []
    for k, n in enumerate(sizes):
        base = len(verts)
        verts.append([10.0 * k + 0.5, 0.5, 0.5])
        for i in range(n + 1):
            verts.append([10.0 * k + 1.5 + rng.random() * 0.9, i + 0.05 + rng.random() * 0.9, 0.05 + rng.random() * 0.9])
        faces += [(base, base + 1 + i, base + 2 + i) for i in range(n)]
    return np.array(verts, dtype=np.float32), np.array(faces, dtype=np.int32)


def test_segment_lengths_of_the_lane_loop(dev):
    sizes = [1, 2, 63, 64, 65, 255, 256, 257]
    verts, faces = _fans(sizes, 46)
    assert len(verts) % 256 != 0 and len(verts) > 256  # more than one workgroup, the last one partly filled
    interleaved = np.stack([faces[sum(sizes[:k]) + i] for i in range(max(sizes)) for k in range(len(sizes)) if i < sizes[k]])
    for what, f in (("contiguous", faces), ("interleaved", interleaved)):
        v, fd, order, start = _check(dev, verts, f, "fans, " + what)
        seg = (start[1:] - start[:-1]).cpu().numpy()
        hubs = np.cumsum([0] + [n + 2 for n in sizes[:-1]])
        assert seg[hubs].tolist() == sizes


def test_one_vertex_and_sizes_around_the_block(dev):
    _check(dev, np.array([[1.5, -2.5, 3.25]], dtype=np.float32), np.array([[0, 0, 0]], dtype=np.int32), "V = 1")
    rng = np.random.default_rng(47)
    for V in (2, 255, 256, 257, 513):
        verts = rng.random((V, 3)).astype(np.float32)
        faces = rng.integers(0, V, size=(2 * V, 3)).astype(np.int32)
        _check(dev, verts, faces, f"V = {V}", factors=(0.5,))


# ------------------------------------------------------------------------------------------------ 3. random triples
def _random_mesh():
    rng = np.random.default_rng(45)
    V, F = 20000, 15000
    verts = (rng.random((V, 3)) * 6.0 - 3.0).astype(np.float32)
    faces = rng.integers(0, V, size=(F, 3)).astype(np.int32)
    faces[::50, 1] = faces[::50, 0]             # degenerate faces: a == b, and a == b == c
    faces[::250, 2] = faces[::250, 0]
    return verts, faces


def test_random_triples_shuffled_faces_and_a_second_run(dev):
    from clm_gs_amd import clm_kernels
    verts, faces = _random_mesh()
    assert len(np.unique(faces)) < len(verts)  # unreferenced vertices
    v, f, order, start = _check(dev, verts, faces, "random")
    shuffled = faces[np.random.default_rng(44).permutation(len(faces))]
    sv, sf, sorder, sstart = _check(dev, verts, shuffled, "random, shuffled")
    for c in (0.5, -0.53):
        a, b = (clm_kernels.mesh_smooth_step(sv, sf, sorder, sstart, c) for _ in range(2))
        assert torch.equal(a, b)
    a, b = (clm_kernels.mesh_vertex_normals(sv, sf, sorder, sstart) for _ in range(2))
    assert torch.equal(a, b)
    free = np.setdiff1d(np.arange(len(verts)), faces)
    out = clm_kernels.mesh_smooth_step(v, f, order, start, 0.5).cpu().numpy()
    assert out[free].tobytes() == verts[free].tobytes()
    assert not clm_kernels.mesh_vertex_normals(v, f, order, start).cpu().numpy()[free].any()


# ------------------------------------------------------------------------------------------------ 4. empties
def test_empty_inputs(dev):
    from clm_gs_amd import clm_kernels, mesh_smooth
    verts = torch.rand((5, 3), device=dev)
    colours = torch.zeros((5, 3), dtype=torch.uint8, device=dev)
    none = torch.empty((0, 3), dtype=torch.int32, device=dev)
    for vv, cc in ((verts, colours), (verts[:0], colours[:0])):
        V = int(vv.shape[0])
        order, start = clm_kernels.mesh_incidence(none, V)
        assert order.shape == (0,) and order.dtype == torch.int64 and start.tolist() == [0] * (V + 1) and start.dtype == torch.int64
        out = clm_kernels.mesh_smooth_step(vv, none, order, start, 0.5)
        assert torch.equal(out, vv) and (V == 0 or out.data_ptr() != vv.data_ptr())  # a copy
        n = clm_kernels.mesh_vertex_normals(vv, none, order, start)
        assert n.shape == (V, 3) and n.dtype == torch.float32 and not n.any()
        sv, sc, sf, rep = mesh_smooth.smooth(vv, cc, none, 2)
        assert torch.equal(sv, vv) and sc is cc and sf is none
        assert rep == S.smooth(vv.cpu().numpy(), cc.cpu().numpy(), none.cpu().numpy(), 2)[3] and rep["vertices_fixed"] == V
        assert mesh_smooth.vertex_normals(vv, none).shape == (V, 3)
    same = mesh_smooth.smooth(verts, colours, none, 0)
    assert same[0] is verts and same[1] is colours and same[2] is none and same[3] is None
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ 5. refusals
def test_refusals_come_before_any_launch(dev, monkeypatch):
    from clm_gs_amd import _lib, clm_kernels, mesh_smooth
    verts = torch.rand((5, 3), device=dev)
    colours = torch.zeros((5, 3), dtype=torch.uint8, device=dev)
    good = torch.tensor([[0, 1, 2], [2, 3, 4]], dtype=torch.int32, device=dev)
    order, start = clm_kernels.mesh_incidence(good, 5)
    wide = torch.zeros((5, 6), device=dev)
    launched = []

    class Counting:  # the library with the two entries counted: nothing below may reach them
        def __init__(self, lib):
            self._lib = lib

        def __getattr__(self, name):
            if name in ("clmgs_mesh_smooth_step", "clmgs_mesh_vertex_normals"):
                launched.append(name)
            return getattr(self._lib, name)

    real = _lib.lib()
    monkeypatch.setattr(_lib, "lib", lambda: Counting(real))
    cases = [((verts.cpu(), good, order, start), "verts must be a tensor on the device"),
             ((verts, good.cpu(), order, start), "faces must be a tensor on the device"),
             ((verts, good, order.cpu(), start), "order must be a tensor on the device"),
             ((verts, good, order, start.cpu()), "start must be a tensor on the device"),
             ((verts.double(), good, order, start), r"verts must be float32 \[N,3\]"),
             ((verts, good.long(), order, start), r"faces must be int32 \[F,3\]"),
             ((verts, good, order.int(), start), r"order must be int64 \[6\]"),
             ((verts, good, order, start.int()), r"start must be int64 \[6\]"),
             ((torch.zeros((5, 4), device=dev), good, order, start), r"verts must be float32 \[N,3\]"),
             ((verts, torch.zeros((2, 4), dtype=torch.int32, device=dev), order, start), r"faces must be int32 \[F,3\]"),
             ((verts, good, order[:5], start), r"order must be int64 \[6\]"),
             ((verts, good, torch.cat([order, order]), start), r"order must be int64 \[6\]"),
             ((verts, good, order, start[:5]), r"start must be int64 \[6\]"),
             ((verts[:4], good[:1], order[:3], start), r"start must be int64 \[5\]"),
             ((wide[:, ::2], good, order, start), "verts must be contiguous"),
             ((verts, torch.zeros((2, 6), dtype=torch.int32, device=dev)[:, ::2], order, start), "faces must be contiguous"),
             ((verts, good, torch.cat([order, order])[::2], start), "order must be contiguous"),
             ((verts, good, order, torch.cat([start, start])[::2]), "start must be contiguous"),
             ((verts, torch.tensor([[0, 1, 5]], dtype=torch.int32, device=dev), order[:3], start), r"outside \[0, 5\)"),
             ((verts, torch.tensor([[0, -1, 2]], dtype=torch.int32, device=dev), order[:3], start), r"outside \[0, 5\)")]
    for args, match in cases:
        with pytest.raises(_lib.ClmgsError, match=match):
            clm_kernels.mesh_smooth_step(*args, 0.5)
        with pytest.raises(_lib.ClmgsError, match=match):
            clm_kernels.mesh_vertex_normals(*args)
    for bad in (float("nan"), float("inf"), "0.5", None, True):
        with pytest.raises(ValueError, match="factor must be a finite number"):
            clm_kernels.mesh_smooth_step(verts, good, order, start, bad)
    for args, match in (((good.cpu(), 5), "faces must be a tensor on the device"), ((good.long(), 5), r"faces must be int32 \[F,3\]"),
                        ((good, 4), r"outside \[0, 4\)")):
        with pytest.raises(_lib.ClmgsError, match=match):
            clm_kernels.mesh_incidence(*args)
    for args, match in (((verts.cpu(), colours, good), "verts must be a tensor on the device"),
                        ((verts, colours.cpu(), good), "colours must be a tensor on the device"),
                        ((verts, colours, good.cpu()), "faces must be a tensor on the device"),
                        ((verts, colours[:4], good), r"colours must be uint8 \[5,3\]"),
                        ((verts, colours, good + 3), r"outside \[0, 5\)")):
        with pytest.raises(_lib.ClmgsError, match=match):
            mesh_smooth.smooth(*args, 2)
    with pytest.raises(_lib.ClmgsError, match="verts must be a tensor on the device"):
        mesh_smooth.vertex_normals(verts.cpu(), good)
    with pytest.raises(ValueError, match=r"lam must be a finite number in \(0, 1\]"):
        mesh_smooth.smooth(verts, colours, good, 2, 1.5)
    assert not launched
    out = clm_kernels.mesh_smooth_step(verts, good, order, start, 0.5)  # (the good input runs, through the counted entries)
    n = clm_kernels.mesh_vertex_normals(verts, good, order, start)
    assert launched == ["clmgs_mesh_smooth_step", "clmgs_mesh_vertex_normals"] and out.shape == n.shape == (5, 3)
    # the C entries themselves: an output that is an input, a null pointer, sizes out of range -- CLMGS_EINVAL, no launch
    p = lambda t, dt: _lib.dptr(t, dt)
    f32, i32, i64 = torch.float32, torch.int32, torch.int64
    for V, F, vin, vout in ((5, 2, verts, verts), (0, 2, verts, out), (5, 0, verts, out)):
        with pytest.raises(_lib.ClmgsError):
            _lib.check(real.clmgs_mesh_smooth_step(_lib.stream(), V, F, p(vin, f32), p(good, i32), p(order, i64), p(start, i64),
                                                   0.5, p(vout, f32)))
        with pytest.raises(_lib.ClmgsError):
            _lib.check(real.clmgs_mesh_vertex_normals(_lib.stream(), V, F, p(vin, f32), p(good, i32), p(order, i64),
                                                      p(start, i64), p(vout, f32)))
    with pytest.raises(_lib.ClmgsError):
        _lib.check(real.clmgs_mesh_smooth_step(_lib.stream(), 5, 2, p(verts, f32), p(good, i32), p(order, i64), p(start, i64),
                                               float("nan"), p(out, f32)))
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ 6. end to end
def test_export_with_and_without_smoothing_and_the_tool(dev, tmp_path, capsys, monkeypatch):
    from clm_gs_amd import io_ply, mesh_clean, mesh_model, tsdf, utils
    from clm_gs_amd.render_ortho import map_frame
    from tests import mesh_clean_reference as M
    from tests import mesh_decimate_reference as D
    from tests.test_gpu_mesh_clean import _shell_scene
    extracted = []
    extract = tsdf.TsdfVolume.extract

    def recording(self, *a, **kw):
        out = extract(self, *a, **kw)
        extracted.append(tuple(t.cpu().numpy() for t in out))
        return out

    monkeypatch.setattr(tsdf.TsdfVolume, "extract", recording)
    try:
        gaussians, cams, args = _shell_scene(tmp_path)
        kw = dict(frame=map_frame(), bounds=(-14.0,) * 3 + (14.0,) * 3, min_weight=1.0)
        plain, smooth, every = (str(tmp_path / d / "mesh.ply") for d in ("plain", "smooth", "every"))
        capsys.readouterr()
        meta0 = mesh_model.build_mesh(gaussians, cams, args, plain, 1.0, **kw)
        line0 = capsys.readouterr().out
        meta1 = mesh_model.build_mesh(gaussians, cams, args, smooth, 1.0, smooth_iterations=2, normals=True, **kw)
        line1 = capsys.readouterr().out
        meta2 = mesh_model.build_mesh(gaussians, cams, args, every, 1.0, smooth_iterations=2, normals=True, keep_components=1,
                                      decimate_cell=2.0, **kw)
        line2 = capsys.readouterr().out
    finally:
        utils.set_args(utils.default_args())
    # without the flags: the file of before -- what the extraction returned in the layout without normals -- and no word
    # of smoothing or normals anywhere
    v0, c0, f0, n0 = io_ply.load_mesh_ply(plain, with_normals=True)
    assert len(extracted) == 3 and all(np.array_equal(a, b) for a, b in zip((v0, c0, f0), extracted[0])) and n0 is None
    before = str(tmp_path / "before.ply")
    io_ply.save_mesh_ply(before, *extracted[0])
    assert open(plain, "rb").read() == open(before, "rb").read()
    assert len(f0) > 0 and meta0 == json.load(open(plain[:-4] + ".json"))
    assert "smoothing" not in meta0 and "normals" not in meta0 and "smoothed" not in line0 and "normals" not in line0
    # with them: the reference applied to the first mesh
    wv, _, _, wrep = S.smooth(v0, c0, f0, 2)
    wn = S.vertex_normals(wv, f0)
    v1, c1, f1, n1 = io_ply.load_mesh_ply(smooth, with_normals=True)
    print(line1.strip(), "|", wrep)
    assert np.array_equal(v1, wv) and np.array_equal(c1, c0) and np.array_equal(f1, f0) and np.array_equal(n1, wn)
    assert not np.array_equal(v1, v0)
    assert meta1 == json.load(open(smooth[:-4] + ".json")) and meta1["smoothing"] == wrep and meta1["normals"] is True
    assert {k: v for k, v in meta1.items() if k not in ("smoothing", "normals")} == meta0
    assert " smoothed 2 x (0.5, -0.53) normals -> " in line1
    # everything: reference cleanup -> reference smoothing -> reference decimation -> reference normals
    kv, kc, kf, krep = M.clean(v0, c0, f0, keep_largest=1)
    sv, _, _, srep = S.smooth(kv, kc, kf, 2)
    dv, dc, df, drep = D.decimate(sv, kc, kf, 2.0)
    v2, c2, f2, n2 = io_ply.load_mesh_ply(every, with_normals=True)
    assert np.array_equal(v2, dv) and np.array_equal(c2, dc) and np.array_equal(f2, df)
    assert np.array_equal(n2, S.vertex_normals(dv, df))
    assert meta2["smoothing"] == srep and meta2["decimation"] == drep and meta2["cleanup"]["components_kept"] == 1
    assert meta2["normals"] is True and meta2["faces"] == len(f2) and meta2["vertices"] == len(v2)
    assert " components " in line2 and " decimated " in line2 and " smoothed 2 x (0.5, -0.53) normals -> " in line2
    # the tool on the first file writes the bytes of the second export, and of the third with the other options as well;
    # given a file WITH normals it ignores them: smoothing the smoothed file without --normals writes a file without
    for extra, want in (([], smooth), (["--keep_largest", "1", "--decimate_cell", "2.0"], every)):
        tool = str(tmp_path / ("tool%d" % len(extra)) / "out.ply")
        capsys.readouterr()
        assert mesh_clean.main(["-i", plain, "-o", tool, "--smooth_iterations", "2", "--normals"] + extra) == 0
        line = capsys.readouterr().out
        assert line.startswith("mesh cleanup:") and " smoothed 2 x (0.5, -0.53) normals in " in line, line
        assert open(tool, "rb").read() == open(want, "rb").read()
        assert json.load(open(tool[:-4] + ".json")) == json.load(open(want[:-4] + ".json"))
    again = str(tmp_path / "again" / "out.ply")
    assert mesh_clean.main(["-i", smooth, "-o", again, "--smooth_iterations", "1", "--smooth_mu", "0"]) == 0
    av, ac, af, an = io_ply.load_mesh_ply(again, with_normals=True)
    assert an is None and np.array_equal(av, S.smooth(v1, c1, f1, 1, 0.5, 0)[0]) and np.array_equal(af, f1)
    meta = json.load(open(again[:-4] + ".json"))
    assert "normals" not in meta and meta["smoothing"]["mu"] == 0.0 and meta["smoothing"]["iterations"] == 1


def test_trainer_smooths_and_writes_normals(dev, tmp_path):
    """trainer --mesh_voxel --mesh_smooth_iterations --mesh_normals, in the shape of test_gpu_mesh_decimate.test_trainer_decimates."""
    from clm_gs_amd import io_ply, trainer
    from tests.test_gpu_exposure import _tiny_scene
    work = _tiny_scene(tmp_path)
    out = tmp_path / "smooth"
    trainer.train_from_colmap(str(work), str(out), strategy="clm_offload", iterations=8, bsz=4,
                              disable_auto_densification=True, mesh_voxel=0.5, mesh_min_weight=1.0,
                              mesh_smooth_iterations=2, mesh_normals=True)
    verts, colours, faces, normals = io_ply.load_mesh_ply(str(out / "mesh.ply"), with_normals=True)
    assert len(io_ply.load_mesh_ply(str(out / "mesh.ply"))) == 3
    meta = json.load(open(out / "mesh.json"))
    log = open(out / "python_ws=1_rk=0.log").read()
    assert len(faces) > 0 and meta["faces"] == len(faces) and meta["vertices"] == len(verts)
    named = np.zeros(len(verts), dtype=bool)
    named[faces.reshape(-1)] = True
    assert meta["normals"] is True and meta["smoothing"] == dict(iterations=2, lam=0.5, mu=-0.53, vertices=len(verts),
                                                                faces=len(faces), vertices_fixed=int((~named).sum()))
    assert " smoothed 2 x (0.5, -0.53) normals" in log
    assert normals is not None and normals.shape == verts.shape and normals.dtype == np.float32
    length = np.linalg.norm(normals.astype(np.float64), axis=1)
    print("trainer mesh:", len(verts), "vertices", len(faces), "faces, |n| - 1 max", np.abs(length[named] - 1).max())
    assert np.abs(length[named] - 1).max() <= 1e-6 and not normals[~named].any()
    assert np.array_equal(normals, S.vertex_normals(verts, faces))
