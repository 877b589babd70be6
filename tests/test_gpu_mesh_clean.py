"""Mesh cleanup on the device ("Mesh cleanup"): csrc/mesh.hip through clm_kernels.mesh_components /
mesh_component_faces, mesh_clean.clean, the mesh export, the clean_mesh tool and the trainer, against the numpy restatement
(tests/mesh_clean_reference.py).  Every comparison is exact: integer labels, counts and indices, torch.equal /
array_equal on floats that are only copied."""
import json
import math
import os

import numpy as np
import pytest
import torch

from tests import mesh_clean_reference as M
from tests import tsdf_reference as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(dev, faces, V):
    """-> (labels, counts, rounds) of the kernels as numpy / int."""
    from clm_gs_amd import clm_kernels
    f = torch.from_numpy(np.ascontiguousarray(faces, dtype=np.int32).reshape(-1, 3)).to(dev)
    labels, rounds = clm_kernels.mesh_components(f, V)
    counts = clm_kernels.mesh_component_faces(f, labels)
    assert labels.dtype == torch.int32 and counts.dtype == torch.int32 and labels.shape == counts.shape == (V,)
    assert isinstance(rounds, int) and rounds <= clm_kernels.MESH_MAX_ROUNDS
    return labels.cpu().numpy(), counts.cpu().numpy(), rounds


def _check(dev, faces, V, what):
    lab, cnt, rounds = _run(dev, faces, V)
    want = M.labels(faces, V)
    print(f"{what}: V {V} F {len(faces)} rounds {rounds} components {int((M.sizes(faces, want) > 0).sum())}")
    assert np.array_equal(lab, want), what
    assert np.array_equal(cnt, M.sizes(faces, want)), what
    return lab, cnt, rounds


# ------------------------------------------------------------------------------------------------ 1. strip
@pytest.mark.parametrize("numbering", ["identity", "reversed", "random"])
def test_strip(dev, numbering):
    """4096 triangles in a strip, one component of diameter 2049: a form that only passes labels to neighbours needs
    thousands of rounds and fails the cap."""
    from clm_gs_amd import clm_kernels
    n, V = 4096, 4098
    i = np.arange(n)
    perm = {"identity": np.arange(V), "reversed": np.arange(V)[::-1], "random": np.random.default_rng(41).permutation(V)}[numbering]
    faces = perm[np.stack([i, i + 1, i + 2], 1)].astype(np.int32)
    lab, cnt, rounds = _run(dev, faces, V)
    print(f"strip/{numbering}: rounds {rounds}")
    assert rounds <= clm_kernels.MESH_MAX_ROUNDS, f"strip/{numbering}: {rounds} rounds"
    assert (lab == 0).all(), f"strip/{numbering}: {int((lab != 0).sum())} labels are not 0 after {rounds} rounds"
    assert int(cnt[0]) == n and int(cnt.sum()) == n


# ------------------------------------------------------------------------------------------------ 2. disjoint triangles
def test_disjoint_triangles_and_unreferenced_vertices(dev):
    T, extra = 1000, 37
    V = 3 * T + extra
    perm = np.random.default_rng(42).permutation(V)
    faces = perm[np.arange(3 * T).reshape(T, 3)].astype(np.int32)
    lab, cnt, rounds = _check(dev, faces, V, "disjoint")
    assert int((cnt > 0).sum()) == T and set(cnt[cnt > 0].tolist()) == {1}
    assert np.array_equal(lab[faces[:, 0]], faces.min(axis=1))
    free = perm[3 * T:]
    assert np.array_equal(lab[free], free) and (cnt[free] == 0).all()


# ------------------------------------------------------------------------------------------------ 3. hub
def test_hub(dev):
    """5000 triangles that all share vertex V - 1: every face adds to one count, the minimum is elsewhere."""
    T = 5000
    V = 2 * T + 1
    i = np.arange(T)
    faces = np.stack([np.full(T, V - 1), 2 * i, 2 * i + 1], 1).astype(np.int32)
    lab, cnt, rounds = _check(dev, faces, V, "hub")
    assert (lab == 0).all() and int(cnt[0]) == T and int(np.count_nonzero(cnt)) == 1


# ------------------------------------------------------------------------------------------------ 4. random
def test_random_triples_any_face_order_and_again(dev):
    rng = np.random.default_rng(43)
    V, F = 20000, 15000
    faces = rng.integers(0, V, size=(F, 3)).astype(np.int32)
    faces[::50, 1] = faces[::50, 0]             # degenerate faces: a == b, and a == b == c
    faces[::250, 2] = faces[::250, 0]
    lab, cnt, rounds = _check(dev, faces, V, "random")
    assert 1 < int((cnt > 0).sum()) < F and int(cnt.max()) > 1
    shuffled = faces[rng.permutation(F)]
    lab2, cnt2, _ = _check(dev, shuffled, V, "random, shuffled")
    lab3, cnt3, _ = _run(dev, faces, V)
    assert np.array_equal(lab2, lab) and np.array_equal(lab3, lab) and np.array_equal(cnt3, cnt)
    # the size of a component is counted at the first vertex of its faces: a shuffle moves no face to another component
    assert np.array_equal(cnt2, cnt)


# ------------------------------------------------------------------------------------------------ 5. run boundaries
def test_run_boundaries_of_the_size_kernel(dev):
    sizes = [63, 64, 65, 255, 256, 257]
    faces, base, starts = [], 0, []
    for n in sizes:                             # fans: island k has sizes[k] + 2 vertices of its own
        starts.append(base)
        faces.append(np.array([(base, base + i + 1, base + i + 2) for i in range(n)], dtype=np.int32))
        base += n + 2
    V = base
    contiguous = np.concatenate(faces)
    longest = max(sizes)
    interleaved = np.stack([f[i] for i in range(longest) for f in faces if i < len(f)])  # round robin over the islands
    assert len(interleaved) == len(contiguous) == sum(sizes)
    for what, f in (("contiguous", contiguous), ("interleaved", interleaved)):
        lab, cnt, rounds = _check(dev, f, V, "runs, " + what)
        assert cnt[starts].tolist() == sizes and int(np.count_nonzero(cnt)) == len(sizes)


# ------------------------------------------------------------------------------------------------ 6. empty inputs
def test_empty_inputs(dev):
    from clm_gs_amd import clm_kernels, mesh_clean
    none = torch.empty((0, 3), dtype=torch.int32, device=dev)
    labels, rounds = clm_kernels.mesh_components(none, 5)
    assert labels.tolist() == [0, 1, 2, 3, 4] and labels.dtype == torch.int32 and rounds == 0
    assert clm_kernels.mesh_component_faces(none, labels).tolist() == [0] * 5
    labels, rounds = clm_kernels.mesh_components(none, 0)
    assert labels.shape == (0,) and labels.dtype == torch.int32 and rounds == 0
    assert clm_kernels.mesh_component_faces(none, labels).shape == (0,)
    verts, colours = torch.zeros((5, 3), device=dev), torch.zeros((5, 3), dtype=torch.uint8, device=dev)
    v, c, f, rep = mesh_clean.clean(verts, colours, none, min_faces=1)
    assert v.shape == (0, 3) and c.shape == (0, 3) and f.shape == (0, 3)
    assert rep == dict(components=0, components_kept=0, vertices_removed=5, faces_removed=0, largest_faces=0, rounds=0)
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ 7. two spheres
def test_two_spheres_through_the_extraction(dev):
    from clm_gs_amd import clm_kernels, mesh_clean
    x, y, z = R.centres()
    ball = lambda c, r: np.sqrt((x - c) ** 2 + (y - c) ** 2 + (z - c) ** 2) - r
    grid = R.grid_from_sdf(np.minimum(ball(-0.3, 0.7), ball(0.8, 0.25)))
    verts, colours, faces = clm_kernels.tsdf_extract(torch.from_numpy(grid).to(dev), 2.0, R.G2W)
    assert verts.shape == (658, 3) and faces.shape == (1308, 3)
    hv, hc, hf = verts.cpu().numpy(), colours.cpu().numpy(), faces.cpu().numpy()
    lab, cnt, rounds = _check(dev, hf, 658, "two spheres")
    assert np.nonzero(cnt)[0].tolist() == [0, 590] and cnt[[0, 590]].tolist() == [1176, 132]
    for kw in (dict(min_faces=133), dict(keep_largest=1)):
        v, c, f, rep = mesh_clean.clean(verts, colours, faces, **kw)
        assert v.dtype == torch.float32 and c.dtype == torch.uint8 and f.dtype == torch.int32
        assert v.is_contiguous() and c.is_contiguous() and f.is_contiguous()
        wv, wc, wf, wrep = M.clean(hv, hc, hf, **kw)
        assert np.array_equal(v.cpu().numpy(), wv) and np.array_equal(c.cpu().numpy(), wc) and np.array_equal(f.cpu().numpy(), wf)
        assert rep == dict(wrep, rounds=rounds), (rep, wrep)
        t = R.topology(v.cpu().numpy(), f.cpu().numpy())
        assert (t["V"], t["F"], t["euler"], t["closed"], t["oriented"]) == (590, 1176, 2, True, True), t
    v, c, f, rep = mesh_clean.clean(verts, colours, faces, min_faces=1)
    assert torch.equal(v, verts) and torch.equal(c, colours) and torch.equal(f, faces)
    assert rep["components"] == rep["components_kept"] == 2 and rep["vertices_removed"] == rep["faces_removed"] == 0
    same = mesh_clean.clean(verts, colours, faces)  # both off: the inputs themselves
    assert same[0] is verts and same[1] is colours and same[2] is faces and same[3] is None


# ------------------------------------------------------------------------------------------------ 8. refusals
def test_refusals_come_before_any_launch(dev):
    from clm_gs_amd import _lib, clm_kernels, mesh_clean
    good = torch.tensor([[0, 1, 2], [2, 3, 4]], dtype=torch.int32, device=dev)
    labels = torch.arange(5, dtype=torch.int32, device=dev)
    wide = torch.zeros((2, 6), dtype=torch.int32, device=dev)
    cases = [(good.cpu(), 5, "device"), (good.long(), 5, r"int32 \[F,3\]"), (wide[:, ::2], 5, "contiguous"),
             (torch.zeros((2, 4), dtype=torch.int32, device=dev), 5, r"int32 \[F,3\]"),
             (torch.tensor([[0, 1, 5]], dtype=torch.int32, device=dev), 5, r"outside \[0, 5\)"),
             (torch.tensor([[0, -1, 2]], dtype=torch.int32, device=dev), 5, r"outside \[0, 5\)"),
             (good, 0, r"outside \[0, 0\)")]
    for faces, V, match in cases:
        with pytest.raises(_lib.ClmgsError, match=match):
            clm_kernels.mesh_components(faces, V)
        if V == 5:
            with pytest.raises(_lib.ClmgsError, match=match):
                clm_kernels.mesh_component_faces(faces, labels)
    with pytest.raises(ValueError, match="V must be in"):
        clm_kernels.mesh_components(good, -1)
    with pytest.raises(_lib.ClmgsError, match="labels"):
        clm_kernels.mesh_component_faces(good, labels.long())
    with pytest.raises(_lib.ClmgsError, match="labels"):
        clm_kernels.mesh_component_faces(good, labels.cpu())
    verts, colours = torch.zeros((5, 3), device=dev), torch.zeros((5, 3), dtype=torch.uint8, device=dev)
    with pytest.raises(ValueError, match="min_faces must be a non-negative integer"):
        mesh_clean.clean(verts, colours, good, min_faces=-1)
    with pytest.raises(ValueError, match="keep_largest must be a non-negative integer"):
        mesh_clean.clean(verts, colours, good, keep_largest=-1)
    with pytest.raises(_lib.ClmgsError, match=r"outside \[0, 4\)"):
        mesh_clean.clean(verts[:4], colours[:4], good, min_faces=1)
    lab, rounds = clm_kernels.mesh_components(good, 5)  # (the good input runs)
    assert lab.tolist() == [0] * 5 and clm_kernels.mesh_component_faces(good, lab).tolist() == [2, 0, 0, 0, 0]


# ------------------------------------------------------------------------------------------------ 9. end to end
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


def _shell_scene(tmp_path):
    """The shell as a model and the cameras of tests/golden/colmap_tiny, set up as mesh_model.main does."""
    from clm_gs_amd import io_ply, utils
    from clm_gs_amd.colmap_scene import load_colmap_scene
    from clm_gs_amd.strategies.no_offload import GaussianModelNoOffload
    rows = _shell_rows()
    ply = str(tmp_path / "shell.ply")
    io_ply.save_ply(ply, rows["xyz"], rows["shs48"], rows["opacity"], rows["scaling"], rows["rotation"])
    args = utils.default_args(bsz=4, no_offload=True)
    utils.set_args(args)
    scene = load_colmap_scene(os.path.join(ROOT, "tests", "golden", "colmap_tiny"), device="cuda", load_images=False)
    cams = scene.train_cameras
    utils.set_img_size(cams[0].image_height, cams[0].image_width)
    gaussians = GaussianModelNoOffload(3, only_for_rendering=True)
    gaussians.load_ply(ply)
    gaussians.active_sh_degree = gaussians.max_sh_degree
    return gaussians, cams, args


def test_export_with_and_without_the_filter_and_the_tool(dev, tmp_path, capsys, monkeypatch):
    from clm_gs_amd import io_ply, mesh_clean, mesh_model, tsdf, utils
    from clm_gs_amd.render_ortho import map_frame
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
        plain, kept = str(tmp_path / "plain" / "mesh.ply"), str(tmp_path / "kept" / "mesh.ply")
        capsys.readouterr()
        meta0 = mesh_model.build_mesh(gaussians, cams, args, plain, 1.0, **kw)
        line0 = capsys.readouterr().out
        meta1 = mesh_model.build_mesh(gaussians, cams, args, kept, 1.0, keep_components=1, **kw)
        line1 = capsys.readouterr().out
    finally:
        utils.set_args(utils.default_args())
    # without the filter: what the extraction returned, a .json and a log line without a word of the cleanup
    v0, c0, f0 = io_ply.load_mesh_ply(plain)
    assert len(extracted) == 2 and all(np.array_equal(a, b) for a, b in zip((v0, c0, f0), extracted[0]))
    assert len(f0) > 0 and meta0 == json.load(open(plain[:-4] + ".json"))
    assert "cleanup" not in meta0 and "components" not in line0 and meta0["faces"] == len(f0)
    # with it: the numpy reference applied to the first mesh
    wv, wc, wf, wrep = M.clean(v0, c0, f0, keep_largest=1)
    v1, c1, f1 = io_ply.load_mesh_ply(kept)
    print(line1.strip(), "|", wrep)
    assert np.array_equal(v1, wv) and np.array_equal(c1, wc) and np.array_equal(f1, wf)
    meta1 = json.load(open(kept[:-4] + ".json"))
    clean = meta1.pop("cleanup")
    rounds = clean.pop("rounds")
    assert clean == dict(wrep, min_faces=0, keep_largest=1) and 1 <= rounds <= 64
    assert clean["components_kept"] == 1 and clean["largest_faces"] == len(f1) == meta1["faces"] and meta1["vertices"] == len(v1)
    assert meta1["vertices"] + clean["vertices_removed"] == meta0["vertices"]
    assert meta1["faces"] + clean["faces_removed"] == meta0["faces"]
    assert {k: v for k, v in meta1.items() if k not in ("vertices", "faces")} == \
           {k: v for k, v in meta0.items() if k not in ("vertices", "faces")}
    assert " components {} kept 1 -> ".format(clean["components"]) in line1
    assert int((M.sizes(f1, M.labels(f1, len(v1))) > 0).sum()) == 1
    # the tool on the first file writes the bytes of the second export
    tool = str(tmp_path / "tool" / "clean.ply")
    capsys.readouterr()
    assert mesh_clean.main(["-i", plain, "-o", tool, "--keep_largest", "1"]) == 0
    line = capsys.readouterr().out
    assert line.startswith("mesh cleanup: components {} kept 1 ".format(clean["components"])) and "rounds" in line, line
    assert open(tool, "rb").read() == open(kept, "rb").read()
    meta2 = json.load(open(tool[:-4] + ".json"))
    assert meta2 == json.load(open(kept[:-4] + ".json"))


def test_trainer_keeps_one_component(dev, tmp_path):
    """trainer --mesh_voxel --mesh_keep_components 1, in the shape of test_gpu_tsdf.test_trainer_mesh_voxel."""
    from clm_gs_amd import io_ply, trainer
    from tests.test_gpu_exposure import _tiny_scene
    work, out = _tiny_scene(tmp_path), tmp_path / "out"
    trainer.train_from_colmap(str(work), str(out), strategy="clm_offload", iterations=8, bsz=4,
                              disable_auto_densification=True, mesh_voxel=0.5, mesh_min_weight=1.0, mesh_keep_components=1)
    verts, colours, faces = io_ply.load_mesh_ply(str(out / "mesh.ply"))
    meta = json.load(open(out / "mesh.json"))
    count = M.sizes(faces, M.labels(faces, len(verts)))
    print("trainer mesh:", meta["vertices"], meta["faces"], meta["cleanup"])
    assert int((count > 0).sum()) == 1 and int(count.max()) == len(faces) == meta["faces"]
    assert meta["cleanup"]["components_kept"] == 1 and meta["cleanup"]["keep_largest"] == 1
    assert meta["cleanup"]["components"] >= 1 and meta["vertices"] == len(verts) == len(np.unique(faces))
    log = open(out / "python_ws=1_rk=0.log").read()
    assert " components {} kept 1".format(meta["cleanup"]["components"]) in log
