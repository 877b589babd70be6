"""The median depth without a GPU: the float64 reference (tests/median_depth_reference.py) on hand-made pixels, its
exclusion cap on every case the GPU tests use, the render mode's name, and the refusals of the four command lines, which
fire before anything is loaded."""
import pytest
import torch

from tests import median_depth_reference as R


def _pixel(alphas, kinds=None, depths=None):
    """A 1x1 image whose one tile lists len(alphas) entries centred on the pixel: sigma = 0, so alpha = opacity.
    kinds[i]: "ok", "neg" (sigma < 0 at the pixel: a negative-definite conic, off centre) or "thin" (opacity below
    1/255).  -> (case, reference, (depth, id) maps under the threshold 0.5)."""
    K = len(alphas)
    kinds = kinds or ["ok"] * K
    m2 = torch.tensor([[0.5, 0.5] if k != "neg" else [1.5, 0.5] for k in kinds], dtype=torch.float32).reshape(1, K, 2)
    cn = torch.tensor([[1.0, 0.0, 1.0] if k != "neg" else [-1.0, 0.0, -1.0] for k in kinds], dtype=torch.float32).reshape(1, K, 3)
    op = torch.tensor([a if k != "thin" else 0.003 for a, k in zip(alphas, kinds)], dtype=torch.float32).reshape(1, K)
    case = dict(m2=m2, cn=cn, op=op, w=1, h=1, off=torch.zeros((1, 1, 1), dtype=torch.int32),
                fids=torch.arange(K, dtype=torch.int32))
    ref = R.case_median(case)
    depths = torch.tensor(depths if depths is not None else [float(i + 1) for i in range(K)]).reshape(1, K)
    return case, ref, R.reference_depth_and_id(ref, case, depths)


def test_hand_made_pixels():
    _, ref, (dep, ids) = _pixel([0.3, 0.6, 0.9])  # T before: 1, 0.7, 0.28 -> the crossing entry is 1
    assert int(ids[0, 0, 0]) == 1 and float(dep[0, 0, 0]) == 2.0
    assert int(ref["pos_hi"][0, 0, 0]) == int(ref["pos_lo"][0, 0, 0]) == 1 and bool(ref["has"][0, 0, 0])
    _, _, (dep, ids) = _pixel([0.6, 0.9])  # T before: 1, 0.4 -> entry 0
    assert int(ids[0, 0, 0]) == 0 and float(dep[0, 0, 0]) == 1.0
    _, _, (dep, ids) = _pixel([0.1, 0.1, 0.1, 0.1], depths=[4.0, 1.0, 3.0, 2.0])  # all translucent: the last contributor
    assert int(ids[0, 0, 0]) == 3 and float(dep[0, 0, 0]) == 2.0
    # the depth is that of the entry, whatever the order of the values: not a minimum, a maximum or a blend
    _, _, (dep, ids) = _pixel([0.3, 0.6, 0.9], depths=[5.0, 9.0, 1.0])
    assert int(ids[0, 0, 0]) == 1 and float(dep[0, 0, 0]) == 9.0


def test_an_empty_list_gives_depth_zero_and_id_minus_one():
    case = dict(m2=torch.zeros((1, 0, 2)), cn=torch.zeros((1, 0, 3)), op=torch.zeros((1, 0)), w=3, h=2,
                off=torch.zeros((1, 1, 1), dtype=torch.int32), fids=torch.zeros((0,), dtype=torch.int32))
    ref = R.case_median(case)
    dep, ids = R.reference_depth_and_id(ref, case, torch.zeros((1, 0)))
    assert not bool(ref["has"].any()) and bool((ids == -1).all()) and bool((dep == 0).all())
    assert bool((ref["pos_hi"] == -1).all()) and bool((ref["pos_lo"] == -1).all())
    # entries that are all skipped: the same
    _, ref, (dep, ids) = _pixel([0.9, 0.9], kinds=["neg", "thin"])
    assert not bool(ref["has"].any()) and int(ids[0, 0, 0]) == -1 and float(dep[0, 0, 0]) == 0.0


@pytest.mark.parametrize("kind", ["neg", "thin"])
def test_a_skipped_entry_is_never_the_median(kind):
    # the skipped entry stands where T would cross one half, and last in an open pixel
    _, _, (_, ids) = _pixel([0.3, 0.9, 0.6, 0.9], kinds=["ok", kind, "ok", "ok"])  # T before: 1, 0.7, (0.7), 0.28
    assert int(ids[0, 0, 0]) == 2
    _, _, (_, ids) = _pixel([0.2, 0.2, 0.9], kinds=["ok", "ok", kind])
    assert int(ids[0, 0, 0]) == 1
    _, _, (_, ids) = _pixel([0.9, 0.2], kinds=[kind, "ok"])
    assert int(ids[0, 0, 0]) == 1


def test_the_interval_brackets_a_near_tie():
    # T before entry 1 is 0.5 (1 + 1e-4): above one half, inside the band -> the kernel may answer 0 or 1
    _, ref, (_, ids) = _pixel([0.5 * (1 - 1e-4), 0.9, 0.9])
    assert int(ids[0, 0, 0]) == 1
    assert (int(ref["pos_hi"][0, 0, 0]), int(ref["pos_lo"][0, 0, 0])) == (0, 1) and ref["wide"] == 1
    assert not bool(ref["excluded"].any())
    # an alpha at 1/255 that is looked at excludes the pixel; behind the crossing it does not
    _, ref, _ = _pixel([1.0 / 255.0, 0.9])
    assert bool(ref["excluded"][0, 0, 0])
    _, ref, _ = _pixel([0.9, 1.0 / 255.0])
    assert not bool(ref["excluded"][0, 0, 0])


CAP_CASES = ["special"] + R.list_names() + ["list65_sat_middle"] + list(R.CPU_SHAPES)


@pytest.mark.parametrize("name", CAP_CASES)
def test_exclusion_cap(name):
    case, ref = R.cached(name)
    share = float(ref["excluded"].sum()) / ref["inside"]
    print(f"{name}: excluded {int(ref['excluded'].sum())} of {ref['inside']} pixels ({100 * share:.3f} %), "
          f"{ref['wide']} with more than one admissible entry, list entries up to the median {ref['visited']} of "
          f"{ref['listed']}")
    assert share <= R.EXCLUDED_CAP
    assert bool((ref["pos_hi"] <= ref["pos_lo"]).all()) and bool(((ref["pos_hi"] >= 0) == ref["has"]).all())
    # the reference checks itself: its own maps pass its own check, with depths not monotone in list order
    depths = R.case_depths(case, "permuted")
    dep, ids = R.reference_depth_and_id(ref, case, depths)
    res = R.check_maps(ref, case, depths, dep, ids)
    assert not any(v for k, v in res.items() if k.startswith("bad_")), res
    wrong = ids.clone()
    wrong[ref["has"]] = -1
    if bool(ref["has"].any()):
        assert R.check_maps(ref, case, depths, dep, wrong)["bad_none"] > 0


def test_list_order_rank_increases_along_every_list():
    for name in ("special", "tiles9_C3", "list129_sat"):
        case, _ = R.cached(name)
        d = R.case_depths(case, "increasing").reshape(-1)
        p = R.case_depths(case, "permuted").reshape(-1)
        offs = case["off"].flatten().tolist() + [int(case["fids"].shape[0])]
        monotone = True
        for s, e in zip(offs[:-1], offs[1:]):
            g = case["fids"][s:e].long()
            assert bool((d[g][1:] > d[g][:-1]).all())
            monotone &= bool((p[g][1:] > p[g][:-1]).all())
        assert not monotone


def test_render_mode_is_known():
    from clm_gs_amd.strategies import base_engine as B
    assert "RGB+MD" in B.RENDER_MODES
    col, bg = torch.rand(1, 5, 3), torch.rand(1, 3)
    c2, b2 = B.colors_with_depth(col, torch.rand(1, 5), bg, "RGB+MD")  # no fourth colour, the backgrounds as they are
    assert c2 is col and b2 is bg
    with pytest.raises(ValueError, match="RGB\\+MD"):
        B.refuse_median_training("RGB+MD", "training entry")
    B.refuse_median_training("RGB+ED", "training entry")


def test_command_lines_refuse_before_anything_is_loaded(tmp_path):
    from clm_gs_amd import mesh_model, render_ortho, render_trajectory, trainer, utils
    missing, out = str(tmp_path / "no_model"), tmp_path / "out"
    # mesh_model: an unknown mode, by check_options
    with pytest.raises(ValueError, match="--depth_mode"):
        mesh_model.check_options(0.1, depth_mode="mode7")
    mesh_model.check_options(0.1, depth_mode="median")
    with pytest.raises(SystemExit, match="--depth_mode"):
        mesh_model.main(["-m", missing, "-s", missing, "-o", str(out / "mesh.ply"), "--voxel", "0.1", "--depth_mode", "mode7"])
    # render_trajectory: without --render_depth, and an unknown mode with it
    with pytest.raises(SystemExit, match="--depth_mode median has effect only with --render_depth"):
        render_trajectory.main(["-m", missing, "--output_dir", str(out), "--depth_mode", "median"])
    with pytest.raises(SystemExit, match="--depth_mode"):
        render_trajectory.main(["-m", missing, "--output_dir", str(out), "--render_depth", "--depth_mode", "mode7"])
    render_trajectory.check_depth_options(True, "median")
    render_trajectory.check_depth_options(False, None)
    assert render_trajectory.depth_render_mode(None) == render_trajectory.depth_render_mode("expected") == "RGB+ED"
    assert render_trajectory.depth_render_mode("median") == "RGB+MD"
    # render_ortho
    with pytest.raises(SystemExit, match="--depth_mode"):
        render_ortho.main(["-m", missing, "--output_dir", str(out), "--gsd", "0.1", "--depth_mode", "mode7"])
    # trainer: the flag without --mesh_voxel, an unknown mode with it; both through check_training, before the scene loads
    assert trainer.mesh_rules(utils.default_args()) == []
    rules = trainer.mesh_rules(utils.default_args(mesh_depth_mode="median"))
    assert any(r and "--mesh_depth_mode median has effect only with --mesh_voxel" in m for r, m in rules)
    rules = trainer.mesh_rules(utils.default_args(mesh_voxel=0.1, mesh_depth_mode="mode7"))
    assert any(r and "--mesh_depth_mode must be one of" in m for r, m in rules)
    assert not any(r for r, _ in trainer.mesh_rules(utils.default_args(mesh_voxel=0.1, mesh_depth_mode="median")))
    with pytest.raises(ValueError, match="--mesh_depth_mode"):
        trainer.main(["-s", missing, "-m", str(out), "--mesh_depth_mode", "median"])
    ns = trainer.build_arg_parser().parse_args(["-s", "a", "-m", "b", "--mesh_voxel", "0.25", "--mesh_depth_mode", "median"])
    assert trainer.train_kwargs(ns)["mesh_depth_mode"] == "median"
    assert trainer.train_kwargs(trainer.build_arg_parser().parse_args(["-s", "a", "-m", "b"]))["mesh_depth_mode"] is None
    assert not out.exists()
    utils.set_args(utils.default_args())
