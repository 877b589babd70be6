"""The trainer's three tables on the CPU: the command-line options (trainer.OPTIONS), the refusal pass
(trainer.check_training) and the side models (trainer.SIDE_MODELS)."""
import inspect
import json

import numpy as np
import pytest
import torch

from clm_gs_amd import dp, trainer, utils
from clm_gs_amd.cameras import Camera

REQUIRED = ["-s", "src", "-m", "out"]


def _other_than_default(kw, default):
    """The words that follow an option's name on a command line so that it parses to something else than `default`."""
    if kw.get("action") in ("store_true", "store_const"):
        return []
    if "choices" in kw:
        return [str(next(c for c in kw["choices"] if c != default))]
    typ = kw.get("type", str)
    if "nargs" in kw:
        n = kw["nargs"] if isinstance(kw["nargs"], int) else 2
        return [repr(typ(default[i]) + 1) if i < len(default or ()) else repr(typ(11 + i)) for i in range(n)]
    return ["other"] if typ is str else [repr(typ(default) + 1)]


def test_every_option_reaches_train_from_colmap_under_a_name_it_knows():
    ap = trainer.build_arg_parser()
    known = set(vars(utils.default_args())) | set(inspect.signature(trainer.train_from_colmap).parameters)
    assert set(trainer.train_kwargs(ap.parse_args(REQUIRED))) <= known
    for names, kw, dest, name, conv in trainer.OPTIONS:
        default = ap.get_default(dest)
        words = _other_than_default(kw, default)
        argv = [names[-1]] + words if kw.get("required") else REQUIRED + [names[-1]] + words
        if names[-1] == "--source_path":
            argv += ["-m", "out"]
        elif names[-1] == "--model_path":
            argv += ["-s", "src"]
        parsed = getattr(ap.parse_args(argv), dest)
        if kw.get("action") == "store_const":
            assert parsed == kw["const"], names
        else:
            assert parsed != default, names
        out = trainer.train_kwargs(ap.parse_args(argv))
        assert name in known, (names, name)
        assert out[name] == (conv(parsed) if conv else parsed), (names, name)
    # the renames, and the tuple of evaluation points
    base = trainer.train_kwargs(ap.parse_args(REQUIRED))
    assert (base["rasterize_mode"], base["defer_pose_step"], base["mcmc_cap_max"]) == ("classic", True, 1_000_000)
    assert base["strategy"] == "clm_offload" and base["test_iterations"] == (7000, 30000)
    out = trainer.train_kwargs(ap.parse_args(REQUIRED + ["--cap_max", "5", "--antialiased", "--immediate_pose_step",
                                                         "--test_iterations", "10", "20", "--naive_offload"]))
    assert (out["mcmc_cap_max"], out["rasterize_mode"], out["defer_pose_step"]) == (5, "antialiased", False)
    assert out["test_iterations"] == (10, 20) and out["strategy"] == "naive_offload"
    assert not {"cap_max", "antialiased", "immediate_pose_step"} & set(out)
    with pytest.raises(SystemExit):
        ap.parse_args(REQUIRED + ["--no_offload", "--naive_offload"])


class _Stub:
    """A model as training() is handed one: the pass only asks whether it is there."""


# (the rule, train_from_colmap's keyword arguments, the args of a direct training() call, the models handed to it, ranks)
REFUSALS = [
    ("absgrad + depths", dict(absgrad=True, depths="depths"), dict(absgrad=True), (), 1),
    ("exposure + bilagrid", dict(exposure=True, bilagrid=True), {}, ("exposure", "bilagrid"), 1),
    ("sky + white_background", dict(sky=True, white_background=True), dict(white_background=True), ("sky",), 1),
    ("sky + pose_opt", dict(sky=True, pose_opt=True), {}, ("sky", "pose"), 1),
    ("exposure under camera-DP", dict(exposure=True), {}, ("exposure",), 2),
    ("bilagrid under camera-DP", dict(bilagrid=True), {}, ("bilagrid",), 2),
    ("sky under camera-DP", dict(sky=True), {}, ("sky",), 2),
]


@pytest.mark.parametrize("rule,by_flag,direct_args,handed_in,ranks", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_both_entries_refuse_with_the_same_message(monkeypatch, tmp_path, rule, by_flag, direct_args, handed_in, ranks):
    monkeypatch.setattr(dp, "world_size", lambda: ranks)
    before = utils.ARGS
    with pytest.raises(ValueError) as by_name:  # before anything is loaded: the source directory does not even exist
        trainer.train_from_colmap(str(tmp_path / "no_such_scene"), str(tmp_path / "out"), **by_flag)
    assert not (tmp_path / "out").exists() and utils.ARGS is before
    args = utils.default_args(clm_offload=True, **direct_args)
    with pytest.raises(ValueError) as by_model:  # as training() calls the pass: the model is there, its flag is off
        trainer.check_training(args, depth_priors="depths" in by_flag, models={n: _Stub() for n in handed_in})
    assert str(by_name.value) == str(by_model.value)
    for word in rule.replace("under", "+").split(" + "):
        assert word.strip() in str(by_name.value), (rule, str(by_name.value))
    if ranks > 1:
        assert "camera-DP (world_size {})".format(ranks) in str(by_name.value)
    trainer.check_training(utils.default_args(clm_offload=True))  # nothing asked for, nothing refused


def _cameras(n):
    w2c = torch.eye(4)
    w2c[2, 3] = 4.0
    return [Camera(i, w2c.clone(), 1.0, 0.8, 16, 12, image_name=f"img_{i:03d}.png", device="cpu") for i in range(n)]


def test_side_model_table_builds_steps_and_saves(tmp_path):
    from clm_gs_amd.bilagrid import BilagridModel
    from clm_gs_amd.exposure import ExposureModel
    from clm_gs_amd.pose import PoseModel
    from clm_gs_amd.sky import SkyModel
    assert [(r.name, r.flag, r.file) for r in trainer.SIDE_MODELS] == [
        ("exposure", "exposure", "exposure.json"), ("bilagrid", "bilagrid", "bilagrid.npz"), ("sky", "sky", "sky.npz"),
        ("pose", "pose_opt", "poses.json")]
    assert all(r.flag in vars(utils.default_args()) for r in trainer.SIDE_MODELS)
    cams, other = _cameras(3), _cameras(1)
    models = {"exposure": trainer.build_exposure(cams, 100, device="cpu"),
              "bilagrid": trainer.build_bilagrid(cams, 100, device="cpu", grid=(3, 2, 2)),
              "sky": trainer.build_sky(cams, other, 100, device="cpu", shape=(4, 8)),
              "pose": trainer.build_pose(cams, 100, device=None, noise=0.01)}
    g = torch.Generator().manual_seed(3)
    for name in ("exposure", "bilagrid", "sky"):  # a table that is no longer the initial one
        with torch.no_grad():
            models[name].param += torch.rand(models[name].param.shape, generator=g) * 0.1
    for row in trainer.SIDE_MODELS:
        d = tmp_path / row.name
        d.mkdir()
        models[row.name].flush()
        models[row.name].save_to(str(d), cams)
        assert [p.name for p in d.iterdir()] == [row.file], row.name
    fresh = ExposureModel(3, "cpu")
    fresh.load_json(str(tmp_path / "exposure" / "exposure.json"), cams)
    assert torch.equal(fresh.param.detach(), models["exposure"].param.detach())
    fresh = BilagridModel(3, "cpu", grid=(3, 2, 2))
    fresh.load(str(tmp_path / "bilagrid" / "bilagrid.npz"), cams)
    assert torch.equal(fresh.param.detach(), models["bilagrid"].param.detach())
    fresh = SkyModel.from_file(str(tmp_path / "sky"), "cpu")
    assert torch.equal(fresh.param.detach(), models["sky"].param.detach())
    fresh = PoseModel(3, device=None)
    fresh.attach(_cameras(3))
    fresh.load_json(str(tmp_path / "pose" / "poses.json"), cams)
    assert torch.equal(fresh.table, models["pose"].table) and float(fresh.table.abs().max()) > 0
    assert sorted(json.load(open(tmp_path / "pose" / "poses.json"))) == [c.image_name for c in cams]
    assert sorted(np.load(tmp_path / "bilagrid" / "bilagrid.npz")["image_names"]) == [c.image_name for c in cams]
    # end_batch of a colour model = the trainer's former two calls: one step at the scheduled rate, then a zero gradient
    for name, twin in (("exposure", trainer.build_exposure(_cameras(3), 100, device="cpu")),
                       ("sky", trainer.build_sky(_cameras(3), [], 100, device="cpu", shape=(4, 8)))):
        model = models[name]
        with torch.no_grad():
            twin.param.copy_(model.param)
        grad = torch.rand(model.grad.shape, generator=g) - 0.5
        model.grad.copy_(grad)
        twin.grad.copy_(grad)
        start = model.param.detach().clone()
        model.end_batch(7, cams)
        twin.step(7)
        twin.zero_grad()
        assert not bool(model.grad.any()), name
        assert float((model.param.detach() - start).abs().max()) > 0, name
        assert torch.equal(model.param.detach(), twin.param.detach()), name
    # the pose model's end_batch is its step with the batch's cameras (host gradients here: the model has no device)
    pose = models["pose"]
    pose.defer = False
    table = pose.table.clone()
    pose._collect = lambda ids: (ids, torch.ones((len(ids), 16)), None)
    pose.end_batch(7, cams[:2])
    assert pose.t == 1 and not torch.equal(pose.table, table)
