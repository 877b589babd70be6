"""CPU-only checks of the camera pose refinement: the host model (clm_gs_amd/pose.py) against the float64 reference of
tests/pose_reference.py, the refusals, the new arguments, the ABI table, and the host build of csrc/pose_math.h against
central differences (tests/host_shim/pose_math_host.cpp)."""
import json
import math
import os
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from clm_gs_amd import pose as P  # noqa: E402
from clm_gs_amd import utils  # noqa: E402
from clm_gs_amd.cameras import Camera, camera_pose_grad  # noqa: E402
from tests import pose_reference as R  # noqa: E402

F64 = torch.float64


def _cameras(n=6, seed=0):
    g = torch.Generator().manual_seed(seed)
    cams = []
    for i in range(n):
        q = torch.randn(4, generator=g, dtype=F64)
        q = q / q.norm()
        w, x, y, z = q.tolist()
        Rm = torch.tensor([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                           [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                           [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]], dtype=F64)
        w2c = torch.eye(4, dtype=F64)
        w2c[:3, :3] = Rm
        w2c[:3, 3] = torch.randn(3, generator=g, dtype=F64) * 2
        cams.append(Camera(i, w2c.float(), 1.0, 0.8, 64, 48, device="cpu"))
    return cams


def _model(cams, **kw):
    m = P.PoseModel(len(cams), device=None, **kw)
    m.attach(cams)
    return m


def _fields(c):
    return (c.world_view_transform.clone(), c.camtoworlds.clone(), tuple(a.copy() for a in c._clmgs_host))


def test_zero_table_is_the_identity_bit_for_bit():
    cams = _cameras()
    before = [_fields(c) for c in cams]
    m = _model(cams)
    assert m.refresh() == 0
    m.apply([], torch.zeros(0, 15))  # a step without any gradient: zero rows stay zero (no moments, decay of zero)
    assert torch.equal(m.table, torch.zeros(len(cams), 9, dtype=F64))
    for c, (wvt, c2w, host) in zip(cams, before):
        assert torch.equal(c.world_view_transform, wvt) and torch.equal(c.camtoworlds, c2w)
        for a, b in zip(c._clmgs_host, host):
            assert a.dtype == b.dtype and a.tobytes() == b.tobytes()
    # and the composition itself: rot6d of the identity offset is the identity matrix exactly
    assert torch.equal(P.rot6d_to_matrix(torch.tensor(P._I6, dtype=F64)), torch.eye(3, dtype=F64))
    assert camera_pose_grad(cams[0]) is None  # no device: no buffer


def test_composed_gradient_equals_autograd_of_the_reference_chain():
    cams = _cameras()
    m = _model(cams)
    g = torch.Generator().manual_seed(3)
    m.table += torch.randn(m.table.shape, generator=g, dtype=F64) * 0.05
    ids = [4, 1, 2]
    g15 = torch.randn(len(ids), 15, generator=g, dtype=F64)
    got = m.compose_grad(ids, g15)
    for j, i in enumerate(ids):
        vv = torch.cat((g15[j, :9].reshape(3, 3), g15[j, 9:12].reshape(3, 1)), dim=1)
        ref = R.row_gradient(m.c2w0[i], m.table[i], vv, g15[j, 12:15])
        assert float((got[j] - ref).abs().max()) <= 1e-10 * max(1.0, float(ref.abs().max())), (i, got[j], ref)
    # the composition against the reference's, too
    for i in range(len(cams)):
        assert float((m.camtoworlds()[i] - R.camtoworld(m.c2w0[i], m.table[i])).abs().max()) < 1e-13


def _feed(n_cams, batches, seed=5):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(len(b), 15, generator=g, dtype=F64) for b in batches]


def test_ten_steps_equal_the_reference_optimiser():
    cams = _cameras()
    m = _model(cams, lr=1e-3, reg=1e-2, max_steps=10, defer=False)
    m.perturb(0.02, seed=1)
    ref = R.Adam(m.table, 1e-3, 1e-2, 10)
    batches = [[(2 * k) % 6, (2 * k + 1) % 6] for k in range(10)]
    for ids, g15 in zip(batches, _feed(6, batches)):
        grad = torch.zeros(6, 9, dtype=F64)
        for j, i in enumerate(ids):
            vv = torch.cat((g15[j, :9].reshape(3, 3), g15[j, 9:12].reshape(3, 1)), dim=1)
            grad[i] += R.row_gradient(m.c2w0[i], ref.p[i], vv, g15[j, 12:15])
        ref.step(grad)
        m.step([cams[i] for i in ids], g15)
        assert float((m.table - ref.p).abs().max()) < 1e-12
    assert m.t == 10 and abs(m.learning_rate(10) - 1e-5) < 1e-18 and abs(R.schedule(1e-3, 10, 10) - 1e-5) < 1e-18


def test_deferred_and_immediate_stepping_give_the_same_table():
    batches = [[0, 1], [2, 3], [4, 5], [1, 0], [3, 5], [2, 4]]  # no camera in two consecutive batches
    feed = _feed(6, batches)
    tables = []
    for defer in (False, True):
        cams = _cameras()
        m = _model(cams, lr=1e-3, defer=defer)
        for k, (ids, g15) in enumerate(zip(batches, feed)):
            m.step([cams[i] for i in ids], g15)
            if defer:  # one step behind until flushed
                assert m.t == k
        m.flush()
        assert m.t == len(batches)
        tables.append(m.table.clone())
    assert torch.equal(tables[0], tables[1])


def test_camera_fields_agree_after_a_step():
    cams = _cameras()
    m = _model(cams, lr=1e-2, defer=False)
    untouched = _fields(cams[5])
    m.step([cams[0], cams[3]], _feed(6, [[0, 3]])[0])
    assert torch.equal(cams[5].world_view_transform, untouched[0])  # a row that has not moved is not rewritten
    c2w64 = m.camtoworlds()
    for i in (0, 3):
        c = cams[i]
        vm, K, cp = c._clmgs_host
        assert vm.dtype == np.float32 and vm.shape == (16,) and cp.shape == (3,) and vm.flags["C_CONTIGUOUS"]
        assert torch.equal(c.world_view_transform.t().contiguous(), torch.from_numpy(vm.copy()).reshape(4, 4))
        assert torch.equal(c.camtoworlds[0, :3, 3], torch.from_numpy(cp.copy()))
        assert torch.equal(c.camtoworlds[0], c2w64[i].float())
        assert torch.equal(c.world_view_transform.t(), torch.inverse(c2w64[i]).float())
        assert c.world_view_transform.is_contiguous() and tuple(c.camtoworlds.shape) == (1, 4, 4)
        assert not torch.equal(c.camtoworlds[0], m.c2w0[i].float())  # and it did move


def test_json_round_trip(tmp_path):
    cams = _cameras()
    m = _model(cams, lr=1e-2, defer=False)
    m.perturb(0.03, seed=2)
    path = str(tmp_path / "poses.json")
    m.save_json(path, cams)
    data = json.load(open(path))
    assert sorted(data) == sorted(c.image_name for c in cams)
    assert len(data[cams[0].image_name]["delta"]) == 9 and np.array(data[cams[0].image_name]["world_to_camera"]).shape == (4, 4)
    cams2 = _cameras()
    m2 = _model(cams2)
    m2.load_json(path, cams2)
    assert torch.equal(m2.table, m.table)
    for a, b in zip(cams, cams2):
        assert torch.equal(a.world_view_transform, b.world_view_transform) and torch.equal(a.camtoworlds, b.camtoworlds)
    w2c = torch.tensor(data[cams[2].image_name]["world_to_camera"], dtype=F64)
    assert torch.equal(w2c.float(), cams[2].world_view_transform.t())


@pytest.mark.parametrize("over,word", [
    (dict(naive_offload=True), "naive_offload"),
    (dict(fused_front_end=False), "fused_front_end=False"),
    (dict(sh_residency="host"), 'sh_residency="host"'),
    (dict(sh_hbm_budget_gb=1.0), "sh_hbm_budget_gb"),
    (dict(depths="depth_dir"), "--depths"),
])
def test_refusals_by_name(over, word):
    with pytest.raises(ValueError, match="pose_opt is not supported with") as e:
        P.check_pose_args(utils.default_args(pose_opt=True, **over))
    assert word in str(e.value)
    P.check_pose_args(utils.default_args(**over))  # without pose_opt nothing is refused


def test_refusal_of_depth_priors_camera_dp_and_acceptance(monkeypatch):
    with pytest.raises(ValueError, match="depth render modes"):
        P.check_pose_args(utils.default_args(pose_opt=True), depth_priors=True)
    from clm_gs_amd import dp
    monkeypatch.setattr(dp, "world_size", lambda: 2)
    with pytest.raises(ValueError, match="camera-DP"):
        P.check_pose_args(utils.default_args(pose_opt=True, clm_offload=True))
    monkeypatch.setattr(dp, "world_size", lambda: 1)
    for over in (dict(clm_offload=True), dict(no_offload=True), dict(clm_offload=True, absgrad=True, mcmc=True),
                 dict(no_offload=True, rasterize_mode="antialiased", exposure=True), dict(clm_offload=True, bilagrid=True)):
        P.check_pose_args(utils.default_args(pose_opt=True, **over))
    # a model handed to the trainer is refused like the flag
    with pytest.raises(ValueError, match="naive_offload"):
        P.check_pose_args(utils.default_args(naive_offload=True), enabled=True)


def test_argument_defaults_and_command_line():
    a = utils.default_args()
    assert (a.pose_opt, a.pose_opt_lr, a.pose_opt_reg, a.pose_noise, a.defer_pose_step) == (False, 1e-5, 1e-6, 0.0, True)
    from clm_gs_amd import trainer
    ns = trainer.build_arg_parser().parse_args(["-s", "x", "-m", "y"])
    assert (ns.pose_opt, ns.pose_opt_lr, ns.pose_opt_reg, ns.pose_noise, ns.immediate_pose_step) == (False, 1e-5, 1e-6, 0.0, False)
    ns = trainer.build_arg_parser().parse_args(["-s", "x", "-m", "y", "--pose_opt", "--pose_opt_lr", "1e-4", "--pose_noise", "0.01"])
    assert ns.pose_opt and ns.pose_opt_lr == 1e-4 and ns.pose_noise == 0.01


def test_abi_table_and_header_carry_the_entries():
    from clm_gs_amd import _lib
    header = open(os.path.join(ROOT, "include", "clmgs.h")).read()
    for name in ("clmgs_pose_grad", "clmgs_pose_grad_finish", "clmgs_pose_grad_partials_rows",
                 "clmgs_projection_viewmat_bwd", "clmgs_projection_viewmat_partials_rows"):
        assert name in _lib.SIGNATURES and name + "(" in header, name
    # the inputs of clmgs_preprocess_bwd up to radii, in its order
    assert _lib.SIGNATURES["clmgs_pose_grad"][1][:17] == _lib.SIGNATURES["clmgs_preprocess_bwd"][1][:17]
    assert _lib.SIGNATURES["clmgs_pose_grad_finish"] == _lib.SIGNATURES["clmgs_exposure_grad_finish"]
    if os.path.exists(_lib.LIB_PATH):  # a host entry: no device needed
        L = _lib.lib()
        assert [int(L.clmgs_pose_grad_partials_rows(v)) for v in (0, 1, 64, 65, 196608, 196609, 300000)] == \
            [0, 1, 1, 2, 3072, 3072, 3072]


def test_projection_without_viewmat_gradient_launches_nothing_new():
    """The operator's backward asks for the camera gradient only when the view matrices require one: otherwise the helper
    returns None before it touches the library (the GPU test holds the outputs and gradients to the earlier ones)."""
    from clm_gs_amd import gsplat as G
    ctx = types.SimpleNamespace(needs_input_grad=(True, True, True, False, False), cfg=(64, 48, 0.3))
    assert G._viewmats_grad(ctx, *([None] * 10)) is None


def test_pose_math_header_against_central_differences(tmp_path):
    exe = str(tmp_path / "pose_math_host")
    subprocess.check_call(["g++", "-O1", "-I", os.path.join(ROOT, "clm_gs_amd", "csrc"),
                           os.path.join(ROOT, "tests", "host_shim", "pose_math_host.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True)
    print(out.stdout)
    assert out.returncode == 0, out.stdout + out.stderr
    worst = float(out.stdout.split("worst relative error")[1].split()[0])
    assert worst < 2e-3 and math.isfinite(worst)
