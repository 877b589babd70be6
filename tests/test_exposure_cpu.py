"""CPU-only: the host side of per-camera exposure compensation (clm_gs_amd/exposure.py, cameras.camera_exposure, the
trainer's flags) and the float64 restatement the GPU tests compare against (tests/exposure_reference.py)."""
import json
import math

import pytest
import torch

from tests import exposure_reference as R


class _Cam:
    def __init__(self, name):
        self.image_name = name


def _cams(n):
    return [_Cam(f"img_{i:03d}.png") for i in range(n)]


def test_model_starts_as_identity_and_attach_hands_out_views():
    from clm_gs_amd.cameras import camera_exposure
    from clm_gs_amd.exposure import ExposureModel
    m = ExposureModel(3, "cpu")
    assert m.param.shape == (3, 3, 4) and m.grad.shape == (3, 3, 4) and m.param.dtype == torch.float32
    assert torch.equal(m.param.detach(), torch.eye(3, 4).expand(3, 3, 4)) and not bool(m.grad.any())
    cams = _cams(3)
    assert camera_exposure(cams[0]) == (None, None)  # a camera object without the attribute
    m.attach(cams)
    row, grad_row = camera_exposure(cams[1])
    assert row.shape == (3, 4) and not row.requires_grad and row.is_contiguous() and grad_row.is_contiguous()
    grad_row[2, 3] = 5.0  # a view: what a kernel adds into the camera's row shows in the table
    cams[2].exposure_grad += 1.0
    assert m.grad[1, 2, 3] == 5.0 and bool((m.grad[2] == 1.0).all()) and not bool(m.grad[0].any())
    with torch.no_grad():
        m.param[1, 0, 0] = 2.0
    assert cams[1].exposure[0, 0] == 2.0
    m.zero_grad()
    assert not bool(m.grad.any()) and cams[1].exposure_grad.data_ptr() == m.grad[1].data_ptr()
    cams[0].exposure = None  # explicitly none
    assert camera_exposure(cams[0]) == (None, None)


def test_model_steps_like_a_hand_written_adam():
    """Five steps with given gradients == Adam (beta 0.9 / 0.999, eps 1e-8, bias correction) over the WHOLE table at the
    scheduled learning rate exp(lerp(log lr_init, log lr_final, step / max_steps)), to 1e-6."""
    from clm_gs_amd.exposure import ExposureModel
    n, steps, lr0, lr1 = 4, 40, 0.01, 0.001
    m = ExposureModel(n, "cpu", lr_init=lr0, lr_final=lr1, max_steps=steps)
    cams = _cams(n)
    m.attach(cams)
    g = torch.Generator().manual_seed(3)
    p = torch.eye(3, 4, dtype=torch.float64).repeat(n, 1, 1)
    mom, var = torch.zeros_like(p), torch.zeros_like(p)
    for t, iteration in enumerate(range(1, 5 * 4 + 1, 4), start=1):  # the trainer's image counter, batch size 4
        grads = torch.randn(n, 3, 4, generator=g)
        grads[t % n] = 0.0  # a camera outside the batch: zero gradient, its moments still move it
        for c, row in zip(cams, grads):
            c.exposure_grad += row
        lr = m.step(iteration)
        want_lr = math.exp(math.log(lr0) * (1 - iteration / steps) + math.log(lr1) * (iteration / steps))
        assert abs(lr - want_lr) < 1e-12
        m.zero_grad()
        gd = grads.double()
        mom = 0.9 * mom + 0.1 * gd
        var = 0.999 * var + 0.001 * gd * gd
        p = p - want_lr * (mom / (1 - 0.9 ** t)) / ((var / (1 - 0.999 ** t)).sqrt() + 1e-8)
        assert float((m.param.detach().double() - p).abs().max()) < 1e-6, t
        assert torch.equal(cams[2].exposure, m.param.detach()[2])
    assert float((m.param.detach() - torch.eye(3, 4)).abs().max()) > 1e-3


def test_zero_learning_rate_leaves_the_table_alone():
    from clm_gs_amd.exposure import ExposureModel
    m = ExposureModel(2, "cpu", lr_init=0.0, lr_final=0.0, max_steps=10)
    m.grad += 3.0
    assert m.step(1) == 0.0
    assert torch.equal(m.param.detach(), torch.eye(3, 4).expand(2, 3, 4))


def test_json_round_trip_is_exact(tmp_path):
    from clm_gs_amd.exposure import ExposureModel
    cams = _cams(5)
    m = ExposureModel(5, "cpu")
    with torch.no_grad():
        m.param.copy_(torch.randn(5, 3, 4, generator=torch.Generator().manual_seed(1)) * 1.7 + 1e-7)
    path = tmp_path / "exposure.json"
    m.save_json(str(path), cams)
    table = json.load(open(path))
    assert sorted(table) == [c.image_name for c in cams]
    assert all(len(v) == 3 and all(len(r) == 4 for r in v) for v in table.values())
    assert table["img_003.png"][1][2] == float(m.param.detach()[3, 1, 2])
    fresh = ExposureModel(5, "cpu")
    fresh.load_json(str(path), list(reversed(cams)))  # keyed by image name, not by position
    assert torch.equal(fresh.param.detach(), m.param.detach().flip(0))
    partial = ExposureModel(2, "cpu")
    partial.load_json(str(path), [cams[4], _Cam("not_in_the_file.png")])
    assert torch.equal(partial.param.detach()[0], m.param.detach()[4])
    assert torch.equal(partial.param.detach()[1], torch.eye(3, 4))


def test_trainer_parses_the_exposure_flags():
    from clm_gs_amd import trainer, utils
    ap = trainer.build_arg_parser()
    a = ap.parse_args(["-s", "src", "-m", "out"])
    assert a.exposure is False and a.exposure_lr_init == 0.01 and a.exposure_lr_final == 0.001
    a = ap.parse_args(["-s", "src", "-m", "out", "--exposure", "--exposure_lr_init", "0.02", "--exposure_lr_final", "5e-4"])
    assert a.exposure is True and a.exposure_lr_init == 0.02 and a.exposure_lr_final == 5e-4
    d = utils.default_args()
    assert d.exposure is False and d.exposure_lr_init == 0.01 and d.exposure_lr_final == 0.001


def test_exposure_under_camera_dp_raises(monkeypatch, tmp_path):
    from clm_gs_amd import dp, trainer
    cams = _cams(4)
    model = trainer.build_exposure(cams, 100, device="cpu", lr_init=0.02, lr_final=0.002)
    assert model.n_cameras == 4 and cams[3].exposure.data_ptr() == model.param.detach()[3].data_ptr()
    assert abs(model.lr_func(0) - 0.02) < 1e-12 and abs(model.lr_func(100) - 0.002) < 1e-12
    monkeypatch.setattr(dp, "world_size", lambda: 2)
    with pytest.raises(ValueError, match="camera-DP"):
        trainer.build_exposure(_cams(4), 100, device="cpu")
    # the trainer's entry refuses before it loads anything: the source directory does not even exist
    with pytest.raises(ValueError, match="camera-DP"):
        trainer.train_from_colmap(str(tmp_path / "no_such_scene"), str(tmp_path / "out"), exposure=True)
    assert not (tmp_path / "out").exists()


def test_reference_vjp_is_the_autograd_of_apply():
    g0 = torch.Generator().manual_seed(2)
    x = torch.rand(3, 5, 7, generator=g0, dtype=torch.float64).requires_grad_()
    E = (torch.rand(3, 4, generator=g0, dtype=torch.float64) * 3 - 1.5).requires_grad_()
    g = torch.randn(3, 5, 7, generator=g0, dtype=torch.float64)
    y = R.apply(x, E)
    assert torch.equal(R.apply(x.detach(), R.identity()), x.detach())
    want = y.detach()[1, 2, 3]
    got = sum(x.detach()[k, 2, 3] * E.detach()[k, 1] for k in range(3)) + E.detach()[1, 3]
    assert abs(float(want - got)) < 1e-15
    y.backward(g)
    v_x, v_E = R.vjp(x.detach(), E.detach(), g)
    assert float((v_x - x.grad).abs().max()) < 1e-13 and float((v_E - E.grad).abs().max()) < 1e-12


def test_reference_recovers_a_known_transform():
    """A 32x48 scene of smooth ramps plus 5 % noise, seen through a known transform (gains 0.8-1.3, cross terms up to 0.1,
    biases up to 0.04) and quantised to uint8: 300 Adam steps (0.01 -> 0.001) on E alone through the restated loss.
    The restatement run on its own: loss 0.1301 -> 0.00099, max|E - E*| 0.29 -> 0.0116; asserted with room: final loss
    under 1/20 of the first, error under 0.05."""
    torch.manual_seed(0)
    H, W = 32, 48
    yy, xx = torch.meshgrid(torch.linspace(0, 1, H), torch.linspace(0, 1, W), indexing="ij")
    base = (torch.stack([0.2 + 0.5 * xx, 0.3 + 0.4 * yy, 0.25 + 0.3 * (xx * yy)]) + 0.05 * torch.rand(3, H, W)).double()
    E_true = torch.tensor([[1.3, 0.05, 0.0, 0.04], [0.0, 0.8, 0.1, -0.03], [0.05, 0.0, 1.15, 0.02]], dtype=torch.float64)
    gt_u8 = (R.apply(base, E_true).clamp(0, 1) * 255).round().to(torch.uint8)
    mask = torch.ones(H, W, dtype=torch.uint8)
    E = R.identity().requires_grad_(True)
    opt = torch.optim.Adam([E], lr=0.01)
    steps, first, last = 300, None, None
    err0 = float((E.detach() - E_true).abs().max())
    for i in range(steps):
        for group in opt.param_groups:
            group["lr"] = math.exp(math.log(0.01) * (1 - i / steps) + math.log(0.001) * (i / steps))
        opt.zero_grad()
        l = R.loss(base, E, gt_u8, mask, 0.2)
        l.backward()
        opt.step()
        first, last = (float(l) if first is None else first), float(l)
    err = float((E.detach() - E_true).abs().max())
    print(f"exposure recovery: loss {first:.4f} -> {last:.5f}, max|E - E*| {err0:.2f} -> {err:.4f}")
    assert last < first / 20.0
    assert err < 0.05
