"""CPU-only: the host side of the learnable sky (clm_gs_amd/sky.py, cameras.camera_sky, the trainer's and the trajectory
renderer's flags) and the float64 restatement the GPU tests compare against (tests/sky_reference.py)."""
import math

import numpy as np
import pytest
import torch

from tests import masked_loss_reference as M
from tests import sky_reference as R

UNIT = 2.0 ** -48


class _Cam:
    def __init__(self, name="a"):
        self.image_name = name


# ------------------------------------------------------------------------------------------ the restatement
def _map(Hs, Ws, seed=0):
    return torch.rand(Hs, Ws, 3, generator=torch.Generator().manual_seed(seed), dtype=torch.float64)


def test_a_camera_looking_along_z_hits_the_map_centre():
    """d = (0,0,1): u = Ws/2 - 1/2, v = Hs/2 - 1/2 -- between the four central texels of an even map, weights 1/4 each;
    on the central texel of an odd map, weight 1."""
    vm, K = torch.eye(4, dtype=torch.float64), torch.tensor([[10.0, 0, 0.5], [0, 10.0, 0.5], [0, 0, 1]], dtype=torch.float64)
    u, v = R.coordinates(vm, K, 1, 1, 8, 16)
    assert float(u) == 7.5 and float(v) == 3.5
    S = _map(8, 16)
    s = R.sample(S, vm, K, 1, 1)[:, 0, 0]
    assert float((s - S[3:5, 7:9].mean(dim=(0, 1))).abs().max()) < 1e-15
    S = _map(5, 9)
    assert float((R.sample(S, vm, K, 1, 1)[:, 0, 0] - S[2, 4]).abs().max()) < 1e-15
    # y = x + (1 - alpha) s
    x, a = torch.full((3, 1, 1), 0.25, dtype=torch.float64), torch.tensor([[0.75]], dtype=torch.float64)
    assert float((R.apply(x, a, S, vm, K)[:, 0, 0] - (0.25 + 0.25 * S[2, 4])).abs().max()) < 1e-15


def test_the_seam_wraps():
    """A camera looking along -z sees u = -1/2 or Ws - 1/2 at its centre: the two texels are columns Ws - 1 and 0."""
    vm = R.look_at_camera((0.0, 0.0, -1.0))
    K = torch.tensor([[50.0, 0, 1.0], [0, 50.0, 0.5], [0, 0, 1]], dtype=torch.float64)  # two pixels, left and right of the axis
    S = _map(4, 8)
    rows, cols, w = R.taps(vm, K, 1, 2, 4, 8)
    assert set(cols.reshape(-1).tolist()) == {7, 0}
    assert bool((w >= 0).all()) and float((w.sum(-1) - 1).abs().max()) < 1e-15
    s = R.sample(S, vm, K, 1, 2)
    # by hand for pixel 0: dc = (-.5/50, 0, 1)
    d = vm[:3, :3].T @ (torch.tensor([-0.01, 0.0, 1.0], dtype=torch.float64) / math.sqrt(1 + 1e-4))
    u = (math.atan2(float(d[0]), float(d[2])) / (2 * math.pi) + 0.5) * 8 - 0.5
    iu, fu = math.floor(u), u - math.floor(u)
    want = 0.5 * ((1 - fu) * (S[1, iu % 8] + S[2, iu % 8]) + fu * (S[1, (iu + 1) % 8] + S[2, (iu + 1) % 8]))
    assert float((s[:, 0, 0] - want).abs().max()) < 1e-14


def test_the_poles_clamp():
    """Straight up (world -y) and straight down: v = -1/2 resp. Hs - 1/2, both rows clamp to the first resp. last row."""
    K = torch.tensor([[10.0, 0, 0.5], [0, 10.0, 0.5], [0, 0, 1]], dtype=torch.float64)
    S = _map(6, 4)
    for fwd, row in (((0.0, -1.0, 0.0), 0), ((0.0, 1.0, 0.0), 5)):
        vm = R.look_at_camera(fwd)
        rows, cols, w = R.taps(vm, K, 1, 1, 6, 4)
        assert set(rows.reshape(-1).tolist()) == {row}
        s = R.sample(S, vm, K, 1, 1)[:, 0, 0]
        c0, c1 = int(cols[0, 0, 0]), int(cols[0, 0, 1])
        wa, wb = float(w[0, 0, 0] + w[0, 0, 2]), float(w[0, 0, 1] + w[0, 0, 3])
        assert float((s - (wa * S[row, c0] + wb * S[row, c1])).abs().max()) < 1e-15


def test_a_one_texel_map_is_a_constant():
    S = _map(1, 1)
    vm = R.look_at_camera((0.3, -0.5, 0.8), roll=0.4)
    s = R.sample(S, vm, R.intrinsics(7, 5, 80.0), 5, 7)
    assert float((s - S[0, 0][:, None, None]).abs().max()) < 1e-15


def test_reference_vjp_is_the_autograd_of_apply():
    g0 = torch.Generator().manual_seed(2)
    x = torch.rand(3, 5, 7, generator=g0, dtype=torch.float64).requires_grad_()
    a = torch.rand(5, 7, generator=g0, dtype=torch.float64).requires_grad_()
    S = _map(4, 8, 3).requires_grad_()
    g = torch.randn(3, 5, 7, generator=g0, dtype=torch.float64)
    vm, K = R.look_at_camera((0.2, 0.1, -1.0), roll=0.3), R.intrinsics(7, 5, 100.0)
    R.apply(x, a, S, vm, K).backward(g)
    v_a, v_S = R.vjp(a.detach(), S.detach(), vm, K, g)
    assert torch.equal(x.grad, g)
    assert float((v_a - a.grad).abs().max()) < 1e-13 and float((v_S - S.grad).abs().max()) < 1e-13


# ------------------------------------------------------------------------------------------ SkyModel
def test_model_starts_constant_and_attach_hands_out_the_shared_map():
    from clm_gs_amd.cameras import camera_sky
    from clm_gs_amd.sky import SkyModel
    m = SkyModel((4, 8), "cpu", init=(0.1, 0.2, 0.3))
    assert m.param.shape == (4, 8, 3) and m.param.dtype == torch.float32 and m.shape == (4, 8)
    assert torch.equal(m.param.detach(), torch.tensor([0.1, 0.2, 0.3]).expand(4, 8, 3))
    assert m.acc.dtype == torch.int64 and m.acc.shape == (4, 8, 3) and not bool(m.acc.any()) and not bool(m.grad.any())
    d = SkyModel(device="cpu")
    assert d.shape == (256, 512) and bool((d.param.detach() == 0.5).all())
    train, test = [_Cam(), _Cam()], [_Cam()]
    assert camera_sky(train[0]) is None  # a camera object without the attribute
    m.attach(train, train=True)
    m.attach(test, train=False)
    (s0, a0), (s1, a1), (s2, a2) = (camera_sky(c) for c in train + test)
    assert s0.data_ptr() == s1.data_ptr() == s2.data_ptr() == m.param.data_ptr() and not s0.requires_grad
    assert a0 is m.acc and a1 is m.acc and a2 is None
    with torch.no_grad():
        m.param[1, 2, 0] = 2.0
    assert test[0].sky[1, 2, 0] == 2.0  # one table, shared
    train[0].sky = None
    assert camera_sky(train[0]) is None
    with pytest.raises(ValueError, match="sky_shape"):
        SkyModel((0, 8), "cpu")


def test_model_steps_like_a_hand_written_adam():
    """Five steps, the gradients handed over as the kernels do -- fixed-point sums of two cameras in the int64 accumulator --
    == Adam (beta 0.9 / 0.999, eps 1e-8, bias correction) over the whole map at the scheduled learning rate, to 1e-6 (the
    bound of tests/test_exposure_cpu.py)."""
    from clm_gs_amd.sky import SkyModel
    steps, lr0, lr1 = 40, 0.01, 0.001
    m = SkyModel((3, 5), "cpu", lr_init=lr0, lr_final=lr1, max_steps=steps)
    cams = [_Cam(), _Cam()]
    m.attach(cams)
    g = torch.Generator().manual_seed(3)
    p = torch.full((3, 5, 3), 0.5, dtype=torch.float64)
    mom, var = torch.zeros_like(p), torch.zeros_like(p)
    for t, iteration in enumerate(range(1, 5 * 4 + 1, 4), start=1):
        q = [torch.round(torch.randn(3, 5, 3, generator=g, dtype=torch.float64) / UNIT).to(torch.int64) for _ in cams]
        q[0][t % 3] = 0
        q[1][t % 3] = 0  # texels no camera saw: zero gradient, their moments still move them
        for c, qi in zip(cams, q):
            c.sky_acc += qi
        lr = m.step(iteration)
        want_lr = math.exp(math.log(lr0) * (1 - iteration / steps) + math.log(lr1) * (iteration / steps))
        assert abs(lr - want_lr) < 1e-12
        assert not bool(m.acc.any()), "the step converts the accumulator and zeroes it"
        gd = ((q[0] + q[1]).double() * UNIT).float()
        assert torch.equal(m.grad, gd), "the cameras are summed in integers and converted once"
        m.zero_grad()
        gd = gd.double()
        mom = 0.9 * mom + 0.1 * gd
        var = 0.999 * var + 0.001 * gd * gd
        p = p - want_lr * (mom / (1 - 0.9 ** t)) / ((var / (1 - 0.999 ** t)).sqrt() + 1e-8)
        assert float((m.param.detach().double() - p).abs().max()) < 1e-6, t
        assert cams[1].sky.data_ptr() == m.param.data_ptr()
    assert float((m.param.detach() - 0.5).abs().max()) > 1e-3


def test_npz_round_trip_is_exact(tmp_path):
    from clm_gs_amd import sky
    m = sky.SkyModel((5, 7), "cpu")
    with torch.no_grad():
        m.param.copy_(torch.randn(5, 7, 3, generator=torch.Generator().manual_seed(1)) * 1.7 + 1e-7)
    path = m.save(str(tmp_path))
    assert path == str(tmp_path / "sky.npz")
    with np.load(path) as f:
        assert sorted(f.files) == ["convention", "shape", "sky"]
        assert tuple(f["shape"]) == (5, 7) and str(f["convention"]) == sky.CONVENTION and f["sky"].dtype == np.float32
    fresh = sky.SkyModel.from_file(str(tmp_path), "cpu")
    assert fresh.shape == (5, 7) and torch.equal(fresh.param.detach(), m.param.detach())
    other = sky.SkyModel((4, 7), "cpu")
    with pytest.raises(ValueError, match="the model is"):
        other.load(str(tmp_path))
    with pytest.raises(FileNotFoundError, match="sky.npz"):
        sky.SkyModel.from_file(str(tmp_path / "nothing_here"), "cpu")


# ------------------------------------------------------------------------------------------ flags and refusals
def test_trainer_parses_the_sky_flags():
    from clm_gs_amd import trainer, utils
    ap = trainer.build_arg_parser()
    a = ap.parse_args(["-s", "src", "-m", "out"])
    assert a.sky is False and a.sky_shape == [256, 512] and a.sky_init == [0.5, 0.5, 0.5]
    assert a.sky_lr_init == 0.01 and a.sky_lr_final == 0.001
    a = ap.parse_args(["-s", "src", "-m", "out", "--sky", "--sky_shape", "64", "128", "--sky_init", "0.1", "0.2", "0.3",
                       "--sky_lr_init", "0.02", "--sky_lr_final", "5e-4"])
    assert a.sky is True and a.sky_shape == [64, 128] and a.sky_init == [0.1, 0.2, 0.3]
    assert a.sky_lr_init == 0.02 and a.sky_lr_final == 5e-4
    d = utils.default_args()
    assert d.sky is False and tuple(d.sky_shape) == (256, 512) and tuple(d.sky_init) == (0.5, 0.5, 0.5)
    assert d.sky_lr_init == 0.01 and d.sky_lr_final == 0.001


def test_build_sky_attaches_training_and_other_cameras():
    from clm_gs_amd import trainer
    train, test = [_Cam(), _Cam()], [_Cam()]
    model = trainer.build_sky(train, test, 100, device="cpu", shape=(4, 8), init=(0.2, 0.3, 0.4), lr_init=0.02, lr_final=0.002)
    assert model.shape == (4, 8) and train[1].sky_acc is model.acc and test[0].sky_acc is None
    assert test[0].sky.data_ptr() == model.param.data_ptr()
    assert abs(model.lr_func(0) - 0.02) < 1e-12 and abs(model.lr_func(100) - 0.002) < 1e-12


def test_sky_with_a_white_background_raises(tmp_path):
    from clm_gs_amd import render_trajectory, trainer
    from clm_gs_amd.cameras import check_sky_background
    with pytest.raises(ValueError, match="white_background"):  # before anything is loaded: the source does not exist
        trainer.train_from_colmap(str(tmp_path / "no_such_scene"), str(tmp_path / "out"), sky=True, white_background=True)
    assert not (tmp_path / "out").exists()
    check_sky_background(None)
    check_sky_background(torch.zeros(3))
    with pytest.raises(ValueError, match="non-zero background"):
        check_sky_background(torch.tensor([0.0, 1.0, 0.0]))
    with pytest.raises(SystemExit, match="white_background"):
        render_trajectory.main(["-m", str(tmp_path), "--sky", "--white_background"])
    with pytest.raises(SystemExit, match="sky.npz"):  # a clear message when the map is missing
        render_trajectory.main(["-m", str(tmp_path), "--sky"])


def test_sky_with_pose_refinement_raises(tmp_path):
    from clm_gs_amd import trainer
    from clm_gs_amd.cameras import camera_sky
    with pytest.raises(ValueError, match="pose_opt"):
        trainer.train_from_colmap(str(tmp_path / "no_such_scene"), str(tmp_path / "out"), sky=True, pose_opt=True)
    assert not (tmp_path / "out").exists()
    cam = _Cam()
    cam.sky, cam.sky_acc, cam.pose_grad = torch.zeros(2, 2, 3), None, torch.zeros(15)
    with pytest.raises(ValueError, match="pose"):
        camera_sky(cam)


def test_sky_under_camera_dp_raises(monkeypatch, tmp_path):
    from clm_gs_amd import dp, trainer
    monkeypatch.setattr(dp, "world_size", lambda: 2)
    with pytest.raises(ValueError, match="camera-DP"):
        trainer.build_sky([_Cam()], [], 100, device="cpu")
    with pytest.raises(ValueError, match="camera-DP"):
        trainer.train_from_colmap(str(tmp_path / "no_such_scene"), str(tmp_path / "out"), sky=True)
    assert not (tmp_path / "out").exists()


# ------------------------------------------------------------------------------------------ recovery
def _partial_cover(H, W, seed):
    """A small synthetic scene that covers only part of the frame: a handful of opaque 2D Gaussians blended front to back
    -> (x [3,H,W] with no background, alpha [H,W])."""
    g = torch.Generator().manual_seed(seed)
    yy, xx = torch.meshgrid(torch.arange(H, dtype=torch.float64) + 0.5, torch.arange(W, dtype=torch.float64) + 0.5, indexing="ij")
    x, T = torch.zeros(3, H, W, dtype=torch.float64), torch.ones(H, W, dtype=torch.float64)
    for _ in range(5):
        cx, cy = float(torch.rand(1, generator=g)) * W, (0.55 + 0.45 * float(torch.rand(1, generator=g))) * H  # lower half
        sig = (0.08 + 0.1 * float(torch.rand(1, generator=g))) * W
        a = (0.95 * torch.exp(-((xx - cx) ** 2 + (yy - cy) ** 2) / (2 * sig * sig))).clamp(max=0.999)
        col = torch.rand(3, generator=g, dtype=torch.float64)
        x = x + (T * a)[None] * col[:, None, None]
        T = T * (1 - a)
    return x, 1 - T


def test_reference_recovers_a_known_map():
    """Six 24x32 cameras at the origin looking around the horizon and upwards (fields of view of 70 degrees), each in front
    of five opaque blobs in the lower half of its frame, ground truth rendered with a known smooth non-constant 8x16 map and
    quantised to uint8; 300 Adam steps (0.01 -> 0.001, the model's defaults) on the map alone, from its constant start,
    through the restated composite and loss.  Compared over the texels that some camera sees with 1 - alpha > 0.5 at a
    bilinear weight above 0.25 (the others are not determined by the images).
    The restatement run on its own: summed loss 0.6013 -> 0.00492, max|S - S*| 0.400 -> 0.0056 over 78 of 128 texels;
    asserted with room: final loss under 1/20 of the first, error under 1/8 of the first."""
    H, W, Hs, Ws = 24, 32, 8, 16
    jj, ii = torch.meshgrid(torch.arange(Hs, dtype=torch.float64), torch.arange(Ws, dtype=torch.float64), indexing="ij")
    S_true = torch.stack([0.5 + 0.4 * torch.sin(2 * math.pi * ii / Ws), 0.2 + 0.6 * jj / (Hs - 1),
                          0.5 + 0.4 * torch.cos(2 * math.pi * ii / Ws) * (jj / (Hs - 1))], dim=-1)
    K = R.intrinsics(W, H, 70.0)
    views = [R.look_at_camera(f) for f in ((0, 0, 1), (1, -0.2, 0.3), (0.2, -0.3, -1), (-1, -0.1, -0.2), (-0.5, -1, 0.6),
                                           (0.6, -0.9, -0.5))]
    scenes = [_partial_cover(H, W, 40 + i) for i in range(len(views))]
    gts = [(R.apply(x, a, S_true, vm, K).clamp(0, 1) * 255).round().to(torch.uint8) for (x, a), vm in zip(scenes, views)]
    seen = torch.zeros(Hs * Ws, dtype=torch.bool)
    for (x, a), vm in zip(scenes, views):
        rows, cols, w = R.taps(vm, K, H, W, Hs, Ws)
        hit = ((1 - a)[..., None] > 0.5) & (w > 0.25)
        seen[(rows * Ws + cols)[hit]] = True
    seen = seen.reshape(Hs, Ws)
    assert int(seen.sum()) >= 32
    S = torch.full((Hs, Ws, 3), 0.5, dtype=torch.float64).requires_grad_()
    opt = torch.optim.Adam([S], lr=0.01)
    steps, first, last = 300, None, None
    err0 = float((S.detach() - S_true)[seen].abs().max())
    for i in range(steps):
        for group in opt.param_groups:
            group["lr"] = math.exp(math.log(0.01) * (1 - i / steps) + math.log(0.001) * (i / steps))
        opt.zero_grad()
        l = sum(M.masked_loss(R.apply(x, a, S, vm, K), gt, None, 0.2) for (x, a), vm, gt in zip(scenes, views, gts))
        l.backward()
        opt.step()
        first, last = (float(l.detach()) if first is None else first), float(l.detach())
    err = float((S.detach() - S_true)[seen].abs().max())
    print(f"sky recovery: summed loss {first:.4f} -> {last:.5f}, max|S - S*| {err0:.3f} -> {err:.4f} over {int(seen.sum())} of "
          f"{Hs * Ws} texels")
    assert last < first / 20.0
    assert err < err0 / 8.0
