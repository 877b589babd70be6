"""CPU-only: the host side of the bilateral-grid colour correction (clm_gs_amd/bilagrid.py, cameras.camera_bilagrid, the
trainer's flags and refusals) and the float64 restatement the GPU tests compare against (tests/bilagrid_reference.py)."""
import math

import numpy as np
import pytest
import torch

from tests import bilagrid_reference as R
from tests import exposure_reference as ER


class _Cam:
    def __init__(self, name):
        self.image_name = name


def _cams(n):
    return [_Cam(f"img_{i:03d}.png") for i in range(n)]


def _small_case():
    """A 5x7 image with a pixel clamped on each side, a random (3, 4, 5) = (L, Hg, Wg) grid, a cotangent."""
    gen = torch.Generator().manual_seed(5)
    x = torch.rand(3, 5, 7, generator=gen, dtype=torch.float64) * 0.9 + 0.05
    x[:, 1, 2] = torch.tensor([1.2, 1.1, 1.3], dtype=torch.float64)   # s > 1
    x[:, 3, 4] = torch.tensor([-0.2, -0.1, 0.05], dtype=torch.float64)  # s < 0
    G = torch.randn(3, 4, 5, 12, generator=gen, dtype=torch.float64)
    g = torch.randn(3, 5, 7, generator=gen, dtype=torch.float64)
    return x, G, g


def _loop(x, G, g):
    """The definition, pixel by pixel and node by node: y, dL/dx (with the guidance term), dL/dG."""
    L, Hg, Wg, _ = G.shape
    _, H, W = x.shape
    lum = R.LUM
    y, v, dG = torch.zeros_like(x), torch.zeros_like(x), torch.zeros_like(G)
    for py in range(H):
        for px in range(W):
            xs = [float(x[k, py, px]) for k in range(3)] + [1.0]
            s = sum(lum[k] * xs[k] for k in range(3))
            fx, fy, fz = (px + 0.5) / W * (Wg - 1), (py + 0.5) / H * (Hg - 1), min(max(s, 0.0), 1.0) * (L - 1)
            x0, y0, z0 = min(math.floor(fx), Wg - 2), min(math.floor(fy), Hg - 2), min(math.floor(fz), L - 2)
            tx, ty, tz = fx - x0, fy - y0, fz - z0
            A, lo, hi = torch.zeros(12, dtype=x.dtype), torch.zeros(12, dtype=x.dtype), torch.zeros(12, dtype=x.dtype)
            for dz, wz in ((0, 1 - tz), (1, tz)):
                for dy, wy in ((0, 1 - ty), (1, ty)):
                    for dx, wx in ((0, 1 - tx), (1, tx)):
                        node = G[z0 + dz, y0 + dy, x0 + dx]
                        A += wz * wy * wx * node
                        (lo if dz == 0 else hi).add_(wy * wx * node)
                        for c in range(3):
                            for k in range(4):
                                dG[z0 + dz, y0 + dy, x0 + dx, 4 * c + k] += wz * wy * wx * float(g[c, py, px]) * xs[k]
            for c in range(3):
                y[c, py, px] = sum(float(A[4 * c + k]) * xs[k] for k in range(4))
            guide = sum(float(hi[4 * c + k] - lo[4 * c + k]) * float(g[c, py, px]) * xs[k] for c in range(3) for k in range(4))
            for k in range(3):
                v[k, py, px] = sum(float(A[4 * c + k]) * float(g[c, py, px]) for c in range(3))
                if 0.0 < s < 1.0:
                    v[k, py, px] += lum[k] * (L - 1) * guide
    return y, v, dG


def test_reference_is_the_hand_written_loop():
    x, G, g = _small_case()
    y0, v0, dG0 = _loop(x, G, g)
    y = R.apply(x, G)
    v, dG = R.vjp(x, G, g)
    P = R.parts(x, G)
    e = [float((a - b).abs().max()) for a, b in ((y, y0), (v, v0), (dG, dG0), (R.affine(P["A"].permute(2, 0, 1), x), y0))]
    print("bilagrid reference against the loop: max |difference| of y, dL/dx, dL/dG, parts:", e)
    assert max(e) < 1e-13
    assert not bool(P["inside"][1, 2]) and not bool(P["inside"][3, 4]) and int(P["inside"].sum()) == 33
    # the guidance term is there: without it dL/dx is another vector
    plain = torch.einsum("hwck,chw->khw", P["A"].reshape(5, 7, 3, 4)[..., :3], g)
    assert float((v - plain).abs().max()) > 0.1
    assert float((plain[:, 1, 2] - v[:, 1, 2]).abs().max()) < 1e-13  # ... and absent where s is clamped
    # an identity grid is the identity
    assert float((R.apply(x, R.identity(3, 4, 5)) - x).abs().max()) < 1e-15


def test_bounds_are_finite_positive_and_zero_only_where_no_pixel_reaches():
    """The bounds of the GPU tests, on their own (the kernels are held to them in tests/test_gpu_bilagrid.py): finite,
    positive for every element of y and dL/dx, positive for exactly the grid elements some pixel touches."""
    x, G, g = _small_case()
    b_y, b_v, b_G = R.bounds(x, G, g, chain=20)
    for b in (b_y, b_v, b_G):
        assert bool(torch.isfinite(b).all()) and bool((b >= 0).all())
    assert bool((b_y > 0).all()) and bool((b_v > 0).all())
    touched = R.vjp(x, G, g)[1] != 0
    assert bool((b_G[touched] > 0).all()) and not bool(b_G[~touched].any())


def test_tv_and_its_gradient():
    from clm_gs_amd import bilagrid as B
    gen = torch.Generator().manual_seed(2)
    for n, shape in ((1, (2, 2, 2)), (3, (4, 3, 5))):
        T = torch.randn(n, *shape, 12, generator=gen, dtype=torch.float64)
        L, Hg, Wg = shape
        want = 0.0
        for axis, count in ((1, (L - 1) * Hg * Wg), (2, L * (Hg - 1) * Wg), (3, L * Hg * (Wg - 1))):
            want += float((torch.diff(T, dim=axis) ** 2).sum()) / (12 * count)
        want /= n
        assert abs(float(R.tv(T)) - want) < 1e-12 and abs(float(B.tv_value(T)) - want) < 1e-12
        got, ref = B.tv_grad_reference(T, 10.0), R.tv_grad(T, 10.0)
        assert float((got - ref).abs().max()) < 1e-12 * float(ref.abs().max())
    assert float(B.tv_value(R.identity(4, 3, 5)[None])) == 0.0


def test_model_starts_as_identity_and_attach_hands_out_views():
    from clm_gs_amd.bilagrid import BilagridModel
    from clm_gs_amd.cameras import camera_bilagrid
    m = BilagridModel(3, "cpu", grid=(5, 3, 4))
    assert m.param.shape == (3, 4, 3, 5, 12) and m.grad.shape == m.param.shape and m.param.dtype == torch.float32
    assert torch.equal(m.param.detach(), R.identity(4, 3, 5, torch.float32).expand(3, 4, 3, 5, 12)) and not bool(m.grad.any())
    assert BilagridModel(1, "cpu").param.shape == (1, 8, 16, 16, 12)
    assert float(m.tv()) == 0.0
    cams = _cams(3)
    assert camera_bilagrid(cams[0]) == (None, None)
    m.attach(cams)
    grid, grad = camera_bilagrid(cams[1])
    assert grid.shape == (4, 3, 5, 12) and not grid.requires_grad and grid.is_contiguous() and grad.is_contiguous()
    grad[2, 1, 3, 7] = 5.0
    cams[2].bilagrid_grad += 1.0
    assert m.grad[1, 2, 1, 3, 7] == 5.0 and bool((m.grad[2] == 1.0).all()) and not bool(m.grad[0].any())
    with torch.no_grad():
        m.param[1, 0, 0, 0, 0] = 2.0
    assert cams[1].bilagrid[0, 0, 0, 0] == 2.0
    m.zero_grad()
    assert not bool(m.grad.any()) and cams[1].bilagrid_grad.data_ptr() == m.grad[1].data_ptr()
    cams[0].bilagrid = None
    assert camera_bilagrid(cams[0]) == (None, None)
    for bad in ((1, 16, 8), (16, 65, 8), (16, 16, 33), (16, 16, 1)):
        with pytest.raises(ValueError, match="bilateral grid shape"):
            BilagridModel(1, "cpu", grid=bad)


def test_model_steps_like_a_hand_written_adam():
    """Five steps with given gradients == Adam (beta 0.9 / 0.999, eps 1e-15, bias correction) over the WHOLE table on the
    given gradient plus the gradient of tv_weight * tv, at the scheduled learning rate (log-linear decay times the sine
    warm-up over 1000 steps from 0.01), to 1e-6."""
    from clm_gs_amd.bilagrid import BilagridModel
    n, steps, lr0, lr1, tvw = 3, 2000, 2e-3, 2e-5, 10.0
    m = BilagridModel(n, "cpu", grid=(3, 4, 2), lr_init=lr0, lr_final=lr1, max_steps=steps, tv_weight=tvw)
    cams = _cams(n)
    m.attach(cams)
    gen = torch.Generator().manual_seed(3)
    p = m.param.detach().double().clone()
    mom, var = torch.zeros_like(p), torch.zeros_like(p)
    for t, iteration in enumerate(range(1, 1602, 400), start=1):
        grads = torch.randn(n, 2, 4, 3, 12, generator=gen)
        grads[t % n] = 0.0  # a camera outside the batch
        for c, row in zip(cams, grads):
            c.bilagrid_grad += row
        lr = m.step(iteration)
        delay = 0.01 + 0.99 * math.sin(0.5 * math.pi * min(iteration / 1000, 1.0))
        want_lr = delay * math.exp(math.log(lr0) * (1 - iteration / steps) + math.log(lr1) * (iteration / steps))
        assert abs(lr - want_lr) < 1e-12
        m.zero_grad()
        gd = grads.double() + R.tv_grad(p, tvw)
        mom = 0.9 * mom + 0.1 * gd
        var = 0.999 * var + 0.001 * gd * gd
        p = p - want_lr * (mom / (1 - 0.9 ** t)) / ((var / (1 - 0.999 ** t)).sqrt() + 1e-15)
        assert float((m.param.detach().double() - p).abs().max()) < 1e-6, t
        assert torch.equal(cams[2].bilagrid, m.param.detach()[2])
    assert float((m.param.detach() - R.identity(2, 4, 3, torch.float32)).abs().max()) > 5e-4
    assert float(m.tv()) > 0.0


def test_zero_learning_rate_leaves_the_table_alone():
    from clm_gs_amd.bilagrid import BilagridModel
    m = BilagridModel(2, "cpu", grid=(2, 2, 2), lr_init=0.0, lr_final=0.0, max_steps=10)
    m.grad += 3.0
    assert m.step(1) == 0.0
    assert torch.equal(m.param.detach(), R.identity(2, 2, 2, torch.float32).expand(2, 2, 2, 2, 12))


def test_npz_round_trip_is_exact_and_in_gsplats_layout(tmp_path):
    from clm_gs_amd.bilagrid import BilagridModel
    cams = _cams(4)
    m = BilagridModel(4, "cpu", grid=(5, 3, 4))
    with torch.no_grad():
        m.param.copy_(torch.randn(4, 4, 3, 5, 12, generator=torch.Generator().manual_seed(1)) * 1.7 + 1e-7)
    path = tmp_path / "bilagrid.npz"
    m.save(str(path), cams)
    with np.load(path) as f:
        grids, names = f["grids"], list(f["image_names"])
    assert grids.shape == (4, 12, 4, 3, 5) and grids.dtype == np.float32 and names == [c.image_name for c in cams]
    assert grids[2, 7, 3, 1, 4] == float(m.param.detach()[2, 3, 1, 4, 7])  # [n, 12, L, Hg, Wg] <- [n, L, Hg, Wg, 12]
    fresh = BilagridModel(4, "cpu", grid=(5, 3, 4))
    fresh.load(str(path), list(reversed(cams)))  # keyed by image name, not by position
    assert torch.equal(fresh.param.detach(), m.param.detach().flip(0))
    partial = BilagridModel(2, "cpu", grid=(5, 3, 4))
    partial.load(str(path), [cams[3], _Cam("not_in_the_file.png")])
    assert torch.equal(partial.param.detach()[0], m.param.detach()[3])
    assert torch.equal(partial.param.detach()[1], R.identity(4, 3, 5, torch.float32))
    with pytest.raises(ValueError):
        BilagridModel(4, "cpu", grid=(5, 3, 5)).load(str(path), cams)


def test_trainer_parses_the_bilagrid_flags():
    from clm_gs_amd import trainer, utils
    ap = trainer.build_arg_parser()
    a = ap.parse_args(["-s", "src", "-m", "out"])
    assert a.bilagrid is False and a.bilagrid_shape == [16, 16, 8] and a.bilagrid_lr_init == 2e-3
    assert a.bilagrid_lr_final == 2e-5 and a.bilagrid_tv_weight == 10.0
    a = ap.parse_args(["-s", "src", "-m", "out", "--bilagrid", "--bilagrid_shape", "8", "6", "4", "--bilagrid_lr_init", "0.01",
                       "--bilagrid_lr_final", "1e-4", "--bilagrid_tv_weight", "5"])
    assert a.bilagrid is True and a.bilagrid_shape == [8, 6, 4] and a.bilagrid_lr_init == 0.01
    assert a.bilagrid_lr_final == 1e-4 and a.bilagrid_tv_weight == 5.0
    d = utils.default_args()
    assert d.bilagrid is False and tuple(d.bilagrid_shape) == (16, 16, 8) and d.bilagrid_lr_init == 2e-3
    assert d.bilagrid_lr_final == 2e-5 and d.bilagrid_tv_weight == 10.0
    assert utils.default_args(bilagrid=True).bilagrid is True


def test_the_two_refusals(monkeypatch, tmp_path):
    from clm_gs_amd import dp, trainer
    from clm_gs_amd.cameras import camera_bilagrid
    from clm_gs_amd.exposure import ExposureModel
    cams = _cams(4)
    model = trainer.build_bilagrid(cams, 100, device="cpu", grid=(5, 3, 4), lr_init=0.02, lr_final=0.002, tv_weight=3.0)
    assert model.n_cameras == 4 and model.tv_weight == 3.0 and model.shape == (4, 3, 5)
    assert cams[3].bilagrid.data_ptr() == model.param.detach()[3].data_ptr()
    # a camera carrying both an exposure row and a grid
    ExposureModel(4, "cpu").attach(cams)
    with pytest.raises(ValueError, match="both an exposure row and a bilateral grid"):
        camera_bilagrid(cams[0])
    # --exposure --bilagrid: refused before anything is loaded (the source directory does not even exist)
    with pytest.raises(ValueError, match="--exposure and --bilagrid"):
        trainer.train_from_colmap(str(tmp_path / "no_such_scene"), str(tmp_path / "out"), exposure=True, bilagrid=True)
    # camera-DP
    monkeypatch.setattr(dp, "world_size", lambda: 2)
    with pytest.raises(ValueError, match="camera-DP"):
        trainer.build_bilagrid(_cams(4), 100, device="cpu")
    with pytest.raises(ValueError, match="--bilagrid is not supported with camera-DP"):
        trainer.train_from_colmap(str(tmp_path / "no_such_scene"), str(tmp_path / "out"), bilagrid=True)
    assert not (tmp_path / "out").exists()


def test_grid_recovers_a_vignette_and_shadow_lift_a_global_fit_cannot():
    """A 32x48 scene of smooth ramps plus 5 % noise, seen through a gain that varies with position (vignette, 1 - 0.9 r^2)
    and with luminance (shadow lift, 1 + 0.6 (1 - s)^2), quantised to uint8.  300 Adam steps (0.01 -> 0.001) through the
    restated loss, once on a (Wg, Hg, L) = (6, 6, 4) grid and once on a single global 3x4 transform
    (tests/exposure_reference.py), both from the identity.  Run on their own: the loss goes 0.05324 -> 0.04857 for the
    global fit and 0.05324 -> 0.00167 for the grid, a factor 29; asserted with room: the grid ends below 1/10 of the global
    fit."""
    torch.manual_seed(0)
    H, W = 32, 48
    yy, xx = torch.meshgrid(torch.linspace(0, 1, H), torch.linspace(0, 1, W), indexing="ij")
    base = (torch.stack([0.15 + 0.6 * xx, 0.2 + 0.5 * yy, 0.1 + 0.7 * (xx * yy)]) + 0.05 * torch.rand(3, H, W)).double()
    r2 = ((xx - 0.5) ** 2 + (yy - 0.5) ** 2).double()
    gain = (1.0 - 0.9 * r2) * (1.0 + 0.6 * (1.0 - R.luminance(base)) ** 2)
    gt_u8 = ((base * gain[None]).clamp(0, 1) * 255).round().to(torch.uint8)

    def fit(param, loss_of, steps=300):
        opt = torch.optim.Adam([param], lr=0.01)
        first = last = None
        for i in range(steps):
            for group in opt.param_groups:
                group["lr"] = math.exp(math.log(0.01) * (1 - i / steps) + math.log(0.001) * (i / steps))
            opt.zero_grad()
            l = loss_of(param)
            l.backward()
            opt.step()
            first, last = (float(l.detach()) if first is None else first), float(l.detach())
        return first, last

    g_first, g_last = fit(ER.identity().requires_grad_(True), lambda E: ER.loss(base, E, gt_u8, None, 0.2))
    b_first, b_last = fit(R.identity(4, 6, 6).requires_grad_(True), lambda G: R.loss(base, G, gt_u8, None, 0.2))
    print(f"bilagrid recovery: global 3x4 fit {g_first:.5f} -> {g_last:.5f}, grid {b_first:.5f} -> {b_last:.5f}")
    assert abs(g_first - b_first) < 1e-12  # both start as the identity
    assert g_last > 0.5 * g_first, "the global fit cannot explain the gain"
    assert b_last < g_last / 10.0


def test_tv_grad_refuses_a_table_its_launch_grid_cannot_cover():
    """Host side of the entry only (refused before any launch, so it needs no device): n within the accepted range whose
    float4 count / 256 exceeds the launch grid's 2^31 - 1 blocks is an error, not a truncated grid."""
    import ctypes
    from clm_gs_amd import _lib
    L = _lib.lib()
    a, b = (ctypes.c_float * 64)(), (ctypes.c_float * 64)()
    pa, pb = (ctypes.c_void_p((ctypes.addressof(t) + 15) // 16 * 16) for t in (a, b))
    assert (1 << 24) * 32 * 64 * 64 * 3 // 256 > 2 ** 31 - 1
    assert L.clmgs_bilagrid_tv_grad(None, pa, 1 << 24, 32, 64, 64, 1.0, pb) == 10001
    assert b"INT32_MAX" in L.clmgs_last_error()
    assert L.clmgs_bilagrid_tv_grad(None, pa, (1 << 24) + 1, 2, 2, 2, 1.0, pb) == 10001
    assert L.clmgs_bilagrid_tv_grad(None, pa, 0, 2, 2, 2, 1.0, pb) == 10001
