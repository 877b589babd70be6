"""Compressed models on the device: csrc/vq.hip through clm_kernels.vq_assign / vq_update and clm_gs_amd/compress.py
against the float64 / Python-int restatement (tests/compress_reference.py): the exact arg-min on integer data, the
bounded arg-min on random floats, the guard elements, the bit-exact order-independent Lloyd update, fit_codebook, the
whole pipeline through a render, and the CLI."""
import ctypes
import os

import numpy as np
import pytest
import torch

from tests import compress_reference as R

pytestmark = pytest.mark.gpu

# (N, K): every N of {1, 31, 32, 33, 63, 64, 65, 257, 1000} and every K of {1, 2, 31, 32, 33, 65, 257, 4099} at least once;
# (513, 129): one row past the 512 rows of a workgroup with one centroid past the 128 of a staged codebook tile
SHAPES = [(1, 1), (31, 2), (32, 31), (33, 32), (63, 33), (64, 65), (65, 257), (257, 4099), (1000, 4099), (1000, 1), (1, 4099),
          (33, 257), (1000, 33), (513, 129)]
_CACHE = {}


def _int_case(N, K):
    """Small integers, so that every product and sum is exact in float32, and asymmetric: a value depends on its row
    and its column differently, rows and centroids differently.  Every tenth centroid repeats the one three before it
    (ties); columns 0..2 hold large values on both sides (the DC is ignored)."""
    key = ("int", N, K)
    if key not in _CACHE:
        n, k, j = np.arange(N)[:, None], np.arange(K)[:, None], np.arange(48)[None, :]
        x = ((n * 5 + j * 11 + (n ^ j) % 7) % 9 - 4).astype(np.float32)
        c = ((k * 7 + j * 3 + (k * j) % 5) % 9 - 4).astype(np.float32)
        for kk in range(9, K, 10):
            c[kk] = c[kk - 3]
        x[:, :3] = 1000.0 + (np.arange(N)[:, None] % 17) * 3 + np.arange(3)[None]
        c[:, :3] = -777.0 - (np.arange(K)[:, None] % 5)
        idx, d = R.assign64(x, c)
        _CACHE[key] = (x, c, idx, d)
    return _CACHE[key]


def _float_case(N, K, sigma):
    key = ("float", N, K, sigma)
    if key not in _CACHE:
        g = np.random.default_rng(N * 100003 + K)
        x = (g.standard_normal((N, 48)) * sigma).astype(np.float32)
        c = (g.standard_normal((K, 48)) * sigma).astype(np.float32)
        c[: K // 2] = x[g.integers(0, N, K // 2)] + (g.standard_normal((K // 2, 48)) * sigma * 0.05).astype(np.float32)
        _CACHE[key] = (x, c, R.dist64(x, c))
    return _CACHE[key]


def _dev(a, dev, dtype=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev, dtype).contiguous()


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


# ---------------------------------------------------------------------------------------------- 1. exact arg-min
@pytest.mark.parametrize("N,K", SHAPES)
def test_assign_is_exact_on_integer_data(dev, N, K):
    from clm_gs_amd import clm_kernels as CK
    x, c, idx64, d64 = _int_case(N, K)
    idx, dist = CK.vq_assign(_dev(x, dev), _dev(c, dev), want_dist=True)
    assert idx.dtype == torch.int32 and dist.dtype == torch.float32 and idx.shape == dist.shape == (N,)
    assert np.array_equal(idx.cpu().numpy().astype(np.int64), idx64)      # the lowest index on the planted ties
    assert np.array_equal(dist.cpu().numpy().astype(np.float64), d64)    # exact: integers below 2^24
    assert torch.equal(CK.vq_assign(_dev(x, dev), _dev(c, dev)), idx)


# ---------------------------------------------------------------------------------------------- 2. bounded arg-min
@pytest.mark.parametrize("sigma", [0.1, 1.0])
@pytest.mark.parametrize("N,K", [(1000, 4099), (257, 257), (65, 33), (513, 129)])
def test_assign_on_random_floats_is_within_the_rounding_bound(dev, N, K, sigma):
    """The kernel orders centroids by score = |c|^2 - 2 x.c.  x.c is a column-ordered float32 fmaf chain of length 48
    (the f32 MFMA), |c|^2 one of length 45, and one more fmaf joins them: at most 48 + 2 roundings, each of relative
    size 2^-24 of a partial sum; the partial sums of 2 x.c and |c|^2 together stay below 2 |x||c| + |c|^2 <=
    (|x| + max_k |c_k|)^2 (Cauchy-Schwarz).  So a computed score is within e = (48 + 2) 2^-24 (|x| + max_k |c_k|)^2 of the
    true one (the true score is d64 - |x|^2, the same shift for every centroid of a row); the chosen centroid's computed
    score is no larger than the best one's, hence d64[chosen] - d64[best] <= 2 e (e once for each).  `dist` is one value
    with no more roundings than that: within e of d64[chosen].  Nothing here is measured."""
    from clm_gs_amd import clm_kernels as CK
    x, c, d64 = _float_case(N, K, sigma)
    idx, dist = CK.vq_assign(_dev(x, dev), _dev(c, dev), want_dist=True)
    idx = idx.cpu().numpy().astype(np.int64)
    assert idx.min() >= 0 and idx.max() < K
    xn = np.linalg.norm(x[:, 3:].astype(np.float64), axis=1)
    cn = np.linalg.norm(c[:, 3:].astype(np.float64), axis=1).max()
    e = (48 + 2) * 2.0 ** -24 * (xn + cn) ** 2
    chosen = d64[np.arange(N), idx]
    excess = chosen - d64.min(1)
    print(f"N {N} K {K} sigma {sigma}: max excess / bound {float((excess / (2 * e)).max()):.3g}, rows not at the float64 "
          f"arg-min {int((idx != d64.argmin(1)).sum())}, max |dist - d64| / bound "
          f"{float((np.abs(dist.cpu().numpy().astype(np.float64) - chosen) / e).max()):.3g}")
    assert (excess <= 2 * e).all()
    assert (np.abs(dist.cpu().numpy().astype(np.float64) - chosen) <= e).all()


# ---------------------------------------------------------------------------------------------- 3. guards
@pytest.mark.parametrize("N,K", [(1, 1), (33, 31), (65, 257), (1000, 33), (513, 129)])
def test_outputs_are_written_inside_their_bounds_only(dev, N, K):
    from clm_gs_amd import _lib
    L = _lib.lib()
    x, c, idx64, d64 = _int_case(N, K)
    rows, cb = _dev(x, dev), _dev(c, dev)
    G = 64
    idx = torch.full((N + 2 * G,), -12345, dtype=torch.int32, device=dev)
    dist = torch.full((N + 2 * G,), -54321.0, dtype=torch.float32, device=dev)
    nbytes = int(L.clmgs_vq_assign_temp_bytes(K))
    temp = torch.full((nbytes + 2 * 256,), 0x5A, dtype=torch.uint8, device=dev)
    at = lambda t, off: ctypes.c_void_p(t.data_ptr() + off)
    _lib.check(L.clmgs_vq_assign(_lib.stream(), N, K, _lib.dptr(rows), _lib.dptr(cb), at(idx, 4 * G), at(dist, 4 * G),
                                 at(temp, 256), nbytes))
    assert np.array_equal(idx[G:G + N].cpu().numpy().astype(np.int64), idx64)
    assert np.array_equal(dist[G:G + N].cpu().numpy().astype(np.float64), d64)
    for t, fill in ((idx, -12345), (dist, -54321.0)):
        assert bool((t[:G] == fill).all()) and bool((t[G + N:] == fill).all())
    assert bool((temp[:256] == 0x5A).all()) and bool((temp[256 + 4 * K:] == 0x5A).all())
    # the update: accumulator, counts and codebook between guards
    acc = torch.full((K * 45 + 2 * G,), 7, dtype=torch.int64, device=dev)
    cnt = torch.full((K + 2 * G,), 7, dtype=torch.int64, device=dev)
    acc[G:G + K * 45] = 0
    cnt[G:G + K] = 0
    out = torch.full((K * 48 + 2 * G,), -3.0, dtype=torch.float32, device=dev)
    out[G:G + K * 48] = cb.reshape(-1)
    ii = idx[G:G + N].clone()
    _lib.check(L.clmgs_vq_accumulate(_lib.stream(), N, K, _lib.dptr(rows), _lib.dptr(ii), 1.0, at(acc, 8 * G), at(cnt, 8 * G)))
    _lib.check(L.clmgs_vq_finish(_lib.stream(), K, at(acc, 8 * G), at(cnt, 8 * G), 1.0, at(out, 4 * G)))
    for t, fill in ((acc, 7), (cnt, 7), (out, -3.0)):
        assert bool((t[:G] == fill).all()) and bool((t[-G:] == fill).all())
    ref, counts = R.update_int(x, idx64, c, 1.0)
    assert np.array_equal(cnt[G:G + K].cpu().numpy(), counts)
    assert np.array_equal(out[G:G + K * 48].cpu().numpy().reshape(K, 48).view(np.int32), ref.view(np.int32))


# ---------------------------------------------------------------------------------------------- 4. bit-exact update
def _update_case(name):
    g = np.random.default_rng(7)
    if name == "spread":       # centroid 5 receives no row
        N, K = 1000, 33
        idx = g.integers(0, K - 1, N)
        idx[idx >= 5] += 1
    elif name == "one_centroid":  # the worst atomic collision: every row adds to the same 45 words
        N, K = 1000, 5
        idx = np.full(N, 3)
    elif name == "one_row":
        N, K = 1, 2
        idx = np.array([1])
    else:                      # more than one grid-stride pass is not reached at these sizes; many centroids, few rows each
        N, K = 257, 4099
        idx = g.integers(0, K, N)
    x = (g.standard_normal((N, 48)) * g.choice([0.1, 1.0, 30.0], (N, 1))).astype(np.float32)
    c = g.standard_normal((K, 48)).astype(np.float32)
    return x, idx.astype(np.int32), c


@pytest.mark.parametrize("name", ["spread", "one_centroid", "one_row", "sparse"])
def test_update_equals_the_integer_definition_bit_for_bit(dev, name):
    from clm_gs_amd import clm_kernels as CK
    x, idx, c = _update_case(name)
    N, K = x.shape[0], c.shape[0]
    scale = R.vq_scale(N, float(np.abs(x).max()))
    assert CK.vq_scale(N, float(np.abs(x).max())) == scale and N * float(np.abs(x).max()) * scale < 2.0 ** 62
    ref, counts = R.update_int(x, idx, c, scale)
    rows, ii, cb = _dev(x, dev), _dev(idx, dev, torch.int32), _dev(c, dev)
    got, cnt = CK.vq_update(rows, ii, cb)
    assert got.shape == (K, 48) and got.dtype == torch.float32 and cnt.dtype == torch.int64
    assert torch.equal(cb.cpu(), torch.from_numpy(c))                       # the input codebook is left as it was
    assert np.array_equal(cnt.cpu().numpy(), counts)
    assert np.array_equal(got.cpu().numpy().view(np.int32), ref.view(np.int32))
    assert not got[:, :3].any()
    empty = counts == 0
    if empty.any():
        assert np.array_equal(got.cpu().numpy()[empty, 3:], c[empty, 3:])
    again, cnt2 = CK.vq_update(rows, ii, cb)
    assert torch.equal(_bits(again), _bits(got)) and torch.equal(cnt2, cnt)
    perm = torch.from_numpy(np.random.default_rng(11).permutation(N)).to(dev)
    shuffled, cnt3 = CK.vq_update(rows[perm].contiguous(), ii[perm].contiguous(), cb)
    assert torch.equal(_bits(shuffled), _bits(got)) and torch.equal(cnt3, cnt)


def test_operator_refusals(dev):
    from clm_gs_amd import clm_kernels as CK
    from clm_gs_amd._lib import ClmgsError
    rows, cb = torch.zeros(8, 48, device=dev), torch.zeros(4, 48, device=dev)
    with pytest.raises(ClmgsError, match="on the device"):
        CK.vq_assign(rows.cpu(), cb)
    with pytest.raises(ClmgsError, match="contiguous"):
        CK.vq_assign(torch.zeros(48, 8, device=dev).t(), cb)
    with pytest.raises(ClmgsError, match="float32"):
        CK.vq_assign(rows.double(), cb)
    with pytest.raises(ClmgsError, match="float32"):
        CK.vq_assign(torch.zeros(8, 45, device=dev), cb)
    with pytest.raises(ClmgsError, match="K must be"):
        CK.vq_assign(rows, torch.zeros(0, 48, device=dev))
    with pytest.raises(ClmgsError, match="K must be"):
        CK.vq_assign(rows, torch.zeros(65537, 48, device=dev))
    with pytest.raises(ClmgsError, match="idx"):
        CK.vq_update(rows, torch.zeros(8, dtype=torch.int64, device=dev), cb)


# ---------------------------------------------------------------------------------------------- 5. fit_codebook
def _clustered(n=4000, clusters=80, seed=3):
    g = np.random.default_rng(seed)
    centres = (g.standard_normal((clusters, 48)) * 0.3).astype(np.float32)
    which = np.sort(g.integers(0, clusters, n))  # neighbouring rows are alike, as in a Z-ordered table
    return (centres[which] + g.standard_normal((n, 48)).astype(np.float32) * 0.03).astype(np.float32)


def test_fit_codebook_descends_and_repeats(dev):
    from clm_gs_amd import compress
    x = _clustered()
    rows = _dev(x, dev)
    cb, hist = compress.fit_codebook(rows, K=64, iters=6)
    assert cb.shape == (64, 48) and len(hist) == 6 and not cb[:, :3].any()
    # a near-tie may flip at rounding level: the slack of the arg-min bound (test 2), summed over the rows; a centroid is
    # a mean of rows, so max_k |c_k| <= max_n |x_n|
    xn = np.linalg.norm(x[:, 3:].astype(np.float64), axis=1)
    slack = float((2 * (48 + 2) * 2.0 ** -24 * (xn + xn.max()) ** 2).sum())
    print("history", hist, "slack", slack)
    for a, b in zip(hist, hist[1:]):
        assert b <= a + slack
    assert hist[-1] < hist[0]
    cb2, hist2 = compress.fit_codebook(rows, K=64, iters=6)
    assert torch.equal(_bits(cb2), _bits(cb)) and hist2 == hist
    # the first assignment is against the same codebook as the float64 fit's: per row the chosen centroid is within 2 e of
    # the best and `dist` within e of the chosen one's distance, 3 e in all = 1.5 x the slack (later sums may drift apart)
    _, hist64 = R.fit_codebook64(x, 64, 1)
    assert abs(hist[0] - hist64[0]) <= 1.5 * slack
    # K is clamped to the sample; the sample is every ceil(N / sample)-th row
    cb3, _ = compress.fit_codebook(rows, K=65536, iters=1, sample=100)
    assert cb3.shape[0] == len(range(0, 4000, 40))


def _rows_dict(n, sh, seed=0):
    """A load_ply-style dict of host tensors whose Morton order is the row order (x grows with the row, y = 0)."""
    g = torch.Generator().manual_seed(seed)
    xyz = torch.stack([torch.arange(n, dtype=torch.float32) * 0.25, torch.zeros(n), torch.rand(n, generator=g)], 1)
    return dict(xyz=xyz, shs48=torch.from_numpy(np.ascontiguousarray(sh)), opacity=torch.randn(n, 1, generator=g),
                scaling=torch.randn(n, 3, generator=g) * 0.4 - 1.5, rotation=torch.randn(n, 4, generator=g))


def test_enough_centroids_reproduce_the_sh_rows_bit_for_bit(dev):
    from clm_gs_amd import compress
    g = np.random.default_rng(5)
    distinct = (g.standard_normal((64, 48)) * 0.3).astype(np.float32)
    sh = np.repeat(distinct, 64, axis=0)  # 4096 rows, 64 distinct ones in runs of 64: the even-stride start meets each
    rows = _rows_dict(4096, sh)
    cb, hist = compress.fit_codebook(_dev(sh, dev), K=64, iters=3)
    assert hist == [0.0, 0.0, 0.0]
    arrays, meta = compress.compress(rows, K=64, iters=3)
    assert meta["distortion"] == 0.0 and meta["empty"] == 0 and meta["K"] == 64
    back = compress.decompress(arrays, meta)
    assert torch.equal(_bits(back["shs48"][:, 3:]), _bits(rows["shs48"][:, 3:]))
    R.check_round_trip({k: v.numpy() for k, v in rows.items()}, {k: v.numpy() for k, v in back.items()})


# ---------------------------------------------------------------------------------------------- 6. end to end
E2E_MARGIN_DB = 0.1


def _scene_rows(n, seed=0):
    from tests.scenes import small_scene
    s = small_scene(n=n, width=64, height=48, seed=seed)
    rows = dict(xyz=s["means"].float(), shs48=s["shs"].reshape(n, 48).float().contiguous(),
                opacity=torch.logit(s["opac"].float().clamp(1e-4, 1 - 1e-4)), scaling=torch.log(s["scales"].float()),
                rotation=s["quats"].float())
    return s, rows


def _render(rows, s, dev):
    import math
    from clm_gs_amd import utils
    from clm_gs_amd.cameras import Camera
    from clm_gs_amd.render_trajectory import eval_one_cam
    from clm_gs_amd.strategies.no_offload import GaussianModelNoOffload
    args = utils.default_args(bsz=1)
    args.no_offload = True
    utils.set_args(args)
    utils.set_img_size(s["height"], s["width"])
    utils.set_cur_iter(1)
    f = float(s["K"][0, 0])
    cam = Camera(0, s["viewmat"], 2 * math.atan(s["width"] / (2 * f)), 2 * math.atan(s["height"] / (2 * f)), s["width"],
                 s["height"], device=dev)
    m = GaussianModelNoOffload(3, only_for_rendering=True)
    t = lambda k: torch.as_tensor(rows[k]).float().clone()
    m.create_from_tensors(t("xyz"), t("shs48"), t("scaling"), t("rotation"), t("opacity"), spatial_lr_scale=1.0)
    m.active_sh_degree = 3
    with torch.no_grad():
        return eval_one_cam(cam, m, None, args).clamp(0, 1).cpu()


def test_pipeline_renders_as_well_as_the_float64_pipeline(dev, tmp_path):
    """compress -> save -> io_ply.load_model -> render against the same through tests/compress_reference.pipeline64.
    Measured once on an MI355X (3000 rows, K = 256, 4 iterations, 64 x 48): 18.469 dB for the product, 18.469 dB for
    the float64 pipeline, no row assigned differently ("Compressed models").  Where no assignment flips the two pipelines are the same arithmetic (the update is bit-exact, the
    quantisers are float64 on both sides) and the two renders are equal; a flipped row takes a centroid that is as near
    as the best one up to rounding, i.e. an equally good approximation, and changes the codebook fit after it.  A margin
    of 0.1 dB is a 2.3 % change of the mean squared error: what a percent of the rows swapping one approximation for
    an equally good, independent one can do, and nothing a wrong centroid, a wrong field or a lost bit would stay under
    (one bit less in any field costs dBs)."""
    from clm_gs_amd import compress, io_ply
    from tests.scenes import psnr
    s, rows = _scene_rows(3000)
    arrays, meta = compress.compress(rows, K=256, iters=4)
    path = str(tmp_path / "scene.vq.npz")
    compress.save_compressed(path, arrays, meta)
    back = io_ply.load_model(path)
    ref, order, _, idx64 = R.pipeline64({k: v.numpy() for k, v in rows.items()}, 256, 4)
    orig = {k: v[torch.from_numpy(order)] for k, v in rows.items()}
    R.check_round_trip({k: v.numpy() for k, v in orig.items()}, {k: v.numpy() for k, v in back.items()})
    img0, img_p, img_r = _render(orig, s, dev), _render(back, s, dev), _render(ref, s, dev)
    p_prod, p_ref = psnr(img_p, img0), psnr(img_r, img0)
    flips = int((arrays["sh_idx"].astype(np.int64) != idx64).sum())
    print(f"PSNR decompressed vs original: product {p_prod:.3f} dB, float64 pipeline {p_ref:.3f} dB; "
          f"rows assigned differently {flips} of {len(idx64)}")
    assert float(img0.max()) > 0.2  # the scene is seen
    assert p_prod >= p_ref - E2E_MARGIN_DB


# ---------------------------------------------------------------------------------------------- 7. CLI
def test_cli_round_trip_and_render_trajectory(dev, tmp_path):
    from clm_gs_amd import compress, compress_model, io_ply, render_trajectory
    s, rows = _scene_rows(2000, seed=1)
    ply, npz, out_ply = (str(tmp_path / n) for n in ("in.ply", "out.vq.npz", "back.ply"))
    io_ply.save_ply(ply, rows["xyz"], rows["shs48"], rows["opacity"], rows["scaling"], rows["rotation"])
    assert compress_model.main(["-m", ply, "-o", npz, "--codebook", "128", "--iters", "3", "--decompress", out_ply]) == 0
    arrays, meta = compress.read_compressed(npz)
    assert meta["N"] == 2000 and meta["K"] == 128 and sum(a.nbytes for a in arrays.values()) == compress.expected_nbytes(meta)
    assert os.path.getsize(npz) < 2000 * 62 * 4 / 4
    back = io_ply.load_ply(out_ply)
    order = R.morton_order64(rows["xyz"].numpy())
    R.check_round_trip({k: v.numpy()[order] for k, v in rows.items()}, {k: v.numpy() for k, v in back.items()})
    cb = arrays["codebook"]
    assert np.array_equal(back["shs48"].numpy()[:, 3:], cb[arrays["sh_idx"].astype(np.int64)])
    frames = str(tmp_path / "frames")
    assert render_trajectory.main(["-m", npz, "--no_offload", "--n_frames", "1", "--width", "64", "--height", "48",
                                   "--manual_height", "8", "--hull", "0,0", "1,0", "0,0", "--output_dir", frames]) == 0
    img = render_trajectory.read_png(os.path.join(frames, "frame_00000.png"))
    assert img.shape == (48, 64, 3)


# ---------------------------------------------------------------------------------------------- 8. trainer and -s
def test_trainer_compress_and_the_scene_report(dev, tmp_path, capsys):
    """trainer --compress writes point_cloud.vq.npz next to the final .ply and logs the size line; compress_model -s on the
    model directory renders the scene's cameras from both models and reports the three PSNRs."""
    import re
    from clm_gs_amd import compress_model, io_ply, trainer
    from tests.test_gpu_exposure import _tiny_scene
    work, out = _tiny_scene(tmp_path), tmp_path / "out"
    gaussians, _, _ = trainer.train_from_colmap(str(work), str(out), strategy="clm_offload", iterations=8, bsz=4,
                                                disable_auto_densification=True, compress=True, compress_codebook=64,
                                                compress_iters=2, compress_pos_bits=14)
    it = out / "point_cloud" / "iteration_8"
    n = gaussians.get_xyz.shape[0]
    rows, packed = io_ply.load_ply(str(it / "point_cloud.ply")), io_ply.load_model(str(it / "point_cloud.vq.npz"))
    assert rows["xyz"].shape == packed["xyz"].shape == (n, 3) and packed["shs48"].shape == (n, 48)
    order = R.morton_order64(rows["xyz"].numpy())
    R.check_round_trip({k: v.numpy()[order] for k, v in rows.items()}, {k: v.numpy() for k, v in packed.items()},
                       dict(R.BITS, pos_bits=14))
    log = open(out / "python_ws=1_rk=0.log").read()
    assert re.search(rf"compressed model: rows {n} bytes {n * 248} -> \d+ \(\d+\.\dx\) K 64 empty centroids \d+ mean distortion", log)
    capsys.readouterr()
    assert compress_model.main(["-m", str(out), "-o", str(tmp_path / "again.vq.npz"), "--codebook", "64", "--iters", "2",
                                "-s", str(work)]) == 0
    line = capsys.readouterr().out
    m = re.search(r"PSNR original/gt ([\d.]+) compressed/gt ([\d.]+) compressed/original ([\d.]+|inf)", line)
    assert m, line
    print(line)
    assert float(m.group(3)) > float(m.group(2))  # the compressed model is nearer to the original than to the photographs
