"""Compressed models without a GPU: the host side of clm_gs_amd/compress.py (quantisers, the file, the size formula,
io_ply.load_model) against tests/compress_reference.py, and the reference pipeline's own lossless case.  The codebook
fit and the assignment need the device (tests/test_gpu_compress.py); here the SH indices come from the float64
reference."""
import json
import os

import numpy as np
import pytest
import torch

from tests import compress_reference as R


def _rows(n, seed=0, distinct_sh=None):
    """A load_ply-style dict of host tensors; a city-like extent (kilometres in x and y) so that chunking matters."""
    g = torch.Generator().manual_seed(seed)
    xyz = torch.rand(n, 3, generator=g) * torch.tensor([2000.0, 1500.0, 80.0]) - torch.tensor([1000.0, 700.0, 0.0])
    sh = torch.randn(n, 48, generator=g) * 0.1
    sh[:, :3] = torch.randn(n, 3, generator=g)
    if distinct_sh is not None:
        pool = torch.randn(distinct_sh, 45, generator=g) * 0.2
        sh[:, 3:] = pool[torch.randint(0, distinct_sh, (n,), generator=g)]
    return dict(xyz=xyz, shs48=sh.contiguous(), opacity=torch.randn(n, 1, generator=g) * 1.5,
                scaling=torch.randn(n, 3, generator=g) * 0.4 - 0.3, rotation=torch.randn(n, 4, generator=g))


def _sorted_np(rows):
    order = R.morton_order64(rows["xyz"].numpy())
    return {k: v.numpy()[order] for k, v in rows.items()}, order


def _encode(rows, K=16, bits=None):
    """Product encode of the Morton-sorted rows with the float64 reference's codebook and indices."""
    from clm_gs_amd import compress
    srt, order = _sorted_np(rows)
    cb, _ = R.fit_codebook64(srt["shs48"], K, 2)
    idx, _ = R.assign64(srt["shs48"], cb)
    arrays, meta = compress.encode(srt, idx, cb, bits)
    return srt, arrays, meta, cb, idx


@pytest.mark.parametrize("bits", [None, dict(pos_bits=12, scale_bits=6, opacity_bits=5, rot_bits=10, dc_bits=7),
                                  dict(pos_bits=8, scale_bits=16, opacity_bits=16, rot_bits=6, dc_bits=16)])
@pytest.mark.parametrize("n", [1, 255, 256, 257, 1000])
def test_quantiser_round_trip_is_within_half_a_step(n, bits):
    """|x - dq(q(x))| <= (hi - lo) / (2^b - 1) / 2 plus one float32 ulp of max(|lo|, |hi|), per chunk of 256 rows for
    positions and log-scales, globally for opacity and the DC; the quaternion up to sign within the same bound per
    stored component, the rebuilt largest one within the bound check_round_trip derives."""
    from clm_gs_amd import compress
    rows = _rows(n, seed=n)
    srt, arrays, meta, cb, idx = _encode(rows, K=min(16, n), bits=bits)
    full = dict(R.BITS, **(bits or {}))
    assert {k: meta[k] for k in R.BITS} == full
    back = {k: v.numpy() for k, v in compress.decompress(arrays, meta).items()}
    R.check_round_trip(srt, back, full)
    # the codes are the reference's codes, the decoded values the reference's values
    rep = np.arange(n) // 256
    lo, hi = R.chunk_bounds(srt["xyz"])
    assert np.array_equal(arrays["pos"], R.quantise(srt["xyz"], lo[rep], hi[rep], full["pos_bits"]))
    assert np.array_equal(back["xyz"], R.dequantise(arrays["pos"], lo[rep], hi[rep], full["pos_bits"]))
    codes, big = R.quat_encode(srt["rotation"], full["rot_bits"])
    assert np.array_equal(arrays["rot"], codes) and np.array_equal(arrays["rot_big"], big)
    assert np.array_equal(back["rotation"], R.quat_decode(codes, big, full["rot_bits"]))
    assert np.array_equal(back["shs48"][:, 3:], cb[idx][:, 3:])


def test_constant_fields_and_quaternion_edge_cases():
    """hi == lo gives code 0 and decodes to the value; a quaternion with a negative largest component, a tie of the
    largest, an axis-aligned one and an un-normalised one."""
    from clm_gs_amd import compress
    rows = _rows(300, seed=4)
    rows["opacity"][:] = 0.75
    rows["scaling"][:256, 1] = -2.0
    rows["rotation"][:5] = torch.tensor([[0.1, -0.9, 0.2, 0.1], [0.5, 0.5, -0.5, 0.5], [0.0, 0.0, 0.0, -3.0],
                                         [10.0, 0.0, 0.0, 0.0], [-0.5, -0.5, -0.5, -0.5]])
    srt, arrays, meta, _, _ = _encode(rows)
    back = {k: v.numpy() for k, v in compress.decompress(arrays, meta).items()}
    assert not arrays["opacity"].any() and (back["opacity"] == np.float32(0.75)).all()
    R.check_round_trip(srt, back)
    assert (np.abs(np.linalg.norm(back["rotation"].astype(np.float64), axis=1) - 1.0) < 1e-6).all()


def test_file_round_trip_and_load_model(tmp_path):
    from clm_gs_amd import compress, io_ply
    rows = _rows(700, seed=2)
    srt, arrays, meta, _, _ = _encode(rows)
    path = str(tmp_path / "m.vq.npz")
    compress.save_compressed(path, arrays, meta)
    assert os.path.exists(path) and not os.path.exists(path + ".npz")
    arrays2, meta2 = compress.read_compressed(path)
    assert meta2 == json.loads(json.dumps(meta)) and set(arrays2) == set(arrays)
    for k in arrays:
        assert arrays2[k].dtype == arrays[k].dtype and np.array_equal(arrays2[k], arrays[k]), k
    ply = str(tmp_path / "m.ply")
    io_ply.save_ply(ply, *(torch.from_numpy(srt[k]) for k in ("xyz", "shs48", "opacity", "scaling", "rotation")))
    from_ply, from_npz = io_ply.load_model(ply), io_ply.load_model(path)
    assert set(from_npz) == set(from_ply) == {"xyz", "shs48", "opacity", "scaling", "rotation"}
    for k, v in from_ply.items():
        assert from_npz[k].shape == v.shape and from_npz[k].dtype == v.dtype == torch.float32, k
        assert from_npz[k].is_contiguous() and not from_npz[k].is_cuda
    assert torch.equal(from_ply["xyz"], torch.from_numpy(srt["xyz"]))  # .ply still goes to load_ply
    want = compress.decompress(arrays, meta)
    assert all(torch.equal(from_npz[k], want[k]) for k in want)
    with pytest.raises(ValueError, match="a .ply or a compressed .npz"):
        io_ply.load_model(str(tmp_path / "m.bin"))
    # render_trajectory._find_ply: a model file is passed through, a directory still resolves to its .ply
    from clm_gs_amd.render_trajectory import _find_ply
    assert _find_ply(path, -1) == path and _find_ply(ply, -1) == ply
    os.makedirs(tmp_path / "model" / "point_cloud" / "iteration_30")
    os.makedirs(tmp_path / "model" / "point_cloud" / "iteration_7")
    assert _find_ply(str(tmp_path / "model"), -1) == str(tmp_path / "model" / "point_cloud" / "iteration_30" / "point_cloud.ply")


def test_unknown_version_and_other_sh_degrees_are_refused_by_name(tmp_path):
    from clm_gs_amd import compress
    rows = _rows(50, seed=3)
    srt, arrays, meta, cb, idx = _encode(rows, K=4)
    path = str(tmp_path / "future.vq.npz")
    with open(path, "wb") as f:
        np.savez_compressed(f, meta=np.array(json.dumps(dict(meta, version=99))), **arrays)
    with pytest.raises(ValueError, match="format version 99 is unknown"):
        compress.load_compressed(path)
    with pytest.raises(ValueError, match="format version 99 is unknown"):
        compress.save_compressed(str(tmp_path / "x.npz"), arrays, dict(meta, version=99))
    deg2 = dict(srt, shs48=srt["shs48"][:, :27])
    with pytest.raises(ValueError, match="SH degree 3 only"):
        compress.encode(deg2, idx, cb)
    with pytest.raises(ValueError, match="SH degree 3 only"):
        compress.compress({k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in deg2.items()})
    with pytest.raises(ValueError, match="SH degree 2 is not supported"):
        compress.decompress(arrays, dict(meta, sh_degree=2))
    with pytest.raises(ValueError, match="pos_bits must be an integer in"):
        compress.encode(srt, idx, cb, dict(pos_bits=17))
    with pytest.raises(ValueError, match="unknown bit width"):
        compress.encode(srt, idx, cb, dict(colour_bits=8))


# zip: per member a 30-byte local header and a 46-byte central entry, each with the member's name ("<array>.npy",
# at most 16 characters here), optional 20-byte zip64 extras on both, a 22-byte end record; numpy's own .npy header is
# at most 128 bytes per array at these shapes; deflate's stored-block fallback adds 5 bytes per 65535 bytes of input
ZIP_OVERHEAD_PER_ARRAY = 30 + 46 + 2 * 16 + 2 * 20 + 128
ZIP_END = 22


@pytest.mark.parametrize("n,K,bits", [(1000, 16, None), (257, 5, dict(pos_bits=8, scale_bits=12, rot_bits=16)), (1, 1, None)])
def test_size_is_the_formula(tmp_path, n, K, bits):
    """Sum of nbytes = N (3 w(pos) + 3 w(scale) + w(opacity) + 3 w(rot) + 3 w(dc) + 1 + 2) + ceil(N / chunk) 2 (12 + 12)
    + (2 + 6) 4 + K 45 4, with w(b) = 1 byte up to 8 bits and 2 above: the codes, one byte for the index of the largest
    quaternion component, the uint16 SH index; float32 min and max per axis and chunk for positions and log-scales; the
    global bounds of opacity (2) and DC (2 x 3); the codebook.  On disk: no more than that plus the zip overhead per
    array stated above (incompressible data is stored, not grown) plus the meta string."""
    from clm_gs_amd import compress
    rows = _rows(n, seed=n + K)
    srt, arrays, meta, _, _ = _encode(rows, K=K, bits=bits)
    full = dict(R.BITS, **(bits or {}))
    w = lambda b: 1 if full[b] <= 8 else 2
    chunks = -(-n // 256)
    want = (n * (3 * w("pos_bits") + 3 * w("scale_bits") + w("opacity_bits") + 3 * w("rot_bits") + 3 * w("dc_bits") + 1 + 2)
            + chunks * 2 * (12 + 12) + (2 + 6) * 4 + K * 45 * 4)
    total = sum(a.nbytes for a in arrays.values())
    assert total == want == compress.expected_nbytes(meta)
    assert meta["N"] == n and meta["K"] == K and meta["chunk"] == 256 and meta["version"] == 1
    path = str(tmp_path / "m.vq.npz")
    compress.save_compressed(path, arrays, meta)
    meta_bytes = 4 * len(json.dumps(meta))  # numpy stores the string as UCS-4
    stored_blocks = sum(5 * (1 + a.nbytes // 65535) for a in arrays.values())
    assert os.path.getsize(path) <= total + (len(arrays) + 1) * ZIP_OVERHEAD_PER_ARRAY + ZIP_END + meta_bytes + stored_blocks


def test_reference_pipeline_is_lossless_with_enough_centroids():
    """K >= the number of distinct SH-rest rows, and the even-stride start meets every one of them (rows alike are
    neighbours, as in a Z-ordered table): the reference pipeline gives the SH-rest rows back exactly."""
    g = np.random.default_rng(0)
    distinct = (g.standard_normal((32, 48)) * 0.2).astype(np.float32)
    n = 32 * 24
    rows = {k: v.numpy() for k, v in _rows(n, seed=9).items()}
    rows["xyz"][:, 0] = np.arange(n) * 0.5  # Morton order = row order
    rows["xyz"][:, 1] = 0.0
    rows["shs48"][:, 3:] = np.repeat(distinct, 24, axis=0)[:, 3:]
    out, order, cb, idx = R.pipeline64(rows, 32, 3)
    assert np.array_equal(order, np.arange(n))
    assert np.array_equal(out["shs48"][:, 3:].view(np.int32), rows["shs48"][:, 3:].view(np.int32))
    _, hist = R.fit_codebook64(rows["shs48"], 32, 3)
    assert hist == [0.0, 0.0, 0.0]
    R.check_round_trip(rows, out)
    # and more centroids than rows: K is clamped to the rows
    cb2, _ = R.fit_codebook64(rows["shs48"][:10], 64, 1)
    assert cb2.shape == (10, 48)


def test_reference_update_and_scale_definitions():
    """update_int on a case small enough to do by hand; vq_scale keeps N * max|x| * scale below 2^62 and agrees with the
    operator's."""
    from clm_gs_amd import clm_kernels as CK
    x = np.zeros((3, 48), np.float32)
    x[:, 3] = [1.0, 2.0, 4.0]
    x[:, 47] = [0.5, -0.25, 8.0]
    x[:, 0] = 99.0
    cb = np.full((3, 48), 7.0, np.float32)
    out, counts = R.update_int(x, np.array([0, 0, 2]), cb, 4.0)
    assert list(counts) == [2, 0, 1]
    assert out[0, 3] == 1.5 and out[0, 47] == 0.125 and out[2, 3] == 4.0 and out[2, 47] == 8.0
    assert (out[1, 3:] == 7.0).all() and not out[:, :3].any() and not out[0, 4:47].any()
    for n, m in ((1, 1.0), (1000, 0.3), (1 << 22, 5.0), (28_000_000, 1e-3), (7, 3e38), (5, 0.0)):
        s = R.vq_scale(n, m)
        assert s == CK.vq_scale(n, m) and np.frexp(s)[0] == 0.5
        assert n * m * s < 2.0 ** 62 and (m == 0.0 or n * m * s >= 2.0 ** 60)


def test_trainer_options_and_refusals(tmp_path):
    """--compress and its knobs are in default_args and OPTIONS, off by default; a bad knob is refused by check_training
    before anything is loaded, and is not looked at when --compress is off."""
    from clm_gs_amd import trainer, utils
    a = utils.default_args()
    assert a.compress is False and a.compress_codebook == 65536 and a.compress_iters == 10 and a.compress_sample == 1 << 22
    assert [getattr(a, "compress_" + b) for b in R.BITS] == list(R.BITS.values())
    ns = trainer.build_arg_parser().parse_args(["-s", "x", "-m", "y"])
    assert trainer.train_kwargs(ns)["compress"] is False
    ns = trainer.build_arg_parser().parse_args(["-s", "x", "-m", "y", "--compress", "--compress_codebook", "4096",
                                                "--compress_pos_bits", "12", "--compress_iters", "3"])
    kw = trainer.train_kwargs(ns)
    assert kw["compress"] is True and kw["compress_codebook"] == 4096 and kw["compress_pos_bits"] == 12
    assert kw["compress_iters"] == 3 and kw["compress_dc_bits"] == 8
    for bad, match in ((dict(compress_pos_bits=17), "pos_bits must be an integer in"),
                       (dict(compress_codebook=65537), "compress_codebook must be in"),
                       (dict(compress_codebook=0), "compress_codebook must be in"),
                       (dict(compress_sample=0), "compress_sample"), (dict(sh_degree=2), "SH degrees other than 3")):
        with pytest.raises(ValueError, match=match):
            trainer.train_from_colmap(str(tmp_path / "no_such_scene"), str(tmp_path / "out"), compress=True, **bad)
        trainer.check_training(utils.default_args(clm_offload=True, **bad))  # not asked for: not looked at
    assert not (tmp_path / "out").exists()
