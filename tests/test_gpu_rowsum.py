"""-m gpu: the summation order of csrc/rowsum.h itself ("Row sums"), bit for bit, through the C ABI.
rows_finish_kernel<COLS, PITCH, ADD> sums a table of `rows` partial rows with one wave: lane COLS * slice + j takes the rows
slice, slice + 64 / COLS, ... of column j in ascending order (eight loads in flight, added one at a time, which is simply
ascending), the slices are joined by the xor tree COLS, 2 COLS, ... 32.  Plain float32 additions are IEEE on both sides, so
a numpy float32 emulation of that order must equal the device result in every bit: no tolerance."""
import ctypes
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def _p(t):
    return ctypes.c_void_p(t.data_ptr())


@functools.lru_cache(maxsize=None)
def _table(rows, pitch):
    """float32 [rows, pitch] with magnitudes spread over 2^-12 .. 2^12: a different order of additions shows in the bits."""
    rng = np.random.default_rng(0)
    t = rng.standard_normal((rows, pitch)) * 2.0 ** rng.integers(-12, 13, (rows, pitch))
    t = t.astype(np.float32)
    t.setflags(write=False)
    return t


def _emulate(table, cols):
    """The documented order on a float32 [rows, pitch] table -> float32 [pitch]: what lane j < pitch of slice 0 holds."""
    rows, pitch = table.shape
    slices = 64 // cols
    acc = np.zeros((slices, pitch), np.float32)
    for s in range(slices):
        for r in range(s, rows, slices):
            acc[s] = acc[s] + table[r]
    o = cols
    while o < 64:  # acc += __shfl_xor(acc, o): lane COLS * s + j meets lane COLS * (s ^ (o / COLS)) + j
        acc = acc + acc[np.arange(slices) ^ (o // cols)]
        o <<= 1
    assert acc.dtype == np.float32
    return acc[0]


def _ascending(table):
    acc = np.zeros(table.shape[1], np.float32)
    for r in range(table.shape[0]):
        acc = acc + table[r]
    return acc


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _dev(a, dev, min_rows=1):
    """The table on the device; at least one row is allocated so that rows = 0 still passes a pointer."""
    t = torch.zeros((max(a.shape[0], min_rows),) + a.shape[1:], dtype=torch.float32, device=dev)
    t[: a.shape[0]] = torch.from_numpy(np.array(a))
    return t


def test_the_inputs_tell_the_orders_apart():
    """A condition on the test's own inputs: the plain ascending sum and the emulated order differ, so the comparisons
    below cannot pass vacuously.  (Needs no device.)"""
    for rows, pitch, cols in ((100, 12, 16), (100, 16, 16), (1000, 1, 1)):
        t = _table(rows, pitch)
        n = int((_bits(_ascending(t)) != _bits(_emulate(t, cols))).sum())
        print(f"rows {rows} pitch {pitch}: ascending sum differs from the emulated order in {n} of {pitch} elements")
        assert n >= 1


@pytest.mark.parametrize("rows", [0, 1, 2, 3, 4, 5, 28, 29, 32, 33, 36, 37, 100])
def test_exposure_grad_finish(dev, rows):
    """[rows, 12], four slices: the unrolled loop's condition r + 28 < rows flips inside 29..36.  The entry ADDS: once onto
    zeros, once onto a row that is not zero."""
    from clm_gs_amd import _lib
    t = _table(rows, 12)
    want = _emulate(t, 16)
    partials = _dev(t, dev)
    row0 = _table(1, 12)[0] * np.float32(3.0)
    for start in (np.zeros(12, np.float32), row0):
        grad = torch.from_numpy(start.copy()).to(dev)
        _lib.check(_lib.lib().clmgs_exposure_grad_finish(_lib.stream(), rows, _p(partials), _p(grad)))
        got = grad.cpu().numpy()
        assert np.array_equal(_bits(got), _bits(start + want)), (rows, got, start + want)


@pytest.mark.parametrize("rows", [0, 1, 4, 5, 29, 32, 33, 100])
def test_pose_grad_finish(dev, rows):
    """[rows, 16], 15 words out: word 15 of the gradient buffer is not touched; rows = 0 returns without a launch."""
    from clm_gs_amd import _lib
    t = _table(rows, 16)
    want = _emulate(t, 16)
    partials = _dev(t, dev)
    start = _table(1, 16)[0] * np.float32(3.0)
    grad = torch.from_numpy(start.copy()).to(dev)
    _lib.check(_lib.lib().clmgs_pose_grad_finish(_lib.stream(), rows, _p(partials), _p(grad)))
    got = grad.cpu().numpy()
    assert np.array_equal(_bits(got[:15]), _bits((start + want)[:15])), (rows, got, start + want)
    assert _bits(got[15:])[0] == _bits(start[15:])[0]


@pytest.mark.parametrize("rows", [0, 1, 63, 64, 65, 448, 449, 511, 512, 513, 1000])
def test_invdepth_finish(dev, rows):
    """[rows], one column, 64 slices, the ascending six-step tree: the unrolled loop's condition is r + 448 < rows.  The
    entry STORES (rows = 0: a zero)."""
    from clm_gs_amd import _lib
    t = _table(rows, 1)
    want = _emulate(t, 1)
    partials = _dev(t, dev)
    out = torch.full((2,), float("nan"), device=dev)
    _lib.check(_lib.lib().clmgs_invdepth_finish(_lib.stream(), rows, _p(partials), _p(out)))
    got = out.cpu().numpy()
    assert _bits(got[:1])[0] == _bits(want)[0], (rows, got, want)
    assert np.isnan(got[1])


def test_projection_viewmat_bwd_finishes_per_camera(dev):
    """The store form, one block per camera: C = 2 cameras, N = 300 Gaussians (two partial rows per camera).  The partial
    rows the entry left are finished again on the host by the emulation: per-camera offset, 12 words out, words 12..15
    stored as zeros."""
    from clm_gs_amd import _lib
    L = _lib.lib()
    C, N, W, H = 2, 300, 64, 48
    gen = torch.Generator().manual_seed(0)
    means = torch.cat([torch.rand(N, 2, generator=gen) * 2 - 1, torch.rand(N, 1, generator=gen) * 4 + 2], dim=1)
    quats = torch.nn.functional.normalize(torch.randn(N, 4, generator=gen), dim=1)
    scales = torch.rand(N, 3, generator=gen) * 0.2 + 0.05
    viewmats = torch.eye(4).repeat(C, 1, 1)
    viewmats[1, 0, 3] = 0.25
    Ks = torch.tensor([[50.0, 0, W / 2], [0, 50.0, H / 2], [0, 0, 1]]).repeat(C, 1, 1)
    radii = torch.full((C, N), 3, dtype=torch.int32)
    radii[:, ::7] = 0  # culled rows are skipped
    v_means2d, v_conics = torch.randn(C, N, 2, generator=gen), torch.randn(C, N, 3, generator=gen)
    d = [t.contiguous().to(dev) for t in (means, quats, scales, viewmats, Ks, radii, v_means2d, v_conics)]
    rows = int(L.clmgs_projection_viewmat_partials_rows(N))
    assert rows == 2
    partials = torch.full((C * rows, 16), float("nan"), device=dev)
    out = torch.full((C, 16), float("nan"), device=dev)
    _lib.check(L.clmgs_projection_viewmat_bwd(_lib.stream(), C, N, _p(d[0]), _p(d[1]), _p(d[2]), _p(d[3]), _p(d[4]), W, H, 0.3,
                                              _p(d[5]), _p(d[6]), None, _p(d[7]), None, _p(partials), _p(out)))
    tables, got = partials.cpu().numpy().reshape(C, rows, 16), out.cpu().numpy()
    assert np.isfinite(tables).all() and (tables[:, :, :12] != 0).any(axis=(1, 2)).all()
    assert not (tables[:, :, 12:] != 0).any(), "the pad words of a partial row are zeros"
    for c in range(C):
        want = _emulate(tables[c], 16)
        want[12:] = 0.0
        assert np.array_equal(_bits(got[c]), _bits(want)), (c, got[c], want)
    assert not np.array_equal(_bits(got[0]), _bits(got[1]))
