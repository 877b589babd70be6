"""CPU-only: the 4-channel (depth) rasterizer is part of the C ABI and of the operator's contract.

The library exports clmgs_rasterize4_fwd / clmgs_rasterize4_bwd and the binding table lists them; the operator takes
3 or 4 colour channels and nothing else, and has no CPU fallback for either."""
import ctypes

import numpy as np
import pytest
import torch

NEW_SYMBOLS = ("clmgs_rasterize4_fwd", "clmgs_rasterize4_bwd")


def test_library_exports_the_four_channel_entries():
    from clm_gs_amd import _lib
    l = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert name in _lib.SIGNATURES, name
        assert hasattr(l, name), name
    # same argument lists as the 3-channel neighbours (rows of four instead of three, nothing else)
    assert _lib.SIGNATURES["clmgs_rasterize4_fwd"] == _lib.SIGNATURES["clmgs_rasterize_fwd"]
    assert _lib.SIGNATURES["clmgs_rasterize4_bwd"] == _lib.SIGNATURES["clmgs_rasterize_bwd"]


def _cpu_inputs(nch):
    n = 5
    return (torch.zeros(1, n, 2), torch.ones(1, n, 3), torch.zeros(1, n, nch), torch.ones(1, n), 16, 16, 16,
            torch.zeros(1, 1, 1, dtype=torch.int32), torch.zeros(0, dtype=torch.int32))


@pytest.mark.parametrize("nch", [1, 2, 5])
def test_other_channel_counts_are_not_implemented(nch):
    from clm_gs_amd import gsplat
    with pytest.raises(NotImplementedError):
        gsplat.rasterize_to_pixels(*_cpu_inputs(nch))


@pytest.mark.parametrize("nch", [3, 4])
def test_no_cpu_fallback(nch):
    """CPU tensors reach the library's pointer check (no eager path): an error, and not NotImplementedError."""
    from clm_gs_amd import gsplat
    with pytest.raises(Exception) as e:
        gsplat.rasterize_to_pixels(*_cpu_inputs(nch))
    assert not isinstance(e.value, NotImplementedError), e.value


def test_backgrounds_follow_the_channel_count():
    from clm_gs_amd import gsplat
    with pytest.raises(ValueError):
        gsplat.rasterize_to_pixels(*_cpu_inputs(4), backgrounds=torch.zeros(3))
    with pytest.raises(ValueError):
        gsplat.rasterize_to_pixels(*_cpu_inputs(3), backgrounds=torch.zeros(1, 4))


def test_render_mode_helpers():
    from clm_gs_amd.strategies.base_engine import colors_with_depth, split_depth
    col, z, bg = torch.rand(1, 7, 3), torch.rand(1, 7) + 1, torch.tensor([[0.1, 0.2, 0.3]])
    c, b = colors_with_depth(col, z, bg, "RGB")
    assert c is col and b is bg
    c, b = colors_with_depth(col, z, bg, "RGB+D")
    assert torch.equal(c[..., :3], col) and torch.equal(c[..., 3], z) and torch.equal(b, torch.tensor([[0.1, 0.2, 0.3, 0.0]]))
    c, b = colors_with_depth(col, z, torch.tensor([0.1, 0.2, 0.3]), "RGB+ED")  # the 1-D form of the no_offload engine
    assert b.shape == (4,) and float(b[3]) == 0.0
    assert colors_with_depth(col, z, None, "RGB+ED")[1] is None
    with pytest.raises(ValueError):
        colors_with_depth(col, z, bg, "D")
    out = torch.rand(1, 4, 5, 4)
    al = torch.tensor([0.0, 0.5, 1.0, 0.25, 1e-12]).expand(1, 4, 5)[..., None].contiguous()
    out[..., 3] = out[..., 3] * (al[..., 0] > 0)
    img, d, a = split_depth(out, al, "RGB+D")
    assert img.shape == (3, 4, 5) and torch.equal(d, out[..., 3]) and torch.equal(a, al[..., 0])
    _, ed, _ = split_depth(out, al, "RGB+ED")
    assert torch.equal(ed, out[..., 3] / al[..., 0].clamp(min=1e-10)) and float(ed[0, :, 0].abs().max()) == 0.0


def test_depth_to_grey_uses_the_masked_range():
    from clm_gs_amd.render_trajectory import depth_to_grey
    d = np.array([[0.0, 2.0, 4.0], [3.0, 100.0, 2.5]], dtype=np.float32)
    mask = np.array([[False, True, True], [True, False, True]])
    g = depth_to_grey(d, mask)  # range 2 .. 4 from the masked pixels; the others are clipped to it
    assert g.shape == (2, 3, 3) and g.dtype == np.uint8 and (g[..., 0] == g[..., 1]).all() and (g[..., 0] == g[..., 2]).all()
    assert g[0, 0, 0] == 0 and g[0, 1, 0] == 0 and g[0, 2, 0] == 255 and g[1, 1, 0] == 255 and g[1, 0, 0] == 127
    assert int(depth_to_grey(np.full((2, 2), 3.0, dtype=np.float32), np.ones((2, 2), bool)).max()) == 0
    assert depth_to_grey(d, np.zeros_like(mask))[1, 1, 0] == 255  # empty mask: the whole map's range
