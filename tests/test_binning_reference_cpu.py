"""CPU-only: oracle.gs_oracle.isect_two_level_lists (the vectorised restatement of the two-level binning chain that
tests/test_gpu_ops.py holds the library to) against the looped oracle isect_tiles + isect_offset_encode."""
import math

import pytest
import torch

from oracle import gs_oracle as O


def _scene(n, w, h, seed):
    """Whole-image boxes, a run of culled rows, boxes clipped to nothing, exact depth ties."""
    g = torch.Generator().manual_seed(seed)
    m2 = torch.rand(1, n, 2, generator=g) * torch.tensor([w * 1.4, h * 1.4]) - torch.tensor([w * 0.2, h * 0.2])
    radii = torch.randint(1, 40, (1, n), generator=g, dtype=torch.int32)
    radii[0, :5] = 3000
    radii[0, 50:200] = 0
    m2[0, 400:460] = torch.tensor([-500.0, -500.0])
    d = torch.rand(1, n, generator=g) * 50 + 1
    d[0, 300:340] = 7.0
    d[0, 100] = 7.0  # a culled row inside the tie
    return m2, radii, d, math.ceil(w / 16), math.ceil(h / 16), g


@pytest.mark.parametrize("n,wh", [(900, (70, 37)), (4000, (160, 128))])
def test_two_level_reference_equals_looped_oracle(n, wh):
    m2, radii, d, tw, th, g = _scene(n, wh[0], wh[1], seed=3)
    _, ids, fids = O.isect_tiles(m2, radii, d, 16, tw, th)
    off = O.isect_offset_encode(ids, 1, tw, th)
    R = O.isect_two_level_lists(m2, radii, d, tw, th)
    I = fids.numel()
    assert I > 4 * n
    assert torch.equal(R["flatten_ids"], fids) and torch.equal(R["isect_ids"], ids) and torch.equal(R["offsets"], off)
    assert int(R["totals"][0]) == int(R["row_cum"][-1]) == int(R["cum"][-1]) == I == int(R["totals"][1])
    assert torch.equal(torch.sort(R["emit_slot"].long()).values, torch.arange(I))
    # order: culled rows last, depth ties in row order
    order = R["order"].long()
    n_alive = int((radii > 0).sum())
    assert bool((radii[0, order[:n_alive]] > 0).all()) and bool((radii[0, order[n_alive:]] <= 0).all())
    dk = d[0, order[:n_alive]]
    assert bool((dk[1:] >= dk[:-1]).all())
    tie = order[:n_alive][dk == 7.0]
    assert tie.numel() == 40 and bool((tie[1:] > tie[:-1]).all())
    # the slot of an entry: its place in the (row, tile row-major) list -> ascending inside each row's range
    row_start = R["row_cum"] - torch.diff(R["row_cum"], prepend=torch.zeros(1, dtype=torch.int64))
    s, f = R["emit_slot"].long(), R["flatten_ids"].long()
    assert bool((s >= row_start[f]).all()) and bool((s < R["row_cum"][f]).all())

    # capacity below the count: the tile-sorted form of the first `capacity` emitted entries
    cap = int(I * 0.6)
    Rc = O.isect_two_level_lists(m2, radii, d, tw, th, capacity=cap)
    for nm in ("order", "cum", "boxes", "totals", "row_cum"):
        assert torch.equal(Rc[nm], R[nm]), nm
    rank = torch.empty(n, dtype=torch.int64)
    rank[order] = torch.arange(n)
    tiles = R["isect_ids"] >> 32
    # emit position of every entry of the full list: entries of earlier ranks + its place inside its row
    emit_pos = (R["cum"] - torch.diff(R["cum"], prepend=torch.zeros(1, dtype=torch.int64)))[rank[f]] + s - row_start[f]
    assert torch.equal(torch.sort(emit_pos).values, torch.arange(I))
    first = emit_pos < cap  # the full list is tile-sorted and stable, so a mask of it is the sorted prefix
    assert Rc["flatten_ids"].numel() == cap
    assert torch.equal(Rc["flatten_ids"], R["flatten_ids"][first]) and torch.equal(Rc["emit_slot"], R["emit_slot"][first])
    assert torch.equal(Rc["isect_ids"], R["isect_ids"][first])
    assert torch.equal(Rc["offsets"].reshape(-1).long(), torch.searchsorted(tiles[first].contiguous(), torch.arange(tw * th)))

    # random mask words: the un-culled total stays, the emitted total drops, big boxes are not masked
    mk = torch.randint(-2**62, 2**62, (n,), generator=g, dtype=torch.int64)
    Rm = O.isect_two_level_lists(m2, radii, d, tw, th, masks=mk)
    Im = int(Rm["totals"][0])
    assert int(Rm["totals"][1]) == int(R["totals"][1]) and Im < I
    assert Im == Rm["flatten_ids"].numel() == int(Rm["row_cum"][-1]) == int(Rm["cum"][-1])
    assert torch.equal(Rm["order"], R["order"])
    assert torch.equal(torch.sort(Rm["emit_slot"].long()).values, torch.arange(Im))
    per_row = torch.diff(R["row_cum"], prepend=torch.zeros(1, dtype=torch.int64))
    per_row_m = torch.diff(Rm["row_cum"], prepend=torch.zeros(1, dtype=torch.int64))
    big = per_row > 64
    assert bool(big.any()) == (tw * th > 64) and torch.equal(per_row_m[big], per_row[big])  # (the larger image has them)
    small = ~big
    want = torch.tensor([bin(v & ((1 << k) - 1)).count("1") for v, k in zip(mk[small].tolist(), per_row[small].tolist())])
    assert torch.equal(per_row_m[small], torch.where(radii[0, small] > 0, want, torch.zeros_like(want)))
    # the masked list is a sub-list of the full one, in the same order
    keys_full = R["isect_ids"].tolist()
    sub = set(zip(Rm["isect_ids"].tolist(), Rm["flatten_ids"].tolist()))
    assert len(sub) == Im and sub <= set(zip(keys_full, R["flatten_ids"].tolist()))
    assert bool((Rm["isect_ids"][1:] >= Rm["isect_ids"][:-1]).all())
    # boxes: zero where nothing is emitted, the mask word as given (all ones on culled rows)
    b = Rm["boxes"]
    emitted = per_row_m[order] > 0
    assert bool((b[~emitted, 0] == 0).all()) and bool((b[emitted, 0] != 0).all())
    assert torch.equal(b[:, 1], torch.where(radii[0] > 0, mk, torch.full_like(mk, -1))[order])
