"""CPU-only: tests/front_end_reference.py, the float64 reference of the fused front end, held to independent computations
-- the oracle's projection + SH, the existing antialias reference, central differences -- and the conditions its scenes
promise to tests/test_gpu_front_end.py (no row within the margins of a float32 decision; the special rows are what their
names say)."""
import os

import numpy as np
import pytest
import torch

from oracle import gs_oracle as O
from tests import antialias_reference as R
from tests import front_end_reference as FR
from tests.scenes import rel_l2

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F64 = torch.float64
S = FR.SPECIAL
# about eight rows per degree: ordinary ones and every special row
FD_ROWS = torch.tensor([0, 3, S["clamped_tx"][0], S["clamped_tx"][1], S["dark"], S["one_channel"], S["behind"], S["far"], S["tiny"],
                        S["off_screen"]])


def _lines(V, seed):
    g = torch.Generator().manual_seed(seed)
    pg = torch.randn(V, 16, generator=g)
    pg[:, 9:] = float("nan")  # not read by the reference
    return pg


@pytest.mark.parametrize("deg", [0, 1, 2, 3])
def test_plain_forward_is_the_oracles_composition(deg):
    raw, cam = FR.scene()
    rows = torch.randperm(400, generator=torch.Generator().manual_seed(deg))[:333]
    for name, cull in FR.CULLS.items():
        ref = FR.reference(raw, rows, cam, deg, False, **cull)
        with torch.no_grad():
            xyz = raw["xyz"].double()[rows]
            r, m2, d, cn, _ = O.fully_fused_projection(xyz, None, raw["rotation"].double()[rows], torch.exp(raw["scaling"].double()[rows]),
                                                       cam["viewmat"].double()[None], cam["K"].double()[None], cam["width"],
                                                       cam["height"], **cull)
            dirs = xyz[None] - FR.campos_of(cam["viewmat"])
            col = torch.clamp_min(O.spherical_harmonics(deg, dirs, raw["shs"].double()[rows].reshape(1, -1, 16, 3), masks=r > 0) + 0.5, 0.0)
            op = torch.sigmoid(raw["opacity"].double()[rows])
        assert torch.equal(ref["radii"], r[0]), name
        vis = r[0] > 0
        assert bool(vis.any()) and not bool(vis.all())
        for k, want in (("m2", m2[0]), ("dep", d[0]), ("cn", cn[0]), ("col", col[0]), ("op", op)):
            e = float((ref[k] - want).abs().max())
            assert e < 1e-12, (name, k, e)
        assert float(ref["col"][~vis].sub(0.5).abs().max()) == 0.0  # masked SH + 0.5: the kernel writes 0 there instead


@pytest.mark.parametrize("deg", [0, 3])
def test_antialiased_forward_and_gradients_are_the_antialias_references(deg):
    """aa=True against the composition tests/test_gpu_antialias.py used before it imported this helper, written out here."""
    raw, cam = FR.scene()
    rows = torch.randperm(400, generator=torch.Generator().manual_seed(5))[:200]
    pg = _lines(200, 3)
    ref = FR.reference(raw, rows, cam, deg, True, lines=pg)
    P = {k: v.double().clone().requires_grad_() for k, v in raw.items()}
    xyz = P["xyz"][rows]
    radii, m2, d, cn, comp = R.projection(xyz, P["rotation"][rows], torch.exp(P["scaling"][rows]), cam["viewmat"].double()[None],
                                          cam["K"].double()[None], cam["width"], cam["height"])
    dirs = xyz[None] - torch.inverse(cam["viewmat"].double())[:3, 3]
    col = torch.clamp_min(O.spherical_harmonics(deg, dirs, P["shs"][rows].reshape(1, -1, 16, 3), masks=radii > 0) + 0.5, 0.0)
    op = torch.sigmoid(P["opacity"][rows])[None] * comp
    g = pg.double()
    ((m2[0] * g[:, 0:2]).sum() + (cn[0] * g[:, 2:5]).sum() + (col[0] * g[:, 5:8]).sum() + (op[0] * g[:, 8]).sum()).backward()
    assert torch.equal(ref["radii"], radii[0])
    assert torch.equal(ref["op"], op[0].detach()) and torch.equal(ref["comp"], comp[0].detach()) and torch.equal(ref["col"], col[0].detach())
    assert float(ref["op"][radii[0] == 0].abs().max()) == 0.0
    for k in FR.GROUPS:
        assert torch.equal(ref["grads"][k], P[k].grad if P[k].grad is not None else torch.zeros_like(P[k])), k
    # and the plain entry differs from it in the opacity and in the scale gradient only through the compensation
    plain = FR.reference(raw, rows, cam, deg, False, lines=pg)
    vis = radii[0] > 0
    assert torch.allclose(plain["op"][vis] * ref["comp"][vis], ref["op"][vis], rtol=1e-14, atol=0)
    assert rel_l2(plain["grads"]["scaling"], ref["grads"]["scaling"]) > 1e-3
    assert torch.equal(plain["grads"]["shs"], ref["grads"]["shs"])


def _scalar(raw, rows, cam, deg, aa, g):
    """sum over rows of <outputs, lines>, float64, no autograd: what reference()'s gradients differentiate."""
    with torch.no_grad():
        o = FR.reference(raw, rows, cam, deg, aa)
    vis = (o["radii"] > 0).double()
    # per row, so that one perturbed column of every row is read off in one evaluation (the rows are independent)
    return (o["m2"] * g[:, 0:2]).sum(1) + (o["cn"] * g[:, 2:5]).sum(1) + (o["col"] * g[:, 5:8]).sum(1) + o["op"] * vis * g[:, 8]


@pytest.mark.parametrize("aa", [False, True])
@pytest.mark.parametrize("deg", [0, 1, 2, 3])
def test_gradients_against_central_differences(deg, aa):
    """h = 1e-5 in float64: truncation h^2 f''' / 6 and rounding 1e-16 / h are both near 1e-10 of the derivative, the bound
    1e-6 leaves four orders for the third derivatives of exp and of the conic's 1 / det.  The antialiased entry is
    differentiated with the plain square root (guarded=False); the guarded form gsplat uses, 0.5 / (c + 1e-6) for
    0.5 / c, is then within 1e-6 / min(c) of it."""
    raw0, cam = FR.scene()
    raw = {k: v.double() for k, v in raw0.items()}
    rows, V, h = FD_ROWS, FD_ROWS.numel(), 1e-5
    pg = _lines(V, 20 + deg)
    g = pg.double()
    ref = FR.reference(raw, rows, cam, deg, aa, lines=pg, guarded=False)
    vis = ref["radii"] > 0
    assert int(vis.sum()) == V - 2  # the row behind the camera and the one off screen
    worst = 0.0
    for k in FR.GROUPS:
        base = raw[k].reshape(400, -1)
        fd = torch.zeros(V, base.shape[1], dtype=F64)
        for c in range(base.shape[1]):
            vals = []
            for sgn in (1.0, -1.0):
                p = base.clone()
                p[rows, c] += sgn * h
                vals.append(_scalar({**raw, k: p.reshape(raw[k].shape)}, rows, cam, deg, aa, g))
            fd[:, c] = (vals[0] - vals[1]) / (2 * h)
        got = ref["grads"][k].reshape(400, -1)[rows]
        assert float(got[~vis].abs().max()) == 0.0 and float(fd[~vis].abs().max()) == 0.0, k
        if k == "shs":
            nb3 = 3 * (deg + 1) ** 2
            assert float(got[:, nb3:].abs().sum()) == 0.0 and float(fd[:, nb3:].abs().sum()) == 0.0
            dark = list(rows.tolist()).index(S["dark"])
            assert float(got[dark].abs().max()) == 0.0  # every channel clamped: nothing reaches the coefficients
            one = list(rows.tolist()).index(S["one_channel"])
            assert float(got[one, 0::3].abs().max()) == 0.0 and float(got[one, 1].abs()) > 0
        e = rel_l2(got, fd)
        worst = max(worst, e)
        assert e < 1e-6, (k, e)
        untouched = torch.ones(400, dtype=torch.bool)
        untouched[rows] = False
        assert float(ref["grads"][k][untouched].abs().max()) == 0.0, k
    print(f"deg={deg} aa={aa}: worst rel_l2 against central differences {worst:.3g}")
    if aa:
        guarded = FR.reference(raw, rows, cam, deg, True, lines=pg)
        e = rel_l2(guarded["grads"]["scaling"], ref["grads"]["scaling"])
        assert 0 < e < 1e-6 / float(ref["comp"][vis].min()), e


def test_float32_reference_runs():
    """dtype=float32 is what the GPU tests measure the formulas' own float32 error with."""
    raw, cam = FR.scene()
    pg = _lines(400, 1)
    a, b = FR.reference(raw, None, cam, 3, False, lines=pg), FR.reference(raw, None, cam, 3, False, lines=pg, dtype=torch.float32)
    assert b["grads"]["xyz"].dtype == torch.float32 and torch.equal(a["radii"], b["radii"])
    for k in FR.GROUPS:
        assert rel_l2(b["grads"][k], a["grads"][k]) < 2e-4, k


def test_statistics_restatement():
    g = np.random.default_rng(0)
    N, V, W, H = 50, 20, 64, 48
    rows = g.permutation(N)[:V]
    radii = g.integers(0, 4, V)
    lines = g.standard_normal((V, 16))
    old = [g.random(N) * 3, g.random(N), g.integers(0, 5, N).astype(np.float64)]
    for abs_pair in (False, True):
        for only in (False, True):
            mr, ga, dn = FR.statistics(*old, rows, radii, lines, W, H, abs_pair=abs_pair, only_visible=only)
            for j in range(N):  # the same, row by row
                hit = np.nonzero(rows == j)[0]
                on = hit.size == 1 and (radii[hit[0]] > 0 or not only)
                if not on:
                    assert (mr[j], ga[j], dn[j]) == (old[0][j], old[1][j], old[2][j])
                    continue
                i = hit[0]
                gx, gy = (lines[i, 10], lines[i, 11]) if abs_pair else (lines[i, 0], lines[i, 1])
                assert mr[j] == max(old[0][j], radii[i]) and dn[j] == old[2][j] + 1
                assert abs(ga[j] - old[1][j] - np.hypot(gx * W / 2, gy * H / 2)) < 1e-12


def test_scene_conditions():
    """The 400-row scene: no row's 3 sqrt(v1) within 1e-3 of an integer, no cull comparison within 1e-3 of its threshold
    under any of the cull settings the GPU tests run, and the special rows visible / culled as named."""
    raw, cam = FR.scene()
    assert raw["xyz"].shape == (400, 3) and (cam["width"], cam["height"]) == (64, 48)
    out = FR.scene_conditions(raw, cam)
    for cull in FR.CULLS.values():
        m = FR.margins(raw, cam, cull)
        print({k: f"{float(v.min()):.3g}" for k, v in m.items()})
        assert all(float(v.min()) >= FR.MARGIN for v in m.values())
    r = out["default"]["radii"]
    print(f"visible {int((r > 0).sum())} of 400, largest radius {int(r.max())}")
    assert int(r.max()) <= 60  # the margin is sized for radii of tens of pixels
    # the float32 reference takes the same decisions: the margins are wide enough for its own rounding
    for name, cull in FR.CULLS.items():
        r32 = FR.reference(raw, None, cam, 0, False, dtype=torch.float32, **cull)["radii"]
        assert torch.equal(r32, out[name]["radii"]), name


def test_tiled_scene_conditions():
    """The second-chunk case: 64 x cap + 70 unique rows (the cap is clmgs_preprocess_grid_cap, 3072)."""
    V = 64 * 3072 + 70
    raw, cam = FR.tiled_scene(V)
    assert raw["xyz"].shape[0] == V
    assert torch.unique(raw["xyz"], dim=0).shape[0] == V
    assert not bool(FR.violations(raw, cam).any())
    r = FR.reference(raw, None, cam, 0, False)["radii"]
    r32 = FR.reference(raw, None, cam, 0, False, dtype=torch.float32)["radii"]
    assert torch.equal(r, r32)
    tail = r[64 * 3072:]
    assert bool((tail > 0).any()) and not bool((tail > 0).all())


def test_grid_cap_accessor_in_header_table_and_library():
    from clm_gs_amd import _lib
    header = open(os.path.join(ROOT, "include", "clmgs.h")).read()
    assert "clmgs_preprocess_grid_cap(" in header and _lib.SIGNATURES["clmgs_preprocess_grid_cap"][1] == []
    assert "clmgs_preprocess_grid_cap" in _lib._NO_STREAM
    if os.path.exists(_lib.LIB_PATH):  # a host entry: no device needed
        assert int(_lib.lib().clmgs_preprocess_grid_cap()) == 3072
