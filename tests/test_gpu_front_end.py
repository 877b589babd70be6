"""-m gpu: every shipped variant of the fused front end (csrc/preprocess.hip: clmgs_preprocess_fwd / _bwd and their abs /
antialiased entries) through the C ABI, against the float64 reference of tests/front_end_reference.py (which
tests/test_front_end_cpu.py holds to the oracle and to central differences): degrees 0-3, packed and unpacked attribute
tables, the three SH addressings, the [V,16] table and the partial lines + row_cum, accumulation into tables that hold
earlier sums, first-touch stamps, both statistics forms, a second chunk per wave, tables in pinned host memory.

The scene keeps 1e-3 clear of every decision the float32 kernel takes (FR.margins; asserted on the CPU), so radii are
compared exactly.  Bounds are the project's own: gradients rel-L2 < GRAD_TOL = 2e-4 (tests/test_gpu_ops.py); forward as
test_projection_fwd_bwd / test_sh_fwd_bwd: means2d 1e-5 relative to 1 + |x|, depths rel-L2 1e-6, conics rel-L2 1e-5,
colours 1e-5 max-abs; opacity rel-L2 < COMP_TOL = 1e-5 (tests/test_gpu_antialias.py); grad_accum rel-L2 1e-6 (the abs
test).  Every test prints its worst deviation (run with -s)."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from tests import front_end_reference as FR
from tests.scenes import rel_l2
from tests.test_gpu_antialias import COMP_TOL
from tests.test_gpu_ops import GRAD_TOL

pytestmark = pytest.mark.gpu

# TOLERANCES, measured on an MI355X (this file with -s).  Every project bound holds as it stands, so none is replaced by
# the float32 reference's own deviation (the fallback of tests/test_gpu_pose.py::_tolerance is not needed here).
#   forward, 1 .. 400 rows, all variants: means2d 3e-8 .. 2.1e-6 of 1 + |x| (bound 1e-5), depths rel-L2 3.4e-8 .. 4.3e-8
#     (1e-6), conics rel-L2 1.7e-7 .. 3.5e-7 (1e-5), colours max-abs 3e-8 (degree 0) .. 4.0e-7 (degree 3) (1e-5), opacity
#     rel-L2 5.5e-8 .. 7.0e-8 (1e-5); with near_plane / far_plane / radius_clip the same figures, 98 / 121 / 69 rows
#     changing sides; 196 678 rows: means2d 4.1e-6, depths 4.2e-8, conics 2.2e-7, colours 1.7e-7, opacity 3.9e-8
#   gradients, worst group, rel-L2 (bound 2e-4): plain entry into zeroed tables 4.4e-7 .. 9.9e-7 (1.5e-6 for the single
#     row of V = 1 at degree 3); out - init from pre-filled tables 4.6e-7 .. 1.1e-6; partial lines 4.5e-7 .. 7.2e-7 for the
#     four entries; 196 678 rows 5.2e-7 (dropping the rows past 64 x cap moves the reference by 1.5e-2 .. 2.1e-2)
#   grad_accum rel-L2 4.0e-8 .. 5.2e-8 (bound 1e-6); radii, denom, max_radii, stamps and every bit comparison: exact

F32, I32, I64 = torch.float32, torch.int32, torch.int64
N0 = 400
VS = [1, 63, 64, 65, 400]
S = FR.SPECIAL
SPECIAL_ROWS = [S["clamped_tx"][0], S["clamped_tx"][1], S["dark"], S["one_channel"], S["behind"], S["far"], S["tiny"], S["off_screen"]]
ENTRIES = {"plain": ("clmgs_preprocess_fwd", "clmgs_preprocess_bwd", False, False),
           "abs": ("clmgs_preprocess_fwd", "clmgs_preprocess_abs_bwd", True, False),
           "aa": ("clmgs_preprocess_aa_fwd", "clmgs_preprocess_aa_bwd", False, True),
           "aa_abs": ("clmgs_preprocess_aa_fwd", "clmgs_preprocess_aa_abs_bwd", True, True)}
SENT = 777.0


def _npp(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def _bits(t):
    return t.contiguous().view(I32)


def _same(a, b):
    """Bit equality (NaN-safe)."""
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def nf4(deg):
    return (3 * (deg + 1) ** 2 + 3) // 4


@functools.lru_cache(maxsize=None)
def _filter(V, on):
    """The rows of a launch: a shuffled filter that holds the special rows (V >= 63; the one row of V = 1 is clamped in
    tx), or None: rows 0 .. V-1."""
    if not on:
        return None
    if V == 1:
        return torch.tensor([S["clamped_tx"][0]])
    g = torch.Generator().manual_seed(V)
    rest = [r for r in torch.randperm(N0, generator=g).tolist() if r not in SPECIAL_ROWS]
    rows = torch.tensor(SPECIAL_ROWS + rest[:V - len(SPECIAL_ROWS)])
    return rows[torch.randperm(V, generator=g)].contiguous()


def _rows(V, filt):
    return filt if filt is not None else torch.arange(V)


def _lines16(V, seed, abs_pair=False):
    """[V,16] gradient lines  x y ca cb | cc r g b | o - ax ay; the words an entry does not read are NaN."""
    g = torch.Generator().manual_seed(seed)
    pg = torch.randn(V, 16, generator=g)
    pg[:, 9:] = float("nan")
    if abs_pair:
        pg[:, 10:12] = torch.rand(V, 2, generator=g)
    return pg


@functools.lru_cache(maxsize=None)
def _ref(V, filt_on, deg, aa, seed=None, cull="default", dtype=torch.float64):
    raw, cam = FR.scene()
    lines = _lines16(V, seed) if seed is not None else None
    return FR.reference(raw, _rows(V, _filter(V, filt_on)), cam, deg, aa, lines=lines, dtype=dtype, **FR.CULLS[cull])


class _Launch:
    """Device tables of one scene and the camera; fwd() and bwd() call the C ABI as tests/test_gpu_antialias.py::_run_pre."""

    def __init__(self, dev, raw, cam, pk):
        from clm_gs_amd import _lib
        self.L, self.dev, self.pk, self.cam = _lib.lib(), dev, pk, cam
        self.N = raw["xyz"].shape[0]
        d = {k: raw[k].to(dev).contiguous() for k in FR.GROUPS}
        self.shs = d["shs"]
        self.raw = raw
        if pk:
            self.tab = torch.zeros(self.N, 12, device=dev)
            self.tab[:, 0:3], self.tab[:, 3], self.tab[:, 4:7], self.tab[:, 7:11] = d["xyz"], d["opacity"], d["scaling"], d["rotation"]
            self.keep = (self.tab,)
        else:
            self.keep = (d["xyz"], d["opacity"], d["scaling"], d["rotation"])
        self.vmh = np.ascontiguousarray(cam["viewmat"].numpy().astype(np.float32).reshape(16))
        self.Kh = np.ascontiguousarray(cam["K"].numpy().astype(np.float32).reshape(9))
        self.cph = np.ascontiguousarray(FR.campos_of(cam["viewmat"]).numpy().astype(np.float32))

    def small(self):
        from clm_gs_amd._lib import dptr
        return (dptr(self.tab), None, None, None) if self.pk else tuple(dptr(x) for x in self.keep)

    def sh_tables(self, V, filt, sh_mode, host=False):
        """-> (sh table, sh_by_filter, sh_index or None, sid: the row of the SH tables position i uses, table rows)."""
        rows = _rows(V, filt)
        if sh_mode == "by_row":
            return self.shs, 1, None, rows, self.N
        if sh_mode == "by_position":
            return self.shs[rows.to(self.dev)].contiguous(), 0, None, torch.arange(V), V
        perm = torch.randperm(V, generator=torch.Generator().manual_seed(V + 1))
        stage = torch.full((V + 3, 48), float("nan"))  # three rows nothing indexes
        stage[perm] = self.raw["shs"][rows]
        if host:
            from clm_gs_amd.host import pinned_empty
            t = pinned_empty((V + 3, 48))
            t.copy_(stage)
        else:
            t = stage.to(self.dev)
        return t, 1, perm.to(I32).to(self.dev), perm, V + 3

    def fwd(self, V, filt, deg, sh_mode="by_row", entry="plain", full=True, cull="default", host=False):
        from clm_gs_amd._lib import check, dptr, stream
        dev, c = self.dev, FR.CULLS[cull]
        sh, by_filter, sh_index, _, _ = self.sh_tables(V, filt, sh_mode, host)
        fd = filt.to(dev) if filt is not None else None
        nan = float("nan")
        radii = torch.full((V,), -7, dtype=I32, device=dev)
        m2, dep, cn, col, op = (torch.full(s_, nan, device=dev) for s_ in ((V, 2), (V,), (V, 3), (V, 3), (V,)))
        packed = torch.full((V, 16), nan, device=dev)
        opt = (dptr(cn), dptr(col), dptr(op)) if full else (None, None, None)
        check(getattr(self.L, ENTRIES[entry][0])(
            stream(), V, dptr(fd, I64, True), *self.small(), dptr(sh, F32, allow_host=host), by_filter, _npp(self.vmh), _npp(self.Kh),
            _npp(self.cph), self.cam["width"], self.cam["height"], deg, 0.3, c["near_plane"], c["far_plane"], c["radius_clip"],
            dptr(radii), dptr(m2), dptr(dep), *opt, dptr(packed), dptr(sh_index, I32, True)))
        torch.cuda.synchronize()
        out = dict(radii=radii, m2=m2, dep=dep, packed=packed)
        if full:
            out.update(cn=cn, col=col, op=op)
        return {k: v.cpu() for k, v in out.items()}

    def state(self, n_sh, init=None, stats=None, stamp=None, host=False):
        """The tables a backward launch accumulates into: zeros, or copies of `init` (CPU tensors by name)."""
        dev, N = self.dev, self.N
        shape = {"gtab": (N, 12), "g_xyz": (N, 3), "g_opacity": (N,), "g_scaling": (N, 3), "g_rotation": (N, 4), "g_shs": (n_sh, 48),
                 "maxr": (N,), "acc": (N,), "den": (N,), "stab": (N, 4)}
        names = (["gtab"] if self.pk else ["g_xyz", "g_opacity", "g_scaling", "g_rotation"]) + ["g_shs"]
        names += {None: [], "arrays": ["maxr", "acc", "den"], "table": ["stab"], "no_max": ["acc", "den"]}[stats]
        st = {}
        for k in names:
            t = init[k].clone() if init is not None and k in init else torch.zeros(shape[k])
            assert tuple(t.shape) == shape[k], (k, t.shape)
            if k == "g_shs" and host:
                from clm_gs_amd.host import pinned_empty
                h = pinned_empty(shape[k])
                h.copy_(t)
                st[k] = h
            else:
                st[k] = t.to(dev)
        st["stats"], st["host"] = stats, host
        if stamp is not None:
            st["stamp"] = stamp.clone().to(I32).to(dev)
        return st

    def bwd(self, st, V, filt, deg, radii, sh_mode="by_row", entry="plain", lines=None, partials=None, row_cum=None,
            only_visible=0, cur_step=0, want_m2=False):
        """One launch into the tables of `st` -> v_means2d_out (and the abs one) if asked for."""
        from clm_gs_amd._lib import check, dptr, stream
        dev = self.dev
        _, name, abs_pair, _ = ENTRIES[entry]
        sh, by_filter, sh_index, _, n_sh = self.sh_tables(V, filt, sh_mode, st["host"])
        assert st["g_shs"].shape[0] == n_sh
        fd = filt.to(dev) if filt is not None else None
        rd = radii.to(I32).to(dev)
        pgd = lines.to(dev).contiguous() if lines is not None else None
        prd = partials.to(dev).contiguous() if partials is not None else None
        rcd = row_cum.to(dev) if row_cum is not None else None
        gsmall = (dptr(st["gtab"]), None, None, None) if self.pk else tuple(dptr(st[k]) for k in ("g_xyz", "g_opacity", "g_scaling", "g_rotation"))
        stats = {None: (None, None, None), "arrays": ("maxr", "acc", "den"), "table": ("stab", None, None),
                 "no_max": (None, "acc", "den")}[st["stats"]]
        stats = tuple(dptr(st[k]) if k else None for k in stats)
        m2o = torch.full((V, 2), float("nan"), device=dev) if want_m2 else None
        m2a = torch.full((V, 2), float("nan"), device=dev) if want_m2 and abs_pair else None
        tail = (dptr(m2a, F32, True),) if abs_pair else ()
        check(getattr(self.L, name)(
            stream(), V, dptr(fd, I64, True), *self.small(), dptr(sh, F32, allow_host=st["host"]), by_filter, _npp(self.vmh),
            _npp(self.Kh), _npp(self.cph), self.cam["width"], self.cam["height"], deg, 0.3, dptr(rd), dptr(pgd, F32, True), *gsmall,
            dptr(st["g_shs"], F32, allow_host=st["host"]), *stats, dptr(m2o, F32, True), int(only_visible), dptr(prd, F32, True),
            dptr(rcd, I64, True), dptr(sh_index, I32, True), dptr(st.get("stamp"), I32, True), int(cur_step), *tail))
        torch.cuda.synchronize()
        return (m2o.cpu() if m2o is not None else None), (m2a.cpu() if m2a is not None else None)

    def snap(self, st):
        """CPU copies of the tables, the packed gradient table also as its four groups."""
        out = {k: v.detach().cpu().clone() for k, v in st.items() if torch.is_tensor(v)}
        if self.pk:
            g = out["gtab"]
            out.update(g_xyz=g[:, 0:3], g_opacity=g[:, 3], g_scaling=g[:, 4:7], g_rotation=g[:, 7:11])
        return out


@functools.lru_cache(maxsize=None)
def _launcher(dev, pk):
    raw, cam = FR.scene()
    return _Launch(dev, raw, cam, pk)


def _grad_errors(got, ref, what, n_sh_rows=None, sid=None, base=None):
    """rel-L2 of the five gradient groups (minus `base`, the tables' initial content) against the reference's; the SH
    table may be indexed by position or staged id (sid: position -> table row)."""
    worst = 0.0
    for k in FR.GROUPS:
        g = got["g_" + k].double()
        if base is not None:
            g = g - base["g_" + k].double()
        y = ref["grads"][k].reshape(ref["grads"][k].shape[0], -1)
        if k == "shs" and sid is not None:
            rows, tbl = sid
            full = torch.zeros(g.shape, dtype=torch.float64)
            full[tbl] = y[rows]
            y = full
        e = rel_l2(g.reshape(y.shape), y) if float(y.abs().max()) > 0 else float(g.abs().max())
        worst = max(worst, e)
        assert e < GRAD_TOL, (what, k, e)
    return worst


# ------------------------------------------------------------------------------------------------ a. forward
def _check_forward(out, ref, what, aa):
    assert torch.equal(out["radii"], ref["radii"]), what
    vis = ref["radii"] > 0
    dead = ~vis
    if bool(dead.any()):  # culled rows: exact zeros (the plain entry's opacity is sigmoid(o) for every row, as the reference's)
        for k in ("m2", "dep", "cn", "col") + (("op",) if aa else ()):
            assert float(out[k][dead].abs().max()) == 0.0, (what, k)
        if not aa:
            assert rel_l2(out["op"][dead], ref["op"][dead]) < COMP_TOL, what
    if not bool(vis.any()):
        return {}
    e = dict(m2=float(((out["m2"].double() - ref["m2"]).abs() / (1 + ref["m2"].abs()))[vis].max()),
             dep=rel_l2(out["dep"][vis], ref["dep"][vis]), cn=rel_l2(out["cn"][vis], ref["cn"][vis]),
             col=float((out["col"].double() - ref["col"])[vis].abs().max()), op=rel_l2(out["op"][vis], ref["op"][vis]))
    for k, bound in (("m2", 1e-5), ("dep", 1e-6), ("cn", 1e-5), ("col", 1e-5), ("op", COMP_TOL)):
        assert e[k] < bound, (what, k, e[k])
    # the record, word for word:  x y o ca | cb cc r g | b 0 0 0 | (fourth float4: not written)
    rec = out["packed"]
    want = torch.cat((out["m2"], out["op"][:, None], out["cn"], out["col"], torch.zeros(rec.shape[0], 3)), dim=1)
    assert _same(rec[:, :12], want), what
    assert bool(torch.isnan(rec[:, 12:]).all()), what
    return e


@pytest.mark.parametrize("deg", [0, 1, 2, 3])
@pytest.mark.parametrize("V", VS)
def test_forward_every_variant(dev, V, deg):
    worst = {}
    for entry, aa in (("plain", False), ("aa", True)):
        for filt_on in (True, False):
            filt = _filter(V, filt_on)
            ref = _ref(V, filt_on, deg, aa)
            assert not filt_on or bool((ref["radii"] > 0).any())
            for pk in (False, True):
                la = _launcher(dev, pk)
                base = None
                for sh_mode in ("by_row", "by_position", "staged"):
                    what = f"V={V} deg={deg} {entry} filter={filt_on} packed={pk} sh={sh_mode}"
                    out = la.fwd(V, filt, deg, sh_mode, entry)
                    for k, e in _check_forward(out, ref, what, aa).items():
                        worst[k] = max(worst.get(k, 0.0), e)
                    if base is None:
                        base = out
                    for k in base:  # the three addressings: the same bits
                        assert _same(out[k], base[k]), (what, k)
                ship = la.fwd(V, filt, deg, "by_row", entry, full=False)  # conics = colors = opacities = NULL
                for k in ("radii", "m2", "dep", "packed"):
                    assert _same(ship[k], base[k]), (V, deg, entry, filt_on, pk, k)
    print(f"forward V={V} deg={deg}: worst " + " ".join(f"{k} {v:.3g}" for k, v in worst.items()))


@pytest.mark.parametrize("cull", ["near", "far", "clip"])
def test_forward_culls(dev, cull):
    """near_plane, a finite far_plane, radius_clip: rows on both sides (FR.scene_conditions), radii exact."""
    for entry, aa in (("plain", False), ("aa", True)):
        for filt_on in (True, False):
            ref, dflt = _ref(N0, filt_on, 3, aa, cull=cull), _ref(N0, filt_on, 3, aa)
            flipped = (ref["radii"] > 0) != (dflt["radii"] > 0)
            assert int(flipped.sum()) >= 10
            for pk in (False, True):
                out = _launcher(dev, pk).fwd(N0, _filter(N0, filt_on), 3, "by_row", entry, cull=cull)
                e = _check_forward(out, ref, f"{cull} {entry} filter={filt_on} packed={pk}", aa)
    print(f"cull {cull}: {int(flipped.sum())} rows change sides; " + " ".join(f"{k} {v:.3g}" for k, v in e.items()))


# ------------------------------------------------------------------------------------------------ b. backward, plain
@pytest.mark.parametrize("deg", [0, 1, 2, 3])
@pytest.mark.parametrize("V", VS)
def test_plain_backward_against_float64(dev, V, deg):
    """The default entry of every run, [V,16] table, into zeroed tables; the SH gradient columns at or above the degree's
    last float4 keep their bits."""
    worst = 0.0
    for filt_on in (True, False):
        filt = _filter(V, filt_on)
        ref = _ref(V, filt_on, deg, False, seed=10 * V + deg)
        lines = _lines16(V, 10 * V + deg)
        vis = ref["radii"] > 0
        if filt_on and V >= 63:  # the clamped-tx branch and the per-channel clamp mask are exercised
            pos = {int(r): i for i, r in enumerate(filt.tolist())}
            for r in (*S["clamped_tx"], S["dark"], S["one_channel"], S["far"], S["tiny"]):
                assert bool(vis[pos[r]]), r
            assert not bool(vis[pos[S["behind"]]]) and not bool(vis[pos[S["off_screen"]]])
            one = ref["grads"]["shs"][S["one_channel"]].reshape(16, 3)
            assert float(one[:, 0].abs().max()) == 0.0 and float(one[0, 1:].abs().min()) > 0
        for pk in (False, True):
            la = _launcher(dev, pk)
            init = {"g_shs": torch.zeros(N0, 48)}
            init["g_shs"][:, 4 * nf4(deg):] = SENT
            st = la.state(N0, init)
            la.bwd(st, V, filt, deg, ref["radii"], lines=lines)
            got = la.snap(st)
            assert float((got["g_shs"][:, 4 * nf4(deg):] - SENT).abs().sum()) == 0.0
            got["g_shs"][:, 4 * nf4(deg):] = 0.0
            worst = max(worst, _grad_errors(got, ref, f"V={V} deg={deg} filter={filt_on} packed={pk}"))
            if pk:
                assert float(got["gtab"][:, 11].abs().max()) == 0.0  # the pad word
    print(f"plain backward V={V} deg={deg}: worst gradient rel_l2 {worst:.3g}")


# ------------------------------------------------------------------------------------------------ c. accumulation
def _garbage(ref, seed, n_sh=N0, pk=None):
    """Random content of the gradients' magnitude for every gradient table (the packed one included)."""
    g = torch.Generator().manual_seed(seed)
    out = {}
    for k in FR.GROUPS:
        y = ref["grads"][k]
        rms = float(y[y != 0].abs().mean()) if bool((y != 0).any()) else 1.0
        shape = (n_sh, 48) if k == "shs" else tuple(y.shape)
        out["g_" + k] = (torch.randn(shape, generator=g) * rms).float()
    gt = torch.randn(out["g_xyz"].shape[0], 12, generator=g)
    gt[:, 0:3], gt[:, 3], gt[:, 4:7], gt[:, 7:11] = out["g_xyz"], out["g_opacity"], out["g_scaling"], out["g_rotation"]
    out["gtab"] = gt
    n = gt.shape[0]
    out["maxr"], out["acc"] = torch.rand(n, generator=g) * 20, torch.rand(n, generator=g)
    out["den"] = torch.randint(0, 5, (n,), generator=g).float()
    out["stab"] = torch.stack((out["maxr"], out["acc"], out["den"], torch.randn(n, generator=g)), dim=1).contiguous()
    return out


@pytest.mark.parametrize("V", VS)
def test_accumulation_into_tables_that_hold_earlier_sums(dev, V):
    worst = 0.0
    for deg in (1, 3):
        filt = _filter(V, True)
        ref1, ref2 = _ref(V, True, deg, False, seed=V + 1), _ref(V, True, deg, False, seed=V + 2)
        l1, l2 = _lines16(V, V + 1), _lines16(V, V + 2)
        vis = ref1["radii"] > 0
        inside = torch.zeros(N0, dtype=torch.bool)
        inside[filt] = True
        touched = torch.zeros(N0, dtype=torch.bool)
        touched[filt[vis]] = True
        for pk in (False, True):
            la = _launcher(dev, pk)
            init = _garbage(ref1, 50 + V)
            st = la.state(N0, init, stats="table")
            la.bwd(st, V, filt, deg, ref1["radii"], lines=l1)
            a = la.snap(st)
            names = ["gtab", "g_shs"] if pk else ["g_xyz", "g_opacity", "g_scaling", "g_rotation", "g_shs"]
            for k in names:  # rows outside the filter, and rows with radius 0, keep their bits
                assert _same(a[k][~touched], init[k][~touched]), (V, deg, pk, k)
                assert not _same(a[k][touched], init[k][touched])
            assert _same(a["stab"][~inside], init["stab"][~inside])
            assert _same(a["g_shs"][:, 4 * nf4(deg):], init["g_shs"][:, 4 * nf4(deg):])
            worst = max(worst, _grad_errors(a, ref1, f"V={V} deg={deg} packed={pk} first", base=init))
            la.bwd(st, V, filt, deg, ref1["radii"], lines=l2)  # other lines add again
            b = la.snap(st)
            worst = max(worst, _grad_errors(b, ref2, f"V={V} deg={deg} packed={pk} second", base=a))
            st2 = la.state(N0, init, stats="table")  # identical launches from identical state: identical bits
            la.bwd(st2, V, filt, deg, ref1["radii"], lines=l1)
            a2 = la.snap(st2)
            for k in names + ["stab"]:
                assert _same(a2[k], a[k]), (V, deg, pk, k)
    print(f"accumulation V={V}: worst rel_l2 of (out - init) {worst:.3g}")


# ------------------------------------------------------------------------------------------------ d. partial lines
COUNTS = (0, 1, 4, 5, 8, 9, 13)


def _partial_case(V, seed, abs_pair, shift):
    """tests/test_gpu_pose.py::_partial_case for this kernel: row ranges of COUNTS lines in turn (starting at `shift`), lines
    of clmgs_rasterize_partials_bytes(1) bytes whose unread words are NaN, and the [V,16] table of their ascending float32
    sums from zero."""
    from clm_gs_amd import _lib
    LF = int(_lib.lib().clmgs_rasterize_partials_bytes(1)) // 4
    assert LF >= 12
    counts = torch.tensor(COUNTS)[(torch.arange(V) + shift) % len(COUNTS)]
    row_cum = torch.cumsum(counts, 0).to(I64)
    T = max(int(row_cum[-1]), 1)
    g = torch.Generator().manual_seed(seed)
    part = torch.full((T, LF), float("nan"))
    part[:, :9] = torch.randn(T, 9, generator=g)
    if abs_pair:
        part[:, 10:12] = torch.rand(T, 2, generator=g)
    used = list(range(9)) + ([10, 11] if abs_pair else [])
    sums = np.zeros((V, 16), dtype=np.float32)
    start = (row_cum - counts).numpy()
    pn = part.numpy()
    for l in range(max(COUNTS)):  # float32, ascending
        on = np.nonzero(counts.numpy() > l)[0]
        for w in used:
            sums[on, w] = sums[on, w] + pn[start[on] + l, w]
    lines = torch.from_numpy(sums)
    unused = [w for w in range(16) if w not in used]
    lines[:, unused] = float("nan")
    return part, row_cum, lines, counts


@pytest.mark.parametrize("entry", ["plain", "abs", "aa", "aa_abs"])
@pytest.mark.parametrize("V", VS)
def test_partial_lines_and_row_cum(dev, V, entry):
    """The shipped route.  Bit-equal to the [V,16] route fed the ascending sums, and against float64."""
    _, _, abs_pair, aa = ENTRIES[entry]
    deg, filt = 3, _filter(V, True)
    radii = _ref(V, True, deg, aa)["radii"]
    vis = radii > 0
    # a shift that gives a VISIBLE row no line at all
    shift = next(s for s in range(len(COUNTS)) if bool(vis[((torch.arange(V) + s) % len(COUNTS)) == 0].any()))
    part, row_cum, lines, counts = _partial_case(V, 3 * V, abs_pair, shift)
    assert bool((vis & (counts == 0)).any())
    assert V < 63 or set(counts.tolist()) == set(COUNTS)
    raw, cam = FR.scene()
    ref = FR.reference(raw, filt, cam, deg, aa, lines=torch.nan_to_num(lines))
    worst = 0.0
    for pk in (False, True):
        la = _launcher(dev, pk)
        init = _garbage(ref, 7)
        names = (["gtab"] if pk else ["g_xyz", "g_opacity", "g_scaling", "g_rotation"]) + ["g_shs", "stab"]
        sa, sb = la.state(N0, init, stats="table"), la.state(N0, init, stats="table")
        m2a, absa = la.bwd(sa, V, filt, deg, radii, entry=entry, partials=part, row_cum=row_cum, want_m2=True)
        m2b, absb = la.bwd(sb, V, filt, deg, radii, entry=entry, lines=lines, want_m2=True)
        a, b = la.snap(sa), la.snap(sb)
        for k in names:
            assert _same(a[k], b[k]), (V, entry, pk, k)
        # the screen-space gradient copies: the summed words, for every filter row (dead ones included)
        assert _same(m2a, lines[:, 0:2]) and _same(m2b, lines[:, 0:2])
        if abs_pair:
            assert _same(absa, lines[:, 10:12]) and _same(absb, lines[:, 10:12])
        worst = max(worst, _grad_errors(a, ref, f"V={V} {entry} packed={pk}", base=init))
    print(f"partial lines V={V} {entry}: worst gradient rel_l2 {worst:.3g}")


# ------------------------------------------------------------------------------------------------ e. first-touch stamps
@pytest.mark.parametrize("sh_mode", ["by_row", "staged"])
@pytest.mark.parametrize("V", VS)
def test_first_touch_stamps(dev, V, sh_mode):
    """cur_step = 5, stamps 5 / 3 / 0.  A fresh visible row ends with the bits of a launch into zeroed tables in its
    degree's float4s and is stamped; its float4s BEYOND the degree's are not written (they keep what the table held:
    DESIGN.md, "Gradient rows are stored on first touch", says why nothing stale can wait there); a row already stamped 5
    accumulates; a row with radius 0 keeps row and stamp; the four unpacked arrays accumulate whatever the stamp."""
    cur, worst = 5, 0.0
    for deg in (0, 1, 2, 3):
        filt = _filter(V, True)
        ref = _ref(V, True, deg, False, seed=V + 9)
        lines = _lines16(V, V + 9)
        vis = ref["radii"] > 0
        for pk in (False, True):
            la = _launcher(dev, pk)
            _, _, _, sid, n_sh = la.sh_tables(V, filt, sh_mode)
            g = torch.Generator().manual_seed(V + deg)
            stamp0 = torch.tensor([5, 3, 0], dtype=I32)[torch.randint(0, 3, (n_sh,), generator=g)]
            init = _garbage(ref, 60 + V, n_sh=n_sh)
            runs = {}
            for name, ini, stp in (("zero", None, None), ("acc", init, None), ("stamped", init, stamp0)):
                st = la.state(n_sh, ini, stamp=stp)
                la.bwd(st, V, filt, deg, ref["radii"], sh_mode=sh_mode, lines=lines, cur_step=cur if stp is not None else 0)
                runs[name] = la.snap(st)
            z, a, c = runs["zero"], runs["acc"], runs["stamped"]
            was5 = stamp0[sid] == cur
            fresh, again = vis & ~was5, vis & was5
            assert V < 63 or (bool(fresh.any()) and bool(again.any()) and bool((~vis).any()))
            k4 = 4 * nf4(deg)
            what = (V, sh_mode, deg, pk)
            # the SH gradient rows, by the table row position i uses
            assert _same(c["g_shs"][sid[fresh], :k4], z["g_shs"][sid[fresh], :k4]), what
            assert _same(c["g_shs"][sid[fresh], k4:], init["g_shs"][sid[fresh], k4:]), what  # not written
            assert _same(c["g_shs"][sid[again]], a["g_shs"][sid[again]]), what
            assert _same(c["g_shs"][sid[~vis]], init["g_shs"][sid[~vis]]), what
            other = torch.ones(n_sh, dtype=torch.bool)
            other[sid] = False
            assert _same(c["g_shs"][other], init["g_shs"][other]), what
            # stamps
            want = stamp0.clone()
            want[sid[fresh]] = cur
            assert torch.equal(c["stamp"], want), what
            # the small gradients, by row id
            if pk:
                assert _same(c["gtab"][filt[fresh]], z["gtab"][filt[fresh]]), what
                assert _same(c["gtab"][filt[again]], a["gtab"][filt[again]]), what
                assert _same(c["gtab"][filt[~vis]], init["gtab"][filt[~vis]]), what
            else:
                for k in ("g_xyz", "g_opacity", "g_scaling", "g_rotation"):
                    assert _same(c[k], a[k]), (what, k)
            worst = max(worst, _grad_errors(z, ref, f"{what} zeroed", sid=(filt, sid) if sh_mode == "staged" else None))
    print(f"first touch V={V} {sh_mode}: every comparison bit-exact; the zeroed launch's worst gradient rel_l2 {worst:.3g}")


# ------------------------------------------------------------------------------------------------ f. statistics
@pytest.mark.parametrize("V", VS)
def test_statistics_forms(dev, V):
    raw, cam = FR.scene()
    W, H = cam["width"], cam["height"]
    worst = 0.0
    for entry in ("plain", "abs"):
        abs_pair = ENTRIES[entry][2]
        for filt_on in (True, False):
            filt, deg = _filter(V, filt_on), 2
            rows = _rows(V, filt)
            ref = _ref(V, filt_on, deg, False, seed=V + 4)
            lines = _lines16(V, V + 4, abs_pair)
            init = _garbage(ref, 70 + V)
            for only in (0, 1):
                for pk in (False, True):
                    la = _launcher(dev, pk)
                    sa, sb = la.state(N0, init, stats="arrays"), la.state(N0, init, stats="table")
                    la.bwd(sa, V, filt, deg, ref["radii"], entry=entry, lines=lines, only_visible=only)
                    la.bwd(sb, V, filt, deg, ref["radii"], entry=entry, lines=lines, only_visible=only)
                    a, b = la.snap(sa), la.snap(sb)
                    what = (V, entry, filt_on, only, pk)
                    hit = torch.zeros(N0, dtype=torch.bool)
                    hit[rows[ref["radii"] > 0] if only else rows] = True
                    for j, k in enumerate(("maxr", "acc", "den")):  # the two forms: the same bits
                        assert _same(b["stab"][:, j], a[k]), (what, k)
                    assert float(b["stab"][hit, 3].abs().max() if bool(hit.any()) else 0.0) == 0.0, what
                    assert _same(b["stab"][~hit], init["stab"][~hit]), what
                    mr, ga, dn = FR.statistics(init["maxr"], init["acc"], init["den"], rows, ref["radii"], torch.nan_to_num(lines), W, H,
                                               abs_pair=abs_pair, only_visible=bool(only))
                    assert np.array_equal(a["maxr"].double().numpy(), mr) and np.array_equal(a["den"].double().numpy(), dn), what
                    e = rel_l2(a["acc"], torch.from_numpy(ga))
                    worst = max(worst, e)
                    assert e < 1e-6, (what, e)
                    for k in ("g_xyz", "g_shs"):  # the gradients do not depend on the statistics form
                        assert _same(a[k], b[k])
                    # max_radii2D = NULL: no statistics, whatever the other two pointers say
                    sn = la.state(N0, init, stats="no_max")
                    la.bwd(sn, V, filt, deg, ref["radii"], entry=entry, lines=lines, only_visible=only)
                    n = la.snap(sn)
                    assert _same(n["acc"], init["acc"]) and _same(n["den"], init["den"]) and _same(n["g_shs"], a["g_shs"]), what
    print(f"statistics V={V}: worst grad_accum rel_l2 {worst:.3g}")


# ------------------------------------------------------------------------------------------------ g. second chunk
def test_a_wave_runs_a_second_chunk(dev):
    """V = 64 x clmgs_preprocess_grid_cap() + 70 unique rows (FR.tiled_scene), degree 1, packed tables: forward and
    backward of the whole launch against float64; the rows past 64 x cap, which only a second chunk reaches, are held to
    the reference on their own, and dropping them changes the reference by far more than the tolerance."""
    from clm_gs_amd import _lib
    cap = int(_lib.lib().clmgs_preprocess_grid_cap())
    V = 64 * cap + 70
    assert 100_000 < V <= 300_000
    raw, cam = FR.tiled_scene(V)
    deg = 1
    filt = torch.randperm(V, generator=torch.Generator().manual_seed(2)).contiguous()
    lines = _lines16(V, 8)
    ref = FR.reference(raw, filt, cam, deg, False, lines=lines)
    la = _Launch(dev, raw, cam, True)
    out = la.fwd(V, filt, deg)
    e = _check_forward(out, ref, f"V={V}", False)
    tail_pos = torch.arange(64 * cap, V)
    assert torch.equal(out["radii"][tail_pos], ref["radii"][tail_pos]) and bool((ref["radii"][tail_pos] > 0).any())
    init = {"g_shs": torch.full((V, 48), SENT)}
    init["g_shs"][:, :4 * nf4(deg)] = 0.0
    st = la.state(V, init, stats="table")
    la.bwd(st, V, filt, deg, ref["radii"], lines=lines)
    got = la.snap(st)
    assert float((got["g_shs"][:, 4 * nf4(deg):] - SENT).abs().sum()) == 0.0
    got["g_shs"][:, 4 * nf4(deg):] = 0.0
    worst = _grad_errors(got, ref, f"V={V}")
    # the second chunks alone
    tail_rows = filt[tail_pos]
    cut = {}
    for k in FR.GROUPS:
        y = ref["grads"][k].reshape(V, -1)
        g = got["g_" + k].reshape(V, -1)
        et = rel_l2(g[tail_rows], y[tail_rows])
        assert et < GRAD_TOL, (k, et)
        dropped = y.clone()
        dropped[tail_rows] = 0.0
        cut[k] = rel_l2(dropped, y)
        assert cut[k] > 10 * GRAD_TOL, (k, cut[k])
    assert float(got["stab"][:, 2].sum()) == V  # every row counted once
    print(f"second chunk V={V}: forward " + " ".join(f"{k} {v:.3g}" for k, v in e.items()) + f"; worst gradient rel_l2 {worst:.3g}; "
          f"without the rows past 64 x cap the reference moves by {min(cut.values()):.3g} .. {max(cut.values()):.3g}")


# ------------------------------------------------------------------------------------------------ h. host tables
def test_tables_in_pinned_host_memory(dev):
    """The host-resident route: sh_rows and g_sh_rows are staging tables in clmgs_pinned_alloc memory, addressed through
    sh_index.  Degree 3, V = 400: the bits of the same launch on device tables."""
    V, deg = N0, 3
    filt = _filter(V, True)
    ref = _ref(V, True, deg, False, seed=31)
    lines = _lines16(V, 31)
    for pk in (False, True):
        la = _launcher(dev, pk)
        fd, fh = la.fwd(V, filt, deg, "staged"), la.fwd(V, filt, deg, "staged", host=True)
        for k in fd:
            assert _same(fd[k], fh[k]), (pk, k)
        init = _garbage(ref, 90, n_sh=V + 3)
        sd, sh = la.state(V + 3, init), la.state(V + 3, init, host=True)
        assert not sh["g_shs"].is_cuda and sd["g_shs"].is_cuda
        la.bwd(sd, V, filt, deg, ref["radii"], sh_mode="staged", lines=lines)
        la.bwd(sh, V, filt, deg, ref["radii"], sh_mode="staged", lines=lines)
        a, b = la.snap(sd), la.snap(sh)
        for k in a:
            assert _same(a[k], b[k]), (pk, k)
        assert not _same(a["g_shs"], init["g_shs"])
    print("pinned host tables: forward outputs and every gradient table bit-equal to the device tables' (deviation 0)")

