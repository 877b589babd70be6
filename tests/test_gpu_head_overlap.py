"""head_overlap: the head of a batch (small-attribute catch-up + visibility words) in two launches over disjoint sets of
256-row blocks -- the blocks the previous batch's last camera could not see under that camera's backward, the rest at the
head -- is bit for bit the single launch: the two kernels with their block selector, the engine with the option on
against off, and every case in which the engine must fall back to the single launch."""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu

BSZ = 4


class _Scene:
    cameras_extent = 30.0


# ------------------------------------------------------------------------------------------------- 1. the kernels
K_N, K_C, K_W, K_H = 256 * 37 + 19, 3, 160, 128


def _kernel_state():
    """Host tensors of one head: Z-ordered rows, three cameras, blocks 0..3 steps behind and one at kmax, gradient lines
    stamped at different steps."""
    from clm_gs_amd import _lib, utils
    from clm_gs_amd.synthetic import nadir_cameras, synth_gaussians
    kmax = int(_lib.lib().clmgs_small_deferred_kmax())
    to_step = kmax + 4
    sc = synth_gaussians(K_N, seed=3, device="cuda")
    order = utils.morton_order(sc["xyz"])
    g = torch.Generator().manual_seed(11)
    st = {}
    for name, key, w in (("xyz", "xyz", 3), ("opacity", "opacity", 1), ("scaling", "scaling", 3), ("rotation", "rotation", 4)):
        st[name] = utils.gather_rows(sc[key], order).float().reshape(K_N, w).cpu().contiguous()
        st[name + "_m"] = (torch.randn(K_N, w, generator=g) * 1e-3).contiguous()
        st[name + "_v"] = (torch.rand(K_N, w, generator=g) * 1e-5).contiguous()
    st["packed_p"] = torch.cat([st["xyz"], st["opacity"], st["scaling"], st["rotation"],
                                torch.zeros(K_N, 1)], dim=1).contiguous()
    st["packed_g"] = (torch.randn(K_N, 12, generator=g) * 1e-3).contiguous()
    st["g_stamp"] = torch.randint(0, to_step + 1, (K_N,), generator=g, dtype=torch.int32)
    nb = (K_N + 255) // 256
    last = to_step - (torch.arange(nb, dtype=torch.int32) % 4)
    last[17] = to_step - kmax
    st["blk_last"] = last.contiguous()
    cams = nadir_cameras(K_C, K_N, K_W, K_H, 0.12, seed=5, device="cuda")
    st["vm"] = torch.stack([c.world_view_transform.transpose(0, 1) for c in cams]).cpu().contiguous()
    st["Ks"] = torch.stack([c.K for c in cams]).cpu().contiguous()
    return st, to_step, kmax, nb


def _run_head(st, to_step, kmax, nb, launches):
    """One head on a fresh device copy of `st`.  launches: None = the plain entries (one launch, today's kernels);
    else a list of (sel_words | None, mask, want) for clmgs_adam_small_deferred_sel and the visibility pass.
    -> dict of every tensor the head leaves."""
    from clm_gs_amd import _lib
    from clm_gs_amd.gsplat import visibility_select, visibility_select_words
    L = _lib.lib()
    d = {k: v.cuda() for k, v in st.items()}
    flags = torch.full((nb,), 7, dtype=torch.uint8, device="cuda")
    cams_w = torch.full((nb,), -1, dtype=torch.int64, device="cuda")
    P = lambda names: (ctypes.c_void_p * 4)(*[d[n].data_ptr() for n in names])
    ps, ms, vs = (P(["xyz", "opacity", "scaling", "rotation"]), P(["xyz_m", "opacity_m", "scaling_m", "rotation_m"]),
                  P(["xyz_v", "opacity_v", "scaling_v", "rotation_v"]))
    lr = (ctypes.c_double * (4 * kmax))(*[x * (1.0 + 0.01 * j) for j in range(kmax) for x in (1.6e-4, 5e-2, 5e-3, 1e-3)])
    sidx = (ctypes.c_int32 * kmax)(*[to_step - j for j in range(kmax)])
    pm = (ctypes.c_float * (kmax + 1))(*[1e-12 + 0.002 * k for k in range(kmax + 1)])
    sg = (ctypes.c_float * (kmax + 1))(*[1.001 + 0.01 * k for k in range(kmax + 1)])
    common = lambda: (_lib.stream(), K_N, ps, ms, vs, _lib.dptr(d["packed_p"]), _lib.dptr(d["packed_g"]),
                      _lib.dptr(d["g_stamp"], torch.int32), _lib.dptr(d["blk_last"], torch.int32), to_step, kmax, lr, sidx,
                      pm, sg, 0.9, 0.999, 1e-15, 0.25, K_C, _lib.dptr(d["vm"]), _lib.dptr(d["Ks"]), K_W, K_H, 0.3, 0.01,
                      1e10, 0, _lib.dptr(flags, torch.uint8))
    vis = lambda **kw: visibility_select(d["xyz"], d["rotation"], d["scaling"], d["vm"], d["Ks"], K_W, K_H,
                                         block_flags=flags, **kw)
    if launches is None:
        _lib.check(L.clmgs_adam_small_deferred(*common()))
        filters, touched = vis()
        cams_w = None
    else:
        for words, mask, want in launches:
            _lib.check(L.clmgs_adam_small_deferred_sel(*common(), _lib.dptr(cams_w, torch.int64),
                                                       _lib.dptr(words, torch.int64, True), mask, want))
        if len(launches) == 1:
            filters, touched = vis()
        else:
            (w0, m0, t0), (w1, m1, t1) = launches
            temp = visibility_select_words(d["xyz"], d["rotation"], d["scaling"], d["vm"], d["Ks"], K_W, K_H,
                                           (w0, m0, t0), block_flags=flags)
            filters, touched = vis(block_sel=(w1, m1, t1), temp=temp)
    torch.cuda.synchronize()
    out = {k: d[k] for k in st if k not in ("vm", "Ks", "packed_g", "g_stamp")}
    out["blk_flag"] = flags
    for i, f in enumerate(filters):
        out["filter%d" % i] = f
    out["touched"] = touched
    return out, cams_w


@pytest.fixture(scope="module")
def kernel_ref(dev):
    st, to_step, kmax, nb = _kernel_state()
    ref, _ = _run_head(st, to_step, kmax, nb, None)
    one, words = _run_head(st, to_step, kmax, nb, [(None, 0, 0)])
    return st, to_step, kmax, nb, ref, one, words


def _same(a, b):
    assert a.keys() == b.keys()
    for k in a:
        assert a[k].shape == b[k].shape and torch.equal(a[k], b[k]), k


def test_camera_words_launch_equals_plain_entry(kernel_ref):
    """The <SEL> kernel without a selector (it tests every camera to leave the camera words) == the plain entry; the words
    agree with the flags, differ between blocks, and the state exercises what it claims to."""
    st, to_step, kmax, nb, ref, one, words = kernel_ref
    _same(ref, one)
    assert torch.equal(words != 0, ref["blk_flag"] != 0)
    assert int((words >> K_C).abs().max()) == 0  # no bit beyond the cameras
    assert len(set(words.tolist())) >= 3  # blocks near different cameras, and blocks near none
    assert 0 < int((ref["blk_flag"] == 0).sum()) < nb
    assert not torch.equal(ref["xyz"].cpu(), st["xyz"])  # something was replayed
    assert int(ref["blk_last"][17]) == to_step  # the block at kmax was forced
    assert all(f.numel() > 0 for f in (ref["filter0"], ref["filter1"], ref["filter2"]))


@pytest.mark.parametrize("table", ["clear", "set", "random"])
def test_two_launches_equal_one(kernel_ref, table):
    """sel_want 0 then 1 over a selector table == one launch: the four tensors, their moments, the mirror, blk_last,
    blk_flag, the camera words, the visibility filters and the union."""
    st, to_step, kmax, nb, ref, one, words = kernel_ref
    if table == "clear":
        sel = torch.zeros((nb,), dtype=torch.int64, device="cuda")
    elif table == "set":
        sel = torch.full((nb,), -1, dtype=torch.int64, device="cuda")
    else:
        sel = torch.randint(0, 1 << K_C, (nb,), generator=torch.Generator().manual_seed(5), dtype=torch.int64).cuda()
        assert 0 < int(((sel & 2) != 0).sum()) < nb
    two, words2 = _run_head(st, to_step, kmax, nb, [(sel, 2, 0), (sel, 2, 1)])
    _same(ref, two)
    assert torch.equal(words2, words)


def test_unselected_blocks_are_left_alone(kernel_ref):
    """One launch with sel_want = 0 alone: the blocks it does not take keep every entry they had (poisoned flag and word
    entries, blk_last, rows)."""
    st, to_step, kmax, nb, ref, one, words = kernel_ref
    sel = torch.randint(0, 1 << K_C, (nb,), generator=torch.Generator().manual_seed(5), dtype=torch.int64).cuda()
    half, w = _run_head(st, to_step, kmax, nb, [(sel, 2, 0)])
    skipped = ((sel & 2) != 0)
    assert torch.equal(half["blk_flag"][skipped], torch.full_like(half["blk_flag"][skipped], 7))
    assert torch.equal(w[skipped], torch.full_like(w[skipped], -1))
    assert torch.equal(half["blk_last"][skipped].cpu(), st["blk_last"][skipped.cpu()])
    rows = skipped.repeat_interleave(256)[:K_N]
    for k in ("xyz", "xyz_m", "xyz_v", "rotation", "packed_p"):
        assert torch.equal(half[k][rows].cpu(), st[k][rows.cpu()]), k
        assert torch.equal(half[k][~rows], ref[k][~rows]), k


# ------------------------------------------------------------------------------------------------- 2. / 3. the engine
E_N, E_W, E_H = 20_000, 160, 128


def _engine_run(head_overlap, batches, bsz=BSZ, between=None, **extra):
    """`batches` (lists of camera indices into one seeded camera set) through the HBM engine -> (per-batch log, final
    tensors after flush_lazy_rows, per-batch records, split count).  between(m, b, it): called after batch b."""
    from clm_gs_amd import _lib, utils
    from clm_gs_amd.strategies.clm_offload import GaussianModelCLMOffload, engine
    from clm_gs_amd.synthetic import nadir_cameras, synth_gaussians
    torch.manual_seed(0)
    args = utils.default_args(bsz=bsz, sh_residency="hbm", head_overlap=head_overlap, densify_from_iter=0,
                              densification_interval=10 ** 6, densify_until_iter=10 ** 6, opacity_reset_interval=10 ** 6,
                              densify_grad_threshold=0.00002, **extra)
    args.clm_offload = True
    utils.set_args(args)
    utils.set_img_size(E_H, E_W)
    utils.set_cur_iter(1)
    sc = synth_gaussians(E_N, seed=2, device="cuda")
    order = utils.morton_order(sc["xyz"])
    for k in ("xyz", "scaling", "rotation", "opacity", "shs48"):
        sc[k] = utils.gather_rows(sc[k], order)
    m = GaussianModelCLMOffload(3)
    m.create_from_tensors(sc["xyz"], sc["shs48"], sc["scaling"], sc["rotation"], sc["opacity"], spatial_lr_scale=2.0)
    m.active_sh_degree = 3
    m.training_setup(args)
    assert m.small_deferred
    m.fuse_sort_into_prune = True
    cams = nadir_cameras(25, E_N, E_W, E_H, 0.04, seed=6, device="cuda")  # a 5 x 5 grid of small footprints
    g = torch.Generator().manual_seed(8)
    for c in cams:
        c.original_image = (torch.rand(3, E_H, E_W, generator=g) * 255).to(torch.uint8).cuda()
    comm = torch.cuda.Stream()
    log, recs = [], []
    orig = engine.select_filters

    def logged(*a, **kw):
        filters, touched = orig(*a, **kw)
        log.extend(f.clone() for f in filters)
        log.append(touched.clone())
        return filters, touched
    engine.select_filters = logged
    split0 = _lib.STATS.get("head_overlap_split", 0)
    try:
        it = 1
        for b, idx in enumerate(batches):
            utils.set_cur_iter(it)
            m.update_learning_rate(it)
            losses, ordered, sparsity = engine._train_one_batch_hbm(
                m, _Scene, [cams[i] for i in idx], m.parameters_grad_buffer, None, None, comm, args)
            log.append(torch.stack(losses).clone())
            log.append(torch.tensor(sparsity))
            rec = (m._small_def or {}).get("head")
            recs.append(None if rec is None else dict(rec, ordered=list(ordered), words=rec["words"].clone()))
            if between is not None:
                between(m, b, it)
            it += bsz
    finally:
        engine.select_filters = orig
    m.flush_lazy_rows()
    torch.cuda.synchronize()
    assert (m._small_def or {}).get("head") is None  # nothing survives a flush
    st = m.optimizer.cpu_adam.state[m._parameters]
    final = [m._xyz.detach().clone(), m._opacity.detach().clone(), m._scaling.detach().clone(),
             m._rotation.detach().clone(), m._parameters.detach().clone(), st["exp_avg"].clone(), st["exp_avg_sq"].clone()]
    final += [m.optimizer.gpu_adam.state[p][k].clone() for p in (m._xyz, m._opacity, m._scaling, m._rotation)
              for k in ("exp_avg", "exp_avg_sq", "step")]
    return log, final, recs, _lib.STATS.get("head_overlap_split", 0) - split0


def _equal_runs(a, b):
    for x, y in zip(a[:2], b[:2]):
        assert len(x) == len(y)
        for i, (p, q) in enumerate(zip(x, y)):
            assert p.shape == q.shape and torch.equal(p.cpu(), q.cpu()), i


# the 5 x 5 camera grid (lawn-mower order).  The first batch has no step history yet, so its head leaves no words and
# the second head is a single launch.  Batch 2 revisits the position of batch 1's LAST camera (the late set holds blocks
# the new head needs); batch 3 lies at the far side of the grid from batch 2's last camera (nothing the new head needs is late)
E_BATCHES = [[0, 1, 2, 3], [4, 5, 6, 7], [7, 8, 9, 10], [3, 4, 23, 24], [12, 13, 16, 17], [11, 12, 13, 18]]
E_SPLITS = len(E_BATCHES) - 2


@pytest.fixture(scope="module")
def engine_off(dev):
    return _engine_run(False, E_BATCHES)


@pytest.mark.parametrize("depth", [1, 2, 3])
def test_engine_overlap_on_equals_off(engine_off, depth):
    """Six batches, head_overlap on against off: every batch's filters, union, losses and visible fractions, the five
    parameter tensors and every Adam moment, bit for bit; the split really ran, with and without needed late blocks.
    depth = head_overlap_cameras: the early part stays clear of the last 1 / 2 / 3 cameras of the previous batch."""
    on = _engine_run(True, E_BATCHES, head_overlap_cameras=depth)
    _equal_runs(on, engine_off)
    assert engine_off[3] == 0 and all(r is None for r in engine_off[2])
    assert on[3] == E_SPLITS  # every head but the first two ran in two launches
    recs = on[2]
    assert recs[0] is None
    mask = sum(1 << c for c in range(BSZ - depth, BSZ))
    assert all(r is not None and r["last"] == 3 and r["mask"] == mask and r["step"] == i + 1 for i, r in enumerate(recs) if i)
    # needed late blocks of head b+1: admitted by one of batch b's last `depth` cameras AND by some camera of batch b+1
    late = {i: int((((recs[i]["words"] & mask) != 0) & (recs[i + 1]["words"] != 0)).sum()) for i in range(1, len(recs) - 1)}
    early = {i: int((((recs[i]["words"] & mask) == 0) & (recs[i + 1]["words"] != 0)).sum()) for i in range(1, len(recs) - 1)}
    print("needed late / early blocks per head:", late, early)
    # rows: what batch b's last camera really touched against what batch b+1 touches -- shared for the pair 1 -> 2,
    # disjoint for 2 -> 3 (at the level of BLOCKS a few of the 79 straddle a jump of the Z-curve and are candidates of
    # far-apart cameras, so the conservative block sets of 2 -> 3 still meet in a few blocks)
    log = on[0]
    shared = {b: int(torch.isin(log[7 * b + 3], log[7 * (b + 1) + 4]).sum()) for b in (1, 2)}
    print("rows of the last camera touched again by the next batch:", shared)
    assert shared[1] > 0 and shared[2] == 0, shared
    assert late[1] > late[2], late
    assert all(e > 0 for e in early.values()), early


def test_fallback_bsz1(dev):
    """One camera per batch (the engine's batch driver called directly): there is no earlier camera to wait for, no record
    is ever left, every head is a single launch."""
    batches = [[0], [1], [1], [7]]
    on, off = _engine_run(True, batches, bsz=1), _engine_run(False, batches, bsz=1)
    _equal_runs(on, off)
    assert on[3] == 0 and all(r is None for r in on[2])


def test_fallback_reference_camera_order(dev):
    """The cameras are reordered after the head: the record names the camera that RAN last, by its position in the batch
    as given (the bit index of the words)."""
    on = _engine_run(True, E_BATCHES, reference_camera_order=True)
    off = _engine_run(False, E_BATCHES, reference_camera_order=True)
    _equal_runs(on, off)
    assert on[3] == E_SPLITS
    assert all(r is not None and r["last"] == r["ordered"][-1]
               and r["mask"] == sum(1 << c for c in r["ordered"][-2:]) for r in on[2][1:])  # (head_overlap_cameras = 2)
    print("cameras that ran last:", [r["last"] for r in on[2][1:]])
    assert any(r["last"] != BSZ - 1 for r in on[2][1:])  # the order really changed somewhere


def test_fallback_densify_and_flush(dev):
    """A densify_and_prune (+ re-sort) after batch 1 and a flush_small after batch 3: the record is gone at once, the next
    head runs as one launch, and the results are head_overlap=false's."""
    from clm_gs_amd import utils

    def between(m, b, it):
        if b == 1:
            n0 = m.get_xyz.shape[0]
            m.flush_lazy_rows()
            m.densify_and_prune(utils.get_args().densify_grad_threshold, 0.005, _Scene.cameras_extent, None)
            m.spatial_sort()
            assert m.get_xyz.shape[0] != n0
        if b == 3:
            m.flush_small()
        if b in (1, 3):
            assert (m._small_def or {}).get("head") is None
    on, off = _engine_run(True, E_BATCHES, between=between), _engine_run(False, E_BATCHES, between=between)
    _equal_runs(on, off)
    assert on[3] == E_SPLITS - 2  # heads 2 and 4 fell back
