"""Host-resident SH rows with PER-CAMERA staging windows (sh_residency="host", host_staging="window": the default).

The reference's offloading pipeline keeps, per micro-batch, only what that camera needs on the GPU and retains the rows the
next camera shares with it (retention sets H / D / G, strategies/clm_offload/engine.py:566-636; 13.0 GB of GPU memory at
28 M Gaussians, release_scripts/rubble4k_README.md:113).  `host_batch.py` (host_staging="batch") stages the
UNION of a batch's rows instead -- three [T, 48] tables, 6.6 GB at 28 M.  This module keeps that mode's properties

  * every touched row crosses the host link ONCE per direction and batch (parameters in before the first camera that
    uses it, gradient home after the last one; plain stores, no read-modify-write over the link),
  * the deferred host row optimizer + staging copy on the host pool, chunked hipMemcpyAsync on a side stream,
  * speculative prefetch of the hinted next batch while the present one renders (here: of its FIRST camera's rows),

with tables sized for ONE camera plus the rows that several cameras of the batch share:

    params   PT = [ P: rows used by >= 2 cameras, kept from their first to their last use | A: the current camera's arrivals ]
    grads    GT = [ GP                                                                    | GA ]       (same slot numbers)
    bounce   BB = [ the NEXT camera's arrivals land here (hipMemcpyAsync) while the current camera renders ]

Per camera k:  BB -> A (one device copy; BB is free for camera k+1's rows)  ->  render + backward from / into PT / GT by slot
->  the rows whose LAST camera this was send their gradient row home (zero-copy stores on a side stream)  ->  the arrivals
that a later camera uses again ("survivors") move, parameters and partial gradient, from A to their P slot.
Slots are planned once per batch from the visibility bitmap (a row is a survivor iff more than one bit is set); nothing is
recycled inside a batch, so the plan is a handful of scans over the batch's row list and two small read-backs.

28 M Gaussians, 4K, bsz 4: 3.4 GB of staging instead of 6.6 GB (peak 14.9 GB instead of 18.1 GB).
"""
import threading
import time

import torch

from ... import _lib, clm_kernels, utils
from ...gsplat import bucket_size
from ...host import pinned_empty
from ..base_engine import select_filters
from . import host_stages as S
from .engine import _encode_bitmap, _zero_small_grads


def _buffers(gaussians, need_a, need_p, need_late, dev, K=0):
    """Device tables (bucketed capacity, 8 % head room) + pinned host twins (50 %: host memory is cheap, and a pinned
    re-allocation is a hipHostMalloc of hundreds of ms).  `gen` counts device re-allocations: rows staged into an older
    generation are gone.  K > 0 (sh_hbm_budget_gb): the first K rows of the parameter and of the gradient table are the
    HBM-resident prefix of the model (slot r = row r), the P and A regions follow; a re-allocation carries them over."""
    hb = getattr(gaussians, "_hwin_bufs", None)
    N = gaussians._xyz.shape[0]
    if hb is None or hb["N"] != N or hb.get("K", 0) != K or hb["cap_a"] < need_a or hb["cap_p"] < need_p:
        gen = hb["gen"] + 1 if hb else 0
        keep, old_pt = None, None
        if hb is not None:
            # the tables are written by hipMemcpyAsync issued through ctypes on side streams (the caching allocator does not
            # know): drain the device before the old blocks go back to it
            torch.cuda.synchronize()
            same = hb["N"] == N and hb.get("K", 0) == K
            if same:
                keep = hb
                px = getattr(gaussians, "_hbm_prefix", None)
                if K and px is not None and not px["fill"]:
                    # the resident rows move to the new table; their waiting gradients are applied first (one pass of the
                    # deferred row optimizer over the K rows, ~4 ms at 14 M), so the gradient table holds zeros there and
                    # is not carried over: the only transient is the old parameter table beside the new one
                    if not gaussians.args.sparse_adam:
                        gaussians.hbm_prefix_catch_up(None, int(gaussians.optimizer.cpu_adam.global_step))
                    old_pt = hb["pt"]
            cap_a = max(hb["cap_a"] if same else 0, bucket_size(max(int(need_a * 1.08), 1)))
            cap_p = max(hb["cap_p"] if same else 0, bucket_size(max(int(need_p * 1.08), 1)))
            for k in ("pt", "gt", "bb"):
                hb[k] = None
        else:
            cap_a, cap_p = bucket_size(max(int(need_a * 1.08), 1)), bucket_size(max(int(need_p * 1.08), 1))
        gaussians._hwin_bufs = None
        new = dict(N=N, K=K, gen=gen, cap_a=cap_a, cap_p=cap_p, bb=torch.empty((cap_a, 48), device=dev),
                   rows_h=keep["rows_h"] if keep else None, stage_h=keep["stage_h"] if keep else None,
                   spec_rows_h=keep["spec_rows_h"] if keep else None, spec_stage_h=keep["spec_stage_h"] if keep else None)
        new["pt"] = torch.empty((K + cap_p + cap_a, 48), device=dev)
        if old_pt is not None:
            new["pt"][:K].copy_(old_pt[:K])
            old_pt = None
        new["gt"] = torch.empty((K + cap_p + cap_a, 48), device=dev)
        if K:
            new["gt"][:K].zero_()
        hb = gaussians._hwin_bufs = new
    if hb["rows_h"] is None or hb["rows_h"].shape[0] < need_late:
        cap_h = bucket_size(max(int(need_late * 1.5), 1))
        hb["rows_h"], hb["stage_h"] = pinned_empty((cap_h,), dtype=torch.int32), pinned_empty((cap_h, 48))
    if hb["spec_rows_h"] is None or hb["spec_rows_h"].shape[0] < hb["cap_a"]:
        hb["spec_rows_h"], hb["spec_stage_h"] = pinned_empty((hb["cap_a"],), dtype=torch.int32), pinned_empty((hb["cap_a"], 48))
    return hb


def _tables(gaussians, dev, K=0):
    """Row-indexed scratch (independent of the batch): the slot every touched row lives in right now, two row masks.
    Rows of the HBM-resident prefix [0, K) live in slot r for good."""
    N = gaussians._xyz.shape[0]
    ht = getattr(gaussians, "_hwin_tabs", None)
    if ht is None or ht["N"] != N or ht.get("K", 0) != K:
        ht = gaussians._hwin_tabs = dict(N=N, K=K, cur_slot=torch.zeros((N,), dtype=torch.int32, device=dev),
                                         scratch_slot=torch.zeros((N,), dtype=torch.int32, device=dev),
                                         mark=torch.zeros((N,), dtype=torch.bool, device=dev),
                                         in_spec=torch.zeros((N,), dtype=torch.bool, device=dev),
                                         cam0=torch.zeros((N,), dtype=torch.bool, device=dev))
        if K:
            ht["cur_slot"][:K] = torch.arange(K, dtype=torch.int32, device=dev)
    return ht


# ------------------------------------------------------------------------------------------------------------ stage 1
def _plan(w):
    """Visibility filters, the verdict on what was staged speculatively, the rows grouped by first / last camera, and the
    slot plan: arrival slots (A region) of every touched row, the survivors (rows used by more than one camera) with their
    P slots, the slot every row leaves from."""
    g, dev, bsz, N, K = w.gaussians, w.dev, w.bsz, w.N, w.K
    S.select(w)
    touched = w.touched_all
    w.prefix_rows = None
    if K:
        # sh_hbm_budget_gb: rows [0, K) are resident (slot r = row r, stepped in HBM); only the rest is planned, staged and
        # stepped on the host below.  (touched is ascending: one comparison pass, one host read of the split point)
        n_lo = int((touched < K).sum())
        w.prefix_rows = touched[:n_lo].to(torch.int32)
        touched = touched[n_lo:]
    _lib.STATS.setdefault("host_touched_rows", []).append(int(touched.shape[0]))
    # ---- what was staged for this batch's first camera while the previous batch rendered
    spec = S.take_speculation(w, "_hwin_spec", "_hwin_bufs", id(w.cameras[0]))
    ht = _tables(g, dev, K)
    mark, in_spec, cam0, cur_slot = ht["mark"], ht["in_spec"], ht["cam0"], ht["cur_slot"]
    with _lib.host_region("host_groups"):
        mark.zero_()
        utils.fill_rows(mark, touched, True)
        bitmap = _encode_bitmap(w.filters, N, bsz)  # bit bsz-1-i = camera i

        def group(sp):
            """-> (n_p, staged mask | None, wasted rows, late_all, rows_by_last32, cl)"""
            n_p, staged, wasted = 0, None, touched[:0]
            if sp is not None and sp["n"]:
                n_p = sp["n"]
                P = sp["rows"]
                in_spec.zero_()
                utils.fill_rows(in_spec, P, True)
                cam0.zero_()
                utils.fill_rows(cam0, w.filters[0], True)
                staged = in_spec & cam0                      # staged AND used by the camera they were staged for
                wasted = P[~staged[P]]                       # no gradient of this batch will land on them ...
                wasted = wasted[~mark[wasted]]               # ... unless a later camera stages them again (then re-stamped)
            return (n_p, staged, wasted) + S.group_rows(w, touched, bitmap, staged, 0, ht["scratch_slot"])

        n_p, staged, wasted, late_all, rows_by_last32, cl = group(spec)
        n_first, n_last, n_late = cl[:bsz], cl[bsz:2 * bsz], cl[2 * bsz]
        # multi-use rows: more than one bit of the bitmap set  <=>  first camera < last camera
        multi = (bitmap & (bitmap - 1)) != 0

        def survivors(n_p_, staged_, late_all_, n_first_):
            """Arrival order = [speculative block | late rows by first camera]; -> (rows in arrival order, survivor flag,
            survivors up to the end of each camera's arrivals (device))."""
            late = late_all_[:n_late].long()
            if n_p_:
                arr = torch.cat((spec["rows"].long(), late))
                flag = torch.cat((multi[spec["rows"]] & staged_[spec["rows"]], multi[late]))
            else:
                arr, flag = late, multi[late]
            ends, e = [], n_p_
            for k in range(bsz):
                e += n_first_[k]
                ends.append(e)
            if arr.numel() == 0:
                return arr, flag, torch.zeros((bsz,), dtype=torch.int64, device=dev)
            cs = torch.cumsum(flag, 0, dtype=torch.int64)
            ends_d = torch.tensor(ends, device=dev)               # (tiny, blocking copy: the GPU is idle here anyway)
            cum = torch.where(ends_d > 0, cs[torch.clamp(ends_d - 1, min=0)], torch.zeros_like(ends_d))
            return arr, flag, cum

        arr, flag, cum = survivors(n_p, staged, late_all, n_first)
        _t0 = time.perf_counter()
        cum_h = [int(x) for x in cum.tolist()]               # second (and last) host read of the plan
        _lib.STATS["host_wait_s"] += time.perf_counter() - _t0
        n_surv = cum_h[-1] if cum_h else 0
        need_a = max([n_p + n_first[0]] + n_first[1:])
        hb = _buffers(g, need_a, n_surv, n_late, dev, K)
        if spec is not None and spec["gen"] != hb["gen"]:
            # the tables had to grow: what was staged went with the old ones -- everything is late (re-preparing a current
            # row is the identity; the stamps of the touched rows stay right, the untouched ones are un-stamped below)
            gone = spec["rows"]
            spec = None
            n_p, staged, _w, late_all, rows_by_last32, cl = group(None)
            wasted = gone[~mark[gone]]
            n_first, n_last, n_late = cl[:bsz], cl[bsz:2 * bsz], cl[2 * bsz]
            arr, flag, cum = survivors(0, None, late_all, n_first)
            cum_h = [int(x) for x in cum.tolist()]
            n_surv = cum_h[-1] if cum_h else 0
            hb = _buffers(g, max(n_first), n_surv, n_late, dev, K)
        # ---- slots (table rows: [prefix 0..K | P | A]).  A-region slot of every arrival: base_a + position inside its
        # camera's arrival block
        base_p, base_a = K, K + hb["cap_p"]
        w.base_a = base_a
        if n_p:
            cur_slot[spec["rows"].long()] = base_a + torch.arange(n_p, dtype=torch.int32, device=dev)
        g0 = 0
        for k in range(bsz):
            if n_first[k]:
                base = base_a + (n_p if k == 0 else 0)
                cur_slot[late_all[g0:g0 + n_first[k]].long()] = base + torch.arange(n_first[k], dtype=torch.int32, device=dev)
            g0 += n_first[k]
        surv_pos = torch.nonzero(flag).flatten()              # (size n_surv, known: no extra synchronisation in effect)
        w.surv_rows = arr[surv_pos]
        w.surv_src = cur_slot[w.surv_rows].long()             # their A slots ...
        w.surv_dst = base_p + torch.arange(n_surv, dtype=torch.int64, device=dev)  # ... and their P slots, in arrival order
        w.surv_cum = cum_h
        rbl = rows_by_last32.long()
        leave = cur_slot[rbl].long()
        if n_surv:  # a multi-use row leaves from its P slot
            pslot = ht["scratch_slot"]
            pslot[w.surv_rows] = w.surv_dst.to(torch.int32)
            leave = torch.where(multi[rbl], pslot[rbl].long(), leave)
        w.rows_by_last, w.leave_slots = rbl, leave
        w.n_p, w.n_first, w.n_last, w.n_late, w.n_surv, w.spec, w.hb = n_p, n_first, n_last, n_late, n_surv, spec, hb
        w.late_all, w.mark, w.touched = late_all, mark, touched
        _lib.STATS.setdefault("host_late_rows", []).append(n_late)
        if n_late:
            S.list_to_host(hb["rows_h"], late_all[:n_late])
        # ---- the NEXT batch's first camera on the positions current now; what this batch touches cannot be staged early
        w.spec_rows = None
        if w.hint is not None:
            try:
                f_next, _ = select_filters(w.hint[:1], g._xyz.detach(), g._scaling.detach(), g._rotation.detach())
                sr = f_next[0]
                if K:
                    sr = sr[sr >= K]
                sr = sr[~mark[sr]]
                n_s = int(sr.shape[0])
                if 0 < n_s <= hb["cap_a"]:
                    w.spec_rows = sr
                    S.list_to_host(hb["spec_rows_h"], sr.to(torch.int32))
            except AssertionError:  # the hinted camera sees nothing yet: that batch will complain itself
                w.spec_rows = None
        S.unstamp_wasted(w, wasted)


# ------------------------------------------------------------------------------------------------------------ stage 2
def _start_feeders(w):
    """Feeder thread: per first-use group, the host pool brings the rows up to date (deferred row optimizer) and copies them
    into pinned staging, chunk by chunk; each chunk goes to the bounce table with hipMemcpyAsync on the side stream -- group
    k+1 only once camera k has taken its rows out of the bounce table.  Speculation thread: the hinted next batch's first
    camera, after this batch's own rows."""
    g, hb, bsz = w.gaussians, w.hb, w.bsz
    prev = g._host_grads_event
    w.prev_grads = prev         # (the camera stage makes the default stream wait for it)
    g._host_grads_event = None
    S.start_staging(w)
    step = w.step
    w.arrived = [None] * bsz
    w.bb_free_flag = [threading.Event() for _ in range(bsz)]
    w.bb_free_ev = [None] * bsz
    rows_h, stage_h, bb, n_p = hb["rows_h"], hb["stage_h"], hb["bb"], w.n_p

    # Two helper threads: the PREPARER drives the host pool through the batch's late rows chunk by chunk (deferred row
    # optimizer + copy into pinned staging; it never waits for the GPU, so the pool -- the scarcer resource: 16 CPUs prepare
    # ~170 M rows/s = 33 GB/s against the link's 57 -- works without gaps), the COPIER sends finished chunks to the bounce
    # table in order, the first chunk of group k+1 only once camera k has emptied it.
    chunks = S.chunk_plan(w.n_first)
    prepared = [threading.Event() for _ in chunks]

    def preparer():
        try:
            if prev is not None:  # gradients of the previous batch must have landed before any row is stepped
                prev.synchronize()
            for n_, (_i, c0, c1, _f, _l, _g0) in enumerate(chunks):
                if c1 > c0:
                    S.prepare_chunk(w, rows_h[c0:c1], stage_h[c0:c1], step - 1, 0 if w.skip_opt else step)
                prepared[n_].set()
        except BaseException as e:  # surface in the main thread
            w.err.append(e)
        finally:
            if w.err:
                for ev_ in prepared:
                    ev_.set()

    def feeder():
        try:
            for n_, (i, c0, c1, first, last, g0) in enumerate(chunks):
                prepared[n_].wait()
                if w.err:
                    break
                if first and i > 0 and c1 > c0:  # camera i-1 has emptied the bounce table (device order: its copy's event)
                    w.bb_free_flag[i - 1].wait()
                    if w.err:
                        break
                    w.comm_stream.wait_event(w.bb_free_ev[i - 1])
                if c1 > c0:
                    dst0 = (n_p if i == 0 else 0) + c0 - g0
                    S.copy_rows(w, bb[dst0:dst0 + c1 - c0], stage_h[c0:c1])
                if last:
                    ev = torch.cuda.Event()
                    ev.record(w.comm_stream)
                    w.arrived[i] = ev
                    w.ready[i].set()
        except BaseException as e:  # surface in the main thread
            w.err.append(e)
        finally:
            if w.err:
                for r in w.ready + w.bb_free_flag:  # (the flags: the speculation thread waits for the last one)
                    r.set()

    w.prep_thread = threading.Thread(target=preparer, name="clmgs-hostwin-prepare")
    w.prep_thread.start()
    w.worker = threading.Thread(target=feeder, name="clmgs-hostwin-feeder")
    w.worker.start()
    w.workers = [w.worker, w.prep_thread]
    w.new_spec = None
    if w.spec_rows is not None:
        n_s = int(w.spec_rows.shape[0])
        s_rows_h, s_stage_h = hb["spec_rows_h"][:n_s], hb["spec_stage_h"][:n_s]
        ev_list = torch.cuda.Event()
        ev_list.record(w.default_stream)  # the row list has reached pinned memory once this has passed
        spec_err, spec_done = [], torch.cuda.Event()
        s_chunks = S.chunk_plan([n_s])

        def speculate():
            try:
                w.prep_thread.join()      # after this batch's own rows: the host pool is free from here on
                ev_list.synchronize()
                for _i, c0, c1, *_ in s_chunks:  # brought up to date + copied to pinned staging right away ...
                    S.prepare_chunk(w, s_rows_h[c0:c1], s_stage_h[c0:c1], step, step + 1)
                w.worker.join()           # ... sent once this batch's copies are queued (stream order on the side stream)
                w.bb_free_flag[bsz - 1].wait()  # and the last camera has taken its rows out of the bounce table
                if w.err:
                    return
                w.comm_stream.wait_event(w.bb_free_ev[bsz - 1])
                for _i, c0, c1, *_ in s_chunks:
                    S.copy_rows(w, bb[c0:c1], s_stage_h[c0:c1])
                spec_done.record(w.comm_stream)
            except BaseException as e:
                spec_err.append(e)

        th = threading.Thread(target=speculate, name="clmgs-hostwin-speculate")
        w.new_spec = dict(key=id(w.hint[0]), N=w.N, rows=w.spec_rows, n=n_s, thread=th, gen=hb["gen"], event=spec_done,
                          err=spec_err, rows_h=hb["spec_rows_h"])


# ------------------------------------------------------------------------------------------------------------ stage 3
def _cameras(w):
    """One camera after the other (the mode is bound by the host link, not by the GPU)."""
    from ...fused import train_one_camera
    g, hb = w.gaussians, w.hb
    pt, gt, bb, base_a = hb["pt"], hb["gt"], hb["bb"], w.base_a  # (base_a: first row of the arrival region)
    cur_slot = g._hwin_tabs["cur_slot"]
    ds = w.default_stream
    _zero_small_grads(g)
    if w.spec is not None:
        ds.wait_event(w.spec["event"])      # the speculative block has landed in the bounce table
    if w.new_spec is not None:
        w.new_spec["thread"].start()
    if w.prev_grads is not None:            # the previous batch's hand-back still reads the gradient table
        ds.wait_event(w.prev_grads)
    losses, l0, c_prev, ev_out = [], 0, 0, None
    try:
        for k in range(w.bsz):
            with _lib.host_region("wait_rows"):
                w.ready[k].wait()
            if w.err:
                raise w.err[0]
            if w.arrived[k] is not None:
                ds.wait_event(w.arrived[k])
            n_arr = (w.n_p if k == 0 else 0) + w.n_first[k]
            if n_arr:
                pt[base_a:base_a + n_arr].copy_(bb[:n_arr])          # bounce -> this camera's arrival block
            ev = torch.cuda.Event()
            ev.record(ds)
            w.bb_free_ev[k] = ev
            w.bb_free_flag[k].set()                                   # the feeder may send camera k+1's rows
            if ev_out is not None:
                ds.wait_event(ev_out)                                 # camera k-1's hand-back has read its gradient rows
            if n_arr:
                gt[base_a:base_a + n_arr].zero_()
            f = w.filters[k]
            losses.append(train_one_camera(g, w.cameras[k], f, pt, 1, gt, w.background, w.cameras[k].original_image,
                                           sh_index=cur_slot[f]))
            l1 = l0 + w.n_last[k]
            if l1 > l0:
                ev_out = S.send_grads_home(w, gt, w.rows_by_last[l0:l1], w.leave_slots[l0:l1], want_event=True)
            l0 = l1
            # arrivals a later camera uses again: parameters and partial gradient move to their P slot
            c1 = w.surv_cum[k]
            if c1 > c_prev:
                src, dst = w.surv_src[c_prev:c1], w.surv_dst[c_prev:c1]
                clm_kernels._rows("clmgs_rows_gather", pt, pt, dst, src, 0)
                clm_kernels._rows("clmgs_rows_gather", gt, gt, dst, src, 0)
                cur_slot[w.surv_rows[c_prev:c1]] = dst.to(torch.int32)
            c_prev = c1
        S.end_cameras(w, "_hwin_spec")
    finally:  # whatever happens, no helper thread may be left waiting for this thread, or running once it has gone on
        for f in w.bb_free_flag:
            f.set()
        for t in w.workers:
            t.join()
    g._hwin_keep = (w.filters, w.rows_by_last, w.leave_slots, w.surv_rows, w.surv_src, w.surv_dst, w.late_all, w.touched)
    return losses


# ------------------------------------------------------------------------------------- the HBM-resident prefix (budget)
def _prefix_head(w):
    """Before the cameras: the resident rows this batch renders from are brought up to the previous step by the deferred
    row optimizer of the HBM engine (their waiting gradient at its own step, then the zero-gradient steps they skipped;
    consumed gradient rows are cleared, so the cameras accumulate into zeros).  Runs while the host pool prepares the
    first camera's rows."""
    px, g = w.px, w.gaussians
    if px is None:
        return
    K, hb = px["K"], w.hb
    if px["fill"]:  # first batch after a load: the rows themselves (the moments came with hbm_prefix_ensure)
        hb["pt"][:K].copy_(g._parameters.data[:K])
        hb["gt"][:K].zero_()
        px["fill"] = False
    if not w.args.sparse_adam:
        g.hbm_prefix_catch_up(w.prefix_rows, w.step - 1)


def _prefix_tail(w):
    """After the cameras: the resident rows' gradient of this batch waits in the table, stamped with this step (dense Adam:
    applied at the row's next touch / at a flush), or is applied now (sparse_adam: only touched rows ever step)."""
    px, g = w.px, w.gaussians
    if px is None or w.prefix_rows.numel() == 0:
        return
    K, hb, rows = px["K"], w.hb, w.prefix_rows
    if w.skip_opt:  # test hook: the unscaled sums go where the host rows' gradients go, and nothing is left behind
        idx = rows.long()
        clm_kernels._rows("clmgs_rows_gather", w.parameters_grad_buffer[:w.N, :], hb["gt"], idx, idx, 0)
        torch.cuda.synchronize()
        hb["gt"].index_fill_(0, idx, 0.0)
        return
    px["dirty"] = True
    if w.args.sparse_adam:
        opt = g.optimizer.cpu_adam
        gr = opt.param_groups[0]
        clm_kernels.adam_rows(hb["pt"][:K], hb["gt"][:K], px["m"], px["v"], rows, opt._col_lr(w.dev), gr["betas"][0],
                              gr["betas"][1], gr["eps"], w.step, gr["bias_correction"], 1.0 / float(w.bsz), True)
    else:
        utils.fill_rows(px["g_step"], rows.long(), w.step)


def train_one_batch_host_windowed(gaussians, scene, batched_cameras, parameters_grad_buffer, background, pipe_args,
                                  comm_stream, perm_generator, args):
    """-> (losses, ordered_cams, sparsity); see the module docstring."""
    w = S.begin_batch(gaussians, batched_cameras, parameters_grad_buffer, background, comm_stream, perm_generator, args)
    if getattr(args, "reference_camera_order", False):  # (staged is the FIRST camera's share: that order picks it only now)
        w.hint = None
    w.px = gaussians.hbm_prefix_ensure()  # (sh_hbm_budget_gb; a first call flushes the host rows and loads the prefix)
    w.K = w.px["K"] if w.px is not None else 0
    with torch.no_grad():
        _plan(w)
        _start_feeders(w)
        _prefix_head(w)
        losses = _cameras(w)
        _prefix_tail(w)
    return S.finish_batch(w, losses)
