"""Host-resident SH rows staged as the UNION of a batch's rows (sh_residency="host", host_staging="batch").

What the reference's retention pipeline and cpu-adam thread do (strategies/clm_offload/engine.py:494-508, 622-641, 789-825,
301-335), re-shaped around what this machine's host link and host cores reward; rounds 2-5's form of the mode, kept beside
the per-camera windows of host_window.py (the default: the same link traffic from half the staging memory).

* Every row the batch touches crosses the link ONCE per direction (the minimum the H / D / G retention sets aim at, reached
  without camera re-ordering): the union of the batch's filters is staged, grouped by the camera that uses a row FIRST
  (host -> GPU) and LAST (GPU -> host), so camera k renders as soon as its own new rows have arrived while the rows only
  later cameras need are still being prepared, and a row's gradient leaves right after the last camera that contributes.
* Host -> GPU: a feeder thread drives the host thread pool, which brings the touched rows up to date (DEFERRED row
  optimizer: the gradient a row received in an earlier batch is applied, and the zero-gradient Adam steps it has skipped
  since are replayed, only now -- one read and one write of p / m / v per touched row and batch, where the dense reference
  optimizer streams all N rows every batch) and copies them into a contiguous pinned staging buffer, chunk by chunk; each
  finished chunk goes to the GPU with a hipMemcpyAsync on the side stream (SDMA engine: no compute unit is taken from the
  renderer) while the pool works on the next chunk.
* SPECULATIVE PREFETCH (engine.hint_next_batch): the host pool is busy for the first ~60 % of a batch and the link for less;
  the rows of the NEXT batch that the present one does not touch (their state is final until then) are prepared and shipped
  in that idle time into the second staging table.  When the next batch arrives, its exact selection is compared with what
  was staged: only the LATE rows (touched by both batches: their gradient had to come home first -- plus the few a position
  update moved into view) go through the feeder at batch time, so the first camera waits for a third of its rows.
* The cameras render from / accumulate into GPU staging tables ([T,48] parameters and gradients, row -> slot through an
  index the fused front end follows).
* GPU -> host: zero-copy scatter STORES of the gradient rows into the pinned gradient table (plain stores, no
  read-modify-write over the link, no host pass), on a second side stream; they wait there, stamped with this batch's step,
  until the row is needed again.

Four stages, as in host_window.py: plan (filters, verdict on the speculation, row groups, slots) -> feeders (the two helper
threads) -> cameras -> the small attributes' optimizer step.
"""
import threading

import torch

from ... import _lib, utils
from ...gsplat import bucket_size
from ...host import pinned_empty
from ..base_engine import select_filters
from . import host_stages as S
from .engine import _encode_bitmap, _zero_small_grads


def _host_tables(gaussians, dev):
    """Row-indexed scratch of the host-resident mode (independent of the batch size): row -> slot, two row masks."""
    N = gaussians._xyz.shape[0]
    ht = getattr(gaussians, "_host_tabs", None)
    if ht is None or ht["N"] != N:
        ht = gaussians._host_tabs = dict(N=N, slot_of=torch.zeros((N,), dtype=torch.int32, device=dev),
                                         mark=torch.zeros((N,), dtype=torch.bool, device=dev),
                                         in_spec=torch.zeros((N,), dtype=torch.bool, device=dev))
    return ht


def _host_buffers(gaussians, T, dev):
    """Per-batch buffers of the host-resident mode, kept between batches (bucketed capacity):
    pinned row lists + pinned staging rows on the host (one set for the batch's late rows, one for the
    speculative rows of the next batch), TWO staging parameter tables on the GPU (the batch in flight renders
    from one while the next batch's speculative rows land in the other) and the gradient staging table.
    `gen` counts re-allocations: rows staged into an older generation are gone."""
    hb = getattr(gaussians, "_host_bufs", None)
    N = gaussians._xyz.shape[0]
    if hb is None or hb["cap"] < T or hb["N"] != N:
        # Two capacities.  DEVICE tables (they count against the GPU peak of the offloading mode): 8 % over the need,
        # grown when a batch exceeds them.  PINNED host twins: 50 % over the need -- host memory is cheap, and a new
        # pinned table is a hipHostMalloc of 2 GB at 28 M (300+ ms: ONE such re-allocation inside a 20-batch run was
        # 21 of the 24 ms of average "host_groups" time rounds 2-3 reported); they are kept when only the device tables
        # grow.  The union of a batch's filters varies by several percent from batch to batch (shuffled cameras), and
        # staged-but-unused rows of a hinted batch ride along.
        cap = bucket_size(max(int(T * 1.08), 1))
        gen = hb["gen"] + 1 if hb else 0
        keep_pinned = None
        if hb is not None:
            # The staging tables are written by hipMemcpyAsync issued through ctypes on the side streams (speculative
            # prefetch, feeder): the caching allocator knows nothing of that use, and a dropped speculation is only
            # JOINED (its last copy may still be in flight).  Growing the tables is rare: drain the device before the
            # old blocks go back to the allocator, so no late copy can land in a recycled block.
            torch.cuda.synchronize()
            if hb["N"] == N and hb["rows_h"].shape[0] >= cap:
                keep_pinned = (hb["rows_h"], hb["stage_h"], hb["spec_rows_h"], hb["spec_stage_h"])
            hb.clear()  # the old tables go back to the allocator BEFORE the new ones are requested
        gaussians._host_bufs = None
        if keep_pinned is None:
            cap_h = bucket_size(max(int(T * 1.5), cap))
            keep_pinned = (pinned_empty((cap_h,), dtype=torch.int32), pinned_empty((cap_h, 48)), None, None)
        hb = gaussians._host_bufs = dict(
            cap=cap, N=N, cur=0, gen=gen,
            rows_h=keep_pinned[0], stage_h=keep_pinned[1], spec_rows_h=keep_pinned[2], spec_stage_h=keep_pinned[3],
            sh_stage=[torch.empty((cap, 48), device=dev), None],
            g_stage=torch.empty((cap, 48), device=dev))
    return hb


def _host_spec_buffers(hb, dev):
    """The second staging table + its pinned twin: allocated when the first hint arrives (a caller that never
    hints pays nothing for the speculative prefetch)."""
    if hb["sh_stage"][1] is None:
        hb["sh_stage"][1] = torch.empty((hb["cap"], 48), device=dev)
    if hb["spec_rows_h"] is None:
        cap_h = hb["rows_h"].shape[0]
        hb["spec_rows_h"] = pinned_empty((cap_h,), dtype=torch.int32)
        hb["spec_stage_h"] = pinned_empty((cap_h, 48))


# ------------------------------------------------------------------------------------------------------------ stage 1
def _plan(h):
    """Visibility filters, the verdict on what was staged speculatively, the rows grouped by first / last camera and
    their slots, the staging tables, the row list of the hinted next batch."""
    g, dev, bsz, N = h.gaussians, h.dev, h.bsz, h.N
    S.select(h)
    filters, touched_rows = h.filters, h.touched_all
    # ---- what was staged for this batch while the previous one rendered
    spec = S.take_speculation(h, "_host_spec", "_host_bufs", tuple(sorted(id(c) for c in h.cameras)))
    n_p = spec["n"] if spec is not None else 0
    ht = _host_tables(g, dev)
    slot_of, mark, in_spec = ht["slot_of"], ht["mark"], ht["in_spec"]
    with _lib.host_region("host_groups"):
        mark.zero_()
        utils.fill_rows(mark, touched_rows, True)          # rows this batch touches
        wasted = touched_rows[:0]
        staged_mask = None
        if spec is not None and n_p:
            P = spec["rows"]                                 # staged rows, slot k = P[k]
            wasted = P[~mark[P]]                             # staged but not touched: no gradient will land
            in_spec.zero_()
            utils.fill_rows(in_spec, P, True)
            staged_mask = in_spec
        bitmap = _encode_bitmap(filters, N, bsz)                     # MSB = camera 0
        # (slot_of of the late rows needs slot0 = n_p, which is only final once the staging tables are known not to have
        #  been re-allocated: n_p is re-checked below and the call repeated in that rare case)
        late_all, rows_by_last32, cl = S.group_rows(h, touched_rows, bitmap, staged_mask, n_p, slot_of)
        n_late = cl[2 * bsz]
        hb = _host_buffers(g, n_p + n_late, dev)
        if spec is not None and spec["gen"] != hb["gen"]:
            # the staging tables had to grow: what was staged went with the old ones -- everything is late
            # (re-preparing a current row is the identity; the stamps of the touched rows stay right)
            n_p, spec = 0, None
            late_all, rows_by_last32, cl = S.group_rows(h, touched_rows, bitmap, None, 0, slot_of)
            n_late = cl[2 * bsz]
        if spec is not None and n_p:
            slot_of[spec["rows"]] = torch.arange(n_p, dtype=torch.int32, device=dev)
        h.sh_stage = hb["sh_stage"][hb["cur"]]
        T_slots = n_p + n_late
        _lib.STATS.setdefault("host_late_rows", []).append(n_late)
        h.g_stage = hb["g_stage"][:T_slots]
        h.rows32 = late_all[:n_late]                                 # slot n_p + k holds row rows32[k]
        h.rows_h, h.stage_h = hb["rows_h"][:n_late], hb["stage_h"][:n_late]
        if n_late:
            S.list_to_host(h.rows_h, h.rows32)
        h.sh_index = [slot_of[f] for f in filters]
        h.rows_by_last = rows_by_last32.to(torch.int64)
        h.slots_by_last = slot_of[h.rows_by_last]
        # ---- the NEXT batch's rows on the positions current now; what this batch touches cannot be staged early
        h.spec_rows = None
        t_next = None
        if h.hint is not None:
            try:
                _, t_next = select_filters(h.hint, g._xyz.detach(), g._scaling.detach(), g._rotation.detach())
            except AssertionError:  # a hinted camera sees nothing yet: that batch will complain itself
                t_next = None
        if t_next is not None:
            spec_rows = t_next[~mark[t_next]]
            n_s = int(spec_rows.shape[0])
            del t_next
            if n_s and n_s <= hb["cap"]:
                _host_spec_buffers(hb, dev)
                S.list_to_host(hb["spec_rows_h"], spec_rows.to(torch.int32))
                h.spec_rows = spec_rows
        S.unstamp_wasted(h, wasted)
    h.n_first, h.n_last = cl[:bsz], cl[bsz:2 * bsz]
    h.n_p, h.spec, h.hb = n_p, spec, hb


# ------------------------------------------------------------------------------------------------------------ stage 2
def _start_feeders(h):
    """Feeder thread: prepare + stage + hipMemcpyAsync chunk by chunk, one event per first-use group.  Speculation thread
    (started by the camera stage): the hinted next batch's rows, after this batch's own, in the pool's idle time."""
    g, hb, bsz = h.gaussians, h.hb, h.bsz
    prev = g._host_grads_event
    if prev is not None:  # the previous batch's scatter still reads g_stage
        h.default_stream.wait_event(prev)
    h.g_stage.zero_()
    S.start_staging(h)
    step = h.step
    h.ev_group = [None] * bsz
    n_p, rows_h, stage_h, sh_stage = h.n_p, h.rows_h, h.stage_h, h.sh_stage
    chunks = S.chunk_plan(h.n_first)

    def feeder():
        try:
            if prev is not None:  # gradients of the previous batch must have landed before any row is stepped
                prev.synchronize()
            for i, c0, c1, _first, last, _g0 in chunks:
                if c1 > c0:
                    S.prepare_chunk(h, rows_h[c0:c1], stage_h[c0:c1], step - 1, 0 if h.skip_opt else step)
                    S.copy_rows(h, sh_stage[n_p + c0:n_p + c1], stage_h[c0:c1])
                if last:
                    ev = torch.cuda.Event()
                    ev.record(h.comm_stream)
                    h.ev_group[i] = ev
                    h.ready[i].set()
        except BaseException as e:  # surface in the main thread
            h.err.append(e)
        finally:
            if h.err:
                for r in h.ready:
                    r.set()

    if prev is not None:
        g._host_grads_event = None  # consumed by the feeder above
    h.worker = threading.Thread(target=feeder, name="clmgs-host-feeder")
    h.workers = [h.worker]
    h.worker.start()
    h.new_spec = None
    if h.spec_rows is not None:
        nb = 1 - hb["cur"]
        n_s = int(h.spec_rows.shape[0])
        s_rows_h, s_stage_h, s_dst = hb["spec_rows_h"][:n_s], hb["spec_stage_h"][:n_s], hb["sh_stage"][nb]
        ev_list = torch.cuda.Event()
        ev_list.record(h.default_stream)   # the row list has reached pinned memory once this has passed
        spec_err, spec_done = [], torch.cuda.Event()

        def speculate():
            try:
                h.worker.join()            # after this batch's own rows
                ev_list.synchronize()
                for _i, c0, c1, *_ in S.chunk_plan([n_s]):
                    S.prepare_chunk(h, s_rows_h[c0:c1], s_stage_h[c0:c1], step, step + 1)
                    S.copy_rows(h, s_dst[c0:c1], s_stage_h[c0:c1])
                spec_done.record(h.comm_stream)
            except BaseException as e:
                spec_err.append(e)

        th = threading.Thread(target=speculate, name="clmgs-host-speculate")
        h.new_spec = dict(key=tuple(sorted(id(c) for c in h.hint)), N=h.N, rows=h.spec_rows, n=n_s, buf=nb, thread=th,
                          gen=hb["gen"], event=spec_done, err=spec_err, rows_h=hb["spec_rows_h"])


# ------------------------------------------------------------------------------------------------------------ stage 3
def _cameras(h):
    """One camera after the other (the mode is bound by the host side, not by the GPU: the camera pipeline of the HBM mode
    would only add its per-camera buffers to the peak)."""
    from ...fused import train_one_camera
    g, ds = h.gaussians, h.default_stream
    _zero_small_grads(g)
    if h.spec is not None:
        ds.wait_event(h.spec["event"])  # the staged block has landed
    if h.new_spec is not None:
        h.new_spec["thread"].start()
    losses = []
    l0 = 0
    for i in range(h.bsz):
        with _lib.host_region("wait_rows"):
            h.ready[i].wait()
        if h.err:
            h.worker.join()
            raise h.err[0]
        ds.wait_event(h.ev_group[i])
        losses.append(train_one_camera(g, h.cameras[i], h.filters[i], h.sh_stage, 1, h.g_stage, h.background,
                                       h.cameras[i].original_image, sh_index=h.sh_index[i]))
        l1 = l0 + h.n_last[i]
        if l1 > l0:
            S.send_grads_home(h, h.g_stage, h.rows_by_last[l0:l1], h.slots_by_last[l0:l1])
        l0 = l1
    S.end_cameras(h, "_host_spec")
    g._host_keep = (h.rows32, h.sh_index, h.touched_all, h.filters, h.rows_by_last, h.slots_by_last)
    if h.new_spec is not None:
        h.hb["cur"] = h.new_spec["buf"]      # the next batch renders from the table its staged rows are landing in
    return losses


def train_one_batch_host_batched(gaussians, scene, batched_cameras, parameters_grad_buffer, background, pipe_args,
                                 comm_stream, perm_generator, args):
    """-> (losses, ordered_cams, sparsity); see the module docstring."""
    assert not float(getattr(args, "sh_hbm_budget_gb", 0.0) or 0.0), "sh_hbm_budget_gb is built on host_staging='window'"
    h = S.begin_batch(gaussians, batched_cameras, parameters_grad_buffer, background, comm_stream, perm_generator, args)
    with torch.no_grad():
        _plan(h)
        _start_feeders(h)
        losses = _cameras(h)
    return S.finish_batch(h, losses)


