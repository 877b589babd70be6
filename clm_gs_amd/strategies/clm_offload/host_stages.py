"""What the two staging forms of the host-resident mode (sh_residency="host") do identically: plain functions over the
per-batch state that `host_window.py` (per-camera windows, the default) and `host_batch.py` (the union of the batch) hand
from stage to stage.  The forms keep what differs: the slot plan, the tables, where a chunk lands, what moves between
cameras -- and which thread waits for what.
"""
import ctypes
import threading
import time

import torch

from ... import _lib, clm_kernels, dp, utils
from ..base_engine import select_filters
from .engine import _gpu_adam_step, _mark_batch, order_calculation

CHUNK_ROWS = 262144  # staging granularity: 48 MB of parameter rows per hipMemcpyAsync


def ptr(t):
    return ctypes.c_void_p(t.data_ptr())


class HostBatch:
    """State of one host-resident batch, handed from stage to stage."""


# ------------------------------------------------------------------------------------------------- the batch's two ends
def begin_batch(gaussians, batched_cameras, parameters_grad_buffer, background, comm_stream, perm_generator, args):
    """-> the state of a new batch: model, cameras, streams, sizes, and the hint given for the batch after this one."""
    assert not dp.active(), "camera-DP is built for sh_residency='hbm' (every rank holds a full replica)"
    assert gaussians.deferred_host_rows
    assert getattr(args, "fused_front_end", True), "the host-resident mode runs the fused front end"
    assert args.lr_scale_mode == "sqrt", "Overlap CPUAdam only supports sqrt lr scaling"
    assert not args.stop_update_param, "Overlap CPUAdam does not support stop_update_param"
    s = HostBatch()
    s.gaussians, s.args, s.cameras, s.background = gaussians, args, list(batched_cameras), background
    s.parameters_grad_buffer, s.comm_stream, s.perm_generator = parameters_grad_buffer, comm_stream, perm_generator
    s.bsz, s.N, s.dev = len(batched_cameras), gaussians._xyz.shape[0], gaussians._xyz.device
    s.skip_opt = bool(getattr(args, "debug_skip_optimizer", False))  # test hook, see engine._train_one_batch_hbm
    s.default_stream = torch.cuda.current_stream()
    if getattr(gaussians, "_host_out_stream", None) is None:
        gaussians._host_out_stream = torch.cuda.Stream()
    s.out_stream = gaussians._host_out_stream
    s.hint = getattr(gaussians, "_next_batch_hint", None)
    gaussians._next_batch_hint = None
    if s.skip_opt or not getattr(args, "host_speculative_prefetch", True):
        s.hint = None
    return s


def finish_batch(s, losses):
    """The small attributes' optimizer step and the row optimizer's step counter -> (losses, ordered_cams, sparsity)."""
    gaussians, args = s.gaussians, s.args
    if s.skip_opt:
        torch.cuda.synchronize()
        return losses, s.ordered_cams, s.sparsity
    visibility_mask = None
    if args.sparse_adam:
        visibility_mask = torch.zeros((s.N,), dtype=torch.bool, device=s.dev)
        utils.fill_rows(visibility_mask, s.touched_all, True)
    _gpu_adam_step(gaussians, args, visibility_mask)
    gaussians.invalidate_small_packed()
    _mark_batch(gaussians)
    row_adam = gaussians.optimizer.cpu_adam
    row_adam.global_step = s.step
    row_adam.state[gaussians._parameters]["step"] = s.step
    return losses, s.ordered_cams, s.sparsity


# ------------------------------------------------------------------------------------------------------------ stage 1
def select(s):
    """Visibility filters of the batch's cameras and the union of the rows they touch (s.touched_all, ascending)."""
    g, args = s.gaussians, s.args
    with _lib.host_region("select_filters"):
        s.filters, s.touched_all = select_filters(s.cameras, g._xyz.detach(), g._scaling.detach(), g._rotation.detach())
    _lib.STATS.setdefault("touched_rows", []).append(int(s.touched_all.shape[0]))
    s.sparsity = [len(f) / float(s.N) for f in s.filters]
    s.ordered_cams = list(range(s.bsz))
    if getattr(args, "reference_camera_order", False):  # the reference's TSP order (engine.py:135-298)
        _, s.cameras, s.filters, s.sparsity, s.ordered_cams = order_calculation(
            list(s.filters), list(s.cameras), s.N, s.bsz, s.perm_generator, args)[:5]


def take_speculation(s, spec_attr, bufs_attr, key):
    """What was staged for this batch while the previous one rendered (model attribute `spec_attr`, staged into the
    buffers `bufs_attr`), or None: a speculation for other cameras (`key`), another model size or an older generation of
    the buffers is dropped.  The thread that staged it has finished when this returns."""
    g = s.gaussians
    spec = getattr(g, spec_attr, None)
    gen0 = (getattr(g, bufs_attr, None) or {}).get("gen")
    if spec is not None and (spec["key"] != key or spec["N"] != s.N or spec["gen"] != gen0):
        g.drop_host_speculation()
        spec = None
    setattr(g, spec_attr, None)
    if spec is not None:
        with _lib.host_region("spec_join"):
            spec["thread"].join()
        if spec["err"]:
            raise spec["err"][0]
    return spec


def group_rows(s, touched, bitmap, staged, slot0, slot_of):
    """ONE library call (clmgs_host_groups) groups the rows: the rows still to be staged ("late": not marked in `staged`)
    by the camera that uses them FIRST (slot order), all touched rows by the camera that uses them LAST (hand-back
    order), slot_of[] = slot0 + position of the late rows, and the 2 bsz + 1 group sizes -- two stable one-digit radix
    sorts.  Rounds 2-3 did this with ~60 torch index ops (float64 log2 of the bitmap words, two 64-bit sorts, bincounts,
    boolean selections): 24 ms of a 114 ms batch during which the GPU did little else.
    -> (late rows i32, rows by last camera i32, [n_first[bsz] | n_last[bsz] | n_late] as python ints)"""
    bsz, dev, L = s.bsz, s.dev, _lib.lib()
    T = int(touched.shape[0])
    late_all = torch.empty((T,), dtype=torch.int32, device=dev)
    rows_by_last32 = torch.empty((T,), dtype=torch.int32, device=dev)
    counts = torch.empty((2 * bsz + 1,), dtype=torch.int64, device=dev)
    if T == 0:  # (every touched row is resident in HBM: nothing to stage)
        return late_all, rows_by_last32, [0] * (2 * bsz + 1)
    tb = L.clmgs_host_groups_temp_bytes(T)
    tmp = torch.empty((tb,), dtype=torch.uint8, device=dev)
    _lib.check(L.clmgs_host_groups(_lib.stream(), T, _lib.dptr(touched, torch.int64), _lib.dptr(bitmap),
                                   bitmap.element_size(), bsz,
                                   _lib.dptr(staged.view(torch.uint8), None, True) if staged is not None else None,
                                   int(slot0), _lib.dptr(late_all), _lib.dptr(rows_by_last32), _lib.dptr(slot_of),
                                   _lib.dptr(counts), _lib.dptr(tmp), tb))
    _t0 = time.perf_counter()
    cl = counts.tolist()                                      # one host read: the group sizes
    _lib.STATS["host_wait_s"] += time.perf_counter() - _t0
    return late_all, rows_by_last32, cl


def unstamp_wasted(s, wasted):
    """Rows staged for this batch but not touched by it: they expect no gradient after all."""
    _t0 = time.perf_counter()
    wasted_h = wasted.cpu() if wasted.numel() else None
    _lib.STATS["host_wait_s"] += time.perf_counter() - _t0
    if wasted_h is not None:
        s.gaussians._host_g_step[wasted_h] = 0


def list_to_host(rows_h, rows32):
    """A device row list (int32) into its pinned twin, on the current stream."""
    n = int(rows32.shape[0])
    _lib.check(_lib.lib().clmgs_memcpy_async(_lib.stream(), ptr(rows_h[:n]), ptr(rows32), n * 4, 2))


# ------------------------------------------------------------------------------------------------------------ stage 2
def chunk_plan(n_first, chunk_rows=CHUNK_ROWS):
    """The batch's late rows, in slot order, cut into staging chunks that never span two first-use groups.
    -> [(group, c0, c1, first_of_group, last_of_group, group_start)]; a group without rows gets one empty chunk, so
    every group has exactly one first and one last chunk."""
    chunks = []
    k0 = 0
    for i, n in enumerate(n_first):
        k1 = k0 + n
        cc = list(range(k0, k1, chunk_rows))
        for j, c0 in enumerate(cc):
            chunks.append((i, c0, min(k1, c0 + chunk_rows), j == 0, j == len(cc) - 1, k0))
        if not cc:
            chunks.append((i, k0, k0, True, True, k0))
        k0 = k1
    return chunks


def start_staging(s):
    """The step this batch's rows are brought up to, the side stream ordered after the plan, one `ready` event per
    first-use group for the camera stage, the list the helper threads leave their errors in."""
    s.step = s.gaussians.optimizer.cpu_adam.global_step + 1
    s.comm_stream.wait_stream(s.default_stream)
    s.cs = ctypes.c_void_p(s.comm_stream.cuda_stream)
    s.ready = [threading.Event() for _ in range(s.bsz)]
    s.err = []


def prepare_chunk(s, rows_h, stage_h, to_step, next_g_step):
    """The host pool brings the rows up to `to_step` (deferred row optimizer) and copies them into pinned staging; they
    are stamped as expecting the gradient of step `next_g_step`.  Called from the helper threads."""
    _tp = time.perf_counter()
    s.gaussians.host_rows_prepare(rows_h, stage_h, to_step=to_step, next_g_step=next_g_step, sync_grads=False)
    _lib.STATS["host_prepare_s"] = _lib.STATS.get("host_prepare_s", 0.0) + time.perf_counter() - _tp


def copy_rows(s, dst, src):
    """Pinned staging rows -> device table, hipMemcpyAsync on the side stream."""
    _lib.check(_lib.lib().clmgs_memcpy_async(s.cs, ptr(dst), ptr(src), src.shape[0] * 192, 1))


# ------------------------------------------------------------------------------------------------------------ stage 3
def send_grads_home(s, g_table, rows, slots, want_event=False):
    """Rows whose LAST camera this was: their gradient rows go home now (plain stores, side stream).
    -> with want_event, the event after which the hand-back has read `g_table`."""
    s.out_stream.wait_stream(s.default_stream)
    with torch.cuda.stream(s.out_stream):
        # (launch width: the kernel is bound by the link -- 51 GB/s of stores -- and its stalled waves take wave slots from
        # the render kernels next to it (preprocess_fwd 0.3 -> 4.7 ms in the trace), but narrowing it to the reference's
        # grid_size_H = 32 / 128 / 512 workgroups measured 101.3 / 100.6 / 101.1 ms per batch against 99.1 at full width:
        # the batch is bound by the link either way)
        clm_kernels._rows("clmgs_rows_gather", s.parameters_grad_buffer[:s.N, :], g_table, rows,
                          slots.to(torch.int64),  # (the batch form's int32 slots are widened on this stream)
                          int(getattr(s.args, "host_scatter_grid", 0)))
        if want_event:
            ev = torch.cuda.Event()
            ev.record(s.out_stream)
            return ev
    return None


def end_cameras(s, spec_attr):
    """The helper threads are done; the next batch waits for this one's gradient rows through `_host_grads_event`, and
    finds what was staged for it under `spec_attr`."""
    g = s.gaussians
    for t in s.workers:
        t.join()
    ev_g = torch.cuda.Event()
    ev_g.record(s.out_stream)
    g._host_grads_event = ev_g
    if s.new_spec is not None:
        setattr(g, spec_attr, s.new_spec)
