"""Engine-internal fast path: one camera forward + loss + backward with NO autograd tape and the
fused front-end kernels (csrc/preprocess.hip).  It computes exactly what the op-by-op chain of
strategies/clm_offload/engine.py:650-742 computes (gather -> activations -> projection -> SH ->
clamp -> isect -> rasterize -> loss -> backward of all of it -> scatter-add -> densification
stats) in 9 launches; the op-by-op path (clm_gs_amd.gsplat / clm_kernels) stays as the API-parity
surface and as the cross-check (tests/test_gpu_engines.py).
"""
import ctypes
import math

import numpy as np
import torch

from . import _lib, utils
from ._lib import check, dptr
from .cameras import (camera_colour, camera_invdepth, camera_loss_mask, camera_pose_grad, camera_sky, check_sky_background,
                      refuse_ortho)
from .clm_kernels import COLOUR, check_depth_prior_args, check_sky, masked_loss_value, sky_acc_add, sky_backward, sky_forward
from .gsplat import _record_counts, bucket_size, empty_bucketed, isect_begin, isect_counts, isect_finish

F32, I32, U8, U16 = torch.float32, torch.int32, torch.uint8, torch.uint16
TILE = 16


def _partial_line_floats():
    """Floats per partial-gradient line of the atomic-free rasterize backward, as the library reports it
    (csrc/common.h PART_F4: 16 = one 64 B line; the 48 B form was measured slower)."""
    global _PART_FLOATS
    if _PART_FLOATS is None:
        _PART_FLOATS = int(_lib.lib().clmgs_rasterize_partials_bytes(1)) // 4
    return _PART_FLOATS


_PART_FLOATS = None


def _cam_host(camera):
    """Host copies of viewmat (row-major world->camera), K and the camera centre, cached.  Every kernel that takes them
    by value is a pinhole one: an orthographic camera is refused here, before anything is enqueued."""
    refuse_ortho(camera, "the fused front end (fused.camera_front)")
    h = getattr(camera, "_clmgs_host", None)
    if h is None:
        vm = camera.world_view_transform.detach().t().contiguous().cpu().numpy().astype(np.float32)
        K = camera.K.detach().cpu().numpy().astype(np.float32) if getattr(camera, "K", None) is not None \
            else camera.create_k_on_gpu().cpu().numpy().astype(np.float32)
        c2w = getattr(camera, "camtoworlds", None)
        if c2w is not None:
            campos = c2w.detach().reshape(-1, 4, 4)[0, :3, 3].cpu().numpy().astype(np.float32)
        else:
            campos = np.linalg.inv(vm.astype(np.float64))[:3, 3].astype(np.float32)
        h = (np.ascontiguousarray(vm.reshape(16)), np.ascontiguousarray(K.reshape(9)),
             np.ascontiguousarray(campos.reshape(3)))
        camera._clmgs_host = h
    return h


def _np(a):
    return a.ctypes.data_as(ctypes.c_void_p)


class _CameraPass:
    """Everything one camera's forward leaves behind for its backward (kept alive by the caller
    until the streams involved have consumed it)."""
    __slots__ = ("V", "cam", "filt", "sh_rows", "sh_by_filter", "small_in", "small_packed", "radii",
                 "packed", "fids", "offsets", "emit_slot", "row_cum", "out", "alphas", "last_ids",
                 "bg", "v_out", "maps", "loss", "ev_loss", "streams", "deg", "aux", "loss_partials",
                 "lambda_dssim", "gt_u8", "background", "isect", "sh_index", "means2d", "n_dev", "antialiased",
                 "loss_mask", "mask_count", "colour", "colour_partials",
                 "invdepth", "depth_weight", "depths", "id_partials", "id_term", "pose_grad",
                 "sky", "v_alphas", "sky_scratch")


def _sptr(torch_stream):
    return ctypes.c_void_p(torch_stream.cuda_stream)


# ---- device-side intersection counts (include/clmgs.h "device-count forms").  The reference reads every
# data-dependent size back before it can go on (base_engine.py:64-69, gsplat's cum[-1].item()); here the
# consumers of a camera's intersection list are enqueued against a PREDICTED capacity and read the true count
# on the device, and the host checks the count later (camera_verify, when it enqueues the camera's backward --
# by then the asynchronous readback has long arrived), redoing the camera exactly if the capacity was exceeded.
# Predictor: decaying maximum of the counts seen at this image size, x `isect_capacity_margin`.
_CAPACITY = {}   # (image size, model) -> decaying maximum of the counts seen
_CAP_HELD = {}   # (image size, model) -> the capacity the buffers are currently built for
_CAP_IDS = __import__("itertools").count(1)


def _cap_key(gaussians, W, H):
    """Predictions are per MODEL and image size: a second scene in the same process (a ground-truth renderer, a
    sub-scene of a test) must not inherit the first one's intersection counts."""
    k = getattr(gaussians, "_clmgs_cap_id", None)
    if k is None:
        k = gaussians._clmgs_cap_id = next(_CAP_IDS)
    return (int(W), int(H), k)


def _observe_count(key, n):
    _CAPACITY[key] = max(int(n), int(0.98 * _CAPACITY.get(key, 0)))


def _capacity_for(key, args):
    """Capacity for the next camera at this image size, with hysteresis: the capacity in use is kept while it
    still leaves 10 % over the largest recent count, and a new one is chosen `isect_capacity_margin` (1.25) above it
    -- buffer sizes then change once per ~15 % of growth of the scene's intersection count instead of at every
    1/8-octave bucket boundary, so a training run does not keep calling hipMalloc (20 ms stalls each on a box whose
    memory has not been touched yet: measured as a 90 ms hiccup in the first process of a fresh box)."""
    seen = _CAPACITY.get(key)
    if not seen or not getattr(args, "device_side_counts", True):
        return None
    margin = float(getattr(args, "isect_capacity_margin", 1.25))
    floor = int(getattr(args, "isect_capacity_floor", 4096))
    held = _CAP_HELD.get(key)
    if held is not None and margin > 1.0 and int(seen * 1.10) + floor <= held <= int(seen * margin * 1.5) + floor:
        return held
    cap = int(seen * margin) + floor
    cap = bucket_size(cap) if cap > 4096 else max(cap, 1)
    _CAP_HELD[key] = cap
    return cap


def camera_forward(gaussians, camera, this_filter, sh_rows, sh_by_filter, background, gt_u8,
                   lambda_dssim=0.2, small_packed=None, streams=None, sh_index=None, exact=True):
    """Projection + binning (stream `front`), alpha-blend forward (stream `raster`), loss forward +
    backward (stream `mem`) of one camera; returns the _CameraPass for camera_backward.  The three
    streams may be one and the same; distinct streams are chained by events, so the caller can put
    all cameras' tile kernels on one low-priority stream and order them RF0 RF1 RB0 RF2 RB1 ...
    (software pipelining over the cameras of a batch: the tile stream never waits for a loss).
    = camera_front (nothing blocks) + camera_forward_finish.
    exact=True (default: forward-only callers -- evaluation-style use, parity checks -- get a COMPLETE image): the host
    waits for the intersection count and sizes the lists exactly.  exact=False: lists built for the predicted capacity
    (device-count forms); the render is only valid once camera_verify / camera_backward has checked the count --
    train_one_camera, which runs the backward right after, passes False."""
    return camera_forward_finish(gaussians, camera_front(
        gaussians, camera, this_filter, sh_rows, sh_by_filter, background, gt_u8, lambda_dssim,
        small_packed, streams, sh_index), exact=exact)


def camera_front(gaussians, camera, this_filter, sh_rows, sh_by_filter, background, gt_u8,
                 lambda_dssim=0.2, small_packed=None, streams=None, sh_index=None):
    """Projection and the first half of the binning (depth order, per-row tile counts, asynchronous
    readback of the intersection count) on stream `front`; no host wait."""
    L = _lib.lib()
    args = utils.get_args()
    W, H = int(utils.get_img_width()), int(utils.get_img_height())
    dev = gaussians._xyz.device
    cur = torch.cuda.current_stream()
    s_front, s_mem, s_raster = streams if streams is not None else (cur, cur, cur)
    p = _CameraPass()
    p.streams = (s_front, s_mem, s_raster)
    V = p.V = int(this_filter.shape[0]) if this_filter is not None else int(gaussians._xyz.shape[0])
    p.cam = _cam_host(camera)
    vm, K, campos = p.cam
    deg = p.deg = int(gaussians.active_sh_degree)
    p.sh_rows, p.sh_by_filter, p.small_packed = sh_rows, sh_by_filter, small_packed
    p.sh_index = sh_index  # int32[V]: SH row of position i in a staging table (host-resident mode)
    p.gt_u8, p.lambda_dssim, p.background = gt_u8, float(lambda_dssim), background
    p.loss_mask, p.mask_count = camera_loss_mask(camera)  # a mask on the camera selects the masked loss kernels
    # a colour stage on the camera -- (kind, param, grad): an exposure row or a bilateral grid -- puts its transform between
    # the tile kernel and the loss (a camera carrying both is refused, here, before anything is enqueued)
    p.colour, p.colour_partials = camera_colour(camera), None
    # an inverse-depth prior on the camera (depth regularisation): the camera is rendered with a fourth channel, the
    # inverse depth, and trained with the L1 term; without one, not one launch differs.  Refused with absgrad, here,
    # before anything is enqueued.
    p.invdepth = camera_invdepth(camera) if check_depth_prior_args(camera) else None
    p.depth_weight, p.id_partials, p.id_term, p.depths = 0.0, None, None, None
    if p.invdepth is not None:
        raw = p.invdepth[0]
        if tuple(raw.shape) != (H, W) or raw.dtype != U16:
            raise _lib.ClmgsError(f"camera.invdepth must be uint16 [{H}, {W}], got {raw.dtype} {tuple(raw.shape)}")
        p.depth_weight = utils.depth_l1_weight()  # of the current iteration, read once per camera
    # a pose-gradient buffer on the camera (pose refinement): camera_backward launches the camera-gradient kernel after the
    # row backward; without one, not one launch differs.  Refused with a depth prior, here, before anything is enqueued:
    # the fourth channel's cotangent reaches the positions outside the projection VJP.
    p.pose_grad = camera_pose_grad(camera)
    if p.pose_grad is not None:
        if p.invdepth is not None:
            raise ValueError("a camera carries both a pose-gradient buffer and an inverse-depth prior: pose refinement is not "
                             "supported with the depth regularisation")
        if tuple(p.pose_grad.shape) != (15,) or p.pose_grad.dtype != F32 or not p.pose_grad.is_contiguous():
            raise _lib.ClmgsError(f"camera.pose_grad must be contiguous float32 [15], got {p.pose_grad.dtype} "
                                  f"{tuple(p.pose_grad.shape)}")
        if sh_index is not None or not sh_rows.is_cuda:
            raise ValueError("pose refinement needs the SH rows in HBM (sh_residency=\"hbm\")")
    # a sky on the camera -- (map, accumulator or None) -- is composited behind the tile kernel's render, which then runs
    # with NO background; without one, not one launch differs.  Refused with a pose-gradient buffer (camera_sky) and with
    # a non-zero background, here, before anything is enqueued.
    p.sky, p.v_alphas, p.sky_scratch = camera_sky(camera), None, None
    if p.sky is not None:
        check_sky(p.sky[0], "camera.sky")
        check_sky_background(background)
    p.antialiased = utils.antialiased()  # the backward follows the mode its forward ran in
    filt = p.filt = this_filter.contiguous() if this_filter is not None else None  # None: all rows
    if small_packed is not None:
        small_in = (dptr(small_packed, F32), None, None, None)
        p.aux = (small_packed,)
    else:
        xyz, opa = gaussians._xyz.detach(), gaussians._opacity.detach()
        sca, rot = gaussians._scaling.detach(), gaussians._rotation.detach()
        small_in = (dptr(xyz, F32), dptr(opa, F32), dptr(sca, F32), dptr(rot, F32))
        p.aux = (xyz, opa, sca, rot)
    p.small_in = small_in
    tw, th = math.ceil(W / float(TILE)), math.ceil(H / float(TILE))
    with torch.cuda.stream(s_front):
        # data-dependent sizes -> bucketed capacity (gsplat.bucket_size): no hipMalloc mid-step
        radii = p.radii = empty_bucketed(V, (), I32, dev).reshape(1, V)
        means2d = empty_bucketed(V, (2,), F32, dev).reshape(1, V, 2)
        depths = empty_bucketed(V, (), F32, dev).reshape(1, V)
        packed = p.packed = empty_bucketed(V, (16,), F32, dev)
        # gsplat's rasterize_mode="antialiased" (args.rasterize_mode, read once per camera): the aa entries, whose records
        # carry sigmoid(opacity) * compensation
        check((L.clmgs_preprocess_aa_fwd if p.antialiased else L.clmgs_preprocess_fwd)(
            _sptr(s_front), V, dptr(filt, torch.int64, True), *small_in,
            dptr(sh_rows, F32, allow_host=True), int(sh_by_filter), _np(vm), _np(K), _np(campos), W, H, deg,
            0.3, 0.01, 1e10, float(getattr(args, "radius_clip", 0.0)), dptr(radii), dptr(means2d),
            dptr(depths), None, None, None, dptr(packed),  # conics/colours/opacities live in `packed`
            dptr(sh_index, I32, True)))
        if p.invdepth is not None:  # 1/z into the records' spare word: the fourth colour of the 4-channel tile kernels
            check(L.clmgs_invdepth_pack(_sptr(s_front), V, dptr(radii), dptr(depths), dptr(packed)))
            p.depths = depths
        # binning route: "tile" (default, csrc/isect3.hip: no global sort) | "sort" (csrc/isect.hip: depth sort + tile sort);
        # identical lists (tests/test_gpu_ops.py)
        p.isect = isect_begin("tile" if getattr(args, "binning", "tile") == "tile" else "sort", means2d, radii, depths, TILE,
                              tw, th, want_slots=True, packed=packed if getattr(args, "exact_tile_cull", True) else None)
        p.aux = p.aux + (means2d, depths)
        p.means2d = means2d  # [1,V,2] pixel centres (parity checks read them; kept alive through p.aux)
    return p


def camera_forward_finish(gaussians, p, exact=False):
    """Second half of the binning, alpha-blend forward, loss forward + backward.  With a capacity prediction
    for this image size (device-side counts, see above) nothing is waited for; otherwise (first cameras of a
    run, `exact`, device_side_counts=False) the host waits for the intersection count and sizes exactly.
    OBLIGATION of the caller when a capacity was used (p.n_dev is not None): the image, loss and lists are built
    from capacity-sized lists whose overflow is DROPPED -- call camera_verify(gaussians, p) (camera_backward does)
    before consuming or accumulating anything of this camera; it redoes the forward exactly if the count exceeded
    the capacity."""
    L = _lib.lib()
    args = utils.get_args()
    W, H = int(utils.get_img_width()), int(utils.get_img_height())
    dev = gaussians._xyz.device
    s_front, s_mem, s_raster = p.streams
    V, packed, background, gt_u8, lambda_dssim = p.V, p.packed, p.background, p.gt_u8, p.lambda_dssim
    tw, th = math.ceil(W / float(TILE)), math.ceil(H / float(TILE))
    cap = None if (exact or V == 0) else _capacity_for(_cap_key(gaussians, W, H), args)
    with torch.cuda.stream(s_front):
        with _lib.host_region("fwd_isect"):
            p.fids, p.offsets, _, (p.emit_slot, p.row_cum) = isect_finish(p.isect, capacity=cap)
        if cap is None:
            p.isect, p.n_dev = None, None
            if V:
                _observe_count(_cap_key(gaussians, W, H), p.fids.numel())
        else:
            p.n_dev = p.isect.totals  # int64[2] on the device: {emitted, reference}; p.isect stays for camera_verify
        nch = 4 if p.invdepth is not None else 3  # with a prior: [H,W,4], channel 3 = the inverse depth
        p.out = torch.empty((H, W, nch), dtype=F32, device=dev)
        p.alphas = torch.empty((H, W), dtype=F32, device=dev)
        p.last_ids = torch.empty((H, W), dtype=I32, device=dev)
        p.bg = background.reshape(1, 3).to(F32).contiguous() if background is not None and p.sky is None else None
        if nch == 4 and p.bg is not None:  # the inverse depth's background is 0
            p.bg = torch.cat([p.bg, p.bg.new_zeros((1, 1))], dim=1).contiguous()
    if s_raster is not s_front:
        s_raster.wait_stream(s_front)
    n_isects = p.fids.numel()
    raster_fwd, raster_fwd_dev = (L.clmgs_rasterize4_fwd, L.clmgs_rasterize4_fwd_dev) if nch == 4 else \
        (L.clmgs_rasterize_fwd, L.clmgs_rasterize_fwd_dev)
    if p.n_dev is None:
        check(raster_fwd(_sptr(s_raster), 1, V, n_isects, None, None, None, None, dptr(p.bg, F32, True),
                         W, H, TILE, tw, th, dptr(p.offsets), dptr(p.fids), dptr(packed), dptr(p.out),
                         dptr(p.alphas), dptr(p.last_ids)))
    else:
        check(raster_fwd_dev(_sptr(s_raster), 1, V, n_isects, dptr(p.n_dev), dptr(p.bg, F32, True),
                             W, H, TILE, tw, th, dptr(p.offsets), dptr(p.fids), dptr(packed), dptr(p.out),
                             dptr(p.alphas), dptr(p.last_ids)))
    if s_mem is not s_raster:
        ev = torch.cuda.Event()
        ev.record(s_raster)
        s_mem.wait_event(ev)
    with torch.cuda.stream(s_mem):
        # loss forward + backward straight on the [H,W,3] ([H,W,4] with a prior) buffer viewed as [3,H,W]
        slots = L.clmgs_loss_slots()
        partials = torch.zeros((slots, 2), dtype=F32, device=dev)
        maps = p.maps = torch.empty((3, 3, H, W), dtype=F32, device=dev)
        sc, sy, sx = 1, nch * W, nch
        gt = gt_u8.contiguous()
        sm = _sptr(s_mem)
        mask = p.loss_mask
        if p.sky is not None:
            # the sky behind the render, IN PLACE on p.out (rendered with no background): the colour stage and the loss
            # read the composite, and so does the colour stage's backward; the tile backward never reads p.out
            sky_forward(sm, H, W, dptr(p.out), (sc, sy, sx), p.alphas, p.cam[0], p.cam[1], p.sky[0],
                        dptr(p.out), (sc, sy, sx))
        img = p.out  # what the loss sees
        if p.colour is not None:
            # the camera's colour stage (exposure transform, or bilateral grid sliced per pixel) into a second buffer of
            # p.out's shape, allocated and used on s_mem only (like the maps); p.out stays: the stage's backward reads it.
            # With a depth prior the fourth word of a pixel is not touched.
            kind, param, _ = p.colour
            COLOUR[kind].check(param, f"camera.{kind}")
            img = torch.empty_like(p.out)
            COLOUR[kind].forward(sm, H, W, dptr(p.out), (sc, sy, sx), param, dptr(img), (sc, sy, sx))
        if mask is None:
            check(L.clmgs_l1_ssim_loss_fwd(sm, H, W, dptr(img), sc, sy, sx, dptr(gt, U8), dptr(partials),
                                           dptr(maps[0]), dptr(maps[1]), dptr(maps[2])))
        else:
            if tuple(mask.shape) != (H, W):
                raise _lib.ClmgsError(f"loss_mask is {tuple(mask.shape)}, the image is {(H, W)}")
            check(L.clmgs_l1_ssim_loss_masked_fwd(sm, H, W, dptr(img), sc, sy, sx, dptr(gt, U8), dptr(partials),
                                                  dptr(maps[0]), dptr(maps[1]), dptr(maps[2]), dptr(mask, U8)))
        # the loss VALUE is not needed by the backward (d loss / d loss = 1): its handful of tiny
        # reduction kernels is enqueued by camera_loss(), off the forward -> backward chain
        p.loss_partials, p.loss = partials, None
        one = getattr(gaussians, "_clmgs_one", None)
        if one is None or one.device != dev:
            one = gaussians._clmgs_one = torch.ones((1,), dtype=F32, device=dev)
        p.v_out = torch.empty_like(p.out)
        if mask is None:
            check(L.clmgs_l1_ssim_loss_bwd(sm, H, W, dptr(img), sc, sy, sx, dptr(gt, U8), dptr(one),
                                           float(lambda_dssim), dptr(maps[0]), dptr(maps[1]), dptr(maps[2]),
                                           dptr(p.v_out)))
        else:
            check(L.clmgs_l1_ssim_loss_masked_bwd(sm, H, W, dptr(img), sc, sy, sx, dptr(gt, U8), dptr(one),
                                                  float(lambda_dssim), dptr(maps[0]), dptr(maps[1]), dptr(maps[2]),
                                                  dptr(p.v_out), dptr(mask, U8)))
        if p.colour is not None:
            # dL/dy -> dL/dx IN PLACE on p.v_out (no third image buffer) + one row of partial sums per workgroup (12 floats for
            # an exposure row, a slab row for a grid); the rows wait on the pass: camera_backward adds them to the camera's
            # gradient view once camera_verify has accepted THIS forward (a forward repeated for capacity replaces them)
            kind, param, _ = p.colour
            p.colour_partials = COLOUR[kind].backward(sm, H, W, dptr(p.out), (sc, sy, sx), param, dptr(p.v_out), (sc, sy, sx),
                                                      dptr(p.v_out), (sc, sy, sx), dev)
        p.v_alphas, p.sky_scratch = None, None
        if p.sky is not None and p.sky[1] is not None:
            # p.v_out is dL/d(composite) here: dL/dalpha for the tile backward, and the map's gradient into a zeroed
            # fixed-point scratch of this pass -- camera_backward adds it to the camera's accumulator once camera_verify
            # has accepted THIS forward (a forward repeated for capacity replaces it).  Allocated and used on s_mem only.
            p.v_alphas = torch.empty((H, W), dtype=F32, device=dev)
            p.sky_scratch = torch.zeros(p.sky[0].shape, dtype=torch.int64, device=dev)
            sky_backward(sm, H, W, dptr(p.v_out), (sc, sy, sx), p.alphas, p.cam[0], p.cam[1], p.sky[0], p.v_alphas,
                         p.sky_scratch)
        if p.invdepth is not None:
            # the depth term, after the loss (and exposure) backward on the same stream, into the same [H,W,4] cotangent:
            # they wrote words 0..2 of every pixel through their strides, this writes word 3.  One partial sum per
            # workgroup; camera_loss finishes them (a forward repeated for capacity replaces the rows: counted once).
            raw, scale, offset = p.invdepth
            p.id_partials = torch.empty((int(L.clmgs_invdepth_partials_rows(H, W)),), dtype=F32, device=dev)
            p.id_term = None
            ch3 = 3 * p.out.element_size()
            check(L.clmgs_invdepth_l1_fwd_bwd(sm, H, W, ctypes.c_void_p(p.out.data_ptr() + ch3), 4 * W, 4, dptr(raw, U16),
                                              scale, offset, dptr(mask, U8, True), p.depth_weight,
                                              ctypes.c_void_p(p.v_out.data_ptr() + ch3), 4 * W, 4, dptr(p.id_partials)))
        p.ev_loss = None
        if s_raster is not s_mem:
            p.ev_loss = torch.cuda.Event()
            p.ev_loss.record(s_mem)
        p.aux = p.aux + (gt, one, partials) + ((mask,) if mask is not None else ())
        # the three derivative maps (573 MB at 4K) were allocated, written and read on s_mem only: dropping
        # them here hands the block back to that stream's pool, where the next camera's maps reuse it in
        # stream order (they used to stay alive until the next batch: 4 x 573 MB).  The exposure-corrected image goes
        # the same way: nothing after the loss backward reads it.
        p.maps = None
        del maps, img
    return p


def camera_loss(p):
    """The camera's loss value (0-dim tensor) from the partial sums its forward left; enqueued on
    the CURRENT stream, which must be ordered after the camera's loss kernel."""
    if p.loss is None:
        W, H = int(utils.get_img_width()), int(utils.get_img_height())
        if p.loss_mask is None:
            tot = p.loss_partials.sum(dim=0) / float(3 * H * W)
            p.loss = ((1.0 - p.lambda_dssim) * tot[0] + p.lambda_dssim * (1.0 - tot[1])).detach()
        else:  # sums over counted pixels; the count is a host integer
            tot = p.loss_partials.sum(dim=0)
            p.loss = masked_loss_value(tot[0], tot[1], p.lambda_dssim, p.mask_count, H, W).detach()
        if p.id_partials is not None:  # L_rgb + L_depth: the partial sums of the forward that was accepted, finished once
            L = _lib.lib()
            total = torch.empty((1,), dtype=F32, device=p.id_partials.device)
            check(L.clmgs_invdepth_finish(_lib.stream(), int(p.id_partials.numel()), dptr(p.id_partials), dptr(total)))
            p.id_term = (total[0] * (p.depth_weight / float(H * W))).detach()
            p.loss = p.loss + p.id_term
    return p.loss


def camera_verify(gaussians, p):
    """Device-count form: the camera's intersection count against the capacity its lists were built for.  Called
    before anything of the camera is accumulated (camera_backward); the readback was issued a whole forward ago.
    Exceeded capacity (a view much denser than any seen so far): the camera's forward is repeated exactly."""
    c = p.isect
    if c is None or p.n_dev is None:
        return
    W, H = int(utils.get_img_width()), int(utils.get_img_height())
    n, n_ref = isect_counts(c)
    _observe_count(_cap_key(gaussians, W, H), n)
    if n <= p.fids.numel():
        _record_counts(n, n_ref)
        p.isect = None
        return
    _lib.STATS["isect_capacity_redo"] = _lib.STATS.get("isect_capacity_redo", 0) + 1
    for st in set(p.streams):
        st.synchronize()
    p.n_dev = None
    camera_forward_finish(gaussians, p, exact=True)


def camera_backward(gaussians, p, g_sh_rows, small_grad=None, update_stats=True, stats_delta=None,
                    stats_only_visible=False, visibility_out=None, accumulate_after=None, sh_stamp=None,
                    cur_step=0, release=False):
    """Alpha-blend backward (stream `raster`) + projection / SH backward (stream `mem`) of the
    camera whose forward left `p`.  Gradients are ACCUMULATED (see train_one_camera); with `sh_stamp`
    (int32 [N], the deferred optimizer's per-row gradient-step table) + `cur_step` the SH gradient rows
    are STORED on their first touch of the step and stamped (clmgs_preprocess_bwd)."""
    L = _lib.lib()
    args = utils.get_args()
    W, H = int(utils.get_img_width()), int(utils.get_img_height())
    dev = gaussians._xyz.device
    camera_verify(gaussians, p)
    s_front, s_mem, s_raster = p.streams
    if p.colour_partials is not None:
        # the colour stage's gradient of the forward camera_verify has just accepted (an overflowed forward was repeated exactly
        # and left its own rows): summed in a fixed order and added ONCE, on the stream that wrote the rows.  Allocated,
        # written and read on s_mem only.
        kind, param, grad = p.colour
        if grad is not None:
            COLOUR[kind].finish(_sptr(s_mem), H, W, param, p.colour_partials, grad)
        p.colour_partials = None
    if p.sky_scratch is not None:
        # the map's gradient of the accepted forward, added ONCE, in integers, on the stream that wrote the scratch
        with torch.cuda.stream(s_mem):
            sky_acc_add(_sptr(s_mem), p.sky_scratch, p.sky[1])
        p.sky_scratch = None
    V = p.V
    vm, K, campos = p.cam
    tw, th = math.ceil(W / float(TILE)), math.ceil(H / float(TILE))
    n_isects = p.fids.numel()
    if p.small_packed is not None:
        assert small_grad is not None
        small_out = (dptr(small_grad, F32), None, None, None)
    else:
        small_out = (dptr(gaussians._xyz.grad, F32), dptr(gaussians._opacity.grad, F32),
                     dptr(gaussians._scaling.grad, F32), dptr(gaussians._rotation.grad, F32))
    with torch.cuda.stream(s_raster):
        # atomic-free accumulation: the tile kernel stores one 64 B line per intersection (row-ordered
        # slots); clmgs_preprocess_bwd sums each row's contiguous range while it gathers the row.
        # Allocated on the stream of its WRITER (the caching allocator orders reuse by allocation stream).
        partials = empty_bucketed(max(n_isects, 1), (_partial_line_floats(),), F32, dev)
    if p.ev_loss is not None:
        s_raster.wait_event(p.ev_loss)
    # gsplat's absgrad (args.absgrad, read once): the three abs entries, whose lines carry sum_p |dL_p/dmean2d| in words
    # 10 and 11 and whose row kernel takes the densification statistic from that pair
    absgrad = bool(getattr(args, "absgrad", False))
    raster_bwd, raster_bwd_dev = (L.clmgs_rasterize_abs_bwd, L.clmgs_rasterize_abs_bwd_dev) if absgrad else \
        (L.clmgs_rasterize_bwd, L.clmgs_rasterize_bwd_dev)
    if p.invdepth is not None:  # four channels on the slot route: word 9 of every partial line is dL/d(1/z) of its tile
        assert not absgrad  # refused by camera_front
        raster_bwd, raster_bwd_dev = L.clmgs_rasterize4_slot_bwd, L.clmgs_rasterize4_bwd_dev
    if p.n_dev is None:
        check(raster_bwd(_sptr(s_raster), 1, V, n_isects, dptr(p.packed), dptr(p.bg, F32, True), W, H,
                         TILE, tw, th, dptr(p.offsets), dptr(p.fids), dptr(p.alphas), dptr(p.last_ids),
                         dptr(p.v_out), dptr(p.v_alphas, F32, True), None, None, None, None, None,
                         dptr(p.emit_slot), dptr(p.row_cum), dptr(partials), *((None,) if absgrad else ())))
    else:
        check(raster_bwd_dev(_sptr(s_raster), 1, V, n_isects, dptr(p.n_dev), dptr(p.packed),
                             dptr(p.bg, F32, True), W, H, TILE, tw, th, dptr(p.offsets), dptr(p.fids),
                             dptr(p.alphas), dptr(p.last_ids), dptr(p.v_out), dptr(p.v_alphas, F32, True),
                             dptr(p.emit_slot), dptr(p.row_cum), dptr(partials)))
    if s_mem is not s_raster:
        ev = torch.cuda.Event()
        ev.record(s_raster)
        s_mem.wait_event(ev)
    stats = update_stats and (not args.disable_auto_densification) and \
        utils.get_cur_iter() <= args.densify_until_iter
    if stats and stats_delta is not None:  # [N,4] delta table (see GaussianModelCLMOffload.stats_delta)
        stat_ptrs = (dptr(stats_delta, F32), None, None)
    else:
        stat_ptrs = (dptr(gaussians.max_radii2D if stats else None, F32, True),
                     dptr(gaussians.xyz_gradient_accum if stats else None, F32, True),
                     dptr(gaussians.denom if stats else None, F32, True))
    with torch.cuda.stream(s_mem):
        if accumulate_after is not None:
            s_mem.wait_event(accumulate_after)
        if visibility_out is not None:
            visibility_out |= (p.radii.reshape(-1) > 0)
        if p.antialiased:
            pre_bwd = L.clmgs_preprocess_aa_abs_bwd if absgrad else L.clmgs_preprocess_aa_bwd
        else:
            pre_bwd = L.clmgs_preprocess_abs_bwd if absgrad else L.clmgs_preprocess_bwd
        check(pre_bwd(
            _sptr(s_mem), V, dptr(p.filt, torch.int64, True), *p.small_in, dptr(p.sh_rows, F32, allow_host=True),
            int(p.sh_by_filter), _np(vm), _np(K), _np(campos), W, H, p.deg, 0.3, dptr(p.radii),
            None, *small_out, dptr(g_sh_rows, F32, allow_host=True),
            *stat_ptrs, None, int(bool(stats_only_visible)), dptr(partials), dptr(p.row_cum),
            dptr(p.sh_index, I32, True), dptr(sh_stamp, I32, True), int(cur_step), *((None,) if absgrad else ())))
        if p.pose_grad is not None:
            # the camera's own gradient, from the same lines and rows, directly behind the row backward on the memory
            # stream (partials, row_cum, radii and the row inputs are alive here): one row of 16 floats per workgroup,
            # allocated, written and read on s_mem only, summed in a fixed order and added to the camera's buffer ONCE
            pose_rows = torch.empty((int(L.clmgs_pose_grad_partials_rows(V)), 16), dtype=F32, device=dev)
            check(L.clmgs_pose_grad(
                _sptr(s_mem), V, dptr(p.filt, torch.int64, True), *p.small_in, dptr(p.sh_rows, F32),
                int(p.sh_by_filter), _np(vm), _np(K), _np(campos), W, H, p.deg, 0.3, dptr(p.radii), None,
                dptr(partials), dptr(p.row_cum), None, int(bool(p.antialiased)), dptr(pose_rows)))
            check(L.clmgs_pose_grad_finish(_sptr(s_mem), int(pose_rows.shape[0]), dptr(pose_rows), dptr(p.pose_grad, F32)))
            del pose_rows
        if p.invdepth is not None:
            # dL/d(1/z) -> the xyz gradient, on the memory stream directly after the camera's preprocess backward: that
            # kernel's first-touch store has initialised the row for this step (and accumulated into it otherwise), so
            # a plain read-modify-write of the row's three xyz words is correct here
            check(L.clmgs_invdepth_rows_bwd(_sptr(s_mem), V, dptr(p.filt, torch.int64, True), dptr(p.radii),
                                            dptr(p.depths), _np(vm), dptr(partials), dptr(p.row_cum), None,
                                            small_out[0], 1 if p.small_packed is not None else 0))
    # partials (64 B per intersection, 576 MB at 4K) and the loss cotangent image are dead once the two
    # kernels above have run: hand them back now instead of at the next batch.  Each was used on a second
    # stream (partials: written on s_raster, read on s_mem; v_out: written on s_mem, read on s_raster), so
    # the allocator is told (record_stream) and delays the reuse until that stream has passed this point.
    if s_mem is not s_raster:
        partials.record_stream(s_mem)
        p.v_out.record_stream(s_raster)
        if p.v_alphas is not None:
            p.v_alphas.record_stream(s_raster)
    del partials
    p.v_out, p.v_alphas = None, None
    if release:
        # Nothing reads this camera's forward outputs after the two kernels above.  They were allocated on the
        # front stream and used on the tile and memory streams: tell the allocator, then drop them, so the next
        # cameras reuse the blocks in stream order instead of the whole batch's outputs staying alive until the
        # next batch (4 x 0.7 GB at 4K).  Only what camera_loss() needs is kept.
        for name in ("radii", "packed", "fids", "offsets", "emit_slot", "row_cum", "out", "alphas", "last_ids", "n_dev",
                     "depths"):
            t = getattr(p, name)
            if t is not None:
                for st in {s_mem, s_raster} - {s_front}:
                    t.record_stream(st)
                setattr(p, name, None)
        for t in p.aux:
            if isinstance(t, torch.Tensor) and t.is_cuda and t is not p.loss_partials:
                for st in {s_mem, s_raster} - {s_front}:
                    t.record_stream(st)
        p.aux = (p.loss_partials,)
        p.means2d = None
    return p


def train_one_camera(gaussians, camera, this_filter, sh_rows, sh_by_filter, g_sh_rows, background,
                     gt_u8, lambda_dssim=0.2, update_stats=True, keep=None, accumulate_after=None,
                     return_event=False, stats_only_visible=False, visibility_out=None,
                     raster_stream=None, small_packed=None, small_grad=None, stats_delta=None, sh_index=None,
                     sh_stamp=None, cur_step=0):
    """Forward, loss, backward for one camera over the rows of `this_filter`.

    Gradients are ACCUMULATED into gaussians._xyz/_opacity/_scaling/_rotation .grad (full size, must
    exist) and into g_sh_rows (indexed like sh_rows: by row id when sh_by_filter else by position).
    Returns the detached loss (0-dim tensor).  `keep`, if a list, receives tensors that must stay
    alive until the stream has consumed them.  Everything is enqueued on the CURRENT torch stream;
    `accumulate_after` (an event) gates the gradient-accumulating kernel so two cameras can be in
    flight on two streams while their read-modify-write accumulations stay ordered.
    `raster_stream`: if given, the two ALU-bound tile kernels are enqueued there (event-chained
    with the current stream) so that a shared low-priority stream carries all cameras' tile work
    while the latency-bound kernels of the other camera get CU slots first.
    `small_packed` / `small_grad`: the [N,12] mirror of the four small parameter tensors and the
    packed [N,12] gradient table (GaussianModelCLMOffload.small_packed / small_grad); the kernels
    then gather one 48 B row per Gaussian and accumulate into one, instead of four pieces each."""
    cur = torch.cuda.current_stream()
    p = camera_forward(gaussians, camera, this_filter, sh_rows, sh_by_filter, background, gt_u8,
                       lambda_dssim, small_packed, (cur, cur, raster_stream if raster_stream is not None else cur),
                       sh_index, exact=False)  # verified by camera_backward below
    camera_backward(gaussians, p, g_sh_rows, small_grad, update_stats, stats_delta,
                    stats_only_visible, visibility_out, accumulate_after, sh_stamp, cur_step)
    loss = camera_loss(p)  # on `cur`, which the loss kernels ran on
    if keep is not None:
        keep.append(p)
    if return_event:
        ev = torch.cuda.Event()
        ev.record(cur)
        return loss, ev
    return loss
