"""The five gsplat operators the CLM-GS engines import
(strategies/base_engine.py:6-12, strategies/no_offload/engine.py:4-10,
strategies/clm_offload/engine.py:7-13), with the same names, argument meaning
and return shapes, served by the gfx950 kernels of libclmgs_hip.so.

Differentiable operators are ``torch.autograd.Function``s whose forward and
backward call the C ABI; there is no eager fallback.
"""

import time

import torch

from . import _lib
from ._lib import check, dptr, stream

F32, I32, I64 = torch.float32, torch.int32, torch.int64


def _viewmats_grad(ctx, means, quats, scales, viewmats, Ks, radii, v_means2d, v_depths, v_conics, v_comps):
    """gsplat's v_viewmats (fully_fused_projection with viewmats_requires_grad): [C,4,4], rows 0..2 = v_R | v_t, row 3
    zero -- clmgs_projection_viewmat_bwd, launched only when the view matrices ask for a gradient."""
    if not ctx.needs_input_grad[3]:
        return None
    L = _lib.lib()
    width, height, eps2d = ctx.cfg
    C, N = radii.shape
    rows = int(L.clmgs_projection_viewmat_partials_rows(N))
    partials = torch.empty((C * max(rows, 1), 16), dtype=F32, device=means.device)
    v_viewmats = torch.empty((C, 4, 4), dtype=F32, device=means.device)
    check(L.clmgs_projection_viewmat_bwd(
        stream(), C, N, dptr(means), dptr(quats), dptr(scales), dptr(viewmats), dptr(Ks), width, height, eps2d,
        dptr(radii), dptr(v_means2d, F32), dptr(v_depths, F32, True), dptr(v_conics, F32), dptr(v_comps, F32, True),
        dptr(partials), dptr(v_viewmats)))
    return v_viewmats



# --------------------------------------------------------------------- projection
class _Projection(torch.autograd.Function):
    """clmgs_projection_fwd / _bwd; with calc_compensations the _aa_ entries, whose opacity compensations are a fifth,
    differentiable output (None otherwise: no buffer, no cotangent)."""

    @staticmethod
    def forward(ctx, means, quats, scales, viewmats, Ks, width, height, eps2d, near_plane,
                far_plane, radius_clip, calc_compensations):
        L = _lib.lib()
        means, quats, scales = means.contiguous(), quats.contiguous(), scales.contiguous()
        viewmats, Ks = viewmats.contiguous(), Ks.contiguous()
        C, N = viewmats.shape[0], means.shape[0]
        dev = means.device
        radii = torch.empty((C, N), dtype=I32, device=dev)
        means2d = torch.empty((C, N, 2), dtype=F32, device=dev)
        depths = torch.empty((C, N), dtype=F32, device=dev)
        conics = torch.empty((C, N, 3), dtype=F32, device=dev)
        comps = torch.empty((C, N), dtype=F32, device=dev) if calc_compensations else None
        fwd, extra = (L.clmgs_projection_aa_fwd, (dptr(comps),)) if calc_compensations else (L.clmgs_projection_fwd, ())
        check(fwd(
            stream(), C, N, dptr(means, F32), dptr(quats, F32), dptr(scales, F32),
            dptr(viewmats, F32), dptr(Ks, F32), int(width), int(height), float(eps2d),
            float(near_plane), float(far_plane), float(radius_clip), dptr(radii), dptr(means2d),
            dptr(depths), dptr(conics), *extra))
        ctx.save_for_backward(means, quats, scales, viewmats, Ks, radii)
        ctx.cfg = (int(width), int(height), float(eps2d))
        ctx.aa = bool(calc_compensations)
        ctx.mark_non_differentiable(radii)
        return radii, means2d, depths, conics, comps

    @staticmethod
    def backward(ctx, _v_radii, v_means2d, v_depths, v_conics, v_comps):
        L = _lib.lib()
        means, quats, scales, viewmats, Ks, radii = ctx.saved_tensors
        width, height, eps2d = ctx.cfg
        C, N = radii.shape
        dev = means.device
        if v_means2d is None:
            v_means2d = torch.zeros((C, N, 2), dtype=F32, device=dev)
        if v_conics is None:
            v_conics = torch.zeros((C, N, 3), dtype=F32, device=dev)
        v_means2d, v_conics = v_means2d.contiguous(), v_conics.contiguous()
        v_depths = v_depths.contiguous() if v_depths is not None else None
        v_comps = v_comps.contiguous() if v_comps is not None else None
        v_means = torch.empty_like(means)
        v_quats = torch.empty_like(quats)
        v_scales = torch.empty_like(scales)
        bwd, extra = (L.clmgs_projection_aa_bwd, (dptr(v_comps, F32, True),)) if ctx.aa else (L.clmgs_projection_bwd, ())
        check(bwd(
            stream(), C, N, dptr(means), dptr(quats), dptr(scales), dptr(viewmats), dptr(Ks),
            width, height, eps2d, dptr(radii), dptr(v_means2d, F32), dptr(v_depths, F32, True),
            dptr(v_conics, F32), *extra, dptr(v_means), dptr(v_quats), dptr(v_scales)))
        v_viewmats = _viewmats_grad(ctx, means, quats, scales, viewmats, Ks, radii, v_means2d, v_depths, v_conics, v_comps)
        return v_means, v_quats, v_scales, v_viewmats, None, None, None, None, None, None, None, None


CAMERA_MODELS = ("pinhole", "ortho")


def _check_camera_model(camera_model):
    if camera_model not in CAMERA_MODELS:
        raise ValueError(f"camera_model must be one of {CAMERA_MODELS}, got {camera_model!r}")
    return camera_model == "ortho"


class _ProjectionOrtho(torch.autograd.Function):
    """clmgs_projection_ortho_fwd / _bwd (gsplat's camera_model="ortho"): _Projection's arguments and results; the
    compensations buffer and its cotangent are handed over only with calc_compensations.  The view matrices receive no
    gradient (refused by fully_fused_projection before anything is launched)."""

    @staticmethod
    def forward(ctx, means, quats, scales, viewmats, Ks, width, height, eps2d, near_plane,
                far_plane, radius_clip, calc_compensations):
        L = _lib.lib()
        means, quats, scales = means.contiguous(), quats.contiguous(), scales.contiguous()
        viewmats, Ks = viewmats.contiguous(), Ks.contiguous()
        C, N = viewmats.shape[0], means.shape[0]
        dev = means.device
        radii = torch.empty((C, N), dtype=I32, device=dev)
        means2d = torch.empty((C, N, 2), dtype=F32, device=dev)
        depths = torch.empty((C, N), dtype=F32, device=dev)
        conics = torch.empty((C, N, 3), dtype=F32, device=dev)
        comps = torch.empty((C, N), dtype=F32, device=dev) if calc_compensations else None
        check(L.clmgs_projection_ortho_fwd(
            stream(), C, N, dptr(means, F32), dptr(quats, F32), dptr(scales, F32),
            dptr(viewmats, F32), dptr(Ks, F32), int(width), int(height), float(eps2d),
            float(near_plane), float(far_plane), float(radius_clip), dptr(radii), dptr(means2d),
            dptr(depths), dptr(conics), dptr(comps, F32, True)))
        ctx.save_for_backward(means, quats, scales, viewmats, Ks, radii)
        ctx.cfg = (int(width), int(height), float(eps2d))
        ctx.mark_non_differentiable(radii)
        return radii, means2d, depths, conics, comps

    @staticmethod
    def backward(ctx, _v_radii, v_means2d, v_depths, v_conics, v_comps):
        L = _lib.lib()
        means, quats, scales, viewmats, Ks, radii = ctx.saved_tensors
        width, height, eps2d = ctx.cfg
        C, N = radii.shape
        dev = means.device
        if v_means2d is None:
            v_means2d = torch.zeros((C, N, 2), dtype=F32, device=dev)
        if v_conics is None:
            v_conics = torch.zeros((C, N, 3), dtype=F32, device=dev)
        v_means2d, v_conics = v_means2d.contiguous(), v_conics.contiguous()
        v_depths = v_depths.contiguous() if v_depths is not None else None
        v_comps = v_comps.contiguous() if v_comps is not None else None
        v_means = torch.empty_like(means)
        v_quats = torch.empty_like(quats)
        v_scales = torch.empty_like(scales)
        check(L.clmgs_projection_ortho_bwd(
            stream(), C, N, dptr(means), dptr(quats), dptr(scales), dptr(viewmats), dptr(Ks),
            width, height, eps2d, dptr(radii), dptr(v_means2d, F32), dptr(v_depths, F32, True),
            dptr(v_conics, F32), dptr(v_comps, F32, True), dptr(v_means), dptr(v_quats), dptr(v_scales)))
        return v_means, v_quats, v_scales, None, None, None, None, None, None, None, None, None


def fully_fused_projection(means, covars, quats, scales, viewmats, Ks, width, height, eps2d=0.3,
                           near_plane=0.01, far_plane=1e10, radius_clip=0.0, packed=False,
                           sparse_grad=False, calc_compensations=False, camera_model="pinhole"):
    """EWA projection of N Gaussians into C cameras.

    Unpacked -> (radii[C,N] i32, means2d[C,N,2], depths[C,N], conics[C,N,3], compensations).
    Packed (no grad; strategies/base_engine.py:36-47 uses it under no_grad only)
    -> (camera_ids, gaussian_ids, radii, means2d, depths, conics, compensations), ordered
    by (camera, gaussian).
    The view matrices receive a gradient ([C,4,4], gsplat's viewmats_requires_grad) when `viewmats.requires_grad`;
    otherwise nothing more is launched.
    compensations: None, or with calc_compensations=True (gsplat's; Mip-Splatting) the differentiable opacity
    factors sqrt(max(0, det(cov2d) / det(cov2d + eps2d I))), [C,N] with 0 where culled (packed: [nnz]).
    camera_model: "pinhole", or "ortho" (gsplat's): Ks = [[sx,0,cx],[0,sy,cy],[0,0,1]] in pixels per world unit, the
    orthographic kernels of csrc/ortho.hip; same forms and results.  An orthographic view matrix that asks for a
    gradient raises NotImplementedError before anything is launched; any other string raises ValueError.
    """
    ortho = _check_camera_model(camera_model)
    if covars is not None:
        raise NotImplementedError("the CLM-GS engines always pass covars=None")
    if ortho and viewmats.requires_grad:
        raise NotImplementedError('camera_model="ortho" carries no view-matrix gradient (viewmats.requires_grad)')
    projection = _ProjectionOrtho if ortho else _Projection
    args = (means, quats, scales, viewmats, Ks, width, height, eps2d, near_plane, far_plane, radius_clip,
            bool(calc_compensations))
    if not packed:
        return projection.apply(*args)
    with torch.no_grad():
        radii, *outs = projection.apply(*args)
        camera_ids, gaussian_ids = torch.nonzero(radii > 0, as_tuple=True)
        return (camera_ids, gaussian_ids, radii[camera_ids, gaussian_ids],
                *(t[camera_ids, gaussian_ids] if t is not None else None for t in outs))


def visibility_radii(means, quats, scales, viewmats, Ks, width, height, eps2d=0.3,
                     near_plane=0.01, far_plane=1e10, radius_clip=0.0, raw=False, camera_model="pinhole"):
    """radii[C,N] only: the cull of fully_fused_projection without writing the 24 B of
    per-pair outputs (what calculate_filters, strategies/base_engine.py:18-76, needs).
    raw=True: `quats` un-normalised and `scales` as logs (the stored parameters).
    camera_model="ortho": the cull-only form of clmgs_projection_ortho_fwd; not with raw (nothing calls it)."""
    ortho = _check_camera_model(camera_model)
    if ortho and raw:
        raise NotImplementedError('visibility_radii(raw=True) has no camera_model="ortho" form')
    L = _lib.lib()
    means, quats, scales = means.contiguous(), quats.contiguous(), scales.contiguous()
    viewmats, Ks = viewmats.contiguous(), Ks.contiguous()
    C, N = viewmats.shape[0], means.shape[0]
    radii = torch.empty((C, N), dtype=I32, device=means.device)
    if raw:
        check(L.clmgs_visibility_raw(
            stream(), C, N, dptr(means, F32), dptr(quats, F32), dptr(scales, F32), dptr(viewmats, F32),
            dptr(Ks, F32), int(width), int(height), float(eps2d), float(near_plane), float(far_plane),
            float(radius_clip), dptr(radii)))
        return radii
    fwd, extra = (L.clmgs_projection_ortho_fwd, (None,)) if ortho else (L.clmgs_projection_fwd, ())
    check(fwd(
        stream(), C, N, dptr(means, F32), dptr(quats, F32), dptr(scales, F32), dptr(viewmats, F32),
        dptr(Ks, F32), int(width), int(height), float(eps2d), float(near_plane), float(far_plane),
        float(radius_clip), dptr(radii), None, None, None, *extra))
    return radii


def visibility_select_words(means, quats_raw, log_scales, viewmats, Ks, width, height, block_sel, eps2d=0.3,
                            near_plane=0.01, far_plane=1e10, radius_clip=0.0, block_flags=None):
    """The first of two launches of visibility_select over disjoint sets of 256-row blocks: the ballot words of the
    blocks block_sel = (words int64 [ceil(N/256)], mask, want) selects -- ((words[blk] & mask) != 0) == want -- and
    nothing else; no scan, no host read.  -> temp, to be handed to visibility_select(temp=, block_sel=(words, mask,
    1 - want)), which takes the other blocks and finishes.  Enqueued, and `temp` allocated, on the current stream."""
    L = _lib.lib()
    means, quats_raw, log_scales = means.contiguous(), quats_raw.contiguous(), log_scales.contiguous()
    viewmats, Ks = viewmats.contiguous(), Ks.contiguous()
    C, N = viewmats.shape[0], means.shape[0]
    tb = L.clmgs_visibility_select_temp_bytes(C, N)
    temp = torch.empty((tb,), dtype=torch.uint8, device=means.device)
    words, mask, want = block_sel
    check(L.clmgs_visibility_select_count_blocks_sel(
        stream(), C, N, dptr(means, F32), dptr(quats_raw, F32), dptr(log_scales, F32), dptr(viewmats, F32),
        dptr(Ks, F32), int(width), int(height), float(eps2d), float(near_plane), float(far_plane),
        float(radius_clip), dptr(temp), tb, None, dptr(block_flags, torch.uint8, True), dptr(words, I64),
        int(mask) & 0xFFFFFFFFFFFFFFFF, int(want), 0))
    return temp


def visibility_select(means, quats_raw, log_scales, viewmats, Ks, width, height, eps2d=0.3,
                      near_plane=0.01, far_plane=1e10, radius_clip=0.0, block_flags=None, block_sel=None, temp=None):
    """The batch's visibility filters selected on the GPU: same cull as visibility_radii(raw=True)
    but without the radii[C,N] round trip and torch.nonzero -- one ballot word per (camera, 64
    Gaussians), a scan, and an emit pass.  -> (filters: tuple of C int64 index tensors (ascending),
    touched_rows: int64 indices of the union over the cameras).  One host read (the C+1 totals).
    block_sel + temp: the second of two launches (visibility_select_words made `temp` and the other blocks' words)."""
    L = _lib.lib()
    means, quats_raw, log_scales = means.contiguous(), quats_raw.contiguous(), log_scales.contiguous()
    viewmats, Ks = viewmats.contiguous(), Ks.contiguous()
    C, N = viewmats.shape[0], means.shape[0]
    dev = means.device
    tb = L.clmgs_visibility_select_temp_bytes(C, N)
    assert (block_sel is None) == (temp is None)
    if temp is None:
        temp = torch.empty((tb,), dtype=torch.uint8, device=dev)
    else:
        assert temp.numel() == tb
        temp.record_stream(torch.cuda.current_stream())  # (allocated on the first launch's stream)
    cum = torch.empty((C + 1,), dtype=I64, device=dev)
    words, mask, want = block_sel if block_sel is not None else (None, 0, 0)
    # block_flags (uint8 per 256 rows, 0 = no row of the block can be visible: clmgs_adam_small_deferred's candidate test)
    check(L.clmgs_visibility_select_count_blocks_sel(
        stream(), C, N, dptr(means, F32), dptr(quats_raw, F32), dptr(log_scales, F32), dptr(viewmats, F32),
        dptr(Ks, F32), int(width), int(height), float(eps2d), float(near_plane), float(far_plane),
        float(radius_clip), dptr(temp), tb, dptr(cum), dptr(block_flags, torch.uint8, True), dptr(words, I64, True),
        int(mask) & 0xFFFFFFFFFFFFFFFF, int(want), 1))
    _t0 = time.perf_counter()
    ends = cum.tolist()  # the one host sync of the filter stage
    _lib.STATS["host_wait_s"] += time.perf_counter() - _t0
    out = torch.empty((max(ends[-1], 1),), dtype=I64, device=dev)
    if ends[-1] > 0:
        check(L.clmgs_visibility_select_emit(stream(), C, N, dptr(temp), dptr(out)))
    starts = [0] + ends[:-1]
    pieces = tuple(out[a:b] for a, b in zip(starts, ends))
    return pieces[:C], pieces[C]


def visibility_candidates(means, log_scales, viewmats, Ks, width, height, pos_margin, scale_gain, own_lo, own_hi,
                          eps2d=0.3, near_plane=0.01, far_plane=1e10):
    """Camera-DP, small attributes computed by their owners: ascending int64 ids of the rows OUTSIDE [own_lo, own_hi)
    that may pass visibility_select's cull in any camera while their stored mean is off by up to pos_margin and their
    largest scale by a factor up to scale_gain (clmgs_visibility_candidates: a superset of what the exact cull keeps
    for the true values).  One host read inside torch.nonzero (the count)."""
    L = _lib.lib()
    means, log_scales = means.contiguous(), log_scales.contiguous()
    viewmats, Ks = viewmats.contiguous(), Ks.contiguous()
    C, N = viewmats.shape[0], means.shape[0]
    mask = torch.empty((N,), dtype=torch.uint8, device=means.device)
    check(L.clmgs_visibility_candidates(
        stream(), C, N, int(own_lo), int(own_hi), dptr(means, F32), dptr(log_scales, F32), dptr(viewmats, F32),
        dptr(Ks, F32), int(width), int(height), float(eps2d), float(near_plane), float(far_plane),
        float(pos_margin), float(scale_gain), dptr(mask)))
    return torch.nonzero(mask).flatten()


# ------------------------------------------------------------ spherical harmonics
class _SphericalHarmonics(torch.autograd.Function):
    @staticmethod
    def forward(ctx, degree, dirs, coeffs, masks):
        L = _lib.lib()
        lead = dirs.shape[:-1]
        n = dirs.numel() // 3
        assert coeffs.shape[-2:] == (16, 3) or coeffs.shape[-1] == 48, coeffs.shape
        d2, c2 = dirs.contiguous(), coeffs.contiguous()
        m2 = masks.contiguous().view(torch.uint8) if masks is not None else None
        colors = torch.empty(lead + (3,), dtype=F32, device=dirs.device)
        check(L.clmgs_sh_fwd(stream(), n, int(degree), dptr(d2, F32), dptr(c2, F32),
                             dptr(m2, torch.uint8, True), dptr(colors)))
        ctx.save_for_backward(d2, c2, m2)
        ctx.degree = int(degree)
        ctx.n = n
        return colors

    @staticmethod
    def backward(ctx, v_colors):
        L = _lib.lib()
        d2, c2, m2 = ctx.saved_tensors
        v_colors = v_colors.contiguous()
        v_coeffs = torch.empty_like(c2) if ctx.needs_input_grad[2] else None
        v_dirs = torch.empty_like(d2) if ctx.needs_input_grad[1] else None
        if v_coeffs is None:  # kernel always produces v_coeffs; give it scratch
            v_coeffs_buf = torch.empty_like(c2)
        else:
            v_coeffs_buf = v_coeffs
        check(L.clmgs_sh_bwd(stream(), ctx.n, ctx.degree, dptr(d2), dptr(c2),
                             dptr(m2, torch.uint8, True), dptr(v_colors, F32), dptr(v_coeffs_buf),
                             0, dptr(v_dirs, F32, True)))
        return None, v_dirs, v_coeffs, None


def spherical_harmonics(degrees_to_use, dirs, coeffs, masks=None):
    """colors[...,3] from dirs[...,3] (normalised inside) and coeffs[...,16,3]; rows with
    masks == False produce 0 and receive 0 gradient."""
    return _SphericalHarmonics.apply(degrees_to_use, dirs, coeffs, masks)


# ------------------------------------------------------------------- tile binning
@torch.no_grad()
def isect_tiles(means2d, radii, depths, tile_size, tile_width, tile_height, sort=True,
                packed=False, n_cameras=None, camera_ids=None, gaussian_ids=None):
    """-> (tiles_per_gauss[C,N] i32, isect_ids[I] i64 sorted, flatten_ids[I] i32)."""
    if packed or not sort:
        raise NotImplementedError("the CLM-GS engines call isect_tiles(packed=False, sort=True)")
    L = _lib.lib()
    C, N = radii.shape
    dev = radii.device
    means2d, radii, depths = means2d.contiguous(), radii.contiguous(), depths.contiguous()
    tiles_per_gauss = torch.empty((C, N), dtype=I32, device=dev)
    cum = torch.empty((C * N,), dtype=I64, device=dev)
    if C * N == 0:
        return tiles_per_gauss, torch.empty(0, dtype=I64, device=dev), torch.empty(0, dtype=I32, device=dev)
    tb = L.clmgs_isect_count_temp_bytes(C * N)
    temp = torch.empty((tb,), dtype=torch.uint8, device=dev)
    check(L.clmgs_isect_count(stream(), C, N, dptr(means2d, F32), dptr(radii, I32), int(tile_size),
                              int(tile_width), int(tile_height), dptr(tiles_per_gauss), dptr(cum),
                              dptr(temp), tb))
    n_isects = int(cum[-1].item())  # data-dependent size: the one host sync of the front end
    _lib.STATS["n_isects"].append(n_isects)
    if len(_lib.STATS["n_isects"]) > 4096:
        del _lib.STATS["n_isects"][:2048]
        del _lib.STATS["n_emitted"][:2048]
    isect_ids = torch.empty((n_isects,), dtype=I64, device=dev)
    flatten_ids = torch.empty((n_isects,), dtype=I32, device=dev)
    if n_isects:
        sb = L.clmgs_isect_sort_temp_bytes(n_isects)
        temp2 = torch.empty((sb,), dtype=torch.uint8, device=dev)
        check(L.clmgs_isect_emit_sort(stream(), C, N, n_isects, dptr(means2d), dptr(radii),
                                      dptr(depths, F32), dptr(cum), int(tile_size),
                                      int(tile_width), int(tile_height), dptr(isect_ids),
                                      dptr(flatten_ids), dptr(temp2), sb))
    return tiles_per_gauss, isect_ids, flatten_ids


@torch.no_grad()
def isect_offset_encode(isect_ids, n_cameras, tile_width, tile_height):
    """offsets[C, tile_height, tile_width] i32 = first sorted index of each tile."""
    L = _lib.lib()
    offsets = torch.empty((n_cameras, tile_height, tile_width), dtype=I32, device=isect_ids.device)
    check(L.clmgs_isect_offsets(stream(), isect_ids.numel(), dptr(isect_ids.contiguous(), I64),
                                int(n_cameras), int(tile_width), int(tile_height), dptr(offsets)))
    return offsets


def bucket_size(n):
    """n rounded up to 1/8 steps of its leading power of two (<= 12.5 % more).  The data-dependent
    buffers of a camera (rows V, intersections I) are allocated at bucketed capacity and viewed
    [:n]: the same few sizes then recur batch after batch and the caching allocator serves them
    from its cache instead of calling hipMalloc in the middle of a step (a 9 ms stall when it
    happened inside the 5 timed steps of the bench)."""
    n = int(n)
    if n <= 4096:
        return 4096
    sh = n.bit_length() - 4
    return ((n + (1 << sh) - 1) >> sh) << sh


def empty_bucketed(n, trailing, dtype, device):
    """torch.empty((n, *trailing)) backed by a bucket_size(n)-row allocation."""
    return torch.empty((bucket_size(n),) + tuple(trailing), dtype=dtype, device=device)[:n]


_PINNED_TOTALS = None  # ring of pinned int64[2] slots for the asynchronous size readbacks
_PINNED_NEXT = 0


def _pinned_totals_slot():
    global _PINNED_TOTALS, _PINNED_NEXT
    if _PINNED_TOTALS is None:
        _PINNED_TOTALS = torch.empty((256, 2), dtype=I64).pin_memory()
    _PINNED_NEXT = (_PINNED_NEXT + 1) % _PINNED_TOTALS.shape[0]
    return _PINNED_TOTALS[_PINNED_NEXT]


class _Isect:
    """State between isect_begin and isect_finish (one camera's binning in flight)."""
    __slots__ = ("args", "V", "dev", "depths", "order", "cum", "boxes", "totals", "host", "event",
                 "offsets", "temp", "means2d", "radii", "packed", "row_cum", "route")


@torch.no_grad()
def isect_begin(route, means2d, radii, depths, tile_size, tile_width, tile_height, want_isect_ids=False,
                want_slots=False, packed=None):
    """First half of a camera's binning on the CURRENT stream, then an asynchronous copy of the two totals into pinned
    memory and an event.  Nothing blocks: the caller can enqueue other work (the next camera's projection) before
    isect_finish waits for the event -- unlike a `.tolist()`, which waits for everything enqueued on the stream so far.
    route "sort" (csrc/isect.hip, clmgs_isect2_order_count): depth order + per-row tile counts, for a depth sort of the
    rows and one stable sort on tile-id bits.  route "tile" (csrc/isect3.hip, clmgs_isect3_front): per-row tile boxes /
    masks, tile counters and row_cum, for the same lists without a global sort."""
    if route not in ("tile", "sort"):
        raise ValueError(f"binning route must be 'tile' or 'sort', got {route!r}")
    L = _lib.lib()
    c = _Isect()
    c.route = route
    c.args = (int(tile_size), int(tile_width), int(tile_height), bool(want_isect_ids), bool(want_slots))
    V = c.V = radii.numel()
    dev = c.dev = radii.device
    c.means2d, c.radii, c.depths = means2d.contiguous(), radii.contiguous(), depths.contiguous()
    c.packed = packed
    c.offsets = torch.empty((1, tile_height, tile_width), dtype=I32, device=dev)
    c.event = None
    c.order = c.cum = c.boxes = None
    if V == 0:
        return c
    if route == "sort":
        c.order = empty_bucketed(V, (), I32, dev)
        c.cum = empty_bucketed(V, (), I64, dev)
        c.boxes = empty_bucketed(V, (2,), I64, dev)
    c.totals = torch.empty((2,), dtype=I64, device=dev)
    c.row_cum = empty_bucketed(V, (), I64, dev) if (want_slots or route == "tile") else None
    tb = (L.clmgs_isect2_order_temp_bytes(V) if route == "sort"
          else L.clmgs_isect3_front_temp_bytes(V, int(tile_width) * int(tile_height)))
    c.temp = empty_bucketed(tb, (), torch.uint8, dev)
    if route == "sort":
        check(L.clmgs_isect2_order_count(stream(), V, dptr(c.means2d, F32), dptr(c.radii, I32), dptr(c.depths, F32),
                                         c.args[0], c.args[1], c.args[2], dptr(packed, F32, True), dptr(c.order),
                                         dptr(c.cum), dptr(c.boxes), dptr(c.totals), dptr(c.temp), tb,
                                         dptr(c.row_cum, I64, True)))
    else:
        check(L.clmgs_isect3_front(stream(), V, dptr(c.means2d, F32), dptr(c.radii, I32), c.args[0], c.args[1], c.args[2],
                                   dptr(packed, F32, True), dptr(c.totals), dptr(c.row_cum), dptr(c.temp), tb))
    c.host = _pinned_totals_slot()
    c.host.copy_(c.totals, non_blocking=True)
    c.event = torch.cuda.Event()
    c.event.record(torch.cuda.current_stream())
    return c


def _record_counts(n_isects, n_ref):
    _lib.STATS["n_isects"].append(n_ref)        # the reference's (3-sigma box) intersection count
    _lib.STATS["n_emitted"].append(n_isects)    # what is actually sorted and blended
    if len(_lib.STATS["n_isects"]) > 4096:
        del _lib.STATS["n_isects"][:2048]
        del _lib.STATS["n_emitted"][:2048]


def isect_counts(c):
    """Wait for the totals of isect_begin (an event on an asynchronous readback) -> (emitted, reference)."""
    _t0 = time.perf_counter()
    c.event.synchronize()
    n_isects, n_ref = int(c.host[0]), int(c.host[1])
    _lib.STATS["host_wait_s"] += time.perf_counter() - _t0
    return n_isects, n_ref


@torch.no_grad()
def isect_finish(c, capacity=None):
    """Second half on the CURRENT stream (the stream isect_begin ran on, or one ordered after it), by the route
    isect_begin was given: emit + tile sort + offsets (clmgs_isect2_emit_sort) or tile scan, scatter, per-tile sort
    (clmgs_isect3_bin).
    capacity None: wait for the totals (the one host wait of the front end) and size everything exactly.
    capacity = K (device-count form, the entries' _dev variants): NOTHING is waited for -- buffers and launches
    are sized for K intersections and the kernels read the true count from c.totals on the device; the returned
    lists have K entries of which the first `count` are valid.  The caller must check isect_counts(c)[0] <= K
    later (fused.camera_verify) and redo the camera exactly otherwise."""
    L = _lib.lib()
    tile_size, tile_width, tile_height, want_isect_ids, want_slots = c.args
    dev, V = c.dev, c.V
    if V == 0:
        c.offsets.zero_()
        e = torch.empty(0, dtype=I32, device=dev)
        res = (e, c.offsets, (torch.empty(0, dtype=I64, device=dev) if want_isect_ids else None))
        return res + ((e, torch.empty(0, dtype=I64, device=dev)),) if want_slots else res
    if capacity is None:
        n_isects, n_ref = isect_counts(c)
        _record_counts(n_isects, n_ref)
    else:
        n_isects = int(capacity)
    sort = c.route == "sort"
    fids = empty_bucketed(n_isects, (), I32, dev)
    ids = empty_bucketed(n_isects, (), I64, dev) if want_isect_ids else None
    sb = (L.clmgs_isect2_sort_temp_bytes(n_isects) if sort
          else L.clmgs_isect3_bin_temp_bytes(n_isects, tile_width * tile_height))
    temp2 = empty_bucketed(sb, (), torch.uint8, dev)
    emit_slot = empty_bucketed(n_isects, (), I32, dev) if want_slots else None
    count = () if capacity is None else (dptr(c.totals),)  # the _dev entries: the true count, after n_isects
    if sort:
        check((L.clmgs_isect2_emit_sort if capacity is None else L.clmgs_isect2_emit_sort_dev)(
            stream(), V, n_isects, *count, dptr(c.depths), dptr(c.order), dptr(c.cum), dptr(c.boxes), tile_width,
            tile_height, dptr(fids), dptr(c.offsets), dptr(ids, I64, True), dptr(emit_slot, I32, True), dptr(temp2), sb,
            dptr(c.row_cum, I64, True)))
    else:
        check((L.clmgs_isect3_bin if capacity is None else L.clmgs_isect3_bin_dev)(
            stream(), V, n_isects, *count, dptr(c.depths), tile_width, tile_height, dptr(c.row_cum), dptr(c.temp),
            dptr(fids), dptr(c.offsets), dptr(ids, I64, True), dptr(emit_slot, I32, True), dptr(temp2), sb))
    return (fids, c.offsets, ids, (emit_slot, c.row_cum)) if want_slots else (fids, c.offsets, ids)


@torch.no_grad()
def isect_tiles_two_level(means2d, radii, depths, tile_size, tile_width, tile_height,
                          want_isect_ids=False, want_slots=False, packed=None):
    """Single-camera binning through the two-level sort (depth sort of the rows, then one stable
    sort on tile-id bits).  -> (flatten_ids[I] i32, offsets[1,th,tw] i32, isect_ids[I] i64 | None),
    identical to isect_tiles + isect_offset_encode for C = 1.  want_slots: a 4th result
    (emit_slot[I] i32, row_cum[V] i64) for the atomic-free rasterize backward: row i owns the
    contiguous slot range [row_cum[i-1], row_cum[i]).
    packed: the [V,16] raster records -> EXACT per-tile culling (pairs whose tile cannot reach
    alpha >= 1/255 are not emitted; image and gradients unchanged, the list gets ~29 % shorter).
    = isect_begin("sort", ...) + isect_finish back to back."""
    return isect_finish(isect_begin("sort", means2d, radii, depths, tile_size, tile_width, tile_height,
                                    want_isect_ids, want_slots, packed))


# ---------------------------------------------------------------------- rasterize
class _Rasterize(torch.autograd.Function):
    @staticmethod
    def forward(ctx, means2d, conics, colors, opacities, backgrounds, width, height, tile_size,
                isect_offsets, flatten_ids, absgrad=False):
        L = _lib.lib()
        C, N = opacities.shape
        dev = means2d.device
        ctx.absgrad_of = means2d if absgrad else None  # the tensor the caller passed in: backward sets .absgrad on it
        means2d, conics, colors, opacities = (t.contiguous() for t in (means2d, conics, colors, opacities))
        bg = backgrounds.contiguous() if backgrounds is not None else None
        offsets = isect_offsets.contiguous()
        fids = flatten_ids.contiguous()
        th, tw = offsets.shape[1:]
        nch = colors.shape[-1]  # 3, or 4 (the fourth channel rides in the record's spare word: clmgs_rasterize4_*)
        fwd = L.clmgs_rasterize4_fwd if nch == 4 else L.clmgs_rasterize_fwd
        out = torch.empty((C, height, width, nch), dtype=F32, device=dev)
        alphas = torch.empty((C, height, width, 1), dtype=F32, device=dev)
        last_ids = torch.empty((C, height, width), dtype=I32, device=dev)
        n_isects = fids.numel()
        packed = torch.empty((C * N, 16), dtype=F32, device=dev)  # one 64 B record per Gaussian
        check(fwd(
            stream(), C, N, n_isects, dptr(means2d, F32), dptr(conics, F32), dptr(colors, F32),
            dptr(opacities, F32), dptr(bg, F32, True), int(width), int(height), int(tile_size), tw,
            th, dptr(offsets, I32), dptr(fids, I32), dptr(packed), dptr(out), dptr(alphas),
            dptr(last_ids)))
        ctx.save_for_backward(packed, bg, offsets, fids, alphas, last_ids)
        ctx.shapes = (means2d.shape, conics.shape, colors.shape, opacities.shape)
        ctx.cfg = (int(width), int(height), int(tile_size))
        return out, alphas

    @staticmethod
    def backward(ctx, v_out, v_alphas):
        L = _lib.lib()
        packed, bg, offsets, fids, alphas, last_ids = ctx.saved_tensors
        width, height, tile_size = ctx.cfg
        s_m2, s_cn, s_col, s_op = ctx.shapes
        C, N = s_op
        th, tw = offsets.shape[1:]
        dev = packed.device
        v_out = v_out.contiguous()
        v_alphas = v_alphas.contiguous() if v_alphas is not None else None
        v_means2d = torch.empty(s_m2, dtype=F32, device=dev)
        v_conics = torch.empty(s_cn, dtype=F32, device=dev)
        v_colors = torch.empty(s_col, dtype=F32, device=dev)
        v_opacities = torch.empty(s_op, dtype=F32, device=dev)
        packed_grad = torch.empty_like(packed)
        bwd = L.clmgs_rasterize4_bwd if s_col[-1] == 4 else L.clmgs_rasterize_bwd
        extra = ()
        if ctx.absgrad_of is not None:  # gsplat's absgrad: sum_p |dL_p/dmean2d| next to the signed sum (atomic route)
            v_abs = torch.empty(s_m2, dtype=F32, device=dev)
            bwd, extra = L.clmgs_rasterize_abs_bwd, (dptr(v_abs),)
        check(bwd(
            stream(), C, N, fids.numel(), dptr(packed), dptr(bg, F32, True), width, height,
            tile_size, tw, th, dptr(offsets), dptr(fids), dptr(alphas), dptr(last_ids),
            dptr(v_out, F32), dptr(v_alphas, F32, True), dptr(packed_grad), dptr(v_means2d),
            dptr(v_conics), dptr(v_colors), dptr(v_opacities), None, None, None, *extra))
        if ctx.absgrad_of is not None:
            ctx.absgrad_of.absgrad = v_abs
        return v_means2d, v_conics, v_colors, v_opacities, None, None, None, None, None, None, None


def rasterize_to_pixels(means2d, conics, colors, opacities, image_width, image_height, tile_size,
                        isect_offsets, flatten_ids, backgrounds=None, masks=None, packed=False,
                        absgrad=False):
    """-> (render_colors[C,H,W,3], render_alphas[C,H,W,1]).  backgrounds: None, [3] or [C,3]
    (the reference passes both shapes: no_offload/engine.py:96 vs base_engine.py:189-191).
    colors[..., 4] (gsplat's render_mode="RGB+D": the camera-space depth as a fourth colour) -> render_colors[C,H,W,4],
    backgrounds None, [4] or [C,4]; channels 0..2 and the alphas are bit-identical to the 3-channel call.
    absgrad=True (gsplat's, AbsGS; three channels only): the backward also sets `means2d.absgrad`, shaped like means2d, on
    the tensor passed in: sum over the pixels each Gaussian contributes to of |dL_p/dmean2d|, componentwise."""
    if packed or masks is not None:
        raise NotImplementedError("packed/masks are not used by the CLM-GS engines")
    nch = colors.shape[-1]
    if nch not in (3, 4):
        raise NotImplementedError("3 or 4 colour channels only")
    if absgrad and nch != 3:
        raise NotImplementedError("absgrad blends three channels only (no absgrad with a depth channel)")
    C = opacities.shape[0]
    if backgrounds is not None:
        if backgrounds.shape[-1] != nch:
            raise ValueError(f"backgrounds must hold {nch} values per camera, like colors")
        backgrounds = backgrounds.reshape(-1, nch).to(F32)
        if backgrounds.shape[0] != C:
            backgrounds = backgrounds.expand(C, nch)
    return _Rasterize.apply(means2d, conics, colors, opacities, backgrounds, int(image_width),
                            int(image_height), int(tile_size), isect_offsets, flatten_ids, bool(absgrad))


# ------------------------------------------------------------------ contributions
WSUM_UNIT = 2.0 ** -28  # one unit of the fixed-point weight sums (clmgs_rasterize_contrib)


def contribution_arrays(n, device):
    """The three zeroed raw arrays clmgs_rasterize_contrib adds into, n rows: (wsum_q, wmax_bits, pixels).  uint64 /
    uint32 on the device side, held as int64 / int32 tensors (the sums stay far below 2^63; a non-negative float's bit
    pattern is a non-negative int32)."""
    return (torch.zeros((n,), dtype=I64, device=device), torch.zeros((n,), dtype=I32, device=device),
            torch.zeros((n,), dtype=I64, device=device))


def contribution_values(raw):
    """raw arrays -> (wsum float64, wmax float32, pixels int64)."""
    wsum_q, wmax_bits, pixels = raw
    return wsum_q.to(torch.float64) * WSUM_UNIT, wmax_bits.view(F32), pixels


@torch.no_grad()
def rasterize_contributions(means2d, conics, opacities, image_width, image_height, tile_size, isect_offsets, flatten_ids,
                            rows=None, out=None):
    """Per-Gaussian blend weights w = alpha * T of C views over the lists rasterize_to_pixels would blend, summed over the
    in-image pixels at which it accumulates each Gaussian: -> (wsum float64 [R], wmax float32 [R], pixels int64 [R]).
    R = C*N (row cam * N + g), or len(out) rows when accumulating into `out`, the raw triple of contribution_arrays: the
    kernel ADDS (integer atomics, bit-reproducible), so one triple can take camera after camera.  rows (int64 [N], one
    table for all C cameras): Gaussian g of every camera lands in row rows[g] -- a camera's visibility filter scatters
    straight into model-wide arrays.  Not differentiable: inputs that require grad are detached."""
    L = _lib.lib()
    C, N = opacities.shape
    dev = means2d.device
    means2d, conics, opacities = (t.detach().contiguous() for t in (means2d, conics, opacities))
    offsets, fids = isect_offsets.contiguous(), flatten_ids.contiguous()
    th, tw = offsets.shape[1:]
    if rows is not None:
        rows = rows.contiguous()
        if rows.numel() != N:
            raise ValueError(f"rows must hold one destination per Gaussian ({N}), got {rows.numel()}")
    raw = contribution_arrays(C * N, dev) if out is None else tuple(out)
    n_out = raw[0].numel()
    if not (raw[1].numel() == n_out and raw[2].numel() == n_out):
        raise ValueError("out: three arrays of the same length")
    if n_out == 0:  # no rows: nothing to add to
        return contribution_values(raw)
    pb = L.clmgs_rasterize_contrib_pack_bytes(C, N)
    packed = torch.empty((pb,), dtype=torch.uint8, device=dev)
    check(L.clmgs_rasterize_contrib(
        stream(), C, N, fids.numel(), dptr(means2d, F32), dptr(conics, F32), dptr(opacities, F32), int(image_width),
        int(image_height), int(tile_size), tw, th, dptr(offsets, I32), dptr(fids, I32), dptr(rows, I64, True), n_out,
        dptr(packed), dptr(raw[0], I64), dptr(raw[1], I32), dptr(raw[2], I64)))
    return contribution_values(raw)


# ------------------------------------------------------------------ median depth
@torch.no_grad()
def rasterize_median_depth(means2d, conics, opacities, depths, image_width, image_height, tile_size, isect_offsets,
                           flatten_ids):
    """The median depth of C views over the lists rasterize_to_pixels would blend: per pixel, the entry at which the
    transmittance falls through one half -- the last accumulated entry whose T before blending is > 0.5, so the pixel's
    last contributor where the final T stays above one half (csrc/median.hip; DESIGN.md section 3, "Median depth").
    means2d [C,N,2], conics [C,N,3], opacities [C,N], depths [C,N] (camera-space)
    -> (median_depth float32 [C,H,W]: depths[] of that entry, copied; median_ids int32 [C,H,W]: its row within its camera);
    0.0 and -1 where a pixel accumulates nothing.  Not differentiable: inputs that require grad are detached."""
    L = _lib.lib()
    C, N = opacities.shape
    dev = means2d.device
    means2d, conics, opacities, depths = (t.detach().contiguous() for t in (means2d, conics, opacities, depths))
    offsets, fids = isect_offsets.contiguous(), flatten_ids.contiguous()
    th, tw = offsets.shape[1:]
    H, W = int(image_height), int(image_width)
    median_depth = torch.empty((C, H, W), dtype=F32, device=dev)
    median_ids = torch.empty((C, H, W), dtype=I32, device=dev)
    pb = L.clmgs_rasterize_median_pack_bytes(C, N)
    packed = torch.empty((pb,), dtype=torch.uint8, device=dev)
    check(L.clmgs_rasterize_median(
        stream(), C, N, fids.numel(), dptr(means2d, F32), dptr(conics, F32), dptr(opacities, F32), dptr(depths, F32), W, H,
        int(tile_size), tw, th, dptr(offsets, I32), dptr(fids, I32), dptr(packed), dptr(median_depth, F32),
        dptr(median_ids, I32)))
    return median_depth, median_ids


# ------------------------------------------------------------------ ray depth
RAY_CAMERA_MODELS = {"pinhole": 0, "ortho": 1}


def ray_camera_table(viewmats, Ks):
    """viewmats [C,4,4], Ks [C,3,3] -> the float64 [C,16] table csrc/ray_depth.hip reads: per camera the top 3x4 of the view
    matrix (row-major), then fx, fy, cx, cy.  Made on the device, nothing is read back."""
    C = viewmats.shape[0]
    return torch.cat([viewmats[:, :3, :4].reshape(C, 12), Ks[:, 0, 0:1], Ks[:, 1, 1:2], Ks[:, 0, 2:3], Ks[:, 1, 2:3]],
                     dim=1).to(torch.float64).contiguous()


@torch.no_grad()
def ray_gaussian_depth(means, quats, scales, viewmats, Ks, median_depth, median_ids, near_plane=0.01,
                       camera_model="pinhole"):
    """The ray-Gaussian intersection depth of RaDe-GS / GOF for each pixel's median Gaussian (csrc/ray_depth.hip,
    csrc/ray_math.h; DESIGN.md section 3, "Ray depth"): the depth of the point on the pixel's ray at which that Gaussian's
    3-D density is largest,  t* = d^T S^-1 (m - o) / d^T S^-1 d,  where rasterize_median_depth reports its centre depth.
    means [N,3], quats [N,4] (w,x,y,z; normalised inside), scales [N,3] (ACTIVATED), viewmats [C,4,4], Ks [C,3,3] as
    fully_fused_projection takes them; median_depth float32 [C,H,W] and median_ids int32 [C,H,W] (the row within its camera)
    as rasterize_median_depth returns them.  The ray of pixel (x, y): u = (x + 0.5 - cx) / fx, v = (y + 0.5 - cy) / fy;
    "pinhole": origin 0, direction (u, v, 1); "ortho" (K in pixels per world unit): origin (u, v, 0), direction (0, 0, 1) --
    in both the parameter t is a camera z-depth.  Computed in float64 from the float32 inputs, every operation rounded on
    its own (bit-reproducible; tests/ray_depth_reference.py restates it).
    -> ray_depth float32 [C,H,W]: (float32) t* where t* is finite and > near_plane; else median_depth of the pixel, copied
    (a zero scale, a maximum behind the near plane, non-finite inputs); 0.0 where the id lies outside [0, N).
    Not differentiable: runs under no_grad, inputs that require grad are detached."""
    if camera_model not in RAY_CAMERA_MODELS:
        raise ValueError(f"camera_model must be 'pinhole' or 'ortho', got {camera_model!r}")
    L = _lib.lib()
    means, quats, scales, median_depth, median_ids = (t.detach().contiguous() for t in (means, quats, scales, median_depth,
                                                                                        median_ids))
    N = int(means.shape[0])
    C, H, W = (int(v) for v in median_ids.shape)
    if tuple(median_depth.shape) != (C, H, W) or tuple(viewmats.shape) != (C, 4, 4) or tuple(Ks.shape) != (C, 3, 3):
        raise ValueError(f"ray_gaussian_depth: median_depth {tuple(median_depth.shape)}, viewmats {tuple(viewmats.shape)} and Ks "
                         f"{tuple(Ks.shape)} do not match median_ids {tuple(median_ids.shape)}")
    if tuple(quats.shape) != (N, 4) or tuple(scales.shape) != (N, 3) or tuple(means.shape) != (N, 3):
        raise ValueError(f"ray_gaussian_depth: means [N,3], quats [N,4] and scales [N,3] expected, got {tuple(means.shape)}, "
                         f"{tuple(quats.shape)} and {tuple(scales.shape)}")
    cams = ray_camera_table(viewmats.detach(), Ks.detach())
    out = torch.empty((C, H, W), dtype=F32, device=median_ids.device)
    check(L.clmgs_ray_depth(stream(), C, N, H, W, dptr(means, F32), dptr(quats, F32), dptr(scales, F32),
                            dptr(cams, torch.float64), dptr(median_ids, I32), dptr(median_depth, F32), float(near_plane),
                            RAY_CAMERA_MODELS[camera_model], dptr(out, F32)))
    return out
