"""clm_kernels operator surface used by the CLM-GS engines, on gfx950.

Same names and argument meaning as the reference's call sites
(strategies/base_engine.py:5,93; strategies/clm_offload/engine.py:14-20,152-153,
200-204,227-232,499-505,622-636,709-716,789-825; optimizer.py:3,76-88).
"""
import ctypes

import torch

from . import _lib, utils
from ._lib import check, dptr, stream

F32, I32, I64, U8 = torch.float32, torch.int32, torch.int64, torch.uint8


# ------------------------------------------------------------------- fused SSIM
class _FusedSSIM(torch.autograd.Function):
    @staticmethod
    def forward(ctx, img1, img2):
        L = _lib.lib()
        img1, img2 = img1.contiguous(), img2.contiguous()
        B, CH, H, W = img1.shape
        need = img1.requires_grad
        ssim_sum = torch.zeros((1024,), dtype=F32, device=img1.device)
        maps = [torch.empty_like(img1) for _ in range(3)] if need else [None, None, None]
        check(L.clmgs_ssim_fwd(stream(), B, CH, H, W, dptr(img1, F32), dptr(img2, F32),
                               dptr(ssim_sum), dptr(maps[0], F32, True), dptr(maps[1], F32, True),
                               dptr(maps[2], F32, True)))
        ctx.shape = (B, CH, H, W)
        if need:
            ctx.save_for_backward(img1, img2, *maps)
        return ssim_sum.sum() / float(img1.numel())

    @staticmethod
    def backward(ctx, v):
        L = _lib.lib()
        img1, img2, m0, m1, m2 = ctx.saved_tensors
        B, CH, H, W = ctx.shape
        v_img1 = torch.empty_like(img1)
        v = v.reshape(1).to(F32).contiguous()
        check(L.clmgs_ssim_bwd(stream(), B, CH, H, W, dptr(img1), dptr(img2), dptr(v, F32),
                               1.0 / float(img1.numel()), dptr(m0), dptr(m1), dptr(m2),
                               dptr(v_img1)))
        return v_img1, None


def fused_ssim(img1, img2):
    """Mean SSIM of [B,CH,H,W] images (11x11, sigma 1.5, zero padded), differentiable in img1."""
    return _FusedSSIM.apply(img1, img2)


class _FusedL1SSIMLoss(torch.autograd.Function):
    """mask None: the unmasked entries; a mask: the _masked_ entries, which take it as their last argument."""

    @staticmethod
    def forward(ctx, image, gt_u8, lambda_dssim, mask, mask_count):
        L = _lib.lib()
        assert image.dim() == 3 and image.shape[0] == 3 and image.dtype == F32 and image.is_cuda
        _, H, W = image.shape
        gt_u8 = gt_u8.contiguous()
        assert gt_u8.dtype == U8 and gt_u8.shape == image.shape
        if mask is not None:
            mask = mask.contiguous()
            assert mask.dtype == U8 and tuple(mask.shape) == (H, W) and mask.device == image.device
        need = image.requires_grad
        slots = L.clmgs_loss_slots()
        partials = torch.zeros((slots, 2), dtype=F32, device=image.device)
        maps = torch.empty((3, 3, H, W), dtype=F32, device=image.device) if need else None
        sc, sy, sx = image.stride()
        fwd, extra = (L.clmgs_l1_ssim_loss_fwd, ()) if mask is None else (L.clmgs_l1_ssim_loss_masked_fwd, (dptr(mask, U8),))
        check(fwd(stream(), H, W, ctypes.c_void_p(image.data_ptr()), sc, sy, sx,
                  dptr(gt_u8, U8), dptr(partials),
                  dptr(maps[0] if need else None, F32, True),
                  dptr(maps[1] if need else None, F32, True),
                  dptr(maps[2] if need else None, F32, True), *extra))
        ctx.lam = float(lambda_dssim)
        if need:
            ctx.save_for_backward(image, gt_u8, maps, mask)
        if mask is not None:
            tot = partials.sum(dim=0)
            return masked_loss_value(tot[0], tot[1], ctx.lam, mask_count, H, W)
        tot = partials.sum(dim=0) / float(image.numel())
        return (1.0 - ctx.lam) * tot[0] + ctx.lam * (1.0 - tot[1])

    @staticmethod
    def backward(ctx, v):
        L = _lib.lib()
        image, gt_u8, maps, mask = ctx.saved_tensors
        _, H, W = image.shape
        v = v.reshape(1).to(F32).contiguous()
        v_img = torch.empty_strided(image.shape, image.stride(), dtype=F32, device=image.device)
        sc, sy, sx = image.stride()
        bwd, extra = (L.clmgs_l1_ssim_loss_bwd, ()) if mask is None else (L.clmgs_l1_ssim_loss_masked_bwd, (dptr(mask, U8),))
        check(bwd(stream(), H, W, ctypes.c_void_p(image.data_ptr()), sc, sy, sx,
                  dptr(gt_u8, U8), dptr(v, F32), ctx.lam, dptr(maps[0]),
                  dptr(maps[1]), dptr(maps[2]),
                  ctypes.c_void_p(v_img.data_ptr()), *extra))
        return v_img, None, None, None, None


def masked_loss_value(l1_sum, ssim_sum, lambda_dssim, mask_count, H, W):
    """The masked loss from the masked forward's two partial sums (over counted pixels) and the HOST count of
    counted pixels: ((1-lambda) * l1 + lambda * (3 * count - ss)) / (3 H W)."""
    return ((1.0 - lambda_dssim) * l1_sum + lambda_dssim * (float(3 * int(mask_count)) - ssim_sum)) / float(3 * H * W)


def fused_l1_ssim_loss(image, gt_u8, lambda_dssim=0.2, mask=None, mask_count=None):
    """(1-lambda) * L1 + lambda * (1 - SSIM) of image [3,H,W] (any strides, e.g. a permuted view
    of the rasterizer's [H,W,3] output) against a uint8 [3,H,W] ground truth; one forward and one
    backward kernel (strategies/base_engine.py:79-103 semantics).
    mask: uint8 [H,W] on the image's device, 0 = ignored pixel, anything else = counted (None: every pixel, the
    unmasked kernels).  Ignored pixels add nothing to either term; the SSIM statistics are those of the whole images
    and the divisor stays 3 H W ("Masked loss").  mask_count: the number of counted pixels as a
    host integer (Camera.loss_mask_count); counted here, with one read-back, when not given."""
    if mask is not None and mask_count is None:
        mask_count = int(torch.count_nonzero(mask).item())
    return _FusedL1SSIMLoss.apply(image, gt_u8, lambda_dssim, mask, mask_count)


# ------------------------------------------------------- depth regularisation
class _InvDepthL1(torch.autograd.Function):
    @staticmethod
    def forward(ctx, I, raw, scale, offset, weight, mask):
        L = _lib.lib()
        assert I.dim() == 2 and I.dtype == F32 and I.is_cuda
        H, W = I.shape
        raw = raw.contiguous()
        assert raw.dtype == torch.uint16 and tuple(raw.shape) == (H, W) and raw.device == I.device
        if mask is not None:
            mask = mask.contiguous()
            assert mask.dtype == U8 and tuple(mask.shape) == (H, W) and mask.device == I.device
        rows = int(L.clmgs_invdepth_partials_rows(H, W))
        partials = torch.empty((rows,), dtype=F32, device=I.device)
        total = torch.empty((1,), dtype=F32, device=I.device)
        v_I = torch.empty((H, W), dtype=F32, device=I.device)
        check(L.clmgs_invdepth_l1_fwd_bwd(stream(), H, W, ctypes.c_void_p(I.data_ptr()), *I.stride(),
                                          dptr(raw, torch.uint16), float(scale), float(offset), dptr(mask, U8, True),
                                          float(weight), dptr(v_I), *v_I.stride(), dptr(partials)))
        check(L.clmgs_invdepth_finish(stream(), rows, dptr(partials), dptr(total)))
        ctx.save_for_backward(v_I)
        return total[0] * (float(weight) / float(H * W))

    @staticmethod
    def backward(ctx, v):
        (v_I,) = ctx.saved_tensors
        return v_I * v, None, None, None, None, None


def invdepth_l1_loss(I, raw, scale, offset, weight, mask=None):
    """The depth term of a camera: weight * sum_p m_p |I_p - prior_p| / (H*W) with prior = raw / 65536 * scale + offset.
    I [H,W] float32 (any strides, e.g. channel 3 of the rasterizer's [1,H,W,4] output: the rendered inverse depth),
    raw uint16 [H,W], mask uint8 [H,W] (0 = ignored) or None; differentiable in I, d|x|/dx = 0 at 0.  One kernel computes
    the partial sums and the cotangent (csrc/invdepth.hip; DESIGN.md section 3, "Depth regularisation")."""
    return _InvDepthL1.apply(I, raw, float(scale), float(offset), float(weight), mask)


def camera_depth_term(inv_depth, camera):
    """invdepth_l1_loss of a rendered inverse-depth map [H,W] against the camera's prior (cameras.camera_invdepth), with
    the camera's loss mask and the current iteration's weight.  What the op-by-op engines add to the camera's loss."""
    from .cameras import camera_invdepth, camera_loss_mask
    raw, scale, offset = camera_invdepth(camera)
    return invdepth_l1_loss(inv_depth, raw, scale, offset, utils.depth_l1_weight(), camera_loss_mask(camera)[0])


def check_depth_prior_args(camera):
    """A camera with an inverse-depth prior under absgrad: refused before anything runs (absgrad blends three channels
    only).  -> whether the camera has a prior."""
    if getattr(camera, "invdepth", None) is None:
        return False
    if bool(getattr(utils.get_args(), "absgrad", False)):
        raise ValueError("absgrad with an inverse-depth prior is not built (absgrad blends three channels only): train "
                         "without absgrad or without depth priors")
    return True


# ------------------------------------------- colour stages: exposure compensation, bilateral grid
def _view_ptr(t):
    return ctypes.c_void_p(t.data_ptr())


class _ColourStage:
    """One kind of colour stage between the rasterizer and the loss, as the library offers it: the parameter check, the
    forward entry, the backward entry with its partial rows, the finish entry that ADDS the rows into a gradient in the
    fixed order of csrc/rowsum.h.  An image travels as a pointer and its (sc, sy, sx) element strides.  Driven by
    _ApplyColour below (op by op) and by fused.camera_forward_finish / camera_backward (the engines)."""

    def __init__(self, kind, expected, ok, dims, rows, width, finish_args):
        self.kind, self.expected, self.ok = kind, expected, ok  # ok(P): the shape the kernels take; `expected` names it
        self.dims = dims                # P -> what the forward and backward entries take behind the parameter pointer
        self.rows, self.width = rows, width  # (L, H, W, P) -> partial rows of a backward; P -> floats per row
        self.finish_args = finish_args  # (H, W, P, rows) -> what the finish entry takes before `partials, grad`

    def check(self, P, what):
        if P.dtype != F32 or not self.ok(P):
            raise _lib.ClmgsError(f"{what} must be {self.expected}, got {P.dtype} {tuple(P.shape)}")

    def forward(self, s, H, W, x, xs, P, y, ys):
        check(getattr(_lib.lib(), f"clmgs_{self.kind}_fwd")(s, H, W, x, *xs, dptr(P, F32), *self.dims(P), y, *ys))

    def backward(self, s, H, W, x, xs, P, g, gs, v, vs, device):
        """v = dL/dx from g = dL/dy (v may be g itself, as the same view) -> the partial rows of dL/dP, for finish()."""
        L = _lib.lib()
        partials = torch.empty((self.rows(L, H, W, P), self.width(P)), dtype=F32, device=device)
        check(getattr(L, f"clmgs_{self.kind}_bwd")(s, H, W, x, *xs, dptr(P, F32), *self.dims(P), g, *gs, v, *vs,
                                                   dptr(partials)))
        return partials

    def finish(self, s, H, W, P, partials, grad):
        check(getattr(_lib.lib(), f"clmgs_{self.kind}_grad_finish")(
            s, *self.finish_args(H, W, P, int(partials.shape[0])), dptr(partials), dptr(grad, F32)))


COLOUR = {
    "exposure": _ColourStage(
        "exposure", "float32 [3,4]", lambda E: tuple(E.shape) == (3, 4), lambda E: (),
        lambda L, H, W, E: int(L.clmgs_exposure_partials_rows(H, W)), lambda E: 12, lambda H, W, E, rows: (rows,)),
    "bilagrid": _ColourStage(
        "bilagrid", "contiguous float32 [L,Hg,Wg,12]", lambda G: G.dim() == 4 and G.shape[3] == 12 and G.is_contiguous(),
        lambda G: tuple(G.shape[:3]), lambda L, H, W, G: int(L.clmgs_bilagrid_partials_rows(H, W, G.shape[1], G.shape[2])),
        lambda G: 48 * G.shape[0], lambda H, W, G, rows: (H, W, *G.shape[:3])),
}


class _ApplyColour(torch.autograd.Function):
    @staticmethod
    def forward(ctx, image, param, kind):
        stage = COLOUR[kind]
        assert image.dim() == 3 and image.shape[0] == 3 and image.dtype == F32 and image.is_cuda
        P = param.detach().contiguous()
        assert P.dtype == F32 and P.device == image.device and stage.ok(P)
        _, H, W = image.shape
        out = torch.empty_strided(image.shape, image.stride(), dtype=F32, device=image.device)
        stage.forward(stream(), H, W, _view_ptr(image), image.stride(), P, _view_ptr(out), out.stride())
        ctx.stage = stage
        ctx.save_for_backward(image, P)
        return out

    @staticmethod
    def backward(ctx, v):
        stage, (image, P) = ctx.stage, ctx.saved_tensors
        _, H, W = image.shape
        assert v.dtype == F32 and v.shape == image.shape
        v_img = torch.empty_strided(image.shape, image.stride(), dtype=F32, device=image.device)
        partials = stage.backward(stream(), H, W, _view_ptr(image), image.stride(), P, _view_ptr(v), v.stride(),
                                  _view_ptr(v_img), v_img.stride(), image.device)
        v_P = torch.zeros_like(P)
        stage.finish(stream(), H, W, P, partials, v_P)
        return v_img, v_P, None


def apply_exposure(image, exposure):
    """A camera's exposure transform on a rendered image: image [3,H,W] float32 (any strides, e.g. the permuted view of
    the rasterizer's [H,W,3] output), exposure float32 [3,4] on the same device ->
    y[c] = x[0] E[0][c] + x[1] E[1][c] + x[2] E[2][c] + E[c][3] in the image's layout, unclamped; differentiable in
    both (csrc/exposure.hip; DESIGN.md section 3, "Exposure")."""
    return _ApplyColour.apply(image, exposure, "exposure")


def apply_bilagrid(image, grid):
    """A camera's bilateral grid on a rendered image: image [3,H,W] float32 (any strides, e.g. the permuted view of the
    rasterizer's [H,W,3] output), grid float32 [L,Hg,Wg,12] on the same device -> the image in the same layout, every
    pixel through the 3x4 affine transform the grid gives at its position and luminance, unclamped; differentiable in
    both, the gradient through the luminance included (csrc/bilagrid.hip; DESIGN.md section 3, "Bilateral grid")."""
    return _ApplyColour.apply(image, grid, "bilagrid")


def apply_camera_colour(image, camera):
    """The camera's colour stage (cameras.camera_colour: an exposure row or a bilateral grid) on a rendered image, the
    parameter's gradient ADDED into the camera's gradient view by the backward; the image itself for a camera without a
    stage.  What the op-by-op engines and the evaluation renders call."""
    from .cameras import camera_colour
    colour = camera_colour(camera)
    if colour is None:
        return image
    kind, param, grad = colour
    if not (torch.is_grad_enabled() and image.requires_grad) or grad is None:
        return _ApplyColour.apply(image, param.detach(), kind)
    leaf = param.detach().requires_grad_(True)
    leaf.register_hook(lambda g: (grad.add_(g), None)[1])
    return _ApplyColour.apply(image, leaf, kind)


# ------------------------------------------------------------ learnable sky (csrc/sky.hip)
I64 = torch.int64


def _host_f32(t, n, what):
    """A camera matrix as the entries take it: a contiguous host float32 array of n values."""
    import numpy as np
    a = t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)
    a = np.ascontiguousarray(a, dtype=np.float32).reshape(-1)
    if a.size != n:
        raise _lib.ClmgsError(f"{what} must hold {n} values, got {a.size}")
    return a


def check_sky(sky, what="sky"):
    if not (isinstance(sky, torch.Tensor) and sky.dtype == F32 and sky.dim() == 3 and sky.shape[2] == 3
            and sky.shape[0] >= 1 and sky.shape[1] >= 1 and sky.is_contiguous()):
        raise _lib.ClmgsError(f"{what} must be contiguous float32 [Hs,Ws,3], got "
                              f"{getattr(sky, 'dtype', type(sky))} {tuple(getattr(sky, 'shape', ()))}")


def sky_forward(s, H, W, x, xs, alphas, vm, K, sky, y, ys):
    """clmgs_sky_fwd on raw views: x, y pointers with (sc, sy, sx) strides, vm / K host arrays."""
    check(_lib.lib().clmgs_sky_fwd(s, H, W, x, *xs, dptr(alphas, F32), vm.ctypes.data_as(ctypes.c_void_p),
                                   K.ctypes.data_as(ctypes.c_void_p), dptr(sky, F32), int(sky.shape[0]),
                                   int(sky.shape[1]), y, *ys))


def sky_backward(s, H, W, g, gs, alphas, vm, K, sky, v_alphas, acc):
    """clmgs_sky_bwd on raw views: STORES v_alphas [H,W], ADDS the map gradient into acc int64 [Hs,Ws,3]."""
    if acc.dtype != I64 or tuple(acc.shape) != tuple(sky.shape):
        raise _lib.ClmgsError(f"the sky accumulator must be int64 {tuple(sky.shape)}, got {acc.dtype} {tuple(acc.shape)}")
    check(_lib.lib().clmgs_sky_bwd(s, H, W, g, *gs, dptr(alphas, F32), vm.ctypes.data_as(ctypes.c_void_p),
                                   K.ctypes.data_as(ctypes.c_void_p), dptr(sky, F32), int(sky.shape[0]),
                                   int(sky.shape[1]), dptr(v_alphas, F32), dptr(acc, I64)))


def sky_acc_add(s, src, dst):
    assert src.dtype == I64 and dst.dtype == I64 and src.numel() == dst.numel()
    check(_lib.lib().clmgs_sky_acc_add(s, int(src.numel()), dptr(src, I64), dptr(dst, I64)))


def sky_grad_convert(s, acc, grad):
    """grad += acc * 2^-48, acc = 0 (the one place the fixed-point sums become floats)."""
    assert acc.dtype == I64 and grad.dtype == F32 and acc.numel() == grad.numel()
    check(_lib.lib().clmgs_sky_grad_convert(s, int(acc.numel()), dptr(acc, I64), dptr(grad, F32)))


class _ApplySky(torch.autograd.Function):
    @staticmethod
    def forward(ctx, image, alphas, sky, vm, K, acc):
        assert image.dim() == 3 and image.shape[0] == 3 and image.dtype == F32 and image.is_cuda
        _, H, W = image.shape
        assert alphas.dtype == F32 and alphas.device == image.device and alphas.numel() == H * W
        S = sky.detach()
        check_sky(S)
        assert S.device == image.device
        a = alphas.detach().reshape(H, W).contiguous()
        out = torch.empty_strided(image.shape, image.stride(), dtype=F32, device=image.device)
        sky_forward(stream(), H, W, _view_ptr(image), image.stride(), a, vm, K, S, _view_ptr(out), out.stride())
        ctx.cam, ctx.acc, ctx.alphas_shape = (vm, K), acc, alphas.shape
        ctx.save_for_backward(a, S)
        return out

    @staticmethod
    def backward(ctx, v):
        a, S = ctx.saved_tensors
        H, W = a.shape
        assert v.dtype == F32 and tuple(v.shape) == (3, H, W)
        v_alphas = torch.empty_like(a)
        acc = ctx.acc if ctx.acc is not None else torch.zeros(S.shape, dtype=I64, device=S.device)
        sky_backward(stream(), H, W, _view_ptr(v), v.stride(), a, *ctx.cam, S, v_alphas, acc)
        v_sky = None
        if ctx.acc is None and ctx.needs_input_grad[2]:
            v_sky = torch.zeros_like(S)
            sky_grad_convert(stream(), acc, v_sky)
        return v, v_alphas.reshape(ctx.alphas_shape), v_sky, None, None, None


def apply_sky(image, alphas, sky, viewmat, K):
    """The sky map behind a rendered image: image [3,H,W] float32 rendered with NO background (any strides, e.g. the
    permuted view of the rasterizer's [H,W,3] output), alphas [H,W] or [1,H,W], sky float32 [Hs,Ws,3] (equirectangular,
    world axes) on the same device, viewmat [4,4] world->camera and K [3,3] of the camera ->
    y = x + (1 - alpha) * bilinear(sky; ray of the pixel) in the image's layout, unclamped; differentiable in the image
    (identity), alphas and sky, not in the camera (csrc/sky.hip; DESIGN.md section 3, "Sky")."""
    return _ApplySky.apply(image, alphas, sky, _host_f32(viewmat, 16, "viewmat"), _host_f32(K, 9, "K"), None)


def apply_camera_sky(image, alphas, camera):
    """The camera's sky (cameras.camera_sky) behind a rendered image and its alpha image; the map's gradient ADDED, in
    fixed point, into the accumulator the camera carries (a training camera; sky.SkyModel converts it once per step);
    the image itself for a camera without a sky.  What the op-by-op engines and the evaluation renders call."""
    from .cameras import camera_sky
    from .fused import _cam_host
    sky = camera_sky(camera)
    if sky is None:
        return image
    table, acc = sky
    vm, K, _ = _cam_host(camera)
    train = torch.is_grad_enabled() and (image.requires_grad or alphas.requires_grad)
    return _ApplySky.apply(image, alphas, table.detach(), vm, K, acc if train else None)


# ------------------------------------------------------------ resolution schedule
def level_size(H, W, level):
    """(Ho, Wo) of level `level` of an H x W image: ceil(H / 2^level), ceil(W / 2^level)."""
    f = 1 << int(level)
    return (int(H) + f - 1) // f, (int(W) + f - 1) // f


@torch.no_grad()
def area_resample(t, level, out=None, mask=False, count=None):
    """Exact integer area resampling of a device image to level `level` (csrc/resample.hip; DESIGN.md section 3,
    "Resolution schedule"): t uint8 [3,H,W] (any number of planes) or [H,W], or uint16 [H,W], contiguous -> the same dtype
    and rank at level_size(H, W, level), rounded half up.  `out`: a caller-owned contiguous buffer of that shape and dtype
    (written and returned; nothing is allocated).  mask=True (uint8 [H,W], 0 = ignored): a cell is counted (255) when at
    least half of its area is; returns (mask, count) with count a device int64 [1] (`count=`: a caller-owned one).
    level 0 is the input itself: returned as it is (copied into `out` when one is given), no kernel."""
    level = int(level)
    if level < 0:
        raise ValueError(f"area_resample: level must be >= 0, got {level}")
    if not (t.is_cuda and t.is_contiguous() and t.dim() in (2, 3) and t.dtype in (U8, torch.uint16)):
        raise _lib.ClmgsError(f"area_resample: contiguous uint8 [P,H,W] / [H,W] or uint16 [H,W] device tensor expected, "
                              f"got {t.dtype} {tuple(t.shape)}")
    if t.dtype == torch.uint16 and t.dim() != 2:
        raise _lib.ClmgsError(f"area_resample: a uint16 input is one plane [H,W], got {tuple(t.shape)}")
    if mask and (t.dtype != U8 or t.dim() != 2):
        raise _lib.ClmgsError(f"area_resample: a mask is uint8 [H,W], got {t.dtype} {tuple(t.shape)}")
    H, W = t.shape[-2:]
    shape = tuple(t.shape[:-2]) + level_size(H, W, level)
    if out is not None and not (out.is_cuda and out.is_contiguous() and out.dtype == t.dtype and tuple(out.shape) == shape
                                and out.device == t.device):
        raise _lib.ClmgsError(f"area_resample: out must be a contiguous {t.dtype} {shape} tensor on {t.device}, got "
                              f"{out.dtype} {tuple(out.shape)}")
    if level == 0:
        res = t if out is None else out.copy_(t)
        return (res, torch.count_nonzero(t).reshape(1)) if mask else res
    if out is None:
        out = torch.empty(shape, dtype=t.dtype, device=t.device)
    L = _lib.lib()
    if mask:
        if count is None:
            count = torch.empty((1,), dtype=I64, device=t.device)
        check(L.clmgs_area_resample_mask(stream(), H, W, level, dptr(t, U8), dptr(out, U8), dptr(count, I64)))
        return out, count
    if t.dtype == U8:
        planes = t.shape[0] if t.dim() == 3 else 1
        check(L.clmgs_area_resample_u8(stream(), planes, H, W, level, dptr(t, U8), dptr(out, U8)))
    else:
        check(L.clmgs_area_resample_u16(stream(), H, W, level, dptr(t, torch.uint16), dptr(out, torch.uint16)))
    return out


# ------------------------------------------------------------ lens distortion
# COLMAP camera model -> where its parameters go in the lens record (fx, fy, cx, cy, k1, k2, k3, k4, p1, p2); a model
# with one focal length fills fx and fy with it
_LENS_MODELS = {
    "SIMPLE_PINHOLE": ("f", "cx", "cy"),
    "PINHOLE": ("fx", "fy", "cx", "cy"),
    "SIMPLE_RADIAL": ("f", "cx", "cy", "k1"),
    "RADIAL": ("f", "cx", "cy", "k1", "k2"),
    "OPENCV": ("fx", "fy", "cx", "cy", "k1", "k2", "p1", "p2"),
    "OPENCV_FISHEYE": ("fx", "fy", "cx", "cy", "k1", "k2", "k3", "k4"),
}
_LENS_FIELDS = ("fx", "fy", "cx", "cy", "k1", "k2", "k3", "k4", "p1", "p2")


class Lens:
    """The lens of a COLMAP camera as csrc/undistort.hip takes it ("Lens distortion"): a host object.
    `model_name`, `params`: COLMAP's model and its parameter list; `width`, `height`: the image size the intrinsics are
    in pixels of (COLMAP's convention: the centre of the top-left pixel is at (0.5, 0.5)).  Accepted: SIMPLE_PINHOLE,
    PINHOLE, SIMPLE_RADIAL, RADIAL, OPENCV, OPENCV_FISHEYE; every other model is refused by name."""

    def __init__(self, model_name, params, width, height):
        if model_name not in _LENS_MODELS:
            raise ValueError(f"COLMAP camera model {model_name} cannot be undistorted here: the lens record holds "
                             f"{' / '.join(_LENS_MODELS)} only; undistort the dataset with COLMAP's image_undistorter")
        names = _LENS_MODELS[model_name]
        params = [float(p) for p in params]
        if len(params) != len(names):
            raise ValueError(f"COLMAP camera model {model_name} takes {len(names)} parameters ({', '.join(names)}), "
                             f"got {len(params)}")
        given = dict(zip(names, params))
        if "f" in given:
            given["fx"] = given["fy"] = given.pop("f")
        self.model, self.params = model_name, tuple(params)
        self.width, self.height = int(width), int(height)
        self.fisheye = model_name == "OPENCV_FISHEYE"
        for name in _LENS_FIELDS:
            setattr(self, name, given.get(name, 0.0))
        if self.width < 1 or self.height < 1 or not all(map(_finite, self.record())) or self.fx <= 0 or self.fy <= 0:
            raise ValueError(f"COLMAP camera {model_name} {self.width}x{self.height} {list(params)}: the size and the focal "
                             "lengths must be positive and every parameter finite")

    def record(self):
        """The ten doubles fx, fy, cx, cy, k1, k2, k3, k4, p1, p2."""
        return tuple(getattr(self, name) for name in _LENS_FIELDS)

    def at(self, width, height):
        """The same lens for the image decoded at width x height (`-r`, or files of another size than the model's): focal
        lengths and principal point scale with the size, the distortion terms act on normalised coordinates and stay."""
        width, height = int(width), int(height)
        if (width, height) == (self.width, self.height):
            return self
        out = Lens.__new__(Lens)
        out.__dict__.update(self.__dict__)
        sx, sy = width / self.width, height / self.height
        out.fx, out.cx, out.fy, out.cy = self.fx * sx, self.cx * sx, self.fy * sy, self.cy * sy
        out.width, out.height = width, height
        return out

    def is_identity(self, out_size=None, zoom=1.0):
        """True when undistorting an image of this lens' size to `out_size` (Ho, Wo; None: the same size) changes nothing:
        a perspective model, every k and p zero, zoom 1, the same size and the principal point exactly at the centre.  A
        caller then launches nothing."""
        same = out_size is None or (int(out_size[0]), int(out_size[1])) == (self.height, self.width)
        return (not self.fisheye and same and float(zoom) == 1.0 and not any(self.record()[4:])
                and self.cx == self.width / 2.0 and self.cy == self.height / 2.0)

    def __repr__(self):
        return f"Lens({self.model}, {list(self.params)}, {self.width}x{self.height})"


def _finite(v):
    return v == v and v not in (float("inf"), float("-inf"))


def check_undistort_zoom(zoom):
    """The zoom as a float; anything but a positive finite number is refused (the operator, the loader and
    trainer.check_training share the message)."""
    zoom = float(zoom)
    if not (_finite(zoom) and zoom > 0):
        raise ValueError(f"--undistort_zoom must be positive and finite, got {zoom}")
    return zoom


@torch.no_grad()
def undistort(src, lens, out_size=None, zoom=1.0, src_mask=None, want_valid=False, out=None):
    """Remaps a distorted device image onto the ideal centred pinhole (csrc/undistort.hip; DESIGN.md section 3, "Lens
    distortion"): src uint8 [3,H,W] (any number of planes) / [H,W] or uint16 [H,W], contiguous; `lens` a Lens (taken at
    the size of `src`: Lens.at); out_size (Ho, Wo), None = the size of `src`; the pinhole's focal lengths are
    fx * zoom, fy * zoom (zoom < 1 widens it to keep more of a barrel or fisheye frame).  `src_mask` (uint8 [H,W], uint8
    input only): a pixel is valid only if all four source pixels it blends are non-zero there.  Returns the image (same
    dtype and rank; `out`: a caller-owned buffer, written and returned); with want_valid (uint8 input only)
    (image, valid, count): valid uint8 [Ho,Wo] 255 / 0 and a device int64 [1], the number of valid pixels.  The kernel
    is launched for any lens: a caller that wants to launch nothing for an identity lens asks Lens.is_identity first."""
    zoom = check_undistort_zoom(zoom)
    if not (isinstance(src, torch.Tensor) and src.is_cuda and src.is_contiguous() and src.dim() in (2, 3)
            and src.dtype in (U8, torch.uint16)):
        raise _lib.ClmgsError("undistort: contiguous uint8 [P,H,W] / [H,W] or uint16 [H,W] device tensor expected, got "
                              f"{getattr(src, 'dtype', type(src))} {tuple(getattr(src, 'shape', ()))}")
    u16 = src.dtype == torch.uint16
    if u16 and (src.dim() != 2 or src_mask is not None or want_valid):
        raise _lib.ClmgsError("undistort: a uint16 input is one plane [H,W] and takes no mask and gives no valid map")
    H, W = (int(v) for v in src.shape[-2:])
    lens = lens.at(W, H)
    Ho, Wo = (H, W) if out_size is None else (int(out_size[0]), int(out_size[1]))
    if Ho < 1 or Wo < 1:
        raise ValueError(f"undistort: out_size must be positive, got {out_size}")
    shape = tuple(src.shape[:-2]) + (Ho, Wo)
    if out is not None and not (out.is_cuda and out.is_contiguous() and out.dtype == src.dtype and tuple(out.shape) == shape
                                and out.device == src.device):
        raise _lib.ClmgsError(f"undistort: out must be a contiguous {src.dtype} {shape} tensor on {src.device}, got "
                              f"{out.dtype} {tuple(out.shape)}")
    if src_mask is not None and not (src_mask.is_cuda and src_mask.is_contiguous() and src_mask.dtype == U8
                                     and tuple(src_mask.shape) == (H, W) and src_mask.device == src.device):
        raise _lib.ClmgsError(f"undistort: src_mask must be a contiguous uint8 [{H}, {W}] tensor on {src.device}, got "
                              f"{src_mask.dtype} {tuple(src_mask.shape)}")
    if out is None:
        out = torch.empty(shape, dtype=src.dtype, device=src.device)
    rec = (ctypes.c_double * 10)(*lens.record())
    fxo, fyo = lens.fx * zoom, lens.fy * zoom
    L = _lib.lib()
    if u16:
        check(L.clmgs_undistort_u16(stream(), H, W, Ho, Wo, rec, int(lens.fisheye), fxo, fyo, dptr(src, torch.uint16),
                                    dptr(out, torch.uint16)))
        return out
    valid = torch.empty((Ho, Wo), dtype=U8, device=src.device) if want_valid else None
    count = torch.empty((1,), dtype=I64, device=src.device) if want_valid else None
    planes = src.shape[0] if src.dim() == 3 else 1
    check(L.clmgs_undistort_u8(stream(), planes, H, W, Ho, Wo, rec, int(lens.fisheye), fxo, fyo, dptr(src, U8),
                               dptr(src_mask, U8, allow_none=True), dptr(out, U8), dptr(valid, U8, allow_none=True),
                               dptr(count, I64, allow_none=True)))
    return (out, valid, count) if want_valid else out


# ------------------------------------------------------------ compressed models
VQ_MAX_K = 65536


def _vq_rows(t, what, n=None):
    """A [n,48] float32 contiguous device table (`n`: the number of rows it must have); anything else is refused."""
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise _lib.ClmgsError(f"{what} must be a tensor on the device (no CPU fallback in clm_gs_amd)")
    if not t.is_contiguous():
        raise _lib.ClmgsError(f"{what} must be contiguous")
    if t.dtype != F32 or t.dim() != 2 or t.shape[1] != 48 or (n is not None and t.shape[0] != n):
        raise _lib.ClmgsError(f"{what}: float32 [{'N' if n is None else n}, 48] expected, got {t.dtype} {tuple(t.shape)}")
    return t


def _vq_sizes(rows, codebook):
    _vq_rows(rows, "vq: rows")
    _vq_rows(codebook, "vq: codebook")
    n, k = int(rows.shape[0]), int(codebook.shape[0])
    if not 1 <= k <= VQ_MAX_K:
        raise _lib.ClmgsError(f"vq: K must be in [1, {VQ_MAX_K}], got {k}")
    if n >= 1 << 31:
        raise _lib.ClmgsError(f"vq: N must be below 2^31, got {n}")
    if n < 1:
        raise _lib.ClmgsError("vq: at least one row expected")
    if rows.device != codebook.device:
        raise _lib.ClmgsError(f"vq: rows are on {rows.device}, the codebook on {codebook.device}")
    return n, k


@torch.no_grad()
def vq_assign(rows, codebook, want_dist=False):
    """Nearest centroid of every SH row over its 45 higher-order coefficients (csrc/vq.hip; DESIGN.md section 3,
    "Compressed models"): rows float32 [N,48], codebook float32 [K,48], both contiguous on the device, columns 0..2 (the
    DC) ignored on both sides -> idx int32 [N] = argmin_k sum_{j=3..47} (x_j - c_kj)^2, the lowest k on an exact tie;
    with want_dist (idx, dist), dist float32 [N] that squared distance.  1 <= K <= 65536, N < 2^31."""
    n, k = _vq_sizes(rows, codebook)
    L = _lib.lib()
    idx = torch.empty((n,), dtype=I32, device=rows.device)
    dist = torch.empty((n,), dtype=F32, device=rows.device) if want_dist else None
    nbytes = int(L.clmgs_vq_assign_temp_bytes(k))
    temp = torch.empty((nbytes,), dtype=U8, device=rows.device)
    check(L.clmgs_vq_assign(stream(), n, k, dptr(rows, F32), dptr(codebook, F32), dptr(idx, I32),
                            dptr(dist, F32, allow_none=True), dptr(temp), nbytes))
    return (idx, dist) if want_dist else idx


def vq_scale(n, max_abs):
    """The power of two the Lloyd update multiplies a coefficient by before it rounds it to an integer: 2^(61 - e) with
    e the binary exponent of n * max_abs (n * max_abs < 2^e), so that n * (max_abs * scale + 1/2) < 2^62 and a sum of n
    rounded values fits an int64; an all-zero table takes 1."""
    import math
    prod = float(n) * float(max_abs)
    if not math.isfinite(prod):
        raise ValueError(f"vq: the rows must be finite, got max |x| = {max_abs}")
    if prod <= 0.0:
        return 1.0
    return math.ldexp(1.0, max(-900, min(900, 61 - math.frexp(prod)[1])))


@torch.no_grad()
def vq_update(rows, idx, codebook, scale=None):
    """One Lloyd update (csrc/vq.hip): every centroid becomes the mean of the rows assigned to it, summed in fixed point
    (rint(x * scale) as int64 by integer atomics: the same bits whatever the order of the rows) -> (codebook, counts):
    a NEW float32 [K,48] codebook (columns 0..2 zero; a centroid without rows keeps its previous columns 3..47) and
    counts int64 [K].  idx int32 [N] as vq_assign returns it.  `scale`: None = vq_scale(N, max |x|)."""
    n, k = _vq_sizes(rows, codebook)
    if not (isinstance(idx, torch.Tensor) and idx.is_cuda and idx.is_contiguous() and idx.dtype == I32
            and tuple(idx.shape) == (n,) and idx.device == rows.device):
        raise _lib.ClmgsError(f"vq_update: idx must be a contiguous int32 [{n}] tensor on {rows.device}, got "
                              f"{getattr(idx, 'dtype', type(idx))} {tuple(getattr(idx, 'shape', ()))}")
    if scale is None:
        lo, hi = torch.aminmax(rows)
        scale = vq_scale(n, max(-float(lo), float(hi)))
    L = _lib.lib()
    acc = torch.zeros((k, 45), dtype=I64, device=rows.device)
    counts = torch.zeros((k,), dtype=I64, device=rows.device)
    out = codebook.clone()
    check(L.clmgs_vq_accumulate(stream(), n, k, dptr(rows, F32), dptr(idx, I32), float(scale), dptr(acc, I64),
                                dptr(counts, I64)))
    check(L.clmgs_vq_finish(stream(), k, dptr(acc, I64), dptr(counts, I64), float(scale), dptr(out, F32)))
    return out, counts


# ------------------------------------------------------------------ mesh export
TSDF_MAX_B = 16


def _tsdf_grid(grid):
    if not (isinstance(grid, torch.Tensor) and grid.is_cuda and grid.is_contiguous() and grid.dtype == F32
            and grid.dim() == 4 and grid.shape[0] == 6):
        raise _lib.ClmgsError("tsdf: the volume is a contiguous float32 [6, nz, ny, nx] device tensor, got "
                              f"{getattr(grid, 'dtype', type(grid))} {tuple(getattr(grid, 'shape', ()))}")
    nz, ny, nx = (int(v) for v in grid.shape[1:])
    if min(nx, ny, nz) < 2 or nx * ny * nz >= 1 << 31:
        raise _lib.ClmgsError(f"tsdf: every side of the volume must be >= 2 and nx ny nz < 2^31, got {nx} x {ny} x {nz}")
    return nx, ny, nz


def _tsdf_images(what, dev, cams, depth, alpha, rgb=None):
    """The checks tsdf_integrate makes of its images and records -> (cams float64 [B,16], B, H, W)."""
    import numpy as np
    cams = np.ascontiguousarray(cams.numpy() if isinstance(cams, torch.Tensor) else cams, dtype=np.float64)
    if not (isinstance(depth, torch.Tensor) and depth.dim() == 3 and cams.shape == (depth.shape[0], 16) and depth.shape[0] >= 1):
        raise _lib.ClmgsError(f"{what}: depth [B,H,W] and cams [B,16] expected, got {tuple(getattr(depth, 'shape', ()))} "
                              f"and {cams.shape}")
    B, H, W = (int(v) for v in depth.shape)
    for t, shape, name in ((depth, (B, H, W), "depth"), (alpha, (B, H, W), "alpha"), (rgb, (B, 3, H, W), "rgb")):
        if name == "rgb" and rgb is None:
            continue
        if not (isinstance(t, torch.Tensor) and t.is_cuda and t.is_contiguous() and t.dtype == F32 and tuple(t.shape) == shape
                and t.device == dev):
            raise _lib.ClmgsError(f"{what}: {name} must be a contiguous float32 {shape} tensor on {dev}, got "
                                  f"{getattr(t, 'dtype', type(t))} {tuple(getattr(t, 'shape', ()))}")
    return cams, B, H, W


def _tsdf_trunc(what, trunc):
    trunc32 = float(torch.tensor(float(trunc), dtype=F32))
    if not (_finite(trunc32) and trunc32 > 0):
        raise ValueError(f"{what}: trunc must be positive and finite, got {trunc}")
    return trunc32



def _tsdf_batches(cams, B):
    """The launches of at most 16 cameras, in order -> (b0, b1, the ctypes record of cams[b0:b1]) each."""
    for b0 in range(0, B, TSDF_MAX_B):
        b1 = min(B, b0 + TSDF_MAX_B)
        yield b0, b1, (ctypes.c_double * (16 * (b1 - b0)))(*cams[b0:b1].reshape(-1))


def _tsdf_g2w(what, grid_to_world):
    """A finite 3x4 grid_to_world (numpy or tensor, on the host) -> the ctypes record of its 12 doubles."""
    import numpy as np
    g2w = np.ascontiguousarray(grid_to_world.numpy() if isinstance(grid_to_world, torch.Tensor) else grid_to_world,
                               dtype=np.float64)
    if g2w.shape != (3, 4) or not np.isfinite(g2w).all():
        raise ValueError(f"{what}: grid_to_world must be a finite 3x4 matrix, got shape {g2w.shape}")
    return (ctypes.c_double * 12)(*g2w.reshape(-1))


def _tsdf_min_weight(what, min_weight):
    """min_weight as the float32 the kernels compare with."""
    mw = float(torch.tensor(float(min_weight), dtype=F32))
    if not (_finite(mw) and mw > 0):
        raise ValueError(f"{what}: min_weight must be positive and finite, got {min_weight}")
    return mw


def _tsdf_surface(what, dev, n, cells, vertices, quad_count, quads):
    """The sequence of the four Surface Nets passes (csrc/tsdf_extract.h) over n lane indices, with the two prefix sums and
    the two readbacks between them.  The callables launch the passes of a volume: cells(count), vertices(cell_scan, V, verts,
    colours), quad_count(cell_scan, count), quads(cell_scan, quad_scan, V, Q, faces).  -> (verts float32 [V,3], colours uint8
    [V,3], faces int32 [2 Q,3]) in lane-index order; V = 0 and Q = 0 give empty tensors."""
    empty = (torch.empty((0, 3), dtype=F32, device=dev), torch.empty((0, 3), dtype=U8, device=dev),
             torch.empty((0, 3), dtype=I32, device=dev))
    count = torch.empty((n,), dtype=I32, device=dev)
    cells(count)
    cell_scan = torch.cumsum(count, 0, dtype=I32)
    V = int(cell_scan[-1])
    if V == 0:
        return empty
    verts = torch.empty((V, 3), dtype=F32, device=dev)
    colours = torch.empty((V, 3), dtype=U8, device=dev)
    vertices(cell_scan, V, verts, colours)
    quad_count(cell_scan, count)
    Q = int(count.sum(dtype=I64))
    if Q >= 1 << 30:
        raise _lib.ClmgsError(f"{what}: {Q} quads, 2^30 at the most: extract with a larger voxel or a smaller box")
    if Q == 0:
        return verts, colours, empty[2]
    quad_scan = torch.cumsum(count, 0, dtype=I32)
    del count
    faces = torch.empty((2 * Q, 3), dtype=I32, device=dev)
    quads(cell_scan, quad_scan, V, Q, faces)
    return verts, colours, faces


@torch.no_grad()
def tsdf_integrate(grid, depth, alpha, rgb, cams, near=0.01, depth_max=float("inf"), alpha_min=0.5, trunc=1.0, cull=True):
    """Fuses cameras into a TSDF volume in place (csrc/tsdf.hip; DESIGN.md section 3, "Mesh export"): grid float32
    [6,nz,ny,nx] (tsum, wsum, cr, cg, cb, cw); depth [B,H,W] (expected depth), alpha [B,H,W], rgb [B,3,H,W], float32 on the
    device; cams float64 [B,16] on the HOST (numpy or tensor): per camera the 3x4 matrix from grid coordinates (voxel
    (i,j,k) at (i+0.5, j+0.5, k+0.5)) to camera space, then fx, fy, cx, cy; trunc in camera-space units.  More than 16
    cameras go in launches of 16, in order: the result does not depend on how they are split.  `cull`: the brick-level
    frustum test (the same bits with and without).  Returns grid."""
    nx, ny, nz = _tsdf_grid(grid)
    cams, B, H, W = _tsdf_images("tsdf_integrate", grid.device, cams, depth, alpha, rgb)
    trunc32 = _tsdf_trunc("tsdf_integrate", trunc)
    inv_trunc = float(torch.tensor(1.0, dtype=F32) / torch.tensor(trunc32, dtype=F32))  # the float32 quotient
    L = _lib.lib()
    for b0, b1, rec in _tsdf_batches(cams, B):
        check(L.clmgs_tsdf_integrate(stream(), nx, ny, nz, dptr(grid, F32), b1 - b0, H, W, dptr(depth[b0:b1], F32),
                                     dptr(alpha[b0:b1], F32), dptr(rgb[b0:b1], F32), rec, float(near), float(depth_max),
                                     float(alpha_min), trunc32, inv_trunc, 1 if cull else 0))
    return grid


@torch.no_grad()
def tsdf_extract(grid, min_weight, grid_to_world):
    """Naive Surface Nets on a TSDF volume (csrc/tsdf.hip): a voxel is valid iff wsum >= min_weight and inside iff
    tsum < 0; every cell of eight valid voxels whose flags differ gets one vertex, every sign-changing grid edge whose four
    cells are active one quad (two triangles).  grid_to_world: float64 [3,4] on the host, from grid coordinates to the
    frame the vertices are wanted in.  -> (verts float32 [V,3], colours uint8 [V,3], faces int32 [F,3]) on the device,
    vertices in cell order, faces in (owner voxel, axis) order; V = F = 0 for a volume without a surface."""
    nx, ny, nz = _tsdf_grid(grid)
    rec = _tsdf_g2w("tsdf_extract", grid_to_world)
    mw = _tsdf_min_weight("tsdf_extract", min_weight)
    L, g, dims = _lib.lib(), dptr(grid, F32), (nx, ny, nz)
    return _tsdf_surface(
        "tsdf_extract", grid.device, nx * ny * nz,
        lambda count: check(L.clmgs_tsdf_cells(stream(), *dims, g, mw, dptr(count, I32))),
        lambda cell_scan, V, verts, colours: check(L.clmgs_tsdf_vertices(
            stream(), *dims, g, dptr(cell_scan, I32), V, rec, dptr(verts, F32), dptr(colours, U8))),
        lambda cell_scan, count: check(L.clmgs_tsdf_quad_count(stream(), *dims, g, mw, dptr(cell_scan, I32), dptr(count, I32))),
        lambda cell_scan, quad_scan, V, Q, faces: check(L.clmgs_tsdf_quads(
            stream(), *dims, g, mw, dptr(cell_scan, I32), dptr(quad_scan, I32), V, Q, dptr(faces, I32))))


# ------------------------------------------------------------------ mesh export, sparse volume
TSDF_BRICK = 8
TSDF_MAX_BRICK_GRID = 1 << 30


def tsdf_brick_grid(nx, ny, nz):
    """(nbx, nby, nbz) of a grid of nx x ny x nz voxels in bricks of 8 x 8 x 8; sides below 2 and a brick grid above 2^30 are
    refused by name."""
    nx, ny, nz = int(nx), int(ny), int(nz)
    if min(nx, ny, nz) < 2 or max(nx, ny, nz) >= 1 << 31:
        raise _lib.ClmgsError(f"tsdf: every side of the volume must be >= 2 and below 2^31, got {nx} x {ny} x {nz}")
    nb = tuple(-(-v // TSDF_BRICK) for v in (nx, ny, nz))
    if nb[0] * nb[1] * nb[2] > TSDF_MAX_BRICK_GRID:
        raise _lib.ClmgsError(f"tsdf: the brick grid {nb[0]} x {nb[1]} x {nb[2]} of {nx} x {ny} x {nz} voxels is above 2^30 bricks")
    return nb


@torch.no_grad()
def tsdf_mark(marks, shape, depth, alpha, cams_inv, near=0.01, depth_max=float("inf"), alpha_min=0.5, trunc=1.0, voxel_cam=1.0):
    """Marks, in place, the bricks of a sparse TSDF volume that the cameras can put a surface into (csrc/tsdf_sparse.hip;
    DESIGN.md section 3, "Sparse volume"): marks uint8 [nbz,nby,nbx] on the device for the grid shape = (nx, ny, nz);
    depth, alpha float32 [B,H,W] on the device; cams_inv float64 [B,16] on the HOST: per camera the 3x4 matrix from
    camera space to grid coordinates (the inverse of tsdf_integrate's), then fx, fy, cx, cy; trunc and voxel_cam (the
    length of a voxel) in camera units.  The marked set is a superset of every voxel within 1 voxel of a voxel some
    camera observes with -trunc <= sdf < 0, and a pure function of the set of cameras: more than 16 go in launches of 16,
    and neither their order nor their split changes a byte.  Returns marks."""
    nx, ny, nz = (int(v) for v in shape)
    nbx, nby, nbz = tsdf_brick_grid(nx, ny, nz)
    if not (isinstance(marks, torch.Tensor) and marks.is_cuda and marks.is_contiguous() and marks.dtype == U8
            and tuple(marks.shape) == (nbz, nby, nbx)):
        raise _lib.ClmgsError(f"tsdf_mark: marks must be a contiguous uint8 {(nbz, nby, nbx)} device tensor, got "
                              f"{getattr(marks, 'dtype', type(marks))} {tuple(getattr(marks, 'shape', ()))}")
    cams, B, H, W = _tsdf_images("tsdf_mark", marks.device, cams_inv, depth, alpha)
    trunc32 = _tsdf_trunc("tsdf_mark", trunc)
    if not (_finite(float(voxel_cam)) and voxel_cam > 0 and trunc32 / float(voxel_cam) <= 4096):
        raise ValueError(f"tsdf_mark: voxel_cam must be positive and finite and trunc at most 4096 voxels, got {voxel_cam}, "
                         f"trunc {trunc}")
    L = _lib.lib()
    for b0, b1, rec in _tsdf_batches(cams, B):
        check(L.clmgs_tsdf_mark(stream(), nx, ny, nz, dptr(marks), b1 - b0, H, W, dptr(depth[b0:b1], F32),
                                dptr(alpha[b0:b1], F32), rec, float(near), float(depth_max), float(alpha_min), trunc32,
                                float(voxel_cam)))
    return marks


def _tsdf_sparse(what, shape, bricks, table, pool):
    """The checks of a sparse volume's three tensors against the grid shape -> (nx, ny, nz, S)."""
    nx, ny, nz = (int(v) for v in shape)
    nbx, nby, nbz = tsdf_brick_grid(nx, ny, nz)
    ok = lambda t, dt: isinstance(t, torch.Tensor) and t.is_cuda and t.is_contiguous() and t.dtype == dt
    if not (ok(pool, F32) and pool.dim() == 5 and tuple(pool.shape[1:]) == (6, 8, 8, 8) and pool.shape[0] >= 1):
        raise _lib.ClmgsError(f"{what}: the pool is a contiguous float32 [S, 6, 8, 8, 8] device tensor with S >= 1, got "
                              f"{getattr(pool, 'dtype', type(pool))} {tuple(getattr(pool, 'shape', ()))}")
    S = int(pool.shape[0])
    if S * 512 >= 1 << 31:
        raise _lib.ClmgsError(f"{what}: {S} bricks, S * 512 must stay below 2^31")
    if not (ok(bricks, I32) and tuple(bricks.shape) == (S,) and bricks.device == pool.device):
        raise _lib.ClmgsError(f"{what}: bricks must be a contiguous int32 [{S}] tensor on {pool.device}, got "
                              f"{getattr(bricks, 'dtype', type(bricks))} {tuple(getattr(bricks, 'shape', ()))}")
    if table is not None:
        if not (ok(table, I32) and tuple(table.shape) == (nbz, nby, nbx) and table.device == pool.device):
            raise _lib.ClmgsError(f"{what}: table must be a contiguous int32 {(nbz, nby, nbx)} tensor on {pool.device}, got "
                                  f"{getattr(table, 'dtype', type(table))} {tuple(getattr(table, 'shape', ()))}")
        slots = table.reshape(-1)[bricks.long().clamp_(0, table.numel() - 1)]
        if int(table.max()) != S - 1 or int((table >= 0).sum()) != S or not torch.equal(
                slots, torch.arange(S, dtype=I32, device=pool.device)):
            raise _lib.ClmgsError(f"{what}: the table does not belong to a pool of {S} bricks (its slots must be 0 .. {S - 1}, "
                                  "each once, at the bricks the list names)")
    else:
        lo, hi = (int(v) for v in torch.aminmax(bricks))
        if lo < 0 or hi >= nbx * nby * nbz or (S > 1 and not bool((bricks[1:] > bricks[:-1]).all())):
            raise _lib.ClmgsError(f"{what}: bricks must be ascending indices into the {nbx} x {nby} x {nbz} brick grid")
    return nx, ny, nz, S


@torch.no_grad()
def tsdf_sparse_integrate(pool, bricks, shape, depth, alpha, rgb, cams, near=0.01, depth_max=float("inf"), alpha_min=0.5,
                          trunc=1.0, cull=True):
    """tsdf_integrate on a brick-allocated volume (csrc/tsdf_sparse.hip): pool float32 [S,6,8,8,8], bricks int32 [S] (the
    ascending linear brick indices of the slots) for the grid shape = (nx, ny, nz); the other arguments as tsdf_integrate.
    A stored voxel gets exactly the sums the dense volume gives it.  Returns pool."""
    nx, ny, nz, S = _tsdf_sparse("tsdf_sparse_integrate", shape, bricks, None, pool)
    cams, B, H, W = _tsdf_images("tsdf_sparse_integrate", pool.device, cams, depth, alpha, rgb)
    trunc32 = _tsdf_trunc("tsdf_sparse_integrate", trunc)
    inv_trunc = float(torch.tensor(1.0, dtype=F32) / torch.tensor(trunc32, dtype=F32))  # the float32 quotient
    L = _lib.lib()
    for b0, b1, rec in _tsdf_batches(cams, B):
        check(L.clmgs_tsdf_sparse_integrate(stream(), nx, ny, nz, S, dptr(bricks, I32), dptr(pool, F32), b1 - b0, H, W,
                                            dptr(depth[b0:b1], F32), dptr(alpha[b0:b1], F32), dptr(rgb[b0:b1], F32), rec,
                                            float(near), float(depth_max), float(alpha_min), trunc32, inv_trunc,
                                            1 if cull else 0))
    return pool


@torch.no_grad()
def tsdf_sparse_extract(pool, bricks, table, shape, min_weight, grid_to_world, want_keys=False):
    """tsdf_extract on a brick-allocated volume (csrc/tsdf_sparse.hip): the four passes over the S * 512 stored voxels, then
    the vertices sorted by the dense linear index of their cell and the quads by (owner voxel, axis), on the device
    (torch.sort), so that the output is in tsdf_extract's order.  -> (verts, colours, faces), with want_keys also the
    sorted int64 keys of the vertices (cell index) and the quads (3 * voxel index + axis)."""
    nx, ny, nz, S = _tsdf_sparse("tsdf_sparse_extract", shape, bricks, table, pool)
    rec = _tsdf_g2w("tsdf_sparse_extract", grid_to_world)
    mw = _tsdf_min_weight("tsdf_sparse_extract", min_weight)
    L, dev = _lib.lib(), pool.device

    def run(ps, count=None, cell_scan=None, quad_scan=None, V=0, Q=0, verts=None, colours=None, vkeys=None, faces=None,
            qkeys=None):
        o = lambda t, dt=None: dptr(t, dt, allow_none=True)
        check(L.clmgs_tsdf_sparse_extract(stream(), ps, nx, ny, nz, S, dptr(bricks, I32), dptr(table, I32), dptr(pool, F32), mw,
                                          o(count, I32), o(cell_scan, I32), o(quad_scan, I32), V, Q, rec, o(verts, F32),
                                          o(colours, U8), o(vkeys, I64), o(faces, I32), o(qkeys, I64)))

    keys = {}  # of the vertices and the quads, as the passes wrote them

    def vertices(cell_scan, V, verts, colours):
        keys["v"] = torch.empty((V,), dtype=I64, device=dev)
        run(1, cell_scan=cell_scan, V=V, verts=verts, colours=colours, vkeys=keys["v"])

    def quads(cell_scan, quad_scan, V, Q, faces):
        keys["q"] = torch.empty((Q,), dtype=I64, device=dev)
        run(3, cell_scan=cell_scan, quad_scan=quad_scan, V=V, Q=Q, faces=faces, qkeys=keys["q"])

    verts, colours, faces = _tsdf_surface("tsdf_sparse_extract", dev, S * 512, lambda count: run(0, count=count), vertices,
                                          lambda cell_scan, count: run(2, count=count, cell_scan=cell_scan), quads)
    V, Q = verts.shape[0], faces.shape[0] // 2
    vkeys = qkeys = torch.empty((0,), dtype=I64, device=dev)
    if V:
        vkeys, order = torch.sort(keys["v"])
        verts, colours = verts[order], colours[order]
    if Q:
        new_id = torch.empty((V,), dtype=I32, device=dev)  # the inverse permutation: the rank of every vertex in the dense order
        new_id[order] = torch.arange(V, dtype=I32, device=dev)
        qkeys, qorder = torch.sort(keys["q"])
        faces = new_id[faces.long()].reshape(Q, 6)[qorder].reshape(2 * Q, 3).contiguous()
    return (verts, colours, faces, vkeys, qkeys) if want_keys else (verts, colours, faces)


# ------------------------------------------------------------------ mesh cleanup
MESH_MAX_ROUNDS = 64


def _mesh_faces(faces, V, what):
    """faces: a contiguous int32 [F,3] device tensor whose indices lie in [0, V) (checked on the device, before any
    launch) -> F; anything else is refused by name."""
    if not (isinstance(faces, torch.Tensor) and faces.is_cuda):
        raise _lib.ClmgsError(f"{what}: faces must be a tensor on the device (no CPU fallback in clm_gs_amd), got "
                              f"{getattr(faces, 'device', type(faces))}")
    if faces.dtype != I32 or faces.dim() != 2 or faces.shape[1] != 3:
        raise _lib.ClmgsError(f"{what}: faces must be int32 [F,3], got {faces.dtype} {tuple(faces.shape)}")
    if not faces.is_contiguous():
        raise _lib.ClmgsError(f"{what}: faces must be contiguous")
    if isinstance(V, bool) or int(V) != V:
        raise ValueError(f"{what}: V must be an integer, got {V!r}")
    if V < 0 or V >= 1 << 31:
        raise ValueError(f"{what}: V must be in [0, 2^31), got {V}")
    F = int(faces.shape[0])
    if F >= 1 << 31:
        raise _lib.ClmgsError(f"{what}: F must be below 2^31, got {F}")
    if F:
        lo, hi = (int(v) for v in torch.aminmax(faces))
        if lo < 0 or hi >= V:
            raise _lib.ClmgsError(f"{what}: a face index lies outside [0, {int(V)}): the indices span [{lo}, {hi}]")
    return F


@torch.no_grad()
def mesh_components(faces, V):
    """Connected components of a triangle list (csrc/mesh.hip; DESIGN.md section 3, "Mesh cleanup"): faces int32 [F,3] on
    the device over V vertices; two vertices are connected when a face names both -> (labels int32 [V], rounds):
    labels[v] = the smallest vertex index of v's component (v for a vertex no face names), rounds = how many hook and
    shortcut rounds ran, the last of which changed nothing.  More than MESH_MAX_ROUNDS rounds raise ClmgsError.  F == 0
    or V == 0 launches nothing."""
    F = _mesh_faces(faces, V, "mesh_components")
    V = int(V)
    parent = torch.arange(V, dtype=I32, device=faces.device)
    if F == 0 or V == 0:
        return parent, 0
    L = _lib.lib()
    flags = torch.zeros((MESH_MAX_ROUNDS,), dtype=I32, device=faces.device)
    for r in range(MESH_MAX_ROUNDS):
        check(L.clmgs_mesh_hook(stream(), V, F, dptr(faces, I32), dptr(parent, I32), dptr(flags[r:], I32)))
        check(L.clmgs_mesh_shortcut(stream(), V, dptr(parent, I32), dptr(flags[r:], I32)))
        if int(flags[r]) == 0:
            return parent, r + 1
    raise _lib.ClmgsError(f"mesh_components: no fixed point after {MESH_MAX_ROUNDS} rounds (V {V}, F {F})")


@torch.no_grad()
def mesh_component_faces(faces, labels):
    """The face count of every component (csrc/mesh.hip): labels int32 [V] as mesh_components returns it -> int32 [V],
    count[l] = the number of faces whose first vertex has label l: zero except at labels.  An integer sum: the same bits
    whatever the order."""
    if not (isinstance(labels, torch.Tensor) and labels.is_cuda and labels.is_contiguous() and labels.dtype == I32
            and labels.dim() == 1):
        raise _lib.ClmgsError("mesh_component_faces: labels must be a contiguous int32 [V] device tensor, got "
                              f"{getattr(labels, 'dtype', type(labels))} {tuple(getattr(labels, 'shape', ()))}")
    V = int(labels.shape[0])
    F = _mesh_faces(faces, V, "mesh_component_faces")
    if faces.device != labels.device:
        raise _lib.ClmgsError(f"mesh_component_faces: faces are on {faces.device}, labels on {labels.device}")
    count = torch.zeros((V,), dtype=I32, device=labels.device)
    if F == 0 or V == 0:
        return count
    check(_lib.lib().clmgs_mesh_component_faces(stream(), V, F, dptr(faces, I32), dptr(labels, I32), dptr(count, I32)))
    return count


# ------------------------------------------------------------------ mesh decimation
MESH_DECIMATE_NONFINITE, MESH_DECIMATE_RANGE = 1, 2  # the bits of mesh_decimate_keys' flag


def _mesh_cell(cell, what):
    if isinstance(cell, bool) or not isinstance(cell, (int, float)) or not (0 < cell < float("inf")):
        raise ValueError(f"{what}: cell must be a positive finite number, got {cell!r}")
    return float(cell)


def _mesh_dev(t, dtype, shape, what, name):
    """t: a contiguous device tensor of that dtype and shape (None = any size), or ClmgsError by name."""
    if not (isinstance(t, torch.Tensor) and t.is_cuda):
        raise _lib.ClmgsError(f"{what}: {name} must be a tensor on the device (no CPU fallback in clm_gs_amd), got "
                              f"{getattr(t, 'device', type(t))}")
    if t.dtype != dtype or t.dim() != len(shape) or any(s is not None and int(n) != s for n, s in zip(t.shape, shape)):
        want = "[" + ",".join("N" if s is None else str(s) for s in shape) + "]"
        raise _lib.ClmgsError(f"{what}: {name} must be {str(dtype).replace('torch.', '')} {want}, got {t.dtype} {tuple(t.shape)}")
    if not t.is_contiguous():
        raise _lib.ClmgsError(f"{what}: {name} must be contiguous")


@torch.no_grad()
def mesh_decimate_keys(verts, faces, cell):
    """The key pass of the decimation (csrc/mesh_decimate.hip; DESIGN.md section 3, "Mesh decimation"): verts float32 [V,3]
    and faces int32 [F,3] on the device, cell > 0 -> (keys int64 [V], flag int32 [1]), both on the device: the key of the
    cell of every vertex a face names, -1 for the others; flag holds MESH_DECIMATE_NONFINITE and / or MESH_DECIMATE_RANGE
    when such a vertex has a non-finite coordinate or a cell index outside [-2^20, 2^20).  F == 0 or V == 0 launches
    nothing."""
    what = "mesh_decimate_keys"
    cell = _mesh_cell(cell, what)
    _mesh_dev(verts, F32, (None, 3), what, "verts")
    V = int(verts.shape[0])
    F = _mesh_faces(faces, V, what)
    keys = torch.full((V,), -1, dtype=I64, device=verts.device)
    flag = torch.zeros((1,), dtype=I32, device=verts.device)
    if F == 0 or V == 0:
        return keys, flag
    L = _lib.lib()
    mark = torch.zeros((V,), dtype=U8, device=verts.device)
    check(L.clmgs_mesh_decimate_mark(stream(), V, F, dptr(faces, I32), dptr(mark, U8)))
    check(L.clmgs_mesh_decimate_keys(stream(), V, dptr(verts, F32), dptr(mark, U8), cell, dptr(keys, I64), dptr(flag, I32)))
    return keys, flag


@torch.no_grad()
def mesh_decimate_faces(faces, cluster, C):
    """The face pass (csrc/mesh_decimate.hip): faces int32 [F,3], cluster int32 [V] (the new index of every vertex a face
    names), C clusters -> (rotated int32 [F,3], collapsed uint8 [F], inc int64 [3F]): the corners' clusters with the smallest
    first and the orientation kept, 1 where two corners share a cluster, and per face one (cluster << 32 | face) for every
    distinct cluster among its corners, INT64_MAX in the unused slots."""
    what = "mesh_decimate_faces"
    _mesh_dev(cluster, I32, (None,), what, "cluster")
    V = int(cluster.shape[0])
    F = _mesh_faces(faces, V, what)
    if isinstance(C, bool) or int(C) != C or not 1 <= C <= V:
        raise ValueError(f"{what}: C must be an integer in [1, {V}], got {C!r}")
    C = int(C)
    dev = faces.device
    rotated = torch.empty((F, 3), dtype=I32, device=dev)
    collapsed = torch.empty((F,), dtype=U8, device=dev)
    inc = torch.empty((3 * F,), dtype=I64, device=dev)
    if F:
        check(_lib.lib().clmgs_mesh_decimate_faces(stream(), V, F, C, dptr(faces, I32), dptr(cluster, I32),
                                                   dptr(rotated, I32), dptr(collapsed, U8), dptr(inc, I64)))
    return rotated, collapsed, inc


@torch.no_grad()
def mesh_decimate_place(verts, colours, faces, cluster_keys, vert_order, vert_start, inc, inc_start, lane_order, cell):
    """The placement kernel (csrc/mesh_decimate.hip), one lane per cluster: cluster_keys int64 [C] ascending, vert_order
    int32 [M] the participating vertices by cluster then index, vert_start int64 [C+1], inc int64 [I] the incidences of
    mesh_decimate_faces sorted ascending, inc_start int64 [C+1] their segments, lane_order int32 [C] the permutation of the
    clusters in which the lanes take them (it changes the speed, not one bit of the output) -> (verts float32 [C,3], colours uint8 [C,3], code uint8 [C]); code 0 =
    the quadric's minimiser, 1 = the mean (degenerate quadric), 2 = the mean (minimiser outside)."""
    what = "mesh_decimate_place"
    cell = _mesh_cell(cell, what)
    _mesh_dev(verts, F32, (None, 3), what, "verts")
    V = int(verts.shape[0])
    _mesh_dev(colours, U8, (V, 3), what, "colours")
    F = _mesh_faces(faces, V, what)
    _mesh_dev(cluster_keys, I64, (None,), what, "cluster_keys")
    C = int(cluster_keys.shape[0])
    _mesh_dev(vert_order, I32, (None,), what, "vert_order")
    _mesh_dev(vert_start, I64, (C + 1,), what, "vert_start")
    _mesh_dev(inc, I64, (None,), what, "inc")
    _mesh_dev(inc_start, I64, (C + 1,), what, "inc_start")
    _mesh_dev(lane_order, I32, (C,), what, "lane_order")
    dev = verts.device
    out_verts = torch.empty((C, 3), dtype=F32, device=dev)
    out_colours = torch.empty((C, 3), dtype=U8, device=dev)
    code = torch.empty((C,), dtype=U8, device=dev)
    if C:
        check(_lib.lib().clmgs_mesh_decimate_place(
            stream(), V, F, C, dptr(verts, F32), dptr(colours, U8), dptr(faces, I32), dptr(cluster_keys, I64),
            dptr(vert_order, I32), dptr(vert_start, I64), int(vert_order.shape[0]), dptr(inc, I64), dptr(inc_start, I64),
            int(inc.shape[0]), dptr(lane_order, I32), cell, dptr(out_verts, F32), dptr(out_colours, U8), dptr(code, U8)))
    return out_verts, out_colours, code


# ------------------------------------------------------------------ mesh smoothing and vertex normals
@torch.no_grad()
def mesh_incidence(faces, V):
    """The vertex -> face incidence lists of a mesh ("Mesh smoothing and normals"): faces int32 [F,3]
    on the device with indices in [0, V) -> (order int64 [3F], start int64 [V+1]).  order holds the corner slots
    e = 3 f + k sorted by the vertex faces[f,k], ascending e within a vertex (a stable sort: faces ascending, then corners);
    the segment of vertex v is order[start[v]:start[v+1]].  A face that names a vertex twice is in its segment twice.  The
    sort and the searchsorted are torch."""
    F = _mesh_faces(faces, V, "mesh_incidence")
    V, dev = int(V), faces.device
    skeys, order = torch.sort(faces.reshape(-1), stable=True)
    start = torch.full((V + 1,), 3 * F, dtype=I64, device=dev)  # (every index is below V: the last boundary is 3F)
    if F and V:
        start[:V] = torch.searchsorted(skeys, torch.arange(V, dtype=I32, device=dev))
    return order.contiguous(), start


def _mesh_lists(verts, faces, order, start, what):
    """The checks mesh_smooth_step and mesh_vertex_normals share, all before any launch.  -> (V, F)."""
    _mesh_dev(verts, F32, (None, 3), what, "verts")
    V = int(verts.shape[0])
    F = _mesh_faces(faces, V, what)
    _mesh_dev(order, I64, (3 * F,), what, "order")
    _mesh_dev(start, I64, (V + 1,), what, "start")
    if not (faces.device == order.device == start.device == verts.device):
        raise _lib.ClmgsError(f"{what}: verts are on {verts.device}, faces on {faces.device}, order on {order.device}, "
                              f"start on {start.device}")
    return V, F


@torch.no_grad()
def mesh_smooth_step(verts, faces, order, start, factor):
    """One umbrella step (csrc/mesh_smooth.hip, one lane per vertex): verts float32 [V,3], faces int32 [F,3] and the lists
    of mesh_incidence on the device, factor a finite number -> a NEW float32 [V,3]: every vertex moved by `factor` towards
    the mean of its neighbours over its incidences (each neighbour weighted by the number of faces sharing the edge;
    float64 sums in list order without contraction), a vertex no face names with its own bits.  F == 0 or V == 0 launches
    nothing and returns a copy."""
    what = "mesh_smooth_step"
    if isinstance(factor, bool) or not isinstance(factor, (int, float)) or not (-float("inf") < factor < float("inf")):
        raise ValueError(f"{what}: factor must be a finite number, got {factor!r}")
    V, F = _mesh_lists(verts, faces, order, start, what)
    if F == 0 or V == 0:
        return verts.clone()
    out = torch.empty_like(verts)
    check(_lib.lib().clmgs_mesh_smooth_step(stream(), V, F, dptr(verts, F32), dptr(faces, I32), dptr(order, I64),
                                            dptr(start, I64), float(factor), dptr(out, F32)))
    return out


@torch.no_grad()
def mesh_vertex_normals(verts, faces, order, start):
    """Area-weighted vertex normals (csrc/mesh_smooth.hip, one lane per vertex): the sum over a vertex's incidences of
    (p1 - p0) x (p2 - p0) from each face's corners in stored order, normalised -> float32 [V,3] on the device; (0, 0, 0) for
    a vertex no face names or whose sum has no direction.  F == 0 or V == 0 launches nothing and returns zeros."""
    what = "mesh_vertex_normals"
    V, F = _mesh_lists(verts, faces, order, start, what)
    if F == 0 or V == 0:
        return torch.zeros((V, 3), dtype=F32, device=verts.device)
    out = torch.empty_like(verts)
    check(_lib.lib().clmgs_mesh_vertex_normals(stream(), V, F, dptr(verts, F32), dptr(faces, I32), dptr(order, I64),
                                               dptr(start, I64), dptr(out, F32)))
    return out


# ------------------------------------------------------------------ mesh evaluation
MESH_MAX_SAMPLES = 1 << 28          # the default limit of mesh_sample; the entry itself takes S < 2^31
MESH_GRID_MAX_CELLS = 1 << 27
MESH_GRID_MAX_AXIS = 1 << 20
MESH_GRID_PAIR_BYTES = 32           # per (cell, primitive) pair: the two lists, their sorted forms and the sort's indices


def _mesh_number(x, what, name, allow_inf=False):
    """x: a positive finite number (or +inf where allowed) -> float, or ValueError by name."""
    if isinstance(x, bool) or not isinstance(x, (int, float)) or not (0 < x and (x < float("inf") or (allow_inf and x == float("inf")))):
        raise ValueError(f"{what}: {name} must be a positive {'number' if allow_inf else 'finite number'}, got {x!r}")
    return float(x)


def _mesh_sample_count(verts, faces, V, F, spacing):
    area = torch.empty((F,), dtype=torch.float64, device=verts.device)
    count = torch.empty((F,), dtype=I64, device=verts.device)
    if F and V:
        check(_lib.lib().clmgs_mesh_sample_count(stream(), V, F, dptr(verts, F32), dptr(faces, I32), spacing,
                                                 dptr(area, torch.float64), dptr(count, I64)))
    return area, count


@torch.no_grad()
def mesh_sample(verts, faces, spacing, max_samples=MESH_MAX_SAMPLES, name="max_samples"):
    """Area-weighted surface samples (csrc/mesh_distance.hip; DESIGN.md section 3, "Mesh evaluation"): verts float32 [V,3]
    and faces int32 [F,3] on the device, spacing > 0 -> (points float32 [S,3], face int32 [S], weight float64 [S], area
    float64 [F]), all on the device.  Face f gets n_f = ceil(area_f / spacing^2) samples of weight area_f / n_f each, at
    the first n_f points of the R2 sequence folded into the triangle; a face whose area is zero or not finite gets none.
    A total above max_samples is refused (ValueError, by `name`, with the spacing that fits) before the samples are
    allocated."""
    what = "mesh_sample"
    spacing = _mesh_number(spacing, what, "spacing")
    if isinstance(max_samples, bool) or not isinstance(max_samples, int) or not 1 <= max_samples < 1 << 31:
        raise ValueError(f"{what}: {name} must be an integer in [1, 2^31), got {max_samples!r}")
    _mesh_dev(verts, F32, (None, 3), what, "verts")
    V = int(verts.shape[0])
    F = _mesh_faces(faces, V, what)
    if faces.device != verts.device:
        raise _lib.ClmgsError(f"{what}: verts are on {verts.device}, faces on {faces.device}")
    dev = verts.device
    area, count = _mesh_sample_count(verts, faces, V, F, spacing)
    S = int(count.sum()) if F else 0
    if S > max_samples:
        ok = (area > 0) & torch.isfinite(area)
        total, n_ok = float(area[ok].sum()), int(ok.sum())
        fits = (f"a spacing of {1.001 * (total / (max_samples - n_ok)) ** 0.5:g} fits" if max_samples > n_ok
                else f"no spacing fits: {n_ok} faces have an area")
        raise ValueError(f"{what}: spacing {spacing:g} gives {S} samples, above {name} {max_samples}; {fits}")
    points = torch.empty((S, 3), dtype=F32, device=dev)
    weight = torch.empty((S,), dtype=torch.float64, device=dev)
    if S == 0:
        return points, torch.empty((0,), dtype=I32, device=dev), weight, area
    offsets = torch.zeros((F + 1,), dtype=I64, device=dev)
    torch.cumsum(count, 0, out=offsets[1:])
    face = torch.repeat_interleave(torch.arange(F, dtype=I32, device=dev), count, output_size=S).contiguous()
    check(_lib.lib().clmgs_mesh_sample_emit(stream(), V, F, dptr(verts, F32), dptr(faces, I32), dptr(area, torch.float64),
                                            dptr(offsets, I64), dptr(face, I32), S, dptr(points, F32),
                                            dptr(weight, torch.float64)))
    return points, face, weight, area


class MeshDistanceGrid:
    """What mesh_distance_grid builds and mesh_distance reads: the primitives (verts, faces or None for points), the grid
    (origin, h, dims) and the lists (cell_start int64 [cells + 1], pair_prim int32 [pairs]); primitives = how many of the
    n faces / points are primitives, degenerate = the others."""
    __slots__ = ("verts", "faces", "n", "origin", "h", "dims", "cell_start", "pair_prim", "pairs", "primitives", "degenerate")


def _mesh_grid_default_cell(lo, hi, used, corners):
    """A speed choice, no part of the contract: the median longest bounding-box side of the triangles (measured against
    twice that in DESIGN.md section 3, "Mesh evaluation"); for points the spacing that puts about four of them into an
    occupied cell of a surface."""
    extent = [b - a for a, b in zip(lo, hi)]
    if corners is not None:
        side = (corners.amax(1) - corners.amin(1)).amax(1)
        h = float(side.median())
    else:
        ex, ey, ez = extent
        surface = ex * ey + ey * ez + ex * ez
        n = int(used.shape[0])
        h = (4.0 * surface / n) ** 0.5 if surface > 0 else 4.0 * max(extent) / n
    if not (h > 0 and h < float("inf")):
        h = max(extent) if max(extent) > 0 else 1.0
    return max(h, max(extent) * 2.0 ** -19)  # (at most 2^19 cells along an axis)


@torch.no_grad()
def mesh_distance_grid(verts, faces=None, cell=None, grid_gb=4.0, name="cell"):
    """The primitive grid of mesh_distance (csrc/mesh_distance.hip; DESIGN.md section 3, "Mesh evaluation"): verts float32
    [V,3] on the device and faces int32 [F,3] (the primitives are the triangles) or None (the points) -> MeshDistanceGrid.
    A uniform grid of cell size h over the float64 bounding box of the primitives; a triangle is listed in every cell of
    the index range of its bounding box, a point in its own.  A face whose area is zero or not finite and a point with a
    non-finite coordinate are not primitives.  Without `cell` h is chosen here and raised until the grid has at most 2^27
    cells (2^20 per axis) and its pairs fit grid_gb; a given cell that breaks a limit is refused (ValueError, by `name`,
    with the size that fits).  mesh_distance gives the same result for any h."""
    what = "mesh_distance_grid"
    if cell is not None:
        cell = _mesh_number(cell, what, name)
    grid_gb = _mesh_number(grid_gb, what, "grid_gb")
    _mesh_dev(verts, F32, (None, 3), what, "verts")
    V = int(verts.shape[0])
    N = V if faces is None else _mesh_faces(faces, V, what)
    if faces is not None and faces.device != verts.device:
        raise _lib.ClmgsError(f"{what}: verts are on {verts.device}, faces on {faces.device}")
    dev = verts.device
    g = MeshDistanceGrid()
    g.verts, g.faces, g.n = verts, faces, N
    corners = None
    if faces is not None:
        area, _ = _mesh_sample_count(verts, faces, V, N, 1.0)
        valid = (area > 0) & torch.isfinite(area)
        corners = verts[faces[valid].long().reshape(-1)].double().reshape(-1, 3, 3)
        used = corners.reshape(-1, 3)
    else:
        valid = torch.isfinite(verts).all(dim=1)
        used = verts[valid].double()
    g.primitives = int(valid.sum()) if N else 0
    g.degenerate = N - g.primitives
    if g.primitives == 0:
        g.origin, g.h, g.dims, g.pairs = (0.0, 0.0, 0.0), cell or 1.0, (1, 1, 1), 0
        g.cell_start = torch.zeros((2,), dtype=I64, device=dev)
        g.pair_prim = torch.empty((0,), dtype=I32, device=dev)
        return g
    lo, hi = [float(v) for v in used.amin(0)], [float(v) for v in used.amax(0)]
    L = _lib.lib()
    count = torch.empty((N,), dtype=I64, device=dev)
    fptr = dptr(faces, I32, allow_none=True)

    def fit(h):
        dims = tuple(int((b - a) / h // 1) + 1 for a, b in zip(lo, hi))
        if max(dims) > MESH_GRID_MAX_AXIS or dims[0] * dims[1] * dims[2] > MESH_GRID_MAX_CELLS:
            return dims, None
        check(L.clmgs_mesh_bin_count(stream(), V, N, dptr(verts, F32), fptr, lo[0], lo[1], lo[2], h, *dims, dptr(count, I64)))
        pairs = int(count.sum())
        return dims, pairs if pairs * MESH_GRID_PAIR_BYTES <= grid_gb * 1e9 else None

    h0 = cell if cell is not None else _mesh_grid_default_cell(lo, hi, used, corners)
    h = h0
    for _ in range(400):
        dims, pairs = fit(h)
        if pairs is not None:
            break
        if dims == (1, 1, 1):  # (one cell lists every primitive once: nothing coarser exists)
            raise ValueError(f"{what}: no cell size fits grid_gb {grid_gb:g}: {g.primitives} primitives need "
                             f"{g.primitives * MESH_GRID_PAIR_BYTES} B")
        h *= 1.25
    if pairs is None:
        raise ValueError(f"{what}: no cell size up to {h:g} fits the limits of the grid")
    if cell is not None and h != h0:
        raise ValueError(f"{what}: {name} {cell:g} breaks the limits of the grid (2^27 cells, 2^20 along an axis, pairs "
                         f"of {MESH_GRID_PAIR_BYTES} B within grid_gb {grid_gb:g}); {h:g} fits")
    g.origin, g.h, g.dims, g.pairs = tuple(lo), h, dims, pairs
    offsets = torch.zeros((N + 1,), dtype=I64, device=dev)
    torch.cumsum(count, 0, out=offsets[1:])
    cells = torch.empty((pairs,), dtype=I64, device=dev)
    prims = torch.empty((pairs,), dtype=I32, device=dev)
    check(L.clmgs_mesh_bin_emit(stream(), V, N, dptr(verts, F32), fptr, lo[0], lo[1], lo[2], h, *dims, dptr(offsets, I64),
                                pairs, dptr(cells, I64), dptr(prims, I32)))
    cells, order = torch.sort(cells, stable=True)
    g.pair_prim = prims[order].contiguous()
    n_cells = dims[0] * dims[1] * dims[2]
    g.cell_start = torch.searchsorted(cells, torch.arange(n_cells + 1, dtype=I64, device=dev)).contiguous()
    return g


@torch.no_grad()
def mesh_distance(points, grid, max_distance=float("inf"), with_evaluated=False):
    """The exact distance from every point to its nearest primitive (csrc/mesh_distance.hip, one lane per query): points
    float32 [P,3] on the device, grid from mesh_distance_grid -> (dist float32 [P], prim int32 [P]) on the device: the
    minimum over ALL primitives of the float64 distance of csrc/mesh_distance_math.h, rounded to float32, and the index of
    the primitive, the smallest on ties; (+inf, -1) where that distance exceeds max_distance, where the grid has no
    primitive, and for a point with a non-finite coordinate.  The result does not depend on the grid's cell size.  The
    queries are sorted by cell for the launch and the results scattered back (torch).  with_evaluated: a third item,
    int32 [P], the number of primitives each lane evaluated."""
    what = "mesh_distance"
    if not isinstance(grid, MeshDistanceGrid):
        raise ValueError(f"{what}: grid must come from mesh_distance_grid, got {type(grid).__name__}")
    max_distance = _mesh_number(max_distance, what, "max_distance", allow_inf=True)
    _mesh_dev(points, F32, (None, 3), what, "points")
    if points.device != grid.verts.device:
        raise _lib.ClmgsError(f"{what}: points are on {points.device}, the grid on {grid.verts.device}")
    P, dev = int(points.shape[0]), points.device
    dist = torch.full((P,), float("inf"), dtype=F32, device=dev)
    prim = torch.full((P,), -1, dtype=I32, device=dev)
    evaluated = torch.zeros((P,), dtype=I32, device=dev)
    if P and grid.pairs:
        q = torch.nan_to_num(points.double(), nan=0.0, posinf=0.0, neginf=0.0)
        key = torch.zeros((P,), dtype=I64, device=dev)
        for axis in (2, 1, 0):
            i = torch.floor((q[:, axis] - grid.origin[axis]) / grid.h).clamp_(0, grid.dims[axis] - 1).long()
            key = key * grid.dims[axis] + i
        order = torch.sort(key).indices
        sorted_points = points[order].contiguous()
        d, p, e = torch.empty_like(dist), torch.empty_like(prim), torch.empty_like(evaluated)
        check(_lib.lib().clmgs_mesh_distance(
            stream(), P, dptr(sorted_points, F32), int(grid.verts.shape[0]), grid.n, dptr(grid.verts, F32),
            dptr(grid.faces, I32, allow_none=True), grid.origin[0], grid.origin[1], grid.origin[2], grid.h, *grid.dims,
            dptr(grid.cell_start, I64), dptr(grid.pair_prim, I32), grid.pairs, max_distance, dptr(d, F32), dptr(p, I32),
            dptr(e, I32) if with_evaluated else None))
        dist[order], prim[order] = d, p
        if with_evaluated:
            evaluated[order] = e
    return (dist, prim, evaluated) if with_evaluated else (dist, prim)


# ------------------------------------------------------------ MCMC densification
def _f32_dev(t, shape, what):
    assert t.is_cuda and t.dtype == F32 and t.is_contiguous() and tuple(t.shape) == tuple(shape), \
        f"{what}: contiguous float32 device tensor of shape {tuple(shape)} expected, got {t.dtype} {tuple(t.shape)}"


@torch.no_grad()
def mcmc_relocation(opacities, scales, ratios):
    """gsplat's compute_relocation: ACTIVATED opacities [n] / [n,1] and scales [n,3] of Gaussians that will exist
    ratios[i] times (int32 [n], clamped to 1..51) -> (new_opacities, new_scales) in the shapes given, with
    o' = 1 - (1 - o)^(1/r) and the scales multiplied by o / D(o', r) (csrc/mcmc.hip; DESIGN.md section 3, "MCMC")."""
    n = scales.shape[0]
    _f32_dev(scales, (n, 3), "scales")
    assert opacities.numel() == n
    _f32_dev(opacities, opacities.shape, "opacities")
    assert ratios.is_cuda and ratios.dtype == I32 and ratios.is_contiguous() and tuple(ratios.shape) == (n,)
    new_o, new_s = torch.empty_like(opacities), torch.empty_like(scales)
    check(_lib.lib().clmgs_mcmc_relocation(stream(), n, dptr(opacities, F32), dptr(scales, F32), dptr(ratios, I32),
                                           dptr(new_o), dptr(new_s)))
    return new_o, new_s


def _col_ptr(t, col):
    return ctypes.c_void_p(t.data_ptr() + 4 * col)


@torch.no_grad()
def mcmc_reg_grad_(c_o, c_s, opacity=None, scaling=None, g_opacity=None, g_scaling=None, packed=None, packed_grad=None):
    """ADDS the gradients of the two MCMC regularisers: g_opacity += c_o * s (1 - s), s = sigmoid(opacity);
    g_scaling += c_s * exp(scaling).  Either the four tensors (raw opacity [n,1], raw scaling [n,3] and their gradients)
    or `packed` / `packed_grad`, the [n,12] parameter mirror and gradient table (columns 3 and 4..6).  The caller folds
    1/N, 1/3 and any batch scale into c_o / c_s.  Writes nothing but those four gradient columns."""
    L = _lib.lib()
    if packed is not None:
        assert opacity is None and scaling is None and g_opacity is None and g_scaling is None
        n = packed.shape[0]
        _f32_dev(packed, (n, 12), "packed")
        _f32_dev(packed_grad, (n, 12), "packed_grad")
        assert packed.data_ptr() != packed_grad.data_ptr()
        check(L.clmgs_mcmc_reg_grad(stream(), n, _col_ptr(packed, 3), 12, _col_ptr(packed, 4), 12,
                                    _col_ptr(packed_grad, 3), 12, _col_ptr(packed_grad, 4), 12, float(c_o), float(c_s)))
        return
    n = scaling.shape[0]
    _f32_dev(opacity, (n, 1), "opacity")
    _f32_dev(scaling, (n, 3), "scaling")
    _f32_dev(g_opacity, (n, 1), "g_opacity")
    _f32_dev(g_scaling, (n, 3), "g_scaling")
    check(L.clmgs_mcmc_reg_grad(stream(), n, dptr(opacity, F32), 1, dptr(scaling, F32), 3, dptr(g_opacity, F32), 1,
                                dptr(g_scaling, F32), 3, float(c_o), float(c_s)))


@torch.no_grad()
def mcmc_inject_noise_(xyz, opacity, scaling, rotation, noise, scaler, packed=None):
    """In place: xyz += Sigma (noise * gate * scaler) with gate = 1 / (1 + exp(-100 ((1 - sigmoid(opacity)) - 0.995))) and
    Sigma = R diag(exp(scaling))^2 R^T, R of the normalised raw rotation (gsplat's inject_noise_to_position).  Raw
    parameter tensors [n,3] / [n,1] / [n,3] / [n,4]; noise [n,3] (torch.randn on the device).  packed: the [n,12] mirror
    of the small attributes; its columns 0..2 then receive the new positions in the same pass."""
    n = xyz.shape[0]
    _f32_dev(xyz, (n, 3), "xyz")
    _f32_dev(opacity, (n, 1), "opacity")
    _f32_dev(scaling, (n, 3), "scaling")
    _f32_dev(rotation, (n, 4), "rotation")
    _f32_dev(noise, (n, 3), "noise")
    if packed is not None:
        _f32_dev(packed, (n, 12), "packed")
    check(_lib.lib().clmgs_mcmc_noise(stream(), n, dptr(xyz, F32), dptr(opacity, F32), dptr(scaling, F32),
                                      dptr(rotation, F32), dptr(noise, F32), float(scaler), dptr(packed, F32, True)))


# ------------------------------------------------------------- SH row movement
def _idx64(t):
    return 1 if t is not None and t.dtype == I64 else 0


def _rows(fn, dst, src, dst_idx, src_idx, grid):
    L = _lib.lib()
    n = (dst_idx if dst_idx is not None else src_idx).numel() if (dst_idx is not None or src_idx is not None) else dst.shape[0]
    if dst_idx is not None and src_idx is not None and dst_idx.dtype != src_idx.dtype:
        src_idx = src_idx.to(dst_idx.dtype)
    is64 = _idx64(dst_idx if dst_idx is not None else src_idx)
    cols = src.shape[-1]
    check(getattr(L, fn)(stream(), dptr(dst, F32, allow_host=True), dptr(src, F32, allow_host=True),
                         dptr(dst_idx, None, True), dptr(src_idx, None, True), is64, int(n),
                         int(cols), int(grid)))


def send_shs2gpu_stream(shs, parameters, filter_idx, grid_size=0, block_size=256):
    """shs[i] = parameters[filter[i]]  (parameters may be pinned host memory)."""
    _rows("clmgs_rows_gather", shs, parameters, None, filter_idx, grid_size)


def send_shs2gpu_stream_retention(shs_next, parameters, shs_retent, host_indices_to_param,
                                  rtnt_indices_to_param, param_indices_from_host,
                                  param_indices_from_rtnt, grid_size=0, block_size=256,
                                  grid_size_D=0, block_size_D=256):
    """shs_next[param_indices_from_host[i]] = parameters[host_indices_to_param[i]] and
    shs_next[param_indices_from_rtnt[j]] = shs_retent[rtnt_indices_to_param[j]]."""
    if host_indices_to_param.numel():
        _rows("clmgs_rows_gather", shs_next, parameters, param_indices_from_host,
              host_indices_to_param, grid_size)
    if rtnt_indices_to_param.numel():
        _rows("clmgs_rows_gather", shs_next, shs_retent, param_indices_from_rtnt,
              rtnt_indices_to_param, grid_size_D)


def send_shs2cpu_grad_buffer_stream(shs_grad, grad_buffer, filter_idx, accum=True, grid_size=0,
                                    block_size=256):
    """grad_buffer[filter[i]] (+)= shs_grad[i]."""
    _rows("clmgs_rows_scatter_add" if accum else "clmgs_rows_gather", grad_buffer, shs_grad,
          filter_idx, None, grid_size)


def send_shs2cpu_grad_buffer_stream_retention(shs_grad, grad_buffer, shs_grad_next,
                                              host_indices_from_grad, rtnt_indices_from_grad,
                                              grad_indices_to_host, grad_indices_to_rtnt,
                                              accum=True, grid_size=0, block_size=256,
                                              grid_size_D=0, block_size_D=256):
    """grad_buffer[host_indices_from_grad[i]] += shs_grad[grad_indices_to_host[i]] and
    shs_grad_next[rtnt_indices_from_grad[j]] = shs_grad[grad_indices_to_rtnt[j]]."""
    if host_indices_from_grad.numel():
        _rows("clmgs_rows_scatter_add" if accum else "clmgs_rows_gather", grad_buffer, shs_grad,
              host_indices_from_grad, grad_indices_to_host, grid_size)
    if rtnt_indices_from_grad.numel():
        _rows("clmgs_rows_gather", shs_grad_next, shs_grad, rtnt_indices_from_grad,
              grad_indices_to_rtnt, grid_size_D)


@torch.no_grad()
def spherical_harmonics_bwd_inplace(degrees_to_use, dirs, coeffs, v_coeffs, v_colors):
    """SH backward that ACCUMULATES into the persistent v_coeffs[n,48] buffer and returns
    v_dirs (clm_offload/engine.py:709-716)."""
    L = _lib.lib()
    n = dirs.numel() // 3
    d2, c2, vc = dirs.contiguous(), coeffs.contiguous(), v_colors.contiguous()
    v_dirs = torch.empty_like(d2)
    check(L.clmgs_sh_bwd(stream(), n, int(degrees_to_use), dptr(d2, F32), dptr(c2, F32), None,
                         dptr(vc, F32), dptr(v_coeffs, F32), 1, dptr(v_dirs)))
    return v_dirs


# ------------------------------------------------------------------- bitmaps
def scatter_to_bit(bitmap, filter_idx, bit):
    L = _lib.lib()
    check(L.clmgs_scatter_to_bit(stream(), dptr(bitmap), bitmap.element_size(),
                                 dptr(filter_idx.contiguous(), I64), filter_idx.numel(), int(bit)))


def extract_ffs(bitmap, ffs):
    L = _lib.lib()
    check(L.clmgs_extract_ffs(stream(), dptr(bitmap), bitmap.element_size(), bitmap.numel(),
                              dptr(ffs, U8)))


def compute_cnt_h(bitmap, tmp_buffer, grid_size=64, block_size=256):
    """Reference contract (clm_offload/engine.py:227-233): fill tmp_buffer[bsz-1, T] with
    partial counts whose row sums are cnt_d[i] = #(F_i & F_{i+1}).  Here the full count lands
    in column 0 and the remaining columns are zero."""
    L = _lib.lib()
    bsz = tmp_buffer.shape[0] + 1
    cnt = torch.zeros((bsz - 1,), dtype=I32, device=bitmap.device)
    check(L.clmgs_pair_overlap_count(stream(), dptr(bitmap), bitmap.element_size(), bitmap.numel(),
                                     bsz, dptr(cnt)))
    tmp_buffer.zero_()
    tmp_buffer[:, 0] = cnt
    return cnt


def pair_overlap_count(bitmap, bsz):
    L = _lib.lib()
    cnt = torch.zeros((bsz - 1,), dtype=I32, device=bitmap.device)
    check(L.clmgs_pair_overlap_count(stream(), dptr(bitmap), bitmap.element_size(), bitmap.numel(),
                                     int(bsz), dptr(cnt)))
    return cnt


def set_signal(signal_tensor_pinned, idx, value):
    L = _lib.lib()
    check(L.clmgs_set_signal(stream(), ctypes.c_void_p(signal_tensor_pinned.data_ptr()), int(idx),
                             int(value)))


# ----------------------------------------------------------------------- Adam
def selective_adam_update(param, grad, exp_avg, exp_avg_sq, visibility, lr, beta1, beta2, eps, N, M):
    """Adam on rows where visibility is True, no bias correction (optimizer.py:76-88)."""
    L = _lib.lib()
    col_lr = torch.full((M,), float(lr), dtype=F32, device=param.device)
    vis = visibility.contiguous().view(U8)
    check(L.clmgs_adam_rows(stream(), dptr(param, F32), dptr(grad, F32), dptr(exp_avg, F32),
                            dptr(exp_avg_sq, F32), None, 0, dptr(vis, U8), int(N), int(M),
                            dptr(col_lr), float(beta1), float(beta2), float(eps), 1, 0, 1.0, 0))


def adam_rows(p, g, m, v, rows, col_lr, beta1, beta2, eps, step, bias_correction=True,
              grad_scale=1.0, zero_grad=False, mask=None):
    """Row-sparse Adam with per-column learning rate on device tensors [*, cols]."""
    L = _lib.lib()
    n_rows = rows.numel() if rows is not None else p.shape[0]
    cols = p.shape[-1] if p.dim() > 1 else 1
    check(L.clmgs_adam_rows(stream(), dptr(p, F32), dptr(g, F32, True), dptr(m, F32), dptr(v, F32),
                            dptr(rows, None, True), _idx64(rows),
                            dptr(mask.view(U8) if mask is not None else None, U8, True),
                            int(n_rows), int(cols), dptr(col_lr, F32), float(beta1), float(beta2),
                            float(eps), int(step), int(bool(bias_correction)), float(grad_scale),
                            int(bool(zero_grad))))


def adam_catch_up(p, m, v, last_step, rows, col_lr, beta1, beta2, eps, to_step, bias_correction=True,
                  max_replay=256, g=None, g_step=None, grad_scale=1.0, keep_grad=False, moment_row0=0):
    """Replay the deferred zero-gradient Adam steps of `rows` (None = all) up to `to_step` and
    stamp them; with g / g_step also apply the gradient step that is waiting for a row, at its own
    step (see clmgs_adam_catch_up).  moment_row0 > 0: m / v are a SHARD of the moment tables whose first row is
    global row `moment_row0` (camera-DP, moments held by the owner of a row range only); the explicit row list
    must then stay inside the shard -- the library indexes every table by global row id from the base pointer it
    is given (include/clmgs.h), so the shard travels as a base moved back by moment_row0 rows."""
    L = _lib.lib()
    n_rows = rows.numel() if rows is not None else p.shape[0]
    m_ptr, v_ptr = dptr(m, F32), dptr(v, F32)
    if moment_row0:
        assert rows is not None, "a moment shard needs an explicit row list"
        back = int(moment_row0) * int(p.shape[-1]) * 4
        m_ptr, v_ptr = ctypes.c_void_p(m_ptr.value - back), ctypes.c_void_p(v_ptr.value - back)
    check(L.clmgs_adam_catch_up(stream(), dptr(p, F32), m_ptr, v_ptr, dptr(last_step, I32),
                                dptr(rows, None, True), _idx64(rows), int(n_rows), int(p.shape[-1]),
                                dptr(col_lr, F32), float(beta1), float(beta2), float(eps), int(to_step),
                                int(bool(bias_correction)), int(max_replay), dptr(g, F32, True),
                                dptr(g_step, I32, True), float(grad_scale), int(bool(keep_grad))))
    if rows is None:
        last_step[: p.shape[0]].fill_(int(to_step))
    else:
        utils.fill_rows(last_step, rows.long(), int(to_step))  # scalar as kernel argument: no blocking H2D copy


def densify_stats(filter_idx, v_means2d, radii, width, height, max_radii2D, xyz_gradient_accum,
                  denom, only_visible=True):
    """Fused form of gsplat_add_densification_stats[_exact_filter]
    (clm_offload/gaussian_model.py:833-851, no_offload/gaussian_model.py:767-783)."""
    L = _lib.lib()
    n = radii.numel()
    check(L.clmgs_densify_stats(stream(), n, dptr(filter_idx, I64, True),
                                dptr(v_means2d.contiguous(), F32), dptr(radii.contiguous(), I32),
                                int(bool(only_visible)), float(width) * 0.5, float(height) * 0.5, dptr(max_radii2D, F32),
                                dptr(xyz_gradient_accum, F32), dptr(denom, F32)))
