"""Camera objects exposing what the engines read (scene/cameras.py:39-126,
train.py:278-312): FoVx, FoVy, world_view_transform (row-vector convention,
i.e. the TRANSPOSE of the 4x4 world->camera matrix), K, camtoworlds,
original_image (uint8 [3,H,W] on the GPU), image_name, create_k_on_gpu(); plus loss_mask (uint8 [H,W] or None)
and loss_mask_count, the per-pixel ignore mask of the training loss.  A training camera may also carry ONE colour stage
(camera_colour below) -- `exposure` / `exposure_grad`, float32 [3,4] views of its rows in an exposure.ExposureModel, or
`bilagrid` / `bilagrid_grad`, float32 [L,Hg,Wg,12] views of its grids in a bilagrid.BilagridModel -- and `invdepth`
(uint16 [H,W]) with `invdepth_scale` / `invdepth_offset`, its monocular inverse-depth prior (camera_invdepth below), and
`pose_grad`, the float32 [15] buffer its pose gradient is added into (camera_pose_grad; pose.PoseModel rewrites
world_view_transform, camtoworlds and the cached host triple of a camera whose pose it has moved).  Any camera of a scene
with a learnable sky carries `sky`, the detached float32 [Hs,Ws,3] equirectangular map of a sky.SkyModel (one table shared
by all cameras), and `sky_acc`, the model's int64 [Hs,Ws,3] fixed-point gradient accumulator (unit 2^-48) for a camera
that trains the map, None for one that is only rendered (camera_sky).  OrthoCamera is the orthographic kind
(`camera_model = "ortho"`, read through camera_model()): rendered by the eval entries only, refused by the training ones."""
import math

import numpy as np
import torch


def camera_loss_mask(camera):
    """(mask, count) of a camera's per-pixel ignore mask of the loss (Camera.loss_mask: uint8 [H,W], 0 =
    ignored), or (None, None).  The count is a host integer the camera carries (taken once, before the upload); a
    camera object that only has the tensor gets it counted here, once."""
    mask = getattr(camera, "loss_mask", None)
    if mask is None:
        return None, None
    count = getattr(camera, "loss_mask_count", None)
    if count is None:
        count = camera.loss_mask_count = int(torch.count_nonzero(mask).item())
    return mask, int(count)


def camera_colour(camera):
    """The colour stage a camera carries between the rasterizer and the loss: (kind, param, grad) with kind "exposure"
    (param float32 [3,4]) or "bilagrid" (param float32 [L,Hg,Wg,12]) -- views into the tables of a colour_model.ColourModel
    (`camera.<kind>`, `camera.<kind>_grad`; grad may be None) -- or None: a camera without the attributes, or with None, is
    rendered and trained as the model is.  A camera that carries both is refused: the order in which the two transforms
    compose is not defined."""
    row, grid = getattr(camera, "exposure", None), getattr(camera, "bilagrid", None)
    if row is not None and grid is not None:
        raise ValueError("a camera carries both an exposure row and a bilateral grid: the order of composition is not "
                         "defined; train with --exposure or with --bilagrid")
    if row is not None:
        return "exposure", row, getattr(camera, "exposure_grad", None)
    if grid is not None:
        return "bilagrid", grid, getattr(camera, "bilagrid_grad", None)
    return None


def camera_exposure(camera):
    """(row, grad_row) of camera_colour for a camera whose stage is an exposure row, else (None, None); for callers
    outside the stage (the scene tests)."""
    c = camera_colour(camera)
    return c[1:] if c is not None and c[0] == "exposure" else (None, None)


def camera_bilagrid(camera):
    """(grid, grad) of camera_colour for a camera whose stage is a bilateral grid, else (None, None)."""
    c = camera_colour(camera)
    return c[1:] if c is not None and c[0] == "bilagrid" else (None, None)


def camera_invdepth(camera):
    """(raw, scale, offset) of a camera's inverse-depth prior -- raw uint16 [H,W] on the device, two host floats; the
    prior is raw / 65536 * scale + offset, the INRIA 3DGS 16-bit PNG + depth_params.json convention -- or None: a camera
    without the attribute, or with None, is rendered with three channels and trained without the depth term."""
    raw = getattr(camera, "invdepth", None)
    if raw is None:
        return None
    return raw, float(getattr(camera, "invdepth_scale", 1.0)), float(getattr(camera, "invdepth_offset", 0.0))


def camera_pose_grad(camera):
    """The camera's pose-gradient buffer -- float32 [15] on the device, v_R 9 | v_t 3 | v_campos 3, a view of its row in a
    pose.PoseModel (`camera.pose_grad`) that the kernels of csrc/pose.hip ADD into -- or None: a camera without the
    attribute, or with None, is trained exactly as before (nothing more is launched)."""
    return getattr(camera, "pose_grad", None)


def camera_sky(camera):
    """The sky a camera is rendered in front of: (sky, sky_acc) -- `camera.sky`, the detached float32 [Hs,Ws,3] map of a
    sky.SkyModel (one table, shared by every camera of the scene), and `camera.sky_acc`, the model's int64 [Hs,Ws,3]
    fixed-point gradient accumulator, or None for a camera that does not train the map (evaluation, test, trajectory) --
    or None: a camera without the attribute, or with None, is rendered over the constant background as before (nothing
    more is launched).  Refused with a pose-gradient buffer, here, before anything is enqueued: the gradient of the
    lookup with respect to the ray direction is not carried."""
    sky = getattr(camera, "sky", None)
    if sky is None:
        return None
    if getattr(camera, "pose_grad", None) is not None:
        raise ValueError("a camera carries both a sky and a pose-gradient buffer: the sky's gradient with respect to the "
                         "camera is not carried; train with --sky or with --pose_opt")
    return sky, getattr(camera, "sky_acc", None)


def check_sky_background(background):
    """A camera with a sky is composited over the map, so a constant background has no meaning: a non-zero one is refused
    (before anything is enqueued; the value is read on the host once per tensor)."""
    if background is None:
        return
    ok = getattr(background, "_clmgs_sky_ok", None)
    if ok is None:
        ok = not bool(torch.count_nonzero(background.detach()).item())
        try:
            background._clmgs_sky_ok = ok
        except AttributeError:
            pass
    if not ok:
        raise ValueError("a non-zero background reaches a camera that has a sky: the sky is the background "
                         "(--white_background and --sky exclude each other)")


class Camera:
    def __init__(self, uid, world_to_cam, FoVx, FoVy, width, height, image_u8=None,
                 image_name=None, device="cuda", loss_mask=None, invdepth=None, invdepth_scale=1.0,
                 invdepth_offset=0.0):
        self.uid = uid
        self.FoVx, self.FoVy = float(FoVx), float(FoVy)
        self.image_width, self.image_height = int(width), int(height)
        self.image_name = image_name or f"cam_{uid:05d}"
        w2c = torch.as_tensor(world_to_cam, dtype=torch.float32)
        self.world_view_transform = w2c.t().contiguous().to(device)
        # planar and contiguous, as the reference keeps it (scene/cameras.py:74 "image.contiguous()"): the loss
        # kernels read it in place; a strided image would cost fused.camera_forward_finish a copy per camera
        self.original_image = image_u8.to(device).contiguous() if image_u8 is not None else None
        # per-pixel ignore mask of the training loss: uint8 [H,W], 0 = ignored, anything else = counted; None = every
        # pixel.  The count of counted pixels is taken HERE, on the host, before the upload: the loss value needs it
        # at every step and must not read the device back for it.
        self.loss_mask, self.loss_mask_count = None, None
        if loss_mask is not None:
            m = torch.as_tensor(loss_mask)
            if m.dtype == torch.bool:
                m = m.to(torch.uint8)
            if m.dtype != torch.uint8 or tuple(m.shape) != (self.image_height, self.image_width):
                raise ValueError(f"loss_mask must be uint8 [{self.image_height}, {self.image_width}], "
                                 f"got {m.dtype} {tuple(m.shape)}")
            self.loss_mask_count = int(torch.count_nonzero(m))
            self.loss_mask = m.to(device).contiguous()
        # monocular inverse-depth prior of the depth regularisation: uint16 [H,W], prior = raw / 65536 * scale + offset
        self.invdepth, self.invdepth_scale, self.invdepth_offset = None, float(invdepth_scale), float(invdepth_offset)
        if invdepth is not None:
            d = torch.as_tensor(invdepth)
            if d.dtype != torch.uint16 or tuple(d.shape) != (self.image_height, self.image_width):
                raise ValueError(f"invdepth must be uint16 [{self.image_height}, {self.image_width}], "
                                 f"got {d.dtype} {tuple(d.shape)}")
            if not (math.isfinite(self.invdepth_scale) and math.isfinite(self.invdepth_offset)):
                raise ValueError(f"invdepth_scale / invdepth_offset must be finite, got {invdepth_scale} {invdepth_offset}")
            self.invdepth = d.to(device).contiguous()
        self.K = self.create_k_on_gpu(device)
        c2w = torch.inverse(w2c)
        self.camtoworlds = c2w[None].to(device)  # [1,4,4] as train.py:293-301
        # host copies of the per-camera constants the kernels take by value (fused._cam_host would
        # otherwise read them back from the device: three blocking copies per new camera)
        k_host = self.create_k_on_gpu("cpu")
        self._clmgs_host = (np.ascontiguousarray(w2c.numpy().astype(np.float32).reshape(16)),
                            np.ascontiguousarray(k_host.numpy().astype(np.float32).reshape(9)),
                            np.ascontiguousarray(c2w[:3, 3].numpy().astype(np.float32).reshape(3)))

    def create_k_on_gpu(self, device="cuda"):
        fx = self.image_width / (2 * math.tan(self.FoVx * 0.5))
        fy = self.image_height / (2 * math.tan(self.FoVy * 0.5))
        return torch.tensor([[fx, 0, self.image_width / 2.0], [0, fy, self.image_height / 2.0],
                             [0, 0, 1]], dtype=torch.float32, device=device)


def camera_model(camera):
    """The projection a camera is rendered with: "ortho" for an OrthoCamera, "pinhole" for any object without the
    attribute (every training camera)."""
    return getattr(camera, "camera_model", "pinhole")


def refuse_ortho(camera, where):
    """Training entries: an orthographic camera is refused by name, before anything is enqueued."""
    if camera_model(camera) != "pinhole":
        raise ValueError(f"{where}: camera {getattr(camera, 'image_name', camera)!r} is orthographic "
                         f"(camera_model={camera_model(camera)!r}); orthographic cameras are rendered through the eval "
                         "entries only, training on them is not supported")


class OrthoCamera:
    """An orthographic camera (gsplat's camera_model="ortho") for the eval entries: K = [[sx,0,cx],[0,sy,cy],[0,0,1]]
    with sx, sy in pixels per world unit (`pixels_per_unit`: a scalar or an (sx, sy) pair).  cx, cy default to the image
    centre and may lie outside the image: that is how one window of a larger map is addressed.  Carries K,
    world_view_transform, camtoworlds and the host triple like Camera; no image, masks or colour stage."""
    camera_model = "ortho"

    def __init__(self, uid, world_to_cam, pixels_per_unit, width, height, cx=None, cy=None, image_name=None,
                 device="cuda"):
        self.uid = uid
        try:
            sx, sy = pixels_per_unit
        except TypeError:
            sx = sy = pixels_per_unit
        self.sx, self.sy = float(sx), float(sy)
        if not (self.sx > 0 and self.sy > 0 and math.isfinite(self.sx) and math.isfinite(self.sy)):
            raise ValueError(f"pixels_per_unit must be positive and finite, got {pixels_per_unit}")
        self.image_width, self.image_height = int(width), int(height)
        self.cx = self.image_width / 2.0 if cx is None else float(cx)
        self.cy = self.image_height / 2.0 if cy is None else float(cy)
        self.image_name = image_name or f"ortho_{uid:05d}"
        w2c = torch.as_tensor(world_to_cam, dtype=torch.float32)
        self.world_view_transform = w2c.t().contiguous().to(device)
        self.original_image = None
        self.K = self.create_k_on_gpu(device)
        c2w = torch.inverse(w2c)
        self.camtoworlds = c2w[None].to(device)
        self._clmgs_host = (np.ascontiguousarray(w2c.numpy().astype(np.float32).reshape(16)),
                            np.ascontiguousarray(self.create_k_on_gpu("cpu").numpy().astype(np.float32).reshape(9)),
                            np.ascontiguousarray(c2w[:3, 3].numpy().astype(np.float32).reshape(3)))

    def create_k_on_gpu(self, device="cuda"):
        return torch.tensor([[self.sx, 0, self.cx], [0, self.sy, self.cy], [0, 0, 1]], dtype=torch.float32, device=device)
