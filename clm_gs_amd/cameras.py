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


# ------------------------------------------------------------------------------------------- resolution schedule
# ("Resolution schedule").  Level L of a W x H camera is the same pinhole at
# ceil(W / 2^L) x ceil(H / 2^L): same pose, same FoV, hence its own K (focal lengths and a centred principal point at the
# level's size).  The image EXTENT is the same at every level, which is what the area filter of csrc/resample.hip keeps.

# what a view shares with its camera -- the same tensors, nothing cloned: the side models step the tables the views read
_SHARED_BY_VIEWS = ("exposure", "exposure_grad", "bilagrid", "bilagrid_grad", "sky", "sky_acc", "invdepth_scale",
                    "invdepth_offset")


def level_view(camera, level, image=None, loss_mask=None, loss_mask_count=None, invdepth=None):
    """The Camera that renders `camera` at level `level`: same uid, name, pose and FoV, size (Wo, Ho) =
    ceil(size / 2^level), its own K, camtoworlds and cached host triple, and every side-model attribute of the camera as
    the same object.  `image`, `loss_mask` (+ `loss_mask_count`, a host integer) and `invdepth`: the level's ground truth
    (clm_kernels.area_resample), device tensors taken as they are; a view built without them is a shell (pose and K, no
    image).  level 0 is the camera itself: nothing is copied, nothing is launched.  An orthographic camera is refused."""
    level = int(level)
    if level < 0:
        raise ValueError(f"level_view: level must be >= 0, got {level}")
    refuse_ortho(camera, "level_view (the resolution schedule, --num_downscales)")
    if level == 0:
        return camera
    if getattr(camera, "pose_grad", None) is not None:
        raise ValueError("level_view: the camera carries a pose-gradient buffer (--pose_opt): pose refinement rewrites the "
                         "camera it is attached to and a level view would go stale; --num_downscales and --pose_opt "
                         "exclude each other")
    f = 1 << level
    W, H = int(camera.image_width), int(camera.image_height)
    Wo, Ho = (W + f - 1) // f, (H + f - 1) // f
    view = Camera.__new__(Camera)
    view.uid, view.image_name = camera.uid, camera.image_name
    view.FoVx, view.FoVy = float(camera.FoVx), float(camera.FoVy)
    view.image_width, view.image_height = Wo, Ho
    view.level, view.full_camera = level, camera
    view.world_view_transform = camera.world_view_transform
    view.camtoworlds = camera.camtoworlds
    device = camera.world_view_transform.device
    view.K = view.create_k_on_gpu(device)
    host = getattr(camera, "_clmgs_host", None)
    if host is None:
        w2c = camera.world_view_transform.detach().t().contiguous().cpu()
        host = (np.ascontiguousarray(w2c.numpy().astype(np.float32).reshape(16)), None,
                np.ascontiguousarray(torch.inverse(w2c)[:3, 3].numpy().astype(np.float32).reshape(3)))
    view._clmgs_host = (host[0], np.ascontiguousarray(view.create_k_on_gpu("cpu").numpy().astype(np.float32).reshape(9)),
                        host[2])
    view.original_image = image
    view.loss_mask, view.loss_mask_count = loss_mask, (None if loss_mask is None else loss_mask_count)
    view.invdepth = invdepth
    view.invdepth_scale = getattr(camera, "invdepth_scale", 1.0)
    view.invdepth_offset = getattr(camera, "invdepth_offset", 0.0)
    for name in _SHARED_BY_VIEWS:
        if hasattr(camera, name):
            setattr(view, name, getattr(camera, name))
    return view


class LevelCameras:
    """The training cameras of ONE level L >= 1 of the resolution schedule; the trainer builds one at a level switch and
    drops the previous one.
      - the shells (level_view: pose, K, shared side-model attributes) of every camera, once;
      - the loss masks and inverse-depth priors of the level (small), resampled once; each mask's count is read back
        here, once per camera and level, with one copy for all of them;
      - NO cache of images: batch() resamples the ground truth of a batch's cameras into a ring of 2 x bsz preallocated
        uint8 [3,Ho,Wo] buffers, on the current stream, and hands out the views.  Nothing is allocated per batch.
    Stream order of the ring: the resample kernels are enqueued on the current stream before the engine is called; every
    engine orders its side streams behind the current stream at the head of a batch (they read the parameters the
    optimizer stepped there) and has joined them into it when it returns (DESIGN.md names the lines), and a buffer is
    rewritten two batches after the batch that read it."""

    def __init__(self, cameras, level, bsz):
        from .clm_kernels import area_resample, level_size
        self.level, self.bsz = int(level), int(bsz)
        if self.level < 1:
            raise ValueError(f"LevelCameras: level must be >= 1, got {level} (level 0 is the cameras themselves)")
        sizes = {(int(c.image_height), int(c.image_width)) for c in cameras}
        if len(sizes) != 1:
            raise ValueError(f"LevelCameras: all cameras must share one size, got {sorted(sizes)}")
        (H, W), = sizes
        self.full_size = (H, W)
        self.size = level_size(H, W, self.level)  # (Ho, Wo)
        self.cameras = list(cameras)
        device = cameras[0].world_view_transform.device
        for c in cameras:  # planar and contiguous, as Camera keeps it: a strided image is copied once, here, not per batch
            if c.original_image is not None and not c.original_image.is_contiguous():
                c.original_image = c.original_image.contiguous()
        masked = [c for c in cameras if getattr(c, "loss_mask", None) is not None]
        masks, mask_counts = {}, {}
        if masked:
            counts = torch.zeros((len(masked),), dtype=torch.int64, device=device)
            for k, c in enumerate(masked):
                masks[id(c)] = area_resample(c.loss_mask, self.level, mask=True, count=counts[k:k + 1])[0]
            mask_counts = {id(c): int(n) for c, n in zip(masked, counts.cpu().tolist())}  # the one read-back of the level
        self.views = {}
        for c in cameras:
            raw = getattr(c, "invdepth", None)
            self.views[id(c)] = level_view(
                c, self.level, loss_mask=masks.get(id(c)), loss_mask_count=mask_counts.get(id(c)),
                invdepth=None if raw is None else area_resample(raw, self.level))
        self.ring = [torch.empty((3,) + self.size, dtype=torch.uint8, device=device) for _ in range(2 * self.bsz)]
        self.turn = 0

    def ring_bytes(self):
        return sum(t.numel() for t in self.ring)

    def batch(self, cameras):
        """The level's views of a batch's cameras, their ground truth resampled into the ring's next bsz buffers."""
        from .clm_kernels import area_resample
        if len(cameras) > self.bsz:
            raise ValueError(f"LevelCameras.batch: {len(cameras)} cameras, the ring was built for batches of {self.bsz}")
        base, self.turn = self.turn * self.bsz, self.turn ^ 1
        out = []
        for k, c in enumerate(cameras):
            view = self.views[id(c)]
            view.original_image = area_resample(c.original_image, self.level, out=self.ring[base + k])
            out.append(view)
        return out
