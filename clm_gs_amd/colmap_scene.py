"""COLMAP-lite scene loader: a COLMAP model directory -> the cameras, initial
point cloud and scene radius the engines train from, so a real dataset runs when one is present.

Behaviour follows the reference's reader (scene/dataset_readers.py:59-252, scene/colmap_loader.py):
`<source>/sparse/0/{cameras,images,points3D}.bin` (text `.txt` as the fallback), cameras of the models
SIMPLE_PINHOLE / PINHOLE / OPENCV (distortion ignored, as there), images sorted by name, every
`llffhold`-th image held out when `eval`, scene radius = 1.1 x the largest distance of a training camera
centre from their mean (getNerfppNorm).  The file formats are COLMAP's published model formats
(https://colmap.github.io/format.html); the parsing below is written against that description with
numpy record reads.  Images are decoded with PIL to uint8 [3,H,W] (what the engines' fused loss reads).
With `undistort=True` the distorted models SIMPLE_RADIAL / RADIAL / OPENCV / OPENCV_FISHEYE and off-centre principal
points are remapped onto centred pinholes on the device at load (clm_kernels.undistort; load_colmap_scene's docstring).
"""
import math
import os
from types import SimpleNamespace

import numpy as np
import torch

from .cameras import Camera

# COLMAP camera models: id -> (name, number of parameters)
CAMERA_MODELS = {0: ("SIMPLE_PINHOLE", 3), 1: ("PINHOLE", 4), 2: ("SIMPLE_RADIAL", 4), 3: ("RADIAL", 5),
                 4: ("OPENCV", 8), 5: ("OPENCV_FISHEYE", 8), 6: ("FULL_OPENCV", 12), 7: ("FOV", 5),
                 8: ("SIMPLE_RADIAL_FISHEYE", 4), 9: ("RADIAL_FISHEYE", 5), 10: ("THIN_PRISM_FISHEYE", 12)}
_MODEL_BY_NAME = {name: (mid, n) for mid, (name, n) in CAMERA_MODELS.items()}


class _Reader:
    """Little-endian cursor over a whole model file held in memory."""

    def __init__(self, path):
        with open(path, "rb") as f:
            self.buf = f.read()
        self.pos = 0

    def take(self, dtype, count=1):
        dt = np.dtype(dtype).newbyteorder("<")
        n = dt.itemsize * count
        if self.pos + n > len(self.buf):
            raise ValueError("truncated COLMAP model file")
        out = np.frombuffer(self.buf, dtype=dt, count=count, offset=self.pos)
        self.pos += n
        return out

    def cstring(self):
        end = self.buf.index(b"\x00", self.pos)
        s = self.buf[self.pos:end].decode("utf-8")
        self.pos = end + 1
        return s


def read_cameras_binary(path):
    """cameras.bin -> {camera_id: namespace(id, model, width, height, params)}."""
    r = _Reader(path)
    out = {}
    for _ in range(int(r.take("u8")[0])):
        cam_id, model_id = (int(v) for v in r.take("i4", 2))
        width, height = (int(v) for v in r.take("u8", 2))
        if model_id not in CAMERA_MODELS:
            raise ValueError(f"unknown COLMAP camera model id {model_id}")
        name, n_par = CAMERA_MODELS[model_id]
        out[cam_id] = SimpleNamespace(id=cam_id, model=name, width=width, height=height,
                                      params=r.take("f8", n_par).copy())
    return out


def read_images_binary(path):
    """images.bin -> {image_id: namespace(id, qvec[w,x,y,z], tvec, camera_id, name)} (the 2-D
    observations are skipped)."""
    r = _Reader(path)
    out = {}
    for _ in range(int(r.take("u8")[0])):
        image_id = int(r.take("i4")[0])
        pose = r.take("f8", 7).copy()
        camera_id = int(r.take("i4")[0])
        name = r.cstring()
        n_obs = int(r.take("u8")[0])
        r.pos += 24 * n_obs  # (x f8, y f8, point3D_id i8) per observation
        out[image_id] = SimpleNamespace(id=image_id, qvec=pose[:4], tvec=pose[4:], camera_id=camera_id, name=name)
    return out


def read_points3d_binary(path):
    """points3D.bin -> (xyz float64 [n,3], rgb uint8 [n,3], error float64 [n])."""
    r = _Reader(path)
    n = int(r.take("u8")[0])
    xyz, rgb, err = np.empty((n, 3)), np.empty((n, 3), dtype=np.uint8), np.empty((n,))
    for i in range(n):
        r.pos += 8  # point id
        xyz[i] = r.take("f8", 3)
        rgb[i] = r.take("u1", 3)
        err[i] = r.take("f8")[0]
        track_len = int(r.take("u8")[0])
        r.pos += 8 * track_len  # track: (image_id i4, point2D_idx i4) each
    return xyz, rgb, err


def _data_lines(path):
    with open(path, "r") as f:
        for line in f:
            line = line.strip()
            if line and not line.startswith("#"):
                yield line


def read_cameras_text(path):
    out = {}
    for line in _data_lines(path):
        t = line.split()
        if t[1] not in _MODEL_BY_NAME:
            raise ValueError(f"unknown COLMAP camera model {t[1]}")
        out[int(t[0])] = SimpleNamespace(id=int(t[0]), model=t[1], width=int(t[2]), height=int(t[3]),
                                         params=np.array([float(v) for v in t[4:]]))
    return out


def read_images_text(path):
    """images.txt holds TWO lines per image (pose line, observations line; the second may be empty)."""
    out = {}
    with open(path, "r") as f:
        lines = [ln.rstrip("\n") for ln in f if not ln.lstrip().startswith("#")]
    i = 0
    while i < len(lines):
        if not lines[i].strip():
            i += 1
            continue
        t = lines[i].split()
        out[int(t[0])] = SimpleNamespace(id=int(t[0]), qvec=np.array([float(v) for v in t[1:5]]),
                                         tvec=np.array([float(v) for v in t[5:8]]), camera_id=int(t[8]),
                                         name=" ".join(t[9:]))
        i += 2
    return out


def read_points3d_text(path):
    rows = [ln.split() for ln in _data_lines(path)]
    xyz = np.array([[float(v) for v in t[1:4]] for t in rows]).reshape(-1, 3)
    rgb = np.array([[int(v) for v in t[4:7]] for t in rows], dtype=np.uint8).reshape(-1, 3)
    err = np.array([float(t[7]) for t in rows])
    return xyz, rgb, err


def quat_to_rotation(q):
    """COLMAP quaternion (w, x, y, z), world -> camera rotation matrix."""
    w, x, y, z = (float(v) for v in q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


def focal_to_fov(focal, pixels):
    return 2.0 * math.atan(pixels / (2.0 * focal))


def _intrinsics_to_fov(cam):
    if cam.model == "SIMPLE_PINHOLE":
        fx = fy = cam.params[0]
    elif cam.model in ("PINHOLE", "OPENCV"):  # OPENCV: the four distortion terms are ignored, as upstream
        fx, fy = cam.params[0], cam.params[1]
    else:
        raise ValueError(f"COLMAP camera model {cam.model} is not handled: undistort the dataset "
                         "(PINHOLE / SIMPLE_PINHOLE / OPENCV cameras only)")
    return focal_to_fov(fx, cam.width), focal_to_fov(fy, cam.height)


def scene_radius(world_to_cams):
    """(translate, radius) of getNerfppNorm: radius = 1.1 x max distance of a camera centre from their mean."""
    centres = np.stack([np.linalg.inv(m)[:3, 3] for m in world_to_cams])
    mean = centres.mean(axis=0)
    return -mean, 1.1 * float(np.linalg.norm(centres - mean, axis=1).max())


def _decode_image(path, resolution, want_alpha=False):
    """-> uint8 [3,H,W]; with want_alpha -> (image, alpha) where alpha is the uint8 [H,W] alpha channel of an image
    that has one -- as a band, or as the transparency entry of a palette / grey / RGB PNG -- (resized with nearest
    neighbour, like a mask file) and None otherwise."""
    from PIL import Image
    with Image.open(path) as im:
        alpha = None
        if want_alpha and "A" in im.getbands():
            alpha = im.getchannel("A")
        elif want_alpha and "transparency" in im.info:  # palette / grey / RGB PNG with a tRNS chunk: no A band of its own
            alpha = im.convert("RGBA").getchannel("A")
        im = im.convert("RGB")
        if resolution not in (1, None):
            im = im.resize((round(im.width / resolution), round(im.height / resolution)))
            if alpha is not None:
                alpha = alpha.resize(im.size, Image.NEAREST)
        a = np.array(im, dtype=np.uint8)  # a writable copy
        if alpha is not None:
            alpha = torch.from_numpy(np.array(alpha, dtype=np.uint8))
    img = torch.from_numpy(a).permute(2, 0, 1).contiguous()
    return (img, alpha) if want_alpha else img


def _mask_path(mask_dir, image_file):
    """COLMAP's convention first (`NAME.EXT.png` for image `NAME.EXT`), then `NAME.png`; None if neither exists."""
    for cand in (image_file + ".png", os.path.splitext(image_file)[0] + ".png"):
        p = os.path.join(mask_dir, cand)
        if os.path.exists(p):
            return p
    return None


def _decode_mask(path, size_wh):
    """A mask file as 8-bit grey -> uint8 [H,W] (non-zero = counted), resized with nearest neighbour to the decoded
    image's size when the images were scaled (`resolution`)."""
    from PIL import Image
    with Image.open(path) as im:
        im = im.convert("L")
        if size_wh is not None and im.size != size_wh:
            im = im.resize(size_wh, Image.NEAREST)
        return torch.from_numpy(np.array(im, dtype=np.uint8))


def _decode_invdepth(path, size_wh):
    """A 16-bit grey PNG -> uint16 [H,W] (the raw inverse-depth prior: prior = raw / 65536 * scale + offset).  A map of
    another size than the training image (`resolution`) is resampled to it: bilinear on float32, then rounded back to
    uint16."""
    from PIL import Image
    with Image.open(path) as im:
        a = np.array(im)
    if a.ndim != 2 or a.dtype != np.uint16:
        raise ValueError(f"depth map {path} must be a 16-bit grey PNG, got {a.dtype} {a.shape}")
    if size_wh is not None and (a.shape[1], a.shape[0]) != tuple(size_wh):
        f = Image.fromarray(a.astype(np.float32)).resize(tuple(size_wh), Image.BILINEAR)
        a = np.clip(np.rint(np.array(f, dtype=np.float32)), 0, 65535).astype(np.uint16)
    return torch.from_numpy(np.ascontiguousarray(a))


def read_depth_params(path):
    """`depth_params.json` ({NAME: {"scale": s, "offset": o}}) -> ({NAME: (scale, offset)}, median of the positive
    scales or None); a missing file gives ({}, None)."""
    import json
    if not os.path.exists(path):
        return {}, None
    with open(path) as f:
        raw = json.load(f)
    params = {k: (float(v["scale"]), float(v["offset"])) for k, v in raw.items()}
    pos = [s for s, _ in params.values() if s > 0]
    return params, (float(np.median(pos)) if pos else None)


def reliable_depth_params(params, med_scale, name):
    """(scale, offset) of image `name`, or None by the INRIA code base's reliability rule: no json entry, scale <= 0, or a
    scale outside [0.2, 5] x the median scale."""
    if name not in params or med_scale is None:
        return None
    scale, offset = params[name]
    if scale <= 0 or scale < 0.2 * med_scale or scale > 5.0 * med_scale:
        return None
    return scale, offset


def read_model(sparse_dir):
    """(cameras, images, (xyz, rgb)) from a `sparse/0` directory: binary files first, text as the fallback."""
    def pick(stem, rb, rt):
        b, t = os.path.join(sparse_dir, stem + ".bin"), os.path.join(sparse_dir, stem + ".txt")
        if os.path.exists(b):
            return rb(b)
        if os.path.exists(t):
            return rt(t)
        raise FileNotFoundError(f"no {stem}.bin / {stem}.txt in {sparse_dir}")
    cams = pick("cameras", read_cameras_binary, read_cameras_text)
    imgs = pick("images", read_images_binary, read_images_text)
    try:
        xyz, rgb, _ = pick("points3D", read_points3d_binary, read_points3d_text)
    except FileNotFoundError:
        xyz, rgb = None, None
    return cams, imgs, (xyz, rgb)


class _Undistorter:
    """The remap of load_colmap_scene(undistort=True): one reused device staging buffer per kind (image, mask, prior) that
    a distorted file is uploaded into, one kernel (clm_kernels.undistort) into the tensor the camera keeps -- the distorted
    copy of an image never stays next to the undistorted one -- and, per COLMAP camera id, the number of pixels that have
    no source (taken once, from the first image of that camera)."""

    def __init__(self, device, zoom):
        self.device, self.zoom, self.staging, self.sourced = device, zoom, {}, {}

    def _stage(self, kind, host):
        buf = self.staging.get(kind)
        if buf is None or buf.shape != host.shape or buf.dtype != host.dtype:
            buf = self.staging[kind] = torch.empty(host.shape, dtype=host.dtype, device=self.device)
        return buf.copy_(host)

    def image(self, cam_id, lens, img, mask):
        """(image, loss mask or None, count or None) on the device: the mask is `valid AND file mask` (a pixel blended from
        an ignored pixel is ignored), None when every pixel is counted."""
        from .clm_kernels import undistort
        h, w = int(img.shape[1]), int(img.shape[2])
        lens = lens.at(w, h)
        if lens.is_identity((h, w), self.zoom):  # nothing to remap: nothing is launched
            self.sourced.setdefault(cam_id, (h * w, h * w))
            return img, mask, None
        if torch.device(self.device).type != "cuda":
            raise ValueError(f"undistort=True with images needs a GPU device, got device={self.device!r}: the remap of "
                             f"{lens!r} is a device kernel (load_images=False builds the geometry only)")
        src_mask = None if mask is None else self._stage("mask", mask)
        out, valid, count = undistort(self._stage("image", img), lens, zoom=self.zoom, src_mask=src_mask, want_valid=True)
        count = int(count.item())  # the one read-back of the camera
        if cam_id not in self.sourced:
            n = count if src_mask is None else int(undistort(src_mask, lens, zoom=self.zoom, want_valid=True)[2].item())
            self.sourced[cam_id] = (n, h * w)
        if count == h * w:
            return out, None, None
        return out, valid, count

    def prior(self, lens, raw):
        from .clm_kernels import undistort
        lens = lens.at(int(raw.shape[1]), int(raw.shape[0]))
        if lens.is_identity(tuple(raw.shape), self.zoom):
            return raw
        return undistort(self._stage("prior", raw), lens, zoom=self.zoom)

    def log_lines(self, lenses):
        """One line per COLMAP camera id: the model, its parameters and the share of pixels without a source."""
        out = []
        for cam_id, lens in sorted(lenses.items()):
            line = "undistort: camera {} {} [{}] {}x{} zoom {:g}".format(
                cam_id, lens.model, ", ".join("%.6g" % p for p in lens.params), lens.width, lens.height, self.zoom)
            if cam_id in self.sourced:
                n, total = self.sourced[cam_id]
                lost = 1.0 - n / float(total)
                line += ": {:.2%} of the pixels have no source".format(lost)
                if lens.fisheye and lost > 0.25:
                    line += (" (more than a quarter is lost to the fisheye: a lower --undistort_zoom keeps more of its frame, "
                             "a higher one crops the pinhole to the pixels that have a source)")
            out.append(line)
        return out


def load_colmap_scene(source_path, images="images", eval=False, llffhold=10, resolution=1, device="cuda",
                      load_images=True, masks=None, alpha_mask=False, depths=None, undistort=False, undistort_zoom=1.0):
    """-> namespace(train_cameras, test_cameras, point_cloud(points, colors in [0,1]) or None,
    cameras_extent, nerf_normalization).  `cameras_extent` is what the trainer passes as
    `spatial_lr_scale` and what densification compares scales with (train.py:118-131).
    Per-pixel ignore masks of the loss (Camera.loss_mask): `masks` is a directory (relative to `source_path`, or
    absolute) holding `NAME.EXT.png` (COLMAP's convention) or `NAME.png` for image `NAME.EXT`, read as 8-bit grey,
    non-zero = counted; with `resolution` it is resized (nearest neighbour) to the decoded image's size, a mask of
    another size raises, an image without a mask file stays unmasked.  `alpha_mask`: an image with transparency (an
    alpha band, or a PNG `tRNS` entry) and without a mask file takes `alpha > 0`.  Without both, nothing changes.
    Inverse-depth priors of the depth regularisation (Camera.invdepth, TRAINING cameras only): `depths` is a directory
    (relative to `source_path`, or absolute) of 16-bit grey PNGs `NAME.png` for image `NAME.EXT`, with
    `sparse/0/depth_params.json` = {NAME: {"scale": s, "offset": o}} (prior = raw / 65536 * scale + offset); a map of
    another size than the training image is resampled to it (bilinear on float32, rounded back to uint16).  An image gets
    no prior when its PNG or its json entry is missing, its scale is <= 0, or its scale lies outside [0.2, 5] x the median
    scale (reliable_depth_params).
    Lens distortion (`undistort`, `undistort_zoom`; DESIGN.md section 3, "Lens distortion").  False: SIMPLE_RADIAL, RADIAL
    and OPENCV_FISHEYE cameras are refused, the distortion terms of an OPENCV camera and every principal point are
    ignored.  True: cameras of the models SIMPLE_PINHOLE, PINHOLE, SIMPLE_RADIAL, RADIAL, OPENCV and OPENCV_FISHEYE
    (clm_kernels.Lens; any other is refused by name) become the CENTRED pinhole of the decoded size with
    FoV = 2 atan(size / (2 f zoom)), and the image, its mask file or alpha mask and its inverse-depth prior are remapped
    onto it on the device at load (clm_kernels.undistort).  The loss mask becomes `valid AND file mask`; a camera whose
    every pixel has a source and that has no mask file carries none.  `load_images=False` builds the geometry only; images
    on a CPU `device` with a lens that is not the identity are refused.  The scene carries `undistort_log`, one line per
    COLMAP camera id (also printed)."""
    from .clm_kernels import Lens, check_undistort_zoom
    cams, imgs, (xyz, rgb) = read_model(os.path.join(source_path, "sparse", "0"))
    folder = os.path.join(source_path, images or "images")
    zoom = check_undistort_zoom(undistort_zoom) if undistort else 1.0
    used = sorted({im.camera_id for im in imgs.values()})
    lenses = {cid: Lens(cams[cid].model, cams[cid].params, cams[cid].width, cams[cid].height) for cid in used} if undistort else {}
    remap = _Undistorter(device, zoom) if undistort and load_images else None
    recs = []
    for im in imgs.values():
        intr = cams[im.camera_id]
        fovx, fovy = (None, None) if undistort else _intrinsics_to_fov(intr)  # (with a lens: from the decoded size, in build)
        w2c = np.eye(4)
        w2c[:3, :3] = quat_to_rotation(im.qvec)
        w2c[:3, 3] = im.tvec
        base = os.path.basename(im.name)
        recs.append(SimpleNamespace(uid=intr.id, w2c=w2c, fovx=fovx, fovy=fovy, width=intr.width, height=intr.height,
                                    path=os.path.join(folder, base), name=base.split(".")[0]))
    recs.sort(key=lambda r: r.name)
    if eval:
        train = [r for i, r in enumerate(recs) if i % llffhold != 0]
        test = [r for i, r in enumerate(recs) if i % llffhold == 0]
    else:
        train, test = recs, []
    translate, radius = scene_radius([r.w2c for r in train])

    mask_dir = None
    if masks:
        mask_dir = masks if os.path.isabs(masks) else os.path.join(source_path, masks)
        if not os.path.isdir(mask_dir):
            raise FileNotFoundError(f"mask directory {mask_dir} does not exist")

    depth_dir, depth_params, med_scale = None, {}, None
    if depths:
        depth_dir = depths if os.path.isabs(depths) else os.path.join(source_path, depths)
        if not os.path.isdir(depth_dir):
            raise FileNotFoundError(f"depth directory {depth_dir} does not exist")
        params_path = os.path.join(source_path, "sparse", "0", "depth_params.json")
        if not os.path.exists(params_path):  # a depth directory without its scales: stop, as the INRIA code base does
            raise FileNotFoundError(f"depths={depths!r} was asked for but {params_path} does not exist (the per-image "
                                    "scale and offset of the inverse-depth maps)")
        depth_params, med_scale = read_depth_params(params_path)

    def build(r, training=True):
        img, mask = None, None
        w, h = r.width, r.height
        if load_images:
            if alpha_mask:
                img, alpha = _decode_image(r.path, resolution, want_alpha=True)
            else:
                img, alpha = _decode_image(r.path, resolution), None
            h, w = int(img.shape[1]), int(img.shape[2])  # the decoded size wins, as upstream (image.size)
        elif resolution not in (1, None):
            w, h = round(w / resolution), round(h / resolution)
        if load_images:
            mpath = _mask_path(mask_dir, os.path.basename(r.path)) if mask_dir else None
            if mpath is not None:
                mask = _decode_mask(mpath, (w, h) if resolution not in (1, None) else None)
                if tuple(mask.shape) != (h, w):
                    raise ValueError(f"mask {mpath} is {tuple(mask.shape)[1]}x{tuple(mask.shape)[0]}, "
                                     f"image {r.path} is {w}x{h}")
            elif alpha is not None:
                mask = (alpha > 0).to(torch.uint8)
        prior = {}
        if depth_dir and training:
            so = reliable_depth_params(depth_params, med_scale, r.name)
            dpath = os.path.join(depth_dir, r.name + ".png")
            if so is not None and os.path.exists(dpath):
                prior = dict(invdepth=_decode_invdepth(dpath, (w, h)), invdepth_scale=so[0], invdepth_offset=so[1])
        if not undistort:
            return Camera(r.uid, torch.from_numpy(r.w2c).float(), r.fovx, r.fovy, w, h, image_u8=img,
                          image_name=r.name, device=device, loss_mask=mask, **prior)
        lens = lenses[r.uid].at(w, h)
        count = None
        if remap is not None:
            img, mask, count = remap.image(r.uid, lens, img, mask)
            if "invdepth" in prior:
                prior["invdepth"] = remap.prior(lens, prior["invdepth"])
        cam = Camera(r.uid, torch.from_numpy(r.w2c).float(), focal_to_fov(lens.fx * zoom, w), focal_to_fov(lens.fy * zoom, h),
                     w, h, image_u8=img, image_name=r.name, device=device, loss_mask=mask if count is None else None, **prior)
        if count is not None:  # the kernel's valid map, already on the device, and the kernel's count
            cam.loss_mask, cam.loss_mask_count = mask, count
        return cam

    pcd = None
    if xyz is not None and len(xyz):
        pcd = SimpleNamespace(points=xyz.astype(np.float32), colors=rgb.astype(np.float32) / 255.0,
                              normals=np.zeros_like(xyz, dtype=np.float32))
    train_cameras = [build(r) for r in train]
    if depth_dir:  # said aloud: a run whose priors were all dropped must not look like a run with priors
        n_prior = sum(c.invdepth is not None for c in train_cameras)
        print(f"depth priors: {n_prior} of {len(train_cameras)} training cameras ({depth_dir}; an image without a PNG, "
              "without a depth_params.json entry or with an unreliable scale gets none)")
        if n_prior == 0:
            raise ValueError(f"depths={depths!r}: no training camera received an inverse-depth prior (no PNG matches, or "
                             "every scale of depth_params.json is unreliable)")
    test_cameras = [build(r, False) for r in test]
    undistort_log = []
    if undistort:
        undistort_log = (remap or _Undistorter(device, zoom)).log_lines(lenses)
        print("\n".join(undistort_log))
    return SimpleNamespace(train_cameras=train_cameras, test_cameras=test_cameras,
                           point_cloud=pcd, cameras_extent=radius,
                           nerf_normalization={"translate": translate, "radius": radius}, undistort_log=undistort_log)
