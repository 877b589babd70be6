"""Learnable sky: one equirectangular environment map per scene, composited behind the splats and trained by the same
loss ("Sky").  With S = param (float32 [Hs,Ws,3], world axes, constant at the start), R the
world->camera rotation of a camera and (px, py) a pixel,

    dc = ((px + .5 - cx) / fx, (py + .5 - cy) / fy, 1),   d = R^T dc / |dc|
    u  = (atan2(d.x, d.z) / 2pi + .5) Ws - .5   (columns wrap),   v = (asin(d.y) / pi + .5) Hs - .5   (rows clamp)
    y  = x + (1 - alpha) * bilinear(S; u, v)

The model holds the map, its float gradient, the int64 fixed-point accumulator (unit 2^-48) the kernels of csrc/sky.hip
ADD into, and the optimizer; the composite and its gradients are reached through fused.camera_forward_finish (the
engines) and clm_kernels.apply_sky (the op-by-op path, evaluation).  Every camera of the scene carries the one detached
map (`camera.sky`); the cameras that train it carry the accumulator too (`camera.sky_acc`); cameras.camera_sky reads
them.  before_step() turns the accumulator into floats ONCE per optimizer step, so the cameras of a batch are summed in
integers: the gradient is the same bit for bit whatever the order they ran in."""
import os

import numpy as np
import torch

from . import utils
from .colour_model import ColourModel

CONVENTION = "equirect-world: u=(atan2(d.x,d.z)/2pi+.5)*Ws-.5 wraps, v=(asin(d.y)/pi+.5)*Hs-.5 clamps, bilinear, [Hs,Ws,3] RGB"
UNIT = 2.0 ** -48
FILE = "sky.npz"


class SkyModel(ColourModel):
    KIND = "sky"
    FILE = FILE  # the map, its shape and the convention string

    def __init__(self, shape=(256, 512), device="cuda", init=(0.5, 0.5, 0.5), lr_init=0.01, lr_final=0.001,
                 max_steps=30000):
        Hs, Ws = int(shape[0]), int(shape[1])
        if Hs < 1 or Ws < 1:
            raise ValueError(f"--sky_shape must be two positive integers, got {tuple(shape)}")
        table = torch.tensor([float(v) for v in init], dtype=torch.float32).reshape(1, 1, 3).repeat(Hs, Ws, 1).to(device)
        super().__init__(table)
        self.n_cameras = None  # one map for the scene, not a row per camera
        self.acc = torch.zeros((Hs, Ws, 3), dtype=torch.int64, device=self.param.device)
        # dense Adam over the whole map: texels no camera of the batch saw have a zero gradient
        self.optimizer = torch.optim.Adam([self.param], lr=float(lr_init))
        self.lr_func = utils.get_expon_lr_func(lr_init, lr_final, max_steps=max_steps)

    @property
    def shape(self):
        return tuple(self.param.shape[:2])

    def attach(self, cameras, train=True):
        """Every camera gets the ONE detached map; with `train` also the accumulator, else None (rendered only)."""
        table = self.param.detach()
        for c in cameras:
            c.sky = table
            c.sky_acc = self.acc if train else None

    def before_step(self):
        """grad += acc * 2^-48, acc = 0: once per optimizer step (clmgs_sky_grad_convert on the device)."""
        if self.acc.is_cuda:
            from . import _lib
            from .clm_kernels import sky_grad_convert
            sky_grad_convert(_lib.stream(), self.acc, self.grad)
        else:
            self.grad += (self.acc.to(torch.float64) * UNIT).to(torch.float32)
            self.acc.zero_()

    def zero_grad(self):
        self.grad.zero_()
        self.acc.zero_()

    def save(self, model_dir):
        path = os.path.join(model_dir, FILE)
        np.savez(path, sky=self.param.detach().cpu().numpy(), shape=np.asarray(self.shape, dtype=np.int64),
                 convention=np.asarray(CONVENTION))
        return path

    def save_to(self, model_dir, cameras):
        self.save(model_dir)

    def load(self, model_dir):
        path = os.path.join(model_dir, FILE)
        if not os.path.exists(path):
            raise FileNotFoundError(f"{path} not found: --sky needs the map a run trained with --sky wrote next to the "
                                    "point cloud")
        with np.load(path) as f:
            sky, shape, convention = f["sky"], tuple(int(v) for v in f["shape"]), str(f["convention"])
        if convention != CONVENTION:
            raise ValueError(f"{path}: convention {convention!r}, this build reads {CONVENTION!r}")
        if sky.dtype != np.float32 or sky.shape != (*shape, 3) or shape != self.shape:
            raise ValueError(f"{path}: map {sky.dtype} {sky.shape} (shape entry {shape}), the model is {self.shape}")
        with torch.no_grad():
            self.param.copy_(torch.from_numpy(sky))

    @classmethod
    def from_file(cls, model_dir, device="cuda", **kw):
        path = os.path.join(model_dir, FILE)
        if not os.path.exists(path):
            raise FileNotFoundError(f"{path} not found: --sky needs the map a run trained with --sky wrote next to the "
                                    "point cloud")
        with np.load(path) as f:
            shape = tuple(int(v) for v in f["shape"])
        m = cls(shape, device, **kw)
        m.load(model_dir)
        return m
