"""Bilateral-grid colour correction: one learnable bilateral grid per training image, applied between the rasterizer
and the loss (gsplat's `use_bilateral_grid`, "Bilateral Guided Radiance Field Processing"; DESIGN.md section 3,
"Bilateral grid").  A camera's grid is float32 G[L][Hg][Wg][12], a lattice of 3x4 affine colour transforms
(coefficient 4c + k = A[c][k], the identity at every node at the start), sliced per pixel by its position and its own
luminance and regularised by a total-variation term.

The model holds the two tables [n, L, Hg, Wg, 12] and their optimizer; the slice, its gradients and the gradient of the
total-variation term are the kernels of csrc/bilagrid.hip, reached through fused.camera_forward_finish (the engines) and
clm_kernels.apply_bilagrid (the op-by-op path, evaluation), both through the one description clm_kernels.COLOUR["bilagrid"].
A camera takes part by carrying views of its rows (colour_model.ColourModel.attach); cameras.camera_colour reads them.

Optimizer: a dense torch.optim.Adam with eps 1e-15 (gsplat's).  The learning rate comes from this project's
utils.get_expon_lr_func(lr_init, lr_final, lr_delay_steps=1000, lr_delay_mult=0.01) -- a log-linear decay with a sine
warm-up, NOT gsplat's exact chain of a linear warm-up and an exponential decay -- and is not scaled by sqrt(batch size)."""
import os

import numpy as np
import torch

from . import utils
from .colour_model import ColourModel

IDENTITY = (1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0)


def tv_value(table):
    """gsplat's total variation of a table [n, L, Hg, Wg, 12], in torch (any dtype and device):
    (1/n) sum_{axis in (z, y, x)} sum (G[.. i+1 ..] - G[.. i ..])^2 / count_axis, count_axis = 12 x the number of
    differences along the axis in one camera's grid."""
    n, L, Hg, Wg, _ = table.shape
    dz, dy, dx = table[:, 1:] - table[:, :-1], table[:, :, 1:] - table[:, :, :-1], table[:, :, :, 1:] - table[:, :, :, :-1]
    return ((dz * dz).sum() / (12 * (L - 1) * Hg * Wg) + (dy * dy).sum() / (12 * L * (Hg - 1) * Wg)
            + (dx * dx).sum() / (12 * L * Hg * (Wg - 1))) / n


class BilagridModel(ColourModel):
    KIND = "bilagrid"
    FILE = "bilagrid.npz"  # grids in gsplat's [n,12,L,Hg,Wg] layout + image names

    def __init__(self, n_cameras, device, grid=(16, 16, 8), lr_init=2e-3, lr_final=2e-5, max_steps=30000, tv_weight=10.0):
        Wg, Hg, L = (int(v) for v in grid)  # gsplat's order: grid_X, grid_Y, grid_W (the guidance axis)
        if not (2 <= Wg <= 64 and 2 <= Hg <= 64 and 2 <= L <= 32):
            raise ValueError(f"bilateral grid shape (Wg, Hg, L) = {(Wg, Hg, L)}: 2 <= Wg, Hg <= 64 and 2 <= L <= 32")
        self.shape = (L, Hg, Wg)
        self.tv_weight = float(tv_weight)
        super().__init__(torch.tensor(IDENTITY, dtype=torch.float32).repeat(int(n_cameras), L, Hg, Wg, 1).to(device))
        self.optimizer = torch.optim.Adam([self.param], lr=float(lr_init), eps=1e-15)
        self.lr_func = utils.get_expon_lr_func(lr_init, lr_final, lr_delay_steps=1000, lr_delay_mult=0.01,
                                               max_steps=max_steps)

    def tv(self):
        """The total-variation value (0-dim tensor), in torch: for logging and tests only; the training step takes the
        term's gradient from clmgs_bilagrid_tv_grad."""
        return tv_value(self.param.detach())

    def tv_grad(self):
        """grad += d(tv_weight * tv)/dparam: one elementwise kernel on the current stream (no autograd graph over the
        table).  On the CPU (tests of the host side) the same expression in torch."""
        if self.tv_weight == 0.0 or self.n_cameras == 0:
            return
        if self.param.is_cuda:
            from . import _lib
            L, Hg, Wg = self.shape
            _lib.check(_lib.lib().clmgs_bilagrid_tv_grad(_lib.stream(), _lib.dptr(self.param.detach(), torch.float32),
                                                         self.n_cameras, L, Hg, Wg, self.tv_weight,
                                                         _lib.dptr(self.grad, torch.float32)))
        else:
            self.grad += tv_grad_reference(self.param.detach(), self.tv_weight)

    def before_step(self):
        """ColourModel.step: the total-variation gradient into the table, then the Adam step."""
        self.tv_grad()

    def save(self, path, cameras):
        """An .npz: `grids` float32 [n, 12, L, Hg, Wg] (gsplat's layout, a permutation of the table) and `image_names`."""
        assert len(cameras) == self.n_cameras, (len(cameras), self.n_cameras)
        grids = self.param.detach().cpu().permute(0, 4, 1, 2, 3).contiguous().numpy()
        with open(path, "wb") as f:  # a file object: numpy appends no suffix
            np.savez(f, grids=grids, image_names=np.array([str(c.image_name) for c in cameras]))

    def save_to(self, model_dir, cameras):
        self.save(os.path.join(model_dir, self.FILE), cameras)

    def load(self, path, cameras):
        """Grids of the cameras named in the file; a camera the file does not name keeps its grid."""
        assert len(cameras) == self.n_cameras, (len(cameras), self.n_cameras)
        with np.load(path, allow_pickle=False) as f:
            grids, names = f["grids"], [str(s) for s in f["image_names"]]
        L, Hg, Wg = self.shape
        if grids.dtype != np.float32 or tuple(grids.shape[1:]) != (12, L, Hg, Wg) or len(names) != grids.shape[0]:
            raise ValueError(f"{path}: grids {grids.dtype} {tuple(grids.shape)}, this model holds [n, 12, {L}, {Hg}, {Wg}] float32")
        index = {s: i for i, s in enumerate(names)}
        rows = self.param.detach().cpu()
        for i, c in enumerate(cameras):
            if c.image_name in index:
                rows[i] = torch.from_numpy(grids[index[c.image_name]]).permute(1, 2, 3, 0)
        with torch.no_grad():
            self.param.copy_(rows)


def tv_grad_reference(table, weight):
    """d(weight * tv_value(table))/dtable written out (what clmgs_bilagrid_tv_grad adds): per element and axis
    2 weight / (n count_axis) ((G - G_prev) - (G_next - G)), a missing neighbour's difference left out."""
    n, L, Hg, Wg, _ = table.shape
    out = torch.zeros_like(table)
    for dim, count in ((1, 12 * (L - 1) * Hg * Wg), (2, 12 * L * (Hg - 1) * Wg), (3, 12 * L * Hg * (Wg - 1))):
        d = table.narrow(dim, 1, table.shape[dim] - 1) - table.narrow(dim, 0, table.shape[dim] - 1)
        c = 2.0 * weight / (n * count)
        out.narrow(dim, 1, table.shape[dim] - 1).add_(d, alpha=c)
        out.narrow(dim, 0, table.shape[dim] - 1).sub_(d, alpha=c)
    return out
