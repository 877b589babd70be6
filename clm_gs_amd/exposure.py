"""Per-camera exposure compensation: one learnable 3x4 affine colour transform per training image, applied between
the rasterizer and the loss (the INRIA 3DGS code base's `--exposure_lr_init` / `exposure.json`; DESIGN.md section 3,
"Exposure").  With E = param[i] (float32 [3,4], identity at the start) and x the rendered pixel,

    y[c] = x[0] E[0][c] + x[1] E[1][c] + x[2] E[2][c] + E[c][3]

The model holds the two tables and their optimizer; the transform and its gradients are the kernels of
csrc/exposure.hip, reached through fused.camera_forward_finish (the engines) and clm_kernels.apply_exposure (the
op-by-op path, evaluation), both through the one description clm_kernels.COLOUR["exposure"].  A camera takes part by
carrying views of its rows (colour_model.ColourModel.attach); cameras.camera_colour reads them."""
import json
import os

import torch

from . import utils
from .colour_model import ColourModel


class ExposureModel(ColourModel):
    KIND = "exposure"
    FILE = "exposure.json"  # {image_name: 3x4}, the INRIA code base's exposure.json

    def __init__(self, n_cameras, device, lr_init=0.01, lr_final=0.001, lr_delay_steps=0, lr_delay_mult=0.0,
                 max_steps=30000):
        super().__init__(torch.eye(3, 4, dtype=torch.float32).repeat(int(n_cameras), 1, 1).to(device))
        # dense Adam over the whole table, torch's default eps: rows of cameras outside the batch see a zero gradient
        # (their moments decay and keep moving them), as in the INRIA code base
        self.optimizer = torch.optim.Adam([self.param], lr=float(lr_init))
        self.lr_func = utils.get_expon_lr_func(lr_init, lr_final, lr_delay_steps=lr_delay_steps,
                                               lr_delay_mult=lr_delay_mult, max_steps=max_steps)

    def save_json(self, path, cameras):
        """{image_name: 3x4 list}.  A float32 survives the trip through its shortest decimal form exactly."""
        assert len(cameras) == self.n_cameras, (len(cameras), self.n_cameras)
        rows = self.param.detach().cpu().tolist()
        with open(path, "w") as f:
            json.dump({c.image_name: rows[i] for i, c in enumerate(cameras)}, f, indent=2)

    def save_to(self, model_dir, cameras):
        self.save_json(os.path.join(model_dir, self.FILE), cameras)

    def load_json(self, path, cameras):
        """Rows of the cameras named in the file; a camera the file does not name keeps its row."""
        assert len(cameras) == self.n_cameras, (len(cameras), self.n_cameras)
        with open(path) as f:
            table = json.load(f)
        rows = self.param.detach().cpu()
        for i, c in enumerate(cameras):
            if c.image_name in table:
                row = torch.tensor(table[c.image_name], dtype=torch.float64)
                if tuple(row.shape) != (3, 4):
                    raise ValueError(f"{path}: {c.image_name} is {tuple(row.shape)}, not 3x4")
                rows[i] = row.to(torch.float32)
        with torch.no_grad():
            self.param.copy_(rows)
