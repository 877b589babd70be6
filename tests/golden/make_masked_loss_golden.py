"""Generates tests/golden/masked_loss.npz by IMPORTING the reference's own masked pixelwise losses from
/root/reference (build container only; the reference never travels to the GPU box).

    python tests/golden/make_masked_loss_golden.py

The fixture is data only: a seeded 3x24x40 image, ground truth and mask, the two pixelwise maps the reference's
utils/loss_utils.py (pixelwise_l1_with_mask, pixelwise_ssim_with_mask) produced for them in float64, the masked loss

    (1 - lambda) * sum(l1_map) / n + lambda * sum(mask - ssim_map) / n,   n = 3 H W, lambda = 0.2

formed from those maps, and its gradient by autograd through the reference's functions.
"""
import os
import sys

import numpy as np
import torch

REF = "/root/reference"
OUT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, REF)

from utils import loss_utils as lu  # noqa: E402

LAMBDA = 0.2


def main():
    g = torch.Generator().manual_seed(20261018)
    H, W = 24, 40
    img = torch.rand(3, H, W, generator=g)
    gt = (torch.rand(3, H, W, generator=g) * 255).to(torch.uint8)
    mask = torch.zeros(H, W, dtype=torch.uint8)
    mask[3:17, 6:29] = 255                                    # a block ...
    mask[19:, 30:] = (torch.rand(H - 19, W - 30, generator=g) < 0.5).to(torch.uint8)  # ... and a speckled corner
    mask[0, 0] = 1
    x = img.double().requires_grad_()
    y = torch.clamp(gt.double() / 255.0, 0.0, 1.0)
    m = mask != 0
    l1_map = lu.pixelwise_l1_with_mask(x, y, m)
    ssim_map = lu.pixelwise_ssim_with_mask(x, y, m)
    n = float(3 * H * W)
    loss = (1.0 - LAMBDA) * l1_map.sum() / n + LAMBDA * (3.0 * float(m.sum()) - ssim_map.sum()) / n
    loss.backward()
    path = os.path.join(OUT, "masked_loss.npz")
    np.savez(path, img=img.numpy(), gt=gt.numpy(), mask=mask.numpy(), l1_map=l1_map.detach().numpy(),
             ssim_map=ssim_map.detach().numpy(), loss=np.float64(loss.item()), grad=x.grad.numpy(),
             lambda_dssim=np.float64(LAMBDA))
    print("written", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
