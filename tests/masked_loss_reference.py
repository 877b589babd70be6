"""The masked training loss in float64 torch, stated from its definition ("Masked loss"):

    m_p in {0, 1} per pixel (uint8 mask, non-zero = counted), gt = clamp(u8 / 255), n = 3 H W
    loss = (1 - lambda) * sum_{c,p} m_p |x - gt| / n  +  lambda * sum_{c,p} m_p (1 - ssim_map) / n

ssim_map is the SSIM map of the WHOLE, unmasked images: 11 x 11 Gaussian window (sigma 1.5), zero padding,
C1 = 0.01^2, C2 = 0.03^2.  The window is built the way the original implementation builds it -- the 1-D taps
normalised in float32, their outer product taken in float32 -- and only then widened to the images' dtype, so in
float64 the taps are float32 values (tests/golden/masked_loss.npz was produced with such a window)."""
import math

import torch
import torch.nn.functional as F

C1, C2 = 0.01 ** 2, 0.03 ** 2


def window(dtype=torch.float64):
    taps = torch.tensor([math.exp(-((i - 5) ** 2) / (2.0 * 1.5 ** 2)) for i in range(11)], dtype=torch.float32)
    taps = taps / taps.sum()
    return (taps[:, None] * taps[None, :]).to(dtype)


def gt_from_u8(gt_u8, dtype=torch.float64):
    return torch.clamp(gt_u8.to(dtype) / 255.0, 0.0, 1.0)


def ssim_map(x, y):
    """[3,H,W] x [3,H,W] -> [3,H,W], statistics over the whole images."""
    ch = x.shape[0]
    w = window(x.dtype)[None, None].expand(ch, 1, 11, 11).contiguous()
    blur = lambda t: F.conv2d(t[None], w, padding=5, groups=ch)[0]
    mx, my = blur(x), blur(y)
    vx, vy, cxy = blur(x * x) - mx * mx, blur(y * y) - my * my, blur(x * y) - mx * my
    return ((2 * mx * my + C1) * (2 * cxy + C2)) / ((mx * mx + my * my + C1) * (vx + vy + C2))


def counted(mask):
    """uint8 / bool [H,W] -> bool [H,W]."""
    return mask != 0


def masked_l1_map(x, gt_u8, mask):
    return (x - gt_from_u8(gt_u8, x.dtype)).abs() * counted(mask).to(x.dtype)[None]


def masked_ssim_map(x, gt_u8, mask):
    return ssim_map(x, gt_from_u8(gt_u8, x.dtype)) * counted(mask).to(x.dtype)[None]


def masked_loss(x, gt_u8, mask, lambda_dssim=0.2):
    """x [3,H,W] (float64 for a reference value), gt_u8 uint8 [3,H,W], mask [H,W] or None (every pixel counted)."""
    _, H, W = x.shape
    if mask is None:
        mask = torch.ones((H, W), dtype=torch.uint8)
    m = counted(mask).to(x.dtype)[None]
    y = gt_from_u8(gt_u8, x.dtype)
    n = float(3 * H * W)
    l1 = ((x - y).abs() * m).sum() / n
    ds = ((1.0 - ssim_map(x, y)) * m).sum() / n
    return (1.0 - lambda_dssim) * l1 + lambda_dssim * ds


def masked_eval_metrics(img, gt_u8, mask):
    """L1 and PSNR over the counted pixels of a clamped render (trainer.evaluate): sums divided by 3 * count."""
    img = img.double().clamp(0.0, 1.0)
    y = gt_from_u8(gt_u8)
    m = counted(mask).double()[None]
    k = 3.0 * float(counted(mask).sum())
    l1 = float(((img - y).abs() * m).sum() / k)
    mse = float((((img - y) ** 2) * m).sum() / k)
    return l1, 20.0 * math.log10(1.0 / math.sqrt(mse))


def far_from_counted(mask, radius=5):
    """bool [H,W]: pixels farther than `radius` (Chebyshev) from every counted pixel."""
    m = counted(mask).double()[None, None]
    near = F.max_pool2d(m, 2 * radius + 1, stride=1, padding=radius)[0, 0] > 0
    return ~near
