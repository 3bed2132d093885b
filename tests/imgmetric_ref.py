"""TEST INFRASTRUCTURE ONLY — numpy restatement of the image-quality tail
(gsr_metric, csrc/imgmetric.hip): the 8-bit quantisation of torchvision's
save_image in float32 with the multiply and the add rounded separately, and
L1 / MSE / PSNR / per-image "valid" SSIM in float64 on the compared values.
tests/test_imgmetric.py pins it to the reference's own expressions
(torch_bytes, torch_psnr, torch_ssim below: utils/image_utils.py:18-20,
utils/loss_utils.py:36-72 run with torch on the CPU).
"""
from __future__ import annotations

from math import exp

import numpy as np
import torch
import torch.nn.functional as F

F32 = np.float32


def quantize_planes(x):
    """[..., H, W] float32 -> uint8 of the same shape: trunc(clamp(fl(fl(x * 255) + 0.5), 0, 255)),
    NaN -> 0 (what torch's uint8 cast of NaN gives), +inf -> 255, -inf -> 0."""
    x = np.asarray(x, F32)
    with np.errstate(invalid="ignore", over="ignore"):
        t = x * F32(255.0)  # rounded to float32
        t = t + F32(0.5)  # rounded again
        t = np.where(np.isnan(t), F32(0.0), np.clip(t, F32(0.0), F32(255.0)))
    return t.astype(np.uint8)  # truncation


def quantize8(x):
    """[C,H,W] or [N,C,H,W] float32 -> uint8 [H,W,C] or [N,H,W,C] (the PNG writer's layout)."""
    return np.ascontiguousarray(np.moveaxis(quantize_planes(x), -3, -1))


def compared(x, quantize):
    """The float32 values the metrics compare: byte / 255 in float32 (PIL + to_tensor), or clamp(x, 0, 1)."""
    x = np.asarray(x, F32)
    if quantize:
        return quantize_planes(x).astype(F32) / F32(255.0)
    return np.where(np.isnan(x), x, np.clip(x, F32(0.0), F32(1.0)))


def window2d():
    """create_window(11, ...) of loss_utils.py:36-45: the 1-D Gaussian normalised in float32 by its sum
    rounded once to float32 (what torch's CPU sum returns for these 11 values), the outer product rounded
    to float32, then widened."""
    g = np.array([exp(-((x - 5) ** 2) / float(2 * 1.5 ** 2)) for x in range(11)], dtype=F32)
    g = g / F32(g.astype(np.float64).sum())
    return (g[:, None] * g[None, :]).astype(F32).astype(np.float64)


def ssim_valid(a, b):
    """[N,C,H,W] values -> [N] float64: the mean over C (H-10) (W-10) windows of _ssim's map."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    w = window2d()

    def conv(z):
        return np.einsum("nchwij,ij->nchw", np.lib.stride_tricks.sliding_window_view(z, (11, 11), axis=(2, 3)), w)

    mu1, mu2 = conv(a), conv(b)
    mu1_sq, mu2_sq, mu1_mu2 = mu1 * mu1, mu2 * mu2, mu1 * mu2
    s1, s2, s12 = conv(a * a) - mu1_sq, conv(b * b) - mu2_sq, conv(a * b) - mu1_mu2
    C1, C2 = 0.01 ** 2, 0.03 ** 2
    m = ((2 * mu1_mu2 + C1) * (2 * s12 + C2)) / ((mu1_sq + mu2_sq + C1) * (s1 + s2 + C2))
    return m.reshape(m.shape[0], -1).mean(axis=1)


def psnr_from_mse(mse):
    mse = np.asarray(mse, np.float64)
    with np.errstate(divide="ignore"):
        return np.where(mse == 0, np.inf, -10.0 * np.log10(mse))


def metrics(render, gt, quantize=True, ssim=True):
    """render, gt [N,C,H,W] float32 -> {"L1", "MSE", "PSNR", "SSIM"}: float64 [N]."""
    render, gt = np.asarray(render, F32), np.asarray(gt, F32)
    N = render.shape[0]
    n = float(render[0].size)
    if quantize:
        d = quantize_planes(render).astype(np.int64) - quantize_planes(gt).astype(np.int64)
        d = d.reshape(N, -1)
        l1 = np.abs(d).sum(axis=1).astype(np.float64) / (255.0 * n)  # exact integers, two float64 operations
        mse = (d * d).sum(axis=1).astype(np.float64) / (65025.0 * n)
    else:
        d = (compared(render, False).astype(np.float64) - compared(gt, False).astype(np.float64)).reshape(N, -1)
        l1, mse = np.abs(d).mean(axis=1), (d * d).mean(axis=1)
    out = {"L1": l1, "MSE": mse, "PSNR": psnr_from_mse(mse)}
    if ssim:
        out["SSIM"] = ssim_valid(compared(render, quantize), compared(gt, quantize))
    return out


# ---- the reference's own expressions, with torch on the CPU --------------------------------------------------------

def torch_bytes(x):
    """torchvision.utils.save_image's bytes of a [C,H,W] tensor: [H,W,C] uint8."""
    return x.clone().mul(255).add_(0.5).clamp_(0, 255).permute(1, 2, 0).to(torch.uint8)


def torch_psnr(img1, img2):
    """utils/image_utils.py:18-20 on [N,C,H,W] tensors -> [N] (in the tensors' dtype)."""
    mse = (((img1 - img2)) ** 2).view(img1.shape[0], -1).mean(1, keepdim=True)
    return (20 * torch.log10(1.0 / torch.sqrt(mse)))[:, 0]


def torch_l1(img1, img2):
    """l1_loss of loss_utils.py:28-29 per image."""
    return torch.abs(img1 - img2).view(img1.shape[0], -1).mean(1)


def torch_window(channel):
    """gaussian(11, 1.5) and create_window of loss_utils.py:36-45: float32 throughout."""
    g = torch.Tensor([exp(-((x - 5) ** 2) / float(2 * 1.5 ** 2)) for x in range(11)])
    g = (g / g.sum()).unsqueeze(1)
    return g.mm(g.t()).float()[None, None].expand(channel, 1, 11, 11).contiguous()


def torch_ssim(img1, img2):
    """_ssim of loss_utils.py:52-72 with padding=0, per image: [N,C,H,W] tensors -> [N], evaluated in
    the tensors' dtype (the float32 window widened for float64)."""
    C = img1.shape[1]
    w = torch_window(C).to(img1.dtype)

    def conv(z):
        return F.conv2d(z, w, padding=0, groups=C)

    mu1, mu2 = conv(img1), conv(img2)
    mu1_sq, mu2_sq, mu12 = mu1.pow(2), mu2.pow(2), mu1 * mu2
    s1, s2, s12 = conv(img1 * img1) - mu1_sq, conv(img2 * img2) - mu2_sq, conv(img1 * img2) - mu12
    C1, C2 = 0.01 ** 2, 0.03 ** 2
    m = ((2 * mu12 + C1) * (2 * s12 + C2)) / ((mu1_sq + mu2_sq + C1) * (s1 + s2 + C2))
    return m.mean(1).mean(1).mean(1)


def pair(shape, seed, spread=0.0):
    """A correlated image pair like a render and its target, float32 numpy [N,C,H,W]; `spread` > 0 pushes
    values outside [0, 1] so that the clamps matter."""
    g = torch.Generator().manual_seed(seed)
    a = torch.rand(shape, generator=g) * (1.0 + 2.0 * spread) - spread
    b = a + 0.1 * torch.randn(shape, generator=g)
    if spread == 0.0:
        b = b.clamp(0, 1)
    return a.numpy(), b.numpy()


def edge_image():
    """[1,3,32,32] float32 (3072 values) holding, for every k in 0..255, k / 255 and the byte boundary
    (k - 0.5) / 255, each with its float32 neighbours at +-1 and +-2 ulp; then -0.0, a denormal, -1, 2,
    1 + 1 ulp, NaN and +-inf; the rest uniform in [0, 1)."""
    vals = []
    for k in range(256):
        for c in (F32(k) / F32(255.0), F32((k - 0.5) / 255.0)):
            lo1, hi1 = np.nextafter(c, F32(-np.inf)), np.nextafter(c, F32(np.inf))
            vals += [c, lo1, hi1, np.nextafter(lo1, F32(-np.inf)), np.nextafter(hi1, F32(np.inf))]
    vals += [F32(-0.0), F32(1e-41), F32(-1.0), F32(2.0), np.nextafter(F32(1.0), F32(2.0)), F32(np.nan), F32(np.inf),
             F32(-np.inf)]
    vals = np.array(vals, dtype=F32)
    rest = np.random.default_rng(0).random(3072 - vals.size, dtype=F32)
    flat = np.concatenate([vals, rest])
    return flat[np.random.default_rng(1).permutation(3072)].reshape(1, 3, 32, 32)
