"""TEST INFRASTRUCTURE ONLY — the photometric loss of the reference's training
iteration in plain torch, at the dtype of its inputs (fp32 or float64): the
ground-truth composite of train.py:159-166, the four appearance transforms of
utils/loss_utils.py:90-123 (GOF as a given gain plane over its crop), the L1,
and the SSIM of oracle/ssim_ref.py as it is.  Gradients come from autograd.
The checker of csrc/photoloss.hip (gsr_loss.rgb_loss)."""
from __future__ import annotations

import torch
import torch.nn.functional as F

from oracle import ssim_ref


def composite(gt, mask=None, bg=None):
    """gt [3,H,W]; mask [H,W]: gt where mask > 0.5 (strict), bg [3] elsewhere."""
    if mask is None:
        return gt
    m = (mask.reshape(gt.shape[-2:]) > 0.5).to(gt.dtype)[None]
    b = torch.zeros(3, dtype=gt.dtype, device=gt.device) if bg is None else bg.to(gt.dtype)
    return gt * m + b.view(3, 1, 1) * (1 - m)


def transform(image, app_model="no", embedding=None, gain=None, crop=None):
    """(t, region): the transformed image over the region the L1 covers, and
    that region (top, left, Hc, Wc)."""
    H, W = image.shape[-2:]
    if app_model == "no":
        return image, (0, 0, H, W)
    if app_model == "gs":
        t = torch.addmm(embedding[:3, 3, None], embedding[:3, :3], image.reshape(3, -1))
        return t.reshape(image.shape), (0, 0, H, W)
    if app_model == "pgsr":
        return torch.addcmul(embedding[1], torch.exp(embedding[0]), image), (0, 0, H, W)
    if app_model == "gain":
        top, left, Hc, Wc = crop
        return gain * image[:, top:top + Hc, left:left + Wc], crop
    raise ValueError(app_model)


def l1_terms(image, gt, *, mask=None, bg=None, app_model="no", embedding=None, gain=None, crop=None):
    """t - g over the L1's region."""
    g = composite(gt, mask, bg)
    t, (top, left, Hc, Wc) = transform(image, app_model, embedding, gain, crop)
    return t - g[:, top:top + Hc, left:left + Wc]


def rgb_loss(image, gt, *, mask=None, bg=None, app_model="no", embedding=None, gain=None, crop=None,
             lambda_dssim=0.2, with_ssim=True):
    """(loss, l1, ssim) of [3,H,W] images."""
    l1 = l1_terms(image, gt, mask=mask, bg=bg, app_model=app_model, embedding=embedding, gain=gain,
                  crop=crop).abs().mean()
    if not with_ssim:
        return l1, l1, torch.zeros_like(l1)
    s = ssim_ref.ssim(image[None], composite(gt, mask, bg)[None], padding="valid")
    return (1.0 - lambda_dssim) * l1 + lambda_dssim * (1.0 - s), l1, s


def gof_gain(image, embedding, network):
    """loss_utils.py:105-117: (gain, crop) of the centre crop to multiples of 32."""
    H0, W0 = image.shape[-2:]
    Hc, Wc = H0 // 32 * 32, W0 // 32 * 32
    top, left = (H0 - Hc) // 2, (W0 - Wc) // 2
    c = image[:, top:top + Hc, left:left + Wc]
    down = F.interpolate(c[None], size=(Hc // 32, Wc // 32), mode="bilinear", align_corners=True)[0]
    emb = embedding[None].repeat(Hc // 32, Wc // 32, 1).permute(2, 0, 1)
    return network(torch.cat([down, emb], dim=0)[None])[0], (top, left, Hc, Wc)
