"""MI355X drop-in for the external `fused_ssim` package the reference imports
(utils/loss_utils.py:18, `ssim()` at :48-49 calls fused_ssim(img1, img2,
padding="valid")): mean SSIM of img1 against img2 with the gradient w.r.t.
img1, computed by gsr_fused_ssim_{forward,backward} in libgsr.so
(csrc/ssim.hip).  The SSIM is that of the reference's own _ssim
(loss_utils.py:36-72).  There is no CPU fallback.
"""
from __future__ import annotations

import torch

from diff_gaussian_rasterization._abi import Out, call, dev32, stream


def _planes(img, name):
    t = dev32(img, name, "fused_ssim")
    if img.dim() < 2:
        raise RuntimeError(f"fused_ssim: `{name}` must be [..., H, W]")
    H, W = img.shape[-2:]
    return t, img.numel() // (H * W), H, W


class _FusedSSIM(torch.autograd.Function):
    @staticmethod
    def forward(ctx, img1, img2, padding, train):
        a, NC, H, W = _planes(img1, "img1")
        b, NC2, H2, W2 = _planes(img2, "img2")
        if (NC, H, W) != (NC2, H2, W2):
            raise RuntimeError("fused_ssim: img1 and img2 must have the same shape")
        valid = {"same": 0, "valid": 1}[padding]
        out = torch.empty((), dtype=torch.float32, device=a.device)
        factors = torch.empty(3 * a.numel(), dtype=torch.float32, device=a.device) if train else None
        scratch = Out(a.device, torch.uint8)
        call(a.device, "gsr_fused_ssim_forward", scratch.cb, None, NC, H, W, valid, a.data_ptr(), b.data_ptr(),
             out.data_ptr(), None if factors is None else factors.data_ptr(), stream(a.device))
        ctx.meta = (NC, H, W, valid, img1.shape)
        if train:
            ctx.save_for_backward(a, b, factors)
        return out

    @staticmethod
    def backward(ctx, grad_out):
        NC, H, W, valid, shape = ctx.meta
        if not ctx.saved_tensors:
            raise RuntimeError("fused_ssim: called with train=False, no gradient available")
        a, b, factors = ctx.saved_tensors
        g = grad_out.contiguous().to(torch.float32).reshape(1)
        dimg1 = torch.empty_like(a)
        call(a.device, "gsr_fused_ssim_backward", NC, H, W, valid, a.data_ptr(), b.data_ptr(), factors.data_ptr(),
             g.data_ptr(), dimg1.data_ptr(), stream(a.device))
        return dimg1.reshape(shape), None, None, None


def fused_ssim(img1, img2, padding="same", train=True):
    """Mean SSIM of img1 against img2 ([..., H, W] planes); differentiable in img1."""
    if padding not in ("same", "valid"):
        raise ValueError("padding must be 'same' or 'valid'")
    return _FusedSSIM.apply(img1, img2, padding, train)
