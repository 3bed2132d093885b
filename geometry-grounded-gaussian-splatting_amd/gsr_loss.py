"""The photometric term of the training loss as the reference's geometry
pipelines compute it, on one fused HIP kernel each way (csrc/photoloss.hip,
gsr_photo_loss_{forward,backward} in libgsr.so).

rgb_loss — train.py:159-169 and :189 in one call: the ground truth composited
    over the background outside `mask > 0.5`, the L1 of the rendered image
    after the per-view appearance transform, and the D-SSIM of the raw
    rendered image against the composite.
L1_loss_appearance — utils/loss_utils.py:90-123 with the reference's
    signature, through the kernel's L1-only switch (for GOF the crop, the
    downsample and the network stay in torch; the kernel takes their gain).
AppearanceNetwork — scene/appearance_network.py restated (torch modules; the
    reference's state_dict loads).

There is no CPU fallback.
"""
from __future__ import annotations

import enum

import torch
import torch.nn as nn
import torch.nn.functional as F

from diff_gaussian_rasterization._abi import Out, call, dev32, ptr, stream


class AppModel(enum.Enum):
    """GaussianModel.App_model's members (the kernel's 'gain' mode is its half of GOF)."""

    NO = "no"
    GS = "gs"
    PGSR = "pgsr"
    GOF = "gof"


_MODES = {"no": 0, "gs": 1, "pgsr": 2, "gain": 3}
_EMB_SHAPE = {1: (3, 4), 2: (2,)}


def app_model_name(app_model) -> str:
    """'no' | 'gs' | 'pgsr' | 'gof' for a name, an AppModel, the reference's
    enum member (by its name) or its integer (arguments: 0 NO, 1 GS, 2 GOF, 3 PGSR)."""
    if isinstance(app_model, str):
        name = app_model.lower()
    elif isinstance(app_model, int):
        name = ("no", "gs", "gof", "pgsr")[app_model]
    else:
        name = str(getattr(app_model, "name", app_model)).lower()
    if name not in ("no", "gs", "pgsr", "gof"):
        raise ValueError(f"Unsupported appearance model: {app_model}")
    return name


def _image(img, name):
    """[3,H,W] or [1,3,H,W], any strides (as fused_ssim._planes)."""
    t = dev32(img, name, "rgb_loss")
    if t.dim() < 3 or t.shape[-3] != 3 or t.numel() != 3 * t.shape[-2] * t.shape[-1]:
        raise RuntimeError(f"rgb_loss: `{name}` must be [3, H, W]")
    return t, t.shape[-2], t.shape[-1]


class _PhotoLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, image, embedding, gain, gt, mask, bg, mode, crop, lam, with_ssim):
        a, H, W = _image(image, "image")
        b, H2, W2 = _image(gt, "gt_image")
        if (H, W) != (H2, W2):
            raise RuntimeError("rgb_loss: image and gt_image must have the same shape")
        m = None if mask is None else dev32(mask, "mask", "rgb_loss")
        if m is not None and m.numel() != H * W:
            raise RuntimeError("rgb_loss: `mask` must be [H, W]")
        c = None if bg is None else dev32(bg, "bg", "rgb_loss")
        if c is not None and c.numel() != 3:
            raise RuntimeError("rgb_loss: `bg` must have 3 values")
        e = None if embedding is None else dev32(embedding, "embedding", "rgb_loss")
        if mode in _EMB_SHAPE and e is not None and tuple(e.shape) != _EMB_SHAPE[mode]:
            raise RuntimeError(f"rgb_loss: `embedding` must be {list(_EMB_SHAPE[mode])}")
        g = None if gain is None else dev32(gain, "gain", "rgb_loss")
        top, left, Hc, Wc = crop
        if mode == 3 and g is not None and g.numel() != 3 * Hc * Wc:
            raise RuntimeError("rgb_loss: `gain` must be [3, crop_h, crop_w]")
        train = any(ctx.needs_input_grad[:3])
        dev = a.device
        out = torch.empty(3, dtype=torch.float32, device=dev)
        factors = torch.empty(9 * H * W, dtype=torch.float32, device=dev) if train and with_ssim else None
        sums = torch.empty(12, dtype=torch.float32, device=dev) if train and mode in _EMB_SHAPE else None
        scratch = Out(dev, torch.uint8)
        call(dev, "gsr_photo_loss_forward", scratch.cb, None, H, W, mode, int(with_ssim), lam, a.data_ptr(),
             b.data_ptr(), ptr(m), ptr(c), ptr(e), ptr(g), top, left, Hc, Wc, out.data_ptr(), None, ptr(factors),
             ptr(sums), stream(dev))
        ctx.meta = (H, W, mode, crop, lam, with_ssim, image.shape, train)
        ctx.save_for_backward(a, b, m, c, e, g, factors, sums)
        loss, l1, ssim = out[0], out[1], out[2]
        ctx.mark_non_differentiable(l1, ssim)
        return loss, l1, ssim

    @staticmethod
    def backward(ctx, grad_loss, _g1, _g2):
        H, W, mode, crop, lam, with_ssim, shape, train = ctx.meta
        if not train:
            raise RuntimeError("rgb_loss: no gradient was asked for in the forward")
        a, b, m, c, e, g, factors, sums = ctx.saved_tensors
        up = grad_loss.contiguous().to(torch.float32).reshape(1)
        dimg = torch.empty_like(a)
        demb = torch.empty_like(e) if mode in _EMB_SHAPE else None
        dgain = torch.empty_like(g) if mode == 3 else None
        top, left, Hc, Wc = crop
        call(a.device, "gsr_photo_loss_backward", H, W, mode, int(with_ssim), lam, a.data_ptr(), b.data_ptr(), ptr(m),
             ptr(c), ptr(e), ptr(g), top, left, Hc, Wc, ptr(factors), ptr(sums), up.data_ptr(), dimg.data_ptr(),
             ptr(demb), ptr(dgain), stream(a.device))
        return dimg.reshape(shape), demb, dgain, None, None, None, None, None, None, None


def _call(image, gt_image, mask, bg, app_model, embedding, gain, crop, lam, with_ssim):
    if isinstance(app_model, int):  # (a gsr_app_model value as it is: the library refuses an unknown one)
        mode = app_model
    elif app_model in _MODES:
        mode = _MODES[app_model]
    else:
        raise ValueError("app_model must be 'no', 'gs', 'pgsr' or 'gain'")
    if mode == 3 and crop is None and gain is not None:
        crop = (0, 0, gain.shape[-2], gain.shape[-1])
    crop = (0, 0, 0, 0) if crop is None else tuple(int(v) for v in crop)
    return _PhotoLoss.apply(image, embedding if mode in _EMB_SHAPE else None, gain if mode == 3 else None, gt_image,
                            mask, bg, mode, crop, float(lam), with_ssim)


def rgb_loss(image, gt_image, *, mask=None, bg=None, app_model="no", embedding=None, gain=None, crop=None,
             lambda_dssim=0.2):
    """(loss, l1, ssim) with loss = (1 - lambda_dssim) l1 + lambda_dssim (1 - ssim).

    image, gt_image: [3,H,W] (any strides).  mask [H,W] (or [1,H,W]): the ground
    truth is `bg` (3 values, black when None) where `mask > 0.5` fails.
    app_model: 'no'; 'gs' (embedding [3,4]); 'pgsr' (embedding [2]); 'gain'
    (gain [3,Hc,Wc] over crop = (top, left, Hc, Wc), the L1 over the crop).
    `loss` is differentiable in image, embedding and gain; l1 and ssim are the
    terms' values for logging (not differentiable)."""
    return _call(image, gt_image, mask, bg, app_model, embedding, gain, crop, lambda_dssim, True)


def l1_loss(image, gt_image, *, mask=None, bg=None, app_model="no", embedding=None, gain=None, crop=None):
    """The L1 of rgb_loss alone (the kernel's L1-only switch: no stencil, any H, W >= 1); differentiable."""
    return _call(image, gt_image, mask, bg, app_model, embedding, gain, crop, 0.0, False)[0]


class _UpsampleBlock(nn.Module):
    """PixelShuffle(2), a 3x3 convolution and a ReLU."""

    def __init__(self, n_in, n_out):
        super().__init__()
        self.pixel_shuffle = nn.PixelShuffle(2)
        self.conv = nn.Conv2d(n_in // 4, n_out, 3, stride=1, padding=1)
        self.relu = nn.ReLU()

    def forward(self, x):
        return self.relu(self.conv(self.pixel_shuffle(x)))


class AppearanceNetwork(nn.Module):
    """The GOF appearance CNN: conv1 to 256 channels, four pixel-shuffle
    upsampling blocks (128, 64, 32, 16), a bilinear x2, conv2, conv3 and a
    sigmoid: a [1, n_in, h, w] input gives a [1, n_out, 32 h, 32 w] gain."""

    def __init__(self, num_input_channels, num_output_channels):
        super().__init__()
        self.conv1 = nn.Conv2d(num_input_channels, 256, 3, stride=1, padding=1)
        widths = (256, 128, 64, 32, 16)
        for k in range(4):
            setattr(self, f"up{k + 1}", _UpsampleBlock(widths[k], widths[k + 1]))
        self.conv2 = nn.Conv2d(16, 16, 3, stride=1, padding=1)
        self.conv3 = nn.Conv2d(16, num_output_channels, 3, stride=1, padding=1)
        self.relu = nn.ReLU()
        self.sigmoid = nn.Sigmoid()

    def forward(self, x):
        x = self.relu(self.conv1(x))
        for k in range(4):
            x = getattr(self, f"up{k + 1}")(x)
        x = F.interpolate(x, scale_factor=2, mode="bilinear", align_corners=True)
        return self.sigmoid(self.conv3(self.relu(self.conv2(x))))


def gof_gain(image, embedding, network):
    """(gain [3,Hc,Wc], (top, left, Hc, Wc)) of loss_utils.py:105-117: the
    centre crop to multiples of 32, its bilinear align_corners downsample by
    32, the embedding broadcast over that grid, and the network."""
    H0, W0 = image.shape[-2:]
    Hc, Wc = H0 // 32 * 32, W0 // 32 * 32
    top, left = (H0 - Hc) // 2, (W0 - Wc) // 2
    crop = image.reshape(3, H0, W0)[:, top:top + Hc, left:left + Wc]
    down = F.interpolate(crop[None], size=(Hc // 32, Wc // 32), mode="bilinear", align_corners=True)[0]
    emb_map = embedding[:, None, None].expand(-1, Hc // 32, Wc // 32)
    gain = network(torch.cat([down, emb_map], dim=0)[None])[0]
    return gain, (top, left, Hc, Wc)


def L1_loss_appearance(image, gt_image, gaussians, view_idx):
    """utils/loss_utils.py:90-123 on the kernel: the L1 of `image` against
    `gt_image` after the appearance model of `gaussians` for view `view_idx`."""
    name = app_model_name(gaussians.app_model)
    if name == "no":
        return l1_loss(image, gt_image)
    emb = gaussians.get_apperance_embedding(view_idx)
    if name == "gof":
        gain, crop = gof_gain(image, emb, gaussians.appearance_network)
        return l1_loss(image, gt_image, app_model="gain", gain=gain, crop=crop)
    return l1_loss(image, gt_image, app_model=name, embedding=emb)
