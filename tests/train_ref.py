"""Plain float64 restatements of the per-iteration kernels of training
(csrc/optim.hip), the yardsticks of tests/test_gpu_optim.py and
tests/test_gpu_getters.py beyond the fixtures' sizes.

adam_step        torch.optim.Adam's single-tensor update (torch/optim/adam.py
                 _single_tensor_adam, no weight decay, no amsgrad), the
                 formula quoted at the top of csrc/optim.hip.
scale_opacity    GaussianModel.get_scaling_n_opacity_with_3D_filter
                 (scene/gaussian_model.py:146-212, as gsr_scene.RawGaussians).
normalize_rows   F.normalize(x, dim=1, eps) spelled out: x / max(|x|, eps).

Every function computes in the dtype of its inputs, so the same statement run
on float32 tensors is the fp32 yardstick and on float64 tensors the exact one;
the getters are differentiable.  SSIM and depth_to_normal have their float64
restatements in oracle/ssim_ref.py.  tests/test_train_ref.py pins all three
against torch.optim.Adam, F.normalize and tests/golden/getters.npz.
"""
from __future__ import annotations

import math

import torch


def adam_step(p, g, m, v, lr, step, betas=(0.9, 0.999), eps=1e-15):
    """One Adam update at step count `step` (after increment): returns the new
    (p, m, v); the inputs are left alone."""
    beta1, beta2 = betas
    m = m + (1.0 - beta1) * (g - m)
    v = v * beta2 + (1.0 - beta2) * g * g
    bc1 = 1.0 - beta1 ** step
    bc2 = 1.0 - beta2 ** step
    denom = v.sqrt() / math.sqrt(bc2) + eps
    p = p - (lr / bc1) * (m / denom)
    return p, m, v


def scale_opacity(s, o, f):
    """(sqrt(exp(s)^2 + f^2) [P,3], sigmoid(o) sqrt(prod exp(s)^2 / prod(exp(s)^2 + f^2)) [P,1])
    for s [P,3], o [P,1], f [P,1]."""
    q = torch.exp(s).square()
    a = q + f.square()
    coef = q.prod(dim=1).sqrt() * a.prod(dim=1).rsqrt()
    return a.sqrt(), torch.sigmoid(o) * coef[:, None]


def normalize_rows(x, eps=1e-12):
    """x / max(|x|_2, eps) over dim 1 of x [n, D]."""
    # (vector_norm, not sum().sqrt(): its derivative at an exact-zero row is 0, as in F.normalize, not NaN)
    return x / torch.linalg.vector_norm(x, dim=1, keepdim=True).clamp_min(eps)
