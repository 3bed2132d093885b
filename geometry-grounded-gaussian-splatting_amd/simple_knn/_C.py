"""simple_knn._C.distCUDA2 over the C ABI (gsr_knn_mean_dist, include/gsr.h).

distCUDA2(points [P, 3] float32 HIP tensor) -> [P] float32: per point the
mean of the squared distances to its 3 nearest other points
(submodules/simple-knn/spatial.cu:15-25, simple_knn.cu:175-220).
"""
from __future__ import annotations

import torch

from diff_gaussian_rasterization._abi import Out, call, ptr, stream


def distCUDA2(points):
    if not isinstance(points, torch.Tensor) or not points.is_cuda:
        raise RuntimeError("distCUDA2: `points` must be a HIP device tensor")
    if points.dtype != torch.float32:
        raise RuntimeError("distCUDA2: `points` must be float32")
    if points.ndimension() != 2 or points.size(1) != 3:
        raise RuntimeError("distCUDA2: `points` must have shape (P, 3)")
    P = points.size(0)
    pts = points.contiguous()
    means = torch.zeros(P, dtype=torch.float32, device=points.device)  # torch::full({P}, 0.0), spatial.cu:21
    if P:
        scratch = Out(points.device, torch.uint8)
        call(points.device, "gsr_knn_mean_dist", scratch.cb, None, P, ptr(pts), ptr(means), stream(points.device))
    return means
