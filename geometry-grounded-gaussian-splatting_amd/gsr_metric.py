"""Image-quality evaluation on the device (the reference's render.py and
metric.py, and the test report of train.py:332-365) over the C ABI:
8-bit quantisation, L1, PSNR and per-image SSIM in HIP (gsr_image_quantize8,
gsr_image_metrics; csrc/imgmetric.hip).

    per_view = render_set(out_dir, views, pc, pipe, background, kernel_size)   # renders/ and gt/ PNG pairs
    results = evaluate(model_path)                                             # results.json, per_view.json
    l1, psnr = report(views, pc, pipe, background, kernel_size)                # the in-training report

metric.py does not score the float render: it scores what survives
torchvision's save_image -> PNG -> to_tensor, trunc(clamp(x * 255 + 0.5, 0,
255)) / 255 with the multiply and the add rounded separately in fp32.  The
quantised mode applies that rule on the device, so the numbers render_set
returns are the numbers evaluate reads back from the PNG files.  LPIPS is not
computed here (its VGG weights are fetched by URL); evaluate takes a callable.

Device tensors on the current stream; there is no CPU path.
"""
from __future__ import annotations

import json
import os

import numpy as np
import torch

from diff_gaussian_rasterization._abi import Out, call, ptr, require, stream


def _batched(t, name, who, dtypes=(torch.float32,)):
    """`t` as a contiguous [N,C,H,W] tensor and whether it came as [C,H,W]."""
    if isinstance(t, torch.Tensor) and t.dim() == 3:
        require(t, name, dtypes, 3, who)
        return t.unsqueeze(0).contiguous(), True
    require(t, name, dtypes, 4, who)
    return t.contiguous(), False


@torch.no_grad()
def quantize8(image):
    """image [C,H,W] or [N,C,H,W] float32 -> uint8 [H,W,C] or [N,H,W,C]: the bytes
    torchvision.utils.save_image writes, x.mul(255).add_(0.5).clamp_(0, 255).to(uint8) permuted
    to channels last (NaN and -inf give 0, +inf 255)."""
    x, single = _batched(image, "image", "quantize8")
    N, C, H, W = x.shape
    if min(C, H, W) < 1:
        raise RuntimeError(f"quantize8: `image` must have C, H, W >= 1 (got {tuple(image.shape)})")
    out = torch.empty((N, H, W, C), dtype=torch.uint8, device=x.device)
    call(x.device, "gsr_image_quantize8", N, C, H, W, ptr(x), ptr(out), stream(x.device))
    return out[0] if single else out


def psnr_from_mse(mse):
    """-10 log10(mse) in float64, inf for mse == 0 (utils/image_utils.py:18-20 gives the same:
    20 log10(1 / sqrt(0)))."""
    mse = torch.as_tensor(mse, dtype=torch.float64)
    return torch.where(mse == 0, torch.full_like(mse, float("inf")), -10.0 * torch.log10(mse))


@torch.no_grad()
def image_metrics(render, gt, quantize=True, ssim=True, return_bytes=False):
    """L1, PSNR and SSIM of each image of `render` against `gt` ([C,H,W] or [N,C,H,W] float32, equal
    shapes) -> {"L1", "MSE", "PSNR", "SSIM"}: float64 CPU tensors [N] ("SSIM" only when asked for; PSNR =
    -10 log10(MSE), formed on the host).

    quantize=True scores what metric.py reads back from the PNG pair (both images through quantize8,
    compared as byte / 255 in float32; the sums are exact integers); quantize=False scores the images
    clamped to [0, 1] (train.py:338-339).  SSIM is the mean of the reference's SSIM map over the windows
    inside the image (padding="valid"), per image; it needs H, W >= 11.  With return_bytes (quantised
    mode) the result is (metrics, render_bytes, gt_bytes), uint8 [N,H,W,C] from the same read."""
    who = "image_metrics"
    a, _ = _batched(render, "render", who)
    b, _ = _batched(gt, "gt", who)
    if a.shape != b.shape:
        raise RuntimeError(f"{who}: `render` and `gt` must have the same shape (got {tuple(render.shape)} "
                           f"and {tuple(gt.shape)})")
    if a.device != b.device:
        raise RuntimeError(f"{who}: `render` and `gt` must be on one device")
    N, C, H, W = a.shape
    if min(C, H, W) < 1:
        raise RuntimeError(f"{who}: `render` must have C, H, W >= 1 (got {tuple(render.shape)})")
    if ssim and (H < 11 or W < 11):
        raise RuntimeError(f"{who}: `render` is {H} x {W}; SSIM needs H and W of at least 11 (ssim=False scores "
                           "L1 and PSNR alone)")
    if return_bytes and not quantize:
        raise RuntimeError(f"{who}: return_bytes needs quantize=True")
    if return_bytes and C > 4:
        raise RuntimeError(f"{who}: return_bytes needs `render` of at most 4 channels (got {C})")
    dev = a.device
    out = torch.zeros((N, 3), dtype=torch.float64, device=dev)
    qa = torch.empty((N, H, W, C), dtype=torch.uint8, device=dev) if return_bytes else None
    qb = torch.empty_like(qa) if return_bytes else None
    scratch = Out(dev, torch.uint8)
    call(dev, "gsr_image_metrics", scratch.cb, None, N, C, H, W, int(bool(quantize)), int(bool(ssim)), ptr(a), ptr(b),
         ptr(qa), ptr(qb), ptr(out), stream(dev))
    host = out.cpu()  # the one device-to-host copy
    res = {"L1": host[:, 0].clone(), "MSE": host[:, 1].clone(), "PSNR": psnr_from_mse(host[:, 1])}
    if ssim:
        res["SSIM"] = host[:, 2].clone()
    return (res, qa, qb) if return_bytes else res


def _save_png(path, hwc):
    from PIL import Image

    arr = hwc.cpu().numpy()
    Image.fromarray(arr[..., 0] if arr.shape[-1] == 1 else arr).save(path)


@torch.no_grad()
def render_set(out_dir, views, pc, pipe, background, kernel_size):
    """render.py:24-35: every view rendered and scored against view.original_image[0:3] in quantised mode;
    with `out_dir` the byte images of that same call go to out_dir/renders/00000.png and out_dir/gt/00000.png
    (the reference's model_path/<name>/ours_<iteration>).  -> {"L1", "PSNR", "SSIM"}: float64 [len(views)]."""
    from gaussian_renderer import render

    if out_dir is not None:
        for sub in ("renders", "gt"):
            os.makedirs(os.path.join(out_dir, sub), exist_ok=True)
    rows = []
    for idx, view in enumerate(views):
        rendering = render(view, pc, pipe, background, kernel_size=kernel_size)["render"]
        gt = view.original_image[0:3, :, :]
        if out_dir is None:
            rows.append(image_metrics(rendering, gt))
            continue
        m, qa, qb = image_metrics(rendering, gt, return_bytes=True)
        rows.append(m)
        _save_png(os.path.join(out_dir, "renders", "{0:05d}".format(idx) + ".png"), qa[0])
        _save_png(os.path.join(out_dir, "gt", "{0:05d}".format(idx) + ".png"), qb[0])
    return {k: torch.cat([r[k] for r in rows]) if rows else torch.zeros(0, dtype=torch.float64)
            for k in ("L1", "PSNR", "SSIM")}


def _read_png(path):
    """tf.to_tensor(Image.open(path))[:3]: [C,H,W] float32 byte / 255 (divided in float32 on the host)."""
    from PIL import Image

    arr = np.asarray(Image.open(path))
    if arr.dtype != np.uint8:
        raise RuntimeError(f"evaluate: {path} is not an 8-bit image")
    if arr.ndim == 2:
        arr = arr[:, :, None]
    return torch.from_numpy((arr.astype(np.float32) / np.float32(255.0)).transpose(2, 0, 1)[:3].copy())


def _score_pair(render, gt, device):
    """One PNG pair in quantised mode (the entry evaluate() scores through)."""
    m = image_metrics(render.to(device), gt.to(device))
    return float(m["SSIM"][0]), float(m["PSNR"][0])


def evaluate(model_path, lpips_fn=None, device="cuda", score_fn=None):
    """metric.py:36-91 for one model directory: for every model_path/test/<method>/{renders,gt} the PNG
    pairs are read, cut to their first three channels and scored in quantised mode (quantising byte / 255
    gives the byte back, so the compared values are the file's).  Writes model_path/results.json
    ({method: {"SSIM", "PSNR"}}, plain means over the views) and model_path/per_view.json
    ({method: {"SSIM": {name: v}, "PSNR": {name: v}}}) and returns the two dicts.  A "LPIPS" entry appears
    only with `lpips_fn(render, gt) -> float` ([1,3,H,W] tensors on `device`).  `score_fn(render, gt) ->
    (ssim, psnr)` on [3,H,W] CPU tensors replaces the device call (tests)."""
    score = score_fn or (lambda r, g: _score_pair(r, g, device))
    full, per_view = {}, {}
    test_dir = os.path.join(model_path, "test")
    for method in sorted(os.listdir(test_dir)):
        renders_dir, gt_dir = os.path.join(test_dir, method, "renders"), os.path.join(test_dir, method, "gt")
        names = sorted(os.listdir(renders_dir))
        ssims, psnrs, lpipss = [], [], []
        for fname in names:
            render, gt = _read_png(os.path.join(renders_dir, fname)), _read_png(os.path.join(gt_dir, fname))
            s, p = score(render, gt)
            ssims.append(float(s))
            psnrs.append(float(p))
            if lpips_fn is not None:
                lpipss.append(float(lpips_fn(render[None].to(device), gt[None].to(device))))
        mean = lambda v: float(np.mean(np.asarray(v, np.float64))) if v else float("nan")  # noqa: E731
        full[method] = {"SSIM": mean(ssims), "PSNR": mean(psnrs)}
        per_view[method] = {"SSIM": dict(zip(names, ssims)), "PSNR": dict(zip(names, psnrs))}
        if lpips_fn is not None:
            full[method]["LPIPS"] = mean(lpipss)
            per_view[method]["LPIPS"] = dict(zip(names, lpipss))
    with open(os.path.join(model_path, "results.json"), "w") as fp:
        json.dump(full, fp, indent=True)
    with open(os.path.join(model_path, "per_view.json"), "w") as fp:
        json.dump(per_view, fp, indent=True)
    return full, per_view


@torch.no_grad()
def report(views, pc, pipe, background, kernel_size):
    """training_report's test loop (train.py:332-365): every view rendered, render and
    view.original_image clamped to [0, 1] and scored with quantize=False and no SSIM.
    -> (mean L1, mean PSNR) over the views, float64.  The PSNR of a view is that of the whole
    image's MSE, as metric.py takes it (the reference's psnr() on an unbatched [3,H,W] image
    averages three per-channel PSNRs instead)."""
    from gaussian_renderer import render

    l1, psnr = [], []
    for view in views:
        rendering = render(view, pc, pipe, background, kernel_size=kernel_size)["render"]
        m = image_metrics(rendering, view.original_image.to(rendering.device), quantize=False, ssim=False)
        l1.append(m["L1"])
        psnr.append(m["PSNR"])
    if not views:
        return float("nan"), float("nan")
    return float(torch.cat(l1).mean()), float(torch.cat(psnr).mean())

