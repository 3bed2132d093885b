"""TEST INFRASTRUCTURE ONLY — numpy restatement of the view preparation
(gsr_data, csrc/viewprep.hip): Pillow's 8-bit two-pass fixed-point bicubic
resample, the float planes scene/cameras.py keeps, and the nearest-view
choice of scene/__init__.py:83-118.  tests/test_viewprep.py pins the resize
to PIL.Image.resize byte for byte.

The resize rule (Pillow, Resample.c): per axis a table of out_size windows,
weights of the bicubic filter (a = -0.5, support 2) in float64 normalised to
sum 1 and rounded to 22 fractional bits; one output byte is
clip8((2^21 + sum pixel * k) >> 22) in int32; the horizontal pass first, the
intermediate rounded to uint8, then the vertical pass; a pass that keeps its
size is skipped.
"""
from __future__ import annotations

import math

import numpy as np

F32 = np.float32
PRECISION_BITS = 32 - 8 - 2


def bicubic(x, a=-0.5):
    x = abs(x)
    if x < 1.0:
        return ((a + 2.0) * x - (a + 3.0)) * x * x + 1
    if x < 2.0:
        return (((x - 5) * x + 8) * x - 4) * a
    return 0.0


def coeffs(in_size, out_size):
    """-> (k int32 [out_size, ksize], bounds int32 [out_size, 2] = (xmin, count))."""
    scale = float(in_size) / out_size
    filterscale = max(scale, 1.0)
    support = 2.0 * filterscale
    ksize = int(math.ceil(support)) * 2 + 1
    ss = 1.0 / filterscale
    k = np.zeros((out_size, ksize), np.int32)
    bounds = np.zeros((out_size, 2), np.int32)
    for xx in range(out_size):
        center = (xx + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        xmax = min(int(center + support + 0.5), in_size) - xmin
        w = [bicubic((x + xmin - center + 0.5) * ss) for x in range(xmax)]
        ww = 0.0
        for v in w:
            ww += v
        for x in range(xmax):
            v = w[x] / ww if ww != 0.0 else w[x]
            k[xx, x] = int(-0.5 + v * (1 << PRECISION_BITS)) if v < 0 else int(0.5 + v * (1 << PRECISION_BITS))
        bounds[xx] = (xmin, xmax)
    return k, bounds


def resample_axis(img, out_size, axis):
    """One pass over `axis` of a uint8 array."""
    k, bounds = coeffs(img.shape[axis], out_size)
    src = np.moveaxis(img, axis, 0).astype(np.int32)
    out = np.empty((out_size,) + src.shape[1:], np.uint8)
    for xx in range(out_size):
        xmin, n = bounds[xx]
        acc = np.tensordot(k[xx, :n], src[xmin:xmin + n], axes=(0, 0)) + (1 << (PRECISION_BITS - 1))
        out[xx] = np.clip(acc >> PRECISION_BITS, 0, 255)
    return np.ascontiguousarray(np.moveaxis(out, 0, axis))


def resize_u8(img, size):
    """img uint8 [..., H, W, C] -> [..., size[1], size[0], C]: Image.resize((W, H)) per channel."""
    W, H = size
    img = np.ascontiguousarray(img)
    if img.shape[-2] != W:
        img = resample_axis(img, W, img.ndim - 2)
    if img.shape[-3] != H:
        img = resample_axis(img, H, img.ndim - 3)
    return img


def planes(rgb_u8, mask_u8=None):
    """rgb [H,W,3], mask [H,W] or [H,W,1] uint8 -> (original [3,H,W], gray [1,H,W], gt_mask [1,H,W] or None) float32:
    byte / 255 in float32 and (0.299 r + 0.587 g) + 0.114 b with every product and sum rounded to float32."""
    img = np.ascontiguousarray(np.moveaxis(rgb_u8.astype(F32) / F32(255.0), -1, 0))
    gray = ((F32(0.299) * img[0] + F32(0.587) * img[1]) + F32(0.114) * img[2])[None]
    mask = None
    if mask_u8 is not None:
        mask = (np.asarray(mask_u8).reshape(rgb_u8.shape[:2]).astype(F32) / F32(255.0))[None]
    return img, gray.astype(F32), mask


def nearest_views(centers, R, max_angle, min_dis, max_dis, num):
    """scene/__init__.py:83-118 on float32 camera centres [n,3] and R [n,3,3] (the reference's Camera.R):
    -> the nearest_id lists, with the distance and angle matrices (float32)."""
    centers = np.asarray(centers, F32)
    rays = np.asarray(R, F32)[:, :, 2]  # [0, 0, 1] @ R^T: the third column of R
    rays = rays /np.maximum(np.linalg.norm(rays, axis=-1, keepdims=True), F32(1e-12))
    diff = centers[:, None] - centers[None]
    diss = np.sqrt((diff * diff).sum(-1, dtype=F32)).astype(F32)
    cos = (rays[:, None] * rays[None]).sum(-1, dtype=F32)
    with np.errstate(invalid="ignore"):
        angles = (np.arccos(cos) * F32(180) / F32(3.14159)).astype(F32)
    ids = []
    for i in range(len(centers)):
        order = np.lexsort((angles[i], diss[i]))
        keep = (angles[i][order] < max_angle) & (diss[i][order] > min_dis) & (diss[i][order] < max_dis)
        ids.append([int(j) for j in order[keep][:num]])
    return ids, diss, angles


# ---- the cases tests/test_viewprep.py and tests/test_gpu_viewprep.py share ----------------------------------------

# (H, W) in -> (H, W) out: downscale, one axis only, upscale, identity, 1 x 1, a thin strip, tiny, 83 taps
SHAPES = [((37, 53), (9, 13)), ((37, 53), (37, 13)), ((64, 48), (100, 75)), ((17, 19), (17, 19)), ((40, 40), (1, 1)),
          ((3, 1000), (2, 160)), ((5, 7), (3, 2)), ((2049, 8), (100, 8))]
CHECKER_OUT = [(23, 17), (90, 100)]  # from the 64 x 64 checkerboard of 0 and 255
CHANNELS = (1, 3, 4)


def random_image(shape, C, seed=0):
    return np.random.default_rng(seed).integers(0, 256, tuple(shape) + (C,), dtype=np.uint8)


def checkerboard(C=1, n=64):
    board = (((np.arange(n)[:, None] + np.arange(n)[None]) % 2) * 255).astype(np.uint8)
    return np.ascontiguousarray(np.repeat(board[:, :, None], C, axis=2))


def ring_cameras(n=12, seed=3):
    """n cameras on an irregular ring of radius about 1 looking at its centre: (centers float32 [n,3], R float32
    [n,3,3] camera to world, as Camera.R), with the gaps asserted that keep float32 rounding from reordering
    anything: see assert_gaps."""
    rng = np.random.default_rng(seed)
    th = np.sort(rng.uniform(0, 2 * np.pi, n)) + rng.uniform(-0.05, 0.05, n)
    radius = 1.0 + rng.uniform(-0.15, 0.15, n)
    centers = np.stack([radius * np.sin(th), rng.uniform(-0.1, 0.1, n), -radius * np.cos(th)], -1)
    R = []
    for c in centers:
        z = -c / np.linalg.norm(c)
        x = np.cross([0.0, 1.0, 0.0], z)
        x /= np.linalg.norm(x)
        R.append(np.stack([x, np.cross(z, x), z], -1))
    return centers.astype(F32), np.asarray(R, F32)


def assert_gaps(diss, angles, max_angle, min_dis, max_dis):
    """From any camera no two distances within 1e-4 relative of each other, no angle within 0.01 degrees of
    max_angle, no distance within 1e-4 relative of min_dis or max_dis (the camera itself, at distance 0, aside)."""
    n = len(diss)
    off = ~np.eye(n, dtype=bool)
    for i in range(n):
        d = np.sort(diss[i].astype(np.float64))
        assert np.all(np.diff(d) > 1e-4 * d[1:]), (i, d)
    assert np.all(np.abs(angles[off].astype(np.float64) - max_angle) > 0.01)
    for bound in (min_dis, max_dis):
        assert np.all(np.abs(diss[off].astype(np.float64) - bound) > 1e-4 * bound)
