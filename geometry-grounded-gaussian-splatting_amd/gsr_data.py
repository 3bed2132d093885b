"""From a COLMAP dataset directory to TrainStep.step: the head of the reference's
train.py (Scene(...): scene/dataset_readers.py, utils/camera_utils.py,
scene/cameras.py, scene/__init__.py:83-131, GaussianModel.create_from_pcd).

    scene = load_colmap_scene(path, resolution=-1)            # ColmapScene: views, extent, SfM points
    ids = nearest_views(scene.train_views, 30, 0.01, 1.5, 8)  # the PatchMatch neighbours of every view
    raw = initial_gaussians(scene.points, scene.colors, scene.train_views, sh_degree=3, sg_degree=0)
    g = gsr_train.TrainGaussians(raw, spatial_lr_scale=scene.cameras_extent)

The hot path is the image preparation.  The reference resizes every image and
mask on the CPU (PIL.Image.resize, then / 255.0, then a copy to the device);
here the decoded bytes go to the device once and gsr_image_resample8 /
gsr_view_planes (csrc/viewprep.hip) produce the planes there.  The contract is
the byte: resize_u8 is Pillow's 8-bit two-pass fixed-point bicubic resample bit
for bit, so the ground truth a view holds is the reference's.

One deliberate deviation: with no mask file the reference builds an all-255
mask, so every Camera carries gt_mask = 1; here gt_mask stays None (the
composite gt * 1 + bg * 0 is gt exactly, the losses are unchanged, and the
unfused TrainStep path, which refuses masked views, keeps working).

Device tensors on the current stream; there is no CPU path for the images.
"""
from __future__ import annotations

import functools
import json
import math
import os
import struct
from ctypes import POINTER, c_int
from dataclasses import dataclass, field

import numpy as np
import torch

import gsr_scene as S
from diff_gaussian_rasterization._abi import call, load, ptr, require, stream
from gsr_train import TrainView

ZNEAR, ZFAR = 0.01, 100.0  # scene/cameras.py:64-65


# ---- Pillow's resample on the device ----------------------------------------------------------------------------

def resample_coeffs(in_size, out_size):
    """gsr_resample_coeffs: (k int32 [out_size, ksize], bounds int32 [out_size, 2] = (first index, count)),
    Pillow's bicubic table of one axis (float64 on the host, 22 fractional bits)."""
    in_size, out_size = int(in_size), int(out_size)
    lib = load()
    ksize = lib.gsr_resample_ksize(in_size, out_size)
    if ksize <= 0:
        raise RuntimeError(f"resample_coeffs: sizes must be in [1, 2^20] (got {in_size} -> {out_size})")
    k = np.zeros((out_size, ksize), np.int32)
    bounds = np.zeros((out_size, 2), np.int32)
    ip = POINTER(c_int)
    if lib.gsr_resample_coeffs(in_size, out_size, k.ctypes.data_as(ip), bounds.ctypes.data_as(ip)) != 0:
        raise RuntimeError("gsr: " + lib.gsr_last_error().decode())
    return k, bounds


@functools.lru_cache(maxsize=16)
def _device_table(in_size, out_size, device):
    """The table of one axis on `device`, k transposed to tap-major [ksize, out_size] as the kernels read it."""
    k, bounds = resample_coeffs(in_size, out_size)
    return (torch.from_numpy(np.ascontiguousarray(k.T)).to(device), torch.from_numpy(bounds).to(device))


def _size(size, who):
    try:
        W, H = (int(v) for v in size)
    except (TypeError, ValueError):
        raise RuntimeError(f"{who}: `size` must be (W, H)") from None
    if W < 1 or H < 1:
        raise RuntimeError(f"{who}: `size` must be (W, H) with W, H >= 1 (got {tuple(size)})")
    return W, H


def _resample(x, axis, out_size):
    """One pass of x [N,H,W,C] along H (axis 0) or W (axis 1)."""
    N, H, W, C = x.shape
    out = torch.empty((N, out_size, W, C) if axis == 0 else (N, H, out_size, C), dtype=torch.uint8, device=x.device)
    k, bounds = _device_table((H, W)[axis], out_size, x.device)
    call(x.device, "gsr_image_resample8", N, H, W, C, axis, out_size, ptr(x), ptr(out), ptr(k), ptr(bounds),
         stream(x.device))
    return out


@torch.no_grad()
def resize_u8(image_u8, size):
    """PIL.Image.resize((W, H)) (the default bicubic filter) of `L` / `RGB` / `RGBA` bytes on the device:
    image_u8 uint8 [H,W], [H,W,C] or [N,H,W,C] with C = 1..4 -> the same layout at H x W.  Every channel is
    resized on its own, as loadCam does for an RGBA file (its channels are split and resized as `L`: no
    premultiplication by alpha).  The pass along W runs first, its bytes are the input of the pass along H;
    a pass that keeps its size is skipped."""
    who = "resize_u8"
    if not isinstance(image_u8, torch.Tensor) or image_u8.dim() not in (2, 3, 4):
        raise RuntimeError(f"{who}: `image_u8` must be a uint8 HIP tensor [H,W], [H,W,C] or [N,H,W,C]")
    require(image_u8, "image_u8", (torch.uint8,), image_u8.dim(), who)
    W, H = _size(size, who)
    x = image_u8.contiguous()
    x = x.view({2: (1,) + tuple(x.shape) + (1,), 3: (1,) + tuple(x.shape), 4: tuple(x.shape)}[x.dim()])
    if not 1 <= x.shape[3] <= 4:
        raise RuntimeError(f"{who}: `image_u8` must have 1 to 4 channels (got {x.shape[3]})")
    if x.shape[1] < 1 or x.shape[2] < 1:
        raise RuntimeError(f"{who}: `image_u8` must have H, W >= 1 (got {tuple(image_u8.shape)})")
    if x.shape[2] != W:
        x = _resample(x, 1, W)
    if x.shape[1] != H:
        x = _resample(x, 0, H)
    if x.data_ptr() == image_u8.data_ptr():
        x = x.clone()  # (Image.resize returns a copy)
    return x.view({2: (H, W), 3: (H, W, x.shape[3]), 4: tuple(x.shape)}[image_u8.dim()])


@torch.no_grad()
def view_planes(rgb_u8, mask_u8=None):
    """gsr_view_planes: rgb_u8 uint8 [N,H,W,3] (and mask_u8 [N,H,W]) -> (original_image [N,3,H,W] = byte / 255,
    gray_image [N,1,H,W] = (0.299 r + 0.587 g) + 0.114 b, gt_mask [N,1,H,W] = mask byte / 255 or None),
    float32, what PILtoTorch and Camera.__init__ compute."""
    who = "view_planes"
    require(rgb_u8, "rgb_u8", (torch.uint8,), 4, who)
    N, H, W, C = rgb_u8.shape
    if C != 3 or H < 1 or W < 1:
        raise RuntimeError(f"{who}: `rgb_u8` must have shape (N, H, W, 3) with H, W >= 1 (got {tuple(rgb_u8.shape)})")
    dev = rgb_u8.device
    if mask_u8 is not None:
        require(mask_u8, "mask_u8", (torch.uint8,), 3, who)
        if tuple(mask_u8.shape) != (N, H, W) or mask_u8.device != dev:
            raise RuntimeError(f"{who}: `mask_u8` must have the size of `rgb_u8` and its device (got "
                               f"{tuple(mask_u8.shape)} for {tuple(rgb_u8.shape)})")
        mask_u8 = mask_u8.contiguous()
    original = torch.empty((N, 3, H, W), dtype=torch.float32, device=dev)
    gray = torch.empty((N, 1, H, W), dtype=torch.float32, device=dev)
    gt_mask = torch.empty((N, 1, H, W), dtype=torch.float32, device=dev) if mask_u8 is not None else None
    call(dev, "gsr_view_planes", N, H, W, ptr(rgb_u8.contiguous()), ptr(mask_u8), ptr(original), ptr(gray),
         ptr(gt_mask), stream(dev))
    return original, gray, gt_mask


# ---- cameras ------------------------------------------------------------------------------------------------------

def target_resolution(orig_w, orig_h, resolution, resolution_scale=1.0):
    """loadCam's (W, H) (utils/camera_utils.py:23-42): for `resolution` 1, 2, 4, 8 Python's round (half to even)
    of orig / (resolution_scale * resolution); otherwise int(orig / scale) with scale = orig_w / resolution, and
    for -1 orig_w / 1600 when the image is wider than 1600 pixels (else 1), times resolution_scale."""
    if resolution in [1, 2, 4, 8]:
        return (round(orig_w / (resolution_scale * resolution)), round(orig_h / (resolution_scale * resolution)))
    if resolution == -1:
        global_down = orig_w / 1600 if orig_w > 1600 else 1
    else:
        global_down = orig_w / resolution
    scale = float(global_down) * float(resolution_scale)
    return (int(orig_w / scale), int(orig_h / scale))


def _view(W, H, R, T, FovX, FovY, device, uid, image_name):
    """scene/cameras.py:41-73 for one camera; the matrices are formed on the host in float32 as gsr_scene does."""
    R, T = np.asarray(R, np.float64), np.asarray(T, np.float64)
    wvt = torch.tensor(S.world2view(R, T)).transpose(0, 1).contiguous()
    proj = S.projection(ZNEAR, ZFAR, FovX, FovY).transpose(0, 1)
    full = (wvt.unsqueeze(0).bmm(proj.unsqueeze(0))).squeeze(0).contiguous()
    center = wvt.inverse()[3, :3].contiguous()
    return TrainView(W, H, FovX, FovY, wvt.to(device), full.to(device), center.to(device),
                     torch.tensor(R, dtype=torch.float32).to(device), torch.tensor(T, dtype=torch.float32).to(device),
                     W / (2 * math.tan(FovX / 2.)), H / (2 * math.tan(FovY / 2.)), float(W - 1) / 2, float(H - 1) / 2,
                     uid=uid, image_name=image_name)


def _host_bytes(a, name, who, channels):
    """`a` (numpy array or tensor, on any device) as a uint8 tensor [H,W,C] with C in `channels`."""
    if isinstance(a, np.ndarray):  # (a decoded PIL image is read-only: torch wants a writable array)
        a = np.ascontiguousarray(a) if a.flags.writeable else a.copy()
    t = torch.from_numpy(a) if isinstance(a, np.ndarray) else a
    if not isinstance(t, torch.Tensor) or t.dtype != torch.uint8:
        raise RuntimeError(f"{who}: `{name}` must be uint8 (got {getattr(t, 'dtype', type(t).__name__)})")
    if t.dim() == 2:
        t = t.unsqueeze(-1)
    if t.dim() != 3 or t.shape[2] not in channels or t.shape[0] < 1 or t.shape[1] < 1:
        raise RuntimeError(f"{who}: `{name}` must have shape (H, W, C) with C in {tuple(channels)} "
                           f"(got {tuple(t.shape)})")
    return t


@torch.no_grad()
def _prepare_batch(rgb, mask, size):
    """rgb uint8 [N,H,W,3] and mask [N,H,W] or None on the device -> view_planes of the resized bytes."""
    rgb = resize_u8(rgb, size)
    if mask is not None:
        mask = resize_u8(mask.unsqueeze(-1), size).squeeze(-1)
    return view_planes(rgb, mask)


def prepare_view(rgb_u8, R, T, FovX, FovY, *, mask_u8=None, resolution=-1, resolution_scale=1.0, uid=0, image_name="",
                 device="cuda"):
    """loadCam + Camera.__init__ for one decoded image: rgb_u8 uint8 [H,W,3] or [H,W,4] (numpy or tensor; an alpha
    channel is dropped — the reference resizes it and then overwrites it with the mask), mask_u8 [H,W] of the
    same size or None, R, T in the reference's convention (R = qvec2rotmat(q).T).  -> a TrainView whose
    original_image, gray_image and gt_mask are the reference's to the last bit at target_resolution(...)."""
    who = "prepare_view"
    device = torch.device(device)
    rgb = _host_bytes(rgb_u8, "rgb_u8", who, (3, 4))
    H0, W0 = rgb.shape[:2]
    mask = None
    if mask_u8 is not None:
        mask = _host_bytes(mask_u8, "mask_u8", who, (1,))
        if tuple(mask.shape[:2]) != (H0, W0):
            raise RuntimeError(f"{who}: `mask_u8` must have the size of `rgb_u8` (got {tuple(mask.shape[:2])} for "
                               f"{(H0, W0)})")
        mask = mask[:, :, 0].to(device)[None]
    W, H = target_resolution(W0, H0, resolution, resolution_scale)
    original, gray, gt_mask = _prepare_batch(rgb[:, :, :3].to(device)[None], mask, _size((W, H), who))
    view = _view(W, H, R, T, FovX, FovY, device, uid, image_name)
    view.original_image, view.gray_image = original[0], gray[0]
    view.gt_mask = gt_mask[0] if gt_mask is not None else None
    return view


# ---- COLMAP binary models -----------------------------------------------------------------------------------------
# COLMAP's documented binary format (colmap.github.io/format.html, "Binary File Format"): little endian, every
# file begins with a uint64 count.

# model id -> (name, number of parameters), COLMAP's camera models
_CAMERA_MODELS = {0: ("SIMPLE_PINHOLE", 3), 1: ("PINHOLE", 4), 2: ("SIMPLE_RADIAL", 4), 3: ("RADIAL", 5),
                  4: ("OPENCV", 8), 5: ("OPENCV_FISHEYE", 8), 6: ("FULL_OPENCV", 12), 7: ("FOV", 5),
                  8: ("SIMPLE_RADIAL_FISHEYE", 4), 9: ("RADIAL_FISHEYE", 5), 10: ("THIN_PRISM_FISHEYE", 12)}


@dataclass
class ColmapCamera:
    id: int
    model: str
    width: int
    height: int
    params: np.ndarray  # float64


@dataclass
class ColmapImage:
    id: int
    qvec: np.ndarray  # (qw, qx, qy, qz), world to camera
    tvec: np.ndarray
    camera_id: int
    name: str


def _unpack(fh, fmt):
    size = struct.calcsize("<" + fmt)
    data = fh.read(size)
    if len(data) != size:
        raise RuntimeError(f"read_colmap_model: {fh.name} is truncated")
    return struct.unpack("<" + fmt, data)


def read_colmap_model(sparse_dir):
    """cameras.bin, images.bin and points3D.bin of `sparse_dir` -> (cameras {id: ColmapCamera}, images
    {id: ColmapImage} in file order, xyz float64 [P,3], rgb uint8 [P,3]).  The 2D observations and the tracks
    are skipped.  Only PINHOLE and SIMPLE_PINHOLE cameras are accepted (undistorted datasets)."""
    cameras, images = {}, {}
    with open(os.path.join(sparse_dir, "cameras.bin"), "rb") as fh:
        for _ in range(_unpack(fh, "Q")[0]):
            cam_id, model_id, width, height = _unpack(fh, "IiQQ")
            if model_id not in _CAMERA_MODELS:
                raise RuntimeError(f"read_colmap_model: unknown camera model id {model_id}")
            name, n = _CAMERA_MODELS[model_id]
            params = np.array(_unpack(fh, "d" * n))
            if name not in ("PINHOLE", "SIMPLE_PINHOLE"):  # (the reference's assertion, readColmapCameras)
                raise AssertionError("Colmap camera model not handled: only undistorted datasets (PINHOLE or "
                                     "SIMPLE_PINHOLE cameras) supported!")
            cameras[cam_id] = ColmapCamera(cam_id, name, width, height, params)
    with open(os.path.join(sparse_dir, "images.bin"), "rb") as fh:
        for _ in range(_unpack(fh, "Q")[0]):
            image_id, *qt, camera_id = _unpack(fh, "I7dI")
            name = b""
            while (c := fh.read(1)) != b"\x00":
                if not c:
                    raise RuntimeError(f"read_colmap_model: {fh.name} is truncated")
                name += c
            fh.seek(24 * _unpack(fh, "Q")[0], os.SEEK_CUR)  # (x, y, point3D id) per observation
            images[image_id] = ColmapImage(image_id, np.array(qt[:4]), np.array(qt[4:]), camera_id, name.decode("utf-8"))
    with open(os.path.join(sparse_dir, "points3D.bin"), "rb") as fh:
        P = _unpack(fh, "Q")[0]
        xyz, rgb = np.empty((P, 3), np.float64), np.empty((P, 3), np.uint8)
        for p in range(P):
            _, x, y, z, r, g, b, _, track = _unpack(fh, "QdddBBBdQ")
            xyz[p], rgb[p] = (x, y, z), (r, g, b)
            fh.seek(8 * track, os.SEEK_CUR)  # (image id, point2D index) per track element
    return cameras, images, xyz, rgb


def qvec2rotmat(q):
    """The rotation matrix of COLMAP's (qw, qx, qy, qz), in its published form (float64)."""
    w, x, y, z = q
    return np.array([[1 - 2 * y**2 - 2 * z**2, 2 * x * y - 2 * w * z, 2 * z * x + 2 * w * y],
                     [2 * x * y + 2 * w * z, 1 - 2 * x**2 - 2 * z**2, 2 * y * z - 2 * w * x],
                     [2 * z * x - 2 * w * y, 2 * y * z + 2 * w * x, 1 - 2 * x**2 - 2 * y**2]])


def _focal2fov(focal, pixels):
    return 2 * math.atan(pixels / (2 * focal))


@dataclass
class CameraInfo:
    """What readColmapCameras keeps of one registered image."""
    uid: int  # the COLMAP camera id
    R: np.ndarray
    T: np.ndarray
    FovY: float
    FovX: float
    image_path: str
    image_name: str
    mask_path: str | None
    width: int
    height: int


def read_colmap_cameras(path, images="images", masks=None):
    """readColmapCameras + the sort of readColmapSceneInfo for path/sparse/0: CameraInfo records sorted by
    image name, with the SfM points (xyz float64, rgb uint8)."""
    cameras, registered, xyz, rgb = read_colmap_model(os.path.join(path, "sparse/0"))
    infos = []
    for im in registered.values():
        cam = cameras[im.camera_id]
        fx = cam.params[0]
        fy = cam.params[0] if cam.model == "SIMPLE_PINHOLE" else cam.params[1]
        image_path = os.path.join(path, images or "images", os.path.basename(im.name))
        infos.append(CameraInfo(uid=cam.id, R=np.transpose(qvec2rotmat(im.qvec)), T=np.array(im.tvec),
                                FovY=_focal2fov(fy, cam.height), FovX=_focal2fov(fx, cam.width), image_path=image_path,
                                image_name=os.path.basename(image_path).split(".")[0],
                                mask_path=os.path.join(path, masks, im.name) if masks else None, width=cam.width,
                                height=cam.height))
    return sorted(infos, key=lambda c: c.image_name), xyz, rgb


def nerfpp_radius(infos):
    """getNerfppNorm's radius: 1.1 x the largest distance of a camera centre from their mean, in the float32
    of getWorld2View2."""
    centers = np.hstack([np.linalg.inv(S.world2view(c.R, c.T))[:3, 3:4] for c in infos])
    dist = np.linalg.norm(centers - np.mean(centers, axis=1, keepdims=True), axis=0, keepdims=True)
    return np.max(dist) * 1.1


def split_train_test(infos, eval=False, llffhold=8):
    """readColmapSceneInfo's split of the sorted cameras: with `eval` every llffhold-th one is a test camera."""
    if not eval:
        return list(infos), []
    return ([c for idx, c in enumerate(infos) if idx % llffhold != 0],
            [c for idx, c in enumerate(infos) if idx % llffhold == 0])


@dataclass
class ColmapScene:
    train_views: list
    test_views: list
    cameras_extent: float  # nerf_normalization["radius"]
    points: np.ndarray  # float32 [P,3]
    colors: np.ndarray  # float64 [P,3] in [0, 1]
    train_infos: list = field(default_factory=list)
    test_infos: list = field(default_factory=list)


def _decode(info):
    """(rgb uint8 [H,W,3], mask uint8 [H,W] or None) of one CameraInfo, decoded with PIL on the host."""
    from PIL import Image

    with Image.open(info.image_path) as im:
        if im.mode not in ("RGB", "RGBA"):
            raise RuntimeError(f"load_colmap_scene: {info.image_path} is a `{im.mode}` image; RGB or RGBA expected")
        rgb = np.asarray(im)[:, :, :3]
    mask = None
    if info.mask_path is not None and os.path.exists(info.mask_path):
        with Image.open(info.mask_path) as m:
            mask = np.asarray(m.convert("L"))
        if mask.shape != rgb.shape[:2]:
            raise RuntimeError(f"load_colmap_scene: {info.mask_path} is {mask.shape[1]} x {mask.shape[0]}, its image "
                               f"{rgb.shape[1]} x {rgb.shape[0]}")
    return np.ascontiguousarray(rgb), mask


def _views(infos, resolution, resolution_scale, device, batch):
    """cameraList_from_camInfos: the views of `infos` in order; images of one size (and mask or no mask) are
    prepared together, at most `batch` per launch."""
    views = [None] * len(infos)
    pending = {}  # (H, W, masked) -> [(index, rgb, mask)]

    def flush(key):
        items = pending.pop(key)
        H0, W0, masked = key
        size = target_resolution(W0, H0, resolution, resolution_scale)
        rgb = torch.from_numpy(np.stack([r for _, r, _ in items])).to(device)
        mask = torch.from_numpy(np.stack([m for _, _, m in items])).to(device) if masked else None
        original, gray, gt_mask = _prepare_batch(rgb, mask, _size(size, "load_colmap_scene"))
        for n, (idx, _, _) in enumerate(items):
            c = infos[idx]
            v = _view(size[0], size[1], c.R, c.T, c.FovX, c.FovY, device, idx, c.image_name)
            v.original_image, v.gray_image = original[n], gray[n]
            v.gt_mask = gt_mask[n] if masked else None
            views[idx] = v

    for idx, c in enumerate(infos):
        rgb, mask = _decode(c)
        key = (rgb.shape[0], rgb.shape[1], mask is not None)
        pending.setdefault(key, []).append((idx, rgb, mask))
        if len(pending[key]) >= batch:
            flush(key)
    for key in list(pending):
        flush(key)
    return views


def load_colmap_scene(path, images="images", masks=None, eval=False, llffhold=8, resolution=-1, resolution_scale=1.0,
                      device="cuda", batch=8):
    """readColmapSceneInfo + Scene.__init__'s camera lists for a COLMAP directory (sparse/0 binary model, the
    images under `images`, optional masks under `masks` by the image's file name): cameras sorted by image name,
    every llffhold-th one a test camera with `eval`, cameras_extent from the training cameras, the SfM points as
    the reference's points3D.ply round trip leaves them (xyz float32, colours rgb / 255 float64), and the
    views prepared on `device`.  A view's uid is its index in its list (loadCam's id)."""
    device = torch.device(device)
    infos, xyz, rgb = read_colmap_cameras(path, images, masks)
    train, test = split_train_test(infos, eval, llffhold)
    return ColmapScene(train_views=_views(train, resolution, resolution_scale, device, batch),
                       test_views=_views(test, resolution, resolution_scale, device, batch),
                       cameras_extent=float(nerfpp_radius(train)), points=xyz.astype(np.float32),
                       colors=rgb / 255.0, train_infos=train, test_infos=test)


# ---- PatchMatch neighbours ----------------------------------------------------------------------------------------

@torch.no_grad()
def nearest_views(views, max_angle=30, min_dis=0.01, max_dis=1.5, num=8, json_path=None):
    """scene/__init__.py:83-118: for every view the indices of up to `num` other views, nearest first, whose
    centre is farther than min_dis and nearer than max_dis and whose optical axis is within max_angle degrees
    (float32; arccos * 180 / 3.14159 and lexsort((angle, dist)) as the reference writes them; strict
    inequalities).  With `json_path` the reference's multi_view.json is written, one line per view."""
    if not views:
        return []
    centers = torch.stack([v.camera_center for v in views], dim=0)
    ray = torch.tensor([0.0, 0.0, 1.0], device=centers.device)
    rays = torch.stack([ray @ v.R.transpose(-1, -2) for v in views], dim=0)
    rays = torch.nn.functional.normalize(rays, dim=-1)
    diss = torch.norm(centers[:, None] - centers[None], dim=-1).cpu().numpy()
    angles = (torch.arccos(torch.sum(rays[:, None] * rays[None], dim=-1)) * 180 / 3.14159).cpu().numpy()
    ids, lines = [], []
    for i, view in enumerate(views):
        order = np.lexsort((angles[i], diss[i]))
        keep = (angles[i][order] < max_angle) & (diss[i][order] > min_dis) & (diss[i][order] < max_dis)
        ids.append([int(j) for j in order[keep][:num]])
        lines.append(json.dumps({"ref_name": getattr(view, "image_name", ""),
                                 "nearest_name": [getattr(views[j], "image_name", "") for j in ids[-1]]},
                                separators=(",", ":")))
    if json_path is not None:
        with open(json_path, "w") as fh:
            for line in lines:
                fh.write(line)
                fh.write("\n")
    return ids


# ---- the initial Gaussians ----------------------------------------------------------------------------------------

SH_C0 = 0.28209479177387814


@torch.no_grad()
def initial_gaussians(points, colors, views, sh_degree=3, sg_degree=0, generator=None):
    """GaussianModel.create_from_pcd (scene/gaussian_model.py:304-338) and the per-camera scale clamp of
    scene/__init__.py:126-131 as a RawGaussians on the views' device: positions, the DC colour (rgb - 0.5) / C0,
    log of the root mean squared distance to the three nearest points (simple_knn.distCUDA2, floored at 1e-7)
    as isotropic scale, clamped to log(0.05 x distance) from every view's centre; identity rotations, opacity
    inverse_sigmoid(0.1), random unit SG axes (`generator`, on the device), zero SG sharpness and colour.
    filter_3D is zero: TrainGaussians.compute_3D_filter fills it, as train.py does after Scene(...)."""
    from simple_knn._C import distCUDA2

    if not views:
        raise RuntimeError("initial_gaussians: `views` must hold the training views")
    dev = views[0].camera_center.device
    xyz = torch.tensor(np.asarray(points)).float().to(dev)
    if xyz.dim() != 2 or xyz.shape[1] != 3:
        raise RuntimeError(f"initial_gaussians: `points` must have shape (P, 3) (got {tuple(xyz.shape)})")
    P = xyz.shape[0]
    color = (torch.tensor(np.asarray(colors)).float().to(dev) - 0.5) / SH_C0
    if tuple(color.shape) != (P, 3):
        raise RuntimeError(f"initial_gaussians: `colors` must have shape ({P}, 3) (got {tuple(color.shape)})")
    features = torch.zeros((P, 3, (sh_degree + 1) ** 2), device=dev)
    features[:, :3, 0] = color
    sg_axis = torch.randn(P, sg_degree, 3, device=dev, generator=generator)
    sg_axis = torch.nn.functional.normalize(sg_axis, dim=2)
    dist2 = torch.clamp_min(distCUDA2(xyz.detach().clone()), 0.0000001)
    scaling = torch.log(torch.sqrt(dist2))[..., None].repeat(1, 3)
    for view in views:
        max_scale = 0.05 * torch.norm(xyz - view.camera_center[None, :], dim=1)
        scaling = torch.clamp_max(scaling, torch.log(max_scale).repeat(3, 1).permute(1, 0))
    rotation = torch.zeros((P, 4), device=dev)
    rotation[:, 0] = 1
    opacity = 0.1 * torch.ones((P, 1), dtype=torch.float, device=dev)
    opacity = torch.log(opacity / (1 - opacity))
    return S.RawGaussians(xyz=xyz, features_dc=features[:, :, 0:1].transpose(1, 2).contiguous(),
                          features_rest=features[:, :, 1:].transpose(1, 2).contiguous(), scaling=scaling.contiguous(),
                          rotation=rotation, opacity=opacity, sg_axis=sg_axis,
                          sg_sharpness=torch.zeros(P, sg_degree, device=dev),
                          sg_color=torch.zeros(P, sg_degree, 3, device=dev), filter_3D=torch.zeros(P, 1, device=dev))
