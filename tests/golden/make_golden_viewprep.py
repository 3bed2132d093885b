"""Generate tests/golden/viewprep_scene/ (a tiny COLMAP dataset) and
tests/golden/viewprep.npz (what the reference makes of it): readColmapSceneInfo
(scene/dataset_readers.py) and loadCam -> PILtoTorch -> Camera
(utils/camera_utils.py, scene/cameras.py), run unmodified on the CPU.

Run in the build container (where /root/reference exists, with scipy and PIL):
    python tests/golden/make_golden_viewprep.py
Only DATA is committed: the binary model, the PNG files, and the recorded
results.

How the reference is run: `open3d`, `trimesh`, `cv2` and `simple_knn` (not
installed, not used on this path) are empty stubs; `plyfile` (not installed) is
a stub whose PlyData keeps the structured array storePly builds — float32
positions and uint8 colours, the round trip of the real file; torch's
Tensor.cuda is the identity and data_device is "cpu".

The scene: six 53 x 37 images (one RGBA), names out of file order, a PINHOLE and
a SIMPLE_PINHOLE camera, masks for two images, 40 points; six cameras on an
irregular arc 2 units from the origin, looking at it.
"""
from __future__ import annotations

import os
import shutil
import struct
import sys
import tempfile
import types

import numpy as np
import torch
from PIL import Image

REF = "/root/reference"
OUT = os.path.dirname(os.path.abspath(__file__))
SCENE = os.path.join(OUT, "viewprep_scene")
W, H = 53, 37
LLFFHOLD, RESOLUTION = 3, 2


def rotmat2qvec(R):
    """(qw, qx, qy, qz) of a rotation matrix (trace form; the fixture's rotations are far from 180 degrees)."""
    w = np.sqrt(1.0 + R[0, 0] + R[1, 1] + R[2, 2]) / 2.0
    return np.array([w, (R[2, 1] - R[1, 2]) / (4 * w), (R[0, 2] - R[2, 0]) / (4 * w), (R[1, 0] - R[0, 1]) / (4 * w)])


def write_scene(seed=0):
    rng = np.random.default_rng(seed)
    shutil.rmtree(SCENE, ignore_errors=True)
    for sub in ("sparse/0", "images", "masks"):
        os.makedirs(os.path.join(SCENE, sub))
    # name, camera id, RGBA, masked: registered out of name order
    images = [("view_d.png", 1, False, False), ("view_a.png", 2, False, True), ("view_f.png", 1, True, False),
              ("view_b.png", 1, False, False), ("view_e.png", 2, False, True), ("view_c.png", 1, False, False)]
    angles = {"a": -31.0, "b": -17.5, "c": -6.0, "d": 4.5, "e": 19.0, "f": 36.0}  # degrees about y
    with open(os.path.join(SCENE, "sparse/0/cameras.bin"), "wb") as fh:
        fh.write(struct.pack("<Q", 2))
        fh.write(struct.pack("<IiQQ4d", 1, 1, W, H, 61.25, 58.5, W / 2.0, H / 2.0))  # PINHOLE
        fh.write(struct.pack("<IiQQ3d", 2, 0, W, H, 64.75, W / 2.0, H / 2.0))  # SIMPLE_PINHOLE
    with open(os.path.join(SCENE, "sparse/0/images.bin"), "wb") as fh:
        fh.write(struct.pack("<Q", len(images)))
        for n, (name, cam, rgba, masked) in enumerate(images):
            th = np.radians(angles[name[5]])
            # camera to world: rotated about y, tilted a little about x, on an arc of radius about 2
            ry = np.array([[np.cos(th), 0, np.sin(th)], [0, 1, 0], [-np.sin(th), 0, np.cos(th)]])
            tx = np.radians(3.0 * n - 6.0)
            rx = np.array([[1, 0, 0], [0, np.cos(tx), -np.sin(tx)], [0, np.sin(tx), np.cos(tx)]])
            c2w = ry @ rx
            pos = -c2w @ np.array([0.0, 0.0, 2.0 + 0.07 * n])
            w2c = c2w.T
            q, t = rotmat2qvec(w2c), -w2c @ pos
            fh.write(struct.pack("<I7dI", 10 + n, *q, *t, cam))
            fh.write(name.encode() + b"\x00")
            obs = rng.integers(0, 4)  # a few 2D observations, to be skipped by a reader
            fh.write(struct.pack("<Q", obs))
            for _ in range(obs):
                fh.write(struct.pack("<ddq", rng.uniform(0, W), rng.uniform(0, H), -1))
            pix = rng.integers(0, 256, (H, W, 4 if rgba else 3), dtype=np.uint8)
            Image.fromarray(pix).save(os.path.join(SCENE, "images", name))
            if masked:
                m = (rng.random((H, W)) < 0.7).astype(np.uint8) * 255
                m[::5] = rng.integers(0, 256, m[::5].shape, dtype=np.uint8)  # soft rows: the resize is visible
                Image.fromarray(m).save(os.path.join(SCENE, "masks", name))
    with open(os.path.join(SCENE, "sparse/0/points3D.bin"), "wb") as fh:
        fh.write(struct.pack("<Q", 40))
        for p in range(40):
            track = int(rng.integers(0, 4))
            fh.write(struct.pack("<Q3d3BdQ", 100 + p, *(rng.standard_normal(3) * 0.4), *rng.integers(0, 256, 3),
                                 float(rng.random()), track))
            for _ in range(track):
                fh.write(struct.pack("<II", int(rng.integers(10, 16)), int(rng.integers(0, 3))))


def stub(name, **attrs):
    m = types.ModuleType(name)
    m.__dict__.update(attrs)
    sys.modules[name] = m
    return m


class _PlyElement:
    def __init__(self, data):
        self.data = data

    @staticmethod
    def describe(data, name):
        return _PlyElement(data)


class _PlyData:
    def __init__(self, elements):
        self.elements = elements

    def write(self, path):
        with open(path, "wb") as fh:
            np.save(fh, self.elements[0].data)

    @staticmethod
    def read(path):
        with open(path, "rb") as fh:
            return {"vertex": np.load(fh)}


def run_reference(path):
    for name in ("open3d", "trimesh", "cv2", "simple_knn"):
        stub(name)
    stub("simple_knn._C", distCUDA2=None)
    stub("plyfile", PlyData=_PlyData, PlyElement=_PlyElement)
    sys.path.insert(0, REF)
    torch.Tensor.cuda = lambda self, *a, **k: self
    from scene.dataset_readers import readColmapSceneInfo
    from utils.camera_utils import loadCam

    info = readColmapSceneInfo(path, "images", "masks", True, llffhold=LLFFHOLD)
    args = types.SimpleNamespace(resolution=RESOLUTION, data_device="cpu")
    out = dict(radius=np.asarray(info.nerf_normalization["radius"]), points=np.asarray(info.point_cloud.points),
               colors=np.asarray(info.point_cloud.colors),
               train_names=np.array([c.image_name for c in info.train_cameras]),
               test_names=np.array([c.image_name for c in info.test_cameras]))
    assert out["points"].dtype == np.float32 and out["colors"].dtype == np.float64
    for split, cams in (("train", info.train_cameras), ("test", info.test_cameras)):
        for idx, c in enumerate(cams):
            cam = loadCam(args, idx, c, 1.0)
            has_mask = c.mask_path is not None and os.path.exists(c.mask_path)
            if not has_mask:
                assert bool((cam.gt_mask == 1).all())  # the all-255 mask gsr_data leaves out
            rec = dict(R=np.asarray(c.R), T=np.asarray(c.T), FovX=np.float64(c.FovX), FovY=np.float64(c.FovY),
                       colmap_id=np.int64(c.uid), uid=np.int64(cam.uid), original_image=cam.original_image.numpy(),
                       gray_image=cam.gray_image.numpy(), has_mask=np.bool_(has_mask), gt_mask=cam.gt_mask.numpy(),
                       size=np.array([cam.image_width, cam.image_height]),
                       scalars=np.array([cam.Fx, cam.Fy, cam.Cx, cam.Cy, cam.FoVx, cam.FoVy, cam.znear, cam.zfar]),
                       world_view_transform=cam.world_view_transform.numpy(),
                       full_proj_transform=cam.full_proj_transform.numpy(), camera_center=cam.camera_center.numpy(),
                       R32=cam.R.numpy(), T32=cam.T.numpy())
            for k, v in rec.items():
                out[f"{split}/{c.image_name}/{k}"] = v
    return out


def main():
    write_scene()
    with tempfile.TemporaryDirectory() as tmp:
        work = os.path.join(tmp, "scene")  # (the reference writes points3D.ply beside the model)
        shutil.copytree(SCENE, work)
        out = run_reference(work)
    path = os.path.join(OUT, "viewprep.npz")
    np.savez_compressed(path, **out)
    size = sum(os.path.getsize(os.path.join(d, f)) for d, _, fs in os.walk(SCENE) for f in fs)
    print(f"{path}: {os.path.getsize(path)} bytes; {SCENE}: {size} bytes; train {list(out['train_names'])}, "
          f"test {list(out['test_names'])}, radius {float(out['radius']):.6f}")
    assert os.path.getsize(path) < 400_000 and size < 400_000


if __name__ == "__main__":
    main()
