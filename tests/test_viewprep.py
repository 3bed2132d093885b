"""The numpy restatement of the view preparation (tests/viewprep_ref.py) against PIL.Image.resize, and the
host side of gsr_data (target_resolution, nearest_views, the COLMAP reader) against the restatement and the
reference's own output for the golden scene (tests/golden/make_golden_viewprep.py).  CPU only.

Bars: everything is exact — bytes, names, the split, and R, T, FoVs, radius, points and image tensors to the
last bit (the same float64 / float32 operations in the same order on both sides).
"""
from __future__ import annotations

import os
import types

import numpy as np
import pytest
import torch

import viewprep_ref as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SCENE = os.path.join(GOLDEN, "viewprep_scene")
LLFFHOLD, RESOLUTION = 3, 2  # what make_golden_viewprep.py ran the reference with


def _pil_resize(img, size):
    """Image.resize (default filter) of every channel as `L`, as loadCam resizes an RGBA file."""
    from PIL import Image

    return np.stack([np.asarray(Image.fromarray(img[..., c]).resize(size)) for c in range(img.shape[-1])], -1)


@pytest.mark.parametrize("C", R.CHANNELS)
@pytest.mark.parametrize("shape", R.SHAPES, ids=lambda s: f"{s[0][0]}x{s[0][1]}to{s[1][0]}x{s[1][1]}")
def test_restatement_is_pillow(shape, C):
    from PIL import Image

    (h, w), (oh, ow) = shape
    img = R.random_image((h, w), C, seed=h + w + C)
    got = R.resize_u8(img, (ow, oh))
    assert got.shape == (oh, ow, C) and np.array_equal(got, _pil_resize(img, (ow, oh)))
    if C == 3:  # and the RGB image resized whole
        assert np.array_equal(got, np.asarray(Image.fromarray(img).resize((ow, oh))))


@pytest.mark.parametrize("C", R.CHANNELS)
@pytest.mark.parametrize("out", R.CHECKER_OUT)
def test_restatement_is_pillow_on_the_checkerboard(out, C):
    img = R.checkerboard(C)
    got = R.resize_u8(img, (out[1], out[0]))
    assert np.array_equal(got, _pil_resize(img, (out[1], out[0])))
    if out == (90, 100):  # the upscale overshoots: both ends of the byte range are reached
        assert got.min() == 0 and got.max() == 255


def test_window_of_83_taps():
    k, bounds = R.coeffs(2049, 100)  # scale 20.49: ceil(40.98) * 2 + 1
    assert k.shape == (100, 83) and bounds[:, 1].max() >= 82


def test_target_resolution():
    import gsr_data

    assert gsr_data.target_resolution(5187, 3361, -1) == (1600, 1036)
    assert gsr_data.target_resolution(5187, 3361, 4) == (1297, 840)
    assert gsr_data.target_resolution(5, 3, 2) == (2, 2)  # 2.5 and 1.5: half to even
    assert gsr_data.target_resolution(1600, 1063, -1) == (1600, 1063)
    assert gsr_data.target_resolution(1000, 500, 250) == (250, 125)
    assert gsr_data.target_resolution(5187, 3361, -1, 2.0) == (800, 518)


def test_nearest_views_against_the_restatement(tmp_path):
    import gsr_data

    max_angle, min_dis, max_dis, num = 60, 0.3, 1.2, 4
    centers, rot = R.ring_cameras()
    want, diss, angles = R.nearest_views(centers, rot, max_angle, min_dis, max_dis, num)
    R.assert_gaps(diss, angles, max_angle, min_dis, max_dis)
    views = [types.SimpleNamespace(camera_center=torch.from_numpy(centers[i]), R=torch.from_numpy(rot[i]),
                                   image_name=f"im{i:02d}") for i in range(len(centers))]
    path = tmp_path / "multi_view.json"
    got = gsr_data.nearest_views(views, max_angle, min_dis, max_dis, num, json_path=str(path))
    assert got == want
    assert all(i not in ids for i, ids in enumerate(got))  # never the camera itself
    lengths = {len(ids) for ids in got}
    assert max(lengths) == num and min(lengths) < num  # the cap and the three tests all cut somewhere
    lines = path.read_text().splitlines()
    assert len(lines) == len(views)
    assert lines[0] == '{"ref_name":"im00","nearest_name":[' + ",".join(f'"im{j:02d}"' for j in got[0]) + "]}"


# ---------------------------------------------------------------- the golden COLMAP scene

@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(GOLDEN, "viewprep.npz"))


def test_colmap_reader_against_the_reference(golden):
    import gsr_data

    infos, xyz, rgb = gsr_data.read_colmap_cameras(SCENE, "images", "masks")
    assert [c.image_name for c in infos] == sorted(c.image_name for c in infos) and len(infos) == 6
    train, test = gsr_data.split_train_test(infos, True, LLFFHOLD)
    assert [c.image_name for c in train] == list(golden["train_names"])
    assert [c.image_name for c in test] == list(golden["test_names"])
    for split, cams in (("train", train), ("test", test)):
        for c in cams:
            g = lambda k: golden[f"{split}/{c.image_name}/{k}"]  # noqa: E731
            assert np.array_equal(c.R, g("R")) and np.array_equal(c.T, g("T"))
            assert c.FovX == float(g("FovX")) and c.FovY == float(g("FovY")) and c.uid == int(g("colmap_id"))
            assert (c.mask_path is not None and os.path.exists(c.mask_path)) == bool(g("has_mask"))
    radius = gsr_data.nerfpp_radius(train)
    assert radius.dtype == golden["radius"].dtype and radius == golden["radius"]
    points, colors = xyz.astype(np.float32), rgb / 255.0
    assert np.array_equal(points, golden["points"]) and np.array_equal(colors, golden["colors"])
    assert gsr_data.split_train_test(infos) == (infos, [])


def test_restatement_gives_the_reference_tensors(golden):
    """PILtoTorch and Camera.__init__ on the golden images at resolution 2 (26 x 18: both halves round to even)
    against resize + planes of the restatement, to the last bit."""
    import gsr_data

    infos, _, _ = gsr_data.read_colmap_cameras(SCENE, "images", "masks")
    masked = 0
    for split, cams in zip(("train", "test"), gsr_data.split_train_test(infos, True, LLFFHOLD)):
        for c in cams:
            g = lambda k: golden[f"{split}/{c.image_name}/{k}"]  # noqa: E731
            rgb, mask = gsr_data._decode(c)
            size = gsr_data.target_resolution(rgb.shape[1], rgb.shape[0], RESOLUTION)
            assert size == (26, 18) == tuple(g("size"))
            original, gray, gt_mask = R.planes(R.resize_u8(rgb, size),
                                               None if mask is None else R.resize_u8(mask[:, :, None], size))
            assert np.array_equal(original, g("original_image")) and np.array_equal(gray, g("gray_image"))
            if mask is not None:
                masked += 1
                assert np.array_equal(gt_mask, g("gt_mask")) and 0 < gt_mask.min() < gt_mask.max() <= 1
            else:
                assert np.all(g("gt_mask") == 1)  # the all-255 mask gsr_data leaves out
    assert masked == 2


def test_reader_refuses_other_camera_models(tmp_path):
    import shutil
    import struct

    import gsr_data

    shutil.copytree(os.path.join(SCENE, "sparse"), tmp_path / "sparse")
    with open(tmp_path / "sparse/0/cameras.bin", "wb") as fh:
        fh.write(struct.pack("<Q", 1) + struct.pack("<IiQQ8d", 1, 4, 53, 37, *([1.0] * 8)))  # OPENCV
    with pytest.raises(AssertionError, match="Colmap camera model not handled: only undistorted datasets"):
        gsr_data.read_colmap_model(str(tmp_path / "sparse/0"))
