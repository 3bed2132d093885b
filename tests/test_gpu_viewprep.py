"""GPU tests of the view preparation (gsr_data, csrc/viewprep.hip) against the numpy restatement
(tests/viewprep_ref.py, pinned to PIL.Image.resize by tests/test_viewprep.py) and the reference's own output
for the golden COLMAP scene (tests/golden/make_golden_viewprep.py).

Bars: coefficient tables, bytes, float planes and camera scalars are exact (integer arithmetic, and the same
single float32 operations on both sides).  The one inexact bar is the scale clamp of initial_gaussians: one
float32 ulp of log(0.05 x distance), for torch's log on the device against numpy's.
"""
from __future__ import annotations

import math
import os

import numpy as np
import pytest
import torch

import viewprep_ref as R

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SCENE = os.path.join(GOLDEN, "viewprep_scene")
LLFFHOLD, RESOLUTION = 3, 2  # what make_golden_viewprep.py ran the reference with

# the CPU list, and two output widths that cross a 64-pixel tile with a ragged tail
SHAPES = R.SHAPES + [((70, 300), (33, 65)), ((70, 600), (33, 257))]


def _dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


_WANT = {}


def _want(key, img, size):
    """The restatement's bytes, computed once per case."""
    if key not in _WANT:
        _WANT[key] = R.resize_u8(img, size)
    return _WANT[key]


def _pil_resize(img, size):
    from PIL import Image

    return np.stack([np.asarray(Image.fromarray(img[..., c]).resize(size)) for c in range(img.shape[-1])], -1)


def _have_pil():
    try:
        import PIL  # noqa: F401
        return True
    except ImportError:
        return False


# ---------------------------------------------------------------- tables

def test_coefficient_tables_exact():
    import gsr_data

    for n_in in (1, 2, 7, 53, 64, 1000, 2049):
        for n_out in (1, 2, 13, 65, 100, 257):
            k, bounds = gsr_data.resample_coeffs(n_in, n_out)
            want_k, want_b = R.coeffs(n_in, n_out)
            assert k.shape == want_k.shape and np.array_equal(k, want_k), (n_in, n_out)
            assert np.array_equal(bounds, want_b), (n_in, n_out)


# ---------------------------------------------------------------- bytes

@pytest.mark.parametrize("C", R.CHANNELS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0][0]}x{s[0][1]}to{s[1][0]}x{s[1][1]}")
def test_resize_bytes_exact(shape, C):
    import gsr_data

    (h, w), (oh, ow) = shape
    img = R.random_image((h, w), C, seed=h + w + C)
    got = gsr_data.resize_u8(_dev(img), (ow, oh))
    assert got.dtype == torch.uint8 and tuple(got.shape) == (oh, ow, C)
    got = got.cpu().numpy()
    assert np.array_equal(got, _want((shape, C), img, (ow, oh)))
    if _have_pil():
        assert np.array_equal(got, _pil_resize(img, (ow, oh)))


@pytest.mark.parametrize("C", R.CHANNELS)
@pytest.mark.parametrize("out", R.CHECKER_OUT)
def test_resize_checkerboard_clips_exact(out, C):
    import gsr_data

    img = R.checkerboard(C)
    got = gsr_data.resize_u8(_dev(img), (out[1], out[0])).cpu().numpy()
    assert np.array_equal(got, _want(("checker", out, C), img, (out[1], out[0])))
    if _have_pil():
        assert np.array_equal(got, _pil_resize(img, (out[1], out[0])))


def test_resize_layouts_and_copy():
    """[H,W] is `L`, [N,H,W,C] a batch; an unchanged size returns a copy, not the input."""
    import gsr_data

    img = R.random_image((17, 19), 1, seed=5)
    x = _dev(img[:, :, 0])
    got = gsr_data.resize_u8(x, (7, 11))
    assert tuple(got.shape) == (11, 7) and np.array_equal(got.cpu().numpy(), R.resize_u8(img, (7, 11))[:, :, 0])
    same = gsr_data.resize_u8(x, (19, 17))
    assert same.data_ptr() != x.data_ptr() and torch.equal(same, x)


def test_batch_independence():
    import gsr_data

    imgs = np.stack([R.random_image((37, 53), 3, seed=s) for s in (1, 2, 3)])
    batch = gsr_data.resize_u8(_dev(imgs), (13, 9))
    assert tuple(batch.shape) == (3, 9, 13, 3)
    for n in range(3):
        alone = gsr_data.resize_u8(_dev(imgs[n]), (13, 9))
        assert torch.equal(batch[n], alone)
        assert np.array_equal(alone.cpu().numpy(), R.resize_u8(imgs[n], (13, 9)))


# ---------------------------------------------------------------- planes

def test_view_planes_bit_exact():
    """[3,37,65] holding all 256 byte values in every channel (each channel its own permutation, repeated)."""
    import gsr_data

    rng = np.random.default_rng(0)
    n = 37 * 65
    rgb = np.stack([np.concatenate([rng.permutation(256) for _ in range(n // 256 + 1)])[:n] for _ in range(3)],
                   -1).astype(np.uint8).reshape(37, 65, 3)
    mask = np.concatenate([rng.permutation(256) for _ in range(n // 256 + 1)])[:n].astype(np.uint8).reshape(37, 65)
    for c in range(3):
        assert len(np.unique(rgb[:, :, c])) == 256
    assert len(np.unique(mask)) == 256
    original, gray, gt_mask = gsr_data.view_planes(_dev(rgb[None]), _dev(mask[None]))
    assert tuple(original.shape) == (1, 3, 37, 65) and tuple(gray.shape) == tuple(gt_mask.shape) == (1, 1, 37, 65)
    want_o, want_g, want_m = R.planes(rgb, mask)
    assert np.array_equal(original[0].cpu().numpy(), np.moveaxis(rgb, -1, 0) / np.float32(255))
    assert np.array_equal(original[0].cpu().numpy(), want_o)
    assert np.array_equal(gray[0].cpu().numpy(), want_g)
    assert np.array_equal(gt_mask[0].cpu().numpy(), mask[None] / np.float32(255))
    assert np.array_equal(gt_mask[0].cpu().numpy(), want_m)
    o2, g2, m2 = gsr_data.view_planes(_dev(rgb[None]))
    assert m2 is None and torch.equal(o2, original) and torch.equal(g2, gray)


# ---------------------------------------------------------------- end to end

@pytest.fixture(scope="module")
def scene():
    import gsr_data

    return gsr_data.load_colmap_scene(SCENE, masks="masks", eval=True, llffhold=LLFFHOLD, resolution=RESOLUTION,
                                      device=DEV, batch=3)


def test_scene_views_against_the_reference(scene):
    golden = np.load(os.path.join(GOLDEN, "viewprep.npz"))
    assert [v.image_name for v in scene.train_views] == list(golden["train_names"])
    assert [v.image_name for v in scene.test_views] == list(golden["test_names"])
    assert np.float32(scene.cameras_extent) == golden["radius"]
    assert np.array_equal(scene.points, golden["points"]) and np.array_equal(scene.colors, golden["colors"])
    masked = 0
    for split, views in (("train", scene.train_views), ("test", scene.test_views)):
        for idx, v in enumerate(views):
            g = lambda k: golden[f"{split}/{v.image_name}/{k}"]  # noqa: E731
            assert (v.image_width, v.image_height) == tuple(g("size")) == (26, 18) and v.uid == idx == int(g("uid"))
            assert np.array_equal(v.original_image.cpu().numpy(), g("original_image"))
            assert np.array_equal(v.gray_image.cpu().numpy(), g("gray_image"))
            if bool(g("has_mask")):
                masked += 1
                assert np.array_equal(v.gt_mask.cpu().numpy(), g("gt_mask"))
            else:
                assert v.gt_mask is None and np.all(g("gt_mask") == 1)  # the documented deviation
            scalars = np.array([v.Fx, v.Fy, v.Cx, v.Cy, v.FoVx, v.FoVy, 0.01, 100.0])
            assert np.array_equal(scalars, g("scalars"))
            assert np.array_equal(v.R.cpu().numpy(), g("R32")) and np.array_equal(v.T.cpu().numpy(), g("T32"))
            for name in ("world_view_transform", "full_proj_transform", "camera_center"):
                assert np.allclose(getattr(v, name).cpu().numpy(), g(name), rtol=1e-6, atol=1e-6), name
    assert masked == 2


def test_scene_nearest_views(scene):
    import gsr_data

    views = scene.train_views
    max_angle, min_dis, max_dis, num = 30, 0.3, 1.5, 2
    centers = np.stack([v.camera_center.cpu().numpy() for v in views])
    rot = np.stack([v.R.cpu().numpy() for v in views])
    want, diss, angles = R.nearest_views(centers, rot, max_angle, min_dis, max_dis, num)
    R.assert_gaps(diss, angles, max_angle, min_dis, max_dis)
    assert gsr_data.nearest_views(views, max_angle, min_dis, max_dis, num) == want
    assert any(want) and all(i not in ids for i, ids in enumerate(want))


def test_initial_gaussians_and_one_step(scene):
    import gsr_data
    import gsr_train

    views = scene.train_views
    raw = gsr_data.initial_gaussians(scene.points, scene.colors, views, sh_degree=3, sg_degree=2,
                                     generator=torch.Generator(device=DEV).manual_seed(0))
    P = scene.points.shape[0]
    shapes = {"xyz": (P, 3), "features_dc": (P, 1, 3), "features_rest": (P, 15, 3), "scaling": (P, 3),
              "rotation": (P, 4), "opacity": (P, 1), "sg_axis": (P, 2, 3), "sg_sharpness": (P, 2),
              "sg_color": (P, 2, 3), "filter_3D": (P, 1)}
    for name, shape in shapes.items():
        t = getattr(raw, name)
        assert tuple(t.shape) == shape and t.dtype == torch.float32 and t.device == DEV, name
    assert np.array_equal(raw.xyz.cpu().numpy(), scene.points)
    want_dc = (torch.tensor(scene.colors).float() - 0.5) / 0.28209479177387814
    # (rgb - 0.5) / C0 on the device against the host: one float32 rounding of the quotient apart at most
    assert torch.allclose(raw.features_dc.cpu()[:, 0], want_dc, rtol=2.5e-7, atol=0) and not raw.features_rest.any()
    want_opacity = torch.log(torch.tensor(0.1) / (1 - torch.tensor(0.1)))  # inverse_sigmoid(0.1)
    assert torch.allclose(raw.opacity.cpu(), want_opacity.expand(P, 1), rtol=0, atol=1e-6)
    assert torch.equal(raw.rotation.cpu(), torch.tensor([1.0, 0, 0, 0]).expand(P, 4))
    assert torch.allclose(raw.sg_axis.norm(dim=2).cpu(), torch.ones(P, 2), atol=1e-5)
    assert torch.equal(raw.scaling[:, 0], raw.scaling[:, 1]) and torch.equal(raw.scaling[:, 0], raw.scaling[:, 2])
    # the clamp: log(0.05 x the distance to the nearest camera), float64 on the host, one float32 ulp of it
    centers = np.stack([v.camera_center.cpu().numpy() for v in views]).astype(np.float64)
    dist = np.linalg.norm(scene.points.astype(np.float64)[:, None] - centers[None], axis=-1).min(axis=1)
    bound = np.log(0.05 * dist)
    ulp = np.spacing(np.abs(bound).astype(np.float32)).astype(np.float64)
    scaling = raw.scaling[:, 0].cpu().numpy().astype(np.float64)
    assert np.all(scaling <= bound + ulp), float((scaling - bound).max())
    assert np.isfinite(scaling).all()

    g = gsr_train.TrainGaussians(raw.to(DEV), spatial_lr_scale=scene.cameras_extent, sh_degree=3, sg_degree=2)
    g.compute_3D_filter(views)
    unmasked = [v for v in views if v.gt_mask is None][:2]
    assert len(unmasked) == 2
    loss = gsr_train.TrainStep(g).step(unmasked[0], unmasked[1])
    assert math.isfinite(float(loss))


# ---------------------------------------------------------------- argument errors

def test_argument_errors():
    import gsr_data

    img = _dev(R.random_image((9, 11), 3))
    with pytest.raises(RuntimeError, match="resize_u8: `image_u8` must be torch.uint8"):
        gsr_data.resize_u8(img.float(), (5, 4))
    with pytest.raises(RuntimeError, match="resize_u8: `image_u8` must be a HIP device tensor"):
        gsr_data.resize_u8(img.cpu(), (5, 4))
    with pytest.raises(RuntimeError, match="resize_u8: `image_u8` must have 1 to 4 channels"):
        gsr_data.resize_u8(_dev(R.random_image((9, 11), 5)), (5, 4))
    for size in ((0, 4), (5, 0), (5, -1)):
        with pytest.raises(RuntimeError, match="resize_u8: `size` must be"):
            gsr_data.resize_u8(img, size)
    eye, zero = np.eye(3), np.zeros(3)
    with pytest.raises(RuntimeError, match="prepare_view: `mask_u8` must have the size of `rgb_u8`"):
        gsr_data.prepare_view(img, eye, zero, 1.0, 0.8, mask_u8=_dev(R.random_image((9, 10), 1)), device=DEV)
    with pytest.raises(RuntimeError, match="prepare_view: `rgb_u8` must be uint8"):
        gsr_data.prepare_view(img.float(), eye, zero, 1.0, 0.8, device=DEV)
    with pytest.raises(RuntimeError, match="view_planes: `mask_u8` must have the size of `rgb_u8`"):
        gsr_data.view_planes(img[None], _dev(R.random_image((9, 10), 1))[None, :, :, 0])


def test_c_abi_argument_errors():
    """The checks of the C entry points themselves (a caller that goes round gsr_data)."""
    from diff_gaussian_rasterization._abi import call, ptr, stream

    a = torch.zeros(64, dtype=torch.uint8, device=DEV)
    t = torch.zeros(64, dtype=torch.int32, device=DEV)
    with pytest.raises(RuntimeError, match="image_resample8: `C` must be 1, 2, 3 or 4"):
        call(DEV, "gsr_image_resample8", 1, 2, 2, 5, 1, 2, ptr(a), ptr(a), ptr(t), ptr(t), stream(DEV))
    with pytest.raises(RuntimeError, match="image_resample8: `out_size` must be"):
        call(DEV, "gsr_image_resample8", 1, 2, 2, 3, 1, 0, ptr(a), ptr(a), ptr(t), ptr(t), stream(DEV))
    with pytest.raises(RuntimeError, match="image_resample8: `axis` must be"):
        call(DEV, "gsr_image_resample8", 1, 2, 2, 3, 2, 2, ptr(a), ptr(a), ptr(t), ptr(t), stream(DEV))


def test_prepare_view_is_the_scene_view(scene):
    """prepare_view on one decoded image gives what the batched scene loader gave (an RGBA file: alpha dropped)."""
    import gsr_data

    infos, _, _ = gsr_data.read_colmap_cameras(SCENE, "images", "masks")
    info = next(c for c in infos if c.image_name == "view_f")
    rgb, mask = gsr_data._decode(info)
    from PIL import Image
    with Image.open(info.image_path) as im:
        rgba = np.asarray(im)
    assert rgba.shape[2] == 4 and mask is None
    v = gsr_data.prepare_view(rgba, info.R, info.T, info.FovX, info.FovY, resolution=RESOLUTION, uid=7,
                              image_name=info.image_name, device=DEV)
    ref = next(w for w in scene.train_views if w.image_name == "view_f")
    assert v.uid == 7 and v.gt_mask is None
    assert torch.equal(v.original_image, ref.original_image) and torch.equal(v.gray_image, ref.gray_image)
    assert torch.equal(v.full_proj_transform, ref.full_proj_transform)
