"""GPU tests of the image-quality tail (gsr_metric, csrc/imgmetric.hip) against the numpy restatement
(tests/imgmetric_ref.py, pinned to the reference's expressions by tests/test_imgmetric.py).

Bars.  Bytes: exact.  Quantised L1 / MSE: 1e-15 relative (the same integers and the same two float64
operations on both sides), PSNR 1e-12 dB.  SSIM: helpers.Yardstick against the float64 restatement with e_fp32
from the reference's _ssim in float32 torch, and 1e-6 absolute per image (the bar test_gpu_ssim.py holds
fused_ssim to).  SSIM_FLOOR: the kernel's window sums are float64, so what separates it from the restatement is
the window itself: the kernel applies the two float32 1-D weights one after the other (their exact product)
where the reference rounds the 2-D product to float32, 2^-24 = 6e-8 relative per weight on sums of values in
[0, 1], rounded up to 1e-7.  Float mode: Yardstick with e_fp32 from
torch.abs(a - b).mean() and the reference's psnr in float32; the floors are one float32 rounding of each
difference (2^-24 = 6e-8 relative on L1, rounded up to 1e-7; twice that on the MSE, 10 log10(1 + 1.2e-7) =
5.2e-7 dB, rounded up to 1e-6 dB).
"""
from __future__ import annotations

import json
import os

import numpy as np
import pytest
import torch

import helpers as Hh
import imgmetric_ref as R

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
SSIM_FLOOR = 1e-7
L1_FLOOR, PSNR_FLOOR_DB = 1e-7, 1e-6


def _dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


# ---------------------------------------------------------------- quantise, exact

def test_quantize8_edge_image_exact():
    """Every byte boundary with its float32 neighbours, -0.0, a denormal, out-of-range values, NaN and +-inf:
    the bytes are the restatement's everywhere, channels interleaved (out[y, x, c])."""
    import gsr_metric

    e = R.edge_image()
    out = gsr_metric.quantize8(_dev(e))
    assert out.dtype == torch.uint8 and tuple(out.shape) == (1, 32, 32, 3)
    got = out.cpu().numpy()
    assert np.array_equal(got, R.quantize8(e))
    planes = R.quantize_planes(e)
    for c in range(3):
        assert np.array_equal(got[0, :, :, c], planes[0, c])
    single = gsr_metric.quantize8(_dev(e[0]))  # [C,H,W] -> [H,W,C]
    assert tuple(single.shape) == (32, 32, 3) and np.array_equal(single.cpu().numpy(), got[0])


@pytest.mark.parametrize("shape", [(2, 3, 13, 17), (1, 1, 1, 1), (1, 4, 5, 7), (3, 2, 3, 5)])
def test_quantize8_packed_store_tails(shape):
    """Byte counts that are no multiple of the packed store (1326, 1, 140, 90 bytes) and 1, 2, 4 channels."""
    import gsr_metric

    x = np.random.default_rng(sum(shape)).random(shape, dtype=np.float32) * 1.2 - 0.1
    assert np.array_equal(gsr_metric.quantize8(_dev(x)).cpu().numpy(), R.quantize8(x))


# ---------------------------------------------------------------- integer sums

def _check_quantised_sums(m, want):
    """L1 and MSE 1e-15 relative, PSNR 1e-12 dB (inf where the restatement's is)."""
    for k in ("L1", "MSE"):
        assert np.all(np.abs(m[k].numpy() - want[k]) <= 1e-15 * np.abs(want[k])), (k, m[k], want[k])
    psnr, wp = m["PSNR"].numpy(), want["PSNR"]
    assert np.array_equal(np.isinf(psnr), np.isinf(wp))
    fin = np.isfinite(wp)
    assert np.all(np.abs(psnr[fin] - wp[fin]) <= 1e-12), (psnr, wp)


def test_integer_sums_past_32_bits():
    """All-1.0 against all-0.0 at [1,3,160,160]: 76 800 values, sum of squares 255^2 * 76800 > 2^32."""
    import gsr_metric

    a, b = np.ones((1, 3, 160, 160), np.float32), np.zeros((1, 3, 160, 160), np.float32)
    assert 255 * 255 * a.size > 2 ** 32
    m = gsr_metric.image_metrics(_dev(a), _dev(b), ssim=False)
    assert set(m) == {"L1", "MSE", "PSNR"} and m["L1"].dtype == torch.float64 and m["L1"].device.type == "cpu"
    assert float(m["L1"][0]) == 1.0 and float(m["MSE"][0]) == 1.0 and float(m["PSNR"][0]) == 0.0


@pytest.mark.parametrize("shape", [(1, 3, 160, 160), (3, 3, 27, 43), (2, 1, 5, 7), (1, 5, 33, 70)])
def test_quantised_sums_equal_the_restatement(shape):
    import gsr_metric

    a, b = R.pair(shape, seed=11 + sum(shape), spread=0.1)
    want = R.metrics(a, b, quantize=True, ssim=False)
    if shape[1] <= 4:
        m, qa, qb = gsr_metric.image_metrics(_dev(a), _dev(b), ssim=False, return_bytes=True)
        assert np.array_equal(qa.cpu().numpy(), R.quantize8(a)) and np.array_equal(qb.cpu().numpy(), R.quantize8(b))
    else:
        m = gsr_metric.image_metrics(_dev(a), _dev(b), ssim=False)
    _check_quantised_sums(m, want)


def test_identical_images():
    import gsr_metric

    a, _ = R.pair((2, 3, 27, 43), 5)
    m = gsr_metric.image_metrics(_dev(a), _dev(a))
    assert torch.all(m["L1"] == 0) and torch.all(torch.isinf(m["PSNR"])) and torch.all(m["PSNR"] > 0)
    assert torch.all((1.0 - m["SSIM"]).abs() <= 1e-6), m["SSIM"]
    m = gsr_metric.image_metrics(_dev(a), _dev(a), quantize=False)
    assert torch.all(m["L1"] == 0) and torch.all(torch.isinf(m["PSNR"]))
    assert torch.all((1.0 - m["SSIM"]).abs() <= 1e-6), m["SSIM"]


# ---------------------------------------------------------------- SSIM per image

# the kernel's tile is 32 x 16 window positions: 26 x 42 is exactly one tile, 27 x 43 one position past it
SSIM_SHAPES = [(11, 11), (11, 43), (12, 26), (26, 12), (27, 27), (43, 12), (26, 42), (27, 43), (64, 48)]


@pytest.mark.parametrize("quantize", [True, False])
@pytest.mark.parametrize("N", [1, 3])
@pytest.mark.parametrize("H,W", SSIM_SHAPES)
def test_ssim_per_image(H, W, N, quantize):
    import gsr_metric

    a, b = R.pair((N, 3, H, W), seed=H * 100 + W + N, spread=0.0 if quantize else 0.2)
    want = R.metrics(a, b, quantize=quantize)
    ca, cb = torch.from_numpy(R.compared(a, quantize)), torch.from_numpy(R.compared(b, quantize))
    ref32 = R.torch_ssim(ca, cb).double().numpy()
    m, qa, qb = (gsr_metric.image_metrics(_dev(a), _dev(b), quantize=quantize, return_bytes=True) if quantize
                 else (gsr_metric.image_metrics(_dev(a), _dev(b), quantize=False), None, None))
    got = m["SSIM"].numpy()
    assert got.shape == (N,) and m["SSIM"].dtype == torch.float64
    yard = Hh.Yardstick(f"imgmetric ssim {(N, 3, H, W)} quantize={quantize}")
    for i in range(N):
        print(f"[ssim] image {i}: gpu {got[i]!r} f64 {want['SSIM'][i]!r} fp32 {ref32[i]!r}")
        yard.add(f"ssim[{i}]", abs(got[i] - want["SSIM"][i]), abs(ref32[i] - want["SSIM"][i]), SSIM_FLOOR)
    yard.check()
    assert np.all(np.abs(got - want["SSIM"]) <= 1e-6), (got, want["SSIM"])
    if quantize:  # the same call: bytes and exact sums beside the SSIM
        assert np.array_equal(qa.cpu().numpy(), R.quantize8(a)) and np.array_equal(qb.cpu().numpy(), R.quantize8(b))
        _check_quantised_sums(m, want)
    if N == 3:  # an image's numbers do not depend on the rest of the batch: bit-identical alone
        alone = gsr_metric.image_metrics(_dev(a[1:2]), _dev(b[1:2]), quantize=quantize)
        for k in ("L1", "PSNR", "SSIM"):
            assert torch.equal(alone[k], m[k][1:2]), k


# ---------------------------------------------------------------- float mode

@pytest.mark.parametrize("shape", [(1, 3, 24, 40), (3, 3, 27, 43), (2, 1, 5, 7)])
def test_float_mode_l1_and_psnr(shape):
    """Images reaching outside [0, 1] (so the clamps matter) against float64, in the yardstick form."""
    import gsr_metric

    a, b = R.pair(shape, seed=21 + sum(shape), spread=0.3)
    assert (a < 0).any() and (a > 1).any() and (b < 0).any() and (b > 1).any()
    want = R.metrics(a, b, quantize=False, ssim=False)
    unclamped = R.torch_l1(torch.from_numpy(a).double(), torch.from_numpy(b).double()).numpy()
    assert np.all(np.abs(unclamped - want["L1"]) > 1e-3)  # the clamp is visible in the number
    ca, cb = torch.from_numpy(R.compared(a, False)), torch.from_numpy(R.compared(b, False))
    l1_32, psnr_32 = R.torch_l1(ca, cb).double().numpy(), R.torch_psnr(ca, cb).double().numpy()
    m = gsr_metric.image_metrics(_dev(a), _dev(b), quantize=False, ssim=False)
    assert set(m) == {"L1", "MSE", "PSNR"}
    yard = Hh.Yardstick(f"imgmetric float mode {shape}")
    for i in range(shape[0]):
        yard.add(f"l1[{i}]", abs(float(m["L1"][i]) - want["L1"][i]) / want["L1"][i],
                 abs(l1_32[i] - want["L1"][i]) / want["L1"][i], L1_FLOOR)
        yard.add(f"psnr_db[{i}]", abs(float(m["PSNR"][i]) - want["PSNR"][i]), abs(psnr_32[i] - want["PSNR"][i]),
                 PSNR_FLOOR_DB)
    yard.check()


# ---------------------------------------------------------------- errors

def test_errors_name_the_argument():
    import gsr_metric

    a, b = (torch.rand(1, 3, 10, 40, device=DEV) for _ in range(2))
    with pytest.raises(RuntimeError, match="`render`.*SSIM"):
        gsr_metric.image_metrics(a, b)
    assert set(gsr_metric.image_metrics(a, b, ssim=False)) == {"L1", "MSE", "PSNR"}  # without SSIM any size goes
    with pytest.raises(RuntimeError, match="`render` and `gt`.*same shape"):
        gsr_metric.image_metrics(a, b[..., :39], ssim=False)
    with pytest.raises(RuntimeError, match="`gt`"):
        gsr_metric.image_metrics(a, b.cpu(), ssim=False)
    with pytest.raises(RuntimeError, match="`render`"):
        gsr_metric.image_metrics(a.cpu(), b, ssim=False)
    with pytest.raises(RuntimeError, match="`image`"):
        gsr_metric.quantize8(a.cpu())
    with pytest.raises(RuntimeError, match="`image`"):
        gsr_metric.quantize8(a.double())
    # the library's own check, through gsr_last_error
    from diff_gaussian_rasterization._abi import Out, call, ptr, stream

    out = torch.zeros(1, 3, dtype=torch.float64, device=DEV)
    with pytest.raises(RuntimeError, match="image_metrics: SSIM needs H and W of at least 11"):
        call(DEV, "gsr_image_metrics", Out(DEV, torch.uint8).cb, None, 1, 3, 10, 40, 1, 1, ptr(a), ptr(b), None, None,
             ptr(out), stream(DEV))


# ---------------------------------------------------------------- the tail end to end

def test_render_set_evaluate_and_report(tmp_path):
    """render.py -> metric.py on helpers.small_case-sized Gaussians (40 x 24) and three orbit views whose
    original_image is a render of perturbed Gaussians: six PNGs, and evaluate() returns exactly the numbers
    render_set returned (PNG is lossless, quantising byte / 255 gives the byte back)."""
    import gsr_metric
    import gsr_scene as S
    import gsr_train
    from gaussian_renderer import render

    W, H = 40, 24
    raw = Hh.small_case(P=40, W=W, H=H)["raw"].to(DEV)
    views = gsr_train.orbit_views(3, W, H, DEV)
    gen = torch.Generator().manual_seed(1)
    gt_raw = S.RawGaussians(*[getattr(raw, f).clone() for f in raw.__dataclass_fields__])
    gt_raw.features_dc += (torch.randn(gt_raw.features_dc.shape, generator=gen) * 0.1).to(DEV)
    gt_raw.xyz += (torch.randn(gt_raw.xyz.shape, generator=gen) * 0.01).to(DEV)
    pipe, bg = gsr_train._Pipe(), torch.zeros(3, device=DEV)
    with torch.no_grad():
        gt_pc = gsr_train.TrainGaussians(gt_raw)
        for v in views:  # (not clamped: the report's clamp and the quantiser's have something to do)
            v.original_image = render(v, gt_pc, pipe, bg, 0.0, require_depth=False)["render"].contiguous()
    pc = gsr_train.TrainGaussians(raw)

    out_dir = tmp_path / "test" / "ours_1"
    per = gsr_metric.render_set(str(out_dir), views, pc, pipe, bg, 0.0)
    assert sorted(os.listdir(out_dir / "renders")) == sorted(os.listdir(out_dir / "gt")) == \
        ["00000.png", "00001.png", "00002.png"]
    assert all(per[k].shape == (3,) and per[k].dtype == torch.float64 for k in ("L1", "PSNR", "SSIM"))
    assert torch.all(per["L1"] > 0) and torch.all(torch.isfinite(per["PSNR"]))  # the views differ from their targets
    nofiles = gsr_metric.render_set(None, views, pc, pipe, bg, 0.0)
    for k in per:
        assert torch.equal(nofiles[k], per[k]), k

    full, per_view = gsr_metric.evaluate(str(tmp_path))
    assert json.load(open(tmp_path / "results.json")) == full
    assert json.load(open(tmp_path / "per_view.json")) == per_view
    assert list(full) == ["ours_1"] and set(full["ours_1"]) == {"SSIM", "PSNR"}
    assert set(per_view["ours_1"]) == {"SSIM", "PSNR"}
    for k in ("SSIM", "PSNR"):
        assert list(per_view["ours_1"][k]) == ["00000.png", "00001.png", "00002.png"]
        assert list(per_view["ours_1"][k].values()) == per[k].tolist(), k
        assert full["ours_1"][k] == float(np.mean(per[k].numpy()))

    l1, psnr = gsr_metric.report(views, pc, pipe, bg, 0.0)
    rows = [gsr_metric.image_metrics(render(v, pc, pipe, bg, 0.0)["render"].detach(), v.original_image,
                                     quantize=False, ssim=False) for v in views]
    assert l1 == float(torch.cat([r["L1"] for r in rows]).mean())
    assert psnr == float(torch.cat([r["PSNR"] for r in rows]).mean())
    assert l1 > 0 and np.isfinite(psnr)
