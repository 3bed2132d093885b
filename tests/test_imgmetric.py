"""The numpy restatement of the image-quality tail (tests/imgmetric_ref.py) against the reference's own
expressions run with torch on the CPU, and the host half of gsr_metric (PNG round trip, evaluate's files).
No device is needed: evaluate() is handed the restatement through its `score_fn` injection point."""
from __future__ import annotations

import json
import os

import numpy as np
import pytest
import torch

import imgmetric_ref as R

SHAPES = [(1, 3, 11, 11), (2, 3, 13, 17), (1, 1, 27, 43), (3, 4, 12, 26)]


def test_bytes_equal_torch_chain():
    """x.mul(255).add_(0.5).clamp_(0, 255).to(uint8), on the edge image (every byte boundary with its
    neighbours, NaN, +-inf) and on two million uniform values."""
    e = R.edge_image()
    assert np.array_equal(R.quantize8(e[0]), R.torch_bytes(torch.from_numpy(e[0])).numpy())
    u = np.random.default_rng(2).random((1, 2, 1000, 1000), dtype=np.float32)
    assert np.array_equal(R.quantize8(u[0]), R.torch_bytes(torch.from_numpy(u[0])).numpy())
    # the special values, spelt out
    s = np.array([np.nan, np.inf, -np.inf, -0.0, 1e-41, -1.0, 2.0], dtype=np.float32).reshape(1, 1, 7)
    assert R.quantize8(s).ravel().tolist() == [0, 255, 0, 0, 0, 0, 255]


def test_separate_roundings_matter():
    """The contract's subtle part: x * 255 + 0.5 evaluated without the two float32 roundings (in float64)
    lands on another byte for a few values in a million."""
    u = np.random.default_rng(3).random(2_000_000, dtype=np.float32)
    fused = np.clip(u.astype(np.float64) * 255.0 + 0.5, 0, 255).astype(np.uint8)
    differ = int((fused != R.quantize_planes(u)).sum())
    assert 0 < differ < 200, differ


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("quantize", [True, False])
def test_metrics_equal_reference_expressions_in_float64(shape, quantize):
    """PSNR against utils/image_utils.py:18-20, L1 against l1_loss and SSIM against _ssim
    (loss_utils.py:52-72) with padding=0, each evaluated in float64: 1e-12.  SSIM and the float mode take the
    compared float32 values.  The quantised L1 and PSNR are exact integer sums over the bytes, so the
    reference's expressions are given the bytes' exact values byte / 255 in float64; on the float32-rounded
    byte / 255 (one more rounding per value, 2^-24 relative) they move by about 1e-8 dB, which is printed."""
    a, b = R.pair(shape, seed=sum(shape), spread=0.0 if quantize else 0.3)
    m = R.metrics(a, b, quantize=quantize)
    ta = torch.from_numpy(R.compared(a, quantize)).double()
    tb = torch.from_numpy(R.compared(b, quantize)).double()
    assert np.abs(m["SSIM"] - R.torch_ssim(ta, tb).numpy()).max() <= 1e-12
    if quantize:
        print("PSNR on float32 byte / 255:", np.abs(m["PSNR"] - R.torch_psnr(ta, tb).numpy()).max(), "dB")
        ta = torch.from_numpy(R.quantize_planes(a)).double() / 255.0
        tb = torch.from_numpy(R.quantize_planes(b)).double() / 255.0
    assert np.abs(m["PSNR"] - R.torch_psnr(ta, tb).numpy()).max() <= 1e-12
    assert np.abs(m["L1"] - R.torch_l1(ta, tb).numpy()).max() <= 1e-12


def test_identical_images():
    a, _ = R.pair((1, 3, 12, 12), 0)
    m = R.metrics(a, a)
    assert m["L1"][0] == 0 and np.isinf(m["PSNR"][0]) and abs(1 - m["SSIM"][0]) <= 1e-12
    z = torch.from_numpy(R.compared(a, True)).double()
    assert torch.isinf(R.torch_psnr(z, z)).all()  # the reference: 20 log10(1 / 0)


def _write_pairs(root, method, pairs):
    from gsr_metric import _save_png

    for sub in ("renders", "gt"):
        os.makedirs(os.path.join(root, "test", method, sub))
    for k, (a, b) in enumerate(pairs):
        _save_png(os.path.join(root, "test", method, "renders", f"{k:05d}.png"), torch.from_numpy(R.quantize8(a)))
        _save_png(os.path.join(root, "test", method, "gt", f"{k:05d}.png"), torch.from_numpy(R.quantize8(b)))


def test_png_round_trip_is_exact(tmp_path):
    """PIL writes and reads the bytes unchanged, for 1, 3 and 4 channels; _read_png gives byte / 255 in
    float32 cut to three channels, and quantising that gives the byte back."""
    from PIL import Image

    from gsr_metric import _read_png, _save_png

    for C in (1, 3, 4):
        x = np.random.default_rng(C).random((C, 9, 14), dtype=np.float32)
        q = R.quantize8(x)
        path = str(tmp_path / f"c{C}.png")
        _save_png(path, torch.from_numpy(q))
        back = np.asarray(Image.open(path))
        assert np.array_equal(back.reshape(9, 14, C), q)
        t = _read_png(path)
        assert t.dtype == torch.float32 and tuple(t.shape) == (min(C, 3), 9, 14)
        assert np.array_equal(t.numpy(), (q.astype(np.float32) / np.float32(255)).transpose(2, 0, 1)[:3])
        assert np.array_equal(R.quantize8(t.numpy()), q[..., :3])


def test_evaluate_writes_the_reference_layout(tmp_path):
    """evaluate() on a hand-made directory of two 12 x 13 PNG pairs: results.json {method: {"SSIM", "PSNR"}}
    with the plain means, per_view.json {method: {"SSIM": {name: v}, "PSNR": {name: v}}}, five-digit names; a
    "LPIPS" entry only with lpips_fn."""
    import gsr_metric

    pairs = [tuple(x[0] for x in R.pair((1, 3, 12, 13), seed)) for seed in (5, 6)]
    _write_pairs(str(tmp_path), "ours_7", pairs)

    def score(render, gt):
        m = R.metrics(render[None].numpy(), gt[None].numpy())
        return m["SSIM"][0], m["PSNR"][0]

    full, per_view = gsr_metric.evaluate(str(tmp_path), score_fn=score)
    want = [R.metrics(a[None], b[None]) for a, b in pairs]
    names = ["00000.png", "00001.png"]
    assert json.load(open(tmp_path / "results.json")) == full
    assert json.load(open(tmp_path / "per_view.json")) == per_view
    assert list(full) == ["ours_7"] and set(full["ours_7"]) == {"SSIM", "PSNR"}
    assert set(per_view["ours_7"]) == {"SSIM", "PSNR"}
    for key in ("SSIM", "PSNR"):
        assert list(per_view["ours_7"][key]) == names
        vals = [float(w[key][0]) for w in want]
        assert [per_view["ours_7"][key][n] for n in names] == vals  # the PNG pair is the quantised pair
        assert full["ours_7"][key] == float(np.mean(vals))
    full, per_view = gsr_metric.evaluate(str(tmp_path), lpips_fn=lambda r, g: 0.25, device="cpu", score_fn=score)
    assert full["ours_7"]["LPIPS"] == 0.25 and per_view["ours_7"]["LPIPS"] == dict.fromkeys(names, 0.25)
