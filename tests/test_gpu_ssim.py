"""GPU tests of the fused SSIM (csrc/ssim.hip) against
the float64 restatement of the reference's SSIM (oracle/ssim_ref.py,
utils/loss_utils.py:36-72), in both paddings, with the gradient w.r.t. img1.

Tolerances: |mean_gpu - mean_ref| <= 1e-6; gradient ||a-b|| / ||b|| <= 1e-5
(fp32 separable window sums against float64 conv2d).
"""
from __future__ import annotations

import pytest
import torch

import helpers as Hh
from oracle import ssim_ref

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)


def _pair(shape, seed):
    g = torch.Generator().manual_seed(seed)
    a = torch.rand(shape, generator=g)
    b = (a + 0.1 * torch.randn(shape, generator=g)).clamp(0, 1)  # correlated, like a render and its target
    return a, b


@pytest.mark.parametrize("shape,padding", [((1, 3, 64, 80), "valid"), ((1, 3, 64, 80), "same"),
                                           ((1, 3, 37, 53), "valid"), ((2, 1, 17, 11), "valid"),
                                           ((1, 3, 1080, 1920), "valid")])
def test_fused_ssim_matches_reference(shape, padding):
    import fused_ssim as FS

    a, b = _pair(shape, 0)
    x = a.to(DEV).requires_grad_(True)
    v = FS.fused_ssim(x, b.to(DEV), padding=padding)
    v.backward()
    a64 = a.double().requires_grad_(True)
    r = ssim_ref.ssim(a64, b.double(), padding=padding)
    r.backward()
    assert abs(float(v) - float(r)) <= 1e-6, (float(v), float(r))
    gr = a64.grad
    err = float((x.grad.cpu().double() - gr).norm() / gr.norm())
    assert err <= 1e-5, err


@pytest.mark.parametrize("i", [0, 1, 2])
@pytest.mark.parametrize("padding", ["same", "valid"])
def test_fused_ssim_matches_reference_fixture(i, padding):
    """Against the reference's own _ssim (utils/loss_utils.py:36-72, run in
    fp32 torch by tests/golden/make_golden.py): mean within 1e-6, dSSIM/dimg1
    within 1e-5 relative L2."""
    import os

    import numpy as np

    import fused_ssim as FS

    d = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "losses.npz"))
    x = torch.tensor(d[f"ssim_img1_{i}"], device=DEV).requires_grad_(True)
    v = FS.fused_ssim(x, torch.tensor(d[f"ssim_img2_{i}"], device=DEV), padding=padding)
    v.backward()
    want, g = float(d[f"ssim_{padding}_{i}"]), d[f"ssim_{padding}_grad_{i}"].astype(np.float64)
    assert abs(v.item() - want) <= 1e-6, (v.item(), want)
    assert np.linalg.norm(x.grad.cpu().double().numpy() - g) / np.linalg.norm(g) <= 1e-5


def test_fused_ssim_loss_term_and_no_grad():
    """1 - ssim(...) as train.py:189 uses it; train=False gives the value only."""
    import fused_ssim as FS

    a, b = _pair((1, 3, 48, 48), 1)
    x = a.to(DEV).requires_grad_(True)
    loss = 0.2 * (1.0 - FS.fused_ssim(x.unsqueeze(0)[0], b.to(DEV), padding="valid"))
    loss.backward()
    a64 = a.double().requires_grad_(True)
    (0.2 * (1.0 - ssim_ref.ssim(a64, b.double(), padding="valid"))).backward()
    assert float((x.grad.cpu().double() - a64.grad).norm() / a64.grad.norm()) <= 1e-5
    with torch.no_grad():
        v = FS.fused_ssim(a.to(DEV), b.to(DEV), padding="valid", train=False)
    assert abs(float(v) - float(ssim_ref.ssim(a.double(), b.double(), padding="valid"))) <= 1e-6
    same = FS.fused_ssim(b.to(DEV), b.to(DEV), padding="valid", train=False)
    assert abs(float(same) - 1.0) <= 1e-6


# ---------------------------------------------------------------- edges, per pixel, in the float64 yardstick form
# The yardstick (helpers.Yardstick) is the reference's _ssim restated in fp32 torch (ssim_ref.ssim on fp32
# tensors) against the same in float64.  SSIM_FLOOR: e_gpu measured where that fp32 evaluation is exact, rounded
# up to a power of ten.  SSIM_BAND_FACTOR: the measured worst ratio of the border-band or tile-seam gradient
# error to the error of the remaining pixels over EDGE_SHAPES, doubled.
# Measured on an MI355X: the one comparison with e_fp32 == 0 and e_gpu > 0 is the gradient of two constant 0.5
# images under "valid" padding, e_gpu = 3.5e-8 absolute (torch's conv2d sums cancel exactly there, the kernel's
# separable sums do not): floor 1e-7.  Band ratios between 0.41 and 2.195 (the 11 x 11 image under "same", whose
# remainder is one pixel): factor 4.4.
SSIM_FLOOR = 1e-7
SSIM_BAND_FACTOR = 4.4

EDGE_SHAPES = [((1, 3, 11, 11), "same"), ((1, 3, 11, 11), "valid"), ((1, 3, 11, 75), "same"), ((1, 3, 11, 75), "valid"),
               ((1, 3, 12, 33), "same"), ((1, 3, 12, 33), "valid"), ((1, 3, 16, 32), "same"), ((1, 3, 16, 32), "valid"),
               ((1, 3, 17, 33), "same"), ((1, 3, 17, 33), "valid"), ((1, 3, 5, 7), "same"), ((1, 3, 1, 1), "same"),
               ((1, 3, 47, 95), "same"), ((1, 3, 47, 95), "valid"), ((2, 1, 17, 11), "same")]


def _three_ways(a, b, padding, loss=lambda v: v):
    """(value, dloss/dimg1) of loss(ssim) on the device, in fp32 torch and in float64 torch; a, b are [N,C,H,W]."""
    import fused_ssim as FS

    out = []
    for kind in ("gpu", "fp32", "f64"):
        x = {"gpu": a.to(DEV), "fp32": a.clone(), "f64": a.double()}[kind].requires_grad_(True)
        y = {"gpu": b.to(DEV), "fp32": b, "f64": b.double()}[kind]
        v = FS.fused_ssim(x, y, padding=padding) if kind == "gpu" else ssim_ref.ssim(x, y, padding=padding)
        loss(v).backward()
        assert torch.isfinite(v).all() and torch.isfinite(x.grad).all(), kind
        out.append((float(v), x.grad.detach().cpu().double()))
    return out


def _bands(H, W):
    """(a) the 5-pixel image border, (b) pixels within 5 of a tile seam (a column that is a multiple of 32, a row
    that is a multiple of 16) outside (a), (c) the rest."""
    ys, xs = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
    border = (ys < 5) | (ys >= H - 5) | (xs < 5) | (xs >= W - 5)
    seam = torch.zeros(H, W, dtype=torch.bool)
    for s in range(32, W, 32):  # the seam between columns s - 1 | s
        seam |= (xs >= s - 5) & (xs < s + 5)
    for s in range(16, H, 16):
        seam |= (ys >= s - 5) & (ys < s + 5)
    seam &= ~border
    return border, seam, ~border & ~seam


@pytest.mark.parametrize("shape,padding", EDGE_SHAPES)
def test_fused_ssim_edge_shapes_per_pixel(shape, padding):
    """Value within 1e-6 and gradient within 1e-5 relative L2 as above; then max|g - g_f64| / max|g_f64| apart
    over the border band, the tile-seam band and the remaining pixels: each within the yardstick, and the bands
    no worse than SSIM_BAND_FACTOR times the remainder."""
    a, b = _pair(shape, 2)
    (v, g), (v32, g32), (r, gr) = _three_ways(a, b, padding)
    assert abs(v - r) <= 1e-6, (v, r)
    assert float((g - gr).norm() / gr.norm()) <= 1e-5
    H, W = shape[-2:]
    scale = float(gr.abs().max())
    yard = Hh.Yardstick(f"ssim {shape} {padding}")
    e = {}
    for name, mask in zip(("border", "seam", "rest"), _bands(H, W)):
        if int(mask.sum()) == 0:
            continue
        e[name] = float((g - gr)[..., mask].abs().max()) / scale
        yard.add(name, e[name], float((g32 - gr)[..., mask].abs().max()) / scale, SSIM_FLOOR)
    yard.check()
    if "rest" in e:
        worst = max(e.get("border", 0.0), e.get("seam", 0.0))
        print(f"[band] {shape} {padding}: border {e.get('border')} seam {e.get('seam')} rest {e['rest']} "
              f"ratio {worst / e['rest']:.3f}")
        Hh.record_margins({"band ratio": (worst / e["rest"], SSIM_BAND_FACTOR)}, f"ssim bands {shape} {padding}")
        assert worst <= SSIM_BAND_FACTOR * e["rest"], e


@pytest.mark.parametrize("H,W", [(10, 40), (40, 10), (3, 3)])
def test_fused_ssim_valid_rejects_small_images(H, W):
    import fused_ssim as FS

    a, b = _pair((1, 3, H, W), 3)
    with pytest.raises(RuntimeError):
        FS.fused_ssim(a.to(DEV), b.to(DEV), padding="valid")


def _degenerate(case, shape, seed=4):
    g = torch.Generator().manual_seed(seed)
    rnd = torch.rand(shape, generator=g)
    if case == "identical":
        return rnd, rnd.clone()
    if case.startswith("const="):
        c = torch.full(shape, float(case[6:]))
        return c, c.clone()
    if case == "const_vs_random":
        return torch.full(shape, 0.5), rnd
    a, b = _pair(shape, seed)
    return (a * 1e-3, b * 1e-3) if case == "range1e-3" else (a * 4.0, b * 4.0)


@pytest.mark.parametrize("padding", ["same", "valid"])
@pytest.mark.parametrize("case", ["identical", "const=0", "const=0.5", "const=1", "const_vs_random", "range1e-3",
                                  "range4"])
def test_fused_ssim_degenerate_images(case, padding):
    """Images whose variances cancel in fp32 (identical, constant), where C1 and C2 dominate ([0, 1e-3]) and
    outside the unit range ([0, 4]): nothing is NaN; value and gradient by absolute max against float64 (the relative
    form means nothing where the reference gradient is about 0), in the yardstick form."""
    a, b = _degenerate(case, (1, 3, 37, 53))
    (v, g), (v32, g32), (r, gr) = _three_ways(a, b, padding)
    if case == "identical":
        assert abs(v - 1.0) <= 1e-6
    yard = Hh.Yardstick(f"ssim degenerate {case} {padding}")
    yard.add("value", abs(v - r), abs(v32 - r), SSIM_FLOOR)
    yard.add("grad", float((g - gr).abs().max()), float((g32 - gr).abs().max()), SSIM_FLOOR)
    yard.check()


@pytest.mark.parametrize("case", ["w=-3", "w=1e-6", "squared"])
def test_fused_ssim_upstream_gradient(case):
    loss = (lambda v: v ** 2) if case == "squared" else (lambda v: float(case[2:]) * v)
    a, b = _pair((1, 3, 37, 53), 5)
    (v, g), (v32, g32), (r, gr) = _three_ways(a, b, "valid", loss)
    yard = Hh.Yardstick(f"ssim upstream {case}")
    yard.add("grad", Hh.max_err(g, gr), Hh.max_err(g32, gr), SSIM_FLOOR)
    yard.check()


def _value_and_grad(leaf, view, b, padding):
    import fused_ssim as FS

    v = FS.fused_ssim(view, b, padding=padding)
    v.backward()
    g, leaf.grad = leaf.grad, None
    return v.detach(), g


@pytest.mark.parametrize("padding", ["same", "valid"])
def test_fused_ssim_layouts(padding):
    """[3,H,W] and [H,W] inputs, a channels-last permute, a crop of a larger tensor and a view 4 bytes off a
    16-byte boundary all give what the contiguous [1,3,H,W] copy gives, bit for bit."""
    H, W = 37, 53
    a, b = _pair((1, 3, H, W), 6)
    a, b = a.to(DEV), b.to(DEV)
    x = a.clone().requires_grad_(True)
    want_v, want_g = _value_and_grad(x, x, b, padding)
    # [3, H, W]
    x3 = a[0].clone().requires_grad_(True)
    v, g = _value_and_grad(x3, x3, b[0], padding)
    assert torch.equal(v, want_v) and torch.equal(g, want_g[0])
    # [H, W] against the [1, 1, H, W] copy
    x1 = a[:, :1].clone().requires_grad_(True)
    v1, g1 = _value_and_grad(x1, x1, b[:, :1].contiguous(), padding)
    x2 = a[0, 0].clone().requires_grad_(True)
    v, g = _value_and_grad(x2, x2, b[0, 0].contiguous(), padding)
    assert torch.equal(v, v1) and torch.equal(g, g1[0, 0])
    # channels last
    cl = a.permute(0, 2, 3, 1).contiguous().requires_grad_(True)
    view = cl.permute(0, 3, 1, 2)
    assert not view.is_contiguous()
    v, g = _value_and_grad(cl, view, b, padding)
    assert torch.equal(v, want_v) and torch.equal(g.permute(0, 3, 1, 2), want_g)
    # a crop of a larger tensor
    big = torch.full((1, 3, H + 5, W + 5), 9.0, device=DEV)
    big[..., 3:-2, 1:-4] = a
    big.requires_grad_(True)
    view = big[..., 3:-2, 1:-4]
    assert not view.is_contiguous()
    v, g = _value_and_grad(big, view, b, padding)
    assert torch.equal(v, want_v) and torch.equal(g[..., 3:-2, 1:-4], want_g)
    assert torch.equal(g[..., :3, :], torch.zeros_like(g[..., :3, :]))  # nothing outside the crop
    # 4 bytes off a 16-byte boundary
    flat = torch.zeros(a.numel() + 1, device=DEV)
    flat[1:] = a.flatten()
    flat.requires_grad_(True)
    view = flat[1:].view(a.shape)
    assert view.data_ptr() % 16 == 4
    v, g = _value_and_grad(flat, view, b, padding)
    assert torch.equal(v, want_v) and torch.equal(g[1:].view(a.shape), want_g)


def test_fused_ssim_is_deterministic():
    """The kernel header's claim (partials summed in a fixed order): forward and backward twice, bit-identical."""
    a, b = _pair((1, 3, 47, 95), 7)
    res = []
    for _ in range(2):
        x = a.to(DEV).requires_grad_(True)
        res.append(_value_and_grad(x, x, b.to(DEV), "valid") + _value_and_grad(x, x, b.to(DEV), "same"))
    for p, q in zip(*res):
        assert torch.equal(p, q)
