"""GPU tests of depth_to_normal (csrc/depth_normal.hip)
against the float64 restatement of utils/graphics_utils.py:103-119
(oracle/ssim_ref.py), forward and autograd backward.

Tolerances: valid exact; normals (max abs) and dL/ddepth (relative L2): the
error against the float64 values is at most twice that of the reference's own
fp32 torch arithmetic (or 1e-5) — the central differences of back-projected
fp32 points cancel at 1080p.
"""
from __future__ import annotations

import pytest
import torch

import helpers as Hh
from oracle import ssim_ref

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)


class View:
    def __init__(self, W, H):
        self.image_width, self.image_height = W, H
        self.Fx, self.Fy, self.Cx, self.Cy = 0.9 * W, 0.9 * W, W / 2 - 0.5, H / 2 + 0.25


@pytest.mark.parametrize("W,H", [(40, 30), (1920, 1080)])
def test_depth_to_normal_matches_reference(W, H):
    import gsr_geometry as G

    g = torch.Generator().manual_seed(0)
    base = torch.rand(1, 1, H // 8 + 2, W // 8 + 2, generator=g) * 3 + 2
    depth = torch.nn.functional.interpolate(base, size=(H, W), mode="bicubic", align_corners=True)[0]
    depth[:, : H // 7, : W // 5] = 0.0  # holes (median depth 0 where undefined)
    depth = depth.float().contiguous()
    view = View(W, H)
    d = depth.to(DEV).requires_grad_(True)
    n, valid = G.depth_to_normal(view, d)
    # the depth-normal loss masks by `valid` (train.py:174-180); unmasked, the
    # degenerate cross products at hole edges take F.normalize's 1/eps branch
    gn = torch.randn(3, H, W, generator=g) * valid.cpu()
    (n * gn.to(DEV)).sum().backward()
    d64 = depth.double().requires_grad_(True)
    rn, rvalid = ssim_ref.depth_to_normal(d64, view.Fx, view.Fy, view.Cx, view.Cy)
    (rn * gn.double()).sum().backward()
    # the reference's own arithmetic is fp32 torch: the same formula in fp32
    d32 = depth.clone().requires_grad_(True)
    fn, _ = ssim_ref.depth_to_normal(d32, view.Fx, view.Fy, view.Cx, view.Cy)
    (fn * gn).sum().backward()
    assert torch.equal(valid.cpu(), rvalid)
    e_gpu = float((n.detach().cpu().double() - rn.detach()).abs().max())
    e_f32 = float((fn.detach().double() - rn.detach()).abs().max())
    assert e_gpu <= max(2 * e_f32, 1e-5), (e_gpu, e_f32)  # central differences of fp32 points cancel
    err = float((d.grad.cpu().double() - d64.grad).norm() / d64.grad.norm())
    err32 = float((d32.grad.double() - d64.grad).norm() / d64.grad.norm())
    assert err <= max(2 * err32, 1e-5), (err, err32)


@pytest.mark.parametrize("i", [0, 1])
def test_depth_to_normal_matches_reference_fixture(i):
    """Against utils/graphics_utils.py:103-119 run by the reference itself
    (fp32 torch, tests/golden/make_golden.py): valid exact, normals within
    1e-5, the gradient of <normal, upstream> within 1e-5 relative L2."""
    import os

    import numpy as np

    import gsr_geometry as G

    d = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "losses.npz"))
    W, H, Fx, Fy, Cx, Cy = d[f"dn_view_{i}"]
    view = View(int(W), int(H))
    view.Fx, view.Fy, view.Cx, view.Cy = float(Fx), float(Fy), float(Cx), float(Cy)
    depth = torch.tensor(d[f"dn_depth_{i}"], device=DEV).requires_grad_(True)
    n, valid = G.depth_to_normal(view, depth)
    (n * torch.tensor(d[f"dn_upstream_{i}"], device=DEV)).sum().backward()
    assert np.array_equal(valid.cpu().numpy(), d[f"dn_valid_{i}"])
    assert np.abs(n.detach().cpu().numpy() - d[f"dn_normal_{i}"]).max() <= 1e-5
    g = d[f"dn_grad_{i}"].astype(np.float64)
    assert np.linalg.norm(depth.grad.cpu().double().numpy() - g) / np.linalg.norm(g) <= 1e-5


# ---------------------------------------------------------------- sizes, holes, layouts, per-pixel gradient
# DN_FLOOR: e_gpu measured where the fp32 torch evaluation is exact against float64, rounded up to a power of ten
# (the per-pixel yardstick of the last tests; the size tests keep the bars of the test above).
# Measured on an MI355X: no comparison below has e_fp32 == 0 with e_gpu > 0, so the floor is 0.
DN_FLOOR = 0.0


def _smooth_depth(W, H):
    v, u = torch.meshgrid(torch.arange(H, dtype=torch.float64), torch.arange(W, dtype=torch.float64), indexing="ij")
    return (3.0 + 0.5 * torch.sin(0.3 * u + 0.1) + 0.4 * torch.cos(0.2 * v) + 0.01 * u * v / (1 + 0.05 * u * v))[None].float()


def _three_ways(view, depth, gn):
    """(normal, valid, dL/ddepth) for L = <normal, gn> on the device, in fp32 torch and in float64 torch."""
    import gsr_geometry as G

    d = depth.to(DEV).requires_grad_(True)
    n, valid = G.depth_to_normal(view, d)
    (n * gn.to(DEV)).sum().backward()
    out = [(n.detach().cpu().double(), valid.cpu(), d.grad.cpu().double())]
    for dt in (torch.float32, torch.float64):
        x = depth.clone().to(dt).requires_grad_(True)
        rn, rvalid = ssim_ref.depth_to_normal(x, view.Fx, view.Fy, view.Cx, view.Cy)
        (rn * gn.to(dt)).sum().backward()
        out.append((rn.detach().double(), rvalid, x.grad.double()))
    return out


@pytest.mark.parametrize("W,H", [(1, 1), (2, 2), (1, 40), (40, 2)])
def test_depth_to_normal_without_interior(W, H):
    """No pixel has all four neighbours: normals, valid and the gradient are exactly zero."""
    import gsr_geometry as G

    d = _smooth_depth(W, H).to(DEV).requires_grad_(True)
    n, valid = G.depth_to_normal(View(W, H), d)
    (n * torch.randn(3, H, W, generator=torch.Generator().manual_seed(1)).to(DEV)).sum().backward()
    assert n.shape == (3, H, W) and valid.shape == (1, H, W)
    assert torch.equal(n, torch.zeros_like(n)) and not bool(valid.any())
    assert torch.equal(d.grad, torch.zeros_like(d))


@pytest.mark.parametrize("W,H", [(3, 3), (3, 64), (64, 3), (65, 5), (257, 4)])
def test_depth_to_normal_small_sizes(W, H):
    """One interior pixel, row or column; rows that straddle waves (65) and workgroups (257).  Bars as in
    test_depth_to_normal_matches_reference."""
    view = View(W, H)
    gn = torch.randn(3, H, W, generator=torch.Generator().manual_seed(2))
    (n, valid, g), (fn, _, g32), (rn, rvalid, gr) = _three_ways(view, _smooth_depth(W, H), gn)
    assert torch.equal(valid, rvalid) and int(valid.sum()) == (H - 2) * (W - 2)
    e_gpu, e_f32 = float((n - rn).abs().max()), float((fn - rn).abs().max())
    err, err32 = float((g - gr).norm() / gr.norm()), float((g32 - gr).norm() / gr.norm())
    print(f"[yard] depth_to_normal {W}x{H}: normal e_gpu {e_gpu:.3e} e_fp32 {e_f32:.3e}; grad {err:.3e} {err32:.3e}")
    Hh.record_margins({"normal": (e_gpu, max(2 * e_f32, 1e-5)), "grad": (err, max(2 * err32, 1e-5))},
                      f"depth_to_normal {W}x{H}")
    assert e_gpu <= max(2 * e_f32, 1e-5), (e_gpu, e_f32)
    assert err <= max(2 * err32, 1e-5), (err, err32)


def test_depth_to_normal_all_holes():
    """An all-zero depth: every cross product is exactly zero, so float64, fp32 and the kernel take the 1/eps
    branch of the normalisation; normals zero, nothing valid, and the gradient that of the float64 reference."""
    W, H = 40, 30
    gn = torch.randn(3, H, W, generator=torch.Generator().manual_seed(3))
    (n, valid, g), (fn, _, g32), (rn, rvalid, gr) = _three_ways(View(W, H), torch.zeros(1, H, W), gn)
    assert torch.equal(g32, gr) and torch.equal(fn, rn)  # the references agree here
    assert torch.equal(n, torch.zeros_like(n)) and not bool(valid.any()) and torch.equal(valid, rvalid)
    assert torch.equal(g, gr)


def test_depth_to_normal_single_positive_pixel():
    """One positive pixel in a zero map: its four neighbours have one zero difference, so their cross products
    vanish and the backward's 1e12 (1/eps) branch carries a non-zero gradient."""
    W, H = 40, 30
    depth = torch.zeros(1, H, W)
    depth[0, 11, 17] = 2.5
    gn = torch.randn(3, H, W, generator=torch.Generator().manual_seed(4))
    (n, valid, g), (fn, _, g32), (rn, rvalid, gr) = _three_ways(View(W, H), depth, gn)
    assert torch.equal(valid, rvalid) and not bool(valid.any())
    assert torch.equal(n, torch.zeros_like(n)) and torch.equal(rn, torch.zeros_like(rn))
    assert float(gr.abs().max()) > 1e9  # the branch is live
    yard = Hh.Yardstick("depth_to_normal single positive pixel")
    yard.add("grad", Hh.max_err(g, gr), Hh.max_err(g32, gr), DN_FLOOR)
    yard.check()


def test_depth_to_normal_layouts():
    """[H, W] gives what [1, H, W] gives (both have the view's trailing sizes), and so does a non-contiguous
    column slice of a wider tensor, bit for bit."""
    import gsr_geometry as G

    W, H = 40, 30
    view = View(W, H)
    depth = _smooth_depth(W, H)
    depth[:, :4, :9] = 0.0
    gn = torch.randn(3, H, W, generator=torch.Generator().manual_seed(5)).to(DEV)

    def run(leaf, x):
        n, valid = G.depth_to_normal(view, x)
        (n * gn).sum().backward()
        return n.detach(), valid, leaf.grad

    d = depth.to(DEV).requires_grad_(True)
    want = run(d, d)
    d2 = depth[0].to(DEV).requires_grad_(True)
    n, valid, g = run(d2, d2)
    assert torch.equal(n, want[0]) and torch.equal(valid, want[1]) and torch.equal(g, want[2][0])
    wide = torch.full((1, H, W + 3), -1.0, device=DEV)
    wide[..., 1:W + 1] = depth.to(DEV)
    wide.requires_grad_(True)
    sl = wide[..., 1:W + 1]
    assert not sl.is_contiguous()
    n, valid, g = run(wide, sl)
    assert torch.equal(n, want[0]) and torch.equal(valid, want[1]) and torch.equal(g[..., 1:W + 1], want[2])
    assert torch.equal(g[..., 0], torch.zeros_like(g[..., 0]))


def test_depth_to_normal_gradient_per_pixel():
    """dL/ddepth pixel by pixel on a hole-free 40 x 30 depth with an unmasked upstream gradient: max|g - g_f64| /
    max|g_f64| apart over the outermost two rows and columns (one-sided contributions only) and over the rest,
    each in the yardstick form."""
    W, H = 40, 30
    gn = torch.randn(3, H, W, generator=torch.Generator().manual_seed(6))
    (n, valid, g), (fn, _, g32), (rn, rvalid, gr) = _three_ways(View(W, H), _smooth_depth(W, H), gn)
    assert torch.equal(valid, rvalid)
    v, u = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
    outer = ((v < 2) | (v >= H - 2) | (u < 2) | (u >= W - 2))[None]
    scale = float(gr.abs().max())
    yard = Hh.Yardstick("depth_to_normal gradient per pixel")
    for name, mask in (("outer", outer), ("rest", ~outer)):
        yard.add(name, float((g - gr)[mask].abs().max()) / scale, float((g32 - gr)[mask].abs().max()) / scale, DN_FLOOR)
    yard.add("normal", float((n - rn).abs().max()), float((fn - rn).abs().max()), DN_FLOOR)
    yard.check()
