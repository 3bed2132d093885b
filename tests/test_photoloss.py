"""CPU tests of the photometric-loss restatement (tests/photoloss_ref.py, the
checker of csrc/photoloss.hip) and of gsr_loss.AppearanceNetwork against the
reference's own L1_loss_appearance and AppearanceNetwork, recorded in fp32 by
tests/golden/make_golden_photoloss.py (tests/golden/photoloss.npz).

Tolerances (fp32 round-off): the L1 is a mean of N = 3 H W terms of size
<= 1 summed in fp32, so |l1 - l1_ref| <= 1e-6; a gradient entry is a sum of at
most N terms of size <= 1/N, so it is compared at 1e-6 of the gradient's largest
entry plus 1e-5 relative.  The restatement rounds t as the reference does (the
same torch operations), so the signs agree at every pixel, ties included.
"""
from __future__ import annotations

import os

import numpy as np
import pytest
import torch

import photoloss_ref as R

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "photoloss.npz")
SIZES = ((64, 96), (70, 100))


@pytest.fixture(scope="module")
def gold():
    return np.load(GOLD)


def _images(gold, tag):
    a = torch.tensor(gold[f"image.{tag}.q4096"].astype(np.float32) / 4096)
    b = torch.tensor(gold[f"gt.{tag}.q4096"].astype(np.float32) / 4096)
    return a, b


def _network(gold):
    import gsr_loss

    net = gsr_loss.AppearanceNetwork(3 + 64, 3)
    state = {k[4:-2]: torch.tensor(gold[k].astype(np.float32) * float(gold[k[:-2] + ".scale"]))
             for k in gold.files if k.startswith("net.") and k.endswith(".q")}
    net.load_state_dict(state, strict=True)  # the reference's key names, all of them
    return net


def _close(got, want, what):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    bar = 1e-6 * np.abs(want).max() + 1e-5 * np.abs(want)
    assert (np.abs(got - want) <= bar).all(), (what, float(np.abs(got - want).max()), float(np.abs(want).max()))


@pytest.mark.parametrize("H,W", SIZES)
@pytest.mark.parametrize("name", ["no", "gs", "gof", "pgsr"])
def test_restatement_matches_reference(gold, name, H, W):
    tag = f"{H}x{W}"
    a, b = _images(gold, tag)
    view = int(gold["view"])
    x = a.clone().requires_grad_(True)
    emb = None
    kw = {}
    if name != "no":
        emb = torch.tensor(gold[f"{name}.{tag}.embeddings"]).requires_grad_(True)
    if name == "gof":
        net = _network(gold)
        gain, crop = R.gof_gain(x, emb[view], net)
        assert crop == ((0, 0, 64, 96) if (H, W) == (64, 96) else (3, 2, 64, 96))
        kw = dict(app_model="gain", gain=gain, crop=crop)
    elif name != "no":
        kw = dict(app_model=name, embedding=emb[view])
    d = R.l1_terms(x, b, **kw)
    l1 = d.abs().mean()
    l1.backward()
    assert abs(float(l1.detach()) - float(gold[f"{name}.{tag}.l1"])) <= 1e-6
    _close(x.grad.numpy(), gold[f"{name}.{tag}.dimage"], "dimage")
    if emb is not None:
        _close(emb.grad.numpy(), gold[f"{name}.{tag}.dembeddings"], "dembeddings")
        rows = [k for k in range(emb.shape[0]) if k != view]
        assert not emb.grad[rows].any()
    if name == "gof":
        _close(net.conv3.weight.grad.numpy(), gold[f"gof.{tag}.dconv3_weight"], "dconv3.weight")
        _close(net.conv3.bias.grad.numpy(), gold[f"gof.{tag}.dconv3_bias"], "dconv3.bias")


def test_float64_restatement_agrees_with_fp32(gold):
    a, b = _images(gold, "70x100")
    e = torch.tensor(gold["pgsr.70x100.embeddings"])[1]
    v32 = R.rgb_loss(a, b, app_model="pgsr", embedding=e)
    v64 = R.rgb_loss(a.double(), b.double(), app_model="pgsr", embedding=e.double())
    assert v64[0].dtype == torch.float64
    for p, q in zip(v32, v64):
        assert abs(float(p) - float(q)) <= 1e-6


def test_composite_is_strict_at_one_half():
    """train.py:163 `gt_mask > 0.5`: a mask value of exactly 0.5 is outside, the next float above it is inside."""
    gt = torch.full((3, 2, 3), 0.25)
    bg = torch.tensor([1.0, 0.5, 0.0])
    above = float(np.nextafter(np.float32(0.5), np.float32(1.0)))
    mask = torch.tensor([[0.5, above, 1.0], [0.0, 0.49999997, 0.5]])
    g = R.composite(gt, mask, bg)
    inside = torch.tensor([[False, True, True], [False, False, False]])
    for c in range(3):
        assert torch.equal(g[c], torch.where(inside, gt[c], bg[c]))
    assert R.composite(gt, None, bg) is gt
    # the loss of an all-0.5 mask is the loss against the constant background
    x = torch.rand(3, 12, 13, generator=torch.Generator().manual_seed(0), dtype=torch.float64)
    t = torch.rand(3, 12, 13, generator=torch.Generator().manual_seed(1), dtype=torch.float64)
    half = R.rgb_loss(x, t, mask=torch.full((12, 13), 0.5), bg=bg)
    const = R.rgb_loss(x, bg.double().view(3, 1, 1).expand(3, 12, 13), mask=None)
    for p, q in zip(half, const):
        assert float(p) == float(q)
