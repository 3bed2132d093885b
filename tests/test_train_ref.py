"""CPU tests of the float64 restatements of the training step's kernels
(tests/train_ref.py; no GPU needed), before the GPU tests trust them.

adam_step against torch.optim.Adam run in float64 for 5 steps: the same
formula in another arrangement (lerp as m + w (g - m), addcdiv as a
subtraction), so agreement is to float64 rounding.  Measured on this data:
parameters 1.3e-16, exp_avg 2.1e-16, exp_avg_sq 3.8e-17 of the tensor's
largest magnitude; the bar is 1e-14 (about 50 float64 ulps: the measured
figure rounded up to 1e-15, times ten for another torch build's rounding
order; still eight orders of magnitude below the fp32 errors the reference
is used to judge).
scale_opacity, normalize_rows against tests/golden/getters.npz (the
reference's own getters in fp32): run in fp32 the restatement gives the
fixture's numbers bit for bit, the bar tests/test_oracle.py holds
gsr_scene's getters to; run in float64 it is within fp32 rounding of them
(<= 4 fp32 ulps = 4 * 2^-24 of the tensor's largest magnitude: exp, square,
sqrt, product and quotient each round once in the fixture).
normalize_rows against F.normalize in float64, value and gradient, with an
exact-zero row and rows either side of eps: 1e-15.
"""
from __future__ import annotations

import os

import numpy as np
import torch
import torch.nn.functional as F

import train_ref as T

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _rel(a, b):
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-300))


def test_adam_step_matches_torch_adam_float64():
    g = torch.Generator().manual_seed(0)
    shapes, lrs = [(257, 3), (64, 15, 3), (5,)], [1.6e-4, 5e-2, 1e-3]
    betas = [(0.9, 0.999), (0.9, 0.999), (0.8, 0.99)]
    ps = [torch.nn.Parameter(torch.randn(s, generator=g, dtype=torch.float64)) for s in shapes]
    opt = torch.optim.Adam([{"params": [p], "lr": lr, "betas": b} for p, lr, b in zip(ps, lrs, betas)], lr=0.0,
                           eps=1e-15, foreach=False)
    mine = [(p.detach().clone(), torch.zeros_like(p), torch.zeros_like(p)) for p in ps]
    worst = {"p": 0.0, "m": 0.0, "v": 0.0}
    for step in range(1, 6):
        for k, p in enumerate(ps):
            p.grad = torch.randn(p.shape, generator=g, dtype=torch.float64) * 10.0 ** (1 - step)
            if step == 3:
                p.grad[0] = 0.0
            mine[k] = T.adam_step(*mine[k][:1], p.grad, *mine[k][1:], lrs[k], step, betas[k], 1e-15)
        opt.step()
        for k, p in enumerate(ps):
            st = opt.state[p]
            assert float(st["step"]) == step
            for name, a, b in (("p", mine[k][0], p.detach()), ("m", mine[k][1], st["exp_avg"]),
                               ("v", mine[k][2], st["exp_avg_sq"])):
                worst[name] = max(worst[name], _rel(a, b))
    print("adam_step against torch.optim.Adam (float64):", worst)
    assert max(worst.values()) <= 1e-14, worst


def test_getters_match_reference_fixture():
    d = np.load(os.path.join(GOLD, "getters.npz"))
    s, o, f = (torch.tensor(d[k]) for k in ("raw_scaling", "raw_opacity", "filter_3D"))
    scales, opac = T.scale_opacity(s, o, f)
    np.testing.assert_array_equal(scales.numpy(), d["scales"])
    np.testing.assert_array_equal(opac.numpy(), d["opacity"])
    np.testing.assert_array_equal(T.normalize_rows(torch.tensor(d["raw_rotation"])).numpy(), d["rotation_out"])
    ulp4 = 4 * 2.0 ** -24
    scales, opac = T.scale_opacity(s.double(), o.double(), f.double())
    rot = T.normalize_rows(torch.tensor(d["raw_rotation"]).double())
    for name, a, want in (("scales", scales, d["scales"]), ("opacity", opac, d["opacity"]),
                          ("rotation", rot, d["rotation_out"])):
        e = _rel(torch.tensor(want).double(), a)
        print(f"float64 {name} against the fixture: {e:.3e}")
        assert e <= ulp4, (name, e)


def test_normalize_rows_matches_f_normalize():
    g = torch.Generator().manual_seed(1)
    for D in (1, 3, 4, 7):
        x = torch.randn(12, D, generator=g, dtype=torch.float64)
        x[0] = 0.0  # exact zero: y = 0, dy/dx = 1/eps
        x[1] *= 1e-13 / x[1].norm()
        x[2] *= 1e-11 / x[2].norm()
        x[3] *= 1e-30 / x[3].norm()
        x[4] *= 1e18 / x[4].norm()
        up = torch.randn(12, D, generator=g, dtype=torch.float64)
        a = x.clone().requires_grad_(True)
        b = x.clone().requires_grad_(True)
        ya, yb = T.normalize_rows(a), F.normalize(b, dim=1)
        (ya * up).sum().backward()
        (yb * up).sum().backward()
        assert torch.isfinite(a.grad).all() and torch.isfinite(ya).all()
        assert torch.equal(ya[0], torch.zeros(D, dtype=torch.float64))
        assert torch.equal(a.grad[0], up[0] / 1e-12)
        for r in range(12):  # per row: the rows differ by 48 orders of magnitude
            assert _rel(ya[r].detach(), yb[r].detach()) <= 1e-15 or float(yb[r].abs().max()) == 0.0
            assert _rel(a.grad[r], b.grad[r]) <= 1e-15, (D, r)
