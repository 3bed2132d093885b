"""CPU tests of the densification restatement (no GPU needed).

tests/densify_ref.py, the plain-torch yardstick of the HIP path, against
tests/golden/densify.npz — the reference's own densify_and_prune,
compute_3D_filter and reset_opacity run on the CPU with a recorded random
draw (tests/golden/make_golden_densify.py).  Exact: the return triple, the
final count and order, every copied row of every parameter, both Adam
moments, the zeroed statistics, Q.  torch.allclose at 1e-6: what is computed
(new positions, child scalings, the filter, the reset opacities) — CPU against
CPU, the same operations in another arrangement.
"""
from __future__ import annotations

import os

import numpy as np
import pytest
import torch

import densify_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = np.load(os.path.join(ROOT, "tests", "golden", "densify.npz"))
CASES = ("mixed", "resplit", "nostats", "quiet")
COMPUTED = ("xyz", "scaling")  # rows of new points are computed, not copied


def case(name):
    return {k[len(name) + 1:]: GOLD[k] for k in GOLD.files if k.startswith(name + "_")}


class Cam:
    def __init__(self, R_, T, whf):
        self.R, self.T = torch.tensor(R_), torch.tensor(T)
        self.image_width, self.image_height, self.Fx, self.Fy = int(whf[0]), int(whf[1]), float(whf[2]), float(whf[3])


def cams_of(c):
    return [Cam(c["cam_R"][i], c["cam_T"][i], c["cam_WHF"][i]) for i in range(c["cam_R"].shape[0])]


def model_of(c, device="cpu", **kw):
    g = R.RefGaussians({n: c["in_" + n] for n in R.NAMES}, device=device, **kw)
    g.set_moments({n: (c["in_m_" + n], c["in_v_" + n]) for n in R.NAMES})
    g.set_stats(c["accum"], c["accum_abs"], c["denom"])
    return g


def run_ref(name):
    c = case(name)
    g = model_of(c)
    max_grad, min_opacity, extent = (float(x) for x in c["scalars"])
    triple, Q, used = R.densify_and_prune_ref(g, max_grad, min_opacity, extent, torch.tensor(c["noise"]))
    return c, g, triple, Q, used


@pytest.mark.parametrize("name", CASES)
def test_restatement_reproduces_reference(name):
    c, g, triple, Q, used = run_ref(name)
    assert tuple(triple) == tuple(int(x) for x in c["triple"])
    assert used == c["noise"].shape[0]
    assert np.float32(Q) == c["Q"]
    N = c["out_xyz"].shape[0]
    for n, attr in R.NAMES.items():
        got = getattr(g, attr).detach().numpy()
        want = c["out_" + n]
        assert got.shape == want.shape and got.shape[0] == N
        if n in COMPUTED:
            assert torch.allclose(torch.tensor(got), torch.tensor(want), rtol=1e-6, atol=1e-6), n
        else:
            assert np.array_equal(got, want), n
        m, v = g.moments(n)
        assert np.array_equal(m.numpy(), c["out_m_" + n]) and np.array_equal(v.numpy(), c["out_v_" + n]), n
    # surviving originals are copied: exact for the computed tensors too
    surv = np.flatnonzero(np.any(c["out_m_xyz"] != 0, axis=1))
    for n in COMPUTED:
        assert np.array_equal(getattr(g, R.NAMES[n]).detach().numpy()[surv], c["out_" + n][surv])
    for stat in (g.xyz_gradient_accum, g.xyz_gradient_accum_abs, g.denom):
        assert stat.shape == (N, 1) and not stat.any()
    assert g.max_radii2D.shape == (N,) and not g.max_radii2D.any()


def test_fixture_covers_the_cases():
    c = case("mixed")
    max_grad, min_opacity, extent = (float(x) for x in c["scalars"])
    with np.errstate(invalid="ignore", divide="ignore"):
        gr = np.nan_to_num(c["accum"] / c["denom"], nan=0.0)
        ga = np.nan_to_num(c["accum_abs"] / c["denom"], nan=0.0)
    big = np.exp(c["in_scaling"]).max(axis=1) > 0.01 * extent
    low = (1 / (1 + np.exp(-c["in_opacity"][:, 0]))) < min_opacity
    clone = (gr >= max_grad) & ~big
    split = ((gr >= max_grad) & big) | (ga >= c["Q"])
    assert clone.sum() == c["triple"][0] > 0 and split.sum() == c["triple"][1] > 0
    assert (clone & split).any(), "a point that is cloned and split"
    assert (clone & low).any() and (split & low).any() and (~split & low).any(), "prunes of every kind"
    assert c["Q"] > 0
    r = case("resplit")
    assert r["Q"] == 0 and r["triple"][0] > 0 and r["triple"][1] == r["in_xyz"].shape[0] + r["triple"][0]
    n = case("nostats")
    assert not n["denom"].any() and n["triple"][0] == 0 and n["triple"][1] == n["in_xyz"].shape[0]
    q = case("quiet")
    assert tuple(q["triple"]) == (0, 1, 0)  # the maximum of grads_abs equals Q: the reference always splits it


@pytest.mark.parametrize("name", CASES)
def test_filter_and_reset_opacity(name):
    c, g, *_ = run_ref(name)
    cams = cams_of(c)
    filt, seen = R.compute_3D_filter_ref(g._xyz, cams)
    assert not seen.all() and seen.any()
    assert torch.allclose(filt, torch.tensor(c["filter_3D"]), rtol=1e-6, atol=1e-6)
    g.filter_3D = torch.tensor(c["filter_3D"])
    old = g._opacity
    R.reset_opacity_ref(g)
    assert g._opacity is not old and g.optimizer.param_groups[3]["params"][0] is g._opacity
    assert torch.allclose(g._opacity.detach(), torch.tensor(c["reset_opacity"]), rtol=1e-6, atol=1e-6)
    m, v = g.moments("opacity")
    assert not m.any() and not v.any() and m.shape == g._opacity.shape


def test_quantile_ref_is_torch_quantile():
    gen = torch.Generator().manual_seed(3)
    for n in (1, 2, 255, 1000):
        x = torch.rand(n, generator=gen)
        x[::3] = 0
        for q in (0.0, 1.0, 0.5, 1 / 3):
            assert torch.equal(R.quantile_ref(x, q), torch.quantile(x, torch.tensor(q, dtype=torch.float32)))


def test_optimizer_without_state_and_no_sg():
    c = case("mixed")
    params = {n: c["in_" + n] for n in R.NAMES}
    for n in ("sg_axis", "sg_color"):
        params[n] = np.zeros((params["xyz"].shape[0], 0, 3), np.float32)
    params["sg_sharpness"] = np.zeros((params["xyz"].shape[0], 0), np.float32)
    g = R.RefGaussians(params)
    g.set_stats(c["accum"], c["accum_abs"], c["denom"])
    assert [grp["name"] for grp in g.optimizer.param_groups] == ["xyz", "f_dc", "f_rest", "opacity", "scaling", "rotation"]
    max_grad, min_opacity, extent = (float(x) for x in c["scalars"])
    triple, _, _ = R.densify_and_prune_ref(g, max_grad, min_opacity, extent, torch.tensor(c["noise"]))
    assert tuple(triple) == tuple(int(x) for x in c["triple"])
    assert len(g.optimizer.state) == 0
    assert g._sg_axis.shape == (c["out_xyz"].shape[0], 0, 3)
    assert np.array_equal(g._features_rest.detach().numpy(), c["out_f_rest"])
