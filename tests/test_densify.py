"""CPU tests of the densification restatement (no GPU needed).

tests/densify_ref.py, the plain-torch yardstick of the HIP path, against
tests/golden/densify.npz — the reference's own densify_and_prune,
compute_3D_filter and reset_opacity run on the CPU with a recorded random
draw (tests/golden/make_golden_densify.py).  Exact: the return triple, the
final count and order, every copied row of every parameter, both Adam
moments, the zeroed statistics, Q.  torch.allclose at 1e-6: what is computed
(new positions, child scalings, the filter, the reset opacities) — CPU against
CPU, the same operations in another arrangement.

And the builders of tests/densify_cases.py: every generated case the GPU tests
use reaches the regime its name says with no decision inside the tie margin,
and every constructed input of the radix select, the 3D filter and
reset_opacity has the property it was constructed for.
"""
from __future__ import annotations

import os

import numpy as np
import pytest
import torch

import densify_cases as DC
import densify_ref as R
from densify_cases import Cam

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = np.load(os.path.join(ROOT, "tests", "golden", "densify.npz"))
CASES = ("mixed", "resplit", "nostats", "quiet")
COMPUTED = ("xyz", "scaling")  # rows of new points are computed, not copied


def case(name):
    return {k[len(name) + 1:]: GOLD[k] for k in GOLD.files if k.startswith(name + "_")}


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


# ------------------------------------------------- the builders of the GPU edge tests
@pytest.mark.parametrize("spec", DC.REGIME_CASES, ids=DC.regime_id)
def test_regime_case_reaches_its_regime(spec):
    regime, P = spec[0], spec[1]
    kase = DC.regime_case(P, spec[2], regime, *spec[3:])
    params, stats, moments, noise, sc3 = kase
    assert params["f_rest"].shape == (P, spec[3] if len(spec) > 3 else 3, 3)
    assert params["sg_axis"].shape == (P, spec[4] if len(spec) > 3 else 1, 3)
    g = R.RefGaussians(params)
    g.set_moments(moments)
    g.set_stats(*stats)
    (C, S, pruned), Q, used = R.densify_and_prune_ref(g, *sc3, noise)
    with np.errstate(invalid="ignore", divide="ignore"):
        ga = torch.tensor(np.nan_to_num(stats[1] / stats[2], nan=0.0))
    d = DC.decisions(kase, Q)
    assert np.float32(Q) == R.quantile_ref(ga, 1.0 - torch.tensor(d["hi"]).float().mean()).numpy()
    N = g._xyz.shape[0]
    assert N == P + C + S - pruned and used <= noise.shape[0]
    assert DC.regime_report(kase, Q) is None, DC.regime_report(kase, Q)
    clone, split, low = d["clone"], d["split"], d["low"]
    assert C == clone.sum() and S == split.sum() + (C if d["csplit"] else 0)
    if regime == "mixed":
        assert Q > 0 and (clone & ~split).any() and (split & ~clone).any() and (clone & split).any()
        assert (clone & low).any() and (split & low).any() and (~split & ~clone & low).any() and (~low).any()
    elif regime == "resplit":
        assert Q == 0 and C > 0 and S == P + C and 0 < pruned < P + C + S
    elif regime == "all_hi":
        assert d["hi"].all() and Q == d["ga"].min() > 0 and C > 0 and S == P and d["ties"] == 1
    elif regime == "all_hi_min0":
        assert d["hi"].all() and Q == 0 and (d["ga"] == 0).sum() > 1 and C > 0 and S == P + C
    elif regime.startswith("none_hi"):
        k = int(regime[-1])
        assert not d["hi"].any() and (stats[2] == 0).any()
        assert Q == d["ga"].max() == DC.SHARED_MAX and d["ties"] == k and (C, S) == (0, k)
        assert len(set(stats[2][d["ga"] == Q])) >= min(k, 2)  # the shared maximum comes from different quotients
    elif regime == "nostats":
        assert not stats[2].any() and Q == 0 and (C, S) == (0, P)
    elif regime == "all_low":
        assert low.all() and N == 0 and C > 0 and S > 0
        assert all(getattr(g, a).shape[0] == 0 for a in R.NAMES.values())
    # the layout the GPU test expects, from the inputs alone, is the restatement's
    c = DC.as_fixture(kase, Q, used)
    rows, C2, S2 = DC.layout(c)
    assert (C2, S2) == (C, S) and rows.shape[0] == N
    assert np.array_equal(g._features_dc.detach().numpy()[:, 0, 0], rows[:, 0].astype(np.float32))
    m = g.moments("f_dc")[0].numpy()[:, 0, 0]
    assert np.array_equal(m != 0, rows[:, 1] < 0)  # survivors keep their (non-zero) moments, new rows start from zero


def test_regime_cases_cover_what_the_kernels_branch_on():
    by = {}
    for spec in DC.REGIME_CASES:
        by.setdefault(spec[0], []).append(spec)
    assert set(by) == set(DC.REGIMES)
    for regime in ("mixed", "resplit"):
        assert {s[1] for s in by[regime]} >= {255, 256, 257, 511, 512, 1025, 4099}
        assert {s[1] for s in by[regime] if s[3:] == (15, 7)} == {1025, 4099}
    for regime in ("all_hi", "all_hi_min0", "none_hi_k1", "none_hi_k5"):
        assert {s[1] for s in by[regime]} >= {255, 256, 257, 1025}


@pytest.mark.parametrize("n", [257, 5000])
@pytest.mark.parametrize("byte", [3, 2, 1, 0])
def test_select_pair_cases_diverge_in_their_byte(n, byte):
    a, b = DC.diverging_pair(byte)
    weights = []
    for q in DC.SELECT_Q:
        x, lo, hi, w = DC.select_pair_case(n, q, a, b, seed=byte)
        s = np.sort(x).view(np.uint32)
        assert len(x) == n and (x >= 0).all() and np.isfinite(x).all()
        assert s[lo] == a and s[hi] == b and s[lo - 1] < a and s[hi + 1] > b
        first = max(k for k in range(4) if (int(a) >> 8 * k) & 255 != (int(b) >> 8 * k) & 255)
        assert first == byte
        weights.append(w)
        want = torch.quantile(torch.tensor(x), torch.tensor(q, dtype=torch.float32))
        assert torch.equal(R.quantile_ref(torch.tensor(x), q), want)
    assert 0 < min(weights) < 0.5 < max(weights) < 1  # both branches of the lerp


@pytest.mark.parametrize("byte", [2, 1, 0])
def test_select_digit255_cases(byte):
    a, b = DC.digit255_pair(byte)
    x, lo, hi, w = DC.select_pair_case(1500, 0.3, a, b, seed=10 + byte)
    s = np.sort(x).view(np.uint32)
    assert s[lo] == a and s[hi] == b and (int(a) >> 8 * byte) & 255 == 255 and 0 < w < 1
    # lower digits of that byte are populated under the same prefix: the pick loop has to walk to 255
    same_prefix = (s >> 8 * (byte + 1)) == (int(a) >> 8 * (byte + 1))
    assert (((s[same_prefix] >> 8 * byte) & 255) < 255).any()


@pytest.mark.parametrize("kind", DC.TIE_KINDS)
def test_select_tie_cases(kind):
    x, lo, hi, w, v = DC.select_tie_case(2000, 0.4, kind)
    s = np.sort(x)
    run = np.flatnonzero(s == v)
    assert len(run) == 300 and 0 < w < 1 and len(np.unique(s)) == 2000 - 299
    first, last = run[0], run[-1]
    want = {"inside": first < lo and hi < last, "begins_at_lo": first == lo, "ends_at_hi": last == hi,
            "begins_at_hi": first == hi, "ends_at_lo": last == lo}
    assert want[kind] and sum(want.values()) == 1


def test_select_integer_ranks_and_consecutive_values():
    for n, q in ((257, 0.5), (2049, 0.25), (257, 0.0), (257, 1.0)):
        lo, hi, w = DC.select_ranks(n, q)
        assert lo == hi == round(q * (n - 1)) and w == 0.0
    x = DC.consecutive_values(2049)
    assert len(np.unique(x)) == 2049 and (np.diff(np.sort(x).view(np.uint32)) == 1).all()
    assert DC.select_ranks(100, -0.5) == DC.select_ranks(100, 0.0) and DC.select_ranks(100, 1.5) == DC.select_ranks(100, 1.0)


@pytest.mark.parametrize("n_cam,slots", DC.FILTER_SLOT_CASES)
def test_filter_slot_cases(n_cam, slots):
    xyz, cams = DC.filter_slot_case(n_cam, slots)
    ok, depth = DC.seen_by(xyz, cams)
    assert len(cams) == n_cam and not DC.margin_ok(xyz, cams).any()
    assert ok[list(slots)].all() and ok.sum() == len(slots) * len(xyz)  # these cameras see all, the others nothing
    for a, b in zip(slots, slots[1:]):
        assert a < b and (depth[b] < depth[a] - 1.0).all()  # the nearer one comes later
    assert max(c.Fx for c in cams) > max(cams[k].Fx for k in slots)


def test_filter_block_and_exact_cases():
    for seen_last in (True, False):
        xyz, cams, front = DC.filter_blocks_case(seen_last)
        _, seen, _ = DC.filter64(xyz, cams)
        assert len(xyz) == 600 and np.array_equal(seen, front) and not DC.margin_ok(xyz, cams).any()
        assert (front[512:].all() and not front[:512].any()) if seen_last else (front[:256].all() and not front[256:].any())
    xyz, cams, seen = DC.filter_exact_case()
    filt, got = R.compute_3D_filter_ref(torch.tensor(xyz), cams)
    assert np.array_equal(got.numpy(), seen) and seen.sum() == 6
    z = torch.tensor(np.where(seen, xyz[:, 2], np.float32(2.5)))
    assert torch.equal(filt[:, 0], z / 64.0 * (0.2 ** 0.5))
    assert DC.margin_ok(xyz, cams).sum() == 10  # every point but the anchor sits on a threshold


@pytest.mark.parametrize("kind", ["zero", "large", "mixed"])
def test_reset_cases(kind):
    params, f = DC.reset_case(257, kind)
    y, x = R.reset_opacity_values(torch.tensor(params["scaling"]), torch.tensor(params["opacity"]), torch.tensor(f),
                                  dtype=torch.float64)
    assert params["opacity"][0, 0] == 15 and params["opacity"][-1, 0] == -15 and torch.isfinite(y).all()
    sq = np.exp(params["scaling"].astype(np.float64)) ** 2
    coef = np.sqrt(sq.prod(1) / (sq + f.astype(np.float64) ** 2).prod(1))
    capped = x[:, 0].numpy() * coef >= 0.01 * (1 - 1e-12)
    if kind == "zero":
        assert not f.any() and (coef == 1).all() and capped.any() and not capped.all()
    elif kind == "large":
        assert coef.max() < 1e-3 and not capped.any()
        assert torch.allclose(y, torch.tensor(params["opacity"]).double(), atol=1e-6)  # the cap does not bind: y = o
    else:
        assert capped.any() and not capped.all() and 1e-3 < coef.min() < coef.max() < 1
