"""GPU tests of the densification path (csrc/densify.hip, gsr_densify.py).

Golden cases (tests/golden/densify.npz: the reference's own code on the CPU)
through the HIP path: the counts, the return triple, every copied parameter
row, both Adam moments and the zeroed statistics are exact; what is computed
is bounded against a float64 evaluation of the same formulas:
  new xyz       within 16 * 2^-24 * (|xyz_src| + sum_j |R_ij| |s_j eps_j|)
  child scaling within  8 * 2^-24 * max(1, |s|)
(a few roundings per operation, with headroom; `parity_ratios()` returns the
worst observed error / bound, recorded in profiles/densify_parity.json).

Edge cases against tests/densify_ref.py run on the same device; the radix
select alone against torch.sort + the fp32 lerp (exact); the 3D filter and
reset_opacity against float64 within stated bounds; determinism; and the
continuity of training across a densification.
"""
from __future__ import annotations

import math

import numpy as np
import pytest
import torch

import densify_ref as R
import gsr_densify
import gsr_optim
from densify_cases import U, filter64, filter_random_case, layout, margin_ok, random_case, rows64  # noqa: F401
from test_densify import CASES, Cam, cams_of, case, model_of

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
_RATIOS: dict = {}


def _note(key, ratio):
    _RATIOS[key] = max(_RATIOS.get(key, 0.0), float(ratio))


def hip_model(c, **kw):
    return model_of(c, device=DEV, optimizer_cls=gsr_optim.FusedAdam, **kw)


def scalars(c):
    return tuple(float(x) for x in c["scalars"])


@pytest.mark.parametrize("name", CASES)
def test_golden_cases_through_hip(name):
    c = case(name)
    g = hip_model(c)
    olds = {n: getattr(g, a) for n, a in R.NAMES.items()}
    triple = gsr_densify.densify_and_prune(g, *scalars(c), None, noise=torch.tensor(c["noise"], device=DEV))
    assert tuple(triple) == tuple(int(x) for x in c["triple"])
    rows, C, S = layout(c)
    N = c["out_xyz"].shape[0]
    assert rows.shape[0] == N and (C, S) == (triple[0], triple[1])
    # Q: the same two order statistics; the interpolation may contract to an fma on the device (1 ulp)
    assert g.last_densify["N"] == N and abs(g.last_densify["Q"] - float(c["Q"])) <= 2 * U * float(c["Q"])
    pos, pos_bound, sc, sc_bound, new, child = rows64(c, rows, C)
    for n, attr in R.NAMES.items():
        p = getattr(g, attr)
        got = p.detach().cpu().numpy()
        assert isinstance(p, torch.nn.Parameter) and p.requires_grad and p is not olds[n]
        assert got.shape == c["out_" + n].shape
        grp = [grp for grp in g.optimizer.param_groups if grp["name"] == n][0]
        assert grp["params"][0] is p and olds[n] not in g.optimizer.state
        m, v = g.moments(n)
        assert np.array_equal(m.cpu().numpy(), c["out_m_" + n]) and np.array_equal(v.cpu().numpy(), c["out_v_" + n]), n
        if n == "xyz":
            assert np.array_equal(got[~new], c["out_xyz"][~new])
            err = np.abs(got.astype(np.float64) - pos)
            print(f"{name} xyz: worst error / bound = {np.max(err[new] / pos_bound[new]) if new.any() else 0:.3f}")
            _note("xyz", np.max(err[new] / pos_bound[new]) if new.any() else 0.0)
            assert (err <= pos_bound).all()
        elif n == "scaling":
            assert np.array_equal(got[~child], c["out_scaling"][~child])
            err = np.abs(got.astype(np.float64) - sc)
            print(f"{name} scaling: worst error / bound = {np.max(err[child] / sc_bound[child]) if child.any() else 0:.3f}")
            _note("scaling", np.max(err[child] / sc_bound[child]) if child.any() else 0.0)
            assert (err <= sc_bound).all()
        else:
            assert np.array_equal(got, c["out_" + n]), n
    for stat in (g.xyz_gradient_accum, g.xyz_gradient_accum_abs, g.denom):
        assert stat.shape == (N, 1) and stat.device.type == "cuda" and not stat.any()
    assert g.max_radii2D.shape == (N,) and not g.max_radii2D.any()
    assert g.filter_3D.shape[0] == c["in_xyz"].shape[0]  # left stale, as the reference leaves it


def parity_ratios():
    """Worst error / bound over the golden cases (run the golden tests first)."""
    return dict(_RATIOS)


# ------------------------------------------------------------------ edge cases
def build(params, stats, moments, optimizer_cls):
    g = R.RefGaussians(params, device=DEV, optimizer_cls=optimizer_cls)
    if moments is not None:
        g.set_moments({n: mv for n, mv in moments.items() if mv[0].size})
    g.set_stats(*stats)
    return g


def compare_with_ref(params, stats, moments, noise, sc3):
    ref = build(params, stats, moments, torch.optim.Adam)
    mine = build(params, stats, moments, gsr_optim.FusedAdam)
    # (the sort-based quantile: torch.quantile refuses large inputs and is the same rule)
    t_ref, Q, used = R.densify_and_prune_ref(ref, *sc3, noise.to(DEV), use_torch_quantile=False)
    t = gsr_densify.densify_and_prune(mine, *sc3, None, noise=noise[:used].to(DEV))
    assert tuple(t) == tuple(t_ref)
    N = ref._xyz.shape[0]
    smax = float(torch.exp(torch.tensor(params["scaling"])).sum(1).max() * noise.abs().max()) if len(noise) else 0.0
    for n, attr in R.NAMES.items():
        a, b = getattr(mine, attr).detach(), getattr(ref, attr).detach()
        assert a.shape == b.shape and a.shape[0] == N, n
        if n == "xyz":  # both sides carry the rounding of the same fp32 formula
            assert ((a - b).abs() <= 2 * 16 * U * (b.abs() + 2 * smax)).all()
        elif n == "scaling":
            assert ((a - b).abs() <= 2 * 8 * U * b.abs().clamp_min(1.0)).all()
        else:
            assert torch.equal(a, b), n
        mo, mr = mine.moments(n), ref.moments(n)
        assert (mo is None) == (mr is None)
        if mo is not None:
            assert torch.equal(mo[0], mr[0]) and torch.equal(mo[1], mr[1]) and mo[0].shape == a.shape, n
    assert mine.denom.shape == (N, 1) and mine.max_radii2D.shape == (N,)
    return mine, ref, t


@pytest.mark.parametrize("P", [1, 63, 257, 4099])
def test_sizes_against_restatement(P):
    params, stats, moments, noise, sc3 = random_case(P, 100 + P)
    mine, _, t = compare_with_ref(params, stats, moments, noise, sc3)
    if P >= 63:
        assert t[0] > 0 and t[1] > 0 and t[2] > 0


def test_optimizer_before_first_step():
    params, stats, _, noise, sc3 = random_case(257, 5)
    mine, _, _ = compare_with_ref(params, stats, None, noise, sc3)
    assert len(mine.optimizer.state) == 0
    for grp in mine.optimizer.param_groups:
        grp["params"][0].grad = torch.ones_like(grp["params"][0])
    mine.optimizer.step()  # the new parameters are the optimizer's
    assert all(mine.optimizer.state[grp["params"][0]]["exp_avg"].shape == grp["params"][0].shape
               for grp in mine.optimizer.param_groups)


def test_sg_degree_zero():
    params, stats, moments, noise, sc3 = random_case(257, 6, sg=False)
    mine, _, _ = compare_with_ref(params, stats, moments, noise, sc3)
    assert [grp["name"] for grp in mine.optimizer.param_groups] == ["xyz", "f_dc", "f_rest", "opacity", "scaling", "rotation"]
    N = mine._xyz.shape[0]
    assert mine._sg_axis.shape == (N, 0, 3) and mine._sg_sharpness.shape == (N, 0) and mine._sg_color.shape == (N, 0, 3)


def test_everything_pruned_but_one_point():
    params, stats, moments, noise, sc3 = random_case(257, 7, low_all_but_one=True)
    mine, ref, t = compare_with_ref(params, stats, moments, noise, sc3)
    assert 1 <= mine._xyz.shape[0] <= 5  # the one opaque point, its clone and children


def test_wrong_noise_and_non_contiguous_parameter_are_refused():
    params, stats, moments, noise, sc3 = random_case(63, 8)
    g = build(params, stats, moments, gsr_optim.FusedAdam)
    old = g._xyz
    with pytest.raises(RuntimeError, match="noise"):
        gsr_densify.densify_and_prune(g, *sc3, None, noise=torch.zeros(1, 3, device=DEV))
    with pytest.raises(RuntimeError, match="noise"):
        gsr_densify.densify_and_prune(g, *sc3, None, noise=torch.zeros(3, 5 * 63, device=DEV))
    assert g._xyz is old and g._xyz.shape[0] == 63 and g.denom.any()  # nothing was touched
    g._rotation = torch.nn.Parameter(g._rotation.detach().t().contiguous().t())
    assert not g._rotation.is_contiguous()
    with pytest.raises(RuntimeError, match="contiguous"):
        gsr_densify.densify_and_prune(g, *sc3, None)
    with pytest.raises(RuntimeError, match="HIP tensor"):
        gsr_densify.filter_3D(torch.zeros(4, 3), [])


def test_two_runs_are_bit_identical_and_generators_agree():
    params, stats, moments, noise, sc3 = random_case(4099, 9)
    runs = []
    for _ in range(2):
        g = build(params, stats, moments, gsr_optim.FusedAdam)
        g2 = build(params, stats, moments, gsr_optim.FusedAdam)
        t = gsr_densify.densify_and_prune(g2, *sc3, None, generator=torch.Generator().manual_seed(77))
        used = t[0] + 2 * t[1]
        gsr_densify.densify_and_prune(g, *sc3, None, noise=noise[:used].to(DEV))
        runs.append((g, g2))
    for k in (0, 1):
        for n, attr in R.NAMES.items():
            assert torch.equal(getattr(runs[0][k], attr), getattr(runs[1][k], attr)), n
            assert torch.equal(runs[0][k].moments(n)[0], runs[1][k].moments(n)[0]), n
    drawn = torch.randn((used, 3), generator=torch.Generator().manual_seed(77))
    g3 = build(params, stats, moments, gsr_optim.FusedAdam)
    gsr_densify.densify_and_prune(g3, *sc3, None, noise=drawn.to(DEV))
    assert torch.equal(g3._xyz, runs[0][1]._xyz)


# ---------------------------------------------------------------- radix select
@pytest.mark.parametrize("n", [1, 2, 255, 65537])
def test_radix_select_matches_sort(n):
    gen = torch.Generator().manual_seed(n)
    plain = torch.rand(n, generator=gen) * 3
    dup = torch.randint(0, 4, (n,), generator=gen).float() * 0.25  # heavy duplicates and zeros
    tiny = torch.rand(n, generator=gen) * 1e-38  # denormals and zeros
    tiny[::2] = 0
    for x in (plain, dup, tiny):
        x = x.to(DEV)
        for q in (0.0, 1.0, 0.5, 1.0 / 3.0):
            got, want = gsr_densify.quantile(x, q), R.quantile_ref(x, q)
            assert torch.equal(got, want), (n, q, float(got), float(want))


def test_radix_select_beyond_torch_quantile_limit():
    n = 2 ** 24 + 3
    x = torch.rand(n, generator=torch.Generator().manual_seed(1)).to(DEV)
    x[::5] = 0
    with pytest.raises(RuntimeError):
        torch.quantile(x, 0.5)
    q = torch.tensor(0.7, device=DEV)
    assert torch.equal(gsr_densify.quantile(x, q), R.quantile_ref(x, q))


# ------------------------------------------------------------------- 3D filter
@pytest.mark.parametrize("P", [1, 65, 1000])
@pytest.mark.parametrize("n_cam", [1, 3, 130])
def test_filter_3d(P, n_cam):
    xyz, cams = filter_random_case(P, n_cam)
    assert not margin_ok(xyz, cams).any()
    want, seen, bound = filter64(xyz, cams)
    assert seen.any() and (P == 1 or not seen[P // 2])
    got = gsr_densify.filter_3D(torch.tensor(xyz, device=DEV), cams)
    assert got.shape == (P, 1)
    err = np.abs(got[:, 0].cpu().numpy().astype(np.float64) - want)
    print(f"filter P={P} cams={n_cam}: worst error / bound = {np.max(err / bound):.3f}")
    _note("filter_3D", np.max(err / bound))
    assert (err <= bound).all()


@pytest.mark.parametrize("name", CASES)
def test_filter_3d_and_reset_opacity_on_golden(name):
    c = case(name)
    cams = cams_of(c)
    xyz = c["out_xyz"]
    want, seen, bound = filter64(xyz, cams)
    g = R.RefGaussians({n: c["out_" + n] for n in R.NAMES}, device=DEV, optimizer_cls=gsr_optim.FusedAdam)
    g.set_moments({n: (c["out_m_" + n], c["out_v_" + n]) for n in R.NAMES})
    gsr_densify.compute_3D_filter(g, cams)
    got = g.filter_3D.cpu().numpy().astype(np.float64)
    assert g.filter_3D.shape == (len(xyz), 1) and not seen.all()
    assert (np.abs(got[:, 0] - want) <= bound).all()
    # and the reference's own fp32 values, which carry the same bound
    assert (np.abs(got[:, 0] - c["filter_3D"][:, 0].astype(np.float64)) <= 2 * bound).all()

    # reset_opacity: y = log(x / (1 - x)), x = min(sigmoid(o) coef, 0.01) / coef.  x carries ~20 roundings
    # (three exp at 1-2 ulp each, squared, two 3-term products, their ratio, a square root, the sigmoid and the
    # two divisions), x / (1 - x) amplifies a relative error of x by 1 / (1 - x), the logarithm adds its own
    # ulp: |y - y64| <= 2^-24 (32 / (1 - x) + 4 |y|).
    old = g._opacity
    y64, x64 = R.reset_opacity_values(g._scaling, g._opacity, g.filter_3D, dtype=torch.float64)
    gsr_densify.reset_opacity(g)
    assert g._opacity is not old and isinstance(g._opacity, torch.nn.Parameter)
    grp = [grp for grp in g.optimizer.param_groups if grp["name"] == "opacity"][0]
    assert grp["params"][0] is g._opacity and old not in g.optimizer.state
    m, v = g.moments("opacity")
    assert m.shape == g._opacity.shape and not m.any() and not v.any()
    err = (g._opacity.detach().double() - y64).abs()
    rbound = U * (32 / (1 - x64) + 4 * y64.abs())
    print(f"{name} reset_opacity: worst error / bound = {float((err / rbound).max()):.3f}")
    _note("reset_opacity", float((err / rbound).max()))
    assert (err <= rbound).all()


def test_filter_3d_with_nothing_seen_is_an_error():
    cams = [Cam(np.eye(3, dtype=np.float32), np.zeros(3, np.float32), (64, 48, 60.0, 60.0))]
    xyz = torch.tensor([[0.0, 0.0, -1.0], [5.0, 0.0, 1.0], [0.0, 0.0, 0.1]], device=DEV)
    with pytest.raises(RuntimeError, match="no point is seen"):
        gsr_densify.filter_3D(xyz, cams)
    g = R.RefGaussians(random_case(3, 1)[0], device=DEV)
    g._xyz = torch.nn.Parameter(xyz)
    gsr_densify.reset_3D_filter(g)
    assert g.filter_3D.shape == (3, 1) and not g.filter_3D.any()


# ------------------------------------------------------------------ continuity
def test_training_continues_across_densification():
    import gsr_train

    step, view, nearest = gsr_train.synthetic_training_setup(300, 64, 48, device="cuda", seed=5)
    g = step.g
    assert g.percent_dense == 0.01
    assert math.isfinite(float(step.step(view, nearest)))
    assert g.denom.any()
    t = g.densify_and_prune(0.0002, 0.05, 4.0, None, generator=torch.Generator().manual_seed(0))
    N = g._xyz.shape[0]
    assert N == 300 + t[0] + t[1] - t[2] and N != 300
    g.compute_3D_filter([view, nearest])
    assert g.filter_3D.shape == (N, 1)
    assert math.isfinite(float(step.step(view, nearest)))  # render, backward, statistics and Adam at the new size
    for grp in g.optimizer.param_groups:
        p = grp["params"][0]
        st = g.optimizer.state[p]
        assert p.shape[0] == N and st["exp_avg"].shape == p.shape and st["exp_avg_sq"].shape == p.shape
    assert g.denom.shape == (N, 1) and g.denom.any() and g.max_radii2D.shape == (N,)
    g.reset_opacity()
    assert g._opacity.shape == (N, 1) and math.isfinite(float(step.step(view, nearest)))
    g.reset_3D_filter()
    assert not g.filter_3D.any()
