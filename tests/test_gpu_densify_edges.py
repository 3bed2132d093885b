"""GPU tests of the densification path at its edges (csrc/densify.hip, gsr_densify.py).

The cases come from tests/densify_cases.py; tests/test_densify.py checks on the
CPU that each one has the property its name says.  The bounds are those of
tests/test_gpu_densify.py, whose docstrings derive them; none is new.

1. Decision regimes x sizes (P at and around the 256-lane blocks, 1025 and 4099
   with the real row widths) through `compare_with_ref`, and the documented
   layout read back from `f_dc` rows that hold their source index.
2. The radix select on constructed inputs, against the sort (exact).
3. The 3D filter at the ends of its 64-camera staging chunks and exactly on
   its thresholds.
4. reset_opacity at block-end sizes, with a zero and a large filter, raw
   opacities of +-15 and an optimiser without state.
"""
from __future__ import annotations

import numpy as np
import pytest
import torch

import densify_cases as DC
import densify_ref as R
import gsr_densify
import gsr_optim
from densify_cases import U
from test_gpu_densify import DEV, _note, compare_with_ref

pytestmark = pytest.mark.gpu


# ------------------------------------------------------- 1. regimes x sizes
def ascending(a):
    return bool((np.diff(a) > 0).all())


@pytest.mark.parametrize("spec", DC.REGIME_CASES, ids=DC.regime_id)
def test_regime_against_restatement(spec):
    regime, P = spec[0], spec[1]
    kase = DC.regime_case(P, spec[2], regime, *spec[3:])
    params, stats, moments, noise, sc3 = kase
    mine, ref, (C, S, pruned) = compare_with_ref(*kase)
    info = mine.last_densify
    N, Q = info["N"], info["Q"]
    assert N == P + C + S - pruned == mine._xyz.shape[0] and (info["C"], info["S"]) == (C, S)
    for stat in (mine.xyz_gradient_accum, mine.xyz_gradient_accum_abs, mine.denom):
        assert stat.shape == (N, 1) and stat.device.type == "cuda" and not stat.any()
    assert mine.max_radii2D.shape == (N,) and not mine.max_radii2D.any()
    assert len(mine.optimizer.state) == len(R.NAMES)
    for grp in mine.optimizer.param_groups:  # consistent shapes and groups, at N == 0 too
        p = grp["params"][0]
        st = mine.optimizer.state[p]
        assert p is getattr(mine, R.NAMES[grp["name"]]) and isinstance(p, torch.nn.Parameter) and p.requires_grad
        assert p.shape == (N,) + tuple(params[grp["name"]].shape[1:])
        assert st["exp_avg"].shape == p.shape and st["exp_avg_sq"].shape == p.shape

    # what the regime is about
    if regime == "mixed":
        assert Q > 0 and C > 0 and S > 0 and pruned > 0
    elif regime in ("resplit", "all_hi_min0"):
        assert Q == 0 and C > 0 and S == P + C
    elif regime == "all_hi":
        assert Q > 0 and C > 0 and S == P
    elif regime.startswith("none_hi"):
        assert Q == DC.SHARED_MAX and (C, S) == (0, int(regime[-1]))
    elif regime == "nostats":
        assert Q == 0 and (C, S) == (0, P)
    else:
        assert N == 0

    # the error / bound of compare_with_ref's two computed tensors
    if N:
        smax = float(torch.exp(torch.tensor(params["scaling"])).sum(1).max() * noise.abs().max())
        a, b = mine._xyz.detach(), ref._xyz.detach()
        _note("edges.xyz_vs_restatement", ((a - b).abs() / (2 * 16 * U * (b.abs() + 2 * smax))).max())
        a, b = mine._scaling.detach(), ref._scaling.detach()
        _note("edges.scaling_vs_restatement", ((a - b).abs() / (2 * 8 * U * b.abs().clamp_min(1.0))).max())

    # The layout, without the restatement: every f_dc row holds its source index.  Surviving originals,
    # surviving clones, children copy 0, children copy 1; each in ascending source order, among the
    # children the originals' before the clones'.
    rows, C2, S2 = DC.layout(DC.as_fixture(kase, Q, C + 2 * S))
    assert (C2, S2) == (C, S) and rows.shape[0] == N
    f_dc = mine._features_dc.detach().cpu().numpy()
    assert (f_dc == f_dc[:, :1, :1]).all()
    src = f_dc[:, 0, 0].astype(np.int64)
    assert np.array_equal(src, rows[:, 0])
    kept = (mine.moments("f_dc")[0].cpu().numpy()[:, 0, 0] != 0)  # survivors keep their moments, new rows have none
    n_o = int(kept.sum())
    assert kept[:n_o].all() and n_o == int((rows[:, 1] < 0).sum())
    n_c = int(((rows[:, 1] >= 0) & (rows[:, 1] < C)).sum())
    n_cc = int((rows[:, 2] >= 0).sum()) // 2
    assert (N - n_o - n_c) % 2 == 0 and (n_c == 0 or n_cc == 0)  # a clone stays or is split again, by Q alone
    n_ch = (N - n_o - n_c) // 2
    first = n_o + n_c
    assert ascending(src[:n_o]) and ascending(src[n_o:first])
    for j in range(2):
        child = src[first + j * n_ch:first + (j + 1) * n_ch]
        assert ascending(child[:n_ch - n_cc]) and ascending(child[n_ch - n_cc:])
    assert np.array_equal(src[first:first + n_ch], src[first + n_ch:])
    if N:
        assert src.min() >= 0 and src.max() < P


# ---------------------------------------------------------- 2. radix select
def check_select(x, q):
    xd = torch.as_tensor(x).to(DEV)
    got, want = gsr_densify.quantile(xd, q), R.quantile_ref(xd, min(max(q, 0.0), 1.0))
    assert torch.equal(got, want), (len(x), q, float(got), float(want))
    return float(got)


@pytest.mark.parametrize("n", [257, 5000])
@pytest.mark.parametrize("byte", [3, 2, 1, 0])
def test_select_targets_diverge_in_each_pass(n, byte):
    a, b = DC.diverging_pair(byte)
    for q in DC.SELECT_Q:
        x, lo, hi, w = DC.select_pair_case(n, q, a, b, seed=byte)
        got = check_select(x, q)
        assert DC.from_bits([a])[0] <= got <= DC.from_bits([b])[0]


@pytest.mark.parametrize("byte", [2, 1, 0])
def test_select_digit_255(byte):
    a, b = DC.digit255_pair(byte)
    for q in DC.SELECT_Q:
        x, lo, hi, w = DC.select_pair_case(1500, q, a, b, seed=10 + byte)
        got = check_select(x, q)
        assert DC.from_bits([a])[0] <= got <= DC.from_bits([b])[0]
    x = DC.from_bits(np.full(300, a))  # and as the only digit there is
    assert check_select(x, 0.5) == DC.from_bits([a])[0]


@pytest.mark.parametrize("kind", DC.TIE_KINDS)
def test_select_ties(kind):
    x, lo, hi, w, v = DC.select_tie_case(2000, 0.4, kind)
    got = check_select(x, 0.4)
    if kind in ("inside", "begins_at_lo", "ends_at_hi"):
        assert got == v  # both order statistics are the run's value


def test_select_integer_rank():
    for n, q in ((257, 0.5), (2049, 0.25), (257, 0.0), (257, 1.0), (2049, 0.0), (2049, 1.0)):
        x = DC.consecutive_values(n, seed=n)
        lo, hi, w = DC.select_ranks(n, q)
        assert lo == hi and w == 0.0
        assert check_select(x, q) == np.sort(x)[lo]
        check_select(torch.rand(n, generator=torch.Generator().manual_seed(n)).numpy(), q)


@pytest.mark.parametrize("n", [2047, 2048, 2049])
def test_select_grid_edges(n):
    gen = torch.Generator().manual_seed(n)
    plain = torch.rand(n, generator=gen).numpy() * 3
    dup = torch.randint(0, 4, (n,), generator=gen).float().numpy() * 0.25
    for x in (plain, dup, DC.consecutive_values(n, seed=n)):
        for q in (0.0, 1.0, 0.5, 1.0 / 3.0, 0.9):
            check_select(x, q)
    # the last element alone decides: every lane of the grid has to reach its share
    x = np.full(n, 0.5, np.float32)
    x[-1] = 2.0
    assert check_select(x, 1.0) == 2.0
    x[-1] = 0.25
    assert check_select(x, 0.0) == 0.25


def test_select_beyond_the_grid():
    n = 2048 * 256 * 8 + 2049  # more than 2048 blocks of 256 x 8: the grid is capped and strides on
    x = torch.rand(n, generator=torch.Generator().manual_seed(2)).to(DEV)
    x[::7] = 0
    x[-1] = 5.0
    for q in (0.37, 1.0):
        assert torch.equal(gsr_densify.quantile(x, q), R.quantile_ref(x, q))


@pytest.mark.parametrize("n", [1, 2049])
def test_select_clamps_q(n):
    x = DC.consecutive_values(n, seed=3)
    s = np.sort(x)
    for q in (-0.5, -1e-3, 1.001, 1.5):
        assert check_select(x, q) == (s[0] if q < 0 else s[-1])


# ------------------------------------------------------------ 3. 3D filter
def check_filter(xyz, cams):
    want, seen, bound = DC.filter64(xyz, cams)
    got = gsr_densify.filter_3D(torch.tensor(xyz, device=DEV), cams)
    assert got.shape == (len(xyz), 1)
    got = got[:, 0].cpu().numpy()
    err = np.abs(got.astype(np.float64) - want)
    print(f"filter P={len(xyz)} cams={len(cams)}: worst error / bound = {np.max(err / bound):.3f}")
    _note("edges.filter_3D", np.max(err / bound))
    assert (err <= bound).all()
    return got, seen


@pytest.mark.parametrize("P", [1, 257])
@pytest.mark.parametrize("n_cam", [63, 64, 65, 127, 128, 129])
def test_filter_camera_counts(P, n_cam):
    xyz, cams = DC.filter_random_case(P, n_cam)
    assert not DC.margin_ok(xyz, cams).any()
    got, seen = check_filter(xyz, cams)
    assert seen.any() and (P == 1 or not seen[P // 2])


@pytest.mark.parametrize("n_cam,slots", DC.FILTER_SLOT_CASES)
def test_filter_deciding_camera_by_slot(n_cam, slots):
    xyz, cams = DC.filter_slot_case(n_cam, slots)
    got, seen = check_filter(xyz, cams)
    assert seen.all()
    # the same cameras with the deciding ones moved to the front: a minimum does not depend on the order
    front = [cams[k] for k in reversed(slots)] + [c for k, c in enumerate(cams) if k not in slots]
    moved = gsr_densify.filter_3D(torch.tensor(xyz, device=DEV), front)[:, 0].cpu().numpy()
    assert np.array_equal(got, moved)


def test_filter_two_identical_cameras():
    xyz, cams = DC.filter_random_case(257, 1)
    one = gsr_densify.filter_3D(torch.tensor(xyz, device=DEV), cams)
    for copies in (2, 65):  # within a chunk and across two
        assert torch.equal(gsr_densify.filter_3D(torch.tensor(xyz, device=DEV), cams * copies), one)


def test_filter_exact_thresholds():
    xyz, cams, seen = DC.filter_exact_case()
    want, ref_seen = R.compute_3D_filter_ref(torch.tensor(xyz), cams)
    assert np.array_equal(ref_seen.numpy(), seen)
    for lead in (0, 64):  # the identity camera in the first chunk, and as the first of the second
        away = [DC.yaw_cam(np.pi, (0.0, 0.0, 0.0), 50.0)] * lead
        got = gsr_densify.filter_3D(torch.tensor(xyz, device=DEV), away + cams).cpu()
        assert torch.equal(got, want), (lead, got[:, 0].tolist(), want[:, 0].tolist())
        # z == 0.2f and one float past a bound are not seen: they take the anchor's depth
        assert (got[~seen, 0] == got[10, 0]).all() and (got[2::2, 0][:4] < got[10, 0]).all()


@pytest.mark.parametrize("seen_last", [True, False])
def test_filter_unseen_fallback_across_blocks(seen_last):
    xyz, cams, front = DC.filter_blocks_case(seen_last)
    got, seen = check_filter(xyz, cams)
    assert np.array_equal(seen, front)
    assert (got[~front] == got[front].max()).all()


# -------------------------------------------------------- 4. reset_opacity
def reset_model(P, kind, with_state):
    params, f = DC.reset_case(P, kind)
    g = R.RefGaussians(params, device=DEV, optimizer_cls=gsr_optim.FusedAdam)
    if with_state:
        g.set_moments({n: (np.full(v.shape, 0.5, np.float32), np.full(v.shape, 0.25, np.float32))
                       for n, v in params.items()})
    g.filter_3D = torch.tensor(f, device=DEV)
    return g


def check_reset(g):
    old = g._opacity
    untouched = {a: getattr(g, a) for a in R.NAMES.values() if a != "_opacity"}
    y64, x64 = R.reset_opacity_values(g._scaling, g._opacity, g.filter_3D, dtype=torch.float64)
    gsr_densify.reset_opacity(g)
    assert g._opacity is not old and isinstance(g._opacity, torch.nn.Parameter) and g._opacity.requires_grad
    assert g._opacity.shape == old.shape
    grp = [grp for grp in g.optimizer.param_groups if grp["name"] == "opacity"][0]
    assert grp["params"][0] is g._opacity and old not in g.optimizer.state
    assert all(getattr(g, a) is p for a, p in untouched.items())
    err = (g._opacity.detach().double() - y64).abs()
    rbound = U * (32 / (1 - x64) + 4 * y64.abs())
    print(f"reset_opacity P={old.shape[0]}: worst error / bound = {float((err / rbound).max()):.3f}")
    _note("edges.reset_opacity", float((err / rbound).max()))
    assert torch.isfinite(g._opacity).all() and (err <= rbound).all()


@pytest.mark.parametrize("P", [1, 255, 256, 257, 1025])
@pytest.mark.parametrize("kind", ["zero", "large", "mixed"])
def test_reset_opacity(P, kind):
    g = reset_model(P, kind, with_state=True)
    check_reset(g)
    m, v = g.moments("opacity")
    assert m.shape == g._opacity.shape and v.shape == m.shape and not m.any() and not v.any()
    for n in R.NAMES:  # the other moments stay
        if n != "opacity" and g.moments(n)[0].numel():
            assert (g.moments(n)[0] == 0.5).all() and (g.moments(n)[1] == 0.25).all()


@pytest.mark.parametrize("kind", ["zero", "mixed"])
def test_reset_opacity_before_the_first_step(kind):
    g = reset_model(257, kind, with_state=False)
    assert len(g.optimizer.state) == 0
    check_reset(g)
    assert len(g.optimizer.state) == 0 and g.moments("opacity") is None  # no state is invented
    for grp in g.optimizer.param_groups:
        grp["params"][0].grad = torch.ones_like(grp["params"][0])
    g.optimizer.step()  # the new parameter is the optimizer's
    st = g.optimizer.state[g._opacity]
    assert st["exp_avg"].shape == g._opacity.shape and st["exp_avg"].any()
