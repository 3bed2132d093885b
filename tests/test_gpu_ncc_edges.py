"""warp_patch_ncc (csrc/ncc.hip: ncc_pixel, ncc_kernel) at its edges against
the float64 restatement of the reference's formulas (tests/ncc_ref.py), on the
cases of tests/ncc_cases.py (each checked on the CPU by tests/test_ncc_ref.py).

`valid` is exact except at measured ties: it must equal the float64
reference's wherever both of its decisions (the margins, in pixels; the
variance gates, relative to 5e-6) lie farther from their boundary than four
times the farthest point at which the oracle — the reference's own float32
arithmetic — decides differently (ncc_cases.bands(): measured on the CPU over
every case of this file; 2.1e-5 px and 1.4e-3 when written).  The identity
cases are exact in float32, so they have no ties at all.

Values follow helpers.Yardstick, e_gpu <= 2 e_fp32 + floor against float64 with
e_fp32 the oracle's error, per group of points conditioned alike (grazing or
not by |distance| / depth, and by min(var_r, var_n)), not over the batch.
Where `valid` is false on both sides all five outputs are exactly 0.
"""
from __future__ import annotations

import numpy as np
import pytest
import torch

import helpers as Hh
import ncc_cases as NC
import ncc_ref as NR

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
FIELDS = ("ncc", "grad_depths", "grad_normals")
# floor of e_gpu <= 2 e_fp32 + floor per (case, group, field): 0 unless an MI355X run showed an excess over
# 2 e_fp32, then that excess doubled
FLOORS: dict = {}


def run(case, P=None):
    import warp_patch_ncc as W

    d, n, uv, R, T, ir, inn, K = case
    if P is not None:
        d, n, uv = d[:P], n[:P], uv[:P]
    ncc, gd, gn, valid = W._C.warp_patch_ncc(d.to(DEV), n.to(DEV), uv.to(DEV), R.reshape(3, 3).to(DEV), T.to(DEV),
                                             ir.to(DEV), inn.to(DEV), *K.values(), False)
    return {"ncc": ncc.cpu().numpy(), "grad_depths": gd.cpu().numpy(), "grad_normals": gn.cpu().numpy(),
            "valid": valid.cpu().numpy()}


_GOT = {}


def got(name):
    if name not in _GOT:
        _GOT[name] = run(NC.evaluated()[name][0])
    return _GOT[name]


_RECORDED = set()


def check_valid(name, out):
    """valid against the float64 reference outside ties; zeros where both call a point invalid."""
    case, exact, ref, o = NC.evaluated()[name]
    bm, bg, mm, mg = NC.bands()
    tie = np.zeros(len(ref["valid"]), bool) if exact else NR.ties(ref, bm, bg)
    differ = out["valid"] != ref["valid"]
    tm, tg = NR.valid_decision(ref)
    far = differ & ~tie
    print(f"[valid] {name}: {int(differ.sum())} differ, {int(tie.sum())} ties of {len(tie)}, bands {bm:.2e} px "
          f"{bg:.2e}; farthest differing: margin {tm[differ].max() if differ.any() else 0:.2e} "
          f"gate {tg[differ].max() if differ.any() else 0:.2e}")
    if "bands" not in _RECORDED:  # (the same for every case: once per run)
        _RECORDED.add("bands")
        Hh.record_margins({"band_margin_px": (mm, bm), "band_gate_rel": (mg, bg)}, "valid bands (oracle flip, 4x)")
    if not exact:  # the kernel's own farthest flips against the bands
        flip_m, flip_g = NR.flip_bands(ref, out["valid"])
        Hh.record_margins({"flip_margin_px": (flip_m, bm), "flip_gate_rel": (flip_g, bg)}, f"{name} farthest valid flip")
    assert not far.any(), (name, np.flatnonzero(far)[:10], tm[far][:10], tg[far][:10])
    for f in FIELDS:
        assert not np.any(out[f][~out["valid"]] != 0), (name, f)  # (NaN != 0 too)
    return tie


def check_values(name, out, rows=None):
    """The Yardstick per group over the points all three call valid."""
    case, exact, ref, o = NC.evaluated()[name]
    both = out["valid"] & ref["valid"] & o["valid"]
    if rows is not None:
        both &= rows
    y = Hh.Yardstick(name)
    for gname, m in NC.groups(ref, case[0]).items():
        m = m & both
        if not m.any():
            continue
        for f in FIELDS:
            if not np.isfinite(ref[f][m]).all():  # (the reference itself is not finite: nothing to hold to)
                continue
            y.add(f"{gname}/{f}[{int(m.sum())}]", NC.group_err(out[f], ref[f], m), NC.group_err(o[f], ref[f], m),
                  FLOORS.get((name, gname, f), 0.0))
    y.check()
    return both


def test_reference_margin():
    """ux, uy in {-1 .. 3, W-4 .. W}: the first valid column and row are 2, the last W - 3 and H - 3, exactly
    (integer arithmetic: no tie), and nothing is read for a pixel outside the margin (ncc.hip:74-76)."""
    name = "reference_margin"
    case, _, ref, _ = NC.evaluated()[name]
    out = got(name)
    uv = case[2].numpy()
    Hr, Wr = case[5].shape
    inside = (uv[:, 0] >= 2) & (uv[:, 0] <= Wr - 3) & (uv[:, 1] >= 2) & (uv[:, 1] <= Hr - 3)
    assert np.array_equal(out["valid"], ref["valid"]) and np.array_equal(out["valid"], inside)
    check_valid(name, out)
    check_values(name, out)


def test_neighbour_margin():
    """Warped patches straddling each neighbour bound, among them patches with only one corner tap outside:
    the kernel's test on the extremes of the warps against the reference's AND of 49 per-tap tests."""
    name = "neighbour_margin"
    out = got(name)
    ref = NC.evaluated()[name][2]
    tie = check_valid(name, out)
    one = ref["one_out"] & ~tie
    assert one.sum() >= 8 and not out["valid"][one].any()
    check_values(name, out)


@pytest.mark.parametrize("name", ["margin_ties", "gate_ties"])
def test_ties(name):
    """Points built within 2e-4 px of a neighbour bound / 0.2 % of the variance gate: outside the measured
    band the decision is still the float64 reference's."""
    out = got(name)
    tie = check_valid(name, out)
    assert (~tie).sum() >= 64
    check_values(name, out)


@pytest.mark.parametrize("name", ["identity", "identity_shift"])
def test_identity_warp(name):
    """R = I, T = 0, equal power-of-two focal lengths, integer principal points: every warp is an exact integer
    or half-integer (weights exactly (1, 0) or (1/2, 1/2)), so `valid` has no ties — a patch whose outer taps
    sit exactly on the margin (un - 1.5 == 0) is invalid — and aux = 0 makes both gradients exactly 0."""
    out = got(name)
    ref = NC.evaluated()[name][2]
    assert np.array_equal(out["valid"], ref["valid"])
    on_edge = (np.minimum(ref["margin_r"].min(1), ref["margin_n"].min(1)) == 0)
    assert on_edge.sum() >= 32 and not out["valid"][on_edge].any()
    check_valid(name, out)
    v = out["valid"]
    assert v.sum() >= 100
    assert not np.any(out["grad_depths"][v] != 0) and not np.any(out["grad_normals"][v] != 0)
    check_values(name, out)
    if name == "identity":
        # (NCC = var^2 / (var^2 + 1e-8): 1 up to the reference's own epsilon)
        assert np.all(np.abs(ref["ncc"][v] - 1) <= 1.0001e-8 / (ref["var_r"] * ref["var_n"])[v])


def test_low_texture():
    """Variances spread around the 5e-6 gate: the gate's decisions, and at the valid points the gradients of
    the reference's forward-mode formula (-ncc / (var_n + 1e-8); tests/test_ncc_ref.py shows that the exact
    derivative differs from it here by far more than the float32 error)."""
    name = "low_texture"
    out = got(name)
    ref = NC.evaluated()[name][2]
    tie = check_valid(name, out)
    for gate in ("gate_r", "gate_n"):  # each gate alone decides some points on either side
        other = "gate_n" if gate == "gate_r" else "gate_r"
        alone = ~tie & (ref["margin_n"].min(1) > 0) & (ref[other] > 0) & (ref[gate] <= 0)
        assert alone.sum() >= 32 and not out["valid"][alone].any(), gate
    both = check_values(name, out)
    assert both.sum() >= 200


def test_constant_images():
    """Exactly constant images: variance 0, every point invalid, every output 0 (none non-finite)."""
    out = got("constant")
    assert not out["valid"].any()
    for f in FIELDS:
        assert not np.any(out[f] != 0)


def test_degenerate_rows():
    """distance == 0 exactly (normal perpendicular to the pixel ray), depth 0, NaN and inf in depth and normal,
    in a few rows of an ordinary batch: the gathers are clamped (ncc.hip:135), so nothing is read outside the
    neighbour image; the rows the float64 reference calls invalid are invalid with zero outputs, every output
    the reference has finite is finite, and the other rows are judged as ever.  depth = +-inf is the
    reference's own edge: H = K_n R K_r^-1 (the plane at infinity) can pass every test, and its
    grad_normal is -depth * 0 = NaN, in the reference as here."""
    name = "degenerate"
    case, rows = NC.degenerate()
    out = got(name)
    ref = NC.evaluated()[name][2]
    check_valid(name, out)
    special = sorted(sum(rows.values(), []))
    dist32 = -(((case[2][:, 0].float() - 24.0) / case[7]["fx_r"]) * case[1][:, 0]
               + ((case[2][:, 1].float() - 20.0) / case[7]["fy_r"]) * case[1][:, 1] + case[1][:, 2]) * case[0]
    assert all(float(dist32[i]) == 0.0 for i in rows["perp"] + rows["zero"])
    inf_depth = [i for i in rows["bad"] if np.isinf(float(case[0][i]))]
    for i in special:
        if i in inf_depth:  # the kernel follows the reference: valid alike, NaN exactly where it has NaN
            assert out["valid"][i] == ref["valid"][i]
            for f in FIELDS:
                assert np.array_equal(np.isnan(out[f][i]), np.isnan(ref[f][i])), (i, f)
            continue
        assert not ref["valid"][i] and not out["valid"][i], i
    for f in FIELDS:
        fin = np.isfinite(ref[f]).reshape(len(ref["valid"]), -1).all(1)
        assert np.isfinite(out[f][fin]).all(), f
        assert fin.sum() >= len(fin) - len(inf_depth)
    ordinary = np.ones(len(ref["valid"]), bool)
    ordinary[special] = False
    assert check_values(name, out, ordinary).sum() >= 100


def test_behind_the_neighbour_camera():
    """H_uv.z <= 0 for whole patches and for part of a patch: a patch wholly behind the neighbour camera whose
    warps pass the margin is valid in the reference, and so here; one that straddles z = 0 is not."""
    name = "behind"
    out = got(name)
    ref = NC.evaluated()[name][2]
    tie = check_valid(name, out)
    whole, part = ref["hz_max"] <= 0, (ref["hz_min"] <= 0) & (ref["hz_max"] > 0)
    assert (whole & ref["valid"] & ~tie).sum() >= 4 and out["valid"][whole & ref["valid"] & ~tie].all()
    assert part.sum() >= 32 and not out["valid"][part & ~tie].any()
    for f in FIELDS:
        assert np.isfinite(out[f]).all()
    check_values(name, out)


@pytest.mark.parametrize("name", ["tiny_w2", "tiny_h2", "tiny_5x5"])
def test_tiny_neighbour_image(name):
    """Wn = 2 or Hn = 2 (ncc.hip:95): all invalid.  5 x 5 is the smallest neighbour image that holds a patch
    (1.5 < un < 2.5)."""
    out = got(name)
    check_valid(name, out)
    if name == "tiny_5x5":
        assert check_values(name, out).sum() >= 32
    else:
        assert not out["valid"].any()


def test_grazing_planes():
    """|distance| / depth in [0.02, 0.3]: the gradients' 1 / distance, judged in a group of its own."""
    name = "grazing"
    out = got(name)
    check_valid(name, out)
    assert check_values(name, out).sum() >= 100


def test_block_edges():
    """P in {1, 255, 256, 257, 4099}: the outputs of point i do not depend on P (prefixes bit for bit)."""
    name = "blocks"
    full = got(name)
    check_valid(name, full)
    check_values(name, full)
    for P in NC.BLOCK_P[:-1]:
        part = run(NC.evaluated()[name][0], P)
        for f in FIELDS + ("valid",):
            assert np.array_equal(part[f], full[f][:P], equal_nan=True), (P, f)
