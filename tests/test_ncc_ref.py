"""The float64 references of tests/ncc_ref.py pinned on the CPU, and the edge
cases of tests/ncc_cases.py checked to reach their edges before a device sees
them.

warp_patch_ncc is pinned three ways: against autograd of the independent dense
float64 restatement (tests/torch_ref.py) on textured data, where the
reference's -ncc / (var_n + 1e-8) and the exact derivative agree to
1e-8 / (var_r var_n); against the oracle (the reference's float32 arithmetic
in C); and on a low-texture case, where the forward-mode formula and autograd
differ by far more than the float32 error — the evidence that the case has
teeth.  Recorded float32 figures (oracle against float64, relative L2 per
group): NCC <= 5e-5 (2.0e-4 at the variance-gate ties, where var_r var_n is
far below the 1e-8 of the denominator), gradients <= 7e-5 on ordinary groups
and 5.3e-4 on the grazing group of the degenerate batch.
"""
from __future__ import annotations

import numpy as np
import pytest
import torch

import ncc_cases as NC
import ncc_ref as NR
import pm_cases as PC
import torch_ref as R_
from oracle import gsr_oracle as O
from test_oracle import ncc_case

FIELDS = ("ncc", "grad_depths", "grad_normals")


def _autograd(case):
    dd = case[0].double().clone().requires_grad_(True)
    nd = case[1].double().clone().requires_grad_(True)
    x, v = R_.warp_patch_ncc(dd, nd, *case[2:7], *case[7].values())
    x.sum().backward()
    return {"ncc": x.detach().numpy(), "grad_depths": dd.grad.numpy(), "grad_normals": nd.grad.numpy(),
            "valid": v.numpy()}


@pytest.mark.parametrize("seed", [0, 1])
def test_reference_matches_float64_autograd(seed):
    case = ncc_case(400, seed)
    ref, ag = NR.warp_patch_ncc(*case[:7], *case[7].values()), _autograd(case)
    v = ref["valid"]
    assert np.array_equal(v, ag["valid"]) and v.sum() > 100
    assert np.abs(ref["ncc"] - ag["ncc"]).max() <= 1e-12
    # the two gradient forms differ by 1e-8 / (var_r var_n) relative in the var_n term
    bound = 10.0 * float((1e-8 / (ref["var_r"] * ref["var_n"]))[v].max()) + 1e-10
    assert bound < 1e-5
    for f in FIELDS[1:]:
        e = NC.group_err(ref[f], ag[f], v)
        print(f, e, bound)
        assert e <= bound, (f, e, bound)


def oracle_bar(name, gname, f):
    """Four times the recorded oracle-against-float64 figure of the group's kind: ordinary groups NCC 5e-5,
    gradients 7e-5; the variance-gate ties (var_r var_n far below the denominator's 1e-8) NCC 2.0e-4, gradients
    2.7e-4; grazing planes (and the degenerate batch's integer principal point, whose columns ux = cx_r see
    their planes edge-on) gradients 1.0e-3."""
    if name == "gate_ties":
        return 8e-4 if f == "ncc" else 1.2e-3
    if f != "ncc" and (gname.startswith("grazing") or name == "degenerate"):
        return 4e-3
    return 2e-4 if f == "ncc" else 3e-4


CASES = ["reference_margin", "neighbour_margin", "identity", "identity_shift", "low_texture", "constant",
         "degenerate", "behind", "tiny_w2", "tiny_h2", "tiny_5x5", "blocks", "grazing", "margin_ties", "gate_ties"]


@pytest.mark.parametrize("name", CASES)
def test_reference_against_oracle(name):
    """valid equal outside the measured ties (none at all in the exact cases); values per group within four
    times the float32 figure recorded for that kind of group (ORACLE_BARS)."""
    case, exact, ref, o = NC.evaluated()[name]
    bm, bg, mm, mg = NC.bands()
    differ = o["valid"] != ref["valid"]
    if exact or name not in NC.TIES:
        assert not differ.any()
    assert not (differ & ~NR.ties(ref, bm, bg)).any()
    both = o["valid"] & ref["valid"]
    for gname, m in NC.groups(ref, case[0]).items():
        m = m & both
        for f in FIELDS:
            if m.any() and np.isfinite(ref[f][m]).all():
                e = NC.group_err(o[f], ref[f], m)
                print(name, gname, f, int(m.sum()), e)
                assert e <= oracle_bar(name, gname, f), (name, gname, f, e)
    none = ~o["valid"] & ~ref["valid"]
    for f in FIELDS:
        assert not np.any(ref[f][none] != 0)


def test_bands_are_measured():
    """The oracle does decide differently from float64 at the built ties, on both decisions, so the band is a
    measured figure, and a small one: well under the spacing of the random cases' deciding quantities."""
    bm, bg, mm, mg = NC.bands()
    print("bands", bm, bg, "measured", mm, mg)
    assert 0 < mm and bm <= 1e-4 and 0 < mg and bg <= 1e-2
    for name, (case, exact, ref, o) in NC.evaluated().items():
        if name in NC.TIES or exact:
            continue
        assert NR.ties(ref, bm, bg).mean() <= 0.01, name  # at most 1 % of any random case
    for name in NC.TIES:
        ref = NC.evaluated()[name][2]
        tie = NR.ties(ref, bm, bg)
        assert (~tie & ref["valid"]).sum() >= 32 and (~tie & ~ref["valid"]).sum() >= 32, name


def test_low_texture_has_teeth():
    """At valid low-texture patches (var ~ 1e-5, var_r var_n << 1e-8) the reference's forward-mode gradient is
    not the exact derivative: autograd differs from it by more than 100 times the float32 error."""
    case, _, ref, o = NC.evaluated()["low_texture"]
    ag = _autograd(case)
    m = ref["valid"] & o["valid"]
    assert np.array_equal(ag["valid"], ref["valid"]) and m.sum() >= 200
    assert float(np.median((ref["var_r"] * ref["var_n"])[m])) < 1e-9
    assert np.abs(ag["ncc"] - ref["ncc"])[m].max() <= 1e-12
    for f in FIELDS[1:]:
        differ, fp32 = NC.group_err(ag[f], ref[f], m), NC.group_err(o[f], ref[f], m)
        print(f, "autograd against forward mode", differ, "oracle", fp32)
        assert differ > 100 * fp32 and differ > 0.1


def test_generators_reach_their_edges():
    E = NC.evaluated()
    bm, bg, _, _ = NC.bands()
    # neighbour margin: every bound straddled with >= 32 points outside the band on each side; one corner out
    ref = E["neighbour_margin"][2]
    nearest = np.abs(ref["margin_n"]).argmin(1)
    for b in range(4):
        q = ref["margin_n"][nearest == b, b]
        assert (q > bm).sum() >= 32 and (q < -bm).sum() >= 32, b
    assert ref["one_out"].sum() >= 8
    # reference margin: columns 2 and Wr - 3 valid, 1 and Wr - 2 not
    case, _, ref, _ = E["reference_margin"]
    uv, (Hr, Wr) = case[2].numpy(), case[5].shape
    mid = (uv[:, 1] == 3)
    assert ref["valid"][mid & (uv[:, 0] == 2)].all() and ref["valid"][mid & (uv[:, 0] == Wr - 3)].all()
    assert not ref["valid"][mid & ((uv[:, 0] == 1) | (uv[:, 0] == Wr - 2))].any()
    # identity: exact integer or half-integer warps, in float32 arithmetic too
    for name, shift in (("identity", (0, 0)), ("identity_shift", (2, -1))):
        case, _, ref, o = E[name]
        assert ref["valid"].sum() >= 100 and np.array_equal(ref["valid"], o["valid"])
        m = np.concatenate([ref["margin_r"], ref["margin_n"]], 1)
        assert np.array_equal(m * 2, np.round(m * 2)) and (m.min(1) == 0).sum() >= 32
        assert not np.any(ref["grad_depths"] != 0) and not np.any(o["grad_normals"] != 0)
    # low texture: each gate decides >= 32 points either way outside the band
    ref = E["low_texture"][2]
    tie = NR.ties(ref, bm, bg)
    for gate in ("gate_r", "gate_n"):
        assert (~tie & (ref[gate] > 0)).sum() >= 32 and (~tie & (ref[gate] <= 0)).sum() >= 32
    assert not E["constant"][2]["valid"].any()
    # behind: whole patches behind the neighbour camera that the reference calls valid, and straddling ones
    ref = E["behind"][2]
    assert ((ref["hz_max"] <= 0) & ref["valid"]).sum() >= 4
    assert ((ref["hz_min"] <= 0) & (ref["hz_max"] > 0)).sum() >= 32
    # tiny neighbour images
    assert not E["tiny_w2"][2]["valid"].any() and not E["tiny_h2"][2]["valid"].any()
    assert E["tiny_5x5"][2]["valid"].sum() >= 32
    # grazing planes
    case, _, ref, _ = E["grazing"]
    graze = np.abs(ref["distance"] / case[0].numpy()) < 0.3
    assert graze.all() and (ref["valid"] & graze).sum() >= 100
    # degenerate rows: invalid in the reference; distance exactly 0
    case, rows = NC.degenerate()
    ref = E["degenerate"][2]
    assert all(ref["distance"][i] == 0 for i in rows["perp"] + rows["zero"])
    assert not ref["valid"][rows["perp"] + rows["zero"] + [30, 33, 34, 35]].any()


# ---------------------------------------------------------------- PatchMatch terms
@pytest.mark.parametrize("H,W", [(29, 37), (48, 64)])
def test_patchmatch_reference_matches_float64_autograd(H, W):
    """ncc_ref.patchmatch_terms against autograd of the reference's torch formulation (pm_cases.pm_torch) in
    float64 with the dense float64 NCC: masks equal, losses to 1e-13, dL/dpin to 1e-12, dL/dmd and dL/dnormal
    to the 1e-8 / (var_r var_n) by which the NCC's two gradient forms differ (1e-5 here: var ~ 0.03)."""
    view, nearest, md, normal, pin, inside = PC.inputs(H, W)
    C = PC.consts(view, nearest)
    Cd = PC.consts(view, nearest)
    for k in ("tv", "Mv", "t_rel", "R_ncc", "gray_r", "gray_n"):
        setattr(Cd, k, getattr(Cd, k).double())
    m, n, p = (x.double().requires_grad_(True) for x in (md, normal, pin))
    t = PC.pm_torch(m, n, p, inside, Cd, lambda *a: R_.warp_patch_ncc(*a), NR.TH_Z, NR.TH_NCC)
    (0.7 * t["geo_loss"] + 1.3 * t["ncc_loss"]).backward()
    ref = PC.reference(md, normal, pin, inside, C, g=(0.7, 1.3))
    assert np.array_equal(t["d_mask"].numpy(), ref["d_mask"]) and np.array_equal(t["ncc_mask"].numpy(), ref["ncc_mask"])
    assert abs(float(t["geo_loss"].detach()) - ref["geo_loss"]) <= 1e-13
    assert abs(float(t["ncc_loss"].detach()) - ref["ncc_loss"]) <= 1e-13
    every = np.ones(H * W, bool)
    assert NC.group_err(p.grad.reshape(-1, 3).numpy(), ref["dpin"], every) <= 1e-12
    assert NC.group_err(m.grad.reshape(-1).numpy(), ref["dmd"], every) <= 1e-5
    assert NC.group_err(n.grad.reshape(3, -1).numpy().T, ref["dnormal"].T, every) <= 1e-5
    assert not (ref["ncc_mask"] & ~ref["clamp_pass"]).any()  # (1 - cc stays in [0, 1])


@pytest.mark.parametrize("H,W", [(29, 37), (48, 64)])
def test_patchmatch_inputs_straddle_every_test(H, W):
    """Each test of d_mask decides some pixels alone, either way; ncc = 0.9 and the NCC's valid likewise; no
    pixel of the random inputs is a tie (so the counts of the masks are exact)."""
    view, nearest, md, normal, pin, inside = PC.inputs(H, W)
    ref = PC.reference(md, normal, pin, inside, PC.consts(view, nearest))
    ins, mdv = inside.reshape(-1).numpy(), ref["md"]
    q = {k: ref[k] > 0 for k in ("noise_m", "pinz", "pivz")}
    for k in q:
        others = np.all([v for j, v in q.items() if j != k], 0) & ins & (mdv > 0)
        assert (others & q[k]).sum() >= 500 and (others & ~q[k]).sum() >= (32 if k == "noise_m" else 8), k
    allq = q["noise_m"] & q["pinz"] & q["pivz"]
    assert (allq & (mdv > 0) & ~ins).sum() >= 32 and (allq & ins & (mdv == 0)).sum() >= 16
    assert (allq & ins & (mdv < 0)).sum() >= 16
    dm = ref["d_mask"]
    assert (dm & ref["ncc_valid"] & (ref["ncc_m"] > 0)).sum() >= 200
    assert (dm & ref["ncc_valid"] & (ref["ncc_m"] <= 0)).sum() >= 100 and (dm & ~ref["ncc_valid"]).sum() >= 100
    assert (dm & (ref["noise"] < 0.1)).sum() >= 16 and (ref["pivz_raw"] < 1e-7).sum() >= 8
    assert not PC.ties(ref).any()


def test_patchmatch_bands_are_measured():
    """The float32 formulation does decide the noise threshold and piv.z = 0.2 differently from float64 at the
    built ties; the bands stay far below the spacing of the random inputs."""
    b = PC.bands()
    print("patchmatch bands", b)
    assert 0 < b["noise_m"][1] and b["noise_m"][0] <= 1e-4 and 0 < b["pivz"][1] and b["pivz"][0] <= 1e-6
    assert b["ncc_m"][0] <= 1e-4


def test_lift_reference():
    """ncc_ref.lift against autograd of (md * ray - T) @ M in float64."""
    view, _ = PC.cameras(8, 8, seed=3)
    H, W = 5, 7
    g = torch.Generator().manual_seed(1)
    md = torch.rand(1, H, W, generator=g, dtype=torch.float64).requires_grad_(True)
    up = torch.randn(H, W, 3, generator=g, dtype=torch.float64)
    M = view.R.T.double()
    ix = (torch.arange(W, dtype=torch.float64) - view.Cx) / view.Fx
    iy = (torch.arange(H, dtype=torch.float64) - view.Cy) / view.Fy
    rays = torch.stack([ix[None, :].expand(H, W), iy[:, None].expand(H, W), torch.ones(H, W, dtype=torch.float64)], -1)
    pts = (md.squeeze(0).unsqueeze(-1) * rays - view.T.double()) @ M
    pts.backward(up)
    rp, rg = NR.lift(md, view.T, M, view.Fx, view.Fy, view.Cx, view.Cy, g=up)
    assert np.abs(rp - pts.detach().numpy()).max() <= 1e-14 and np.abs(rg - md.grad[0].numpy()).max() <= 1e-14
