"""The fused PatchMatch kernels (csrc/ncc.hip: pm_lift_kernel, pm_terms_kernel,
pm_finish_kernel, pm_terms_bwd_kernel) alone, on crafted md / normal / pin /
inside (tests/pm_cases.py; no render, no sample_depth), against the float64
restatement tests/ncc_ref.patchmatch_terms (pinned on the CPU by
tests/test_ncc_ref.py).

Masks are exact except at measured ties (pm_cases.bands(): four times the
farthest point at which the float32 formulation on the CPU decides one
comparison differently from float64; 9.3e-6 px for the noise threshold, 1.7e-8
for piv.z = 0.2, none seen for ncc = 0.9 when written; inside, pin.z and md are
inputs and compare exactly).  The random inputs hold no tie, so both counts are
exact there and the values can be judged: helpers.Yardstick, e_gpu <= 2 e_fp32
+ floor against float64, e_fp32 from the reference's torch formulation
(pm_cases.pm_torch with the package's warp_patch_ncc) on the same inputs, per
group of pixels.  Pixels reprojecting less than 0.1 px off are judged by count
and finiteness only (the gradient's direction there is rounding noise in
either formulation, tests/test_gpu_train.py).

1 - cc outside [0, 2] is not constructed: cc <= 1 by Cauchy-Schwarz in exact
arithmetic, and a CPU search over 46,000 identical-patch points (the oracle at
three image scales) found no float32 NCC above 1.0.
"""
from __future__ import annotations

from types import SimpleNamespace

import numpy as np
import pytest
import torch

import helpers as Hh
import ncc_cases as NC
import ncc_ref as NR
import pm_cases as PC

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
G = (0.7, 1.3)  # dL/d(geo_loss, ncc_loss)
# floors of e_gpu <= 2 e_fp32 + floor: 0 unless an MI355X run showed an excess, then that excess doubled
# ("finish", "ncc"): one float32 number has one rounding draw, and at 512x512 torch's masked mean came out 8e-9
# from float64 where the kernel's fixed-order sum was 9.4e-8 (1.5 ulp): excess 7.8e-8 over 2 e_fp32, doubled
FLOORS: dict = {("finish", "ncc"): 1.56e-7}


def on_device(cam):
    return SimpleNamespace(**{k: (v.to(DEV) if torch.is_tensor(v) else v) for k, v in vars(cam).items()})


def setup(H, W, seed=0, **kw):
    """The inputs on the device with the kernels' constants, and those constants back on the CPU."""
    import gsr_patchmatch as PM

    view, nearest, md, normal, pin, inside = PC.inputs(H, W, seed, **kw)
    consts = PM._Consts(on_device(view), on_device(nearest))
    C = SimpleNamespace(tv=consts.tv.cpu(), Mv=consts.Mv.cpu(), t_rel=consts.t_rel.cpu(), R_ncc=consts.R_ncc.cpu(),
                        gray_r=view.gray_image.squeeze(), gray_n=nearest.gray_image.squeeze(), view=view,
                        nearest=nearest)
    return consts, C, md, normal, pin, inside


def raw_terms(md, normal, pin, inside, consts):
    """gsr_patchmatch_terms_forward as _Terms.forward calls it: (w, flags, out) on the CPU."""
    from diff_gaussian_rasterization import _C as _G, _abi

    H, W = md.shape[-2:]
    t = [md.to(DEV).contiguous(), normal.to(DEV).contiguous(), pin.to(DEV).contiguous(), inside.to(DEV).contiguous()]
    w = torch.empty(H * W, dtype=torch.float32, device=DEV)
    flags = torch.empty(H * W, dtype=torch.uint8, device=DEV)
    gd = torch.empty(H * W, dtype=torch.float32, device=DEV)
    gn = torch.empty(H * W, 3, dtype=torch.float32, device=DEV)
    out = torch.empty(4, dtype=torch.float32, device=DEV)
    scratch = _G._ByteBuffer(DEV)
    args = (H, W) + tuple(x.data_ptr() for x in t) + consts.ptrs() + (w.data_ptr(), flags.data_ptr(), gd.data_ptr(),
                                                                      gn.data_ptr())
    _abi.call(DEV, "gsr_patchmatch_terms_forward", scratch.cb, None, *args, out.data_ptr(), _G._stream(DEV))
    torch.cuda.synchronize()
    return w.cpu().numpy(), flags.cpu().numpy(), out.cpu().numpy()


def fused(md, normal, pin, inside, consts):
    """_Terms forward and backward: (geo, ncc, dpin [N, 3], dmd [N], dnormal [3, N]) as numpy."""
    import gsr_patchmatch as PM

    m, n, p = (x.to(DEV).requires_grad_(True) for x in (md, normal, pin))
    geo, ncc = PM._Terms.apply(m, n, p, inside.to(DEV), consts)
    (G[0] * geo + G[1] * ncc).backward()
    return (float(geo), float(ncc), p.grad.reshape(-1, 3).cpu().numpy(), m.grad.reshape(-1).cpu().numpy(),
            n.grad.reshape(3, -1).cpu().numpy())


def torch_fp32(md, normal, pin, inside, consts):
    """The reference's torch formulation in float32 on the device, with the package's warp_patch_ncc."""
    import warp_patch_ncc as Wp

    m, n, p = (x.to(DEV).requires_grad_(True) for x in (md, normal, pin))
    C = SimpleNamespace(tv=consts.tv, Mv=consts.Mv, t_rel=consts.t_rel, R_ncc=consts.R_ncc, gray_r=consts.gray_r,
                        gray_n=consts.gray_n, view=consts.view, nearest=consts.nearest)
    t = PC.pm_torch(m, n, p, inside.to(DEV), C, lambda *a: Wp.warp_patch_ncc(*a, False))
    (G[0] * t["geo_loss"] + G[1] * t["ncc_loss"]).backward()
    z = lambda x, like: torch.zeros_like(like) if x is None else x  # noqa: E731
    return (float(t["geo_loss"]), float(t["ncc_loss"]), z(p.grad, p).reshape(-1, 3).cpu().numpy(),
            z(m.grad, m).reshape(-1).cpu().numpy(), z(n.grad, n).reshape(3, -1).cpu().numpy())


def check_masks(name, ref, flags, out):
    """d_mask, ncc_mask and the clamp flag against float64 outside ties; returns the ties."""
    tie = PC.ties(ref)
    dm, nm, cp = (flags & 1) != 0, (flags & 2) != 0, (flags & 4) != 0
    b = PC.bands()
    print(f"[masks] {name}: d_mask {int(dm.sum())} ncc_mask {int(nm.sum())} ties {int(tie.sum())} differ "
          f"{int((dm != ref['d_mask']).sum())}/{int((nm != ref['ncc_mask']).sum())} bands {b}")
    Hh.record_margins({k: (v[1], v[0]) for k, v in b.items() if v[0] > 0}, f"{name} mask bands (float32 flip, 4x)")
    assert not ((dm != ref["d_mask"]) & ~tie).any() and not ((nm != ref["ncc_mask"]) & ~tie).any()
    assert not ((cp != ref["clamp_pass"]) & ~tie).any()
    assert out[2] == dm.sum() and out[3] == nm.sum()
    return tie, dm, nm


def rel(x, ref):
    return abs(float(x) - float(ref)) / max(abs(float(ref)), 1e-300)


@pytest.mark.parametrize("H,W", [(29, 37), (48, 64)])
def test_masks_values_and_gradients(H, W):
    """Inputs straddling each of inside, pin.z = 0.2, piv.z = 0.2, noise = noise_th, md = 0, md < 0 and
    ncc = 0.9 (tests/test_ncc_ref.py counts each straddle); H * W = 1073 is ragged, 3072 is 12 blocks."""
    name = f"pm {H}x{W}"
    consts, C, md, normal, pin, inside = setup(H, W)
    ref = PC.reference(md, normal, pin, inside, C, g=G)
    w, flags, out = raw_terms(md, normal, pin, inside, consts)
    tie, dm, nm = check_masks(name, ref, flags, out)
    assert not tie.any() and dm.sum() >= 500 and nm.sum() >= 200  # no tie: the counts are the reference's
    got, f32 = fused(md, normal, pin, inside, consts), torch_fp32(md, normal, pin, inside, consts)
    y = Hh.Yardstick(name)
    y.add("geo_loss", rel(got[0], ref["geo_loss"]), rel(f32[0], ref["geo_loss"]), FLOORS.get((name, "geo_loss"), 0.0))
    y.add("ncc_loss", rel(got[1], ref["ncc_loss"]), rel(f32[1], ref["ncc_loss"]), FLOORS.get((name, "ncc_loss"), 0.0))
    noise = ref["noise"]
    for gname, m in (("noise[0.1,0.5)", dm & (noise >= 0.1) & (noise < 0.5)), ("noise[0.5,1)", dm & (noise >= 0.5))):
        assert m.sum() >= 100
        y.add(f"dpin/{gname}", NC.group_err(got[2], ref["dpin"], m), NC.group_err(f32[2], ref["dpin"], m),
              FLOORS.get((name, "dpin", gname), 0.0))
    ys, xs = np.divmod(np.arange(H * W), W)
    unit = NR._np(normal).reshape(3, -1) / ref["len"]
    graze = np.abs((xs - C.view.Cx) / C.view.Fx * unit[0] + (ys - C.view.Cy) / C.view.Fy * unit[1] + unit[2]) < 0.97
    for gname, m in (("oblique", nm & graze), ("facing", nm & ~graze)):
        if not m.any():
            continue
        y.add(f"dmd/{gname}[{int(m.sum())}]", NC.group_err(got[3], ref["dmd"], m),
              NC.group_err(f32[3], ref["dmd"], m), FLOORS.get((name, "dmd", gname), 0.0))
        y.add(f"dnormal/{gname}[{int(m.sum())}]", NC.group_err(got[4].T, ref["dnormal"].T, m),
              NC.group_err(f32[4].T, ref["dnormal"].T, m), FLOORS.get((name, "dnormal", gname), 0.0))
    y.check()
    # below 0.1 px: count and finiteness only; outside the masks: exactly 0
    kink = dm & (noise < 0.1)
    assert kink.sum() >= 16 and np.isfinite(got[2]).all() and np.isfinite(got[3]).all() and np.isfinite(got[4]).all()
    assert (got[2][kink] != 0).any(1).sum() == (f32[2][kink] != 0).any(1).sum()
    assert not got[2][~dm].any() and not got[3][~nm].any() and not got[4][:, ~nm].any()


def test_mask_ties():
    """A third of the pixels within 3e-5 px of the noise threshold, a third within 2e-7 of piv.z = 0.2: outside
    the measured bands the masks are still the float64 reference's."""
    consts, C, md, normal, pin, inside = setup(48, 64, ties=True)
    ref = PC.reference(md, normal, pin, inside, C)
    w, flags, out = raw_terms(md, normal, pin, inside, consts)
    tie, dm, nm = check_masks("pm ties", ref, flags, out)
    near = (np.abs(ref["noise_m"]) < 3.1e-5) & ~tie
    assert (near & (ref["noise_m"] > 0)).sum() >= 64 and (near & (ref["noise_m"] <= 0)).sum() >= 64


def test_tiny_and_zero_normals():
    """|normal| <= 1e-12 (F.normalize's eps): a rendered normal of length 5e-13 at an ncc_mask pixel keeps its
    NCC (the homography does not depend on |n|) and its gradient is g / eps; an exactly zero normal gives
    distance = 0, an invalid NCC and zero gradients, all finite."""
    H, W = 29, 37
    consts, C, md, normal, pin, inside = setup(H, W)
    ref0 = PC.reference(md, normal, pin, inside, C, g=G)
    cand = np.flatnonzero(ref0["ncc_mask"] & ~PC.ties(ref0))
    tiny, zero = cand[:8], cand[8:16]
    n = normal.reshape(3, -1).clone()
    n[:, tiny] = n[:, tiny] / n[:, tiny].norm(dim=0) * 5e-13
    n[:, zero] = 0.0
    normal = n.reshape(3, H, W).contiguous()
    ref = PC.reference(md, normal, pin, inside, C, g=G)
    assert ref["ncc_mask"][tiny].all() and not ref["ncc_mask"][zero].any() and (ref["len"][tiny] <= 1e-12).all()
    w, flags, out = raw_terms(md, normal, pin, inside, consts)
    check_masks("pm normals", ref, flags, out)
    got, f32 = fused(md, normal, pin, inside, consts), torch_fp32(md, normal, pin, inside, consts)
    assert all(np.isfinite(x).all() for x in got[2:])
    assert not got[3][zero].any() and not got[4][:, zero].any()
    m = np.zeros(H * W, bool)
    m[tiny] = True
    assert np.abs(ref["dnormal"][:, tiny]).max() > 1e6  # (g * 1e12)
    y = Hh.Yardstick("pm tiny normals")
    y.add("dnormal", NC.group_err(got[4].T, ref["dnormal"].T, m), NC.group_err(f32[4].T, ref["dnormal"].T, m),
          FLOORS.get(("tiny", "dnormal"), 0.0))
    y.add("dmd", NC.group_err(got[3], ref["dmd"], m), NC.group_err(f32[3], ref["dmd"], m), FLOORS.get(("tiny", "dmd"), 0.0))
    y.check()


def test_point_behind_the_view_has_zero_gradient():
    """piv.z below the 1e-7 clamp (and negative) is outside d_mask: every gradient there is exactly 0."""
    consts, C, md, normal, pin, inside = setup(29, 37)
    ref = PC.reference(md, normal, pin, inside, C, g=G)
    low = ref["pivz_raw"] < 1e-7
    assert low.sum() >= 8 and (ref["pivz_raw"][low] > 0).any() and (ref["pivz_raw"][low] < 0).any()
    got = fused(md, normal, pin, inside, consts)
    assert not ref["d_mask"][low].any()
    assert not got[2][low].any() and not got[3][low].any() and not got[4][:, low].any()


def test_zero_noise_has_zero_gradient():
    """noise == 0 exactly: with the nearest camera at the view's pose (Mv = I, tv = 0), Fx = 64 and Cx = Cy = 0,
    pin = (-1e-6f / 64, -1e-6f / 64, 1) at pixel (0, 0) projects onto pixel - 1e-6 in float32, so proj - pixel +
    1e-6 is (0, 0).  The pixel is in d_mask with weight 1 and sends no gradient (none non-finite)."""
    H, W = 8, 8
    view, nearest = PC.cameras(H, W, identity=True)
    consts, C, md, normal, pin, inside = setup(H, W, view=view, nearest=nearest)
    assert torch.equal(C.Mv, torch.eye(3)) and not C.tv.any()
    e = float(np.float32(1e-6)) / 64.0
    pin[0, 0] = torch.tensor([-e, -e, 1.0])
    md[0, 0, 0] = 2.0
    inside[0, 0] = True
    w, flags, out = raw_terms(md, normal, pin, inside, consts)
    assert flags[0] & 1 and w[0] == 1.0
    got = fused(md, normal, pin, inside, consts)
    assert all(np.isfinite(x).all() for x in got[2:]) and not got[2][0].any()


def test_empty_masks():
    """No pixel inside: both losses and every gradient exactly 0.  Constant images (no valid NCC) with a
    non-empty d_mask: the NCC loss and the gradients into md and normal exactly 0, the geometric loss as ever."""
    consts, C, md, normal, pin, inside = setup(29, 37)
    got = fused(md, normal, pin, torch.zeros_like(inside), consts)
    assert got[0] == 0.0 and got[1] == 0.0 and not any(x.any() for x in got[2:])
    view, nearest = PC.cameras(29, 37, constant=True)
    consts, C, md, normal, pin, inside = setup(29, 37, view=view, nearest=nearest)
    ref = PC.reference(md, normal, pin, inside, C, g=G)
    w, flags, out = raw_terms(md, normal, pin, inside, consts)
    check_masks("pm constant", ref, flags, out)
    assert out[2] >= 500 and out[3] == 0
    got = fused(md, normal, pin, inside, consts)
    assert got[1] == 0.0 and not got[3].any() and not got[4].any() and got[0] > 0 and got[2].any()


@pytest.mark.parametrize("H,W", [(512, 512), (512, 513), (513, 513)])
def test_finish_beyond_1024_blocks(H, W):
    """1024, 1026 and 1029 blocks of partial sums: pm_finish_kernel's strided loop past its 1024 threads.
    `inside` is false except at ~2000 scattered pixels, the last pixel and one of block 1024 (where there is
    one) among them; the float64 reference is evaluated at those only.  Both counts exact, both means by the
    Yardstick."""
    n = H * W
    g = torch.Generator().manual_seed(H * 1000 + W)
    only = torch.randperm(n, generator=g)[:2000].tolist() + [min(1024 * 256 + 5, n - 2), n - 1]
    consts, C, md, normal, pin, inside = setup(H, W, only=only)
    sel = np.flatnonzero(inside.reshape(-1).numpy())
    ref = PC.reference(md, normal, pin, inside, C, only=sel)
    w, flags, out = raw_terms(md, normal, pin, inside, consts)
    tie, dm, nm = check_masks(f"pm {H}x{W}", ref, flags, out)
    assert not tie.any() and out[2] == ref["count_d"] and out[3] == ref["count_n"] and ref["count_n"] >= 100
    if n > 1024 * 256:
        assert ref["d_mask"][1024 * 256:].sum() >= 2 and ref["d_mask"][n - 1]  # blocks past the first stride
    f32 = torch_fp32(md, normal, pin, inside, consts)
    y = Hh.Yardstick(f"pm finish {H}x{W}")
    y.add("geo_loss", rel(out[0], ref["geo_loss"]), rel(f32[0], ref["geo_loss"]), FLOORS.get(("finish", "geo"), 0.0))
    y.add("ncc_loss", rel(out[1], ref["ncc_loss"]), rel(f32[1], ref["ncc_loss"]), FLOORS.get(("finish", "ncc"), 0.0))
    y.check()


@pytest.mark.parametrize("H,W", [(1, 1), (15, 17), (1, 257), (29, 37)])
def test_lift(H, W):
    """pm_lift_kernel, values and dL/dmd, at H * W = 1, 255, 257 and 1073 against float64; e_fp32 from the
    reference's torch expression (md * ray - T) @ R^T (loss_utils.py:147-153)."""
    import gsr_patchmatch as PM

    view, _ = PC.cameras(max(H, 8), max(W, 8), seed=3)
    g = torch.Generator().manual_seed(H * 100 + W)
    md = (2 + 2 * torch.rand(1, H, W, generator=g)).float()
    up = torch.randn(H, W, 3, generator=g)
    M = view.R.T.contiguous()
    intr = (view.Fx, view.Fy, view.Cx, view.Cy)
    ref_pts, ref_g = NR.lift(md, view.T, M, *intr, g=up)
    m = md.to(DEV).requires_grad_(True)
    got = PM._Lift.apply(m, view.T.to(DEV), M.to(DEV), intr)
    got.backward(up.to(DEV))
    m2 = md.to(DEV).requires_grad_(True)
    ix = (torch.arange(W, device=DEV, dtype=torch.float32) - view.Cx) / view.Fx
    iy = (torch.arange(H, device=DEV, dtype=torch.float32) - view.Cy) / view.Fy
    rays = torch.stack([ix[None, :].expand(H, W), iy[:, None].expand(H, W), torch.ones(H, W, device=DEV)], -1)
    t = PC._mat3(m2.squeeze(0).unsqueeze(-1) * rays - view.T.to(DEV), M.to(DEV))
    t.backward(up.to(DEV))
    every = np.ones(H * W, bool)
    y = Hh.Yardstick(f"lift {H}x{W}")
    y.add("points", NC.group_err(got.detach().cpu().numpy().reshape(-1, 3), ref_pts.reshape(-1, 3), every),
          NC.group_err(t.detach().cpu().numpy().reshape(-1, 3), ref_pts.reshape(-1, 3), every),
          FLOORS.get(("lift", "points"), 0.0))
    y.add("dmd", NC.group_err(m.grad.cpu().numpy().reshape(-1), ref_g.reshape(-1), every),
          NC.group_err(m2.grad.cpu().numpy().reshape(-1), ref_g.reshape(-1), every), FLOORS.get(("lift", "dmd"), 0.0))
    y.check()
