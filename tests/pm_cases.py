"""Crafted inputs of the fused PatchMatch kernels (csrc/ncc.hip: pm_lift,
pm_terms, pm_finish, pm_terms_bwd) for tests/test_ncc_ref.py and
tests/test_gpu_patchmatch_edges.py: two plain camera objects with the
attributes gsr_patchmatch._Consts reads, and md / normal / pin / inside built so
that every test of the masks is straddled.  No render, no sample_depth.

pm_torch() is the reference's torch formulation of the terms
(gsr_train.patchmatch_terms and the masked means, utils/loss_utils.py:160-262)
from given sampled points, in the dtype and on the device of its inputs.
"""
from __future__ import annotations

import math
from types import SimpleNamespace

import numpy as np
import torch

import ncc_cases as NC
import ncc_ref as NR

NOISE_TH = 1.0


def cameras(H, W, seed=0, identity=False, constant=False):
    """(view, nearest): world_view_transform [4, 4] (row vectors: x_cam = x @ wv[:3, :3] + wv[3, :3]), R, T,
    intrinsics and a gray image each.  The neighbour image is the view's, blended column by column into an
    unrelated texture, so that the NCC spreads over [0, 1]."""
    g = torch.Generator().manual_seed(9000 + seed)

    def cam(th, t, Fx, Cx, Cy, img, Fy=None):
        wv = torch.eye(4)
        wv[:3, :3] = NC.rotation(g, th).reshape(3, 3)
        wv[3, :3] = torch.tensor(t)
        return SimpleNamespace(world_view_transform=wv, R=wv[:3, :3].clone(), T=wv[3, :3].clone(), Fx=Fx, Fy=Fx + 1.0 if Fy is None else Fy,
                               Cx=Cx, Cy=Cy, gray_image=img[None], image_width=W, image_height=H)

    a = NC.texture(g, H, W)
    b = NC.texture(g, H, W)
    if constant:
        a, b = torch.full((H, W), 0.3), torch.full((H, W), 0.3)
    ramp = torch.linspace(1.0, 0.0, W)[None, :]
    if identity:
        view = cam(0.0, (0.0, 0.0, 0.0), 64.0, 0.0, 0.0, a, 64.0)
        return view, cam(0.0, (0.0, 0.0, 0.0), 64.0, 0.0, 0.0, a.clone(), 64.0)
    view = cam(0.05, (0.01, -0.02, 0.0), 60.0, W / 2 - 0.3, H / 2 + 0.2, a)
    return view, cam(0.08, (0.04, 0.01, 0.0), 60.0, W / 2 - 0.3, H / 2 + 0.2, (ramp * a + (1 - ramp) * b).contiguous())


def consts(view, nearest):
    """gsr_patchmatch._Consts' tensors (loss_utils.py:155-158, :232-235) on the cameras' device."""
    wv, wn = view.world_view_transform, nearest.world_view_transform
    r_rel = wn[:3, :3].transpose(-1, -2) @ wv[:3, :3]
    return SimpleNamespace(tv=(-wv[:3, :3].T @ nearest.R @ nearest.T + wv[3, :3]).contiguous(),
                           Mv=(nearest.R.transpose(1, 0) @ wv[:3, :3]).contiguous(),
                           t_rel=(-r_rel @ wv[3, :3] + wn[3, :3]).contiguous(), R_ncc=r_rel.T.contiguous(),
                           gray_r=view.gray_image.squeeze(), gray_n=nearest.gray_image.squeeze(),
                           view=view, nearest=nearest)


def inputs(H, W, seed=0, ties=False, view=None, nearest=None, only=None):
    """(view, nearest, md [1, H, W], normal [3, H, W], pin [H, W, 3], inside [H, W]) in float32 on the CPU.
    The sampled points are placed so that they reproject r pixels off their own pixel: r in [0.1, 0.9] mostly,
    10 % around the noise threshold 1, 5 % below 0.1; their depth in the view is in [1, 3], 20 % in [0.196, 0.204]
    (piv.z and pin.z, which differ by the relative rotation's ~1e-3, straddle 0.2 in either order), 2 % behind the camera or
    below the 1e-7 clamp.  md is 0 or negative at 10 % of the pixels, `inside` false at 8 %.  ties: a third
    of the pixels within 3e-5 px of the noise threshold and a third within 2e-7 of piv.z = 0.2.
    only: flat pixel indices; `inside` is false everywhere else, and the last two of them pass d_mask."""
    g = torch.Generator().manual_seed(9500 + seed)
    if view is None:
        view, nearest = cameras(H, W, seed)
    C = consts(view, nearest)
    N = H * W
    u = lambda lo=0.0, hi=1.0: (lo + (hi - lo) * torch.rand(N, generator=g, dtype=torch.float64))  # noqa: E731
    force = torch.as_tensor([] if only is None else list(only)[-2:], dtype=torch.long)  # (these pass d_mask)
    kind = torch.rand(N, generator=g)
    kind[force] = 0.9
    z = u(1.0, 3.0)
    z = torch.where(kind < 0.2, u(0.196, 0.204), z)
    z = torch.where((kind >= 0.2) & (kind < 0.21), torch.full_like(z, -0.5), z)
    z = torch.where((kind >= 0.21) & (kind < 0.22), torch.full_like(z, 5e-8), z)
    sel = torch.rand(N, generator=g)
    sel[force] = 0.5
    r = u(0.1, 0.9)
    r = torch.where(sel < 0.10, u(0.9, 1.1), r)
    r = torch.where((sel >= 0.10) & (sel < 0.15), u(0.0, 0.1), r)
    if ties:
        third = torch.rand(N, generator=g)
        r = torch.where(third < 0.33, 1.0 + u(-3e-5, 3e-5), r)
        z = torch.where((third >= 0.33) & (third < 0.66), float(np.float32(0.2)) + u(-2e-7, 2e-7), z)
    ang = u(0.0, 2 * math.pi)
    ys, xs = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
    x, y = xs.reshape(-1).double(), ys.reshape(-1).double()
    zc = z.clamp_min(1e-7)
    piv = torch.stack([(x + r * torch.cos(ang) - 1e-6 - view.Cx) / view.Fx * zc,
                       (y + r * torch.sin(ang) - 1e-6 - view.Cy) / view.Fy * zc, z], 1)
    pin = ((piv - C.tv.double()) @ torch.linalg.inv(C.Mv.double())).float().reshape(H, W, 3).contiguous()
    md = (2 + 2 * torch.rand(N, generator=g)).float()
    mk = torch.rand(N, generator=g)
    mk[force] = 0.9
    md = torch.where(mk < 0.05, torch.zeros(N), md)
    md = torch.where((mk >= 0.05) & (mk < 0.10), -md, md)
    normal = (NC.facing(g, N) * (0.5 + 1.5 * torch.rand(N, 1, generator=g))).T.reshape(3, H, W).contiguous()
    inside = torch.rand(N, generator=g) >= 0.08
    if only is not None:
        keep = torch.zeros(N, dtype=torch.bool)
        keep[torch.as_tensor(only)] = True
        inside = inside & keep
        inside[force] = True
    return view, nearest, md.reshape(1, H, W).contiguous(), normal, pin, inside.reshape(H, W).contiguous()


def _mat3(x, M):
    return torch.addcmul(torch.addcmul(x[..., 0:1] * M[0], x[..., 1:2], M[1]), x[..., 2:3], M[2])


def pm_torch(md, normal, pin, inside, C, ncc_fn, th_z=0.2, th_ncc=0.9):
    """The reference's formulation (gsr_train.patchmatch_terms with its masked means) from sampled points.
    ncc_fn(depths, normals, uvs, R, T, image_r, image_n, 8 intrinsics) -> (cc, valid).  Returns a dict with
    geo_loss, ncc_loss (differentiable), d_mask, ncc_mask (flat), noise, weights, pivz, ncc (at d_mask pixels,
    with their flat indices `sel`)."""
    v, n = C.view, C.nearest
    H, W = md.shape[-2:]
    dev, dt = md.device, md.dtype
    gx, gy = torch.meshgrid(torch.arange(W, device=dev, dtype=torch.int32),
                            torch.arange(H, device=dev, dtype=torch.int32), indexing="xy")
    pixels = torch.stack([gx, gy], dim=-1)
    piv = C.tv.to(dt) + _mat3(pin, C.Mv.to(dt))
    proj = piv[..., :2] / torch.clamp_min(piv[..., 2:], 1e-7)
    proj = torch.addcmul(proj.new_tensor([v.Cx, v.Cy]), proj.new_tensor([v.Fx, v.Fy]), proj)
    noise = torch.pairwise_distance(proj, pixels.to(dt))
    with torch.no_grad():
        dm = (inside & (pin[..., -1] > th_z) & (piv[..., -1] > th_z) & (noise < NOISE_TH) & (md.squeeze() > 0))
        w = torch.exp(-noise).masked_fill(~dm, 0.0)
        sel = torch.argwhere(dm.flatten()).squeeze(1)
        w_sel = w.flatten()[sel]
        px = torch.index_select(pixels.view(-1, 2), 0, sel)
    depth_sel = torch.index_select(md.reshape(-1), 0, sel)
    normal_sel = torch.nn.functional.normalize(torch.index_select(normal.reshape(3, -1), 1, sel).T, dim=-1)
    cc, vm = ncc_fn(depth_sel, normal_sel, px, C.R_ncc, C.t_rel, C.gray_r, C.gray_n, v.Fx, v.Fy, v.Cx, v.Cy, n.Fx,
                    n.Fy, n.Cx, n.Cy)
    ncc = torch.clamp(1 - cc, 0.0, 2.0)
    nm = (ncc < th_ncc) & vm

    def mean(x, m):
        cnt = m.sum()
        s = torch.where(m, x, torch.zeros((), device=dev, dtype=dt)).sum()
        return torch.where(cnt > 0, s / cnt.clamp_min(1), torch.zeros_like(s))

    full_nm = torch.zeros(H * W, dtype=torch.bool, device=dev)
    full_nm[sel] = nm
    return {"geo_loss": mean(w * noise, dm), "ncc_loss": mean(ncc * w_sel, nm), "d_mask": dm.flatten(),
            "ncc_mask": full_nm, "noise": noise.flatten(), "weights": w.flatten(), "pivz": piv[..., 2].flatten(),
            "ncc": ncc, "sel": sel}


def reference(md, normal, pin, inside, C, only=None, g=(1.0, 1.0)):
    """ncc_ref.patchmatch_terms on the same inputs and constants."""
    v, n = C.view, C.nearest
    return NR.patchmatch_terms(md, normal, pin, inside, C.Mv, C.tv, v.Fx, v.Fy, v.Cx, v.Cy, NOISE_TH, C.R_ncc,
                               C.t_rel, C.gray_r, C.gray_n, n.Fx, n.Fy, n.Cx, n.Cy, g_geo=g[0], g_ncc=g[1], only=only)


def oracle_ncc(d, n, uv, R, T, ir, inn, *K):
    """The oracle's warp_patch_ncc as pm_torch's ncc_fn (forward only), on the CPU."""
    from oracle import gsr_oracle as O
    o = O.warp_patch_ncc(d.detach(), n.detach(), uv, R.reshape(-1), T, ir, inn, *K)
    return torch.from_numpy(o["ncc"]), torch.from_numpy(o["valid"])


def computed_q(ref):
    """The deciding quantities that are computed (not inputs), name -> flat float64."""
    return {"noise_m": ref["noise_m"], "pivz": ref["pivz"], "ncc_m": ref["ncc_m"]}


def fp32_q(t, H, W):
    """The same quantities of pm_torch's float32 result (ncc_m only at its d_mask pixels, inf elsewhere)."""
    ncc_m = np.full(H * W, np.inf)
    ncc_m[t["sel"].cpu().numpy()] = NR.TH_NCC - t["ncc"].detach().cpu().double().numpy()
    return {"noise_m": NOISE_TH - t["noise"].detach().cpu().double().numpy(),
            "pivz": t["pivz"].detach().cpu().double().numpy() - NR.TH_Z, "ncc_m": ncc_m}


_BANDS = {}


def bands(H=48, W=64):
    """name -> (band, measured): four times the largest |deciding quantity| (float64) at which the float32
    formulation on the CPU (torch and the oracle's NCC) decides that one comparison differently, over the
    random and the tie inputs of this file; the NCC's own `valid` uses ncc_cases.bands()."""
    if not _BANDS:
        worst = {"noise_m": 0.0, "pivz": 0.0, "ncc_m": 0.0}
        for ties in (False, True):
            view, nearest, md, normal, pin, inside = inputs(H, W, 0, ties)
            C = consts(view, nearest)
            ref, t = reference(md, normal, pin, inside, C), pm_torch(md, normal, pin, inside, C, oracle_ncc)
            q32 = fp32_q(t, H, W)
            ins = ref["d_mask"] | (inside.reshape(-1).numpy() & (ref["md"] > 0) & (ref["pinz"] > 0))
            for k, q in computed_q(ref).items():
                # where this comparison alone decides: the other tests of its mask pass on both sides
                if k == "ncc_m":
                    alone = ref["d_mask"] & t["d_mask"].numpy() & ref["ncc_valid"] & np.isfinite(q32[k])
                else:
                    other = "pivz" if k == "noise_m" else "noise_m"
                    alone = ins & (ref[other] > 0) & (q32[other] > 0)
                flip = alone & np.isfinite(q) & np.isfinite(q32[k]) & ((q > 0) != (q32[k] > 0))
                if flip.any():
                    worst[k] = max(worst[k], float(np.abs(q[flip]).max()))
        _BANDS.update({k: (4.0 * v, v) for k, v in worst.items()})
    return _BANDS


def ties(ref):
    """Pixels at which a mask may differ from the float64 reference's: a computed deciding quantity within its
    band of zero, or the NCC's `valid` within its own bands (ncc_cases.bands())."""
    b = bands()
    bm, bg, _, _ = NC.bands()
    tie = (ref["valid_tm"] <= bm) | (ref["valid_tg"] <= bg)
    for k, q in computed_q(ref).items():
        tie |= np.abs(q) <= b[k][0]
    return tie
