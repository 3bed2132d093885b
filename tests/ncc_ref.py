"""Float64 references of the photometric term (csrc/ncc.hip), one point at a
time, in numpy.

warp_patch_ncc(): forward_mode_differentiation<3, true>
(warp_patch_ncc_impl.cu:18-255) restated with the reference's own formulas:
its forward-mode gradient with grad_variance_n = -ncc / (var_n + 1e-8) (:237,
not the exact derivative where var_r var_n is not >> 1e-8), its per-tap margin
test ANDed over the 49 taps (:87-92, :175-176) and its nextafter / clamp tap
selection (:178-189).  Besides ncc, grad_depth, grad_normal and valid it
returns the quantities that decide `valid`, so that a tie is a measured thing.

patchmatch_terms(), lift(): the PatchMatch terms around it (utils/loss_utils.py:
140-267, as gsr_train.patchmatch_terms states them in torch) with their
gradients into pin, md and normal and the quantities that decide the masks.

Inputs are taken as given (float32 values widen exactly); every operation is
float64.  Non-finite intermediates are allowed and give valid = False.
"""
from __future__ import annotations

import numpy as np

VAR_GATE = 5e-6
# the PatchMatch thresholds as float32 tensors compare against them (torch and the kernel alike)
TH_Z, TH_NCC = float(np.float32(0.2)), float(np.float32(0.9))
_F8 = np.float64


def _np(x, dt=_F8):
    if hasattr(x, "detach"):
        x = x.detach().cpu().numpy()
    return np.ascontiguousarray(np.asarray(x), dtype=dt)


def boundary_distance(q, valid):
    """The distance of each point to the decision boundary of `valid = all(q > 0)`, q [P, K]: a valid point
    turns invalid when its smallest q crosses zero, an invalid one turns valid only when every non-positive q
    does, i.e. at max |q| over them.  NaN counts as -inf (no rounding makes it valid)."""
    q = np.where(np.isnan(q), -np.inf, q)
    neg = np.where(q <= 0, -q, 0.0).max(axis=1)
    return np.where(valid, q.min(axis=1), neg)


def warp_patch_ncc(depths, normals, uvs, R, T, image_r, image_n, fx_r, fy_r, cx_r, cy_r, fx_n, fy_n, cx_n, cy_n):
    """R is the reference's column-major float33 (column i = R[3i:3i+3]).  Returns a dict of [P] (or [P, 3])
    float64 arrays; the deciding quantities are positive on the valid side:
      margin_r  [P, 4] signed distance of the reference pixel's patch to its four margin bounds,
      margin_n  [P, 4] minimum over the 49 taps of the signed distance of (un, vn) to the neighbour bounds,
      gate_r, gate_n   var - 5e-6,
      one_out   [P] bool: exactly one tap (a corner of the patch) fails the neighbour margin test,
      hz_min, hz_max [P] the extremes of H_uv.z over the taps (<= 0: behind the neighbour camera),
      distance, var_r, var_n, ncc_raw, gd_raw, gn_raw (the values before `valid` zeroes them)."""
    with np.errstate(all="ignore"):
        d, n = _np(depths), _np(normals).reshape(-1, 3)
        uv = _np(uvs, np.int64).reshape(-1, 2)
        R, T = _np(R).reshape(-1), _np(T).reshape(3)
        Ir, In = _np(image_r), _np(image_n)
        Hr, Wr = Ir.shape
        Hn, Wn = In.shape
        P = d.shape[0]
        ux, uy = uv[:, 0].astype(_F8), uv[:, 1].astype(_F8)
        pnr = np.stack([(ux - cx_r) / fx_r, (uy - cy_r) / fy_r, np.ones(P)], 1)
        dist = -(pnr * n).sum(1) * d
        margin_r = np.stack([ux - 1.5, (Wr - 1) - (ux + 1.5), uy - 1.5, (Hr - 1) - (uy + 1.5)], 1)
        inside_r = (ux - 1.5 > 0) & (ux + 1.5 < Wr - 1) & (uy - 1.5 > 0) & (uy + 1.5 < Hr - 1)
        # rows outside the reference margin are never read (:59-60): compute them at a safe pixel, zero after
        sx = np.where(inside_r, uv[:, 0], 2 if Wr > 4 else 0)
        sy = np.where(inside_r, uv[:, 1], 2 if Hr > 4 else 0)
        Rc = [R[0:3], R[3:6], R[6:9]]
        Hc = []
        for i in range(3):
            c = Rc[i][None, :] - (n[:, i] / dist)[:, None] * T[None, :]  # :68-70
            Hc.append(np.stack([fx_n * c[:, 0] + cx_n * c[:, 2], fy_n * c[:, 1] + cy_n * c[:, 2], c[:, 2]], 1))
        Hc[2] = Hc[0] * (-cx_r / fx_r) + Hc[1] * (-cy_r / fy_r) + Hc[2]
        Hc[0] = Hc[0] / fx_r
        Hc[1] = Hc[1] / fy_r
        H_uc = Hc[0] * ux[:, None] + Hc[1] * uy[:, None] + Hc[2]
        aux = T[None, :] / dist[:, None]
        z = np.zeros(P)
        s_r, s_n, s_r2, s_n2, s_rn = z.copy(), z.copy(), z.copy(), z.copy(), z.copy()
        g_n, g_n2, g_rn = np.zeros((P, 3)), np.zeros((P, 3)), np.zeros((P, 3))
        margin_n = np.full((P, 4), np.inf)
        n_out = np.zeros(P, np.int64)
        corner_out = np.zeros(P, bool)
        hz_min, hz_max = np.full(P, np.inf), np.full(P, -np.inf)
        all_in = inside_r.copy()
        small = Wr < 5 or Hr < 5  # (no pixel passes the reference margin: nothing to read)

        def px(img, W, H, yy, xx):
            return img[np.clip(yy, 0, H - 1), np.clip(xx, 0, W - 1)]

        for dv in range(-3, 4):
            dv_f = 0.5 * dv
            odd_v = dv & 1
            v0r, v1r = sy + int(np.floor(dv_f)), sy + int(np.ceil(dv_f))
            w_v0, w_v1 = (0.5, 0.5) if odd_v else (1.0, 0.0)
            H_uc_v = H_uc + dv_f * Hc[1]
            for du in range(-3, 4):
                du_f = 0.5 * du
                odd_u = du & 1
                u0r, u1r = sx + int(np.floor(du_f)), sx + int(np.ceil(du_f))
                w_u0, w_u1 = (0.5, 0.5) if odd_u else (1.0, 0.0)
                if small:
                    c_r = z
                else:
                    c00, c01 = px(Ir, Wr, Hr, v0r, u0r), px(Ir, Wr, Hr, v0r, u1r)
                    c10, c11 = px(Ir, Wr, Hr, v1r, u0r), px(Ir, Wr, Hr, v1r, u1r)
                    c_r = (c00 * w_u0 + c01 * w_u1) * w_v0 + (c10 * w_u0 + c11 * w_u1) * w_v1
                H_uv = H_uc_v + du_f * Hc[0]
                hz = H_uv[:, 2]
                un, vn = H_uv[:, 0] / hz, H_uv[:, 1] / hz
                q = np.stack([un - 1.5, (Wn - 1) - (un + 1.5), vn - 1.5, (Hn - 1) - (vn + 1.5)], 1)
                inside = (un - 1.5 > 0) & (un + 1.5 < Wn - 1) & (vn - 1.5 > 0) & (vn + 1.5 < Hn - 1)
                all_in &= inside
                n_out += ~inside
                if abs(du) == 3 and abs(dv) == 3:
                    corner_out |= ~inside
                margin_n = np.minimum(margin_n, np.where(np.isnan(q), -np.inf, q))
                hz_min = np.minimum(hz_min, np.where(np.isnan(hz), -np.inf, hz))
                hz_max = np.maximum(hz_max, np.where(np.isnan(hz), np.inf, hz))
                fin_u, fin_v = np.where(np.isfinite(un), un, 0.0), np.where(np.isfinite(vn), vn, 0.0)
                fin_u, fin_v = np.clip(fin_u, -1e9, 1e9), np.clip(fin_v, -1e9, 1e9)
                u0 = np.floor(fin_u).astype(np.int64)
                v0 = np.floor(fin_v).astype(np.int64)
                u1 = np.ceil(np.nextafter(fin_u, np.inf)).astype(np.int64)  # :178-184
                v1 = np.ceil(np.nextafter(fin_v, np.inf)).astype(np.int64)
                u0, u1 = np.clip(u0, 0, Wn - 1), np.clip(u1, 0, Wn - 1)
                v0, v1 = np.clip(v0, 0, Hn - 1), np.clip(v1, 0, Hn - 1)
                c00n, c01n, c10n, c11n = In[v0, u0], In[v0, u1], In[v1, u0], In[v1, u1]
                wv0, wv1, wu0, wu1 = v1 - vn, vn - v0, u1 - un, un - u0
                c_n = wv0 * (wu0 * c00n + wu1 * c01n) + wv1 * (wu0 * c10n + wu1 * c11n)
                s_r = s_r + c_r
                s_n = s_n + c_n
                s_r2 = s_r2 + c_r * c_r
                s_n2 = s_n2 + c_n * c_n
                s_rn = s_rn + c_r * c_n
                dcx = -c00n * wv0 + c01n * wv0 - c10n * wv1 + c11n * wv1
                dcy = -c00n * wu0 - c01n * wu1 + c10n * wu0 + c11n * wu1
                dH = np.stack([dcx / hz, dcy / hz, (-dcx * un - dcy * vn) / hz], 1)
                left = np.stack([dH[:, 0] * fx_n, dH[:, 1] * fy_n, dH[:, 0] * cx_n + dH[:, 1] * cy_n + dH[:, 2]], 1)
                right = np.stack([(ux + du_f - cx_r) / fx_r, (uy + dv_f - cy_r) / fy_r, np.ones(P)], 1)
                ga = right * (left * aux).sum(1)[:, None]
                g_n = g_n + ga
                g_n2 = g_n2 + 2.0 * c_n[:, None] * ga
                g_rn = g_rn + c_r[:, None] * ga
        inv = 1.0 / 49.0
        cross = s_rn - s_r * s_n * inv
        var_r = s_r2 - s_r * s_r * inv
        var_n = s_n2 - s_n * s_n * inv
        den = var_r * var_n + 1e-8
        ncc = cross * cross / den
        g_cross = 2.0 * cross / den
        g_var_n = -ncc / (var_n + 1e-8)  # :237, the reference's formula
        g_sum_n = (-g_cross * s_r - g_var_n * 2.0 * s_n) * inv
        gaux = g_sum_n[:, None] * g_n + g_var_n[:, None] * g_n2 + g_cross[:, None] * g_rn
        gdist = (gaux * n).sum(1) / dist
        gn = -gaux + (-d * gdist)[:, None] * pnr
        gd = -(pnr * n).sum(1) * gdist
        valid = all_in & (var_r > VAR_GATE) & (var_n > VAR_GATE)
        gate_r = np.where(np.isnan(var_r), -np.inf, var_r - VAR_GATE)
        gate_n = np.where(np.isnan(var_n), -np.inf, var_n - VAR_GATE)
        margin_n = np.where(inside_r[:, None], margin_n, np.inf)  # (not evaluated: decides nothing)
        gate_r = np.where(inside_r, gate_r, np.inf)
        gate_n = np.where(inside_r, gate_n, np.inf)
        zero = lambda a: np.where(valid.reshape((-1,) + (1,) * (a.ndim - 1)), a, 0.0)  # noqa: E731
        return {"ncc": zero(ncc), "grad_depths": zero(gd), "grad_normals": zero(gn), "valid": valid,
                "margin_r": margin_r, "margin_n": margin_n, "gate_r": gate_r, "gate_n": gate_n,
                "one_out": inside_r & (n_out == 1) & corner_out, "hz_min": hz_min, "hz_max": hz_max, "distance": dist,
                "var_r": var_r, "var_n": var_n, "ncc_raw": ncc, "gd_raw": gd, "gn_raw": gn}


def valid_decision(ref):
    """(t_margin, t_gate) of warp_patch_ncc()'s result, [P] each: the distance to the boundary of the two
    decisions `valid` is the AND of, the margins' in pixels and the variance gates' relative to 5e-6.
    `valid` can differ from the float64 reference's only where one of the two decisions does."""
    qm = np.concatenate([ref["margin_r"], ref["margin_n"]], 1)
    qg = np.stack([ref["gate_r"] / VAR_GATE, ref["gate_n"] / VAR_GATE], 1)
    qm, qg = np.where(np.isnan(qm), -np.inf, qm), np.where(np.isnan(qg), -np.inf, qg)
    return boundary_distance(qm, (qm > 0).all(1)), boundary_distance(qg, (qg > 0).all(1))


def flip_bands(ref, other_valid):
    """The largest distance to the boundary at which `other_valid` differs from the reference's, per decision
    (margin, gate): a differing point is counted for a decision unless the other decision alone explains it
    (the other within 1e-2 of its boundary while this one is not)."""
    tm, tg = valid_decision(ref)
    flip = np.asarray(other_valid, bool) != ref["valid"]
    fm = flip & ~((tg < 1e-2) & (tm >= 1e-2))
    fg = flip & ~((tm < 1e-2) & (tg >= 1e-2))
    return float(tm[fm].max()) if fm.any() else 0.0, float(tg[fg].max()) if fg.any() else 0.0


def ties(ref, band_m, band_g):
    """Points at which `valid` may differ from the reference's: a decision within its band of its boundary."""
    tm, tg = valid_decision(ref)
    return (tm <= band_m) | (tg <= band_g)


def patchmatch_terms(md, normal, pin, inside, Mv, tv, Fx, Fy, Cx, Cy, noise_th, R, T, image_r, image_n, fx_n, fy_n,
                     cx_n, cy_n, g_geo=1.0, g_ncc=1.0, only=None):
    """PatchMatch.__call__'s terms (utils/loss_utils.py:140-267) from the sampled points, float64.
    md [H, W], normal [3, H, W] (not normalised), pin [H, W, 3], inside [H, W]; Mv [3, 3] / tv [3]: point in
    view = tv + pin @ Mv; (R, T): warp_patch_ncc's.  `only`: flat pixel indices to evaluate (every other pixel
    must have inside == 0).  Returns flat [H*W] arrays: d_mask, ncc_mask, clamp_pass, weights, noise, ncc
    (clamp(1 - cc, 0, 2)), geo_loss, ncc_loss, the counts, dpin [H*W, 3], dmd [H*W], dnormal [3, H*W] for
    dL/d(geo_loss, ncc_loss) = (g_geo, g_ncc), and the deciding quantities (positive: the mask's side)
    noise_m = noise_th - noise, pinz = pin.z - 0.2, pivz = piv.z - 0.2, md, ncc_m = 0.9 - ncc, one_m,
    one_m2 = 2 - one_m, and the NCC's own (valid_dist)."""
    with np.errstate(all="ignore"):
        md = _np(md)
        H, W = md.shape[-2:]
        N = H * W
        md = md.reshape(N)
        nrm = _np(normal).reshape(3, N)
        pin = _np(pin).reshape(N, 3)
        ins = _np(inside, bool).reshape(N)
        Mv, tv = _np(Mv).reshape(3, 3), _np(tv).reshape(3)
        sel = np.arange(N) if only is None else np.asarray(only, np.int64)
        if only is not None:
            rest = np.ones(N, bool)
            rest[sel] = False
            assert not ins[rest].any(), "`only` must cover every inside pixel"
        y, x = sel // W, sel % W
        p = pin[sel]
        piv = tv[None, :] + p @ Mv
        zc = np.maximum(piv[:, 2], 1e-7)
        dx = Cx + Fx * (piv[:, 0] / zc) - x + 1e-6
        dy = Cy + Fy * (piv[:, 1] / zc) - y + 1e-6
        noise = np.sqrt(dx * dx + dy * dy)
        dm = ins[sel] & (p[:, 2] > TH_Z) & (piv[:, 2] > TH_Z) & (noise < noise_th) & (md[sel] > 0)
        w = np.where(dm, np.exp(-noise), 0.0)
        ln = np.sqrt((nrm[:, sel] ** 2).sum(0))
        unit = (nrm[:, sel] / np.maximum(ln, 1e-12)).T
        k = np.flatnonzero(dm)
        c = warp_patch_ncc(md[sel][k], unit[k], np.stack([x[k], y[k]], 1), R, T, image_r, image_n, Fx, Fy, Cx, Cy,
                           fx_n, fy_n, cx_n, cy_n)
        S = len(sel)
        cc, cv = np.zeros(S), np.zeros(S, bool)
        gd, gn, vdist = np.zeros(S), np.zeros((S, 3)), np.full(S, np.inf)
        ntie_m, ntie_g = np.full(S, np.inf), np.full(S, np.inf)
        cc[k], cv[k], gd[k], gn[k] = c["ncc"], c["valid"], c["grad_depths"], c["grad_normals"]
        ntie_m[k], ntie_g[k] = valid_decision(c)
        vdist[k] = np.minimum(ntie_m[k], ntie_g[k])
        one_m = 1.0 - cc
        ncc = np.clip(one_m, 0.0, 2.0)
        nm = dm & cv & (ncc < TH_NCC)
        cpass = (one_m >= 0.0) & (one_m <= 2.0)
        cnt_d, cnt_n = int(dm.sum()), int(nm.sum())
        geo = float((w * noise)[dm].sum() / cnt_d) if cnt_d else 0.0
        nccl = float((ncc * w)[nm].sum() / cnt_n) if cnt_n else 0.0
        # backward: w under no_grad (loss_utils.py:217-221)
        gnoise = np.where(dm, (g_geo / cnt_d if cnt_d else 0.0) * w, 0.0)
        s = np.where(noise > 0, gnoise / noise, 0.0)
        gx, gy = s * dx * Fx, s * dy * Fy
        iz = 1.0 / zc
        gz = np.where(piv[:, 2] >= 1e-7, -(gx * piv[:, 0] + gy * piv[:, 1]) * iz * iz, 0.0)
        gv = np.stack([gx * iz, gy * iz, gz], 1)
        dpin_s = np.where(dm[:, None], gv @ Mv.T, 0.0)
        gcc = np.where(nm & cpass, -(g_ncc / cnt_n if cnt_n else 0.0) * w, 0.0)
        dmd_s = gcc * gd
        gu = gn * gcc[:, None]
        proj = (gu - unit * (unit * gu).sum(1)[:, None]) / ln[:, None]
        dn_s = np.where((ln > 1e-12)[:, None], proj, gu * 1e12)
        dn_s = np.where((nm & cpass)[:, None], dn_s, 0.0)

        def full(a, fill=0.0):
            out = np.full((N,) + a.shape[1:], fill, a.dtype)
            out[sel] = a
            return out

        return {"d_mask": full(dm, False), "ncc_mask": full(nm, False), "clamp_pass": full(cpass & nm, False),
                "weights": full(w), "noise": full(noise), "ncc": full(ncc), "geo_loss": geo, "ncc_loss": nccl,
                "count_d": cnt_d, "count_n": cnt_n, "dpin": full(dpin_s), "dmd": full(dmd_s),
                "dnormal": full(dn_s).T.copy(), "noise_m": full(noise_th - noise, np.inf),
                "pinz": full(p[:, 2] - TH_Z, np.inf), "pivz": full(piv[:, 2] - TH_Z, np.inf),
                "pivz_raw": full(piv[:, 2], np.inf), "md": full(md[sel], np.inf), "ncc_m": full(TH_NCC - ncc, np.inf),
                "one_m": full(one_m, 1.0), "one_m2": full(2.0 - one_m, 1.0), "valid_dist": full(vdist, np.inf), "valid_tm": full(ntie_m, np.inf), "valid_tg": full(ntie_g, np.inf),
                "ncc_valid": full(cv, False), "len": full(ln, 1.0), "gd": full(gd), "gn": full(gn)}


def lift(md, T, M, Fx, Fy, Cx, Cy, g=None):
    """The median-depth points in world space, (md * ray - T) @ M (loss_utils.py:147-153), float64, [H, W, 3];
    with g [H, W, 3] also dL/dmd [H, W]."""
    md = _np(md)
    H, W = md.shape[-2:]
    md = md.reshape(H, W)
    T, M = _np(T).reshape(3), _np(M).reshape(3, 3)
    ys, xs = np.mgrid[0:H, 0:W]
    ray = np.stack([(xs - Cx) / Fx, (ys - Cy) / Fy, np.ones((H, W))], -1)
    pts = (md[..., None] * ray - T) @ M
    if g is None:
        return pts
    return pts, ((_np(g).reshape(H, W, 3) @ M.T) * ray).sum(-1)
