"""Seeded edge cases of warp_patch_ncc for tests/test_ncc_ref.py (which checks
on the CPU that each generator reaches the edge it is named for) and
tests/test_gpu_ncc_edges.py (which runs them on the device).  A case is
(depths [P], normals [P, 3], uvs [P, 2] int32, R [9] column-major, T [3],
image_r, image_n, K) as tests/test_oracle.ncc_case returns it.
"""
from __future__ import annotations

import math

import numpy as np
import torch

import ncc_ref as NR

EYE = torch.eye(3).reshape(-1).contiguous()


def texture(g, H, W, noise=0.05):
    base = torch.rand(1, 1, H // 4 + 2, W // 4 + 2, generator=g)
    img = torch.nn.functional.interpolate(base, size=(H, W), mode="bicubic", align_corners=True)[0, 0]
    return (img + noise * torch.rand(H, W, generator=g)).float().contiguous()


def rotation(g, th):
    """A rotation by th about a random axis, as the reference's column-major float33 (r to n)."""
    a = torch.randn(3, generator=g, dtype=torch.float64)
    a = a / a.norm()
    K = torch.tensor([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]], dtype=torch.float64)
    Rm = torch.eye(3, dtype=torch.float64) + math.sin(th) * K + (1 - math.cos(th)) * K @ K
    return Rm.T.reshape(-1).float().contiguous()


def facing(g, P, tilt=0.3):
    nrm = torch.randn(P, 3, generator=g) * tilt
    nrm[:, 2] = -1.0
    return (nrm / nrm.norm(dim=1, keepdim=True)).float().contiguous()


def intr(Wr, Hr, Wn, Hn, **kw):
    K = dict(fx_r=50.0, fy_r=52.0, cx_r=Wr / 2 - 0.3, cy_r=Hr / 2 + 0.2, fx_n=55.0, fy_n=54.0, cx_n=Wn / 2,
             cy_n=Hn / 2 - 0.4)
    K.update(kw)
    return K


def ordinary(P, seed, Wr=48, Hr=40, Wn=52, Hn=44):
    """Textured images, a small relative pose, random interior pixels: most points valid."""
    g = torch.Generator().manual_seed(1000 + seed)
    uvs = torch.stack([torch.randint(2, Wr - 2, (P,), generator=g), torch.randint(2, Hr - 2, (P,), generator=g)], 1)
    return ((torch.rand(P, generator=g) * 2 + 2).float(), facing(g, P), uvs.int().contiguous(), rotation(g, 0.08),
            (torch.randn(3, generator=g) * 0.1).float(), texture(g, Hr, Wr), texture(g, Hn, Wn),
            intr(Wr, Hr, Wn, Hn))


def grazing(seed=0, P=1024):
    """ordinary() with normals turned until the plane is seen at a grazing angle, |pnr . n| in [0.02, 0.3]: the
    forward-mode gradients divide by distance = -(pnr . n) depth."""
    d, n, uv, R, T, ir, inn, K = ordinary(P, 20 + seed)
    g = torch.Generator().manual_seed(1500 + seed)
    pnr = torch.stack([(uv[:, 0] - K["cx_r"]) / K["fx_r"], (uv[:, 1] - K["cy_r"]) / K["fy_r"], torch.ones(P)], 1).double()
    ray = pnr / pnr.norm(dim=1, keepdim=True)
    side = torch.randn(P, 3, generator=g, dtype=torch.float64)
    side = side - ray * (side * ray).sum(1, keepdim=True)
    side = side / side.norm(dim=1, keepdim=True)
    c = (0.02 + 0.28 * torch.rand(P, generator=g, dtype=torch.float64))[:, None] / pnr.norm(dim=1, keepdim=True)
    n = -c * ray + (1 - c * c).sqrt() * side
    return d, n.float().contiguous(), uv, R, (T * 0.3).contiguous(), ir, inn, K


def reference_margin(seed=0, Wr=24, Hr=20, Wn=40, Hn=36):
    """ux in {-1, 0, 1, 2, 3, Wr-4 .. Wr} x uy likewise: the first valid column is 2, the last Wr - 3, and uvs
    outside the image are never read.  The warps of the valid ones lie well inside the neighbour image."""
    g = torch.Generator().manual_seed(2000 + seed)
    xs = [-1, 0, 1, 2, 3, Wr - 4, Wr - 3, Wr - 2, Wr - 1, Wr]
    ys = [-1, 0, 1, 2, 3, Hr - 4, Hr - 3, Hr - 2, Hr - 1, Hr]
    uvs = torch.tensor([[x, y] for y in ys for x in xs], dtype=torch.int32)
    P = len(uvs)
    return ((torch.rand(P, generator=g) * 2 + 2).float(), facing(g, P), uvs, rotation(g, 0.02),
            (torch.randn(3, generator=g) * 0.05).float(), texture(g, Hr, Wr), texture(g, Hn, Wn),
            intr(Wr, Hr, Wn, Hn, fx_n=50.0, fy_n=52.0))


def neighbour_margin(seed=0, P=1024, Wr=48, Hr=40, Wn=40, Hn=34):
    """Warped patches that straddle each of the four neighbour bounds: of 40,000 seeded candidates the ones
    whose nearest tap is within half a pixel of a bound (by the float64 reference), P of them."""
    g = torch.Generator().manual_seed(3000 + seed)
    C = 40000
    uvs = torch.stack([torch.randint(2, Wr - 2, (C,), generator=g), torch.randint(2, Hr - 2, (C,), generator=g)],
                      1).int().contiguous()
    case = [(torch.rand(C, generator=g) * 2 + 2).float(), facing(g, C), uvs, rotation(g, 0.1),
            (torch.randn(3, generator=g) * 0.1).float(), texture(g, Hr, Wr), texture(g, Hn, Wn),
            intr(Wr, Hr, Wn, Hn, fx_n=50.0, fy_n=52.0)]
    r = NR.warp_patch_ncc(*case[:7], *case[7].values())
    near = np.flatnonzero(np.abs(r["margin_n"]).min(1) < 0.5)[:P]
    assert len(near) == P
    keep = torch.from_numpy(near)
    return tuple(t[keep].contiguous() for t in case[:3]) + tuple(case[3:])


def identity(shift=(0, 0), seed=0, W=32, H=24):
    """R = I, T = 0, equal intrinsics with a power-of-two focal length and integer principal points: every
    (un, vn) is exactly ux + du/2 + shift, an integer or half-integer, in float32 as in float64, so the
    taps' weights are exactly (1, 0) or (1/2, 1/2); aux = 0, so both gradients are exactly 0.  Every pixel
    of the image is a point.  shift (0, 0) with image_n = image_r: NCC = 1."""
    g = torch.Generator().manual_seed(4000 + seed)
    ys, xs = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
    uvs = torch.stack([xs.reshape(-1), ys.reshape(-1)], 1).int().contiguous()
    P = len(uvs)
    img = texture(g, H, W)
    K = dict(fx_r=64.0, fy_r=64.0, cx_r=16.0, cy_r=12.0, fx_n=64.0, fy_n=64.0, cx_n=16.0 + shift[0],
             cy_n=12.0 + shift[1])
    return ((torch.rand(P, generator=g) * 2 + 2).float(), facing(g, P), uvs, EYE.clone(), torch.zeros(3), img,
            img.clone(), K)


def low_texture(seed=0, P=2000, Wr=48, Hr=40, Wn=52, Hn=44, constant=False):
    """A constant plus noise whose amplitude grows across the image, so that the 49-tap variances spread over
    about [1e-6, 1e-4] around the 5e-6 gate (var_r var_n ~ 1e-10 << 1e-8: the reference's -ncc / (var_n + 1e-8)
    is not the exact derivative here).  The constant is small (0.01): the float32 sums of squares then carry
    the variance to ~1e-4 relative.  constant=True: both images exactly constant (variance 0)."""
    g = torch.Generator().manual_seed(5000 + seed)

    def img(H, W):
        if constant:
            return torch.full((H, W), 0.3)
        amp = torch.exp(torch.linspace(math.log(4e-4), math.log(1.2e-2), W))[None, :]
        # smooth noise (so that the half-pixel warp keeps its variance) on a small constant
        n = torch.nn.functional.interpolate(torch.rand(1, 1, H // 2 + 2, W // 2 + 2, generator=g) - 0.5,
                                            size=(H, W), mode="bilinear", align_corners=True)[0, 0]
        return (0.01 + amp * n).float().contiguous()

    uvs = torch.stack([torch.randint(3, Wr - 3, (P,), generator=g), torch.randint(3, Hr - 3, (P,), generator=g)], 1)
    return ((torch.rand(P, generator=g) * 2 + 2).float(), facing(g, P), uvs.int().contiguous(), rotation(g, 0.03),
            (torch.randn(3, generator=g) * 0.05).float(), img(Hr, Wr), img(Hn, Wn), intr(Wr, Hr, Wn, Hn))


def degenerate(seed=0, P=300, Wr=48, Hr=40, Wn=52, Hn=44):
    """An ordinary batch (integer cx_r, cy_r) with a few degenerate rows; returns (case, rows) with rows a dict
    of index lists.  perp: normals (+-1, 0, 0) at ux = cx_r and (0, +-1, 0) at uy = cy_r, so that
    distance = -(pnr . n) depth is exactly 0 in float32 however the dot product is contracted; zero: depth 0;
    bad: NaN or inf in depth or normal."""
    g = torch.Generator().manual_seed(6000 + seed)
    d, n, uv, R, T, ir, inn, K = ordinary(P, 60 + seed, Wr, Hr, Wn, Hn)
    K = dict(K, cx_r=24.0, cy_r=20.0)
    rows = {"perp": [10, 11, 12, 13], "zero": [20, 21], "bad": [30, 31, 32, 33, 34, 35]}
    uv, n, d = uv.clone(), n.clone(), d.clone()
    for i, (nv, at) in zip(rows["perp"], [((1.0, 0, 0), 0), ((-1.0, 0, 0), 0), ((0, 1.0, 0), 1), ((0, -1.0, 0), 1)]):
        n[i] = torch.tensor(nv)
        uv[i, at] = 24 if at == 0 else 20
    d[rows["zero"][0]] = 0.0
    d[rows["zero"][1]] = -0.0
    d[30], d[31], d[32] = float("nan"), float("inf"), float("-inf")
    n[33, 0], n[34, 1], n[35] = float("nan"), float("inf"), torch.tensor([float("nan")] * 3)
    return (d, n, uv.contiguous(), R, T, ir, inn, K), rows


def behind(seed=0, P=600, Wr=48, Hr=40, Wn=52, Hn=44):
    """The neighbour camera moved forward to about the surface (T.z = -3, depths in [2, 4]): H_uv.z <= 0 for
    whole patches (the plane behind the neighbour camera) and, at tilted normals near depth 3, for part of a
    patch."""
    g = torch.Generator().manual_seed(7000 + seed)
    d, n, uv, R, T, ir, inn, K = ordinary(P, 70 + seed, Wr, Hr, Wn, Hn)
    d = (torch.rand(P, generator=g) * 2 + 2).float()
    d[: P // 2] = 3.0 + (torch.rand(P // 2, generator=g) - 0.5) * 0.1
    n = facing(g, P, tilt=0.8)
    return d, n, uv, rotation(g, 0.02), torch.tensor([0.01, -0.02, -3.0]), ir, inn, K


def tiny_neighbour(Wn, Hn, seed=0, P=256, Wr=48, Hr=40):
    """A neighbour image of Wn x Hn (2: no warp can pass the margin; 5: 1.5 < un < 2.5 is the only room).  The
    neighbour's focal length is an eighth of the reference's, so a 3-pixel patch warps to 3/8 pixel and fits."""
    g = torch.Generator().manual_seed(8000 + seed)
    uvs = torch.stack([torch.randint(20, 29, (P,), generator=g), torch.randint(16, 25, (P,), generator=g)], 1)
    K = dict(fx_r=64.0, fy_r=64.0, cx_r=24.0, cy_r=20.0, fx_n=8.0, fy_n=8.0, cx_n=(Wn - 1) / 2, cy_n=(Hn - 1) / 2)
    return ((torch.rand(P, generator=g) * 2 + 2).float(), facing(g, P), uvs.int().contiguous(), rotation(g, 0.01),
            (torch.randn(3, generator=g) * 0.02).float(), texture(g, Hr, Wr), torch.rand(Hn, Wn, generator=g), K)


def _bisect_depth(case, q_of, lo, hi, tol, want, iters=24):
    """Per point, a float32 depth in [lo, hi] at which the deciding quantity q_of(reference result) is within
    tol of zero, by bisection on the float64 reference; points whose q has the same sign at both ends are
    dropped.  Returns (case at those points, with their depths)."""
    d0, n, uv = case[:3]

    def q_at(d):
        return q_of(NR.warp_patch_ncc(d, n, uv, *case[3:7], *case[7].values()))

    a, b = torch.full_like(d0, lo), torch.full_like(d0, hi)
    qa, qb = q_at(a), q_at(b)
    ok = np.isfinite(qa) & np.isfinite(qb) & ((qa > 0) != (qb > 0))
    first = torch.from_numpy(np.flatnonzero(ok)[: want + want // 2])  # (only bracketed points are refined)
    d0, n, uv, a, b, qa = d0[first], n[first], uv[first], a[first], b[first], qa[first.numpy()]
    ok = np.ones(len(d0), bool)
    out, done = d0.clone(), np.zeros(len(d0), bool)
    for _ in range(iters):
        m = ((a.double() + b.double()) * 0.5).float()
        qm = q_at(m)
        hit = ok & ~done & (np.abs(qm) < tol)
        out[torch.from_numpy(hit)] = m[torch.from_numpy(hit)]
        done |= hit
        left = torch.from_numpy((qm > 0) == (qa > 0))  # the root lies in [m, b]
        a, b = torch.where(left, m, a), torch.where(left, b, m)
    keep = torch.from_numpy(np.flatnonzero(done))
    return (out[keep].contiguous(), n[keep].contiguous(), uv[keep].contiguous()) + tuple(case[3:])


def margin_ties(seed=0, P=512, tol=2e-4):
    """neighbour_margin's poses with each depth moved until the nearest tap is within 2e-4 pixel of its bound:
    where the reference's float32 warp decides differently from float64, measured."""
    g = torch.Generator().manual_seed(3500 + seed)
    Wr, Hr, Wn, Hn, C = 48, 40, 40, 34, 12000
    uvs = torch.stack([torch.randint(2, Wr - 2, (C,), generator=g), torch.randint(2, Hr - 2, (C,), generator=g)],
                      1).int().contiguous()
    case = ((torch.rand(C, generator=g) * 2 + 2).float(), facing(g, C), uvs, rotation(g, 0.1),
            (torch.randn(3, generator=g) * 0.1).float(), texture(g, Hr, Wr), texture(g, Hn, Wn),
            intr(Wr, Hr, Wn, Hn, fx_n=50.0, fy_n=52.0))
    c = _bisect_depth(case, lambda r: r["margin_n"].min(1), 2.0, 4.0, tol, P)
    assert len(c[0]) >= P
    return tuple(t[:P].contiguous() for t in c[:3]) + tuple(c[3:])


def gate_ties(seed=0, P=512, tol=2e-3):
    """low_texture's images with each depth moved until var_n is within 0.2 % of the 5e-6 gate (var_r above
    it, the warp inside the margin)."""
    case = low_texture(seed, P=20000)
    case = case[:4] + ((case[4] * 4).contiguous(),) + case[5:]  # (more parallax: var_n moves with depth)

    def q_of(r):
        ok = (r["margin_n"].min(1) > 0.25) & (r["gate_r"] / NR.VAR_GATE > 0.05)
        return np.where(ok, r["gate_n"] / NR.VAR_GATE, np.nan)

    c = _bisect_depth(case, q_of, 2.0, 4.0, tol, P)
    assert len(c[0]) >= P, len(c[0])
    return tuple(t[:P].contiguous() for t in c[:3]) + tuple(c[3:])


BLOCK_P = (1, 255, 256, 257, 4099)
TIES = ("margin_ties", "gate_ties")  # built at the decision boundaries: they measure the band


def all_cases():
    """name -> (case, exact): every case of tests/test_gpu_ncc_edges.py.  exact: the warps are exact in float32
    (no rounding can move a decision), so `valid` has no ties."""
    deg, _ = degenerate()
    return {
        "reference_margin": (reference_margin(), False),
        "neighbour_margin": (neighbour_margin(), False),
        "identity": (identity(), True),
        "identity_shift": (identity((2, -1)), True),
        "low_texture": (low_texture(), False),
        "constant": (low_texture(constant=True, P=300), False),
        "degenerate": (deg, False),
        "behind": (behind(), False),
        "tiny_w2": (tiny_neighbour(2, 30), False),
        "tiny_h2": (tiny_neighbour(30, 2), False),
        "tiny_5x5": (tiny_neighbour(5, 5), False),
        "blocks": (ordinary(BLOCK_P[-1], 9), False),
        "grazing": (grazing(), False),
        "margin_ties": (margin_ties(), False),
        "gate_ties": (gate_ties(), False),
    }


def groups(ref, depths):
    """Points conditioned alike: by |distance| / depth (= |pnr . n|: grazing below 0.3) and by
    min(var_r, var_n) (below 1e-4, below 1e-2, above).  name -> bool [P] over the valid points."""
    with np.errstate(all="ignore"):
        graze = np.abs(ref["distance"] / NR._np(depths)) < 0.3
        v = np.minimum(ref["var_r"], ref["var_n"])
    out = {}
    for gn, gm in (("grazing", graze), ("facing", ~graze)):
        for vn, vm in (("var<1e-4", v < 1e-4), ("var<1e-2", (v >= 1e-4) & (v < 1e-2)), ("var>=1e-2", v >= 1e-2)):
            m = ref["valid"] & gm & vm
            if m.any():
                out[f"{gn},{vn}"] = m
    return out


def group_err(x, ref, mask):
    """Relative L2 error of x against ref over the masked points (finite figures only: a non-finite x gives
    inf); absolute where the reference is all zero."""
    x, ref = np.asarray(x, np.float64)[mask], np.asarray(ref, np.float64)[mask]
    if not np.isfinite(x).all():
        return float("inf")
    den = np.linalg.norm(ref)
    num = np.linalg.norm(x - ref)
    return float(num if den == 0 else num / den)


_EVAL = {}


def evaluated():
    """name -> (case, exact, float64 reference, oracle) of all_cases(), computed once per process and left
    unchanged."""
    if not _EVAL:
        from oracle import gsr_oracle as O
        for name, (c, exact) in all_cases().items():
            _EVAL[name] = (c, exact, NR.warp_patch_ncc(*c[:7], *c[7].values()),
                           O.warp_patch_ncc(*c[:7], *c[7].values()))
    return _EVAL


def bands():
    """(band_margin [pixels], band_gate [relative to 5e-6], measured_margin, measured_gate): four times the
    largest distance to a decision boundary at which the oracle (the reference's float32 arithmetic) decides
    `valid` differently from the float64 reference, over every case of this file.  The kernel's v_rcp_f32 and
    its reordered sums may add a few ulp over the reference's float32 arithmetic; a flip farther out than
    four times the reference's own is a bug."""
    mm = mg = 0.0
    for c, exact, ref, o in evaluated().values():
        m, g = NR.flip_bands(ref, o["valid"])
        mm, mg = max(mm, m), max(mg, g)
    return 4.0 * mm, 4.0 * mg, mm, mg
