"""Case builders of the densification tests (plain numpy / torch, no GPU).

Shared by tests/test_densify.py (CPU: every case reaches the regime its name
says, with no decision inside the tie margin) and the GPU tests
(tests/test_gpu_densify.py, tests/test_gpu_densify_edges.py):

  Cam, layout, rows64         the final layout of a densification from its
                              inputs alone, and its float64 values and bounds
  random_case, regime_case    densification inputs by decision regime
  decisions, regime_report    the decisions in float64 with their margins
  select_*                    constructed inputs of the radix select
  filter_*, filter64,         cameras and points of the 3D filter, its float64
  margin_ok, seen_by          form and tie margin
  reset_case                  inputs of reset_opacity
"""
from __future__ import annotations

import math

import numpy as np
import torch

import densify_ref as R

U = 2.0 ** -24
SC3 = (0.0002, 0.05, 4.0)  # max_grad, min_opacity, extent of the generated cases
# The tie margins of the generated cases: a decision is at least this far (relative; the opacity in
# logit units) from its threshold, or an exact tie by construction.
TIE = {"hi": 0.05, "big": 0.05, "low": 0.04, "Q": 1e-5}


class Cam:
    def __init__(self, R_, T, whf):
        self.R, self.T = torch.tensor(R_), torch.tensor(T)
        self.image_width, self.image_height, self.Fx, self.Fy = int(whf[0]), int(whf[1]), float(whf[2]), float(whf[3])


# ---------------------------------------------------------------- the final layout
def layout(c):
    """Final rows (source, own noise row, the parent clone's noise row) of a golden case, derived
    from its inputs alone (the fixture's tie margin makes the decisions arithmetic-independent)."""
    max_grad, min_opacity, extent = (float(x) for x in c["scalars"])
    with np.errstate(invalid="ignore", divide="ignore"):
        gr = np.nan_to_num(c["accum"] / c["denom"], nan=0.0)
        ga = np.nan_to_num(c["accum_abs"] / c["denom"], nan=0.0)
    big = np.exp(c["in_scaling"].astype(np.float64)).max(axis=1) > 0.01 * extent
    low = 1 / (1 + np.exp(-c["in_opacity"][:, 0].astype(np.float64))) < min_opacity
    hi = gr >= np.float32(max_grad)
    clone, split, cs = hi & ~big, (hi & big) | (ga >= c["Q"]), bool(0.0 >= c["Q"])
    crank, srank = np.cumsum(clone) - clone, np.cumsum(split) - split
    C, So = int(clone.sum()), int(split.sum())
    S = So + (C if cs else 0)
    idx = np.arange(len(gr))
    rows = [(i, -1, -1) for i in idx[~split & ~low]]
    rows += [(i, crank[i], -1) for i in idx[clone & ~low]] if not cs else []
    for j in range(2):
        rows += [(i, C + j * S + srank[i], -1) for i in idx[split & ~low]]
        if cs:
            rows += [(i, C + j * S + So + crank[i], crank[i]) for i in idx[clone & ~low]]
    return np.array(rows, np.int64).reshape(-1, 3), C, S


def rows64(c, rows, C):
    """float64 new positions and scalings of `rows`, with the two bounds."""
    Rm = R.rotation_matrices(torch.tensor(c["in_rotation"]).double()).numpy()
    s = c["in_scaling"].astype(np.float64)
    xyz, eps = c["in_xyz"].astype(np.float64), c["noise"].astype(np.float64)
    src, own, par = rows[:, 0], rows[:, 1], rows[:, 2]
    new = own >= 0
    base = xyz[src].copy()
    hp = par >= 0
    base[hp] += np.einsum("nij,nj->ni", Rm[src[hp]], np.exp(s[src[hp]]) * eps[par[hp]])
    v = np.zeros_like(base)
    v[new] = np.exp(s[src[new]]) * eps[own[new]]
    pos = base + np.einsum("nij,nj->ni", Rm[src], v)
    pos_bound = 16 * U * (np.abs(base) + np.einsum("nij,nj->ni", np.abs(Rm[src]), np.abs(v)))
    child = own >= C
    sc = s[src].copy()
    sc[child] = np.log(np.exp(sc[child]) / 1.6)
    sc_bound = 8 * U * np.maximum(1.0, np.minimum(np.abs(sc), np.abs(s[src])))
    return pos, pos_bound, sc, sc_bound, new, child


def as_fixture(case, Q, used):
    """A generated case in the key layout of a golden case, for `layout` and `rows64`."""
    params, (accum, accum_abs, denom), _, noise, sc3 = case
    c = {"in_" + n: v for n, v in params.items()}
    c.update(accum=accum, accum_abs=accum_abs, denom=denom, scalars=np.array(sc3, np.float64), Q=np.float32(Q),
             noise=noise[:used].numpy())
    return c


# ------------------------------------------------------------- densification inputs
def random_case(P, seed, sg=True, low_all_but_one=False):
    """Inputs whose decisions sit far from every threshold (values from well-separated sets)."""
    rng = np.random.default_rng(seed)
    max_grad, min_opacity, extent = 0.0002, 0.05, 4.0
    nsg = 1 if sg else 0
    op = rng.standard_normal((P, 1)) * 2.0
    thr = math.log(min_opacity / (1 - min_opacity))
    op[np.abs(op - thr) < 0.05] += 0.2
    if low_all_but_one:
        op[:] = -6.0
        op[P // 2] = 1.0
    sc = np.log(0.01 * extent * rng.choice([0.2, 0.5, 0.8, 1.5, 3.0], (P, 3))) - rng.random((P, 3)) * 0.1
    params = dict(xyz=rng.standard_normal((P, 3)) * 2, f_dc=rng.standard_normal((P, 1, 3)),
                  f_rest=rng.standard_normal((P, 3, 3)) * 0.1, opacity=op, scaling=sc,
                  rotation=rng.standard_normal((P, 4)), sg_axis=rng.standard_normal((P, nsg, 3)),
                  sg_sharpness=rng.standard_normal((P, nsg)), sg_color=rng.standard_normal((P, nsg, 3)))
    params = {k: v.astype(np.float32) for k, v in params.items()}
    denom = rng.integers(0, 20, P).astype(np.float32)
    accum = (max_grad * rng.choice([0.3, 0.7, 1.5, 3.0], P) * denom).astype(np.float32)
    accum_abs = (np.exp(rng.standard_normal(P)) * max_grad * 2 * denom * (rng.random(P) < 0.7)).astype(np.float32)
    moments = {n: ((rng.standard_normal(v.shape) * 0.01).astype(np.float32),
                   (rng.random(v.shape) * 1e-4).astype(np.float32)) for n, v in params.items()}
    noise = torch.randn((5 * P, 3), generator=torch.Generator().manual_seed(seed))
    return params, (accum, accum_abs, denom), moments, noise, (max_grad, min_opacity, extent)


REGIMES = ("mixed", "resplit", "all_hi", "all_hi_min0", "none_hi_k1", "none_hi_k5", "nostats", "all_low")
SHARED_MAX = 0.125  # grads_abs of the points that share the maximum in `none_hi_k*` (a power of two)


def regime_case(P, seed, regime, sh_rest=3, sg=1):
    """`random_case` by decision regime, with `f_dc` rows holding their own index (exact below 2^24)
    so that an output row names its source.  Every value comes from a well-separated set: `hi` from
    grads = max_grad * {0.3, 0.7 | 1.5, 3}, `big` from max exp(s) = limit * {<= 0.8 | >= 1.35}, `low`
    from raw opacities 0.05 away from the threshold's, `>= Q` from grads_abs that are 0 or distinct
    points of a geometric grid of ratio 1.001 (mixed, all_low: a log-normal draw; the CPU test of the
    builders holds each case to the margin).

      mixed        half the points hi, a third of grads_abs zero: Q > 0
      resplit      ~57% hi and ~2/3 of grads_abs zero: Q == 0, every clone is split again
      all_hi       denom > 0 and grads >= max_grad everywhere: q = 0, Q = min(grads_abs) > 0
      all_hi_min0  the same with a tenth of grads_abs zero: Q == 0
      none_hi_k1   no point hi (denom == 0 rows included): q = 1, Q = max(grads_abs), held by one
      none_hi_k5   point or by five (accum_abs = 2^-3 * denom: the quotients are the same bits)
      nostats      denom all zero (the statistics of unseen points are zero with it)
      all_low      mixed, with every opacity below the threshold: N = 0
    """
    if regime not in REGIMES:
        raise ValueError(regime)
    rng = np.random.default_rng(seed)
    max_grad, min_opacity, extent = SC3
    thr = math.log(min_opacity / (1 - min_opacity))
    op = rng.standard_normal((P, 1)) * 2.0
    op[np.abs(op - thr) < 0.05] += 0.2
    if regime == "all_low":
        op = thr - 0.5 - 4.0 * rng.random((P, 1))
    sc = np.log(0.01 * extent * rng.choice([0.2, 0.5, 0.8, 1.5, 3.0], (P, 3))) - rng.random((P, 3)) * 0.1
    index = np.arange(P, dtype=np.float64)
    params = dict(xyz=rng.standard_normal((P, 3)) * 2, f_dc=np.repeat(index[:, None, None], 3, axis=2),
                  f_rest=rng.standard_normal((P, sh_rest, 3)) * 0.1, opacity=op, scaling=sc,
                  rotation=rng.standard_normal((P, 4)), sg_axis=rng.standard_normal((P, sg, 3)),
                  sg_sharpness=rng.standard_normal((P, sg)), sg_color=rng.standard_normal((P, sg, 3)))
    params = {k: v.astype(np.float32) for k, v in params.items()}

    denom = rng.integers(0, 20, P)
    grid = max_grad * 0.5 * 1.001 ** rng.permutation(P)  # distinct, neighbours 1e-3 apart
    lognormal = np.exp(rng.standard_normal(P)) * max_grad * 2
    coin = rng.random(P)
    if regime in ("mixed", "all_low"):
        level, ga = rng.choice([0.3, 0.7, 1.5, 3.0], P), lognormal * (coin < 0.7)
    elif regime == "resplit":
        level, ga = rng.choice([0.3, 0.7, 1.5, 3.0], P, p=[0.2, 0.2, 0.3, 0.3]), grid * (coin < 0.35)
    elif regime in ("all_hi", "all_hi_min0"):
        denom = rng.integers(1, 20, P)
        level, ga = rng.choice([1.5, 3.0], P), grid * (coin < 0.9 if regime == "all_hi_min0" else 1.0)
    elif regime in ("none_hi_k1", "none_hi_k5"):
        level, ga = rng.choice([0.3, 0.7], P), grid * (coin < 0.7)
        if not (denom > 0).any():
            denom[rng.integers(0, P)] = 7
        k = min(int(regime[-1]), int((denom > 0).sum()))
        ga[rng.choice(np.flatnonzero(denom > 0), k, replace=False)] = SHARED_MAX
    else:  # nostats
        denom = np.zeros(P, np.int64)
        level, ga = rng.choice([0.3, 0.7, 1.5, 3.0], P), grid
    denom = denom.astype(np.float32)
    accum = (max_grad * level * denom).astype(np.float32)
    accum_abs = (ga * denom).astype(np.float32)
    moments = {n: ((rng.standard_normal(v.shape) * 0.01).astype(np.float32),
                   (rng.random(v.shape) * 1e-4).astype(np.float32)) for n, v in params.items()}
    noise = torch.randn((5 * P, 3), generator=torch.Generator().manual_seed(seed))
    return params, (accum, accum_abs, denom), moments, noise, SC3


def _wide(cases):
    return [c + (15, 7) for c in cases]  # f_rest 45 wide (SH 3), seven SG lobes: 21 / 7 / 21


# (regime, P, seed[, sh_rest, sg]) of the GPU tests; the CPU test holds each to its regime
REGIME_CASES = (
    [("mixed", P, seed) for P, seed in ((255, 11255), (256, 1256), (257, 11257), (511, 1511), (512, 1512))] + _wide([("mixed", P, 1000 + P) for P in (1025, 4099)])
    + [("resplit", P, 2000 + P) for P in (255, 256, 257, 511, 512)]
    + _wide([("resplit", P, 2000 + P) for P in (1025, 4099)])
    + [("all_hi", P, 3000 + P) for P in (255, 256, 257, 512, 1025)]
    + [("all_hi_min0", P, 4000 + P) for P in (255, 256, 257, 512, 1025, 4099)]
    + [("none_hi_k1", P, 5000 + P) for P in (255, 256, 257, 511, 1025)]
    + [("none_hi_k5", P, 6000 + P) for P in (255, 256, 257, 511, 1025)]
    + [("nostats", P, 7000 + P) for P in (256, 257, 1025)]
    + [("all_low", 257, 8257)])


def regime_id(c):
    return f"{c[0]}-P{c[1]}" + ("-wide" if len(c) > 3 else "")


def select_ranks(n, q):
    """rank = q (n - 1) in fp32, its floor and ceiling and the weight, as ATen's quantile."""
    rank = np.float32(min(max(q, 0.0), 1.0)) * np.float32(n - 1)
    lo, hi = int(np.floor(rank)), int(np.ceil(rank))
    lo, hi = min(max(lo, 0), n - 1), min(max(hi, 0), n - 1)
    return lo, hi, float(rank - np.float32(lo))


def decisions(case, Q):
    """The decisions of a case in float64, given the Q of the run, and the least distance of each
    kind of decision from its threshold (`Q`: over the grads_abs that are not Q's own bits)."""
    params, (accum, accum_abs, denom), _, _, (max_grad, min_opacity, extent) = case
    with np.errstate(invalid="ignore", divide="ignore"):
        ga32 = np.nan_to_num(accum_abs / denom, nan=0.0)  # fp32, IEEE: the bits both sides compare
        gr = np.nan_to_num(accum.astype(np.float64) / denom, nan=0.0)
    ga = ga32.astype(np.float64)
    Q32 = np.float32(Q)
    ms = np.exp(params["scaling"].astype(np.float64)).max(axis=1)
    o = params["opacity"][:, 0].astype(np.float64)
    thr = math.log(min_opacity / (1 - min_opacity))
    hi, big, low = gr >= max_grad, ms > 0.01 * extent, o < thr
    off = ga32 != Q32
    margins = {"hi": float(np.abs(gr / max_grad - 1).min()), "big": float(np.abs(ms / (0.01 * extent) - 1).min()),
               "low": float(np.abs(o - thr).min()),
               "Q": float((np.abs(ga[off] - float(Q32)) / max(float(Q32), max_grad)).min()) if off.any() else math.inf}
    lo_k, hi_k, w = select_ranks(len(ga32), 1.0 - float(np.float32(hi.sum()) / np.float32(len(ga32))))
    s = np.sort(ga32)
    return {"hi": hi, "big": big, "low": low, "clone": hi & ~big, "split": (hi & big) | (ga32 >= Q32),
            "csplit": bool(0.0 >= Q32), "ties": int((~off).sum()), "margins": margins,
            "stats": (s[lo_k], s[hi_k], w), "ga": ga32}


def regime_report(case, Q):
    """None when every decision of `case` is outside the tie margin or an exact tie by construction
    (grads_abs equal to Q only where Q is one order statistic: both equal, or weight 0), else what is not."""
    d = decisions(case, Q)
    m = d["margins"]
    bad = [f"{k}: {m[k]:.3g} < {TIE[k]}" for k in TIE if m[k] < TIE[k]]
    a, b, w = d["stats"]
    if d["ties"] and not (a == b or w == 0.0):
        bad.append(f"{d['ties']} grads_abs equal an interpolated Q")
    if 0.0 < Q < 0.01 * case[4][0]:
        bad.append(f"Q = {Q:.3g} is within rounding of 0")
    return "; ".join(bad) or None


# ------------------------------------------------------------------- radix select
def from_bits(bits):
    return np.asarray(bits, np.uint32).view(np.float32)


SELECT_Q = (0.3, 0.7)  # at n = 257 and 5000 the weights fall on both sides of 0.5
SELECT_BASE = 0x3F404040  # 0.7509...: every byte can move either way without leaving the positive floats


def diverging_pair(byte):
    """Two bit patterns that first differ (from the top) in `byte` (3: the first pass ... 0: the last)."""
    return SELECT_BASE, SELECT_BASE + (1 << (8 * byte))


def digit255_pair(byte):
    """Two neighbours whose digit in `byte` (2, 1 or 0) is 255 for the lower one (and for both when byte > 0)."""
    a = SELECT_BASE | (0xFF << (8 * byte))
    return a, a + (1 << (8 * (byte - 1)) if byte else 1)


def select_pair_case(n, q, a_bits, b_bits, seed):
    """`n` shuffled non-negative floats whose two order statistics at quantile `q` are the bit patterns
    `a_bits` < `b_bits`; the rest lies below and above them, half of it a few bits away (sharing their
    leading bytes), half anywhere.  Returns (values, lo, hi, weight)."""
    lo, hi, w = select_ranks(n, q)
    assert hi == lo + 1 and a_bits < b_bits < 0x7F800000
    rng = np.random.default_rng(seed)

    def around(count, anchor, sign):
        near = 1 + (rng.integers(0, 1 << 16, count) >> rng.integers(0, 16, count))
        far = rng.integers(1, anchor if sign < 0 else 0x7F800000 - anchor, count)
        return anchor + sign * np.where(rng.random(count) < 0.5, near, far)

    bits = np.concatenate([around(lo, a_bits, -1), [a_bits, b_bits], around(n - 1 - hi, b_bits, +1)])
    assert bits.min() >= 0 and bits.max() < 0x7F800000
    return from_bits(rng.permutation(bits)), lo, hi, w


TIE_KINDS = ("inside", "begins_at_lo", "ends_at_hi", "begins_at_hi", "ends_at_lo")


def select_tie_case(n, q, kind, run=300, seed=0):
    """`n` shuffled floats with one run of `run` equal values placed against the two ranks of `q`; every
    other value is a distinct neighbouring bit pattern, so a rank that is off by one changes the result."""
    lo, hi, w = select_ranks(n, q)
    assert hi == lo + 1
    start = {"inside": lo - run // 2, "begins_at_lo": lo, "ends_at_hi": hi - run + 1, "begins_at_hi": hi,
             "ends_at_lo": lo - run + 1}[kind]
    assert 0 < start and start + run < n
    v = 0x3F4080F0
    bits = np.concatenate([v - start + np.arange(start), np.full(run, v), v + 1 + np.arange(n - start - run)])
    return from_bits(np.random.default_rng(seed).permutation(bits)), lo, hi, w, from_bits([v])[0]


def consecutive_values(n, seed=0):
    """`n` shuffled floats with neighbouring bit patterns (distinct: every rank has its own value)."""
    return from_bits(np.random.default_rng(seed).permutation(0x3F407F00 + np.arange(n)))


# ---------------------------------------------------------------------- 3D filter
def filter64(xyz, cams):
    """float64 filter, the seen mask and the issue's bound 4 u (sum|x_i R_i2| + |T_2|) sqrt(0.2) / F."""
    x = xyz.astype(np.float64)
    dist = np.full(len(x), np.inf)
    M = np.zeros(len(x))
    F = max(c.Fx for c in cams)
    for c in cams:
        Rm, T = c.R.double().numpy(), c.T.double().numpy()
        pc = x @ Rm + T
        z = pc[:, 2]
        with np.errstate(divide="ignore", invalid="ignore"):
            ok = (z > 0.2) & (np.abs(pc[:, 0] / z) <= c.image_width / c.Fx * 0.575) & \
                 (np.abs(pc[:, 1] / z) <= c.image_height / c.Fy * 0.575)
        better = ok & (z < dist)
        dist[better] = z[better]
        M[better] = (np.abs(x) @ np.abs(Rm[:, 2]) + abs(T[2]))[better]
    seen = np.isfinite(dist)
    far = np.argmax(np.where(seen, dist, -np.inf))
    dist[~seen], M[~seen] = dist[far], M[far]
    return dist / F * math.sqrt(0.2), seen, 4 * U * M * math.sqrt(0.2) / F


def margin_ok(xyz, cams, m=1e-5):
    """Points within the tie margin of z = 0.2 or a frustum bound of any camera."""
    x = xyz.astype(np.float64)
    bad = np.zeros(len(x), bool)
    for c in cams:
        pc = x @ c.R.double().numpy() + c.T.double().numpy()
        z = pc[:, 2]
        bad |= np.abs(z - 0.2) <= m * 0.2
        for k, b in ((0, c.image_width / c.Fx * 0.575), (1, c.image_height / c.Fy * 0.575)):
            bad |= (z > 0.1) & (np.abs(np.abs(pc[:, k] / z) - b) <= m * b)
    return bad


def seen_by(xyz, cams):
    """[n_cam, P]: camera k sees point i, and [n_cam, P] its depth there (float64, filter64's rule)."""
    x = xyz.astype(np.float64)
    ok, depth = np.zeros((len(cams), len(x)), bool), np.zeros((len(cams), len(x)))
    for k, c in enumerate(cams):
        pc = x @ c.R.double().numpy() + c.T.double().numpy()
        z = pc[:, 2]
        with np.errstate(divide="ignore", invalid="ignore"):
            ok[k] = (z > 0.2) & (np.abs(pc[:, 0] / z) <= c.image_width / c.Fx * 0.575) & \
                    (np.abs(pc[:, 1] / z) <= c.image_height / c.Fy * 0.575)
        depth[k] = z
    return ok, depth


def yaw_cam(th, T, F):
    Rm = np.array([[math.cos(th), 0, math.sin(th)], [0, 1, 0], [-math.sin(th), 0, math.cos(th)]], np.float32)
    return Cam(Rm, np.asarray(T, np.float32), (64, 48, F, F * 1.02))


def _clear_margin(xyz, cams, rng):
    for _ in range(50):  # the tie margin: move the few points that sit on a threshold
        bad = margin_ok(xyz, cams)
        if not bad.any():
            break
        xyz[bad] += (rng.standard_normal((int(bad.sum()), 3)) * 1e-2).astype(np.float32)
    assert not margin_ok(xyz, cams).any()
    return xyz


def filter_random_case(P, n_cam):
    """Cameras turned about y by up to 0.6 rad in front of a cloud, one point behind all of them."""
    rng = np.random.default_rng(1000 * P + n_cam)
    cams = []
    for k in range(n_cam):
        th = rng.uniform(-0.6, 0.6)
        Rm = np.array([[math.cos(th), 0, math.sin(th)], [0, 1, 0], [-math.sin(th), 0, math.cos(th)]], np.float32)
        F = float(rng.uniform(50, 80))
        cams.append(Cam(Rm, (rng.standard_normal(3) * 0.2).astype(np.float32), (64, 48, F, F * 1.02)))
    xyz = (rng.standard_normal((P, 3)) * np.array([1.5, 1.0, 1.0])).astype(np.float32)
    xyz[:, 2] = rng.uniform(0.5, 6.0, P)
    if P > 1:
        xyz[P // 2] = (0.0, 0.0, -5.0)  # behind every camera
    else:
        xyz[0] = (0.05, -0.02, 3.0)
    return _clear_margin(xyz, cams, rng), cams


def filter_slot_case(n_cam, slots, P=257, seed=0):
    """A narrow cloud in front of the origin, `n_cam` cameras that all look away from it, and at
    `slots` cameras that see all of it: the first at the greatest depth, each later one nearer."""
    rng = np.random.default_rng(seed + 131 * n_cam + sum(slots))
    xyz = np.stack([rng.uniform(-0.3, 0.3, P), rng.uniform(-0.2, 0.2, P), rng.uniform(2.0, 5.0, P)], 1).astype(np.float32)
    cams = [yaw_cam(math.pi + rng.uniform(-0.5, 0.5), rng.standard_normal(3) * 0.2, float(rng.uniform(50, 80)))
            for _ in range(n_cam)]
    for j, k in enumerate(slots):
        cams[k] = yaw_cam(0.1 - 0.03 * j, (0.05, -0.02, 0.3 + 1.5 * (len(slots) - 1 - j)), 55.0 + j)
    return _clear_margin(xyz, cams, rng), cams


# (n_cam, the slots of the cameras that see the cloud): the ends of the 64-camera staging chunks
FILTER_SLOT_CASES = [(130, (k,)) for k in (0, 63, 64, 127, 129)] + [(64, (63,)), (65, (64,)), (128, (127,))] \
    + [(130, pair) for pair in ((0, 63), (63, 64), (64, 127), (127, 129), (0, 129))]


def filter_blocks_case(seen_last, P=600, seed=0):
    """Three cameras near the origin looking along +z; the points of one end block (of 256) in front
    of them, every other point behind: the unseen take a maximum that another block found."""
    rng = np.random.default_rng(seed + int(seen_last))
    cams = [yaw_cam(rng.uniform(-0.2, 0.2), rng.standard_normal(3) * 0.1, float(rng.uniform(50, 80))) for _ in range(3)]
    xyz = np.stack([rng.uniform(-0.3, 0.3, P), rng.uniform(-0.2, 0.2, P), rng.uniform(2.0, 5.0, P)], 1).astype(np.float32)
    front = np.arange(P) >= 512 if seen_last else np.arange(P) < 256
    xyz[~front, 2] *= -1
    return _clear_margin(xyz, cams, rng), cams, front


def filter_exact_case():
    """The identity camera (camera space is world space, every product exact) and points exactly on
    and one float past each threshold: (xyz [11,3], cams, seen [11])."""
    cam = Cam(np.eye(3, dtype=np.float32), np.zeros(3, np.float32), (64, 48, 64.0, 60.0))
    bx, by = np.float32(64 / 64.0 * 0.575), np.float32(48 / 60.0 * 0.575)  # as camera_records rounds them
    up = lambda v: np.nextafter(np.float32(v), np.float32(np.inf))
    z0 = np.float32(0.2)
    pts = [((0, 0, z0), False), ((0, 0, up(z0)), True),
           ((bx, 0, 1), True), ((up(bx), 0, 1), False), ((-bx, 0, 1), True), ((-up(bx), 0, 1), False),
           ((0, by, 1), True), ((0, up(by), 1), False), ((0, -by, 1), True), ((0, -up(by), 1), False),
           ((0, 0, 2.5), True)]
    return np.array([p for p, _ in pts], np.float32), [cam], np.array([s for _, s in pts])


# ------------------------------------------------------------------ reset_opacity
def reset_case(P, kind, seed=0):
    """(params, filter [P,1]) for reset_opacity: scales of 0.01-0.1, raw opacities N(0, 3) with +15 and
    -15 at the ends; `kind`: "zero" (the state after reset_3D_filter: coef is 1), "large" (ten to a
    hundred times the scales: coef ~ 1e-5 and the cap at 0.01 never binds) or "mixed" (about the scales)."""
    rng = np.random.default_rng(seed + P)
    params = regime_case(P, seed + P, "mixed")[0]
    s = np.log(rng.uniform(0.01, 0.1, (P, 3)))
    o = rng.standard_normal((P, 1)) * 3
    o[0] = 15.0
    if P > 1:
        o[-1] = -15.0
    params["scaling"], params["opacity"] = s.astype(np.float32), o.astype(np.float32)
    f = {"zero": np.zeros((P, 1)), "large": rng.uniform(1.0, 5.0, (P, 1)), "mixed": rng.uniform(0.005, 0.2, (P, 1))}[kind]
    return params, f.astype(np.float32)
