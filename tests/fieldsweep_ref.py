"""numpy restatement of csrc/fieldsweep.hip, the yardstick of tests/test_gpu_fieldsweep.py.

Every function computes in float32, elementwise and in the kernels' operation
order (numpy fuses no multiply-add), so the kernels must match it bit for
bit.  tests/test_fieldsweep.py pins it to the reference's lines on torch's CPU
ops.  `mask_sample(..., dtype=np.float64)` is the same formula in float64: the
tests use it to keep every tested point's sample away from the 0.5 bar.

A view is a dict: R [3,3] and T [3] float32 (camera = points @ R + T), Fx, Fy,
Cx, Cy (Python floats), W, H, mask [H,W] float32.
"""
from __future__ import annotations

import numpy as np

F = np.float32


def view_constants(view):
    """uv = c + s * (camera.xy / camera.z): float64 on the host, then rounded (mesh_extract_tetrahedra.py:50-57)."""
    W, H = view["W"], view["H"]
    c = np.array([(view["Cx"] * 2.0 + 1.0) / W - 1.0, (view["Cy"] * 2.0 + 1.0) / H - 1.0], np.float64).astype(F)
    s = np.array([view["Fx"] * 2.0 / W, view["Fy"] * 2.0 / H], np.float64).astype(F)
    return c, s


def mask_sample(points, view, dtype=F):
    """The bilinear sample of view["mask"] at the projection of every row of `points` [n,3] (grid_sample with
    align_corners=True and zeros padding), in `dtype` arithmetic on the float32 inputs."""
    D = dtype
    W, H = view["W"], view["H"]
    p, R, T = points.astype(D), view["R"].astype(F).astype(D), view["T"].astype(F).astype(D)
    c, s = (a.astype(D) for a in view_constants(view))
    mask = view["mask"].astype(F).astype(D)
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    with np.errstate(all="ignore"):
        cx = ((x * R[0, 0] + y * R[1, 0]) + z * R[2, 0]) + T[0]
        cy = ((x * R[0, 1] + y * R[1, 1]) + z * R[2, 1]) + T[1]
        cz = ((x * R[0, 2] + y * R[1, 2]) + z * R[2, 2]) + T[2]
        gx, gy = c[0] + s[0] * (cx / cz), c[1] + s[1] * (cy / cz)
        ix, iy = ((gx + D(1)) * D(0.5)) * D(W - 1), ((gy + D(1)) * D(0.5)) * D(H - 1)
        x0, y0 = np.floor(ix), np.floor(iy)
        x1, y1 = x0 + D(1), y0 + D(1)
        tx, ty, sx, sy = ix - x0, iy - y0, x1 - ix, y1 - iy

        def tap(fx, fy, w, acc):  # a texel outside the plane adds nothing
            inb = (fx >= 0) & (fx <= D(W - 1)) & (fy >= 0) & (fy <= D(H - 1))
            xi, yi = np.where(inb, fx, 0).astype(np.int64), np.where(inb, fy, 0).astype(np.int64)
            return np.where(inb, acc + mask[yi, xi] * w, acc)

        acc = np.zeros(p.shape[0], D)
        acc = tap(x0, y0, sx * sy, acc)
        acc = tap(x1, y0, tx * sy, acc)
        acc = tap(x0, y1, sx * ty, acc)
        acc = tap(x1, y1, tx * ty, acc)
    assert acc.dtype == D
    return acc


def view_update(points, alpha, inside, view, weight, seen):
    """gsr_field_view_update: -> the new (weight [N] float32, seen [N] uint8).  `view` None: no mask.  The mask
    test is evaluated where `inside` is set only."""
    ok = np.asarray(inside).astype(bool).copy()
    if view is not None:
        idx = np.nonzero(ok)[0]
        ok[idx] = mask_sample(np.asarray(points, F)[idx], view) > F(0.5)
    alpha, weight = np.asarray(alpha, F), np.asarray(weight, F)
    smaller = ok & ((alpha < weight) | (alpha != alpha))
    return np.where(smaller, alpha, weight).astype(F), (np.asarray(seen, np.uint8) | ok.astype(np.uint8))


def finish(weight, seen):
    """gsr_field_finish: -> (sdf [N] float32, valid [N] bool)."""
    valid = np.asarray(seen) != 0
    return (F(0.5) - np.where(valid, np.asarray(weight, F), F(0))).astype(F), valid


def bisect_step(left, right, left_sdf, right_sdf, mid_sdf):
    """gsr_field_bisect_step: -> the new (left, right [E,3], left_sdf, right_sdf [E], mid [E,3]); points keep
    their dtype (float32 or float64), sdf is float32."""
    D = left.dtype.type
    m, l = np.asarray(mid_sdf, F).reshape(-1), np.asarray(left_sdf, F).reshape(-1)
    low = ((m < 0) & (l < 0)) | ((m > 0) & (l > 0))
    p = (left + right) * D(0.5)
    nl, nr = np.where(low[:, None], p, left), np.where(low[:, None], right, p)
    return (nl, nr, np.where(low, m, l), np.where(low, np.asarray(right_sdf, F).reshape(-1), m),
            ((nl + nr) * D(0.5)).astype(left.dtype))


# ---- test inputs ------------------------------------------------------------------------------------------------
MARGIN = 1e-3  # every tested point's float64 sample is farther than this from the 0.5 bar

KINDS = ("binary", "grey", "one", "one_dark", "odd", "corners")


def make_view(kind, seed=0):
    """A view of one of KINDS: a binary mask (a disc and two border strips) and a grey one at 64x48, two 1x1
    masks, a 7x5 mask with a non-centred principal point, and an 8x6 one whose constants make uv = +-1
    reachable exactly (R = I, T = 0, c = 0, s = 1)."""
    rng = np.random.default_rng([seed, KINDS.index(kind)])
    if kind == "corners":
        W, H, R, T = 8, 6, np.eye(3), np.zeros(3)
        cam = dict(Fx=4.0, Fy=3.0, Cx=3.5, Cy=2.5)
    else:
        W, H = {"binary": (64, 48), "grey": (64, 48), "one": (1, 1), "one_dark": (1, 1), "odd": (7, 5)}[kind]
        R, _ = np.linalg.qr(rng.standard_normal((3, 3)))
        if np.linalg.det(R) < 0:
            R[:, 0] = -R[:, 0]
        T = rng.uniform(-0.5, 0.5, 3)
        cam = dict(Fx=0.9 * W, Fy=0.85 * W, Cx=(W - 1) / 2, Cy=(H - 1) / 2)
        if kind == "odd":
            cam = dict(Fx=6.3, Fy=5.1, Cx=2.2, Cy=2.9)
    yy, xx = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    if kind == "binary":
        mask = ((((xx - 30.5) ** 2 + (yy - 22.0) ** 2) < 15.0 ** 2) | (xx >= 55) | (yy < 5)).astype(F)
    elif kind in ("one", "one_dark"):
        mask = np.full((1, 1), 0.8 if kind == "one" else 0.3, F)
    else:
        mask = np.clip(0.5 + 0.4 * np.sin(0.9 * xx + 0.3) * np.cos(0.7 * yy) + 0.2 * (rng.random((H, W)) - 0.5), 0, 1)
        mask = mask.astype(F)
    return dict(cam, R=R.astype(F), T=T.astype(F), W=W, H=H, mask=mask)


def draw_points(view, n, seed=0):
    """n world points in front of `view`'s camera under the margin rule: 70% project uniformly over the image
    and a quarter of its size around it, 30% into the one-texel band just outside a border (zeros padding
    blends in there).  A draw whose float64 sample lies within MARGIN of 0.5 is dropped and drawn again;
    fewer than 5% of the draws may be (the rule must not be what hides the border cases)."""
    rng = np.random.default_rng([seed, 77])
    c, s = (a.astype(np.float64) for a in view_constants(view))
    R, T = view["R"].astype(np.float64), view["T"].astype(np.float64)
    texel = 2.0 / np.array([max(view["W"] - 1, 1), max(view["H"] - 1, 1)])
    out, draws = [], 0
    while sum(len(p) for p in out) < n:
        k = n - sum(len(p) for p in out)
        g = rng.uniform(-1.25, 1.25, (k, 2))
        band = rng.random(k) < 0.3
        axis, side = rng.integers(0, 2, k), rng.choice([-1.0, 1.0], k)
        rows = np.nonzero(band)[0]
        g[rows, axis[rows]] = side[rows] * (1.0 + rng.random(len(rows)) * texel[axis[rows]])
        z = rng.uniform(0.5, 4.0, k)
        cam = np.concatenate([(g - c) / s * z[:, None], z[:, None]], 1)
        p = ((cam - T) @ np.linalg.inv(R)).astype(F)
        keep = np.abs(mask_sample(p, view, np.float64) - 0.5) > MARGIN
        out.append(p[keep])
        draws += k
    assert draws - n < 0.05 * draws, (draws, n)
    return np.concatenate(out)[:n]
