"""A plain numpy statement of view_color_grads_kernel (csrc/view_grads.hip): the
SH and SG gradient rows of a view-parallel step rebuilt from every view's DC
row and camera centre.

`rebuild(..., dtype=np.float64)` is the reference the GPU tests compare the
kernel with.  `rebuild(..., dtype=np.float32)` is the same arithmetic with
every operation rounded to float32 (numpy rounds after each ufunc, so there is
no FMA), in the kernel's order of operations; it is used only to size the
tolerance: the worst |f32 - f64| / (2^-24 S) over the GPU tests' input families
is `C_KIND[kind]`, and the bar the kernel is held to is

    4 * C_KIND[kind] * 2^-24 * S + 1e-30        per element,

the factor 4 for what the restatement lacks (FMA contraction, the device's
expf, the rounding of its division and square root).  S is the magnitude of an
element's sum, sum_v |term_v| with every monomial of the term taken in absolute
value — the monomials of Y_k, the three products of a . d and its "- 1", the
three products of s = sum_c sg_color[c] dR[c] — so cancellation inside a term
counts as magnitude, as cancellation between the views does.

The SH basis is written from the constants of csrc/gsr_math.h (sh_basis); the
colour model is the forward's (preprocess_fwd.hip, oracle/gsr_oracle.c
color_from_shsg), which uses the SG axis as given, un-normalised.
"""
from __future__ import annotations

import numpy as np

SH_C0 = 0.28209479177387814
SH_C1 = 0.4886025119029199
SH_C2 = (1.0925484305920792, -1.0925484305920792, 0.31539156525252005, -1.0925484305920792, 0.5462742152960396)
SH_C3 = (-0.5900435899266435, 2.890611442640554, -0.4570457994644658, 0.3731763325901154, -0.4570457994644658,
         1.445305721320277, -0.5900435899266435)
MAX_SG = 7  # kMaxSG: lobes past it are written as zero

KINDS = ("sh", "sg_axis", "sg_sharpness", "sg_color")
U = 2.0 ** -24

# The worst |rebuild(float32) - rebuild(float64)| / (2^-24 S) over FAMILIES, per output kind, rounded up
# (tests/test_viewgrads_ref.py measures them again and asserts that these are still at least the measured values).
# Measured: sh 9.44 (deg_sh3_16_sg7_9), sg_axis 166.0, sg_sharpness 165.4, sg_color 168.7 (all chunk_P1000_1000: a
# lobe with sharpness near 30 and |a| near 1.5, where expf turns the rounding of a . d - 1 into ~150 ulp of g).
C_KIND = {"sh": 9.5, "sg_axis": 167.0, "sg_sharpness": 166.0, "sg_color": 169.0}


def bar(kind: str, S):
    """The per-element bar of the module docstring for the kernel's output `kind`."""
    return 4.0 * C_KIND[kind] * U * np.asarray(S, dtype=np.float64) + 1e-30


def sh_basis(x, y, z, degree: int, const=float):
    """(Y, A): the 16 basis values Y_k(x, y, z) in gsr_math.h's order of operations (entries past the degree
    are None) and A_k, the same with every monomial in absolute value.  Works on numpy arrays and torch
    tensors; `const` makes a constant of the arithmetic's type."""
    c = const
    Y = [c(SH_C0) + 0 * x] + [None] * 15
    A = [c(SH_C0) + 0 * x] + [None] * 15
    if degree > 0:
        c1 = c(SH_C1)
        Y[1], Y[2], Y[3] = -c1 * y, c1 * z, -c1 * x
        A[1], A[2], A[3] = c1 * abs(y), c1 * abs(z), c1 * abs(x)
    if degree > 1:
        xx, yy, zz, xy, yz, xz = x * x, y * y, z * z, x * y, y * z, x * z
        k = [c(v) for v in SH_C2]
        Y[4], A[4] = k[0] * xy, abs(k[0]) * abs(xy)
        Y[5], A[5] = k[1] * yz, abs(k[1]) * abs(yz)
        Y[6], A[6] = k[2] * (c(2.0) * zz - xx - yy), abs(k[2]) * (c(2.0) * zz + xx + yy)
        Y[7], A[7] = k[3] * xz, abs(k[3]) * abs(xz)
        Y[8], A[8] = k[4] * (xx - yy), abs(k[4]) * (xx + yy)
    if degree > 2:
        k = [c(v) for v in SH_C3]
        ax, ay, az = abs(x), abs(y), abs(z)
        Y[9], A[9] = k[0] * y * (c(3.0) * xx - yy), abs(k[0]) * ay * (c(3.0) * xx + yy)
        Y[10], A[10] = k[1] * xy * z, abs(k[1]) * abs(xy) * az
        Y[11], A[11] = k[2] * y * (c(4.0) * zz - xx - yy), abs(k[2]) * ay * (c(4.0) * zz + xx + yy)
        Y[12], A[12] = (k[3] * z * (c(2.0) * zz - c(3.0) * xx - c(3.0) * yy),
                        abs(k[3]) * az * (c(2.0) * zz + c(3.0) * xx + c(3.0) * yy))
        Y[13], A[13] = k[4] * x * (c(4.0) * zz - xx - yy), abs(k[4]) * ax * (c(4.0) * zz + xx + yy)
        Y[14], A[14] = k[5] * z * (xx - yy), abs(k[5]) * az * (xx + yy)
        Y[15], A[15] = k[6] * x * (xx - c(3.0) * yy), abs(k[6]) * ax * (xx + c(3.0) * yy)
    return Y, A


def rebuild(gathered_rows, campos, means3D, sh_degree: int, SHM: int, sg_degree: int, SGM: int, sg_axis=None,
            sg_sharpness=None, sg_color=None, dtype=np.float64):
    """(grads, S): dicts over KINDS of the summed gradient rows — sh [P, SHM, 3], sg_axis [P, SGM, 3],
    sg_sharpness [P, SGM], sg_color [P, SGM, 3] — and of their magnitudes S (module docstring), from the views'
    DC rows `gathered_rows` [n_views, P, 3] and camera centres `campos` [n_views, 3], all arithmetic in `dtype`.
    The views are summed in order; rows past the active degrees are zero."""
    dt = np.dtype(dtype).type
    rows = np.asarray(gathered_rows).astype(dt)
    cams = np.asarray(campos).astype(dt)
    m = np.asarray(means3D).astype(dt)
    n_views, P = rows.shape[0], rows.shape[1]
    n = (sh_degree + 1) ** 2
    sgd = min(sg_degree, SGM, MAX_SG)
    z = lambda *s: np.zeros(s, dtype=dt)  # noqa: E731
    out = {"sh": z(P, SHM, 3), "sg_axis": z(P, SGM, 3), "sg_sharpness": z(P, SGM), "sg_color": z(P, SGM, 3)}
    S = {k: np.zeros_like(v) for k, v in out.items()}
    if sgd:
        a = np.asarray(sg_axis).astype(dt)
        lam = np.asarray(sg_sharpness).astype(dt)
        col = np.asarray(sg_color).astype(dt)
    one, c0 = dt(1.0), dt(SH_C0)
    with np.errstate(invalid="ignore", divide="ignore"):
        for v in range(n_views):
            g = rows[v]
            do = m - cams[v, :3]
            dlen = np.sqrt(do[:, 0] * do[:, 0] + do[:, 1] * do[:, 1] + do[:, 2] * do[:, 2])
            d = do / dlen[:, None]
            x, y, zc = d[:, 0], d[:, 1], d[:, 2]
            dR = g / c0
            Y, A = sh_basis(x, y, zc, sh_degree, dt)
            out["sh"][:, 0] += g
            S["sh"][:, 0] += np.abs(g)
            for k in range(1, n):
                out["sh"][:, k] += Y[k][:, None] * dR
                S["sh"][:, k] += A[k][:, None] * np.abs(dR)
            for l in range(sgd):
                al = a[:, l]
                aux = (al[:, 0] * x + al[:, 1] * y + al[:, 2] * zc) - one
                aux_abs = (np.abs(al[:, 0] * x) + np.abs(al[:, 1] * y) + np.abs(al[:, 2] * zc)) + one
                gs = np.exp(lam[:, l] * aux)
                out["sg_color"][:, l] += dR * gs[:, None]
                S["sg_color"][:, l] += np.abs(dR) * gs[:, None]
                cl = col[:, l]
                s = cl[:, 0] * dR[:, 0] + cl[:, 1] * dR[:, 1] + cl[:, 2] * dR[:, 2]
                s_abs = np.abs(cl[:, 0] * dR[:, 0]) + np.abs(cl[:, 1] * dR[:, 1]) + np.abs(cl[:, 2] * dR[:, 2])
                dexp = s * gs
                out["sg_sharpness"][:, l] += dexp * aux
                S["sg_sharpness"][:, l] += s_abs * gs * aux_abs
                daux = dexp * lam[:, l]
                out["sg_axis"][:, l] += daux[:, None] * d
                S["sg_axis"][:, l] += (s_abs * gs * np.abs(lam[:, l]))[:, None] * np.abs(d)
    return out, S


def dc_sum_f32(gathered_rows):
    """The DC row exactly as the kernel forms it: the float32 sum of the views' rows in view order, from 0."""
    rows = np.asarray(gathered_rows, dtype=np.float32)
    acc = np.zeros(rows.shape[1:], dtype=np.float32)
    for v in range(rows.shape[0]):
        acc = acc + rows[v]
    return acc


# ---- the two device layouts of the gathered rows (view_grads.hip's header) ----
def pack_flat(gathered_rows, campos):
    """[n_views][3 P + 4]: each view's DC rows, then its camera centre and one unused float."""
    rows = np.asarray(gathered_rows, dtype=np.float32)
    n_views, P = rows.shape[:2]
    out = np.zeros((n_views, 3 * P + 4), dtype=np.float32)
    out[:, :3 * P] = rows.reshape(n_views, 3 * P)
    out[:, 3 * P:3 * P + 3] = np.asarray(campos, dtype=np.float32)[:, :3]
    return out.reshape(-1)


def unpack_flat(flat, n_views: int, P: int):
    g = np.asarray(flat, dtype=np.float32).reshape(n_views, 3 * P + 4)
    return g[:, :3 * P].reshape(n_views, P, 3).copy(), g[:, 3 * P:3 * P + 3].copy()


def pack_chunked(gathered_rows, campos, chunk: int):
    """(gathered, campos4): the Gaussians in ranges of `chunk` (the last one shorter), range [b, e) stored at
    [3 n_views b, 3 n_views e) as [n_views][e - b][3]; the camera centres a separate [n_views, 4] array."""
    rows = np.asarray(gathered_rows, dtype=np.float32)
    n_views, P = rows.shape[:2]
    out = np.empty(3 * n_views * P, dtype=np.float32)
    for b in range(0, P, chunk):
        e = min(P, b + chunk)
        out[3 * n_views * b:3 * n_views * e] = rows[:, b:e].reshape(-1)
    cam4 = np.zeros((n_views, 4), dtype=np.float32)
    cam4[:, :3] = np.asarray(campos, dtype=np.float32)[:, :3]
    return out, cam4


def unpack_chunked(gathered, campos4, n_views: int, P: int, chunk: int):
    g = np.asarray(gathered, dtype=np.float32)
    rows = np.empty((n_views, P, 3), dtype=np.float32)
    for b in range(0, P, chunk):
        e = min(P, b + chunk)
        rows[:, b:e] = g[3 * n_views * b:3 * n_views * e].reshape(n_views, e - b, 3)
    return rows, np.asarray(campos4, dtype=np.float32)[:, :3].copy()


# ---- the inputs of the GPU tests (tests/test_gpu_viewgrads.py) and of the tolerance sizing ----
def make_inputs(P: int, n_views: int, SGM: int, seed: int = 0, sharpness=None, zero_fraction: float = 0.2):
    """float32 inputs: means in a unit box, camera centres 2-6 units away, DC rows normal(0, 1) with about
    `zero_fraction` of the (view, Gaussian) rows exactly zero (a Gaussian culled or clamped in that view),
    un-normalised SG axes with |a| in [0.5, 1.5], sharpness in [0.5, 30] (or all `sharpness`)."""
    r = np.random.default_rng(seed)
    means = r.uniform(-0.5, 0.5, (P, 3))
    cdir = r.normal(size=(n_views, 3))
    campos = cdir / np.linalg.norm(cdir, axis=1, keepdims=True) * r.uniform(2.0, 6.0, (n_views, 1))
    rows = r.normal(size=(n_views, P, 3))
    rows[r.uniform(size=(n_views, P)) < zero_fraction] = 0.0
    adir = r.normal(size=(P, SGM, 3))
    axis = adir / np.linalg.norm(adir, axis=2, keepdims=True) * r.uniform(0.5, 1.5, (P, SGM, 1))
    lam = r.uniform(0.5, 30.0, (P, SGM)) if sharpness is None else np.full((P, SGM), float(sharpness))
    color = r.normal(0.0, 0.5, (P, SGM, 3))
    f = np.float32
    return {"means3D": means.astype(f), "campos": campos.astype(f), "rows": rows.astype(f),
            "sg_axis": axis.astype(f), "sg_sharpness": lam.astype(f), "sg_color": color.astype(f)}


SH_CASES = ((0, 1), (0, 16), (1, 4), (2, 9), (3, 16), (3, 17), (1, 16))  # (sh_degree, SHM)
SG_CASES = ((0, 0), (0, 3), (3, 3), (3, 7), (7, 7), (7, 9))  # (sg_degree, SGM)
P_EDGES = (1, 255, 256, 257, 1025)
VIEW_COUNTS = (1, 2, 8, 16)
CHUNK_CASES = ((513, 256), (512, 256), (257, 256), (100, 256), (1000, 1), (1000, 7), (1000, 999), (1000, 1000),
               (1000, 1001))  # (P, chunk)


def _families():
    """name -> dict(P, n_views, sh_degree, SHM, sg_degree, SGM, seed, sharpness): every input family of the GPU
    tests that is compared with the float64 reference."""
    f = {}

    def add(name, P, n_views, sh, sg, seed, sharpness=None):
        f[name] = dict(P=P, n_views=n_views, sh_degree=sh[0], SHM=sh[1], sg_degree=sg[0], SGM=sg[1], seed=seed,
                       sharpness=sharpness)
    for i, sh in enumerate(SH_CASES):
        for j, sg in enumerate(SG_CASES):
            add(f"deg_sh{sh[0]}_{sh[1]}_sg{sg[0]}_{sg[1]}", 333, 3, sh, sg, 100 + 10 * i + j)
    for P in P_EDGES:
        add(f"P{P}", P, 3, (3, 16), (7, 7), 200 + P)
    for n in VIEW_COUNTS:
        add(f"views{n}", 300, n, (3, 16), (7, 7), 300 + n)
    add("views16_sharp", 300, 16, (3, 16), (7, 7), 316, sharpness=30.0)
    add("views_swapped", 300, 3, (3, 16), (7, 7), 330)
    for P, chunk in CHUNK_CASES:
        add(f"chunk_P{P}_{chunk}", P, 3, (3, 16), (7, 7), 400 + P + chunk)
    for SHM in (2, 4, 16, 17):
        add(f"split_{SHM}", 300, 3, ({2: 0, 4: 1, 16: 3, 17: 3}[SHM], SHM), (3, 7), 500 + SHM)
    add("misaligned", 300, 3, (3, 16), (3, 7), 600)
    add("isolation", 300, 3, (3, 16), (7, 7), 700)
    return f


FAMILIES = _families()


def family_inputs(name: str):
    """(family, inputs) of FAMILIES[name]."""
    fam = FAMILIES[name]
    return fam, make_inputs(fam["P"], fam["n_views"], fam["SGM"], fam["seed"], fam["sharpness"])


def family_rebuild(name: str, dtype=np.float64, inp=None):
    fam, made = family_inputs(name)
    inp = inp or made
    return rebuild(inp["rows"], inp["campos"], inp["means3D"], fam["sh_degree"], fam["SHM"], fam["sg_degree"],
                   fam["SGM"], inp["sg_axis"], inp["sg_sharpness"], inp["sg_color"], dtype=dtype)
