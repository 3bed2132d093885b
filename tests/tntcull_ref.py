"""A numpy restatement of the TnT mesh-culling contract of DESIGN §6j (csrc/meshraster.hip,
gsr_tnt.render_mesh_depth / mesh_view_votes / cull_mesh), the yardstick of
tests/test_gpu_tntcull.py; tests/test_tntcull.py pins it on the CPU.

depth_ref, votes_ref and cull_ref are float32 in the contract's operation order:
every array below is float32 and every scalar an np.float32, so each elementwise
numpy expression rounds once per operation, as the device's uncontracted
arithmetic does, and the results are the device's bits.  depth_f64 is a
Moller-Trumbore ray cast in float64 that shares nothing with them but the camera.
"""
from __future__ import annotations

import numpy as np

F32 = np.float32
INF = F32(np.inf)


def _f(x):
    return np.asarray(x, dtype=np.float32)


def w2c_rows(w2c):
    """A 4x4 or 3x4 world -> camera matrix (any float type) as the float32 3x4 the device receives."""
    return np.ascontiguousarray(np.asarray(w2c, dtype=np.float64)[:3, :].astype(np.float32))


def cam_points(vertices, m):
    """p = ((m0 x + m1 y) + m2 z) + m3 per row of the float32 3x4."""
    v = _f(vertices).reshape(-1, 3)
    x, y, z = v[:, 0], v[:, 1], v[:, 2]
    return np.stack([((m[r, 0] * x + m[r, 1] * y) + m[r, 2] * z) + m[r, 3] for r in range(3)], 1)


def _cross(a, b):
    return np.stack([a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1], a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2],
                     a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]], 1)


def _affine(n, fx, fy, cx, cy):
    A = n[:, 0] / fx
    B = n[:, 1] / fy
    return A, B, n[:, 2] - (A * cx + B * cy)


def setup_ref(vertices, faces, w2c, H, W, fx, fy, cx, cy, znear, zfar):
    """The per-triangle set-up of the raster: corners sorted by vertex id, edge and plane coefficients, the
    pixel bound.  -> dict of arrays over the triangles; `ok` marks those that can cover a pixel."""
    fx, fy, cx, cy, znear, zfar = (F32(t) for t in (fx, fy, cx, cy, znear, zfar))
    f = np.sort(np.asarray(faces, dtype=np.int64).reshape(-1, 3), axis=1)
    V = np.asarray(vertices).reshape(-1, 3).shape[0]
    if f.size and (f.min() < 0 or f.max() >= V):
        raise ValueError("a face names a vertex outside [0, V)")
    pc = cam_points(vertices, w2c_rows(w2c))
    with np.errstate(all="ignore"):
        p = [pc[f[:, k]] for k in range(3)]
        N = _cross(p[1] - p[0], p[2] - p[0])
        D = (p[0][:, 0] * N[:, 0] + p[0][:, 1] * N[:, 1]) + p[0][:, 2] * N[:, 2]
        ok = (np.abs(D) > 0) & (np.abs(D) < INF)
        z = np.stack([q[:, 2] for q in p], 1)
        zmin = np.fmin(np.fmin(z[:, 0], z[:, 1]), z[:, 2])
        zmax = np.fmax(np.fmax(z[:, 0], z[:, 1]), z[:, 2])
        ok &= (zmax >= znear) & (zmin <= zfar)
        lo = [np.full(f.shape[0], INF), np.full(f.shape[0], INF)]
        hi = [np.full(f.shape[0], -INF), np.full(f.shape[0], -INF)]

        def grow(mask, u, v):
            for a, val in ((0, u), (1, v)):
                lo[a] = np.where(mask, np.fmin(lo[a], val), lo[a])
                hi[a] = np.where(mask, np.fmax(hi[a], val), hi[a])

        for k in range(3):
            grow(p[k][:, 2] >= znear, fx * (p[k][:, 0] / p[k][:, 2]) + cx, fy * (p[k][:, 1] / p[k][:, 2]) + cy)
        for k in range(3):
            k2 = (k + 1) % 3
            in1, in2 = p[k][:, 2] >= znear, p[k2][:, 2] >= znear
            q0 = np.where(in1[:, None], p[k2], p[k])
            q1 = np.where(in1[:, None], p[k], p[k2])
            w = (znear - q0[:, 2]) / (q1[:, 2] - q0[:, 2])
            xx = q0[:, 0] + w * (q1[:, 0] - q0[:, 0])
            yy = q0[:, 1] + w * (q1[:, 1] - q0[:, 1])
            grow(in1 != in2, fx * (xx / znear) + cx, fy * (yy / znear) + cy)
        fj0 = np.fmax(np.ceil(lo[0] - F32(1)), F32(0))
        fj1 = np.fmin(np.floor(hi[0]), F32(W - 1))
        fi0 = np.fmax(np.ceil(lo[1] - F32(1)), F32(0))
        fi1 = np.fmin(np.floor(hi[1]), F32(H - 1))
        ok &= (fj0 <= fj1) & (fi0 <= fi1)
        box = [np.where(ok, t, F32(0)).astype(np.int64) for t in (fj0, fj1, fi0, fi1)]
        E = [_affine(_cross(p[a], p[b]), fx, fy, cx, cy) for a, b in ((1, 2), (2, 0), (0, 1))]
        Aw, Bw, Cw = _affine(N, fx, fy, cx, cy)
    return dict(ok=ok, E=E, Aw=Aw, Bw=Bw, Cw=Cw, D=D, j0=box[0], j1=box[1], i0=box[2], i1=box[3],
                znear=znear, zfar=zfar)


def _fragments(s, t, i, j):
    """Triangles t at pixels (i, j) -> (mask of the covered ones in the slab, z)."""
    u, v = _f(j) + F32(0.5), _f(i) + F32(0.5)
    with np.errstate(all="ignore"):
        e = [(A[t] * u + B[t] * v) + C[t] for A, B, C in s["E"]]
        inside = ((e[0] >= 0) & (e[1] >= 0) & (e[2] >= 0)) | ((e[0] <= 0) & (e[1] <= 0) & (e[2] <= 0))
        z = s["D"][t] / ((s["Aw"][t] * u + s["Bw"][t] * v) + s["Cw"][t])
        inside &= (z >= s["znear"]) & (z <= s["zfar"])
    return inside, z


def bound_sizes(vertices, faces, w2c, H, W, fx, fy, cx, cy, znear=0.01, zfar=20.0):
    """(width, height) in pixels of every triangle's bound, (0, 0) where it can cover nothing."""
    s = setup_ref(vertices, faces, w2c, H, W, fx, fy, cx, cy, znear, zfar)
    return np.where(s["ok"], s["j1"] - s["j0"] + 1, 0), np.where(s["ok"], s["i1"] - s["i0"] + 1, 0)


def depth_ref(vertices, faces, w2c, H, W, fx, fy, cx, cy, znear=0.01, zfar=20.0, return_winner=False):
    """The contract's depth map [H,W] float32 (0 where empty); with return_winner also the lowest id of the
    triangles that reach the pixel's depth (-1 where empty)."""
    s = setup_ref(vertices, faces, w2c, H, W, fx, fy, cx, cy, znear, zfar)
    nF = s["ok"].shape[0]
    w, h = s["j1"] - s["j0"] + 1, s["i1"] - s["i0"] + 1
    n = np.where(s["ok"], w * h, 0)
    frags = []
    small = np.nonzero((n > 0) & (n <= 256))[0]
    for k in range(int(n[small].max()) if small.size else 0):
        t = small[n[small] > k]
        i, j = s["i0"][t] + k // w[t], s["j0"][t] + k % w[t]
        m, z = _fragments(s, t, i, j)
        frags.append((t[m], (i * W + j)[m], z[m]))
    for t in np.nonzero(n > 256)[0]:
        i, j = np.meshgrid(np.arange(s["i0"][t], s["i1"][t] + 1), np.arange(s["j0"][t], s["j1"][t] + 1),
                           indexing="ij")
        i, j = i.reshape(-1), j.reshape(-1)
        tt = np.full(i.shape, t)
        m, z = _fragments(s, tt, i, j)
        frags.append((tt[m], (i * W + j)[m], z[m]))
    depth = np.full(H * W, INF, dtype=np.float32)
    winner = np.full(H * W, nF, dtype=np.int64)
    if frags:
        t, pix, z = (np.concatenate(a) for a in zip(*frags))
        np.minimum.at(depth, pix, z)
        best = z == depth[pix]
        np.minimum.at(winner, pix[best], t[best])
    winner[depth == INF] = -1
    depth[depth == INF] = 0
    depth = depth.reshape(H, W)
    return (depth, winner.reshape(H, W)) if return_winner else depth


def votes_view_ref(vertices, depth, w2c, H, W, fx, fy, cx, cy, eps=0.005):
    """One view's vote per vertex (bool [V]) against its depth map, with the margins the CPU test reads:
    -> (vote, dict u, v, z, d, in_frustum)."""
    fx, fy, cx, cy, eps = (F32(t) for t in (fx, fy, cx, cy, eps))
    p = cam_points(vertices, w2c_rows(w2c))
    d = np.zeros(p.shape[0], dtype=np.float32)
    with np.errstate(all="ignore"):
        z = p[:, 2] + F32(1e-8)
        u = (fx * p[:, 0] + cx * p[:, 2]) / z
        v = (fy * p[:, 1] + cy * p[:, 2]) / z
        inside = (u >= 0) & (u <= F32(W - 1)) & (v >= 0) & (v <= F32(H - 1)) & (z > 0)
        k = np.nonzero(inside)[0]
        uu, vv = u[k], v[k]
        fx0, fy0 = np.floor(uu), np.floor(vv)
        x0, y0 = fx0.astype(np.int64), fy0.astype(np.int64)
        x1, y1 = np.minimum(x0 + 1, W - 1), np.minimum(y0 + 1, H - 1)
        tx, ty, sx, sy = uu - fx0, vv - fy0, (fx0 + F32(1)) - uu, (fy0 + F32(1)) - vv
        dm = _f(depth).reshape(H, W)
        d[k] = ((dm[y0, x0] * (sx * sy) + dm[y0, x1] * (tx * sy)) + dm[y1, x0] * (sx * ty)) + dm[y1, x1] * (tx * ty)
        front = np.where(d > 0, z < d + eps, True)
    return inside & front, dict(u=u, v=v, z=z, d=d, in_frustum=inside)


def votes_ref(vertices, faces, w2cs, H, W, fx, fy, cx, cy, znear=0.01, zfar=20.0, eps=0.005):
    """counts [V] int32 over the views, each against depth_ref of that view."""
    counts = np.zeros(np.asarray(vertices).reshape(-1, 3).shape[0], dtype=np.int32)
    for m in np.asarray(w2cs, dtype=np.float64).reshape(-1, *np.asarray(w2cs).shape[-2:]):
        depth = depth_ref(vertices, faces, m, H, W, fx, fy, cx, cy, znear, zfar)
        counts += votes_view_ref(vertices, depth, m, H, W, fx, fy, cx, cy, eps)[0].astype(np.int32)
    return counts


def compact_ref(vertices, faces, keep_v):
    """Faces whose three corners are kept, the vertices they name, in the surviving order, faces remapped."""
    v, f = np.asarray(vertices).reshape(-1, 3), np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    f = f[keep_v[f[:, 0]] & keep_v[f[:, 1]] & keep_v[f[:, 2]]]
    used = np.zeros(v.shape[0], dtype=bool)
    used[f.reshape(-1)] = True
    return v[used], (np.cumsum(used) - 1)[f]


def cull_ref(vertices, faces, c2ws, H, W, fx, fy, cx, cy, far=20.0, min_views=20, eps=0.005):
    c = np.asarray(c2ws, dtype=np.float64)
    full = np.tile(np.eye(4), (c.shape[0], 1, 1))
    full[:, :c.shape[1], :] = c
    counts = votes_ref(vertices, faces, np.linalg.inv(full) if c.shape[0] else full, H, W, fx, fy, cx, cy, 0.01,
                       far, eps)
    return compact_ref(vertices, faces, counts >= min_views)


# ---- float64, independent ---------------------------------------------------------------------------------------

def _cam64(vertices, w2c):
    m = w2c_rows(w2c).astype(np.float64)
    return np.asarray(vertices, dtype=np.float32).reshape(-1, 3).astype(np.float64) @ m[:, :3].T + m[:, 3]


def depth_f64(vertices, faces, w2c, H, W, fx, fy, cx, cy, znear=0.01, zfar=20.0):
    """Moller-Trumbore from the camera centre through every pixel centre, float64 -> (depth [H,W] float64, 0
    where empty; winner [H,W], -1 where empty)."""
    pc = _cam64(vertices, w2c)
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    p0, e1, e2 = pc[f[:, 0]], pc[f[:, 1]] - pc[f[:, 0]], pc[f[:, 2]] - pc[f[:, 0]]
    depth, winner = np.zeros((H, W)), np.full((H, W), -1, dtype=np.int64)
    if f.shape[0] == 0:
        return depth, winner
    q = np.cross(-p0, e1)
    dx = (np.arange(W) + 0.5 - cx) / fx
    for i in range(H):
        d = np.stack([dx, np.full(W, (i + 0.5 - cy) / fy), np.ones(W)], 1)  # [W,3]
        with np.errstate(all="ignore"):
            hvec = np.cross(d[:, None, :], e2[None, :, :])  # [W,F,3]
            a = (hvec * e1[None]).sum(-1)
            inv = 1.0 / a
            bu = inv * (hvec * (-p0)[None]).sum(-1)
            bv = inv * (d[:, None, :] * q[None]).sum(-1)
            t = inv * (e2 * q).sum(-1)[None]
            hit = (a != 0) & (bu >= 0) & (bv >= 0) & (bu + bv <= 1) & (t >= znear) & (t <= zfar)
        t = np.where(hit, t, np.inf)
        k = t.argmin(1)
        best = t[np.arange(W), k]
        depth[i] = np.where(np.isfinite(best), best, 0.0)
        winner[i] = np.where(np.isfinite(best), k, -1)
    return depth, winner


def edge_distance_px(vertices, faces, w2c, winner, fx, fy, cx, cy):
    """For every pixel the distance in pixels from its centre to the nearest edge line of triangle
    winner[i, j] (float64, homogeneous edge functions); +inf where winner is -1."""
    pc = _cam64(vertices, w2c)
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    H, W = winner.shape
    out = np.full((H, W), np.inf)
    ii, jj = np.nonzero(winner >= 0)
    t = winner[ii, jj]
    u, v = jj + 0.5, ii + 0.5
    for a, b in ((1, 2), (2, 0), (0, 1)):
        n = np.cross(pc[f[t, a]], pc[f[t, b]])
        A, B = n[:, 0] / fx, n[:, 1] / fy
        C = n[:, 2] - (A * cx + B * cy)
        with np.errstate(all="ignore"):
            dist = np.abs(A * u + B * v + C) / np.sqrt(A * A + B * B)
        out[ii, jj] = np.fmin(out[ii, jj], dist)
    return out


# ---- scenes -----------------------------------------------------------------------------------------------------

def look_at(eye, target, up=(0.0, -1.0, 0.0)):
    """Camera -> world 4x4 of an OpenCV camera (x right, y down, z forward) at `eye` looking at `target`."""
    eye, target = np.asarray(eye, float), np.asarray(target, float)
    zc = target - eye
    zc /= np.linalg.norm(zc)
    xc = np.cross(-np.asarray(up, float), zc)
    if np.linalg.norm(xc) < 1e-9:
        xc = np.cross(np.array([1.0, 0.0, 0.0]), zc)
    xc /= np.linalg.norm(xc)
    yc = np.cross(zc, xc)
    c2w = np.eye(4)
    c2w[:3, 0], c2w[:3, 1], c2w[:3, 2], c2w[:3, 3] = xc, yc, zc, eye
    return c2w


def orbit(n, radius, height, target=(0.0, 0.0, 0.0)):
    return np.stack([look_at((radius * np.cos(2 * np.pi * k / n), height, radius * np.sin(2 * np.pi * k / n)), target)
                     for k in range(n)])


def icosphere(level, radius=1.0, centre=(0.0, 0.0, 0.0)):
    """20 * 4^level triangles, outward winding -> (vertices float32, faces int64)."""
    g = (1 + 5 ** 0.5) / 2
    v = [(-1, g, 0), (1, g, 0), (-1, -g, 0), (1, -g, 0), (0, -1, g), (0, 1, g), (0, -1, -g), (0, 1, -g),
         (g, 0, -1), (g, 0, 1), (-g, 0, -1), (-g, 0, 1)]
    v = [np.asarray(p, float) / np.linalg.norm(p) for p in v]
    f = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6),
         (7, 1, 8), (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10),
         (8, 6, 7), (9, 8, 1)]
    for _ in range(level):
        mid, nf = {}, []

        def m(a, b):
            key = (min(a, b), max(a, b))
            if key not in mid:
                p = v[a] + v[b]
                v.append(p / np.linalg.norm(p))
                mid[key] = len(v) - 1
            return mid[key]

        for a, b, c in f:
            ab, bc, ca = m(a, b), m(b, c), m(c, a)
            nf += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        f = nf
    return (np.asarray(v) * radius + np.asarray(centre, float)).astype(np.float32), np.asarray(f, dtype=np.int64)


def around(radius):
    """42 cameras on a sphere about the origin (the corners of a once-subdivided icosahedron), looking in."""
    return np.stack([look_at(radius * p.astype(float), (0.0, 0.0, 0.0)) for p in icosphere(1)[0]])


def terrain(nx, nz, seed=0):
    """A height field over [-2, 2]^2 (y down: the surface faces -y) with an overhanging slab above part of it:
    2 (nx - 1)(nz - 1) + 2 (nx // 3 - 1)(nz // 3 - 1) triangles -> (vertices float32, faces int64)."""
    rng = np.random.default_rng(seed)

    def grid(ax, az, x0, x1, z0, z1, y):
        x, z = np.meshgrid(np.linspace(x0, x1, ax), np.linspace(z0, z1, az), indexing="ij")
        v = np.stack([x, y(x, z), z], -1).reshape(-1, 3)
        k = (np.arange(ax - 1)[:, None] * az + np.arange(az - 1)[None, :]).reshape(-1)
        return v, np.concatenate([np.stack([k, k + 1, k + az], 1), np.stack([k + 1, k + az + 1, k + az], 1)])

    ph = rng.uniform(0, 6, 4)
    v0, f0 = grid(nx, nz, -2, 2, -2, 2, lambda x, z: 0.25 * np.sin(1.7 * x + ph[0]) * np.cos(1.3 * z + ph[1])
                  + 0.1 * np.sin(3.1 * x + ph[2]) * np.sin(2.9 * z + ph[3]))
    v1, f1 = grid(nx // 3, nz // 3, -0.5, 1.0, -0.8, 0.7, lambda x, z: -0.6 + 0.05 * x)
    return np.concatenate([v0, v1]).astype(np.float32), np.concatenate([f0, f1 + v0.shape[0]]).astype(np.int64)
