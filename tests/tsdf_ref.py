"""A numpy restatement of the TSDF contract of DESIGN §6h (csrc/tsdf.hip,
gsr_tsdf.py): touch, integrate and marching cubes, written for clarity and
small sizes.  float64 by default; `dtype=np.float32` runs the same expressions
in float32.  Alongside its results it reports how close every decision came to
flipping (the ambiguity margins), so a test can leave out what float32 rounding
may legitimately decide the other way.

The marching-cubes table is the generator's (tools/gen_mc_table.py), imported,
not the committed header: tests/test_tsdf.py checks that the two agree.
"""
from __future__ import annotations

import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import gen_mc_table as G  # noqa: E402

KEY_BIAS = 1 << 20
MC_ROWS, MC_WIDTH = G.build_table()


def pack_keys(coords):
    c = np.asarray(coords, dtype=np.int64).reshape(-1, 3) + KEY_BIAS
    return c[:, 0] << 42 | c[:, 1] << 21 | c[:, 2]


def _cam(intrinsic, extrinsic, dtype):
    k = np.asarray(intrinsic, dtype=np.float64)
    if k.shape == (3, 3):
        k = np.array([k[0, 0], k[1, 1], k[0, 2], k[1, 2]])
    # the device receives float32 parameters: both modes start from those values
    k = k.astype(np.float32).astype(dtype)
    e = np.asarray(extrinsic, dtype=np.float64).astype(np.float32).astype(dtype)
    return k, e[:3, :3], e[:3, 3]


def touch(depth, intrinsic, extrinsic, voxel_size, R=16, depth_scale=1.0, depth_max=8.0, trunc_voxel_multiplier=8.0,
          dtype=np.float64):
    """-> dict: coords [n,3] int64 unique blocks ascending by key; blocks [M,4,3] the block of
    every sample of the M valid lattice pixels; margin [M,4] the distance of the sample from
    the nearest block boundary over block_size (the smallest over the axes); pixels [M,2] (x, y)."""
    f = dtype
    depth = np.asarray(depth, dtype=np.float32)
    H, W = depth.shape
    (fx, fy, cx, cy), Rm, t = _cam(intrinsic, extrinsic, f)
    trunc = f(f(voxel_size) * f(trunc_voxel_multiplier))
    block_size = f(f(voxel_size) * f(R))
    ys, xs = np.meshgrid(np.arange(0, H, 4), np.arange(0, W, 4), indexing="ij")
    xs, ys = xs.reshape(-1), ys.reshape(-1)
    with np.errstate(invalid="ignore"):
        d = depth[ys, xs].astype(f) / f(depth_scale)
        ok = (d > 0) & (d < f(depth_max))
    xs, ys, d = xs[ok], ys[ok], d[ok]
    o = -(Rm[0] * t[0] + Rm[1] * t[1] + Rm[2] * t[2])  # -R^T t
    px, py = (xs.astype(f) - cx) / fx, (ys.astype(f) - cy) / fy
    dirs = Rm[0][None] * px[:, None] + Rm[1][None] * py[:, None] + Rm[2][None]  # R^T (px, py, 1)
    t_min = np.maximum(d - trunc, f(0))
    t_max = np.minimum(d + trunc, f(depth_max))
    step = (t_max - t_min) / f(3)
    ts = t_min[:, None] + np.arange(4, dtype=f)[None] * step[:, None]
    q = (o[None, None] + ts[:, :, None] * dirs[:, None, :]) / block_size
    blocks = np.floor(q).astype(np.int64)
    if blocks.size and (blocks.min() < -KEY_BIAS or blocks.max() >= KEY_BIAS):
        raise ValueError("a sample falls in a block beyond +-2^20")
    margin = np.abs(q - np.rint(q)).min(axis=2).astype(np.float64) if blocks.size else np.zeros((0, 4))
    flat = blocks.reshape(-1, 3)
    keys = np.unique(pack_keys(flat)) if flat.size else np.zeros(0, np.int64)
    coords = np.stack([(keys >> 42) - KEY_BIAS, (keys >> 21 & 0x1fffff) - KEY_BIAS, (keys & 0x1fffff) - KEY_BIAS], 1)
    return {"coords": coords.reshape(-1, 3), "blocks": blocks, "margin": margin, "pixels": np.stack([xs, ys], 1)}


class Grid:
    """Blocks in insertion order (new blocks of one call in ascending key order), R^3 voxels per
    block linear in (z R + y) R + x, tsdf / weight / colour starting at zero."""

    def __init__(self, voxel_size, R=16, with_color=True, dtype=np.float64):
        self.voxel_size, self.R, self.with_color, self.dtype = voxel_size, R, with_color, dtype
        N = R ** 3
        self.coords = np.zeros((0, 3), np.int64)
        self.slot = {}
        self.tsdf = np.zeros((0, N), dtype)
        self.weight = np.zeros((0, N), dtype)
        self.color = np.zeros((0, N, 3), dtype) if with_color else None

    def add(self, coords):
        coords = np.asarray(coords, np.int64).reshape(-1, 3)
        keys = pack_keys(coords)
        fresh = [i for i in np.argsort(keys, kind="stable") if int(keys[i]) not in self.slot]
        for i in fresh:
            if int(keys[i]) in self.slot:
                continue
            self.slot[int(keys[i])] = self.coords.shape[0]
            self.coords = np.concatenate([self.coords, coords[i:i + 1]])
        grow = self.coords.shape[0] - self.tsdf.shape[0]
        if grow:
            N = self.R ** 3
            self.tsdf = np.concatenate([self.tsdf, np.zeros((grow, N), self.dtype)])
            self.weight = np.concatenate([self.weight, np.zeros((grow, N), self.dtype)])
            if self.with_color:
                self.color = np.concatenate([self.color, np.zeros((grow, N, 3), self.dtype)])
        return np.array([self.slot[int(k)] for k in keys], np.int64)

    def integrate(self, block_coords, depth, color, intrinsic, extrinsic, depth_scale=1.0, depth_max=8.0,
                  trunc_voxel_multiplier=8.0):
        """One view into the listed blocks.  -> dict over those blocks' voxels [n, R^3]:
        updated (bool) and margin: the smallest of the distance of u or v from a rounding tie
        (pixels) and of sdf from -trunc, z_c from 0 and d from depth_max (over trunc), each
        counted only where the voxel got as far as that test."""
        f, R = self.dtype, self.R
        depth = np.asarray(depth, dtype=np.float32)
        H, W = depth.shape
        (fx, fy, cx, cy), Rm, t = _cam(intrinsic, extrinsic, f)
        vs = f(self.voxel_size)
        trunc = f(vs * f(trunc_voxel_multiplier))
        block_coords = np.asarray(block_coords, np.int64).reshape(-1, 3)
        slots = self.add(block_coords)
        i = np.arange(R ** 3)
        local = np.stack([i % R, i // R % R, i // (R * R)], 1)
        p = (block_coords[:, None, :] * R + local[None]).astype(f) * vs  # [n, N, 3]
        cam = [Rm[r, 0] * p[..., 0] + Rm[r, 1] * p[..., 1] + Rm[r, 2] * p[..., 2] + t[r] for r in range(3)]
        xc, yc, zc = cam
        margin = np.abs(zc).astype(np.float64) / float(trunc)
        live = zc > 0
        with np.errstate(divide="ignore", invalid="ignore"):
            ur, vr = fx * xc / zc + cx, fy * yc / zc + cy
        ur, vr = np.where(live, ur, 0), np.where(live, vr, 0)
        tie = np.minimum(np.abs(ur - np.floor(ur) - 0.5), np.abs(vr - np.floor(vr) - 0.5)).astype(np.float64)
        margin = np.where(live, np.minimum(margin, tie), margin)
        u, v = np.rint(ur), np.rint(vr)
        live &= (u >= 0) & (u < W) & (v >= 0) & (v < H)
        ui, vi = np.where(live, u, 0).astype(np.int64), np.where(live, v, 0).astype(np.int64)
        with np.errstate(invalid="ignore"):
            d = depth[vi, ui].astype(f) / f(depth_scale)
            has = live & (d > 0)
            margin = np.where(has, np.minimum(margin, np.abs(d - f(depth_max)).astype(np.float64) / float(trunc)),
                              margin)
            live = has & ~(d > f(depth_max))
            sdf = np.where(live, d - zc, 0)
        margin = np.where(live, np.minimum(margin, np.abs(sdf + trunc).astype(np.float64) / float(trunc)), margin)
        live &= ~(sdf < -trunc)
        s = np.minimum(sdf, trunc) / trunc
        w = self.weight[slots]
        w1 = w + f(1)
        self.tsdf[slots] = np.where(live, (w * self.tsdf[slots] + s) / w1, self.tsdf[slots])
        if self.with_color:
            img = np.asarray(color, dtype=np.float32).astype(f)[vi, ui]
            self.color[slots] = np.where(live[..., None], (w[..., None] * self.color[slots] + img) / w1[..., None],
                                         self.color[slots])
        self.weight[slots] = np.where(live, w1, w)
        return {"updated": live, "margin": margin, "slots": slots}


def extract(block_coords, tsdf, weight, color=None, voxel_size=0.002, R=16, weight_threshold=3.0):
    """Marching cubes over given voxel data (any float dtype: signs and thresholds are decided on
    the values as given, positions computed in float64).  -> (vertices [V,3] float64, faces [F,3]
    int64, colors [V,3] float64 or None, n_sign_change_edges)."""
    block_coords = np.asarray(block_coords, np.int64).reshape(-1, 3)
    n = block_coords.shape[0]
    empty = (np.zeros((0, 3)), np.zeros((0, 3), np.int64), None if color is None else np.zeros((0, 3)), 0)
    if n == 0:
        return empty
    lo = block_coords.min(0)
    span = (block_coords.max(0) - lo + 1) * R + 1
    D = np.zeros(span)
    U = np.zeros(span, bool)
    Cc = np.zeros(tuple(span) + (3,)) if color is not None else None
    for b in range(n):
        x0, y0, z0 = (block_coords[b] - lo) * R
        blk = np.asarray(tsdf[b], np.float64).reshape(R, R, R).transpose(2, 1, 0)  # [x, y, z]
        D[x0:x0 + R, y0:y0 + R, z0:z0 + R] = blk
        U[x0:x0 + R, y0:y0 + R, z0:z0 + R] = (np.asarray(weight[b]).reshape(R, R, R).transpose(2, 1, 0)
                                              > weight_threshold)
        if color is not None:
            Cc[x0:x0 + R, y0:y0 + R, z0:z0 + R] = np.asarray(color[b], np.float64).reshape(R, R, R, 3).transpose(
                2, 1, 0, 3)
    X, Y, Z = span - 1
    corner = lambda A, c: A[(c & 1):(c & 1) + X, (c >> 1 & 1):(c >> 1 & 1) + Y, (c >> 2 & 1):(c >> 2 & 1) + Z]  # noqa: E731
    emitted = np.ones((X, Y, Z), bool)
    case = np.zeros((X, Y, Z), np.int64)
    for c in range(8):
        emitted &= corner(U, c)
        case |= (corner(D, c) < 0).astype(np.int64) << c
    case = np.where(emitted, case, 0)
    # the vertices: bit `axis` of the owner voxel, set by the crossed edges of emitted cubes
    M = np.zeros(tuple(span) + (3,), bool)
    for e in range(12):
        a, b = G.edge_corners(e)
        crossed = ((case >> a & 1) != (case >> b & 1))
        corner(M[..., e // 4], a)[...] |= crossed
    own = np.argwhere(M)  # (x, y, z, axis)
    if own.shape[0] == 0:
        return empty
    gp = own[:, :3] + lo * R  # global voxel coordinates
    keys = pack_keys(gp // R)
    lp = gp % R
    lin = (lp[:, 2] * R + lp[:, 1]) * R + lp[:, 0]
    order = np.lexsort((own[:, 3], lin, keys))
    own, gp = own[order], gp[order]
    vid = -np.ones(tuple(span) + (3,), np.int64)
    vid[own[:, 0], own[:, 1], own[:, 2], own[:, 3]] = np.arange(own.shape[0])
    other = own[:, :3].copy()
    other[np.arange(own.shape[0]), own[:, 3]] += 1
    ta, tb = D[tuple(own[:, :3].T)], D[tuple(other.T)]
    t = ta / (ta - tb)
    pos = gp.astype(np.float64)
    pos[np.arange(own.shape[0]), own[:, 3]] += t
    vertices = pos * voxel_size
    colors = None
    if color is not None:
        ca, cb = Cc[tuple(own[:, :3].T)], Cc[tuple(other.T)]
        colors = ca + t[:, None] * (cb - ca)
    # the triangles, by (block, voxel, table order)
    cubes = np.argwhere(case > 0)
    cubes = cubes[[len(MC_ROWS[case[tuple(c)]]) > 0 for c in cubes]] if cubes.size else cubes
    gq = cubes + lo * R
    lq = gq % R
    corder = np.lexsort(((lq[:, 2] * R + lq[:, 1]) * R + lq[:, 0], pack_keys(gq // R)))
    faces = []
    for x, y, z in cubes[corder]:
        row = MC_ROWS[case[x, y, z]]
        ids = []
        for e in row:
            a, _ = G.edge_corners(e)
            ids.append(vid[x + (a & 1), y + (a >> 1 & 1), z + (a >> 2 & 1), e // 4])
        faces += [ids[k:k + 3] for k in range(0, len(ids), 3)]
    faces = np.asarray(faces, np.int64).reshape(-1, 3)
    return vertices, faces, colors, int(own.shape[0])


# ---- mesh properties -------------------------------------------------------------------------------

def directed_edges(faces):
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    return np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]])


def is_closed_oriented(faces):
    """Every undirected edge is used by exactly two triangles, once in each direction."""
    e = directed_edges(faces)
    if e.shape[0] == 0:
        return False
    fwd = {}
    for a, b in e.tolist():
        if (a, b) in fwd:
            return False
        fwd[(a, b)] = 1
    return all((b, a) in fwd for a, b in fwd)


def boundary_edges(faces):
    """The directed edges without their reverse."""
    s = set(map(tuple, directed_edges(faces).tolist()))
    return [(a, b) for a, b in s if (b, a) not in s]


def euler(faces):
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    e = np.sort(directed_edges(f), axis=1)
    return int(np.unique(f).size - np.unique(e, axis=0).shape[0] + f.shape[0])


def signed_volume(vertices, faces):
    v = np.asarray(vertices, np.float64)
    f = np.asarray(faces, np.int64)
    a, b, c = v[f[:, 0]], v[f[:, 1]], v[f[:, 2]]
    return float(np.einsum("ij,ij->i", a, np.cross(b, c)).sum() / 6.0)
