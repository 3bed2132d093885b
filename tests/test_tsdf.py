"""CPU tests of the TSDF yardsticks: the numpy restatement tests/tsdf_ref.py
pinned to answers known by construction (a wall, a single pixel, a sphere), and
the generated marching-cubes table over all 256 rows.  tests/test_gpu_tsdf.py
compares the HIP kernels with the restatement and shares the cases built here.
"""
from __future__ import annotations

import os
import re

import numpy as np

import tsdf_ref as T

G = T.G
VS, R8 = 0.01, 8  # voxel 0.01, blocks of 8: block_size = trunc = 0.08
IDENT = np.eye(4)


def translated(x, y, z):
    """World -> camera of a camera at (x, y, z) looking along +z."""
    e = np.eye(4)
    e[:3, 3] = [-x, -y, -z]
    return e


def single_pixel_case():
    """One valid pixel on the lattice whose ray is the camera's z axis."""
    depth = np.zeros((16, 12), np.float32)
    depth[8, 4] = 1.0
    return depth, (50.0, 50.0, 4.0, 8.0)


def wall_case():
    """A 32x24 image seeing a wall at z = 0.2 from the origin; fx = 100 makes the image cover
    |x| <= 0.03, |y| <= 0.022 there: inside block (0, 0, *) and (-1, -1, *)."""
    depth = np.full((24, 32), 0.2, np.float32)
    return depth, (100.0, 100.0, 15.5, 11.5)


def sphere_field(centre, radius, blocks, R=R8, vs=VS, weight=4.0):
    """The float32 voxel data of |p - centre| - radius over the listed blocks, truncated like a
    fused field (divided by trunc = 8 vs, clamped to [-1, 1])."""
    blocks = np.asarray(blocks, np.int64)
    i = np.arange(R ** 3)
    local = np.stack([i % R, i // R % R, i // (R * R)], 1)
    p = (blocks[:, None, :] * R + local[None]) * vs
    sdf = np.linalg.norm(p - np.asarray(centre)[None, None], axis=2) - radius
    tsdf = np.clip(sdf / (8 * vs), -1, 1).astype(np.float32)
    return blocks, tsdf, np.full(tsdf.shape, weight, np.float32)


def sphere_case():
    """Radius 0.1 around (-0.013, 0.021, 0.003): 4x4x4 blocks from (-2, -2, -2); the surface crosses
    block faces, edges and the corner at the origin, with negative coordinates on every axis."""
    blocks = np.array([(x, y, z) for x in range(-2, 2) for y in range(-2, 2) for z in range(-2, 2)])
    return sphere_field((-0.013, 0.021, 0.003), 0.1, blocks)


def torus_case():
    blocks = np.array([(x, y, z) for x in range(-3, 3) for y in range(-3, 3) for z in range(-1, 1)])
    i = np.arange(R8 ** 3)
    local = np.stack([i % R8, i // R8 % R8, i // (R8 * R8)], 1)
    p = (blocks[:, None, :] * R8 + local[None]) * VS - np.array([0.004, -0.003, 0.002])
    sdf = np.hypot(np.hypot(p[..., 0], p[..., 1]) - 0.14, p[..., 2]) - 0.045
    tsdf = np.clip(sdf / (8 * VS), -1, 1).astype(np.float32)
    return blocks, tsdf, np.full(tsdf.shape, 4.0, np.float32)


def all_cases_field():
    """All 256 sign patterns, one isolated cube each: cube c has its low corner at voxel
    (3 (c % 16), 3 (c // 16), 1) of a 48x48x8 field; only its 8 corners are usable."""
    blocks = np.array([(x, y, 0) for x in range(6) for y in range(6)])
    tsdf = np.zeros((36, R8 ** 3), np.float32)
    weight = np.zeros((36, R8 ** 3), np.float32)
    rng = np.random.default_rng(5)
    for c in range(256):
        for k in range(8):
            x, y, z = 3 * (c % 16) + (k & 1), 3 * (c // 16) + (k >> 1 & 1), 1 + (k >> 2 & 1)
            b = (x // R8) * 6 + y // R8
            lin = ((z % R8) * R8 + y % R8) * R8 + x % R8
            mag = rng.uniform(0.1, 0.9)
            tsdf[b, lin] = -mag if c >> k & 1 else mag
            weight[b, lin] = 4.0
    return blocks, tsdf, weight


# ---- the restatement, against answers known by construction ----------------------------------------

def test_touch_single_pixel():
    depth, k = single_pixel_case()
    r = T.touch(depth, k, IDENT, VS, R8)
    # t = 0.92, 0.9733, 1.0267, 1.08 along z: blocks floor(t / 0.08) = 11, 12, 12, 13
    assert r["coords"].tolist() == [[0, 0, 11], [0, 0, 12], [0, 0, 13]]
    assert r["blocks"].shape == (1, 4, 3) and r["pixels"].tolist() == [[4, 8]]
    # a camera just below zero on x and y: floor goes down, truncation would stay at 0
    r = T.touch(depth, k, translated(-0.001, -0.001, 0.0), VS, R8)
    assert r["coords"].tolist() == [[-1, -1, 11], [-1, -1, 12], [-1, -1, 13]]
    assert np.allclose(r["margin"][0], [0.0125, 0.0125, 0.0125, 0.0125])
    # off the lattice, or out of range: nothing
    for bad in (0.0, -1.0, 8.0, 9.0, np.nan, np.inf):
        d = np.zeros_like(depth)
        d[8, 4] = bad
        assert T.touch(d, k, IDENT, VS, R8)["coords"].shape == (0, 3)
    d = np.zeros_like(depth)
    d[8, 5] = d[9, 4] = d[7, 7] = 1.0
    assert T.touch(d, k, IDENT, VS, R8)["coords"].shape == (0, 3)


def test_touch_clamps():
    depth, k = single_pixel_case()
    d = depth * 0.03  # t_min = max(0.03 - 0.08, 0) = 0, t_max = 0.11: t = 0, .0367, .0733, .11
    # from z = 0.004 the samples sit at .004, .0407, .0773, .114; an unclamped t_min = -0.05 would reach block -1
    assert T.touch(d, k, translated(0, 0, 0.004), VS, R8)["coords"].tolist() == [[0, 0, 0], [0, 0, 1]]
    d = depth * 7.98  # t_max = min(8.06, 8) = 8: t = 7.9, 7.9333, 7.9667, 8
    # from z = -0.004 they end at 7.996 (block 99); an unclamped t_max = 8.06 would reach block 100
    assert T.touch(d, k, translated(0, 0, -0.004), VS, R8)["coords"][:, 2].tolist() == [98, 99]
    assert T.touch(d, k, translated(0, 0, 0.004), VS, R8)["coords"][:, 2].tolist() == [98, 99, 100]


def test_integrate_wall():
    depth, k = wall_case()
    for dtype in (np.float64, np.float32):
        g = T.Grid(VS, R8, with_color=True, dtype=dtype)
        color = np.full((24, 32, 3), 0.25, np.float32)
        blocks = np.array([[0, 0, 2], [0, 0, 1], [0, 0, 3]])
        out = g.integrate(blocks, depth, color, k, IDENT)
        assert g.coords.tolist() == [[0, 0, 1], [0, 0, 2], [0, 0, 3]]  # ascending key order
        i = np.arange(R8 ** 3)
        x, y, z = i % R8, i // R8 % R8, i // (R8 * R8)
        for b, slot in ((1, 0), (2, 1), (3, 2)):
            wz = (b * R8 + z) * VS
            u, v = np.rint(100 * x * VS / wz + 15.5), np.rint(100 * y * VS / wz + 11.5)
            seen = (u < 32) & (v < 24) & (0.2 - wz >= -0.08 - 1e-12)
            assert np.array_equal(g.weight[slot] == 1, seen) and np.all(g.weight[slot][~seen] == 0)
            want = np.minimum(0.2 - wz, 0.08) / 0.08
            assert np.allclose(g.tsdf[slot][seen], want[seen], atol=1e-5)
            assert np.all(g.tsdf[slot][~seen] == 0)
            assert np.allclose(g.color[slot][seen], 0.25) and np.all(g.color[slot][~seen] == 0)
        assert out["updated"].shape == (3, R8 ** 3)
        # the running mean over views at other depths, in call order
        g.integrate(blocks[:1], depth * 1.1, color * 2, k, IDENT)
        g.integrate(blocks[:1], depth * 0.9, color * 3, k, IDENT)
        lin = (2 * R8 + 1) * R8 + 1  # voxel (1, 1, 2) of block (0, 0, 2): z = 0.18
        assert g.weight[1][lin] == 3
        assert np.isclose(g.tsdf[1][lin], (0.02 + 0.04 + 0.0) / 0.08 / 3, atol=1e-5)
        assert np.isclose(g.color[1][lin][0], (0.25 + 0.5 + 0.75) / 3, atol=1e-6)


def test_extract_sphere():
    blocks, tsdf, weight = sphere_case()
    v, f, c, n_edges = T.extract(blocks, tsdf, weight, None, VS, R8)
    assert c is None and v.shape[0] == n_edges and f.shape[0] > 1000
    assert np.unique(f).size == v.shape[0]  # no unreferenced vertex
    assert T.is_closed_oriented(f) and T.euler(f) == 2
    vol = T.signed_volume(v, f)
    assert 0.97 < vol / (4 / 3 * np.pi * 0.1 ** 3) < 1.0  # positive: normals point outward
    d = np.linalg.norm(v - np.array([-0.013, 0.021, 0.003]), axis=1)
    assert np.abs(d - 0.1).max() < 0.1 * VS  # linear interpolation of a distance field
    # order: vertices by (block key, voxel, axis); triangles by (block key, voxel)
    gp = np.floor(v / VS + 1e-9).astype(np.int64)
    keys = T.pack_keys(gp // R8)
    assert np.all(np.diff(keys) >= 0)


def test_extract_torus_and_threshold():
    blocks, tsdf, weight = torus_case()
    v, f, _, _ = T.extract(blocks, tsdf, weight, None, VS, R8)
    assert T.is_closed_oriented(f) and T.euler(f) == 0
    # weight == threshold is not usable
    assert T.extract(blocks, tsdf, weight, None, VS, R8, weight_threshold=4.0)[1].shape == (0, 3)


# ---- the table -------------------------------------------------------------------------------------

def test_table_rows():
    rows, width = G.build_table()
    assert len(rows) == 256 and width == max(len(r) for r in rows) and width % 3 == 0
    for case, row in enumerate(rows):
        crossed = {e for e in range(12) if G.edge_mask(case) >> e & 1}
        assert set(row) == crossed  # no triangle uses an uncrossed edge, and every crossed edge appears
        assert len(row) % 3 == 0
        for k in range(0, len(row), 3):
            assert len(set(row[k:k + 3])) == 3
        assert set(rows[255 - case]) == crossed  # the complementary pattern crosses the same edges
    assert rows[0] == [] and rows[255] == []


def test_table_faces_agree_between_neighbours():
    """Two cubes sharing a face draw the same segments on it: for every case and face, the
    triangle edges lying in the face depend on that face's four signs alone."""
    rows, _ = G.build_table()
    seen = {}
    for case, row in enumerate(rows):
        for _, ring in G.FACES:
            on_face = {G.EDGE_OF[(min(a, b), max(a, b))] for a, b in zip(ring, ring[1:] + ring[:1])}
            segs = set()
            for k in range(0, len(row), 3):
                tri = row[k:k + 3]
                for a, b in ((tri[0], tri[1]), (tri[1], tri[2]), (tri[2], tri[0])):
                    if a in on_face and b in on_face:
                        segs.add(frozenset((a, b)))
            # interior fan diagonals can join two edges of one face only when the loop has both
            # on it; they come in opposite pairs, boundary segments once
            sign = tuple(case >> c & 1 for c in ring)
            key = (tuple(ring), sign)
            boundary = set()
            for s in segs:
                a, b = tuple(s)
                n = sum(1 for k in range(0, len(row), 3)
                        for x, y in ((row[k], row[k + 1]), (row[k + 1], row[k + 2]), (row[k + 2], row[k]))
                        if {x, y} == {a, b})
                if n == 1:
                    boundary.add(s)
            assert seen.setdefault(key, boundary) == boundary


def test_committed_header_is_the_generators():
    with open(G.HEADER) as fh:
        text = fh.read()
    assert text == G.render()
    rows, width = G.build_table()
    assert int(re.search(r"#define GSR_MC_ROW (\d+)", text).group(1)) == width
    assert os.path.basename(G.HEADER) == "mc_table.h"
