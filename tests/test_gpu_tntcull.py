"""GPU tests of the TnT mesh culling in HIP (csrc/meshraster.hip through gsr_tnt.render_mesh_depth,
mesh_view_votes and cull_mesh).

Yardstick: the numpy float32 restatement tests/tntcull_ref.py, which tests/test_tntcull.py pins on
the CPU against a float64 ray cast and against the reference's point_masks.  Everything here is compared
exactly: the depth map's bits, the int32 counts, the culled arrays.
"""
from __future__ import annotations

import numpy as np
import pytest
import torch

import tntcull_ref as R

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
H, W = 45, 70
K = dict(fx=64.0, fy=60.0, cx=32.0, cy=24.0)  # dyadic fx, cx: u = W - 1 can be hit exactly
EYE = np.eye(4)


def _T():
    import gsr_tnt
    return gsr_tnt


def _t(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return (t if dtype is None else t.to(dtype)).to(DEV)


def _gpu_depth(v, f, w2c, h=H, w=W, k=K, dtype=torch.int64, **kw):
    d, _ = _T().render_mesh_depth(_t(v, torch.float32), _t(np.asarray(f).reshape(-1, 3), dtype), w2c, h, w, **k, **kw)
    return d.cpu().numpy()


def _same_bits(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def _check_depth(v, f, w2c=EYE, h=H, w=W, k=K, **kw):
    v, f = np.asarray(v, np.float32).reshape(-1, 3), np.asarray(f, np.int64).reshape(-1, 3)
    want = R.depth_ref(v, f, w2c, h, w, **k, **kw)
    got = _gpu_depth(v, f, w2c, h, w, k, **kw)
    assert _same_bits(got, want), f"{(got.view(np.uint32) != want.view(np.uint32)).sum()} pixels differ"
    return got


def _px(u, v, z=1.0, k=K):
    """The camera-space point at depth z that projects to pixel coordinates (u, v)."""
    return [(u - k["cx"]) * z / k["fx"], (v - k["cy"]) * z / k["fy"], z]


ONE = {
    # name: (corners, covered: some pixel / none)
    "inside": ([_px(10.2, 8.4, 2), _px(50.7, 12.1, 3), _px(30.3, 40.6, 2.5)], True),
    "whole_image": ([_px(-300, -200, 2), _px(500, -200, 2), _px(35, 900, 2)], True),
    "crossing_znear": ([[-0.5, 0.3, -0.004], [0.6, 0.3, 0.004], [0.0, 0.2, 3.0]], True),
    "crossing_z0_two_behind": ([[-1.0, 0.4, -1.0], [1.0, 0.4, -1.5], [0.1, 0.1, 4.0]], True),
    "behind": ([[-1, -1, -2], [1, -1, -2], [0, 1, -3]], False),
    "beyond_zfar": ([[-1, -1, 21], [1, -1, 22], [0, 1, 25]], False),
    "straddling_zfar": ([[-3, -2, 15], [3, -2, 15], [0, 6, 30]], True),
    "zero_area": ([_px(10, 10, 2), _px(30, 30, 2), _px(20, 20, 2)], False),
    "repeated_corner": ([_px(10, 10, 2), _px(10, 10, 2), _px(40, 30, 2)], False),
    "edge_on": ([[0.0, -1.0, 1.0], [0.0, 1.0, 2.0], [0.0, 0.5, 4.0]], False),
    "corner_on_centre": ([_px(20.5, 10.5, 2), _px(40.5, 10.5, 2), _px(20.5, 30.5, 2)], True),
    "edge_through_centres": ([_px(5.5, 20.5, 2), _px(60.5, 20.5, 2), _px(30.0, 40.0, 2)], True),
    "off_left": ([_px(-40, 10), _px(-5, 20), _px(-20, 40)], False),
    "off_right": ([_px(75, 10), _px(120, 20), _px(90, 40)], False),
    "off_top": ([_px(10, -30), _px(40, -2), _px(60, -20)], False),
    "off_bottom": ([_px(10, 50), _px(40, 47), _px(60, 90)], False),
}


@pytest.mark.parametrize("name", list(ONE))
def test_single_triangle(name):
    corners, covered = ONE[name]
    for f in ([0, 1, 2], [0, 2, 1]):
        d = _check_depth(corners, [f])
        assert bool((d > 0).any()) == covered
    if name == "corner_on_centre":
        assert d[10, 20] == np.float32(2.0)  # the corner itself: edges are inclusive
    if name == "edge_through_centres":
        assert np.all(d[20, 6:60] == np.float32(2.0))
    if name == "whole_image":
        assert np.all(d == np.float32(2.0))


# (width, height) of the screen bound: one below, at and one above 32 centres (one lane / one wave) and one
# 64 x 64 tile (one wave / tile-split), and a bound of 3 x 2 tiles
BOUNDS = [(31, 1), (32, 1), (33, 1), (8, 4), (11, 3), (3, 11), (63, 63), (64, 64), (65, 64), (64, 65), (65, 65),
          (129, 70)]


@pytest.mark.parametrize("bw,bh", BOUNDS)
def test_size_classes(bw, bh):
    h, w = 90, 160
    k = dict(fx=150.0, fy=148.0, cx=80.0, cy=45.0)
    # corners at u in [10.25, 9.5 + bw], v likewise: the bound is ceil(lo - 1) .. floor(hi)
    c = [_px(10.25, 10.25, 2, k), _px(9.5 + bw, 10.25, 2.5, k), _px(10.25, 9.5 + bh, 3, k)]
    for f in ([0, 1, 2], [0, 2, 1]):
        sw, sh = R.bound_sizes(np.asarray(c, np.float32), [f], EYE, h, w, **k)
        assert (int(sw[0]), int(sh[0])) == (bw, bh)
        d = _check_depth(c, [f], EYE, h, w, k)
        assert min(bw, bh) < 3 or (d > 0).any()  # (a sliver one pixel high may miss every centre)


@pytest.fixture(scope="module")
def sphere():
    return R.icosphere(3)


@pytest.mark.parametrize("where", ["outside", "centre"])
def test_watertight_sphere(sphere, where):
    v, f = sphere
    c2w = R.look_at((0.3, -0.4, -3.0), (0, 0, 0)) if where == "outside" else R.look_at((0, 0, 0), (0.3, 0.2, 1.0))
    w2c = np.linalg.inv(c2w)
    d = _check_depth(v, f, w2c)
    inside = R.depth_f64(v, f, w2c, H, W, **K)[0] > 0  # the silhouette, rim included
    assert inside.sum() > 1000 and np.all(d[inside] > 0)
    assert _same_bits(d, _gpu_depth(v, f[:, [0, 2, 1]], w2c))


def test_layers_and_face_order():
    rng = np.random.default_rng(5)
    quads = []
    for z, s in ((3.0, 1.4), (2.5, 0.9)):
        quads += [[-s, -s, z], [s, -s * 0.8, z + 0.3], [s, s, z], [-s * 0.9, s, z - 0.2]]
    c = rng.uniform([-1.5, -1.0, 1.5], [1.5, 1.0, 4.0], (5000, 1, 3))
    small = (c + rng.normal(0, 0.03, (5000, 3, 3))).reshape(-1, 3)
    v = np.concatenate([np.asarray(quads), small]).astype(np.float32)
    f = np.concatenate([[[0, 1, 2], [0, 2, 3], [4, 5, 6], [4, 6, 7]], 8 + np.arange(15000).reshape(-1, 3)])
    d = _check_depth(v, f)
    assert (d > 0).mean() > 0.5
    for seed in (1, 2):
        assert _same_bits(d, _gpu_depth(v, np.random.default_rng(seed).permutation(f), EYE))


def test_empty_and_tiny_sizes(sphere):
    T = _T()
    v, f = sphere
    w2c = np.linalg.inv(R.look_at((0.3, -0.4, -3.0), (0, 0, 0)))
    assert np.all(_gpu_depth(v, np.zeros((0, 3), np.int64), w2c) == 0)
    assert np.all(_gpu_depth(np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int64), w2c) == 0)
    c, _ = T.mesh_view_votes(_t(v), _t(f), np.zeros((0, 4, 4)), H, W, **K)
    assert c.dtype == torch.int32 and c.shape == (v.shape[0],) and int(c.abs().sum()) == 0
    c, _ = T.mesh_view_votes(_t(np.zeros((0, 3), np.float32)), _t(np.zeros((0, 3), np.int64)), w2c[None], H, W, **K)
    assert c.shape == (0,)
    for h, w in ((1, 70), (45, 1), (1, 1)):
        k = dict(fx=64.0, fy=60.0, cx=w / 2, cy=h / 2)
        _check_depth(v, f, w2c, h, w, k)
        got, _ = T.mesh_view_votes(_t(v), _t(f), w2c[None], h, w, **k)
        assert np.array_equal(got.cpu().numpy(), R.votes_ref(v, f, w2c[None], h, w, **k))


def test_face_types_ids_devices_streams(sphere):
    T = _T()
    v, f = sphere
    w2c = np.linalg.inv(R.look_at((0.3, -0.4, -3.0), (0, 0, 0)))
    want = R.depth_ref(v, f, w2c, H, W, **K)
    assert _same_bits(_gpu_depth(v, f, w2c, dtype=torch.int32), want)
    assert _same_bits(_gpu_depth(v.astype(np.float64), f, w2c), want)
    for bad in (-1, v.shape[0]):
        g = f.copy()
        g[7, 1] = bad
        for dtype in (torch.int32, torch.int64):
            with pytest.raises(RuntimeError, match="outside"):
                T.render_mesh_depth(_t(v), _t(g, dtype), w2c, H, W, **K)
            with pytest.raises(RuntimeError, match="outside"):
                T.mesh_view_votes(_t(v), _t(g, dtype), w2c[None], H, W, **K)
    for call in (lambda: T.render_mesh_depth(torch.from_numpy(v), _t(f), w2c, H, W, **K),
                 lambda: T.mesh_view_votes(_t(v), torch.from_numpy(f), w2c[None], H, W, **K),
                 lambda: T.cull_mesh(torch.from_numpy(v), torch.from_numpy(f), w2c[None], H, W, **K)):
        with pytest.raises(RuntimeError, match="HIP device tensor"):
            call()
    s = torch.cuda.Stream(DEV)
    with torch.cuda.stream(s):
        d, _ = T.render_mesh_depth(_t(v), _t(f), w2c, H, W, **K)
        c, _ = T.mesh_view_votes(_t(v), _t(f), np.stack([w2c, w2c]), H, W, **K)
    s.synchronize()
    assert _same_bits(d.cpu().numpy(), want)
    assert np.array_equal(c.cpu().numpy(), R.votes_ref(v, f, np.stack([w2c, w2c]), H, W, **K))


def _wall(z=2.0):
    """A fronto-parallel wall over pixels 10.2 .. 50.7 x 8.3 .. 36.6 of the identity camera."""
    c = [_px(10.2, 8.3, z), _px(50.7, 8.3, z), _px(50.7, 36.6, z), _px(10.2, 36.6, z)]
    return np.asarray(c, np.float32), np.array([[0, 1, 2], [0, 2, 3]])


def _votes(v, f, w2cs, **kw):
    got, _ = _T().mesh_view_votes(_t(np.asarray(v, np.float32)), _t(np.asarray(f, np.int64).reshape(-1, 3)), w2cs,
                                  H, W, **K, **kw)
    want = R.votes_ref(np.asarray(v, np.float32), f, w2cs, H, W, **K, **kw)
    got = got.cpu().numpy()
    assert got.dtype == np.int32 and np.array_equal(got, want)
    return got


def test_vote_edges():
    wv, wf = _wall()
    x_last = np.float32(2 * (W - 1 - 32) / 64)  # u = (64 x + 32 * 2) / 2 = W - 1 exactly
    probes = np.array([
        [x_last, 0.0, 2.0],                            # 0: u = W - 1: inside
        [x_last + np.float32(1e-6), 0.0, 2.0],         # 1: just beyond (u = W - 1 + 3e-5)
        [0.0, 0.0, 0.0],                               # 2: z = 0 (+1e-8: u, v finite, far outside or on the border)
        [0.1, 0.1, -1.0],                              # 3: behind
        _px(30.0, 20.0, 2.0 + 0.005 - 1e-4),           # 4: just in front of wall + eps
        _px(30.0, 20.0, 2.0 + 0.005 + 1e-4),           # 5: just behind it
        _px(10.0, 20.0, 2.0),                          # 6: on the wall's first column (10), column 9 is a hole
        _px(9.6, 8.0, 2.0),                            # 7: between hole column 9 and column 10: d = 0.6 * 2
        _px(60.0, 40.0, 7.0),                          # 8: over empty pixels only
        _px(30.0, 20.0, 1.0),                          # 9: in front of the wall
        _px(30.0, 20.0, 3.0),                          # 10: far behind it
    ], np.float32)
    v = np.concatenate([wv, probes])
    got = _votes(v, wf, EYE[None])[4:]
    assert list(got[[0, 1, 3, 4, 5, 6, 7, 8, 9, 10]]) == [1, 0, 0, 1, 0, 1, 0, 1, 1, 0]
    # the hole is blended in: probe 7 samples 0 < d < 2 from the device's own map and loses its vote to it
    depth, _ = _T().render_mesh_depth(_t(v), _t(wf), EYE, H, W, **K)
    depth = depth.cpu().numpy()
    assert depth[8, 9] == 0 and depth[8, 10] == np.float32(2.0)
    d7 = R.votes_view_ref(v, depth, EYE, H, W, **K)[1]["d"][4 + 7]
    assert 0 < d7 < 2 and abs(d7 - 1.2) < 1e-3
    # an empty map: the wall behind the camera, and no faces at all
    flip = np.diag([1.0, 1.0, -1.0, 1.0])
    _votes(v, wf, flip[None])
    assert list(_votes(v, np.zeros((0, 3), np.int64), EYE[None])[4:][[0, 1, 3, 5, 10]]) == [1, 0, 0, 1, 1]


def test_vote_threshold_19_20_21_of_24():
    # a flat wall in the plane z = 0, a 0.1 grid over x in [-1, 1], y in [-0.4, 0.4]; 19 cameras see all of it,
    # one sees x >= -0.2, one x >= 0.5, three look away: the grid points (-0.6, 0), (0, 0), (0.6, 0) get 19, 20, 21
    x, y = np.meshgrid(np.arange(-10, 11) * 0.1, np.arange(-4, 5) * 0.1, indexing="ij")
    v = np.stack([x, y, np.zeros_like(x)], -1).reshape(-1, 3).astype(np.float32)
    k = (np.arange(20)[:, None] * 9 + np.arange(8)[None, :]).reshape(-1)
    f = np.concatenate([np.stack([k, k + 1, k + 9], 1), np.stack([k + 1, k + 10, k + 9], 1)])
    cams = [R.look_at((0.01 * (k - 9), 0.02 * (k % 3), -3.0), (0.01 * (k - 9), 0.02 * (k % 3), 0.0)) for k in range(19)]
    cams += [R.look_at((1.3, 0, -3.0), (1.3, 0, 0)), R.look_at((2.0, 0, -3.0), (2.0, 0, 0))]
    cams += [R.look_at((0.1 * k, 0, -3.0), (0.1 * k, 0, -9.0)) for k in range(3)]
    c2ws = np.stack(cams)
    got = _votes(v, f, np.linalg.inv(c2ws))
    a, b, c = 4 * 9 + 4, 10 * 9 + 4, 16 * 9 + 4
    assert [int(got[a]), int(got[b]), int(got[c])] == [19, 20, 21]
    v2, f2 = _T().cull_mesh(_t(v), _t(f), c2ws, H, W, **K, min_views=20)
    rv, rf = R.compact_ref(v, f, got >= 20)
    v2, f2 = v2.cpu().numpy(), f2.cpu().numpy()
    assert np.array_equal(v2, rv) and np.array_equal(f2, rf)

    def has(p):
        return bool((v2 == v[p]).all(1).any())

    assert not has(a) and has(b) and has(c)


def test_cull_nested_spheres():
    ov, of = R.icosphere(2, 1.0)
    iv, fi = R.icosphere(2, 0.5)
    v, f = np.concatenate([ov, iv]), np.concatenate([of, fi + ov.shape[0]])
    c2ws = R.around(3.0)
    v2, f2 = _T().cull_mesh(_t(v), _t(f, torch.int32), c2ws, H, W, **K, min_views=6, eps=0.05)
    rv, rf = R.cull_ref(v, f, c2ws, H, W, **K, min_views=6, eps=0.05)
    assert f2.dtype == torch.int64 and np.array_equal(v2.cpu().numpy(), rv) and np.array_equal(f2.cpu().numpy(), rf)
    assert np.array_equal(rv, ov) and np.array_equal(rf, of)


@pytest.fixture(scope="module")
def terrain_scene():
    """19,972 triangles with an overhang, 24 orbit views at 160 x 90; the restatement's counts, once."""
    h, w = 90, 160
    k = dict(fx=140.0, fy=139.0, cx=80.3, cy=44.6)
    v, f = R.terrain(96, 96)
    c2ws = R.orbit(24, 3.4, -1.9)
    counts = R.votes_ref(v, f, np.linalg.inv(c2ws), h, w, **k, zfar=20.0, eps=0.02)
    return h, w, k, v, f, c2ws, counts


def test_cull_terrain(terrain_scene):
    h, w, k, v, f, c2ws, counts = terrain_scene
    T = _T()
    assert f.shape[0] == 19972
    got, _ = T.mesh_view_votes(_t(v), _t(f), np.linalg.inv(c2ws), h, w, **k, eps=0.02)
    assert np.array_equal(got.cpu().numpy(), counts)
    assert 0 < (counts >= 8).sum() < v.shape[0]  # part of the mesh is seen by 8 views, part is not
    for mv in (8, 0, 25):
        v2, f2 = T.cull_mesh(_t(v), _t(f), c2ws, h, w, **k, min_views=mv, eps=0.02)
        rv, rf = R.compact_ref(v, f, counts >= mv)
        assert np.array_equal(v2.cpu().numpy(), rv) and np.array_equal(f2.cpu().numpy(), rf)
        if mv == 0:
            assert np.array_equal(rv, v) and np.array_equal(rf, f)
        if mv == 25:
            assert v2.shape == (0, 3) and f2.shape == (0, 3)
    # order preserved, faces remapped: every kept face names the same positions as before
    v2, f2 = T.cull_mesh(_t(v), _t(f), c2ws, h, w, **k, min_views=8, eps=0.02)
    keep = counts >= 8
    kf = f[keep[f].all(1)]
    assert np.array_equal(v2.cpu().numpy()[f2.cpu().numpy()], v[kf])
