"""GPU tests of the TnT F-score evaluation in HIP (csrc/tnteval.hip through
gsr_tnt).

Yardstick: the numpy restatement tests/tnteval_ref.py, which tests/test_tnteval.py
pins on the CPU, and tests/golden/tnteval.npz (the reference's own histogram
function) for evaluate_histo's rule.

Bars.  Crop positions, voxel cells and counts, nearest indices: exact, and the
points, means and distances bit-equal — the same float64 operations in the same
order.  Every generated case first asserts, on the restatement alone, that it is
free of ties (GUARD, relative: no coordinate on a voxel face, no node on p[u],
no distance on max_dist or tau, no two candidates equally near); the cases that
sit on a boundary on purpose are exact dyadic numbers whose answer follows from
the rules.  ICP sums: (n + 1) 2^-53 sum|term| from math.fsum of the same terms
(any summation order's worst case plus the term's own rounding).  The ICP's
final T: 8 x the difference between the restatement with numpy sums and with
math.fsum sums (the device's sums lie within the same order-of-summation
bound); floor, bar and measured value go to the file GSR_TNT_MARGIN_LOG names.
"""
from __future__ import annotations

import json
import math
import os

import numpy as np
import pytest
import torch

import tnteval_ref as R

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "tnteval.npz")
GUARD = 1e-9
U = 2.0 ** -53
ELL = np.array([(0, 0), (3, 0), (3, 1), (1, 1), (1, 3), (0, 3)], float)


def _t(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return (t if dtype is None else t.to(dtype)).to(DEV)


def _n(t):
    return t.cpu().numpy()


def _crop(axis, poly_uv, lo=-1.0, hi=1.0):
    u, v, w = R.AXES[axis]
    b = np.zeros((len(poly_uv), 3))
    b[:, u], b[:, v] = np.asarray(poly_uv, float).T
    b[:, w] = 7.0  # never read
    return {"orthogonal_axis": axis, "axis_min": lo, "axis_max": hi, "bounding_polygon": b}


def _similarity(deg, scale, shift, axis=(0.2, -0.3, 1.0)):
    a = np.asarray(axis, float) / np.linalg.norm(axis)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    th = math.radians(deg)
    T = np.eye(4)
    T[:3, :3] = scale * (np.eye(3) + math.sin(th) * K + (1 - math.cos(th)) * K @ K)
    T[:3, 3] = shift
    return T


def _log_margin(**row):
    path = os.environ.get("GSR_TNT_MARGIN_LOG")
    if path:
        with open(path, "a") as fh:
            fh.write(json.dumps(row) + "\n")


# ---- crop --------------------------------------------------------------------------------------------------------

def _check_crop(pts, crop, T=None, guard=True):
    import gsr_tnt as G

    if guard:
        assert R.crop_gap(pts, crop, T) > GUARD
    want_idx, want_pts = R.crop_ref(pts, crop, T)
    idx, kept, st = G.crop_points(_t(pts), crop, T)
    assert idx.dtype == torch.int64 and kept.dtype == torch.float64 and tuple(kept.shape) == (idx.numel(), 3)
    assert np.array_equal(_n(idx), want_idx)
    assert np.array_equal(_n(kept).view(np.uint64), want_pts.view(np.uint64))  # bit-equal
    assert "scratch_bytes" in st
    return want_idx


@pytest.mark.parametrize("axis", ["X", "Y", "Z"])
def test_crop_axes_concave_polygon_and_transform(axis):
    rng = np.random.default_rng(ord(axis))
    pts = rng.uniform(-1.5, 4.5, size=(2000, 3))
    crop = _crop(axis, ELL, lo=0.0, hi=2.5)
    T = _similarity(25.0, 1.1, [0.3, -0.2, 0.4])
    for tr in (None, np.eye(4), T):
        kept = _check_crop(pts, crop, tr)
        assert 50 < kept.shape[0] < 1500
    assert np.array_equal(R.crop_ref(pts, crop)[0], R.crop_ref(pts, crop, np.eye(4))[0])


def test_crop_boundary_rules():
    crop = _crop("Z", [(0, 0), (2, 0), (2, 2), (0, 2)], lo=-1.0, hi=1.0)
    up, dn = np.nextafter(1.0, 2.0), np.nextafter(-1.0, -2.0)
    pts = np.array([[1, 1, 1.0], [1, 1, -1.0], [1, 1, up], [1, 1, dn],  # both ends kept, one ulp outside dropped
                    [1, 2.0, 0],   # p[v] on the top vertices' v: the half-open rule makes both side edges active
                    [1, 0.0, 0],   # p[v] on the bottom vertices' v: no edge is active
                    [2.0, 1, 0],   # p[u] equal to the far node: not counted, one node below
                    [0.0, 1, 0]])  # p[u] equal to the near node: not counted, none below
    kept = _check_crop(pts, crop, guard=False)
    assert kept.tolist() == [0, 1, 4, 6]


@pytest.mark.parametrize("n", [0, 1, 255, 256, 257])
def test_crop_sizes(n):
    pts = np.random.default_rng(n).uniform(-0.5, 3.5, size=(n, 3)) * [1, 1, 0.2]
    _check_crop(pts, _crop("Z", ELL))


def test_crop_vertex_counts_and_all_dropped():
    import gsr_tnt as G

    rng = np.random.default_rng(3)
    pts = rng.uniform(-2.5, 2.5, size=(700, 3)) * [1, 1, 0.3]
    tri = [(-2, -2), (2, -1.5), (0.3, 2)]
    assert 0 < _check_crop(pts, _crop("Z", tri)).shape[0] < 700
    for m in (G.CROP_MAX_VERTICES, G.CROP_MAX_VERTICES + 1):
        ang = 2 * np.pi * (np.arange(m) + 0.25) / m
        star = np.stack([np.cos(ang), np.sin(ang)], 1) * (1.5 + 0.5 * (np.arange(m) % 2))[:, None]
        if m <= G.CROP_MAX_VERTICES:
            assert 0 < _check_crop(pts, _crop("Z", star)).shape[0] < 700
        else:
            with pytest.raises(RuntimeError, match="GSR_CROP_MAX_VERTICES"):
                G.crop_points(_t(pts), _crop("Z", star))
    assert _check_crop(pts + [10.0, 0, 0], _crop("Z", tri)).shape[0] == 0
    assert _check_crop(pts, _crop("Z", tri, lo=5.0, hi=6.0)).shape[0] == 0


# ---- voxel mean --------------------------------------------------------------------------------------------------

def _check_voxel(pts, voxel, guard=True):
    import gsr_tnt as G

    if guard and pts.shape[0]:
        assert R.voxel_gap(pts, voxel) > GUARD
    cells, counts, means = R.voxel_ref(pts, voxel)
    m, n, c, st = G.voxel_down_sample(_t(pts), voxel, return_cells=True)
    assert m.dtype == torch.float64 and n.dtype == torch.int64 and c.dtype == torch.int64
    assert np.array_equal(_n(c), cells) and np.array_equal(_n(n), counts)
    assert np.array_equal(_n(m).view(np.uint64), means.view(np.uint64))
    m2, _ = G.voxel_down_sample(_t(pts), voxel)
    assert torch.equal(m, m2)
    return counts


def test_voxel_on_faces_and_negative_coordinates():
    # dyadic coordinates with min 0 and voxel 1: origin -0.5, so k + 0.5 lies exactly on a face (it opens cell k + 1)
    g = np.array([0.0, 0.25, 0.5, 0.75, 1.5, 2.5, 2.75])
    pts = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)
    pts = pts[np.random.default_rng(0).permutation(pts.shape[0])]
    counts = _check_voxel(pts, 1.0, guard=False)
    assert counts.shape[0] == 4 ** 3  # cells 0 {0, .25}, 1 {.5, .75}, 2 {1.5}, 3 {2.5, 2.75} per axis
    _check_voxel(pts - 100.0, 1.0, guard=False)
    rng = np.random.default_rng(1)
    _check_voxel(rng.uniform(-7.0, -1.0, size=(3000, 3)), 0.37)


@pytest.mark.parametrize("n", [0, 1, 257, 1025])
def test_voxel_sizes(n):
    _check_voxel(np.random.default_rng(n).uniform(-1.0, 1.0, size=(n, 3)), 0.21)


def test_voxel_one_cell_and_one_each():
    rng = np.random.default_rng(5)
    one = rng.uniform(0.1, 0.9, size=(600, 3)) * [1.0, 1e3, 1e-3]  # uneven magnitudes: the order of the sum shows
    assert _check_voxel(one, 5e3).tolist() == [600]
    each = rng.permutation(np.stack(np.meshgrid(*[np.arange(9.0)] * 3, indexing="ij"), -1).reshape(-1, 3))
    each = each + rng.uniform(-0.2, 0.2, size=each.shape)
    each[0] = each.min(0) + 0.05  # keep min_bound off the other points' lattice
    counts = _check_voxel(each, 0.4)
    assert (counts == 1).all() and counts.shape[0] == 729


def test_voxel_rejects_overflow_and_nan():
    import gsr_tnt as G

    pts = np.random.default_rng(6).uniform(0, 1, size=(300, 3))
    far = pts.copy()
    far[0] = [1e9, 1e9, 1e9]  # 2^40 voxels of 1e-3 per axis: 120 key bits
    with pytest.raises(RuntimeError, match="64 bits"):
        G.voxel_down_sample(_t(far), 1e-3)
    bad = pts.copy()
    bad[17, 1] = np.nan
    with pytest.raises(RuntimeError, match="not finite"):
        G.voxel_down_sample(_t(bad), 0.1)
    with pytest.raises(RuntimeError, match="voxel"):
        G.voxel_down_sample(_t(pts), 0.0)


# ---- nearest index -----------------------------------------------------------------------------------------------

def _index_case(name):
    rng = np.random.default_rng(sum(map(ord, name)))
    q = rng.uniform(-1, 1, size=(700, 3))
    if name == "empty":
        return q, np.zeros((0, 3)), 0.5
    if name == "single":
        return q, np.array([[0.1, 0.2, 0.3]]), 0.9
    if name == "far":
        return np.concatenate([q, q + 50.0]), rng.uniform(-1, 1, size=(900, 3)), 0.4
    if name == "on_bound":
        ref = rng.uniform(-1, 1, size=(500, 3)) + [0, 0, 10.0]
        base = ref[rng.integers(0, 500, size=300)]
        dirs = rng.standard_normal((300, 3))
        dirs /= np.linalg.norm(dirs, axis=1, keepdims=True)
        md = 0.05
        off = np.where(np.arange(300) % 2 == 0, md * (1 - 1e-6), md * (1 + 1e-6))[:, None]
        return base + dirs * off, ref, md
    if name == "one_cell":
        ref = np.concatenate([rng.uniform(0, 1e-3, size=(5000, 3)), [[40.0, 40, 40], [-40.0, -40, -40]]])
        return np.concatenate([rng.uniform(-2e-3, 3e-3, size=(400, 3)), q]), ref, 100.0
    if name == "flat":
        return q, rng.uniform(-1, 1, size=(3000, 3)) * [1, 1, 0], 1.0
    if name == "line":
        # (few points: a query far from a dense line is nearly as far from the best point's neighbours)
        return q[:200], rng.uniform(-1, 1, size=(300, 1)) * [[1.0, 0.5, -0.25]], 1.5
    raise KeyError(name)


@pytest.mark.parametrize("name", ["empty", "single", "far", "on_bound", "one_cell", "flat", "line"])
def test_index_matches_brute_force_and_nearest(name):
    import gsr_eval as E
    import gsr_tnt as G

    q, ref, md = _index_case(name)
    want_d, want_i, gap = R.nearest_index_ref(q, ref, md, with_gap=True)
    assert gap > GUARD, f"{name}: a tie within {gap}"
    ix = G.NearestIndex.build(_t(ref))
    d, i, st = ix.query(_t(q), md)
    assert d.dtype == torch.float64 and i.dtype == torch.int64
    assert np.array_equal(_n(i), want_i)
    assert np.array_equal(_n(d).view(np.uint64), want_d.view(np.uint64))
    assert torch.equal(d.view(torch.int64), E.nearest_distance(_t(q), _t(ref), md).view(torch.int64))
    if name == "on_bound":
        assert (want_i[::2] >= 0).all() and (want_i >= 0).sum() < want_i.shape[0]


def test_index_duplicates_take_the_lowest_position():
    import gsr_tnt as G

    rng = np.random.default_rng(12)
    base = rng.uniform(-1, 1, size=(400, 3))
    ref = np.concatenate([base, base[::-1], base])  # every point three times: positions k, 799 - k, 800 + k
    q = base + 1e-4 * rng.standard_normal(base.shape)
    want_d, want_i = R.nearest_index_ref(q, ref, 0.5)
    assert np.array_equal(want_i, np.arange(400))
    d, i, _ = G.NearestIndex.build(_t(ref)).query(_t(q), 0.5)
    assert np.array_equal(_n(i), want_i) and np.array_equal(_n(d), want_d)


def test_index_built_once_serves_many_queries():
    import gsr_eval as E
    import gsr_tnt as G

    rng = np.random.default_rng(13)
    ref = _t(rng.uniform(-1, 1, size=(6000, 3)) * [1, 1, 0.1])
    ix = G.NearestIndex.build(ref)
    assert ix.build_stats["index_bytes"] >= 36 * 6000
    for k, md in enumerate((0.02, 0.2, 5.0)):
        q = _t(rng.uniform(-1.2, 1.2, size=(3000 + 100 * k, 3)))
        d, i, _ = ix.query(q, md)
        d2, i2, _ = G.NearestIndex.build(ref).query(q, md)
        assert torch.equal(i, i2) and torch.equal(d.view(torch.int64), d2.view(torch.int64))
        assert torch.equal(d.view(torch.int64), E.nearest_distance(q, ref, md).view(torch.int64))
        hit = i >= 0
        assert torch.equal(torch.isfinite(d), hit) and 0 < int(hit.sum())


# ---- ICP sums ----------------------------------------------------------------------------------------------------

def _check_sums(src, ref, index):
    import gsr_tnt as G

    s1, _ = G.icp_accumulate(_t(src), _t(ref), _t(index))
    n = int((index >= 0).sum())
    assert s1[0] == n  # exact
    t1 = R.icp_terms(src, ref, index)
    for k in range(1, 8):
        assert abs(s1[k] - math.fsum(t1[:, k])) <= (n + 1) * U * math.fsum(np.abs(t1[:, k])), ("pass 1", k)
    again, _ = G.icp_accumulate(_t(src), _t(ref), _t(index))
    assert np.array_equal(s1.view(np.uint64), again.view(np.uint64))
    if n == 0:
        assert not s1.any()
        return
    means = np.concatenate([s1[2:5] / n, s1[5:8] / n])  # the device's own pass-1 means
    s2, _ = G.icp_accumulate(_t(src), _t(ref), _t(index), means)
    t2 = R.icp_terms(src, ref, index, means)
    for k in range(10):
        assert abs(s2[k] - math.fsum(t2[:, k])) <= (n + 1) * U * math.fsum(np.abs(t2[:, k])), ("pass 2", k)
    again, _ = G.icp_accumulate(_t(src), _t(ref), _t(index), means)
    assert np.array_equal(s2.view(np.uint64), again.view(np.uint64))


@pytest.mark.parametrize("N,mode", [(5, "none"), (1, "full"), (300, "one"), (257, "sparse"), (257, "full"),
                                    (4097, "sparse"), (4097, "full")])
def test_icp_sums(N, mode):
    rng = np.random.default_rng(N + len(mode))
    src = rng.standard_normal((N, 3)) * [1, 10, 100] + [3, -20, 500]
    ref = rng.standard_normal((911, 3)) * [1, 10, 100] + [3, -20, 500]
    index = rng.integers(0, 911, size=N).astype(np.int64)
    if mode == "none":
        index[:] = -1
    elif mode == "one":
        index[:] = -1
        index[N // 2] = 7
    elif mode == "sparse":
        index[rng.uniform(size=N) < 0.8] = -1
    _check_sums(src, ref, index)


def test_icp_sums_reject_an_index_outside_ref():
    import gsr_tnt as G

    src, ref = _t(np.zeros((4, 3))), _t(np.ones((3, 3)))
    with pytest.raises(RuntimeError, match=r"outside \[-1, R\)"):
        G.icp_accumulate(src, ref, _t(np.array([0, 1, 3, -1])))


# ---- ICP ---------------------------------------------------------------------------------------------------------

def _surface(x, y):
    return 0.9 * np.sin(0.45 * x) * np.cos(0.38 * y) + 0.35 * np.sin(0.9 * x + 0.6 * y)


@pytest.fixture(scope="module")
def icp_scene():
    rng = np.random.default_rng(21)
    txy = rng.uniform(-2.0, 34.0, size=(6000, 2))
    target = np.concatenate([txy, _surface(txy[:, :1], txy[:, 1:])], 1)
    sxy = np.stack(np.meshgrid(np.arange(64) * 0.5, np.arange(64) * 0.5, indexing="ij"), -1).reshape(-1, 2)
    sxy = sxy + rng.uniform(-0.1, 0.1, size=sxy.shape)
    on = np.concatenate([sxy, _surface(sxy[:, :1], sxy[:, 1:])], 1)
    move = _similarity(3.0, 1.02, [0.9, -0.7, 0.3])  # a few 0.5 spacings
    return R.transform_ref(on, np.linalg.inv(move)), target


@pytest.mark.parametrize("case,max_dist,max_iter,rel", [("converges", 2.0, 40, 1e-3), ("runs_out", 2.0, 3, 1e-6),
                                                        ("no_pair", 1e-7, 20, 1e-6)])
def test_icp_against_restatement(icp_scene, case, max_dist, max_iter, rel):
    import gsr_tnt as G

    src, tgt = icp_scene
    gaps = []
    plain = R.icp_ref(src, tgt, max_dist, max_iter, rel, rel,
                      nearest=R.kdtree_nearest_factory(gaps=gaps)(tgt, max_dist))
    assert min(gaps) > GUARD, f"a tie within {min(gaps)}"
    exact = R.icp_ref(src, tgt, max_dist, max_iter, rel, rel, exact=True,
                      nearest=R.kdtree_nearest_factory()(tgt, max_dist))
    if case == "converges":
        assert 0 < plain["iterations"] < max_iter
    elif case == "runs_out":
        assert plain["iterations"] == max_iter
    else:
        assert plain["iterations"] == 0 and plain["fitness"] == 0.0
    src_d = _t(src)
    keep = src_d.clone()
    got = G.registration_icp(src_d, G.NearestIndex.build(_t(tgt)), max_dist, max_iter, rel, rel)
    assert torch.equal(src_d, keep)  # the caller's source is not moved
    assert got["iterations"] == plain["iterations"] and len(got["history"]) == len(plain["history"])
    for k, (idx, (fit, rmse)) in enumerate(zip(got["indices"], got["history"])):
        assert np.array_equal(_n(idx), plain["indices"][k]), f"correspondences differ at evaluation {k}"
        n = int((plain["indices"][k] >= 0).sum())
        assert fit == plain["history"][k][0]
        assert abs(rmse - plain["history"][k][1]) <= (n + 1) * U * max(plain["history"][k][1], 1e-300)
    assert (got["fitness"], got["rmse"]) == got["history"][-1]
    floor = float(np.abs(plain["T"] - exact["T"]).max())
    bar = 8.0 * floor
    err = float(np.abs(got["T"] - plain["T"]).max())
    print(f"icp {case}: floor {floor:.3e} bar {bar:.3e} measured {err:.3e} iterations {got['iterations']}")
    _log_margin(test="icp_T", case=case, floor=floor, bar=bar, measured=err, iterations=got["iterations"])
    assert err <= bar
    if case == "no_pair":
        assert np.array_equal(got["T"], np.eye(4))


# ---- end to end --------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def tnt_scene():
    rng = np.random.default_rng(31)
    n, h = 39, 0.25

    def bumps(x, y):
        return 0.25 * _surface(4.0 * x, 4.0 * y)

    gx, gy = np.meshgrid(np.arange(n) * h, np.arange(n) * h, indexing="ij")
    gx, gy = gx + rng.uniform(-0.04, 0.04, gx.shape), gy + rng.uniform(-0.04, 0.04, gy.shape)
    sheet = np.stack([gx, gy, bumps(gx, gy)], -1).reshape(-1, 3)
    idx = np.arange(n * n).reshape(n, n)
    a, b, c, d = idx[:-1, :-1].ravel(), idx[1:, :-1].ravel(), idx[:-1, 1:].ravel(), idx[1:, 1:].ravel()
    tris = np.concatenate([np.stack([a, b, c], 1), np.stack([d, c, b], 1)])
    vertices = np.concatenate([sheet, sheet + [0.0, 0.0, 6.0]])
    faces = np.concatenate([tris, tris + n * n]).astype(np.int64)
    gxy = rng.uniform(-0.25, 9.75, size=(10000, 2))
    gt = np.concatenate([gxy, bumps(gxy[:, :1], gxy[:, 1:])], 1) + 0.004 * rng.standard_normal((10000, 3))
    upper = np.arange(10000) % 2 == 1
    gt[upper, 2] += 6.0
    gt = gt[~(upper & (gt[:, 0] > 7.5))]  # the upper sheet is partly missing from the scan
    ell = np.array([(0.5, 0.5), (9, 0.5), (9, 4.25), (4.75, 4.25), (4.75, 9), (0.5, 9)], float)
    crop = _crop("Z", ell, lo=-1.5, hi=7.5)
    off = _similarity(1.0, 1.01, [0.06, -0.05, 0.03])
    init = np.linalg.inv(off)
    tau = 0.05  # 80 tau, the first registration's threshold, stays below the 6 between the sheets
    gaps = []
    want = R.tnt_fscore_ref(R.transform_ref(vertices, off), faces, gt, crop, init, tau,
                            nearest_factory=R.kdtree_nearest_factory(gaps=gaps))
    # ---- what lets the counts be compared exactly: wherever a transform of the device's may differ from the
    # restatement's in its last bits, nothing downstream sits on a boundary
    moved = R.mesh_cloud_ref(R.transform_ref(vertices, off), faces)
    r2, r3, r = want["registrations"]
    for T, voxel in ((r2["T"], tau / 2.0), (r["T"], tau / 2.0)):
        assert R.crop_gap(moved, crop, T) > GUARD
        assert R.voxel_gap(R.crop_ref(moved, crop, T)[1], voxel) > GUARD
    assert R.crop_gap(moved, crop, r3["T"]) > GUARD
    assert min(gaps) > GUARD
    edges = want["edges_source"]
    for dd in (want["dist_source"], want["dist_target"]):
        assert np.abs(dd - tau).min() > GUARD * tau
        assert np.abs(dd[:, None] - edges[None]).min() > GUARD * tau
    assert 0.05 < want["recall"] < 1.0 and 0.05 < want["precision"] < 1.0
    return dict(vertices=R.transform_ref(vertices, off), faces=faces, gt=gt, crop=crop, init=init, tau=tau, want=want)


def test_tnt_fscore_end_to_end(tnt_scene):
    import gsr_tnt as G

    s, want = tnt_scene, tnt_scene["want"]
    got = G.tnt_fscore(_t(s["vertices"]), _t(s["faces"]), _t(s["gt"]), s["crop"], s["init"], s["tau"])
    for k in ("n_source", "n_target", "n_precise", "n_recalled"):
        assert got[k] == want[k], k
    for k in ("precision", "recall", "fscore"):
        assert got[k] == want[k], k  # bit-equal: the same integers divided
    assert got["dTau"] == s["tau"]
    for k in ("edges_source", "cum_source", "edges_target", "cum_target"):
        assert np.array_equal(got[k], want[k]), k
    for a, b in zip(got["registrations"], want["registrations"]):
        assert a["iterations"] == b["iterations"]
    err = float(np.abs(got["transformation"] - want["transformation"]).max())
    print("tnt_fscore: max |T - restatement| =", err, "precision / recall / f =", got["precision"], got["recall"],
          got["fscore"])
    _log_margin(test="tnt_fscore_T", measured=err, precision=got["precision"], recall=got["recall"],
                fscore=got["fscore"])


def test_evaluate_histo_rule_on_golden_distances():
    import gsr_tnt as G

    g = np.load(GOLD)
    tau, stretch = float(g["tau"]), int(g["plot_stretch"])
    out = G.f1_score_histo(tau, stretch, _t(g["d1"]), _t(g["d2"]))
    assert (out["precision"], out["recall"], out["fscore"]) == (float(g["precision"]), float(g["recall"]),
                                                                float(g["fscore"]))
    for k in ("edges_source", "cum_source", "edges_target", "cum_target"):
        assert np.array_equal(out[k], g[k]), k
    empty = G.f1_score_histo(tau, stretch, _t(g["d1"])[:0], _t(g["d2"]))
    assert (empty["precision"], empty["recall"], empty["fscore"]) == (0, 0, 0)


def test_evaluate_histo_of_an_empty_crop_is_zero(tnt_scene):
    import gsr_tnt as G

    s = tnt_scene
    far = _t(s["vertices"] + [500.0, 0, 0])
    out = G.evaluate_histo(far, _t(s["gt"]), np.eye(4), s["crop"], s["tau"] / 2, s["tau"])
    assert (out["precision"], out["recall"], out["fscore"], out["n_source"]) == (0, 0, 0, 0) and out["n_target"] > 0


# ---- errors ------------------------------------------------------------------------------------------------------

def test_errors():
    import gsr_tnt as G

    pts = np.random.default_rng(0).uniform(0, 1, size=(50, 3))
    crop = _crop("Z", ELL)
    cpu, f32 = torch.from_numpy(pts), _t(pts, torch.float32)
    for bad in (cpu, f32, _t(pts)[:, :2]):
        with pytest.raises(RuntimeError):
            G.crop_points(bad, crop)
        with pytest.raises(RuntimeError):
            G.voxel_down_sample(bad, 0.1)
        with pytest.raises(RuntimeError):
            G.NearestIndex.build(bad)
        with pytest.raises(RuntimeError):
            G.transform_points_(bad, np.eye(4))
    ix = G.NearestIndex.build(_t(pts))
    for bad in (cpu, f32):
        with pytest.raises(RuntimeError):
            ix.query(bad, 1.0)
    with pytest.raises(RuntimeError, match="max_dist"):
        ix.query(_t(pts), 0.0)
    idx = np.zeros(50, np.int64)
    for bad in (_t(idx, torch.int32), torch.from_numpy(idx), _t(idx)[:10]):
        with pytest.raises(RuntimeError):
            G.icp_accumulate(_t(pts), _t(pts), bad)
    with pytest.raises(RuntimeError):
        G.registration_icp(_t(pts), _t(pts), 1.0, 5)
    with pytest.raises(RuntimeError):
        G.crop_points(_t(pts), crop, np.eye(3))
