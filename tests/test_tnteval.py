"""CPU pins of the TnT F-score yardstick: the numpy restatement
tests/tnteval_ref.py on cases known by construction, its histogram rule against
the reference's own get_f1_score_histo2 (tests/golden/tnteval.npz, written by
make_golden_tnteval.py), and gsr_tnt's host-side parts (the readers, the
Umeyama formulas, trajectory_alignment).  No GPU.
"""
from __future__ import annotations

import json
import os

import numpy as np
import pytest

import tnteval_ref as R

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "tnteval.npz")


def _crop(axis, poly_uv, lo=-1.0, hi=1.0):
    u, v, w = R.AXES[axis]
    b = np.zeros((len(poly_uv), 3))
    b[:, u], b[:, v] = np.asarray(poly_uv, float).T
    return {"orthogonal_axis": axis, "axis_min": lo, "axis_max": hi, "bounding_polygon": b}


def _pts(axis, uvw):
    u, v, w = R.AXES[axis]
    p = np.zeros((len(uvw), 3))
    p[:, [u, v, w]] = np.asarray(uvw, float)
    return p


SQUARE = [(0, 0), (2, 0), (2, 2), (0, 2)]
ELL = [(0, 0), (3, 0), (3, 1), (1, 1), (1, 3), (0, 3)]


@pytest.mark.parametrize("axis", ["X", "Y", "Z"])
def test_restatement_crop_square_and_ell(axis):
    inside = [(1, 1, 0), (0.5, 1.5, 0.9), (1.9, 0.1, -0.9)]
    outside = [(3, 1, 0), (-0.5, 1, 0), (1, 2.5, 0), (1, -0.1, 0), (1, 1, 1.5), (1, 1, -1.5)]
    idx, kept = R.crop_ref(_pts(axis, inside + outside), _crop(axis, SQUARE))
    assert idx.tolist() == [0, 1, 2] and np.array_equal(kept, _pts(axis, inside))
    inside = [(0.5, 0.5, 0), (2.5, 0.5, 0), (0.5, 2.5, 0)]
    outside = [(2, 2, 0), (1.5, 1.5, 0), (2.5, 1.5, 0), (1.5, 2.5, 0), (3.5, 0.5, 0), (0.5, 3.5, 0)]
    idx, _ = R.crop_ref(_pts(axis, outside[:2] + inside + outside[2:]), _crop(axis, ELL))
    assert idx.tolist() == [2, 3, 4]


def test_restatement_crop_boundary_rules():
    c = _crop("Z", SQUARE, lo=-1.0, hi=1.0)
    up, dn = np.nextafter(1.0, 2.0), np.nextafter(-1.0, -2.0)
    pts = np.array([[1, 1, 1.0], [1, 1, -1.0], [1, 1, up], [1, 1, dn],
                    [1, 2.0, 0],   # p[v] on the top vertices' v: b < p && b' >= p holds for both side edges
                    [1, 0.0, 0],   # p[v] on the bottom vertices' v: no edge is active
                    [2.0, 1, 0],   # p[u] equal to the far node: not counted, one node below -> kept
                    [0.0, 1, 0]])  # p[u] equal to the near node: no node strictly below -> dropped
    idx, _ = R.crop_ref(pts, c)
    assert idx.tolist() == [0, 1, 4, 6]
    T = np.eye(4)
    T[:3, 3] = [0.25, -0.5, 0.125]
    idx, kept = R.crop_ref(pts[:1] - T[:3, 3], c, T)
    assert idx.tolist() == [0] and np.array_equal(kept, pts[:1])


def test_restatement_voxel_grid_of_known_means():
    # a 2 x 2 x 2 grid of voxels of side 1: min_bound 0, so origin -0.5 and cell c = [c - 0.5, c + 0.5); it
    # holds c and c + 0.25, whose mean is c + 0.125; cell (0, 0, 0) holds a third point, 0.125, as well
    cells = np.array([[x, y, z] for x in range(2) for y in range(2) for z in range(2)], float)
    pts = np.concatenate([cells, cells + 0.25, [[0.125, 0.125, 0.125]]])
    got_cells, counts, means = R.voxel_ref(pts, 1.0)
    assert np.array_equal(got_cells, cells.astype(np.int64))
    assert counts.tolist() == [3, 2, 2, 2, 2, 2, 2, 2]
    assert np.array_equal(means, cells + 0.125)
    order = np.random.default_rng(0).permutation(pts.shape[0])
    c2, n2, _ = R.voxel_ref(pts[order], 1.0)
    assert np.array_equal(c2, got_cells) and np.array_equal(n2, counts)  # the output order is the key's
    # the sum is the sequential loop's
    p = np.random.default_rng(1).uniform(0.1, 0.9, size=(600, 3))
    s = np.zeros(3)
    for row in p:
        s += row
    assert np.array_equal(R.voxel_ref(p, 4.0)[2][0], s / 600.0)


def test_restatement_nearest_ties_and_bound():
    ref = np.array([[0, 0, 0], [1, 0, 0], [0, 0, 0], [5, 5, 5]], float)
    q = np.array([[0.1, 0, 0], [0.5, 0, 0], [1.2, 0, 0], [9, 9, 9]], float)
    d, i = R.nearest_index_ref(q, ref, 2.0)
    assert i.tolist() == [0, 0, 1, -1] and np.isinf(d[3]) and d[1] == 0.5
    d, i = R.nearest_index_ref(q, ref[:0], 2.0)
    assert (i == -1).all() and np.isinf(d).all()
    assert R.nearest_index_ref(q[:1], ref, 0.1)[1].tolist() == [-1]  # d == max_dist is not < max_dist


def _similarity(seed=3):
    rng = np.random.default_rng(seed)
    q, _ = np.linalg.qr(rng.standard_normal((3, 3)))
    q *= np.sign(np.linalg.det(q))
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = 1.7 * q, [0.3, -2.0, 5.0]
    return T


def test_restatement_umeyama_recovers_a_similarity():
    import gsr_tnt as G

    T = _similarity()
    src = np.random.default_rng(4).standard_normal((50, 3))
    dst = R.transform_ref(src, T)
    idx = np.arange(50)
    for exact in (False, True):
        s1 = R.column_sums(R.icp_terms(src, dst, idx), exact)
        s2 = R.column_sums(R.icp_terms(src, dst, idx, np.concatenate([s1[2:5], s1[5:8]]) / 50), exact)
        for fn in (R.umeyama_from_sums, G.umeyama_from_sums):
            assert np.abs(fn(s1[0], s1[2:5], s1[5:8], s2[:9], s2[9]) - T).max() < 1e-12
    assert np.abs(R.umeyama_points(src, dst) - T).max() < 1e-12
    # a reflection between the clouds is not a similarity: the S fix keeps det R = +1
    M = R.umeyama_points(src, dst * np.array([1, 1, -1.0]))
    assert np.linalg.det(M[:3, :3]) > 0


def test_restatement_icp_converges_and_stops():
    rng = np.random.default_rng(5)
    g = np.stack(np.meshgrid(np.arange(20.0), np.arange(20.0), indexing="ij"), -1).reshape(-1, 2)
    tgt = np.concatenate([g, (0.6 * np.sin(0.9 * g[:, :1]) * np.cos(0.7 * g[:, 1:]))], 1) + 0.01 * rng.standard_normal((400, 3))
    T = np.eye(4)
    T[:3, 3] = [0.11, -0.07, 0.05]
    src = R.transform_ref(tgt, np.linalg.inv(T))
    out = R.icp_ref(src, tgt, 1.0, 20)
    assert out["iterations"] < 20 and out["fitness"] == 1.0 and np.abs(out["T"] - T).max() < 1e-9
    assert len(out["history"]) == out["iterations"] + 1 == len(out["indices"])
    assert R.icp_ref(src, tgt, 1.0, 1)["iterations"] == 1
    none = R.icp_ref(src + 100.0, tgt, 1e-3, 20)
    assert none["iterations"] == 0 and none["fitness"] == 0.0 and none["rmse"] == 0.0
    assert np.array_equal(none["T"], np.eye(4))


def test_histogram_rule_is_the_references():
    g = np.load(GOLD)
    tau, stretch, d1, d2 = float(g["tau"]), int(g["plot_stretch"]), g["d1"], g["d2"]
    assert np.abs(d1 - tau).min() > 1e-9 and np.abs(d2 - tau).min() > 1e-9
    edges = np.arange(0, tau * stretch, tau / 100)
    assert np.isin(d1, edges).sum() >= 40 and (d1 == edges[-1]).any() and (d1 >= tau * stretch).any()
    p, r, f, e1, c1, e2, c2 = R.histo_ref(tau, stretch, d1, d2)
    assert (p, r, f) == (float(g["precision"]), float(g["recall"]), float(g["fscore"]))
    for got, key in ((e1, "edges_source"), (c1, "cum_source"), (e2, "edges_target"), (c2, "cum_target")):
        assert np.array_equal(got, g[key])
    assert R.histo_ref(tau, stretch, [], d2)[:3] == (0, 0, 0)


def test_readers(tmp_path):
    import gsr_tnt as G

    crop = {"class_name": "SelectionPolygonVolume", "orthogonal_axis": "Y", "axis_min": -1.5, "axis_max": 2.25,
            "bounding_polygon": [[0.0, 0.0, 1.0], [2.0, 0.0, 1.0], [2.0, 0.0, 3.0]], "version_major": 1}
    (tmp_path / "c.json").write_text(json.dumps(crop))
    c = G.read_crop_volume(str(tmp_path / "c.json"))
    assert c["orthogonal_axis"] == "Y" and (c["axis_min"], c["axis_max"]) == (-1.5, 2.25)
    assert c["bounding_polygon"].dtype == np.float64 and c["bounding_polygon"].shape == (3, 3)
    poses = np.random.default_rng(0).standard_normal((3, 4, 4))
    text = ""
    for k, p in enumerate(poses):
        text += f"{k} {k} {k + 1}\n" + "\n".join(" ".join(repr(float(x)) for x in row) for row in p) + "\n"
    (tmp_path / "t.log").write_text(text)
    meta, got = G.read_trajectory(str(tmp_path / "t.log"))
    assert meta == [[0, 0, 1], [1, 1, 2], [2, 2, 3]] and np.array_equal(got, poses)
    assert G.SCENES_TAU == {"Barn": 0.01, "Caterpillar": 0.005, "Church": 0.025, "Courthouse": 0.025,
                            "Ignatius": 0.003, "Meetingroom": 0.01, "Truck": 0.005}
    assert G.MAX_POINT_NUMBER == 4e6


def test_trajectory_alignment_recovers_a_similarity_among_outliers():
    import gsr_tnt as G

    T = _similarity(8)
    rng = np.random.default_rng(9)
    est = rng.standard_normal((200, 3)) * 2.0
    gt = R.transform_ref(est, T)
    gt[::5] += rng.uniform(3.0, 9.0, size=(40, 3))  # 20 % gross outliers
    a = G.trajectory_alignment(est, gt, None, np.random.default_rng(11), max_iteration=2000)
    b = G.trajectory_alignment(est, gt, None, np.random.default_rng(11), max_iteration=2000)
    assert np.abs(a - T).max() < 1e-9 and np.array_equal(a, b)
    # gt_trans moves the ground-truth centres first
    S = _similarity(12)
    c = G.trajectory_alignment(est, R.transform_ref(est, T), S, np.random.default_rng(11), max_iteration=50)
    assert np.abs(c - S @ T).max() < 1e-9
