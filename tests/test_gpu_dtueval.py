"""GPU tests of the DTU Chamfer evaluation in HIP (csrc/pointeval.hip through
gsr_eval).

Yardsticks: tests/golden/dtueval.npz, the reference's own dtu_eval/eval.py run
(make_golden_dtueval.py), and beyond it the numpy / scipy restatement
tests/dtueval_ref.py, which tests/test_dtueval.py pins to that file.

Bars.  Sampled positions: 1e-12 * max|coord| (the same float64 operations in
the same order; the bar leaves a few ulps for sqrt and division).  Kept
indices, counts: exact (the generator asserts that no pair lies on the radius,
no lattice sum on 1, no distance on max_dist; the edge cases below are built
with the same room).  Distances: 1e-12 relative.  Means: 1e-9 relative (the
summation order differs; N * 2^-53 is far below that at these sizes).
"""
from __future__ import annotations

import os

import numpy as np
import pytest
import torch

import dtueval_ref as R

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "dtueval.npz")


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(GOLD))


def _t(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return (t if dtype is None else t.to(dtype)).to(DEV)


# ---- golden ------------------------------------------------------------------------------------------------------

def test_golden_sampling(gold):
    import gsr_eval as E

    got = E.sample_mesh_points(_t(gold["vertices"]), _t(gold["faces"]), float(gold["density"]))
    assert got.dtype == torch.float64 and got.is_cuda and tuple(got.shape) == gold["data_pcd"].shape
    err = np.abs(got.cpu().numpy() - gold["data_pcd"]).max()
    print("sampling: max |gsr - reference| =", err)
    assert err <= 1e-12 * np.abs(gold["data_pcd"]).max()


def test_golden_thinning(gold):
    import gsr_eval as E

    pts, idx = E.downsample_points(_t(gold["data_pcd"]), float(gold["density"]), perm=_t(gold["perm"], torch.int64))
    assert idx.dtype == torch.int64 and pts.dtype == torch.float64
    assert np.array_equal(idx.cpu().numpy(), gold["kept_index"].astype(np.int64))
    assert np.array_equal(pts.cpu().numpy(), gold["data_pcd"][gold["kept_index"]])


def test_golden_chamfer(gold):
    import gsr_eval as E

    md = float(gold["max_dist"])
    out = E.dtu_chamfer(_t(gold["vertices"]), _t(gold["faces"]), _t(gold["stl"]), _t(gold["obs_mask"]), gold["bb"],
                        float(gold["res"]), gold["plane"], density=float(gold["density"]), max_dist=md,
                        perm=_t(gold["perm"], torch.int64))
    assert out["n_sampled"] == gold["data_pcd"].shape[0] and out["n_down"] == gold["kept_index"].shape[0]
    assert (out["n_in"], out["n_in_obs"], out["n_stl_above"]) == (int(gold["n_in"]), int(gold["n_in_obs"]),
                                                                  int(gold["n_stl_above"]))
    for k in ("dist_d2s", "dist_s2d"):
        got, want = out[k].cpu().numpy(), gold[k]
        near = want < md
        assert np.array_equal(np.isfinite(got), near) and np.isinf(got[~near]).all()
        rel = (np.abs(got[near] - want[near]) / want[near]).max()
        print(k, "max relative error", rel)
        assert rel <= 1e-12
    for k in ("mean_d2s", "mean_s2d", "overall"):
        assert isinstance(out[k], float)
        print(k, out[k], float(gold[k]))
        assert abs(out[k] - float(gold[k])) <= 1e-9 * abs(float(gold[k]))


def test_golden_alignment(gold):
    import gsr_eval as E

    scale, rot, t = E.align_to_dtu(_t(gold["cam_centers"]), _t(gold["gt_centers"]))
    assert abs(scale - float(gold["align_scale"])) <= 1e-10 * float(gold["align_scale"])
    assert np.abs(rot - gold["align_R"]).max() <= 1e-10 and np.abs(t - gold["align_t"]).max() <= 1e-10 * 600
    v = E.apply_alignment(_t(gold["vertices"]), scale, rot, t)
    want = (gold["vertices"].astype(np.float64) * float(gold["align_scale"])) @ gold["align_R"].T + gold["align_t"]
    assert v.is_cuda and v.dtype == torch.float64 and np.abs(v.cpu().numpy() - want).max() <= 1e-10 * 700


def test_chamfer_of_nothing_is_nan(gold):
    import gsr_eval as E

    far = gold["stl"] + np.float32(500.0)  # every distance beyond max_dist
    out = E.dtu_chamfer(_t(gold["vertices"]), _t(gold["faces"]), _t(far), _t(gold["obs_mask"]).bool(), gold["bb"],
                        float(gold["res"]), gold["plane"], perm=_t(gold["perm"], torch.int64))
    assert np.isnan(out["mean_d2s"]) and np.isnan(out["mean_s2d"]) and np.isnan(out["overall"])
    assert torch.isinf(out["dist_d2s"]).all() and out["n_down"] == gold["kept_index"].shape[0]


# ---- sampling edges ----------------------------------------------------------------------------------------------

def _sample_case(name):
    rng = np.random.default_rng(7)
    if name == "no_faces":
        return rng.standard_normal((5, 3)), np.zeros((0, 3), np.int64)
    if name == "tiny":  # n1 = 0 or n2 = 0: edges shorter than thr
        v = np.array([[0, 0, 0], [0.15, 0, 0], [0, 0.9, 0], [0.9, 0.05, 0], [0.1, 0.1, 0.02]], float)
        return v, np.array([[0, 1, 2], [0, 3, 1], [0, 1, 4]])
    if name == "degenerate":  # zero-area (collinear, repeated point) and index-degenerate among real ones
        v = np.concatenate([rng.uniform(0, 3, (20, 3)), [[0, 0, 0], [1, 1, 1], [2, 2, 2], [1, 1, 1]]])
        f = rng.integers(0, 20, (30, 3))
        f[3] = [20, 21, 22]
        f[9] = [21, 23, 5]
        f[15] = [4, 4, 8]
        f[16] = [7, 2, 7]
        return v, f
    if name == "big_and_small":  # one triangle of about 5000 samples among 300 tiny ones
        v = np.concatenate([[[0, 0, 0], [20.3, 0.1, 0], [0.2, 20.1, 0.3]], rng.uniform(0, 0.5, (300, 3))])
        small = rng.integers(3, 303, (300, 3))
        f = np.concatenate([small[:140], [[0, 1, 2]], small[140:]])
        return v, f
    n = int(name)  # 255, 256, 257 triangles
    v = rng.uniform(0, 4, (60, 3))
    return v, rng.integers(0, 60, (n, 3))


@pytest.mark.parametrize("dtype", [torch.int32, torch.int64])
@pytest.mark.parametrize("name", ["no_faces", "tiny", "degenerate", "big_and_small", "255", "256", "257"])
def test_sampling_edges(name, dtype):
    import gsr_eval as E

    v, f = _sample_case(name)
    v = v.astype(np.float32)  # the mesh arrives as float32 and is widened
    want = R.sample_mesh_points_ref(v, f, 0.2)
    got = E.sample_mesh_points(_t(v), _t(f, dtype), 0.2).cpu().numpy()
    assert got.shape == want.shape, (got.shape, want.shape)
    if name == "no_faces":
        assert got.shape[0] == v.shape[0]
    if name == "big_and_small":
        assert want.shape[0] > 5000
    assert np.abs(got - want).max() <= 1e-12 * np.abs(want).max()
    got64 = E.sample_mesh_points(_t(v.astype(np.float64)), _t(f, dtype), 0.2).cpu().numpy()
    assert np.array_equal(got64, got)


def test_sampling_tiny_triangles_give_no_samples():
    v, f = _sample_case("tiny")
    lat = R.triangle_lattices(v.astype(np.float32), f, 0.2)
    assert any(n1 == 0 or n2 == 0 for _, n1, n2, *_ in lat)


def test_sampling_refuses_a_bad_vertex_id():
    import gsr_eval as E

    with pytest.raises(RuntimeError, match="outside"):
        E.sample_mesh_points(torch.rand(4, 3, device=DEV), torch.tensor([[0, 1, 2], [1, 2, 4]], device=DEV))


# ---- thinning edges ----------------------------------------------------------------------------------------------

def _thin(points, radius, perm):
    import gsr_eval as E

    E.last_call_stats = {}
    try:
        pts, idx = E.downsample_points(_t(points), radius, perm=_t(perm, torch.int64))
        rounds = E.last_call_stats.get("num_rounds", 0)
    finally:
        E.last_call_stats = None
    want_pts, want_idx = R.downsample_ref(points, radius, perm)
    assert np.array_equal(idx.cpu().numpy(), want_idx), (idx.shape, want_idx.shape)
    assert np.array_equal(pts.cpu().numpy(), want_pts)
    return idx.cpu().numpy(), rounds


def test_thinning_of_nothing_and_of_one_point():
    idx, _ = _thin(np.zeros((0, 3)), 0.2, np.zeros(0, np.int64))
    assert idx.shape == (0,)
    idx, _ = _thin(np.array([[1.0, -2.0, 3.0]]), 0.2, np.zeros(1, np.int64))
    assert idx.tolist() == [0]


def test_thinning_exact_duplicates():
    rng = np.random.default_rng(3)
    base = rng.uniform(-5, 5, (50, 3))
    pts = np.concatenate([base, base, base[:10]])
    perm = rng.permutation(pts.shape[0])
    idx, _ = _thin(pts, 0.05, perm)
    assert idx.shape[0] == 50  # one of every duplicated point (the points are farther apart than 0.05)


def test_thinning_many_points_in_one_radius():
    rng = np.random.default_rng(4)
    d = rng.standard_normal((600, 3))
    pts = 7.0 + 0.099 * d / np.linalg.norm(d, axis=1, keepdims=True) * rng.uniform(0, 1, (600, 1))
    perm = rng.permutation(600)
    idx, _ = _thin(pts, 0.2, perm)  # any two are closer than 0.198
    assert idx.tolist() == [perm[0]]


def test_thinning_chain_in_order_and_shuffled():
    line = np.zeros((400, 3))
    line[:, 0] = 0.75 * 0.2 * np.arange(400) - 11.0
    idx, rounds = _thin(line, 0.2, np.arange(400))
    assert idx.tolist() == list(range(0, 400, 2))  # every other point: each decision waits for the one before
    print("chain in order: rounds =", rounds)
    assert rounds >= 1
    _, rounds = _thin(line, 0.2, np.random.default_rng(5).permutation(400))
    print("chain shuffled: rounds =", rounds)


@pytest.mark.parametrize("offset", [0.0, 1e3])
def test_thinning_across_cell_boundaries(offset):
    rng = np.random.default_rng(6)
    r = 0.25
    corners = rng.integers(-6, 6, (300, 3)) * r  # cell corners on both sides of 0
    pts = np.concatenate([corners + rng.uniform(-0.3, 0.3, (300, 3)) * r,
                          corners + rng.uniform(-0.3, 0.3, (300, 3)) * r]) + offset * np.array([1.0, -1.0, 0.5])
    d = pts[:, None] - pts[None]
    d2 = (d * d).sum(-1)
    assert (np.abs(d2 - r * r) > 1e-9 * r * r).all()  # no pair on the radius
    idx, _ = _thin(pts, r, rng.permutation(600))
    assert 50 < idx.shape[0] < 600


def test_thinning_hashed_cells():
    """An extent of more than 2^64 cells in all: the cells are hashed."""
    rng = np.random.default_rng(8)
    seeds = rng.uniform(-1e6, 1e6, (40, 3))
    pts = (seeds[:, None] + rng.uniform(-0.3, 0.3, (40, 12, 3))).reshape(-1, 3)
    assert ((pts.max(0) - pts.min(0)) / 0.2 > 2 ** 22).all()  # 23 bits an axis
    idx, _ = _thin(pts, 0.2, rng.permutation(pts.shape[0]))
    assert 40 <= idx.shape[0] < pts.shape[0]


def test_thinning_same_seed_same_result():
    import gsr_eval as E

    pts = _t(np.random.default_rng(9).uniform(0, 2, (3000, 3)))
    outs = []
    for _ in range(2):
        g = torch.Generator(device=DEV)
        g.manual_seed(1234)
        outs.append(E.downsample_points(pts, 0.2, generator=g))
    assert torch.equal(outs[0][1], outs[1][1]) and torch.equal(outs[0][0], outs[1][0])
    kept = outs[0][0].cpu().numpy()
    d = kept[:, None] - kept[None]
    d2 = (d * d).sum(-1) + np.eye(kept.shape[0])
    assert (d2 > 0.04).all() and torch.equal(pts[outs[0][1]], outs[0][0])  # independent, and indexes the input


# ---- nearest edges -----------------------------------------------------------------------------------------------

def _nearest(query, ref, max_dist):
    import gsr_eval as E

    got = E.nearest_distance(_t(query), _t(ref), max_dist)
    assert got.dtype == torch.float64 and got.is_cuda and tuple(got.shape) == (query.shape[0],)
    got, want = got.cpu().numpy(), R.nearest_ref(query, ref, max_dist)
    near = np.isfinite(want)
    assert np.array_equal(np.isfinite(got), near) and np.isinf(got[~near]).all()
    if near.any():
        assert (np.abs(got[near] - want[near]) <= 1e-12 * np.maximum(want[near], 1e-300)).all()
    return got


def test_nearest_empty_sets_and_one_point():
    rng = np.random.default_rng(10)
    q = rng.uniform(-1, 1, (7, 3))
    assert _nearest(np.zeros((0, 3)), q, 1.0).shape == (0,)
    assert np.isinf(_nearest(q, np.zeros((0, 3)), 1.0)).all()
    got = _nearest(q, np.array([[0.1, 0.2, 0.3]]), 1.5)
    assert np.isfinite(got).any()


def test_nearest_far_outside_and_around_max_dist():
    rng = np.random.default_rng(11)
    ref = rng.uniform(0, 10, (2000, 3))
    far = rng.uniform(0, 10, (50, 3)) + np.array([500.0, -300.0, 0.0])
    out = np.array([[10.0 + 2.9, 5, 5], [5, -2.9, 5], [5, 5, 10.0 + 3.5]])  # outside the box, within reach or not
    # just inside and just beyond max_dist of an isolated ref point
    lone = np.array([[40.0, 40.0, 40.0]])
    u = rng.standard_normal((40, 3))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    ring = np.concatenate([lone + u[:20] * 3.0 * (1 - 1e-6), lone + u[20:] * 3.0 * (1 + 1e-6)])
    got = _nearest(np.concatenate([far, out, ring]), np.concatenate([ref, lone]), 3.0)
    assert np.isinf(got[:50]).all() and np.isfinite(got[53:73]).all() and np.isinf(got[73:]).all()


def test_nearest_coincident_points():
    rng = np.random.default_rng(12)
    ref = rng.uniform(-3, 3, (500, 3))
    got = _nearest(np.concatenate([ref[::5], ref[:3] + 1e-3]), ref, 0.5)
    assert (got[:100] == 0).all() and (got[100:] > 0).all()


def test_nearest_one_crowded_cell():
    rng = np.random.default_rng(13)
    ref = np.concatenate([rng.uniform(0, 0.01, (5000, 3)), rng.uniform(0, 50, (30, 3))])
    q = np.concatenate([rng.uniform(-0.5, 0.5, (200, 3)), rng.uniform(0, 50, (100, 3))])
    _nearest(q, ref, 20.0)


@pytest.mark.parametrize("Q,Rn", [(257, 1025), (1025, 257)])
def test_nearest_sizes_past_a_block(Q, Rn):
    rng = np.random.default_rng(Q)
    ref = np.concatenate([rng.uniform(-4, 4, (Rn - 200, 3)), rng.uniform(-4, 4, (200, 3)) * [1, 1, 0]])
    _nearest(rng.uniform(-5, 5, (Q, 3)), ref, 2.0)
    _nearest(rng.uniform(-5, 5, (Q, 3)) * [1, 0, 0], ref * [1, 1, 0], 0.7)  # a flat ref: cells from its area


# ---- arguments ---------------------------------------------------------------------------------------------------

def test_arguments():
    import gsr_eval as E

    pts = torch.rand(10, 3, dtype=torch.float64, device=DEV)
    with pytest.raises(RuntimeError):
        E.nearest_distance(pts.cpu(), pts, 1.0)
    with pytest.raises(RuntimeError):
        E.nearest_distance(pts.half(), pts, 1.0)
    with pytest.raises(RuntimeError):
        E.downsample_points(pts.half(), 0.2)
    with pytest.raises(RuntimeError):
        E.downsample_points(pts[:, :2], 0.2)
    with pytest.raises(RuntimeError):
        E.downsample_points(pts, 0.0)
    with pytest.raises(RuntimeError):
        E.sample_mesh_points(pts.cpu(), torch.zeros(1, 3, dtype=torch.int64, device=DEV))
    with pytest.raises(RuntimeError):
        E.sample_mesh_points(pts, torch.zeros(1, 4, dtype=torch.int64, device=DEV))
    with pytest.raises(RuntimeError):
        E.nearest_distance(pts, pts.reshape(-1), 1.0)
