"""A numpy restatement of the TnT F-score contract of DESIGN §6i (csrc/tnteval.hip,
gsr_tnt.py), the yardstick of tests/test_gpu_tnteval.py; tests/test_tnteval.py
pins it to cases known by construction and, for the histogram rule, to the
reference's own get_f1_score_histo2 (tests/golden/tnteval.npz).

Everything is float64 in the contract's operation order: elementwise numpy
expressions round as the device's uncontracted arithmetic does, np.add.at adds
one element after the other in index order (the sequential loop), and the
nearest index is a brute-force argmin, whose ties go to the lowest position.
open3d is not used anywhere: its rules are restated from its published
behaviour (DESIGN §6i lists which).
"""
from __future__ import annotations

import math

import numpy as np

AXES = {"X": (1, 2, 0), "Y": (0, 2, 1), "Z": (0, 1, 2)}
MAX_POINT_NUMBER = 4e6


def transform_ref(points, T):
    """p' = ((r0 x + r1 y) + r2 z) + t per row of the 4x4's first three."""
    p, T = np.asarray(points, np.float64), np.asarray(T, np.float64)
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    return np.stack([((T[r, 0] * x + T[r, 1] * y) + T[r, 2] * z) + T[r, 3] for r in range(3)], 1)


def crop_nodes(points, crop):
    """Per polygon edge: (active [M,N] bool, node [M,N]) for the points as given."""
    u, v, _ = AXES[crop["orthogonal_axis"]]
    b = np.asarray(crop["bounding_polygon"], np.float64).reshape(-1, 3)
    pv = points[:, v]
    act, nodes = [], []
    with np.errstate(all="ignore"):
        for i in range(b.shape[0]):
            j = (i + 1) % b.shape[0]
            a = ((b[i, v] < pv) & (b[j, v] >= pv)) | ((b[j, v] < pv) & (b[i, v] >= pv))
            node = b[i, u] + (pv - b[i, v]) / (b[j, v] - b[i, v]) * (b[j, u] - b[i, u])
            act.append(a)
            nodes.append(node)
    return np.array(act).reshape(b.shape[0], -1), np.array(nodes).reshape(b.shape[0], -1)


def crop_ref(points, crop, T=None):
    """-> (kept positions [K] int64 ascending, kept transformed points [K,3])."""
    p = np.asarray(points, np.float64).reshape(-1, 3)
    if T is not None:
        p = transform_ref(p, T)
    u, _, w = AXES[crop["orthogonal_axis"]]
    act, nodes = crop_nodes(p, crop)
    below = (act & (nodes < p[None, :, u])).sum(0)
    keep = ~((p[:, w] < crop["axis_min"]) | (p[:, w] > crop["axis_max"])) & (below % 2 == 1)
    idx = np.nonzero(keep)[0].astype(np.int64)
    return idx, p[idx]


def crop_gap(points, crop, T=None):
    """How far the case is from a tie: min over points of |p[w] - axis end|, |p[v] - a vertex's v|, and of
    |node - p[u]| over the active edges (absolute)."""
    p = np.asarray(points, np.float64).reshape(-1, 3)
    if T is not None:
        p = transform_ref(p, T)
    if p.shape[0] == 0:
        return np.inf
    u, v, w = AXES[crop["orthogonal_axis"]]
    b = np.asarray(crop["bounding_polygon"], np.float64).reshape(-1, 3)
    act, nodes = crop_nodes(p, crop)
    g = min(np.abs(p[:, w] - crop["axis_min"]).min(), np.abs(p[:, w] - crop["axis_max"]).min(),
            np.abs(p[:, v][None] - b[:, v][:, None]).min())
    d = np.abs(nodes - p[None, :, u])[act]
    return min(g, d.min()) if d.size else g


def voxel_cells(points, voxel):
    p = np.asarray(points, np.float64).reshape(-1, 3)
    origin = p.min(0) - 0.5 * voxel
    return np.floor((p - origin) / voxel).astype(np.int64), origin


def voxel_ref(points, voxel):
    """-> (cells [C,3] int64 ascending in (cx, cy, cz), counts [C] int64, means [C,3])."""
    p = np.asarray(points, np.float64).reshape(-1, 3)
    if p.shape[0] == 0:
        return np.zeros((0, 3), np.int64), np.zeros(0, np.int64), np.zeros((0, 3))
    cells, _ = voxel_cells(p, voxel)
    uniq, inv, counts = np.unique(cells, axis=0, return_inverse=True, return_counts=True)
    sums = np.zeros((uniq.shape[0], 3))
    np.add.at(sums, inv.reshape(-1), p)  # unbuffered: one point after the other, in input order
    return uniq, counts.astype(np.int64), sums / counts[:, None].astype(np.float64)


def voxel_gap(points, voxel):
    """min distance (in voxels) of a coordinate from a voxel face."""
    p = np.asarray(points, np.float64).reshape(-1, 3)
    f = (p - (p.min(0) - 0.5 * voxel)) / voxel
    return np.abs(f - np.round(f)).min()


def nearest_index_ref(query, ref, max_dist, chunk=512, with_gap=False):
    """Brute force: -> (dist [Q], index [Q] int64); the nearest ref point with distance < max_dist (ties: the
    lowest position), else (+inf, -1).  with_gap: also the smallest relative gap between the best and the
    second-best squared distance, and between a distance and max_dist."""
    q, r = np.asarray(query, np.float64).reshape(-1, 3), np.asarray(ref, np.float64).reshape(-1, 3)
    dist, idx = np.full(q.shape[0], np.inf), np.full(q.shape[0], -1, np.int64)
    gap = np.inf
    if r.shape[0]:
        for s in range(0, q.shape[0], chunk):
            d = q[s:s + chunk, None, :] - r[None]
            d2 = d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1] + d[..., 2] * d[..., 2]
            j = d2.argmin(1)
            best = d2[np.arange(d2.shape[0]), j]
            dd = np.sqrt(best)
            ok = dd < max_dist
            dist[s:s + chunk] = np.where(ok, dd, np.inf)
            idx[s:s + chunk] = np.where(ok, j, -1)
            if with_gap and r.shape[0] > 1:
                second = np.partition(d2, 1, axis=1)[:, 1]
                gap = min(gap, ((second - best) / np.maximum(second, 1e-300)).min())
            if with_gap and np.isfinite(max_dist):
                gap = min(gap, (np.abs(dd - max_dist) / max_dist).min())
    return (dist, idx, gap) if with_gap else (dist, idx)


def icp_terms(src, ref, index, means=None):
    """The float64 terms of gsr_icp_accumulate over the pairs with index >= 0, [n, 8] (pass 1: 1, d^2, s, t)
    or [n, 10] (pass 2, with means [6]: (s - ms)(t - mt)^T row-major, |s - ms|^2)."""
    ok = index >= 0
    s, t = src[ok], ref[index[ok]]
    if means is None:
        d = s - t
        d2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
        return np.concatenate([np.ones((s.shape[0], 1)), d2[:, None], s, t], 1)
    a, b = s - np.asarray(means[:3]), t - np.asarray(means[3:])
    h = (a[:, :, None] * b[:, None, :]).reshape(-1, 9)
    v = (a[:, 0] * a[:, 0] + a[:, 1] * a[:, 1]) + a[:, 2] * a[:, 2]
    return np.concatenate([h, v[:, None]], 1)


def column_sums(terms, exact=False):
    if exact:
        return np.array([math.fsum(terms[:, k]) for k in range(terms.shape[1])])
    return terms.sum(0) if terms.shape[0] else np.zeros(terms.shape[1])


def umeyama_from_sums(n, sum_s, sum_t, H, var_sum):
    """Eigen's umeyama with scaling from the two passes' sums: H = sum (s - ms)(t - mt)^T, var_sum =
    sum |s - ms|^2.  -> 4x4."""
    ms, mt = np.asarray(sum_s) / n, np.asarray(sum_t) / n
    sigma = np.asarray(H, np.float64).reshape(3, 3).T / n  # dst x src
    U, D, Vt = np.linalg.svd(sigma)
    S = np.array([1.0, 1.0, 1.0 if np.linalg.det(U) * np.linalg.det(Vt) > 0 else -1.0])
    R = U @ np.diag(S) @ Vt
    c = (D * S).sum() / (var_sum / n)
    T = np.eye(4)
    T[:3, :3] = c * R
    T[:3, 3] = mt - c * (R @ ms)
    return T


def icp_evaluate(src, ref, max_dist):
    dist, idx = nearest_index_ref(src, ref, max_dist)
    return dist, idx


def icp_ref(source, target, max_dist, max_iter, relative_fitness=1e-6, relative_rmse=1e-6, exact=False, nearest=None):
    """open3d's RegistrationICP loop with TransformationEstimationPointToPoint(True), from the identity.
    -> dict T, fitness, rmse, iterations, history [(fitness, rmse)], indices [per evaluation].  `exact`: the
    sums by math.fsum instead of numpy's."""
    nearest = nearest or (lambda q: nearest_index_ref(q, target, max_dist))
    src = np.array(source, np.float64).reshape(-1, 3)
    T = np.eye(4)
    N = src.shape[0]

    def evaluate():
        _, idx = nearest(src)
        s1 = column_sums(icp_terms(src, target, idx), exact)
        n = int(round(s1[0]))
        return idx, s1, (n / N if N else 0.0), (math.sqrt(s1[1] / n) if n else 0.0)

    idx, s1, fit, rmse = evaluate()
    history, indices, it = [(fit, rmse)], [idx], 0
    while it < max_iter and s1[0] > 0:
        n = s1[0]
        means = np.concatenate([s1[2:5] / n, s1[5:8] / n])
        s2 = column_sums(icp_terms(src, target, idx, means), exact)
        update = umeyama_from_sums(n, s1[2:5], s1[5:8], s2[:9], s2[9])
        T = update @ T
        src = transform_ref(src, update)
        it += 1
        prev = (fit, rmse)
        idx, s1, fit, rmse = evaluate()
        history.append((fit, rmse))
        indices.append(idx)
        if abs(prev[0] - fit) < relative_fitness and abs(prev[1] - rmse) < relative_rmse:
            break
    return {"T": T, "fitness": fit, "rmse": rmse, "iterations": it, "history": history, "indices": indices}


def crop_and_downsample_ref(points, crop, method, voxel=0.01, T=None):
    _, p = crop_ref(points, crop, T)
    if method == "voxel":
        return voxel_ref(p, voxel)[2]
    if p.shape[0] > MAX_POINT_NUMBER:
        return p[::int(round(p.shape[0] / float(MAX_POINT_NUMBER)))]
    return p


def registration_ref(source, target, init_T, crop, max_dist, max_iter, voxel=None, exact=False, nearest_factory=None):
    """registration_vol_ds (voxel given) / registration_unif (voxel None) of eval_tnt/registration.py."""
    method = "voxel" if voxel is not None else "uniform"
    s = crop_and_downsample_ref(source, crop, method, voxel or 0.01, init_T)
    t = crop_and_downsample_ref(target, crop, method, voxel or 0.01)
    nearest = nearest_factory(t, max_dist) if nearest_factory else None
    reg = icp_ref(s, t, max_dist, max_iter, exact=exact, nearest=nearest)
    reg["T"] = reg["T"] @ np.asarray(init_T, np.float64)
    return reg


def histo_ref(tau, plot_stretch, d1, d2):
    """get_f1_score_histo2 restated: -> precision, recall, fscore, edges1, cum1, edges2, cum2."""
    if len(d1) and len(d2):
        recall = float((np.asarray(d2) < tau).sum()) / float(len(d2))
        precision = float((np.asarray(d1) < tau).sum()) / float(len(d1))
        fscore = 2 * recall * precision / (recall + precision)
        bins = np.arange(0, tau * plot_stretch, tau / 100)
        h1, e1 = np.histogram(d1, bins)
        h2, e2 = np.histogram(d2, bins)
        return (precision, recall, fscore, e1, np.cumsum(h1).astype(float) / len(d1), e2,
                np.cumsum(h2).astype(float) / len(d2))
    z = np.array([0])
    return 0, 0, 0, z, z, z, z


def evaluate_histo_ref(source, target, T, crop, voxel, tau, plot_stretch=5, nearest_factory=None):
    s = crop_and_downsample_ref(source, crop, "voxel", voxel, T)
    t = crop_and_downsample_ref(target, crop, "voxel", voxel)
    if s.shape[0] == 0 or t.shape[0] == 0:
        return histo_ref(tau, plot_stretch, [], []) + (s, t, np.zeros(0), np.zeros(0))
    if nearest_factory:
        d1, d2 = nearest_factory(t, np.inf)(s)[0], nearest_factory(s, np.inf)(t)[0]
    else:
        d1, d2 = nearest_index_ref(s, t, np.inf)[0], nearest_index_ref(t, s, np.inf)[0]
    return histo_ref(tau, plot_stretch, d1, d2) + (s, t, d1, d2)


def mesh_cloud_ref(vertices, faces):
    v = np.asarray(vertices, np.float64)
    f = np.asarray(faces)
    return np.concatenate([v, ((v[f[:, 0]] + v[f[:, 1]]) + v[f[:, 2]]) / 3.0])


def tnt_fscore_ref(vertices, faces, gt_points, crop, init_T, tau, nearest_factory=None):
    """run.py:93-187: -> dict with precision, recall, fscore, the counts, the curves and the transform."""
    pcd, gt = mesh_cloud_ref(vertices, faces), np.asarray(gt_points, np.float64)
    kw = dict(nearest_factory=nearest_factory)
    r2 = registration_ref(pcd, gt, init_T, crop, tau * 80, 20, voxel=tau, **kw)
    r3 = registration_ref(pcd, gt, r2["T"], crop, tau * 20, 20, voxel=tau / 2.0, **kw)
    r = registration_ref(pcd, gt, r3["T"], crop, 2 * tau, 20, **kw)
    p, rc, f, e1, c1, e2, c2, s, t, d1, d2 = evaluate_histo_ref(pcd, gt, r["T"], crop, tau / 2.0, tau, **kw)
    return {"dTau": tau, "precision": p, "recall": rc, "fscore": f, "edges_source": e1, "cum_source": c1,
            "edges_target": e2, "cum_target": c2, "n_source": int(s.shape[0]), "n_target": int(t.shape[0]),
            "n_precise": int((d1 < tau).sum()), "n_recalled": int((d2 < tau).sum()), "transformation": r["T"],
            "registrations": (r2, r3, r), "dist_source": d1, "dist_target": d2}


def kdtree_nearest_factory(workers=16, gaps=None):
    """cKDTree in place of the brute force (only where ties are excluded).  `gaps`: a list that receives, per
    query call, the smallest relative gap between the nearest and the second-nearest distance and between a
    nearest distance and max_dist — what a caller asserts on to exclude ties."""
    from scipy.spatial import cKDTree

    def factory(ref, max_dist):
        tree = cKDTree(ref) if ref.shape[0] else None

        def query(q):
            if tree is None or q.shape[0] == 0:
                return np.full(q.shape[0], np.inf), np.full(q.shape[0], -1, np.int64)
            if gaps is not None and ref.shape[0] > 1:
                d2, _ = tree.query(q, k=2, workers=workers)
                g = ((d2[:, 1] - d2[:, 0]) / np.maximum(d2[:, 1], 1e-300)).min()
                if np.isfinite(max_dist):
                    g = min(g, (np.abs(d2[:, 0] - max_dist) / max_dist).min())
                gaps.append(float(g))
            _, j = tree.query(q, k=1, workers=workers)
            d = q - ref[j]  # the distance in the contract's own operation order
            dd = np.sqrt(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2])
            ok = dd < max_dist
            return np.where(ok, dd, np.inf), np.where(ok, j, -1).astype(np.int64)

        return query

    return factory


def umeyama_points(src, dst):
    """Umeyama with scale over index-to-index pairs (trajectory_alignment)."""
    src, dst = np.asarray(src, np.float64), np.asarray(dst, np.float64)
    n = src.shape[0]
    ms, mt = src.sum(0) / n, dst.sum(0) / n
    a, b = src - ms, dst - mt
    return umeyama_from_sums(n, src.sum(0), dst.sum(0), a.T @ b, (a * a).sum())
