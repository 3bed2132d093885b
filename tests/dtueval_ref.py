"""numpy / scipy restatement of the DTU Chamfer evaluation (the reference's
dtu_eval/eval.py --mode mesh and evaluate_dtu_mesh.py's alignment): the
yardstick of tests/test_gpu_dtueval.py beyond the golden file, pinned to the
golden file (the reference's own run) by tests/test_dtueval.py.

Sampling follows eval.py:48-71 operation by operation in float64; the thinning
is the sequential loop over a cKDTree radius query; the nearest-point query is
cKDTree.query with distance_upper_bound.
"""
from __future__ import annotations

import numpy as np
from scipy.spatial import cKDTree


def lattice(n1, n2):
    """sample_single_tri's k [m,2] for one triangle (eval.py:12-17) and the sums it thresholds."""
    c = np.mgrid[:n1 + 1, :n2 + 1]
    c = c + 0.5
    c[0] /= max(n1, 1e-7)
    c[1] /= max(n2, 1e-7)
    c = np.transpose(c, (1, 2, 0))
    s = c.sum(axis=-1)
    return c[s < 1], s


def triangle_lattices(vertices, faces, density=0.2):
    """Per triangle with area2 > 0: (index, n1, n2, l1 / thr, l2 / thr, v1, v2, p0)."""
    vertices = np.asarray(vertices, dtype=np.float64)
    tri_vert = vertices[np.asarray(faces).astype(np.int64)]
    v1 = tri_vert[:, 1] - tri_vert[:, 0]
    v2 = tri_vert[:, 2] - tri_vert[:, 0]
    l1 = np.linalg.norm(v1, axis=-1, keepdims=True)
    l2 = np.linalg.norm(v2, axis=-1, keepdims=True)
    area2 = np.linalg.norm(np.cross(v1, v2), axis=-1, keepdims=True)
    out = []
    for t in np.nonzero((area2 > 0)[:, 0])[0]:
        thr = density * np.sqrt(l1[t] * l2[t] / area2[t])
        r1, r2 = (l1[t] / thr)[0], (l2[t] / thr)[0]
        out.append((int(t), np.floor(r1), np.floor(r2), r1, r2, v1[t:t + 1], v2[t:t + 1], tri_vert[t:t + 1, 0]))
    return out


def sample_mesh_points_ref(vertices, faces, density=0.2):
    """eval.py:48-71: [V + S, 3] float64."""
    vertices = np.asarray(vertices, dtype=np.float64).reshape(-1, 3)
    faces = np.asarray(faces).reshape(-1, 3)
    new = [vertices]
    for _, n1, n2, _, _, v1, v2, p0 in (triangle_lattices(vertices, faces, density) if faces.shape[0] else []):
        k, _ = lattice(n1, n2)
        new.append(v1 * k[:, :1] + v2 * k[:, 1:] + p0)
    return np.concatenate(new, axis=0)


def downsample_ref(points, radius, perm, workers=1):
    """eval.py:80-94 with the shuffle given: (kept_points in shuffled order, kept_index into `points`)."""
    points = np.asarray(points, dtype=np.float64).reshape(-1, 3)
    perm = np.asarray(perm, dtype=np.int64)
    data = points[perm]
    if data.shape[0] == 0:
        return data, perm
    near = cKDTree(data).query_ball_point(data, radius, workers=workers)
    mask = np.ones(data.shape[0], dtype=np.bool_)
    for curr, idxs in enumerate(near):
        if mask[curr]:
            mask[idxs] = 0
            mask[curr] = 1
    return data[mask], perm[mask]


def nearest_ref(query, ref, max_dist, workers=1):
    """The distance to the nearest ref point where < max_dist, +inf otherwise."""
    query = np.asarray(query, dtype=np.float64).reshape(-1, 3)
    ref = np.asarray(ref, dtype=np.float64).reshape(-1, 3)
    if ref.shape[0] == 0 or query.shape[0] == 0:
        return np.full(query.shape[0], np.inf)
    d, _ = cKDTree(ref).query(query, k=1, distance_upper_bound=max_dist, workers=workers)
    return d


def dtu_chamfer_ref(vertices, faces, stl, obs_mask, bb, res, plane, perm, density=0.2, patch=60, max_dist=20):
    """eval.py:43-134, 157-166 with the shuffle given."""
    pcd = sample_mesh_points_ref(vertices, faces, density)
    down, kept = downsample_ref(pcd, density, perm)
    bb = np.asarray(bb).astype(np.float32)
    inbound = ((down >= bb[:1] - patch) & (down < bb[1:] + patch * 2)).sum(axis=-1) == 3
    data_in = down[inbound]
    grid = np.around((data_in - bb[:1]) / res).astype(np.int32)
    grid_inbound = ((grid >= 0) & (grid < np.expand_dims(obs_mask.shape, 0))).sum(axis=-1) == 3
    g = grid[grid_inbound]
    in_obs = obs_mask[g[:, 0], g[:, 1], g[:, 2]].astype(np.bool_)
    data_in_obs = data_in[grid_inbound][in_obs]
    stl = np.asarray(stl, dtype=np.float64)
    d2s = nearest_ref(data_in_obs, stl, max_dist)
    hom = np.concatenate([stl, np.ones_like(stl[:, :1])], -1)
    above = (np.asarray(plane, dtype=np.float64).reshape((1, 4)) * hom).sum(-1) > 0
    s2d = nearest_ref(stl[above], data_in, max_dist)
    near_d, near_s = d2s[d2s < max_dist], s2d[s2d < max_dist]
    mean_d2s = near_d.mean() if near_d.size else np.float64("nan")  # the reference's mean of nothing is nan too
    mean_s2d = near_s.mean() if near_s.size else np.float64("nan")
    return {"data_pcd": pcd, "kept_index": kept, "n_in": int(data_in.shape[0]), "n_in_obs": int(data_in_obs.shape[0]),
            "n_stl_above": int(above.sum()), "dist_d2s": d2s, "dist_s2d": s2d, "mean_d2s": float(mean_d2s),
            "mean_s2d": float(mean_s2d), "overall": float((mean_d2s + mean_s2d) / 2)}


def align_ref(points, gt_points):
    """evaluate_dtu_mesh.py:17-58, 158-163: (scale, R, t)."""
    points, gt_points = np.asarray(points, dtype=np.float64), np.asarray(gt_points, dtype=np.float64)
    scale = (np.linalg.norm(gt_points - gt_points.mean(axis=0), axis=1).mean() /
             np.linalg.norm(points - points.mean(axis=0), axis=1).mean())
    A = points * scale
    ca, cb = A.mean(axis=0), gt_points.mean(axis=0)
    U, _, Vt = np.linalg.svd(np.dot((A - ca).T, gt_points - cb))
    R = np.dot(Vt.T, U.T)
    if np.linalg.det(R) < 0:
        Vt[2, :] *= -1
        R = np.dot(Vt.T, U.T)
    return scale, R, cb - np.dot(R, ca)
