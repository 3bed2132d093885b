"""Tanks and Temples F-score evaluation on the device (the reference's
eval_tnt/run.py, which is open3d on the CPU) over the C ABI: polygon-volume
crop, voxel-mean grid, a nearest-point index built once and queried many
times, and the correspondence sums of point-to-point ICP in HIP
(gsr_points_crop_polygon, gsr_points_voxel_mean, gsr_points_index_build /
_query, gsr_icp_accumulate, gsr_points_transform; csrc/tnteval.hip); the 3x3
SVD of each ICP update, the readers and the camera-centre RANSAC on the host in
numpy float64.  All geometry is float64.

The step before it, eval_tnt/cull_mesh.py (pyrender depth maps and a per-vertex
view vote), is here too: render_mesh_depth, mesh_view_votes and cull_mesh over
gsr_mesh_depth / gsr_mesh_view_votes (csrc/meshraster.hip), float32 as the
reference's vote is.

    vertices, faces = cull_mesh(vertices, faces, read_cull_trajectory("Barn_COLMAP_SfM.log"))

    crop = read_crop_volume("Barn.json")
    init = trajectory_alignment(est_centers, gt_centers, gt_trans, np.random.default_rng(0))
    out = tnt_fscore(vertices, faces, gt_points, crop, init, SCENES_TAU["Barn"])
    out["precision"], out["recall"], out["fscore"]

Device tensors on the current stream; there is no CPU path.  Every device call
returns a stats dict as its last value: scratch_bytes, and stage_ms (GPU
milliseconds per stage) when `measure_stages` is set — measuring synchronises,
so it is off by default and stage_ms is then None.
"""
from __future__ import annotations

import ctypes
import json
import math

import numpy as np
import torch

from diff_gaussian_rasterization._abi import (Out, PointIndex as _PointIndex, ScratchBlocks, call, f32ptr, f64ptr, load,
                                              ptr, require, require_points, stage_buffer, stage_stats, stream)

SCENES_TAU = {"Barn": 0.01, "Caterpillar": 0.005, "Church": 0.025, "Courthouse": 0.025, "Ignatius": 0.003,
              "Meetingroom": 0.01, "Truck": 0.005}
MAX_POINT_NUMBER = 4e6
CROP_MAX_VERTICES = 1024  # GSR_CROP_MAX_VERTICES
CROP_STAGES = ("flags_scan", "write")
VOXEL_STAGES = ("bounds", "keys", "sort", "heads_scan", "emit")
BUILD_STAGES = ("bounds", "ref_sort")
QUERY_STAGES = ("query_sort", "search")
ICP_STAGES = ("sums",)
TRANSFORM_STAGES = ("transform",)
RASTER_STAGES = ("clear", "setup_small", "unit_scan", "wave_units", "finish_or_vote")
RASTER_COUNTERS = ("atomics", "centres_tested", "lane_triangles", "wave_units")
_AXIS = {"X": 0, "Y": 1, "Z": 2}
measure_stages = False


def _mat4(T, who):
    T = np.ascontiguousarray(np.asarray(T.detach().cpu().numpy() if isinstance(T, torch.Tensor) else T,
                                        dtype=np.float64))
    if T.shape != (4, 4):
        raise RuntimeError(f"{who}: a transform must have shape (4, 4) (got {T.shape})")
    return T


# ---- readers -----------------------------------------------------------------------------------------------------

def read_crop_volume(path):
    """The crop file of a TnT scene (open3d's SelectionPolygonVolume JSON) -> dict: orthogonal_axis "X" / "Y" /
    "Z", axis_min, axis_max, bounding_polygon [M,3] float64."""
    with open(path) as fh:
        data = json.load(fh)
    axis = str(data["orthogonal_axis"]).upper()
    if axis not in _AXIS:
        raise RuntimeError(f"read_crop_volume: orthogonal_axis must be X, Y or Z (got {data['orthogonal_axis']!r})")
    poly = np.asarray(data["bounding_polygon"], dtype=np.float64).reshape(-1, 3)
    return {"orthogonal_axis": axis, "axis_min": float(data["axis_min"]), "axis_max": float(data["axis_max"]),
            "bounding_polygon": poly}


def read_trajectory(path):
    """The .log trajectory format: per camera a metadata line of integers, then the four rows of its 4x4 pose
    -> (metadata [n] lists of int, poses [n,4,4] float64)."""
    meta, poses = [], []
    with open(path) as fh:
        lines = [ln for ln in fh.read().split("\n")]
    k = 0
    while k < len(lines) and lines[k].strip():
        meta.append([int(x) for x in lines[k].split()])
        rows = [np.array(lines[k + 1 + r].split(), dtype=np.float64) for r in range(4)]
        if any(r.shape != (4,) for r in rows):
            raise RuntimeError(f"read_trajectory: {path}: a pose row without four numbers after line {k + 1}")
        poses.append(np.stack(rows))
        k += 5
    return meta, np.array(poses, dtype=np.float64).reshape(-1, 4, 4)


# ---- device calls ------------------------------------------------------------------------------------------------

@torch.no_grad()
def crop_points(points, crop, transform=None):
    """open3d's SelectionPolygonVolume.crop_point_cloud after an optional 4x4: points [N,3] float64 ->
    (kept_index [K] int64 ascending, kept transformed points [K,3] float64, stats)."""
    who = "crop_points"
    require_points(points, "points", who)
    dev = points.device
    points = points.contiguous()
    poly = np.ascontiguousarray(np.asarray(crop["bounding_polygon"], dtype=np.float64).reshape(-1, 3))
    T = None if transform is None else _mat4(transform, who)
    kept, out, scratch = Out(dev, torch.int64), Out(dev, torch.float64), ScratchBlocks(dev)
    K, ms = ctypes.c_longlong(0), stage_buffer(measure_stages)
    call(dev, "gsr_points_crop_polygon", kept.cb, None, out.cb, None, scratch.cb, None, points.size(0), ptr(points),
         None if T is None else f64ptr(T), _AXIS[crop["orthogonal_axis"]], float(crop["axis_min"]),
         float(crop["axis_max"]), poly.shape[0], f64ptr(poly), ctypes.byref(K), ms, stream(dev))
    return kept.tensor[:K.value], out.tensor[:3 * K.value].view(-1, 3), stage_stats(CROP_STAGES, ms, scratch)


@torch.no_grad()
def voxel_down_sample(points, voxel_size, return_cells=False):
    """open3d's PointCloud.voxel_down_sample: points [N,3] float64 -> (means [C,3] float64, one per occupied
    voxel, ascending in the voxel's (cx, cy, cz); stats) or, with return_cells, (means, counts [C] int64, cells
    [C,3] int64, stats)."""
    who = "voxel_down_sample"
    require_points(points, "points", who)
    dev = points.device
    points = points.contiguous()
    means, counts, cells = Out(dev, torch.float64), Out(dev, torch.int64), Out(dev, torch.int64)
    scratch = ScratchBlocks(dev)
    C, ms = ctypes.c_longlong(0), stage_buffer(measure_stages)
    call(dev, "gsr_points_voxel_mean", means.cb, None, counts.cb, None, cells.cb, None, scratch.cb, None,
         points.size(0), ptr(points), float(voxel_size), ctypes.byref(C), ms, stream(dev))
    st = stage_stats(VOXEL_STAGES, ms, scratch)
    m = means.tensor[:3 * C.value].view(-1, 3)
    if return_cells:
        return m, counts.tensor[:C.value], cells.tensor[:3 * C.value].view(-1, 3), st
    return m, st


def uniform_down_sample(points, every_k):
    """open3d's uniform_down_sample: every k-th point from the first."""
    if int(every_k) < 1:
        raise RuntimeError("uniform_down_sample: every_k must be at least 1")
    return points[::int(every_k)]


class NearestIndex:
    """gsr_points_nearest's ref half, done once: NearestIndex.build(ref) -> index; index.query(query, max_dist)
    any number of times.  The index owns its device buffer and keeps `ref` (the ICP sums read it)."""

    def __init__(self, ref, buffer, desc, stats):
        self.ref, self.buffer, self.desc, self.build_stats = ref, buffer, desc, stats

    @classmethod
    @torch.no_grad()
    def build(cls, ref):
        who = "NearestIndex.build"
        require_points(ref, "ref", who)
        dev = ref.device
        ref = ref.contiguous()
        R = ref.size(0)
        buffer = torch.empty(int(load().gsr_points_index_bytes(R)), dtype=torch.uint8, device=dev)
        desc, scratch, ms = _PointIndex(), ScratchBlocks(dev), stage_buffer(measure_stages)
        call(dev, "gsr_points_index_build", scratch.cb, None, R, ptr(ref), ptr(buffer), buffer.numel(),
             ctypes.byref(desc), ms, stream(dev))
        return cls(ref, buffer, desc, stage_stats(BUILD_STAGES, ms, scratch, index_bytes=int(buffer.numel())))

    @torch.no_grad()
    def query(self, query, max_dist):
        """query [Q,3] float64 -> (dist [Q] float64, index [Q] int64, stats): the distance to and the position
        in `ref` of the nearest point with distance < max_dist (the lowest position among equally near ones),
        (+inf, -1) beyond."""
        who = "NearestIndex.query"
        require_points(query, "query", who)
        dev = query.device
        if dev != self.ref.device:
            raise RuntimeError(f"{who}: `query` must be on the device of the index")
        query = query.contiguous()
        Q = query.size(0)
        dist = torch.empty(Q, dtype=torch.float64, device=dev)
        index = torch.empty(Q, dtype=torch.int64, device=dev)
        scratch, ms = ScratchBlocks(dev), stage_buffer(measure_stages)
        call(dev, "gsr_points_index_query", scratch.cb, None, ctypes.byref(self.desc), Q, ptr(query),
             float(max_dist), ptr(dist), ptr(index), ms, stream(dev))
        return dist, index, stage_stats(QUERY_STAGES, ms, scratch)


@torch.no_grad()
def icp_accumulate(source, ref, index, means=None):
    """The sums of one ICP pass over the pairs (source[i], ref[index[i]]) with index[i] >= 0: without `means`
    pass 1 -> [8] float64 numpy (n, sum d^2, sum s, sum t); with means [6] (m_s, m_t) pass 2 -> [10]
    (sum (s - m_s)(t - m_t)^T row-major, sum |s - m_s|^2).  -> (sums, stats)."""
    who = "icp_accumulate"
    require_points(source, "source", who)
    require_points(ref, "ref", who)
    require(index, "index", (torch.int64,), 1, who)
    if index.size(0) != source.size(0) or ref.device != source.device or index.device != source.device:
        raise RuntimeError(f"{who}: `index` must have one entry per source point, all on one device")
    dev = source.device
    source, ref, index = source.contiguous(), ref.contiguous(), index.contiguous()
    sums = np.zeros(8 if means is None else 10, dtype=np.float64)
    m = None if means is None else np.ascontiguousarray(np.asarray(means, dtype=np.float64).reshape(6))
    scratch, ms = ScratchBlocks(dev), stage_buffer(measure_stages)
    call(dev, "gsr_icp_accumulate", scratch.cb, None, source.size(0), ptr(source), ref.size(0), ptr(ref), ptr(index),
         1 if m is None else 2, None if m is None else f64ptr(m), f64ptr(sums), ms, stream(dev))
    return sums, stage_stats(ICP_STAGES, ms, scratch)


@torch.no_grad()
def transform_points_(points, transform):
    """points [N,3] float64 <- the 4x4, in place: p' = ((r0 x + r1 y) + r2 z) + t.  -> stats."""
    who = "transform_points_"
    require_points(points, "points", who)
    if not points.is_contiguous():
        raise RuntimeError(f"{who}: `points` must be contiguous (it is changed in place)")
    T = _mat4(transform, who)
    ms = stage_buffer(measure_stages)
    call(points.device, "gsr_points_transform", points.size(0), ptr(points), f64ptr(T), ms, stream(points.device))
    return stage_stats(TRANSFORM_STAGES, ms)


# ---- ICP ---------------------------------------------------------------------------------------------------------

def umeyama_from_sums(n, sum_s, sum_t, H, var_sum):
    """Eigen's umeyama with scaling from gsr_icp_accumulate's sums (H = sum (s - m_s)(t - m_t)^T, var_sum =
    sum |s - m_s|^2): sigma = H^T / n, SVD, S = diag(1, 1, sign(det U det V)), R = U S V^T,
    c = tr(D S) / (var_sum / n), t = m_t - c R m_s.  -> 4x4 float64."""
    ms, mt = np.asarray(sum_s, np.float64) / n, np.asarray(sum_t, np.float64) / n
    U, D, Vt = np.linalg.svd(np.asarray(H, np.float64).reshape(3, 3).T / n)
    S = np.array([1.0, 1.0, 1.0 if np.linalg.det(U) * np.linalg.det(Vt) > 0 else -1.0])
    R = U @ np.diag(S) @ Vt
    c = (D * S).sum() / (var_sum / n)
    T = np.eye(4)
    T[:3, :3] = c * R
    T[:3, 3] = mt - c * (R @ ms)
    return T


@torch.no_grad()
def registration_icp(source, target_index, max_dist, max_iter, relative_fitness=1e-6, relative_rmse=1e-6):
    """open3d's registration_icp with TransformationEstimationPointToPoint(with_scaling=True) from the identity:
    evaluate; up to max_iter times: the update from the current correspondences, T = update T, move the
    source, evaluate again, stop when |d fitness| and |d rmse| are both under their bars.  fitness = n / N,
    rmse = sqrt(sum d^2 / n) (0 when n = 0).  Without a correspondence the loop stops and the current T is
    returned with fitness 0 (open3d leaves this undefined).  source [N,3] float64 is not changed.
    -> dict: T [4,4] numpy, fitness, rmse, iterations, history [(fitness, rmse)], indices (the
    correspondence index tensor of every evaluation), stats."""
    who = "registration_icp"
    require_points(source, "source", who)
    if not isinstance(target_index, NearestIndex):
        raise RuntimeError(f"{who}: `target_index` must be a NearestIndex")
    src = source.contiguous().clone()
    ref = target_index.ref
    N = src.size(0)
    T = np.eye(4)
    ms_iter = []

    def evaluate():
        _, idx, st_q = target_index.query(src, max_dist)
        s1, st_a = icp_accumulate(src, ref, idx)
        n = int(round(s1[0]))
        ms_iter.append((st_q, st_a))
        return idx, s1, (n / N if N else 0.0), (math.sqrt(s1[1] / n) if n else 0.0)

    idx, s1, fit, rmse = evaluate()
    history, indices, it = [(fit, rmse)], [idx], 0
    while it < max_iter and s1[0] > 0:
        n = s1[0]
        s2, _ = icp_accumulate(src, ref, idx, np.concatenate([s1[2:5] / n, s1[5:8] / n]))
        update = umeyama_from_sums(n, s1[2:5], s1[5:8], s2[:9], s2[9])
        T = update @ T
        transform_points_(src, update)
        it += 1
        prev = (fit, rmse)
        idx, s1, fit, rmse = evaluate()
        history.append((fit, rmse))
        indices.append(idx)
        if abs(prev[0] - fit) < relative_fitness and abs(prev[1] - rmse) < relative_rmse:
            break
    return {"T": T, "fitness": fit, "rmse": rmse, "iterations": it, "history": history, "indices": indices,
            "stats": {"evaluations": ms_iter}}


@torch.no_grad()
def crop_and_downsample(points, crop, down_sample_method="voxel", voxel_size=0.01, transform=None):
    """registration.py:113-131: transform, crop, then the voxel grid, or every k-th point once more than
    MAX_POINT_NUMBER are left."""
    _, p, _ = crop_points(points, crop, transform)
    if down_sample_method == "voxel":
        return voxel_down_sample(p, voxel_size)[0]
    if down_sample_method == "uniform" and p.size(0) > MAX_POINT_NUMBER:
        return uniform_down_sample(p, int(round(p.size(0) / float(MAX_POINT_NUMBER)))).contiguous()
    return p


def _registration(source, gt_target, init_T, crop, method, voxel_size, threshold, max_iter):
    init = _mat4(init_T, "registration")
    s = crop_and_downsample(source, crop, method, voxel_size, init)
    t = crop_and_downsample(gt_target, crop, method, voxel_size)
    index = NearestIndex.build(t)  # once per registration, not per iteration
    reg = registration_icp(s, index, threshold, max_iter)
    reg["T"] = reg["T"] @ init
    reg["n_source"], reg["n_target"] = int(s.size(0)), int(t.size(0))
    reg["stats"]["index_build"] = index.build_stats
    return reg


def registration_vol_ds(source, gt_target, init_T, crop, voxel_size, threshold, max_iter):
    """registration.py:166-202: both clouds cropped and voxel-averaged at voxel_size, then ICP at `threshold`."""
    return _registration(source, gt_target, init_T, crop, "voxel", voxel_size, threshold, max_iter)


def registration_unif(source, gt_target, init_T, crop, threshold, max_iter):
    """registration.py:134-163: both clouds cropped and thinned uniformly to about MAX_POINT_NUMBER."""
    return _registration(source, gt_target, init_T, crop, "uniform", 0.01, threshold, max_iter)


# ---- histogram and F-score ---------------------------------------------------------------------------------------

def f1_score_histo(tau, plot_stretch, d1, d2):
    """get_f1_score_histo2 (evaluation.py:173-215) over device distances d1 (precision side) and d2 (recall
    side): the counts by torch, the bin edges by numpy's own arange, the last bin closed on the right as
    np.histogram's.  -> dict precision, recall, fscore, n_precise, n_recalled, edges_*, cum_*."""
    if d1.numel() == 0 or d2.numel() == 0:
        z = np.array([0])
        return {"precision": 0, "recall": 0, "fscore": 0, "n_precise": 0, "n_recalled": 0, "edges_source": z,
                "cum_source": z, "edges_target": z, "cum_target": z}
    edges_np = np.arange(0, tau * plot_stretch, tau / 100)
    edges = torch.as_tensor(edges_np, device=d1.device)
    nb = edges_np.shape[0] - 1

    def side(d):
        k = torch.searchsorted(edges, d.contiguous(), right=True) - 1
        k = torch.where(d == edges[-1], torch.full_like(k, nb - 1), k)
        ok = (k >= 0) & (k < nb)
        hist = torch.bincount(k[ok], minlength=nb)
        return int((d < tau).sum()), hist.cpu().numpy()

    (n1, h1), (n2, h2) = side(d1), side(d2)
    recall, precision = float(n2) / float(d2.numel()), float(n1) / float(d1.numel())
    with np.errstate(all="ignore"):
        fscore = float(np.float64(2 * recall * precision) / np.float64(recall + precision))
    return {"precision": precision, "recall": recall, "fscore": fscore, "n_precise": n1, "n_recalled": n2,
            "edges_source": edges_np, "cum_source": np.cumsum(h1).astype(float) / d1.numel(),
            "edges_target": edges_np, "cum_target": np.cumsum(h2).astype(float) / d2.numel()}


@torch.no_grad()
def evaluate_histo(source, target, T, crop, voxel, tau, plot_stretch=5):
    """EvaluateHisto (evaluation.py:60-170) without the normals and the coloured .ply files: the source moved
    by T, both clouds cropped and voxel-averaged at `voxel`, the nearest distance each way (every point gets
    one: the bound covers the joint box), then f1_score_histo.  -> its dict, plus n_source, n_target,
    dist_source, dist_target, stats."""
    s = crop_and_downsample(source, crop, "voxel", voxel, _mat4(T, "evaluate_histo"))
    t = crop_and_downsample(target, crop, "voxel", voxel)
    stats = {}
    if s.size(0) and t.size(0):
        both = torch.cat([s, t])
        bound = 2.0 * float((both.amax(0) - both.amin(0)).norm()) + 1.0
        ti, si = NearestIndex.build(t), NearestIndex.build(s)
        d1, _, stats["query_source"] = ti.query(s, bound)
        d2, _, stats["query_target"] = si.query(t, bound)
        stats["build_target"], stats["build_source"] = ti.build_stats, si.build_stats
    else:
        d1 = d2 = torch.empty(0, dtype=torch.float64, device=source.device)
    out = f1_score_histo(tau, plot_stretch, d1, d2)
    out.update(n_source=int(s.size(0)), n_target=int(t.size(0)), dist_source=d1, dist_target=d2, stats=stats)
    return out


@torch.no_grad()
def tnt_fscore(vertices, faces, gt_points, crop, init_T, tau):
    """run.py:93-187: the evaluated cloud is the mesh's vertices followed by its face centroids ((a + b) + c) /
    3; three registrations refine init_T (voxel tau at threshold 80 tau, voxel tau / 2 at 20 tau, uniform at
    2 tau, 20 iterations each); then evaluate_histo at voxel tau / 2, threshold tau.  vertices [V,3] float32 /
    float64, faces [F,3] int32 / int64, gt_points [G,3] float32 / float64.  -> dict: dTau, precision, recall,
    fscore (what metrics.json holds), the curves, counts, transformation, registrations, stats."""
    who = "tnt_fscore"
    require(vertices, "vertices", (torch.float32, torch.float64), 2, who)
    require(faces, "faces", (torch.int32, torch.int64), 2, who)
    require(gt_points, "gt_points", (torch.float32, torch.float64), 2, who)
    if vertices.size(1) != 3 or faces.size(1) != 3 or gt_points.size(1) != 3:
        raise RuntimeError(f"{who}: `vertices`, `faces` and `gt_points` must have shapes (V, 3), (F, 3), (G, 3)")
    v, f = vertices.to(torch.float64), faces.long()
    pcd = torch.cat([v, ((v[f[:, 0]] + v[f[:, 1]]) + v[f[:, 2]]) / 3.0]).contiguous()
    gt = gt_points.to(torch.float64).contiguous()
    r2 = registration_vol_ds(pcd, gt, init_T, crop, tau, tau * 80, 20)
    r3 = registration_vol_ds(pcd, gt, r2["T"], crop, tau / 2.0, tau * 20, 20)
    r = registration_unif(pcd, gt, r3["T"], crop, 2 * tau, 20)
    out = evaluate_histo(pcd, gt, r["T"], crop, tau / 2.0, tau)
    out.update(dTau=tau, transformation=r["T"], registrations=(r2, r3, r))
    return out


# ---- mesh culling (cull_mesh.py) ---------------------------------------------------------------------------------

def _w2c_rows(w2c, who, batched):
    """World -> camera matrices, 4x4 or 3x4, as contiguous float32 [n,3,4] on the host."""
    m = np.asarray(w2c.detach().cpu().numpy() if isinstance(w2c, torch.Tensor) else w2c, dtype=np.float64)
    if not batched:
        m = m[None]
    if m.ndim != 3 or m.shape[1:] not in ((4, 4), (3, 4)):
        raise RuntimeError(f"{who}: a camera matrix must have shape (4, 4) or (3, 4) (got {m.shape[1:]})")
    return np.ascontiguousarray(m[:, :3, :].astype(np.float32))


def _mesh_args(vertices, faces, who):
    require(vertices, "vertices", (torch.float32, torch.float64), 2, who)
    require(faces, "faces", (torch.int32, torch.int64), 2, who)
    if vertices.size(1) != 3 or faces.size(1) != 3 or faces.device != vertices.device:
        raise RuntimeError(f"{who}: `vertices` and `faces` must have shapes (V, 3) and (F, 3) on one device")
    return vertices.to(torch.float32).contiguous(), faces.contiguous()


@torch.no_grad()
def render_mesh_depth(vertices, faces, w2c, H, W, fx, fy, cx, cy, znear=0.01, zfar=20.0, count=False):
    """The depth map of a triangle mesh from one OpenCV pinhole camera (x right, y down, z forward; w2c 4x4 or
    3x4 world -> camera): depth [H,W] float32 = the smallest camera-space z in [znear, zfar] under each pixel
    centre (j + 0.5, i + 0.5), 0 where no triangle lies.  Both facings count.  vertices [V,3] float32 / float64
    (rendered as float32), faces [F,3] int32 / int64.  -> (depth, stats); stats["counters"] with `count`."""
    who = "render_mesh_depth"
    v, f = _mesh_args(vertices, faces, who)
    dev = v.device
    m = _w2c_rows(w2c, who, False)
    depth = torch.empty(int(H), int(W), dtype=torch.float32, device=dev)
    scratch, ms = ScratchBlocks(dev), stage_buffer(measure_stages)
    ctr = (ctypes.c_ulonglong * 4)() if count else None
    call(dev, "gsr_mesh_depth", scratch.cb, None, v.size(0), ptr(v), f.size(0), ptr(f),
         1 if f.dtype == torch.int64 else 0, f32ptr(m), int(H), int(W), fx, fy, cx, cy, znear, zfar, ptr(depth), ctr,
         ms, stream(dev))
    return depth, stage_stats(RASTER_STAGES, ms, scratch,
                              counters=None if ctr is None else dict(zip(RASTER_COUNTERS, ctr)))


@torch.no_grad()
def mesh_view_votes(vertices, faces, w2cs, H, W, fx, fy, cx, cy, znear=0.01, zfar=20.0, eps=0.005, count=False):
    """cull_mesh.py's point_masks over depth maps rendered here: counts [V] int32 = the number of the views
    w2cs [n,4,4] / [n,3,4] in which the vertex is inside the frustum (0 <= u <= W - 1, 0 <= v <= H - 1, z > 0)
    and not more than eps behind the view's depth map, sampled bilinearly at (u, v).  One depth buffer serves
    every view and nothing but the counts leaves the device.  -> (counts, stats)."""
    who = "mesh_view_votes"
    v, f = _mesh_args(vertices, faces, who)
    dev = v.device
    m = _w2c_rows(w2cs, who, True)
    counts = torch.empty(v.size(0), dtype=torch.int32, device=dev)
    scratch, ms = ScratchBlocks(dev), stage_buffer(measure_stages)
    ctr = (ctypes.c_ulonglong * 4)() if count else None
    call(dev, "gsr_mesh_view_votes", scratch.cb, None, v.size(0), ptr(v), f.size(0), ptr(f),
         1 if f.dtype == torch.int64 else 0, m.shape[0], f32ptr(m), int(H), int(W), fx, fy, cx, cy, znear, zfar, eps,
         ptr(counts), ctr, ms, stream(dev))
    return counts, stage_stats(RASTER_STAGES, ms, scratch,
                               counters=None if ctr is None else dict(zip(RASTER_COUNTERS, ctr)))


def read_cull_trajectory(path):
    """Camera-to-world poses for cull_mesh: a .log trajectory (read_trajectory) or an .npy of [n,4,4] / [n,3,4]
    matrices -> [n,4,4] float64."""
    if str(path).endswith(".npy"):
        m = np.asarray(np.load(path), dtype=np.float64)
        if m.ndim != 3 or m.shape[1:] not in ((4, 4), (3, 4)):
            raise RuntimeError(f"read_cull_trajectory: {path}: expected [n,4,4] or [n,3,4] (got {m.shape})")
        out = np.tile(np.eye(4), (m.shape[0], 1, 1))
        out[:, :m.shape[1], :] = m
        return out
    if str(path).endswith(".log"):
        return read_trajectory(path)[1]
    raise RuntimeError(f"read_cull_trajectory: {path}: a .log or .npy trajectory (the .json branch is not built)")


@torch.no_grad()
def cull_mesh(vertices, faces, c2ws, H=1080, W=1920, fx=1163.8678928442187, fy=1172.793101201448,
              cx=962.3120628412543, cy=542.0667209577691, far=20.0, min_views=20, eps=0.005):
    """cull_mesh.py: keep the vertices that at least `min_views` of the cameras c2ws [n,4,4] / [n,3,4] (camera
    -> world, inverted here in float64) see, the faces whose three corners are kept, and of the kept vertices
    those a kept face names; the surviving order is preserved.  The defaults are the reference's TnT
    intrinsics.  -> (vertices', faces' int64)."""
    who = "cull_mesh"
    _mesh_args(vertices, faces, who)
    c = np.asarray(c2ws.detach().cpu().numpy() if isinstance(c2ws, torch.Tensor) else c2ws, dtype=np.float64)
    if c.ndim != 3 or c.shape[1:] not in ((4, 4), (3, 4)):
        raise RuntimeError(f"{who}: `c2ws` must have shape (n, 4, 4) or (n, 3, 4) (got {c.shape})")
    full = np.tile(np.eye(4), (c.shape[0], 1, 1))
    full[:, :c.shape[1], :] = c
    w2cs = np.linalg.inv(full) if c.shape[0] else full
    counts, _ = mesh_view_votes(vertices, faces, w2cs, H, W, fx, fy, cx, cy, 0.01, far, eps)
    keep_v = counts >= int(min_views)
    f = faces.long()
    keep_f = keep_v[f[:, 0]] & keep_v[f[:, 1]] & keep_v[f[:, 2]]
    f = f[keep_f]
    used = torch.zeros(vertices.size(0), dtype=torch.bool, device=vertices.device)
    used[f.reshape(-1)] = True
    remap = torch.cumsum(used.to(torch.int64), 0) - 1
    return vertices[used], remap[f]


# ---- trajectory alignment (host) ---------------------------------------------------------------------------------

def _umeyama_points(src, dst):
    n = src.shape[0]
    ms, mt = src.sum(0) / n, dst.sum(0) / n
    a, b = src - ms, dst - mt
    return umeyama_from_sums(n, src.sum(0), dst.sum(0), a.T @ b, (a * a).sum())


def trajectory_alignment(est_centers, gt_centers, gt_trans, generator, max_iteration=100000, max_distance=0.2,
                         ransac_n=6):
    """registration.py:66-110 on the host in numpy float64: camera centres est [n,3] onto gt [n,3] (moved by
    the 4x4 gt_trans first, when given), paired index to index.  A seeded RANSAC: `ransac_n` pairs drawn by
    `generator` (a numpy Generator), Umeyama with scale, inliers closer than `max_distance`, the best sample
    by inlier count and then by inlier rmse, and a last estimate from its inliers.  open3d draws from a
    generator of its own, so its samples (and a result to the last digit) cannot be reproduced; the rule can.
    The loop stops early once a sample has every pair as an inlier.  -> 4x4 float64."""
    est = np.asarray(est_centers, np.float64).reshape(-1, 3)
    gt = np.asarray(gt_centers, np.float64).reshape(-1, 3)
    if est.shape != gt.shape or est.shape[0] < ransac_n:
        raise RuntimeError(f"trajectory_alignment: two [n, 3] sets of at least {ransac_n} centres "
                           f"(got {est.shape}, {gt.shape})")
    if gt_trans is not None:
        G = np.asarray(gt_trans, np.float64).reshape(4, 4)
        gt = gt @ G[:3, :3].T + G[:3, 3]
    n = est.shape[0]
    best, best_in = (-1, np.inf), None
    for _ in range(int(max_iteration)):
        pick = generator.choice(n, size=ransac_n, replace=False)
        with np.errstate(all="ignore"):
            T = _umeyama_points(est[pick], gt[pick])
            d = np.linalg.norm(est @ T[:3, :3].T + T[:3, 3] - gt, axis=1)
        inl = d < max_distance
        k = int(inl.sum())
        if k == 0:
            continue
        rmse = float(np.sqrt((d[inl] ** 2).sum() / k))
        if k > best[0] or (k == best[0] and rmse < best[1]):
            best, best_in = (k, rmse), inl
        if k == n:
            break
    if best_in is None or best[0] < 3:
        raise RuntimeError("trajectory_alignment: no sample had three inliers")
    return _umeyama_points(est[best_in], gt[best_in])
