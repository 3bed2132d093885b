"""DTU Chamfer evaluation on the device (the reference's evaluate_dtu_mesh.py
and dtu_eval/eval.py --mode mesh) over the C ABI: mesh sampling, greedy radius
thinning and the bounded nearest-point distance in HIP (gsr_mesh_sample_points,
gsr_points_downsample, gsr_points_nearest; csrc/pointeval.hip), the masking in
between as torch gathers.  All geometry is float64, as in the reference.

    scale, R, t = align_to_dtu(cam_centers, gt_centers)
    vertices = apply_alignment(vertices, scale, R, t)           # recon_post.ply -> the DTU frame
    out = dtu_chamfer(vertices, faces, stl_points, obs_mask, bb, res, plane)
    out["mean_d2s"], out["mean_s2d"], out["overall"]

Device tensors on the current stream; there is no CPU path.
"""
from __future__ import annotations

import ctypes

import numpy as np
import torch

from diff_gaussian_rasterization._abi import (Out, ScratchBlocks, call, ptr, record_stats, require, require_points,
                                              stage_buffer, stream)

SAMPLE_STAGES = ("count", "scan", "emit")
THIN_STAGES = ("bounds", "sort", "rounds", "scan", "write")
NEAREST_STAGES = ("bounds", "ref_sort", "query_sort", "search")
# measurement hook (tools/bench_dtu_eval.py): when a dict, every call leaves its per-stage GPU
# milliseconds and scratch bytes here (the timed call synchronises; leave None otherwise)
last_call_stats = None


@torch.no_grad()
def sample_mesh_points(vertices, faces, density=0.2):
    """eval.py:48-71 on the device: vertices [V,3] float32 / float64 (widened
    first), faces [F,3] int32 / int64 -> points [V+S,3] float64: the vertices,
    then per triangle with a non-zero area, in triangle order, the lattice
    points of sample_single_tri (i outer, j inner)."""
    who = "sample_mesh_points"
    require(vertices, "vertices", (torch.float32, torch.float64), 2, who)
    require(faces, "faces", (torch.int32, torch.int64), 2, who)
    if vertices.size(1) != 3 or faces.size(1) != 3:
        raise RuntimeError(f"{who}: `vertices` and `faces` must have shapes (V, 3) and (F, 3) "
                           f"(got {tuple(vertices.shape)}, {tuple(faces.shape)})")
    if vertices.device != faces.device:
        raise RuntimeError(f"{who}: `vertices` and `faces` must be on one device")
    dev = vertices.device
    vertices, faces = vertices.to(torch.float64).contiguous(), faces.contiguous()
    V, F = vertices.size(0), faces.size(0)
    out, scratch = Out(dev, torch.float64), ScratchBlocks(dev)
    n = ctypes.c_longlong(0)
    ms = stage_buffer(last_call_stats is not None)
    call(dev, "gsr_mesh_sample_points", out.cb, None, scratch.cb, None, V, F, ptr(vertices), ptr(faces),
         int(faces.dtype == torch.int64), float(density), ctypes.byref(n), ms, stream(dev))
    record_stats(last_call_stats, SAMPLE_STAGES, ms, scratch)
    return out.tensor[:3 * n.value].view(-1, 3)


@torch.no_grad()
def downsample_points(points, radius, perm=None, generator=None):
    """eval.py:80-94 on the device: points [N,3] float64 are shuffled (by
    `perm` [N] int64 when given, else torch.randperm on the device with
    `generator`), then a point survives iff no earlier surviving point lies
    within `radius` (dx^2 + dy^2 + dz^2 <= radius^2; duplicates count).
    -> (kept_points [M,3] float64 in shuffled order, kept_index [M] int64 into
    the un-shuffled input)."""
    who = "downsample_points"
    require_points(points, "points", who)
    dev = points.device
    N = points.size(0)
    if perm is None:
        perm = torch.randperm(N, device=dev, generator=generator)
    else:
        require(perm, "perm", (torch.int64,), 1, who)
        if perm.size(0) != N or perm.device != dev:
            raise RuntimeError(f"{who}: `perm` must have {N} entries on the device of `points`")
    shuffled = points[perm].contiguous()
    kept, scratch = Out(dev, torch.int64), ScratchBlocks(dev)
    M, rounds = ctypes.c_longlong(0), ctypes.c_longlong(0)
    ms = stage_buffer(last_call_stats is not None)
    call(dev, "gsr_points_downsample", kept.cb, None, scratch.cb, None, N, ptr(shuffled), float(radius),
         ctypes.byref(M), ctypes.byref(rounds), ms, stream(dev))
    record_stats(last_call_stats, THIN_STAGES, ms, scratch, num_rounds=int(rounds.value))
    ranks = kept.tensor[:M.value]
    return shuffled[ranks], perm[ranks]


@torch.no_grad()
def nearest_distance(query, ref, max_dist):
    """query [Q,3], ref [R,3] float64 -> dist [Q] float64: the Euclidean
    distance to the nearest ref point where that is < max_dist, +inf
    otherwise (eval.py:119-122, 132-134 discard everything >= max_dist)."""
    who = "nearest_distance"
    require_points(query, "query", who)
    require_points(ref, "ref", who)
    if query.device != ref.device:
        raise RuntimeError(f"{who}: `query` and `ref` must be on one device")
    dev = query.device
    query, ref = query.contiguous(), ref.contiguous()
    Q, R = query.size(0), ref.size(0)
    dist = torch.empty(Q, dtype=torch.float64, device=dev)
    scratch = ScratchBlocks(dev)
    ms = stage_buffer(last_call_stats is not None)
    call(dev, "gsr_points_nearest", scratch.cb, None, Q, ptr(query), R, ptr(ref), float(max_dist), ptr(dist), ms,
         stream(dev))
    record_stats(last_call_stats, NEAREST_STAGES, ms, scratch)
    return dist


@torch.no_grad()
def dtu_chamfer(vertices, faces, stl_points, obs_mask, bb, res, plane, *, density=0.2, patch_size=60, max_dist=20,
                perm=None, generator=None):
    """eval.py:43-134, 157-166 (--mode mesh) on the device.  vertices / faces:
    the aligned mesh; stl_points [S,3]: the scanner's cloud; obs_mask [X,Y,Z]
    bool / uint8, bb [2,3], res: ObsMask*.mat's ObsMask, BB and Res; plane [4]:
    Plane*.mat's P.  -> dict: mean_d2s, mean_s2d, overall (floats; the mean
    over an empty set is nan), n_sampled, n_down, n_in, n_in_obs, n_stl_above,
    dist_d2s [n_in_obs], dist_s2d [n_stl_above] (+inf where >= max_dist)."""
    who = "dtu_chamfer"
    require(stl_points, "stl_points", (torch.float32, torch.float64), 2, who)
    require(obs_mask, "obs_mask", (torch.bool, torch.uint8), 3, who)
    if stl_points.size(1) != 3:
        raise RuntimeError(f"{who}: `stl_points` must have shape (S, 3) (got {tuple(stl_points.shape)})")
    dev = stl_points.device
    f64 = dict(dtype=torch.float64, device=dev)
    # BB is rounded to float32 before use (eval.py:100); Res and the plane are float64
    bb32 = np.asarray(torch.as_tensor(bb).cpu().numpy(), dtype=np.float32)
    if bb32.shape != (2, 3):
        raise RuntimeError(f"{who}: `bb` must have shape (2, 3) (got {bb32.shape})")
    patch = np.float32(patch_size)
    # the bounds are float32 sums, as numpy's float32 array +- a Python float (eval.py:103)
    lower = torch.as_tensor((bb32[:1] - patch).astype(np.float64), **f64)
    upper = torch.as_tensor((bb32[1:] + patch * np.float32(2)).astype(np.float64), **f64)
    bb = torch.as_tensor(bb32.astype(np.float64), **f64)
    plane = torch.as_tensor(np.asarray(torch.as_tensor(plane).cpu().numpy(), dtype=np.float64).reshape(4), **f64)
    res = float(np.asarray(torch.as_tensor(res).cpu().numpy(), dtype=np.float64).reshape(-1)[0])

    sampled = sample_mesh_points(vertices, faces, density)
    down, _ = downsample_points(sampled, density, perm=perm, generator=generator)
    inbound = ((down >= lower) & (down < upper)).all(dim=1)
    data_in = down[inbound]
    # np.around and torch.round both round half to even
    grid = torch.round((data_in - bb[:1]) / res).to(torch.int32)
    shape = torch.tensor(list(obs_mask.shape), dtype=torch.int32, device=dev)
    grid_in = ((grid >= 0) & (grid < shape)).all(dim=1)
    g = grid[grid_in].long()
    in_obs = obs_mask[g[:, 0], g[:, 1], g[:, 2]].bool()
    data_in_obs = data_in[grid_in][in_obs]

    stl = stl_points.to(torch.float64)
    above = (plane[None] * torch.cat([stl, torch.ones_like(stl[:, :1])], -1)).sum(-1) > 0
    stl_above = stl[above]
    dist_d2s = nearest_distance(data_in_obs, stl, max_dist)
    dist_s2d = nearest_distance(stl_above, data_in, max_dist)  # data_in, not data_in_obs (eval.py:132)

    def _sum_count(d):
        ok = torch.isfinite(d)
        return torch.stack([torch.where(ok, d, torch.zeros_like(d)).sum(), ok.sum().to(torch.float64)])

    s = torch.cat([_sum_count(dist_d2s), _sum_count(dist_s2d)]).cpu().tolist()  # the one readback of the means
    mean_d2s = s[0] / s[1] if s[1] > 0 else float("nan")
    mean_s2d = s[2] / s[3] if s[3] > 0 else float("nan")
    return {"mean_d2s": mean_d2s, "mean_s2d": mean_s2d, "overall": (mean_d2s + mean_s2d) / 2,
            "n_sampled": int(sampled.size(0)), "n_down": int(down.size(0)), "n_in": int(data_in.size(0)),
            "n_in_obs": int(data_in_obs.size(0)), "n_stl_above": int(stl_above.size(0)),
            "dist_d2s": dist_d2s, "dist_s2d": dist_s2d}


def align_to_dtu(cam_centers, gt_centers):
    """evaluate_dtu_mesh.py:17-58, 158-163 on the host in float64: the scale
    that equalises the mean distance to the centroid, then the least-squares
    rotation (SVD, with the reflection fix) and translation that take the
    scaled camera centres [N,3] onto DTU's [N,3].  -> (scale, R [3,3], t [3])."""
    A = np.asarray(torch.as_tensor(cam_centers).detach().cpu().numpy(), dtype=np.float64)
    B = np.asarray(torch.as_tensor(gt_centers).detach().cpu().numpy(), dtype=np.float64)
    if A.ndim != 2 or A.shape[1] != 3 or A.shape != B.shape or A.shape[0] < 1:
        raise RuntimeError(f"align_to_dtu: two [N, 3] sets of centres (got {A.shape}, {B.shape})")
    scale_a = np.linalg.norm(A - A.mean(axis=0), axis=1).mean()
    scale_b = np.linalg.norm(B - B.mean(axis=0), axis=1).mean()
    A = A * scale_b / scale_a
    ca, cb = np.mean(A, axis=0), np.mean(B, axis=0)
    U, _, Vt = np.linalg.svd(np.dot((A - ca).T, B - cb))
    R = np.dot(Vt.T, U.T)
    if np.linalg.det(R) < 0:
        Vt[2, :] *= -1
        R = np.dot(Vt.T, U.T)
    t = cb.T - np.dot(R, ca.T)
    return float(scale_b / scale_a), R, t


def apply_alignment(vertices, scale, R, t):
    """evaluate_dtu_mesh.py:172-173: vertices * scale @ R.T + t, in float64
    (a tensor stays on its device)."""
    v = torch.as_tensor(vertices).to(torch.float64)
    R = torch.as_tensor(np.asarray(R, dtype=np.float64), device=v.device)
    t = torch.as_tensor(np.asarray(t, dtype=np.float64), device=v.device)
    return (v * float(scale)) @ R.T + t
