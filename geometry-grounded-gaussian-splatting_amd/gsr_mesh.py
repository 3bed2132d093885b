"""Tetrahedral mesh extraction (mesh_extract_tetrahedra.py:18-179 and
utils/tetmesh.py of the reference) over the C ABI: marching tetrahedra in HIP
(gsr_marching_tetrahedra, csrc/tetmesh.hip), the driver around
gaussian_renderer.integrate (with sweep="hip" its per-view glue and its
bisection step are the three kernels of csrc/fieldsweep.hip), and the mesh
clean-up (gsr_mesh_clusters and gsr_mesh_filter, csrc/meshclean.hip).

    points = gsr_scene.tetra_points(inp); scale = gsr_scene.tetra_points_scale(inp)
    cells = <the caller's Delaunay triangulation of points, [T, 4]>
    vertices, faces = extract_mesh(points, scale, cells, views, pc, pipe, kernel_size)
    write_ply("recon.ply", vertices, faces)
    write_ply("recon_post.ply", *post_process_mesh(vertices, faces, cluster_to_keep=1))

and the TSDF path of the DTU script (mesh_extract.py:40-89; gsr_tsdf, csrc/tsdf.hip):

    vertices, faces, colors = extract_mesh_tsdf(views, pc, pipe, background, kernel_size)
    write_ply("recon.ply", vertices, faces, colors)

Face order: a tet's one or two triangles sit next to each other, in tet
order.  The reference lists, chunk by chunk, the one-triangle tets before the
two-triangle tets; the mesh is the same set of oriented triangles.
"""
from __future__ import annotations

import ctypes

import numpy as np
import torch

from diff_gaussian_rasterization._abi import (Out, ScratchBlocks, call, f32ptr, ptr, record_stats, require,
                                              require_mesh, stage_buffer, stream)

STAGES = ("flags", "count", "emit", "sort", "ranks", "edges", "faces")
# measurement hook (tools/bench_tetmesh.py): when a dict, every call leaves its per-stage GPU
# milliseconds and scratch bytes here (the timed call synchronises; leave None otherwise)
last_call_stats = None


@torch.no_grad()
def marching_tetrahedra_ids(tets, sdf, valid):
    """The unbatched kernel call: tets [T,4] int32 / int64, sdf [V] float32,
    valid [V] bool / uint8, all on one HIP device -> (edge_ids [E,2] int64,
    faces [F,3] int64).  Runs on the current stream."""
    who = "marching_tetrahedra"
    require(tets, "tets", (torch.int32, torch.int64), 2, who)
    require(sdf, "sdf", (torch.float32,), 1, who)
    require(valid, "valids", (torch.bool, torch.uint8), 1, who)
    if tets.size(1) != 4:
        raise RuntimeError(f"marching_tetrahedra: `tets` must have shape (T, 4) (got {tuple(tets.shape)})")
    if valid.size(0) != sdf.size(0):
        raise RuntimeError("marching_tetrahedra: `sdf` and `valids` must have the same length")
    if sdf.device != tets.device or valid.device != tets.device:
        raise RuntimeError("marching_tetrahedra: inputs must be on one device")
    dev = tets.device
    tets, sdf = tets.contiguous(), sdf.contiguous()
    valid = valid.contiguous().view(torch.uint8)
    T, V = tets.size(0), sdf.size(0)
    edges, faces, scratch = Out(dev, torch.int64), Out(dev, torch.int64), ScratchBlocks(dev)
    E, F = ctypes.c_longlong(0), ctypes.c_longlong(0)
    ms = stage_buffer(last_call_stats is not None)
    call(dev, "gsr_marching_tetrahedra", edges.cb, None, faces.cb, None, scratch.cb, None, T, V, ptr(tets),
         int(tets.dtype == torch.int64), ptr(sdf), ptr(valid), ctypes.byref(E), ctypes.byref(F), ms, stream(dev))
    record_stats(last_call_stats, STAGES, ms, scratch)
    if E.value == 0:
        return (torch.zeros(0, 2, dtype=torch.int64, device=dev), torch.zeros(0, 3, dtype=torch.int64, device=dev))
    return edges.tensor[:2 * E.value].view(-1, 2), faces.tensor[:3 * F.value].view(-1, 3)


CLEAN_STAGES = ("keys", "sort", "union", "flatten", "ids", "counts", "area")


@torch.no_grad()
def cluster_connected_triangles(vertices, faces, num_vertices=None):
    """open3d's TriangleMesh.cluster_connected_triangles on the device
    (gsr_mesh_clusters, csrc/meshclean.hip): vertices [V,3] float32 or None,
    faces [F,3] int32 / int64 -> (triangle_clusters [F] int64,
    cluster_n_triangles [C] int64, cluster_area [C] float64, None without
    vertices).  Triangles are connected through shared undirected edges;
    clusters are numbered by their lowest triangle index.  Without vertices,
    `num_vertices` bounds the ids (default: 2^31, which costs the edge sort its
    widest keys).  One host readback (C).  Runs on the current stream."""
    who = "cluster_connected_triangles"
    require_mesh(vertices, faces, who, vertices_optional=True)
    dev = faces.device
    F = faces.size(0)
    V = vertices.size(0) if vertices is not None else (1 << 31 if num_vertices is None else int(num_vertices))
    labels = torch.empty(F, dtype=torch.int64, device=dev)
    counts, areas, scratch = Out(dev, torch.int64), Out(dev, torch.float64), ScratchBlocks(dev)
    if F == 0:
        return labels, counts.tensor, (areas.tensor if vertices is not None else None)
    faces = faces.contiguous()
    vertices = vertices.contiguous() if vertices is not None else None
    C = ctypes.c_longlong(0)
    ms = stage_buffer(last_call_stats is not None)
    call(dev, "gsr_mesh_clusters", counts.cb, None, areas.cb, None, scratch.cb, None, F, V, ptr(faces),
         int(faces.dtype == torch.int64), ptr(vertices), ptr(labels), ctypes.byref(C), ms, stream(dev))
    record_stats(last_call_stats, CLEAN_STAGES, ms, scratch)
    return labels, counts.tensor[:C.value], (areas.tensor[:C.value] if vertices is not None else None)


@torch.no_grad()
def post_process_mesh(vertices, faces, cluster_to_keep=1, min_triangles=50):
    """mesh_extract_tetrahedra.py:18-40 post_process_mesh on the device:
    keeps the clusters of connected triangles with at least
    max(sorted(cluster_n_triangles)[-cluster_to_keep], min_triangles)
    triangles (ties at the threshold all stay), then drops the unreferenced
    vertices, then the triangles with two equal vertex ids.  vertices [V,3]
    float32, faces [F,3] int32 / int64 -> (vertices [V',3] float32, faces
    [F',3] int64), order and winding kept.  The threshold never leaves the
    device; the host reads three sizes (C, then V' and F' together)."""
    who = "post_process_mesh"
    require_mesh(vertices, faces, who)
    if isinstance(cluster_to_keep, bool) or not isinstance(cluster_to_keep, int) or cluster_to_keep < 1:
        raise ValueError(f"{who}: `cluster_to_keep` must be an integer >= 1 (got {cluster_to_keep!r})")
    dev = faces.device
    F, V = faces.size(0), vertices.size(0)
    if F == 0:
        return (torch.zeros(0, 3, dtype=torch.float32, device=dev), torch.zeros(0, 3, dtype=torch.int64, device=dev))
    faces, vertices = faces.contiguous(), vertices.contiguous()
    labels, counts, _ = cluster_connected_triangles(None, faces, num_vertices=V)
    C = counts.size(0)
    if cluster_to_keep > C:
        raise ValueError(f"{who}: `cluster_to_keep` = {cluster_to_keep} but the mesh has {C} clusters")
    n_min = torch.sort(counts).values[C - cluster_to_keep].clamp(min=int(min_triangles)).reshape(1).contiguous()
    vout, fout, scratch = Out(dev, torch.float32), Out(dev, torch.int64), ScratchBlocks(dev)
    Vn, Fn = ctypes.c_longlong(0), ctypes.c_longlong(0)
    call(dev, "gsr_mesh_filter", vout.cb, None, fout.cb, None, scratch.cb, None, F, V, C, ptr(vertices), ptr(faces),
         int(faces.dtype == torch.int64), ptr(labels), ptr(counts), ptr(n_min), ctypes.byref(Vn), ctypes.byref(Fn),
         stream(dev))
    return vout.tensor[:3 * Vn.value].view(-1, 3), fout.tensor[:3 * Fn.value].view(-1, 3)


def _unbatched(vertices, tets, sdf, scales, valids):
    ids, faces = marching_tetrahedra_ids(tets, sdf, valids)
    flat = ids.reshape(-1)
    return ((vertices[flat].reshape(-1, 2, 3), sdf[flat].reshape(-1, 2, 1)), scales[flat].reshape(-1, 2, 1), faces,
            ids)


@torch.no_grad()
def marching_tetrahedra(vertices, tets, sdf, scales, valids):
    """utils/tetmesh.py:190-242 marching_tetrahedra: vertices [B,V,3], tets
    [T,4], sdf [B,V], scales [B,V,1], valids [B,V] -> four lists over the
    batch: (edges_to_interp [E,2,3], edges_to_interp_sdf [E,2,1]),
    merged_scales [E,2,1], faces [F,3], merged_verts_ids [E,2]."""
    for t, name in ((vertices, "vertices"), (tets, "tets"), (sdf, "sdf"), (scales, "scales"), (valids, "valids")):
        if not isinstance(t, torch.Tensor) or not t.is_cuda:
            raise RuntimeError(f"marching_tetrahedra: `{name}` must be a HIP device tensor")
    if vertices.dim() != 3 or vertices.size(2) != 3:
        raise RuntimeError(f"marching_tetrahedra: `vertices` must have shape (B, V, 3) (got {tuple(vertices.shape)})")
    B, V = vertices.size(0), vertices.size(1)
    if tuple(sdf.shape) != (B, V) or tuple(valids.shape) != (B, V):
        raise RuntimeError("marching_tetrahedra: `sdf` and `valids` must have shape (B, V)")
    if tuple(scales.shape) != (B, V, 1):
        raise RuntimeError(f"marching_tetrahedra: `scales` must have shape (B, V, 1) (got {tuple(scales.shape)})")
    outs = [_unbatched(vertices[b], tets, sdf[b], scales[b], valids[b]) for b in range(B)]
    return list(zip(*outs))


def _view_mask(view, points, inside):
    """mesh_extract_tetrahedra.py:44-61: the points whose projection falls on the view's gt_mask."""
    mask = getattr(view, "gt_mask", None)
    if mask is None:
        return inside
    cam = points @ view.R.to(points) + view.T.to(points)
    uv = cam[:, :2] / cam[:, 2:]
    W, H = view.image_width, view.image_height
    uv = torch.addcmul(uv.new_tensor([(view.Cx * 2.0 + 1.0) / W - 1.0, (view.Cy * 2.0 + 1.0) / H - 1.0]),
                       uv.new_tensor([view.Fx * 2.0 / W, view.Fy * 2.0 / H]), uv)
    sampled = torch.nn.functional.grid_sample(mask[None].to(points), uv[None, None], align_corners=True)
    return (sampled.squeeze() > 0.5) & inside


def _check_sweep(sweep, who):
    if sweep not in ("torch", "hip"):
        raise ValueError(f"{who}: `sweep` must be \"torch\" or \"hip\" (got {sweep!r})")


def _sweep_views(views, device):
    """What gsr_field_view_update (csrc/fieldsweep.hip) takes of every view, read and uploaded once per
    sweep rather than per chunk: [(view, None)] without a gt_mask, else (view, (R [9] and T [3] host
    float32, Fx, Fy, Cx, Cy, W, H, the mask plane [H,W] float32 on `device`))."""
    out = []
    for view in views:
        mask = getattr(view, "gt_mask", None)
        if mask is None:
            out.append((view, None))
            continue
        W, H = int(view.image_width), int(view.image_height)
        if not isinstance(mask, torch.Tensor) or tuple(mask.shape) != (1, H, W):
            raise RuntimeError(f"alpha_cull_sdf: a view's `gt_mask` must be a tensor of shape (1, {H}, {W})")
        R = np.ascontiguousarray(torch.as_tensor(view.R).to(torch.float32).cpu().numpy())
        T = np.ascontiguousarray(torch.as_tensor(view.T).to(torch.float32).cpu().numpy())
        if R.shape != (3, 3) or T.shape != (3,):
            raise RuntimeError("alpha_cull_sdf: a view's `R` must have shape (3, 3) and its `T` shape (3,)")
        plane = mask.to(device=device, dtype=torch.float32).reshape(H, W).contiguous()
        out.append((view, (R, T, float(view.Fx), float(view.Fy), float(view.Cx), float(view.Cy), W, H, plane)))
    return out


def _alpha_cull_sdf_hip(points, sweep_views, pc, pipe, kernel_size, chunk):
    """alpha_cull_sdf over _sweep_views' list with the running minimum on the device: per chunk and view
    one `integrate` and one gsr_field_view_update, gsr_field_finish at the chunk's end.  The chunk's
    weight / seen live in its slice of the two results, so the sweep allocates nothing else."""
    from gaussian_renderer import integrate

    who = "alpha_cull_sdf"
    require(points, "points", (torch.float32,), 2, who)
    if points.size(1) != 3:
        raise RuntimeError(f"{who}: `points` must have shape (N, 3) (got {tuple(points.shape)})")
    dev, points = points.device, points.contiguous()
    sdf = torch.empty(points.shape[0], dtype=torch.float32, device=dev)
    valid = torch.empty(points.shape[0], dtype=torch.bool, device=dev)
    lo = 0
    for part in torch.chunk(points, points.shape[0] // chunk + 1):
        n = part.shape[0]
        weight, seen = sdf[lo:lo + n], valid[lo:lo + n].view(torch.uint8)
        lo += n
        if n == 0:
            continue
        weight.fill_(1)
        seen.zero_()
        for view, cam in sweep_views:
            ret = integrate(part, view, pc, pipe, kernel_size)
            alpha, inside = ret["alpha_integrated"], ret["inside"]
            require(alpha, "alpha_integrated", (torch.float32,), 1, who)
            require(inside, "inside", (torch.bool, torch.uint8), 1, who)
            if alpha.shape[0] != n or inside.shape[0] != n:
                raise RuntimeError(f"{who}: `integrate` must return one value per point")
            alpha, inside = alpha.contiguous(), inside.contiguous()
            if cam is None:
                call(dev, "gsr_field_view_update", n, None, ptr(alpha), ptr(inside), None, None, 0.0, 0.0, 0.0, 0.0,
                     0, 0, None, ptr(weight), ptr(seen), stream(dev))
            else:
                R, T, Fx, Fy, Cx, Cy, W, H, plane = cam
                call(dev, "gsr_field_view_update", n, ptr(part), ptr(alpha), ptr(inside), f32ptr(R), f32ptr(T), Fx,
                     Fy, Cx, Cy, W, H, ptr(plane), ptr(weight), ptr(seen), stream(dev))
        call(dev, "gsr_field_finish", n, ptr(weight), ptr(seen), ptr(weight), ptr(seen), stream(dev))
    return sdf, valid


@torch.no_grad()
def bisect_step(left_points, right_points, left_sdf, right_sdf, mid_sdf, mid_points):
    """One step of mesh_extract_tetrahedra.py:155-163 in place (gsr_field_bisect_step,
    csrc/fieldsweep.hip): where `mid_sdf` [E], the field at (left + right) * 0.5, has `left_sdf`'s sign the
    midpoint replaces the left end, otherwise (0 included) the right end; `mid_points` [E,3] receives the
    new (left + right) * 0.5.  Points [E,3] float32 or float64, sdf [E] or [E,1] float32, all contiguous
    (they are updated in place).  Runs on the current stream."""
    who = "bisect_step"
    require(left_points, "left_points", (torch.float32, torch.float64), 2, who)
    E, dev = left_points.size(0), left_points.device
    for t, name in ((left_points, "left_points"), (right_points, "right_points"), (mid_points, "mid_points")):
        require(t, name, (left_points.dtype,), 2, who)
        if tuple(t.shape) != (E, 3):
            raise RuntimeError(f"{who}: `{name}` must have shape ({E}, 3) (got {tuple(t.shape)})")
    for t, name in ((left_sdf, "left_sdf"), (right_sdf, "right_sdf"), (mid_sdf, "mid_sdf")):
        if (not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype != torch.float32
                or tuple(t.shape) not in ((E,), (E, 1))):
            raise RuntimeError(f"{who}: `{name}` must be a float32 HIP tensor of shape ({E},) or ({E}, 1)")
    for t in (left_points, right_points, mid_points, left_sdf, right_sdf, mid_sdf):
        if t.device != dev or not t.is_contiguous():
            raise RuntimeError(f"{who}: the buffers must be contiguous and on one device")
    call(dev, "gsr_field_bisect_step", E, ptr(left_points), ptr(right_points),
         int(left_points.dtype == torch.float64), ptr(left_sdf), ptr(right_sdf), ptr(mid_sdf), ptr(mid_points),
         stream(dev))


@torch.no_grad()
def alpha_cull_sdf(points, views, pc, pipe, kernel_size, chunk=10_000_000, sweep="torch"):
    """mesh_extract_tetrahedra.py:64-87: sdf = 0.5 - the smallest integrated
    opacity over the views that see the point (inside the image and, where a
    view has a gt_mask, on it); 0.5 where no view does.  -> (sdf [N], any_valid [N]).
    sweep="hip" keeps the running minimum on the device and folds every view
    in with one kernel (gsr_field_view_update / gsr_field_finish)
    instead of the torch formulation; the results are the same bits as long as
    no mask sample lies within rounding of 0.5."""
    from gaussian_renderer import integrate

    _check_sweep(sweep, "alpha_cull_sdf")
    if not isinstance(points, torch.Tensor) or not points.is_cuda:
        raise RuntimeError("alpha_cull_sdf: `points` must be a HIP device tensor")
    if sweep == "hip":
        return _alpha_cull_sdf_hip(points, _sweep_views(views, points.device), pc, pipe, kernel_size, chunk)
    sdfs, valids = [], []
    for part in torch.chunk(points, points.shape[0] // chunk + 1):
        weight = torch.ones(part.shape[0], dtype=torch.float32, device=points.device)
        seen = torch.zeros(part.shape[0], dtype=torch.bool, device=points.device)
        for view in views:
            ret = integrate(part, view, pc, pipe, kernel_size)
            ok = _view_mask(view, part, ret["inside"].bool())
            seen |= ok
            weight = torch.where(ok, torch.minimum(ret["alpha_integrated"], weight), weight)
        weight[~seen] = 0
        sdfs.append(0.5 - weight)
        valids.append(seen)
    return torch.cat(sdfs), torch.cat(valids)


@torch.no_grad()
def extract_mesh(points, points_scale, cells, views, pc, pipe, kernel_size, n_binary_steps=10, sweep="torch",
                 cluster_to_keep=None):
    """mesh_extract_tetrahedra.py:123-169: the level set sdf = 0 of
    alpha_cull_sdf over the tets `cells` [T,4] of `points` [V,3]
    (`points_scale` [V,1]: gsr_scene.tetra_points_scale), every vertex bisected
    n_binary_steps times along its edge; vertices whose edge is longer than
    the two ends' scales and the faces that use them are dropped.
    -> vertices [N,3] float32, faces [M,3] int64 (the geometry of recon.ply).
    With an integer `cluster_to_keep` the result goes through
    post_process_mesh (the geometry of recon_post.ply).  sweep="hip" runs all
    eleven sweeps as alpha_cull_sdf(sweep="hip") does, the views read once, and
    the bisection in place with bisect_step (no [E,3] temporaries per step)."""
    _check_sweep(sweep, "extract_mesh")
    if sweep == "hip":
        if not isinstance(points, torch.Tensor) or not points.is_cuda:
            raise RuntimeError("extract_mesh: `points` must be a HIP device tensor")
        sweep_views = _sweep_views(views, points.device)
        sdf, valid = _alpha_cull_sdf_hip(points, sweep_views, pc, pipe, kernel_size, 10_000_000)
    else:
        sdf, valid = alpha_cull_sdf(points, views, pc, pipe, kernel_size)
    verts_list, scale_list, faces_list, _ = marching_tetrahedra(points[None], cells, sdf[None], points_scale[None], valid[None])
    end_points, end_sdf = verts_list[0]
    end_scales, faces = scale_list[0], faces_list[0]
    left_points, right_points = end_points[:, 0, :].clone(), end_points[:, 1, :].clone()
    left_sdf, right_sdf = end_sdf[:, 0, :].clone(), end_sdf[:, 1, :].clone()
    distance = torch.norm(left_points - right_points, dim=-1)
    scale = end_scales[:, 0, 0] + end_scales[:, 1, 0]
    vertices = (left_points + right_points) * 0.5
    if sweep == "hip":  # `vertices` is the midpoint buffer: a step's query points, then its result
        for _ in range(n_binary_steps if vertices.shape[0] else 0):
            mid_sdf = _alpha_cull_sdf_hip(vertices, sweep_views, pc, pipe, kernel_size, 10_000_000)[0]
            bisect_step(left_points, right_points, left_sdf, right_sdf, mid_sdf, vertices)
    for _ in range(n_binary_steps if vertices.shape[0] and sweep == "torch" else 0):
        mid_points = (left_points + right_points) * 0.5
        mid_sdf = alpha_cull_sdf(mid_points, views, pc, pipe, kernel_size)[0].unsqueeze(-1)
        # a midpoint on the left end's side replaces it; one with sdf exactly 0 replaces the right end
        low = ((mid_sdf < 0) & (left_sdf < 0)) | ((mid_sdf > 0) & (left_sdf > 0))
        left_sdf = torch.where(low, mid_sdf, left_sdf)
        right_sdf = torch.where(low, right_sdf, mid_sdf)
        left_points = torch.where(low, mid_points, left_points)
        right_points = torch.where(low, right_points, mid_points)
        vertices = (left_points + right_points) * 0.5
    keep = distance <= scale
    faces = faces[keep[faces].all(dim=1)] if faces.shape[0] else faces
    used = torch.zeros(vertices.shape[0], dtype=torch.bool, device=vertices.device)
    used[faces.reshape(-1)] = True
    remap = torch.cumsum(used, 0) - 1
    vertices, faces = vertices[used].float().contiguous(), remap[faces].contiguous()
    if cluster_to_keep is not None:
        return post_process_mesh(vertices, faces, cluster_to_keep)
    return vertices, faces


def _view_camera(view):
    """(fx, fy, cx, cy) and the 4x4 world -> camera matrix of a view (mesh_extract.py:79-81); a view
    without Fx / Fy / Cx / Cy gets them from its field of view, the principal point at the centre."""
    import math

    W, H = view.image_width, view.image_height
    fx = getattr(view, "Fx", None) or W / (2.0 * math.tan(view.FoVx * 0.5))
    fy = getattr(view, "Fy", None) or H / (2.0 * math.tan(view.FoVy * 0.5))
    cx = getattr(view, "Cx", None)
    cy = getattr(view, "Cy", None)
    cx = (W - 1) * 0.5 if cx is None else cx
    cy = (H - 1) * 0.5 if cy is None else cy
    return (float(fx), float(fy), float(cx), float(cy)), view.world_view_transform.T


@torch.no_grad()
def extract_mesh_tsdf(views, pc, pipe, background, kernel_size, voxel_size=0.002, cluster_to_keep=None,
                      block_resolution=16, depth_scale=1.0, depth_max=8.0, trunc_voxel_multiplier=8.0,
                      weight_threshold=3.0):
    """mesh_extract.py:40-89 on the device: every view is rendered, its colour
    clamped to [0,1], its median depth zeroed where gt_mask < 0.5, and fused
    into a gsr_tsdf.VoxelBlockGrid (touch, then integrate); marching cubes
    once at the end.  -> (vertices [V,3] float32, faces [F,3] int64, colors
    [V,3] float32): recon.ply.  With an integer `cluster_to_keep` also the
    post_process_mesh result: (vertices, faces, colors, (vertices_post,
    faces_post)), the geometry of recon_post.ply."""
    from gaussian_renderer import render
    from gsr_tsdf import VoxelBlockGrid

    vbg = None
    for view in views:
        pkg = render(view, pc, pipe, background, kernel_size)
        color = torch.clamp(pkg["render"], min=0, max=1.0).permute(1, 2, 0).contiguous()
        depth = pkg["median_depth"].clone()
        mask = getattr(view, "gt_mask", None)
        if mask is not None:
            depth[mask < 0.5] = 0
        depth = depth[0].contiguous()
        if vbg is None:
            vbg = VoxelBlockGrid(voxel_size, block_resolution, with_color=True, device=depth.device)
        intrinsic, extrinsic = _view_camera(view)
        blocks = vbg.compute_unique_block_coordinates(depth, intrinsic, extrinsic, depth_scale, depth_max,
                                                      trunc_voxel_multiplier)
        vbg.integrate(blocks, depth, color, intrinsic, extrinsic, depth_scale, depth_max, trunc_voxel_multiplier)
    if vbg is None:
        raise ValueError("extract_mesh_tsdf: no views")
    vertices, faces, colors = vbg.extract_triangle_mesh(weight_threshold)
    if cluster_to_keep is not None:
        return vertices, faces, colors, post_process_mesh(vertices, faces, cluster_to_keep)
    return vertices, faces, colors


def write_ply(path, vertices, faces, colors=None):
    """A binary little-endian PLY of float32 vertices [N,3] and triangles [M,3]; with `colors` [N,3]
    in [0,1], uchar red / green / blue per vertex as well."""
    v = np.ascontiguousarray(torch.as_tensor(vertices).detach().cpu().numpy(), dtype="<f4").reshape(-1, 3)
    f = torch.as_tensor(faces).detach().cpu().numpy().reshape(-1, 3)
    rec = np.empty(f.shape[0], dtype=[("n", "u1"), ("v", "<i4", (3,))])
    rec["n"] = 3
    rec["v"] = f
    vertex_props = "property float x\nproperty float y\nproperty float z\n"
    vertex_bytes = v.tobytes()
    if colors is not None:
        c = torch.as_tensor(colors).detach().cpu().numpy().reshape(-1, 3)
        if c.shape[0] != v.shape[0]:
            raise ValueError(f"write_ply: {c.shape[0]} colours for {v.shape[0]} vertices")
        vrec = np.empty(v.shape[0], dtype=[("p", "<f4", (3,)), ("c", "u1", (3,))])
        vrec["p"] = v
        vrec["c"] = np.clip(np.rint(c.astype(np.float64) * 255.0), 0, 255).astype(np.uint8)
        vertex_props += "property uchar red\nproperty uchar green\nproperty uchar blue\n"
        vertex_bytes = vrec.tobytes()
    header = ("ply\nformat binary_little_endian 1.0\n"
              f"element vertex {v.shape[0]}\n{vertex_props}"
              f"element face {f.shape[0]}\nproperty list uchar int vertex_indices\nend_header\n")
    with open(path, "wb") as fh:
        fh.write(header.encode("ascii"))
        fh.write(vertex_bytes)
        fh.write(rec.tobytes())
