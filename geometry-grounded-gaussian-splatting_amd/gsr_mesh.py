"""Tetrahedral mesh extraction (mesh_extract_tetrahedra.py:64-169 and
utils/tetmesh.py of the reference) over the C ABI: marching tetrahedra in HIP
(gsr_marching_tetrahedra, csrc/tetmesh.hip) and the driver around
gaussian_renderer.integrate.

    points = gsr_scene.tetra_points(inp); scale = gsr_scene.tetra_points_scale(inp)
    cells = <the caller's Delaunay triangulation of points, [T, 4]>
    vertices, faces = extract_mesh(points, scale, cells, views, pc, pipe, kernel_size)
    write_ply("recon.ply", vertices, faces)

Face order: a tet's one or two triangles sit next to each other, in tet
order.  The reference lists, chunk by chunk, the one-triangle tets before the
two-triangle tets; the mesh is the same set of oriented triangles.
"""
from __future__ import annotations

import ctypes

import numpy as np
import torch

from diff_gaussian_rasterization import _C as _G

STAGES = ("flags", "count", "emit", "sort", "ranks", "edges", "faces")
# measurement hook (tools/bench_tetmesh.py): when a dict, every call leaves its per-stage GPU
# milliseconds and scratch bytes here (the timed call synchronises; leave None otherwise)
last_call_stats = None


def _lib():
    L = _G._load()
    if not getattr(L, "_tetmesh_bound", False):
        vp, i, ll = ctypes.c_void_p, ctypes.c_int, ctypes.c_longlong
        L.gsr_marching_tetrahedra.restype = i
        L.gsr_marching_tetrahedra.argtypes = [_G._ALLOC, vp, _G._ALLOC, vp, _G._ALLOC, vp, ll, ll, vp, i, vp, vp,
                                              ctypes.POINTER(ll), ctypes.POINTER(ll), ctypes.POINTER(ctypes.c_float),
                                              vp]
        L._tetmesh_bound = True
    return L


class _Int64Out:
    """An int64 output of the C ABI, allocated by its callback once the size is known."""

    def __init__(self, device):
        self.tensor = torch.empty(0, dtype=torch.int64, device=device)

        def _cb(_ctx, n):
            try:
                self.tensor = torch.empty(int(n) // 8, dtype=torch.int64, device=device)
                return self.tensor.data_ptr() or 1
            except Exception:  # noqa: BLE001 - allocation failure is reported as NULL
                return None

        self.cb = _G._ALLOC(_cb)


def _require(t, name, dtypes, ndim):
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise RuntimeError(f"marching_tetrahedra: `{name}` must be a HIP device tensor")
    if t.dtype not in dtypes:
        raise RuntimeError(f"marching_tetrahedra: `{name}` must be {' or '.join(str(d) for d in dtypes)} "
                           f"(got {t.dtype})")
    if t.dim() != ndim:
        raise RuntimeError(f"marching_tetrahedra: `{name}` must have {ndim} dimensions (got {tuple(t.shape)})")


@torch.no_grad()
def marching_tetrahedra_ids(tets, sdf, valid):
    """The unbatched kernel call: tets [T,4] int32 / int64, sdf [V] float32,
    valid [V] bool / uint8, all on one HIP device -> (edge_ids [E,2] int64,
    faces [F,3] int64).  Runs on the current stream."""
    global last_call_stats
    _require(tets, "tets", (torch.int32, torch.int64), 2)
    _require(sdf, "sdf", (torch.float32,), 1)
    _require(valid, "valids", (torch.bool, torch.uint8), 1)
    if tets.size(1) != 4:
        raise RuntimeError(f"marching_tetrahedra: `tets` must have shape (T, 4) (got {tuple(tets.shape)})")
    if valid.size(0) != sdf.size(0):
        raise RuntimeError("marching_tetrahedra: `sdf` and `valids` must have the same length")
    if sdf.device != tets.device or valid.device != tets.device:
        raise RuntimeError("marching_tetrahedra: inputs must be on one device")
    dev = tets.device
    L = _lib()
    tets, sdf = tets.contiguous(), sdf.contiguous()
    valid = valid.contiguous().view(torch.uint8)
    T, V = tets.size(0), sdf.size(0)
    edges, faces, scratch = _Int64Out(dev), _Int64Out(dev), _G._ScratchBlocks(dev)
    E, F = ctypes.c_longlong(0), ctypes.c_longlong(0)
    ms = (ctypes.c_float * 8)() if last_call_stats is not None else None
    with torch.cuda.device(dev):
        rc = L.gsr_marching_tetrahedra(edges.cb, None, faces.cb, None, scratch.cb, None, T, V, _G._ptr(tets),
                                       int(tets.dtype == torch.int64), _G._ptr(sdf), _G._ptr(valid),
                                       ctypes.byref(E), ctypes.byref(F), ms, _G._stream(dev))
    if rc != 0:
        raise RuntimeError("gsr: " + L.gsr_last_error().decode())
    if last_call_stats is not None:
        last_call_stats.clear()
        last_call_stats.update({k: float(ms[i]) for i, k in enumerate(STAGES)},
                               scratch_bytes=[int(b.numel()) for b in scratch.blocks])
    if E.value == 0:
        return (torch.zeros(0, 2, dtype=torch.int64, device=dev), torch.zeros(0, 3, dtype=torch.int64, device=dev))
    return edges.tensor[:2 * E.value].view(-1, 2), faces.tensor[:3 * F.value].view(-1, 3)


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


@torch.no_grad()
def alpha_cull_sdf(points, views, pc, pipe, kernel_size, chunk=10_000_000):
    """mesh_extract_tetrahedra.py:64-87: sdf = 0.5 - the smallest integrated
    opacity over the views that see the point (inside the image and, where a
    view has a gt_mask, on it); 0.5 where no view does.  -> (sdf [N], any_valid [N])."""
    from gaussian_renderer import integrate

    if not isinstance(points, torch.Tensor) or not points.is_cuda:
        raise RuntimeError("alpha_cull_sdf: `points` must be a HIP device tensor")
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
def extract_mesh(points, points_scale, cells, views, pc, pipe, kernel_size, n_binary_steps=10):
    """mesh_extract_tetrahedra.py:123-169: the level set sdf = 0 of
    alpha_cull_sdf over the tets `cells` [T,4] of `points` [V,3]
    (`points_scale` [V,1]: gsr_scene.tetra_points_scale), every vertex bisected
    n_binary_steps times along its edge; vertices whose edge is longer than
    the two ends' scales and the faces that use them are dropped.
    -> vertices [N,3] float32, faces [M,3] int64."""
    sdf, valid = alpha_cull_sdf(points, views, pc, pipe, kernel_size)
    verts_list, scale_list, faces_list, _ = marching_tetrahedra(points[None], cells, sdf[None], points_scale[None], valid[None])
    end_points, end_sdf = verts_list[0]
    end_scales, faces = scale_list[0], faces_list[0]
    left_points, right_points = end_points[:, 0, :].clone(), end_points[:, 1, :].clone()
    left_sdf, right_sdf = end_sdf[:, 0, :].clone(), end_sdf[:, 1, :].clone()
    distance = torch.norm(left_points - right_points, dim=-1)
    scale = end_scales[:, 0, 0] + end_scales[:, 1, 0]
    vertices = (left_points + right_points) * 0.5
    for _ in range(n_binary_steps if vertices.shape[0] else 0):
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
    return vertices[used].float().contiguous(), remap[faces].contiguous()


def write_ply(path, vertices, faces):
    """A binary little-endian PLY of float32 vertices [N,3] and triangles [M,3]."""
    v = np.ascontiguousarray(torch.as_tensor(vertices).detach().cpu().numpy(), dtype="<f4").reshape(-1, 3)
    f = torch.as_tensor(faces).detach().cpu().numpy().reshape(-1, 3)
    rec = np.empty(f.shape[0], dtype=[("n", "u1"), ("v", "<i4", (3,))])
    rec["n"] = 3
    rec["v"] = f
    header = ("ply\nformat binary_little_endian 1.0\n"
              f"element vertex {v.shape[0]}\nproperty float x\nproperty float y\nproperty float z\n"
              f"element face {f.shape[0]}\nproperty list uchar int vertex_indices\nend_header\n")
    with open(path, "wb") as fh:
        fh.write(header.encode("ascii"))
        fh.write(v.tobytes())
        fh.write(rec.tobytes())
