"""TSDF fusion and marching cubes on the device (the open3d VoxelBlockGrid of
the reference's mesh_extract.py:63-85) over the C ABI: gsr_tsdf_touch,
gsr_tsdf_lookup, gsr_tsdf_integrate and gsr_tsdf_extract (csrc/tsdf.hip).

    vbg = VoxelBlockGrid(voxel_size=0.002)
    for depth, color, intrinsic, extrinsic in views:
        blocks = vbg.compute_unique_block_coordinates(depth, intrinsic, extrinsic)
        vbg.integrate(blocks, depth, color, intrinsic, extrinsic)
    vertices, faces, colors = vbg.extract_triangle_mesh()

The contract is DESIGN §6h.  It restates open3d's behaviour from memory; no
bit-parity with open3d is claimed.  `intrinsic` is (fx, fy, cx, cy) or a 3x3
matrix, `extrinsic` the 4x4 world -> camera matrix (the reference's
world_view_transform.T).
"""
from __future__ import annotations

import ctypes

import numpy as np
import torch

from diff_gaussian_rasterization._abi import Out, ScratchBlocks, call, ptr, record_stats, require, stage_buffer, stream

KEY_BIAS = 1 << 20
EXTRACT_STAGES = ("mark", "count", "vertices", "faces")
# measurement hook (tools/bench_tsdf.py): when a dict, extract_triangle_mesh leaves its per-stage GPU
# milliseconds and scratch bytes here (the timed call synchronises; leave None otherwise)
last_call_stats = None


def _camera(intrinsic, extrinsic, who):
    k = np.asarray(torch.as_tensor(intrinsic).detach().cpu().numpy(), dtype=np.float64)
    if k.shape == (3, 3):
        k = np.array([k[0, 0], k[1, 1], k[0, 2], k[1, 2]])
    if k.shape != (4,):
        raise RuntimeError(f"{who}: `intrinsic` must be (fx, fy, cx, cy) or a 3x3 matrix (got shape {k.shape})")
    e = np.asarray(torch.as_tensor(extrinsic).detach().cpu().numpy(), dtype=np.float64)
    if e.shape != (4, 4):
        raise RuntimeError(f"{who}: `extrinsic` must be a 4x4 world -> camera matrix (got shape {e.shape})")
    if not (np.isfinite(k).all() and np.isfinite(e).all()):
        raise RuntimeError(f"{who}: `intrinsic` and `extrinsic` must be finite")
    return (ctypes.c_float * 4)(*k.astype(np.float32)), (ctypes.c_float * 16)(*e.astype(np.float32).reshape(-1))


def _positive(who, **values):
    for name, v in values.items():
        if not (isinstance(v, (int, float)) and not isinstance(v, bool) and v > 0 and np.isfinite(v)):
            raise ValueError(f"{who}: `{name}` must be a positive finite number (got {v!r})")


def pack_keys(block_coords):
    """The packed keys [n] int64 of block coordinates [n,3]: 21 bits per axis, biased by 2^20, x high."""
    c = block_coords.to(torch.int64) + KEY_BIAS
    return c[:, 0] << 42 | c[:, 1] << 21 | c[:, 2]


class VoxelBlockGrid:
    """A sparse grid of R^3-voxel blocks with tsdf, weight and, optionally,
    colour per voxel, all float32.  Blocks keep the slot they were given when
    first seen (insertion order; blocks new in one call in ascending key
    order); capacity grows geometrically."""

    def __init__(self, voxel_size, block_resolution=16, with_color=True, device="cuda", block_count=1024):
        _positive("VoxelBlockGrid", voxel_size=voxel_size)
        if block_resolution not in (8, 16):
            raise ValueError(f"VoxelBlockGrid: `block_resolution` must be 8 or 16 (got {block_resolution!r})")
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError(f"VoxelBlockGrid: `device` must be a HIP device (got {self.device})")
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        self.voxel_size = float(voxel_size)
        self.block_resolution = int(block_resolution)
        self.with_color = bool(with_color)
        self._n = 0
        self._keys = torch.empty(0, dtype=torch.int64, device=self.device)    # by slot
        self._coords = torch.empty(0, 3, dtype=torch.int32, device=self.device)
        self._sorted_keys = torch.empty(0, dtype=torch.int64, device=self.device)
        self._sorted_slots = torch.empty(0, dtype=torch.int32, device=self.device)
        self._tsdf = self._weight = self._color = None
        self._capacity = 0
        self._reserve(max(int(block_count), 1))

    # ---- state -------------------------------------------------------------------------------

    @property
    def voxels_per_block(self):
        return self.block_resolution ** 3

    @property
    def num_blocks(self):
        return self._n

    @property
    def block_keys(self):
        """[n] int64 packed keys, by slot."""
        return self._keys[:self._n]

    @property
    def block_coords(self):
        """[n,3] int32 block coordinates, by slot."""
        return self._coords[:self._n]

    @property
    def tsdf(self):
        """[n, R^3] float32, a view of the grid's storage."""
        return self._tsdf[:self._n]

    @property
    def weight(self):
        return self._weight[:self._n]

    @property
    def color(self):
        """[n, R^3, 3] float32, or None without colour."""
        return self._color[:self._n] if self.with_color else None

    def _reserve(self, blocks):
        """Capacity for `blocks` blocks; storage moves only here, and slots keep their data."""
        if blocks <= self._capacity:
            return
        cap = max(blocks, 2 * self._capacity)
        N = self.voxels_per_block

        def grown(old, *shape):
            new = torch.zeros(cap, *shape, dtype=torch.float32, device=self.device)
            if old is not None and self._n:
                new[:self._n] = old[:self._n]
            return new

        self._tsdf, self._weight = grown(self._tsdf, N), grown(self._weight, N)
        if self.with_color:
            self._color = grown(self._color, N, 3)
        self._capacity = cap

    def _check_coords(self, block_coords, who):
        require(block_coords, "block_coords", (torch.int32,), 2, who)
        if block_coords.size(1) != 3:
            raise RuntimeError(f"{who}: `block_coords` must have shape (n, 3) (got {tuple(block_coords.shape)})")
        if block_coords.device != self.device:
            raise RuntimeError(f"{who}: `block_coords` must be on {self.device}")
        block_coords = block_coords.contiguous()
        if block_coords.numel():
            lo, hi = int(block_coords.min()), int(block_coords.max())
            if lo < -KEY_BIAS or hi >= KEY_BIAS:
                raise RuntimeError(f"{who}: a block coordinate is outside [-2^20, 2^20)")
        return block_coords

    def _ranks(self, block_coords):
        """The position of every coordinate in the sorted index, -1 where the grid lacks the block."""
        n = block_coords.size(0)
        rank = torch.empty(n, dtype=torch.int32, device=self.device)
        call(self.device, "gsr_tsdf_lookup", n, ptr(block_coords), self._n, ptr(self._sorted_keys), ptr(rank),
             stream(self.device))
        return rank

    def _slots(self, block_coords, add):
        """The slot of every coordinate (-1: not in the grid); with `add`, missing blocks get the
        next slots in ascending key order first and the sorted index is rebuilt."""
        rank = self._ranks(block_coords)
        if add and block_coords.size(0) and bool((rank < 0).any()):
            fresh = block_coords[rank < 0]
            keys, first = torch.unique(pack_keys(fresh), return_inverse=True)  # ascending
            coords = torch.empty(keys.size(0), 3, dtype=torch.int32, device=self.device)
            coords[first] = fresh
            m = keys.size(0)
            self._reserve(self._n + m)
            self._keys = torch.cat([self._keys[:self._n], keys])
            self._coords = torch.cat([self._coords[:self._n], coords])
            self._n += m
            self._sorted_keys, order = torch.sort(self._keys)
            self._sorted_slots = order.to(torch.int32).contiguous()
            rank = self._ranks(block_coords)
        slots = torch.full_like(rank, -1)
        found = rank >= 0
        slots[found] = self._sorted_slots[rank[found].long()]
        return slots

    # ---- the three stages --------------------------------------------------------------------

    def _check_depth(self, depth, who):
        require(depth, "depth", (torch.float32,), 2, who)
        if depth.device != self.device:
            raise RuntimeError(f"{who}: `depth` must be on {self.device}")
        if depth.numel() == 0:
            raise RuntimeError(f"{who}: `depth` is empty")
        return depth.contiguous()

    @torch.no_grad()
    def compute_unique_block_coordinates(self, depth, intrinsic, extrinsic, depth_scale=1.0, depth_max=8.0,
                                         trunc_voxel_multiplier=8.0):
        """The blocks a depth image [H,W] float32 (0: no measurement) touches:
        [n,3] int32, unique, ascending by packed key.  The grid is not changed."""
        who = "compute_unique_block_coordinates"
        depth = self._check_depth(depth, who)
        _positive(who, depth_scale=depth_scale, depth_max=depth_max, trunc_voxel_multiplier=trunc_voxel_multiplier)
        k, e = _camera(intrinsic, extrinsic, who)
        out, scratch = Out(self.device, torch.int32), ScratchBlocks(self.device)
        n = ctypes.c_longlong(0)
        call(self.device, "gsr_tsdf_touch", out.cb, None, scratch.cb, None, ptr(depth), depth.size(0), depth.size(1),
             k, e, float(depth_scale), float(depth_max), self.voxel_size * float(trunc_voxel_multiplier),
             self.voxel_size * self.block_resolution, ctypes.byref(n), stream(self.device))
        return out.tensor[:3 * n.value].view(-1, 3)

    @torch.no_grad()
    def integrate(self, block_coords, depth, color, intrinsic, extrinsic, depth_scale=1.0, depth_max=8.0,
                  trunc_voxel_multiplier=8.0):
        """One view into the blocks `block_coords` [n,3] int32 (unique; blocks
        the grid lacks are added first) and into no other block.  `color`
        [H,W,3] float32 in [0,1]; None only for a grid without colour."""
        who = "integrate"
        depth = self._check_depth(depth, who)
        block_coords = self._check_coords(block_coords, who)
        _positive(who, depth_scale=depth_scale, depth_max=depth_max, trunc_voxel_multiplier=trunc_voxel_multiplier)
        if self.with_color:
            require(color, "color", (torch.float32,), 3, who)
            if tuple(color.shape) != (depth.size(0), depth.size(1), 3) or color.device != self.device:
                raise RuntimeError(f"{who}: `color` must have shape (H, W, 3) on {self.device} "
                                   f"(got {tuple(color.shape)} on {color.device})")
            color = color.contiguous()
        else:
            color = None
        k, e = _camera(intrinsic, extrinsic, who)
        n = block_coords.size(0)
        if n == 0:
            return
        if torch.unique(pack_keys(block_coords)).numel() != n:
            raise RuntimeError(f"{who}: `block_coords` lists a block twice")
        slots = self._slots(block_coords, add=True)
        call(self.device, "gsr_tsdf_integrate", n, self.block_resolution, ptr(block_coords), ptr(slots), self._n,
             self.voxel_size, ptr(self._tsdf), ptr(self._weight), ptr(self._color) if self.with_color else None,
             ptr(depth), ptr(color), depth.size(0), depth.size(1), k, e, float(depth_scale), float(depth_max),
             self.voxel_size * float(trunc_voxel_multiplier), stream(self.device))

    @torch.no_grad()
    def extract_triangle_mesh(self, weight_threshold=3.0):
        """Marching cubes over the cubes whose 8 corners have weight >
        weight_threshold -> (vertices [V,3] float32, faces [F,3] int64, colors
        [V,3] float32 or None without colour).  Vertices are shared between
        cubes; there are no vertex normals."""
        who = "extract_triangle_mesh"
        if isinstance(weight_threshold, bool) or not isinstance(weight_threshold, (int, float)) or \
                not np.isfinite(weight_threshold):
            raise ValueError(f"{who}: `weight_threshold` must be a finite number (got {weight_threshold!r})")
        dev = self.device
        vout, cout, fout = Out(dev, torch.float32), Out(dev, torch.float32), Out(dev, torch.int64)
        scratch = ScratchBlocks(dev)
        V, F = ctypes.c_longlong(0), ctypes.c_longlong(0)
        ms = stage_buffer(last_call_stats is not None)
        call(dev, "gsr_tsdf_extract", vout.cb, None, cout.cb, None, fout.cb, None, scratch.cb, None, self._n,
             self.block_resolution, self.voxel_size, float(weight_threshold), ptr(self._sorted_keys),
             ptr(self._sorted_slots), ptr(self._tsdf), ptr(self._weight),
             ptr(self._color) if self.with_color else None, ctypes.byref(V), ctypes.byref(F), ms, stream(dev))
        record_stats(last_call_stats, EXTRACT_STAGES, ms, scratch)
        vertices = vout.tensor[:3 * V.value].view(-1, 3)
        faces = fout.tensor[:3 * F.value].view(-1, 3)
        colors = cout.tensor[:3 * V.value].view(-1, 3) if self.with_color else None
        return vertices, faces, colors

    @classmethod
    def from_arrays(cls, block_coords, tsdf, weight, color=None, voxel_size=0.002, block_resolution=16):
        """A grid holding the given voxel data: block_coords [n,3] int32
        (unique), tsdf / weight [n, R^3] float32, color [n, R^3, 3] float32 or
        None.  Slot i is row i."""
        who = "from_arrays"
        for t, name, nd in ((tsdf, "tsdf", 2), (weight, "weight", 2)):
            require(t, name, (torch.float32,), nd, who)
        if color is not None:
            require(color, "color", (torch.float32,), 3, who)
        g = cls(voxel_size, block_resolution, with_color=color is not None, device=tsdf.device,
                block_count=max(int(tsdf.size(0)), 1))
        block_coords = g._check_coords(block_coords, who)
        n, N = block_coords.size(0), g.voxels_per_block
        if tuple(tsdf.shape) != (n, N) or tuple(weight.shape) != (n, N) or \
                (color is not None and tuple(color.shape) != (n, N, 3)):
            raise RuntimeError(f"{who}: `tsdf` and `weight` must have shape ({n}, {N}) and `color` ({n}, {N}, 3)")
        if weight.device != g.device or (color is not None and color.device != g.device):
            raise RuntimeError(f"{who}: the arrays must be on one device")
        keys = pack_keys(block_coords)
        if torch.unique(keys).numel() != n:
            raise RuntimeError(f"{who}: `block_coords` lists a block twice")
        g._n = n
        g._keys, g._coords = keys, block_coords.clone()
        g._sorted_keys, order = torch.sort(keys)
        g._sorted_slots = order.to(torch.int32).contiguous()
        g._tsdf[:n], g._weight[:n] = tsdf, weight
        if color is not None:
            g._color[:n] = color
        return g
