"""`_abi` — the one ctypes binding of libgsr.so (include/gsr.h).

Every module of the package that calls the C ABI goes through here: the
library is opened once (load), every prototype of the header is written down
once (SIGNATURES; tests/test_abi_table.py holds the table and the three
structures to the header), and the idioms around a call live here too — the
status check, device pointers, the current stream, the device guard (call),
the callback allocators, the stage-time buffer of the measurement hooks and
the tensor checks the mesh and evaluation modules share.

There is no CPU fallback: the library must load, otherwise load() raises.
"""
from __future__ import annotations

import ctypes
import os
from ctypes import POINTER, c_char_p, c_double, c_float, c_int, c_longlong, c_size_t, c_uint, c_ulonglong, c_void_p

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("GSR_LIB") or os.path.join(_HERE, "libgsr.so")  # GSR_LIB: development A/B builds
# include/gsr.h ABI these bindings are written for (gsr_abi_version)
ABI_VERSION = 20

_ALLOC = ctypes.CFUNCTYPE(c_void_p, c_void_p, c_size_t)  # gsr_alloc_fn
_CHUNK = ctypes.CFUNCTYPE(None, c_void_p, c_int, c_int)  # gsr_chunk_fn


class AdamGroup(ctypes.Structure):
    """gsr_adam_group (include/gsr.h)."""
    _fields_ = [("param", c_void_p), ("grad", c_void_p), ("exp_avg", c_void_p), ("exp_avg_sq", c_void_p),
                ("n", c_longlong), ("lr", c_double)]


class PointIndex(ctypes.Structure):
    """gsr_point_index (include/gsr.h)."""
    _fields_ = [("R", c_longlong), ("buffer", c_void_p), ("bounds_min", c_double * 3), ("bounds_max", c_double * 3),
                ("cell_size", c_double), ("cells", c_longlong * 3), ("key_bits", c_int * 3)]


class DensifyParam(ctypes.Structure):
    """gsr_densify_param (include/gsr.h)."""
    _fields_ = [("param", c_void_p), ("exp_avg", c_void_p), ("exp_avg_sq", c_void_p), ("param_out", c_void_p),
                ("exp_avg_out", c_void_p), ("exp_avg_sq_out", c_void_p), ("width", c_int), ("role", c_int)]


# ---- the signature table -----------------------------------------------------------------------------------------
# name -> (restype, argtypes) for every function of include/gsr.h, in the header's order.  Device pointers and
# the stream are vp; host arrays the caller fills or reads are typed pointers.
vp, i, u, ll, sz, f, d = c_void_p, c_int, c_uint, c_longlong, c_size_t, c_float, c_double
ip, llp, ullp, fp, dp = POINTER(c_int), POINTER(c_longlong), POINTER(c_ulonglong), POINTER(c_float), POINTER(c_double)
A = [_ALLOC, vp]  # a (gsr_alloc_fn, ctx) pair

_FWD = (A * 4 + [i] * 5 + [vp, i, i] + [vp] * 10 + [f] + [vp] * 3 + [f] * 3 + [i] + [vp] * 5 + [i, i, vp, ip])
_BWD = (A + [i] * 6 + [vp, i, i] + [vp] * 10 + [f] + [vp] * 3 + [f] * 3 + [vp] * 23 + [i, i])  # (up to `debug`)
_BWD_EX = _BWD + [i, _CHUNK, vp, vp, vp]
_POINTS = A * 6 + [i] * 4 + [vp] * 4 + [f]  # sample_depth / integrate / evaluate_sdf up to scale_modifier
_SAMPLE = _POINTS + [vp] * 5 + [f] * 3 + [i] + [vp, vp, i, vp, ip, ip, ip]
_PM_TERMS = [i, i] + [vp] * 6 + [f] * 5 + [vp] * 4 + [f] * 8 + [i, i] + [vp] * 4  # H ... saved_gn
_PHOTO = [i, i, i, i, f] + [vp] * 6 + [i] * 4  # H ... crop_w

SIGNATURES = {
    # rasterizer
    "gsr_rasterize_forward": (i, _FWD),
    "gsr_rasterize_forward_ex": (i, _FWD + A),
    "gsr_rasterize_backward": (i, _BWD + [vp]),
    "gsr_rasterize_backward_ex": (i, _BWD_EX),
    "gsr_rasterize_forward_ex2": (i, _FWD + A + [vp]),
    "gsr_rasterize_backward_ex2": (i, _BWD_EX + [vp, vp]),
    "gsr_backward_chunk_size": (i, [i, i]),
    "gsr_mark_visible": (i, [i] + [vp] * 5),
    # sample_depth and the point queries
    "gsr_sample_depth_forward": (i, _SAMPLE),
    "gsr_sample_depth_forward_ex": (i, _SAMPLE + A),
    "gsr_integrate_forward": (i, _POINTS + [vp] * 6 + [f] * 3 + [i] + [vp, vp, i, vp, ip]),
    "gsr_evaluate_sdf_forward": (i, _POINTS + [vp] * 6 + [f] * 3 + [i] + [vp, vp, vp, i, vp, ip]),
    "gsr_sample_depth_backward": (i, A + [i] * 7 + [vp] * 4 + [f] + [vp] * 5 + [f] * 3 + [vp] * 14 + [i, vp]),
    # training update and statistics
    "gsr_adam_step": (i, [i, POINTER(AdamGroup), d, d, d, d, vp]),
    "gsr_densify_stats": (i, [i] + [vp] * 7),
    "gsr_view_color_grads_chunked": (i, [i] * 7 + [vp] * 12),
    "gsr_view_color_grads": (i, [i] * 6 + [vp] * 10),
    # multi-view photometric term, getters, PatchMatch
    "gsr_warp_patch_ncc": (i, [i] + [vp] * 7 + [f] * 8 + [i] * 4 + [vp] * 5),
    "gsr_scale_opacity_3d_filter": (i, [i] + [vp] * 6),
    "gsr_scale_opacity_3d_filter_backward": (i, [i] + [vp] * 8),
    "gsr_normalize_rows": (i, [i, i, vp, vp, vp]),
    "gsr_normalize_rows_backward": (i, [i, i, vp, vp, vp, vp]),
    "gsr_patchmatch_lift": (i, [i, i, f, f, f, f] + [vp] * 5),
    "gsr_patchmatch_lift_backward": (i, [i, i, f, f, f, f] + [vp] * 4),
    "gsr_patchmatch_terms_forward": (i, A + _PM_TERMS + [vp, vp]),
    "gsr_patchmatch_terms_backward": (i, _PM_TERMS + [vp] * 6),
    # losses
    "gsr_fused_ssim_forward": (i, A + [i, i, i, i] + [vp] * 5),
    "gsr_fused_ssim_backward": (i, [i, i, i, i] + [vp] * 6),
    "gsr_photo_loss_forward": (i, A + _PHOTO + [vp] * 5),
    "gsr_photo_loss_backward": (i, _PHOTO + [vp] * 7),
    "gsr_depth_to_normal_forward": (i, [vp, i, i, f, f, f, f, vp, vp, vp]),
    "gsr_depth_to_normal_backward": (i, [vp, i, i, f, f, f, f, vp, vp, vp]),
    # initial scales
    "gsr_knn_mean_dist": (i, A + [i, vp, vp, vp]),
    # marching tetrahedra, the extraction sweep and mesh clean-up
    "gsr_marching_tetrahedra": (i, A * 3 + [ll, ll, vp, i, vp, vp, llp, llp, fp, vp]),
    "gsr_field_view_update": (i, [ll, vp, vp, vp, fp, fp, d, d, d, d, i, i, vp, vp, vp, vp]),
    "gsr_field_finish": (i, [ll] + [vp] * 5),
    "gsr_field_bisect_step": (i, [ll, vp, vp, i] + [vp] * 5),
    "gsr_mesh_clusters": (i, A * 3 + [ll, ll, vp, i, vp, vp, llp, fp, vp]),
    "gsr_mesh_filter": (i, A * 3 + [ll, ll, ll, vp, vp, i, vp, vp, vp, llp, llp, vp]),
    # TSDF fusion and marching cubes
    "gsr_tsdf_touch": (i, A * 2 + [vp, i, i, fp, fp, f, f, f, f, llp, vp]),
    "gsr_tsdf_lookup": (i, [ll, vp, ll, vp, vp, vp]),
    "gsr_tsdf_integrate": (i, [ll, i, vp, vp, ll, f] + [vp] * 5 + [i, i, fp, fp, f, f, f, vp]),
    "gsr_tsdf_extract": (i, A * 4 + [ll, i, f, f] + [vp] * 5 + [llp, llp, fp, vp]),
    # point-cloud evaluation (DTU)
    "gsr_mesh_sample_points": (i, A * 2 + [ll, ll, vp, vp, i, d, llp, fp, vp]),
    "gsr_points_downsample": (i, A * 2 + [ll, vp, d, llp, llp, fp, vp]),
    "gsr_points_nearest": (i, A + [ll, vp, ll, vp, d, vp, fp, vp]),
    # Tanks and Temples F-score
    "gsr_points_crop_polygon": (i, A * 3 + [ll, vp, dp, i, d, d, i, dp, llp, fp, vp]),
    "gsr_points_voxel_mean": (i, A * 4 + [ll, vp, d, llp, fp, vp]),
    "gsr_points_index_bytes": (sz, [ll]),
    "gsr_points_index_build": (i, A + [ll, vp, vp, sz, POINTER(PointIndex), fp, vp]),
    "gsr_points_index_query": (i, A + [POINTER(PointIndex), ll, vp, d, vp, vp, fp, vp]),
    "gsr_icp_accumulate": (i, A + [ll, vp, ll, vp, vp, i, dp, dp, fp, vp]),
    "gsr_points_transform": (i, [ll, vp, dp, fp, vp]),
    # Tanks and Temples mesh culling
    "gsr_mesh_depth": (i, A + [ll, vp, ll, vp, i, fp, i, i] + [f] * 6 + [vp, ullp, fp, vp]),
    "gsr_mesh_view_votes": (i, A + [ll, vp, ll, vp, i, i, fp, i, i] + [f] * 7 + [vp, ullp, fp, vp]),
    # per-stage timing
    "gsr_timing_enable": (i, [i]),
    "gsr_timing_stage_mask": (i, [u]),
    "gsr_timing_collect": (i, [dp, ip]),
    "gsr_stage_name": (c_char_p, [i]),
    # options and test hooks
    "gsr_set_option": (i, [i, i]),
    "gsr_debug_render_stats": (i, [ullp, i]),
    "gsr_debug_binning": (i, [vp, vp, i, i, i, vp, vp, vp]),
    "gsr_debug_image": (i, [vp, i, i, vp, vp]),
    "gsr_debug_sample_points": (i, [vp, i, vp, vp, vp]),
    "gsr_debug_tile_stats": (i, [vp, i, i, vp, vp]),
    "gsr_debug_depth_sort_tile_keys": (i, [i]),
    "gsr_debug_depth_sort_bytes": (ll, [i]),
    "gsr_debug_depth_sort": (i, [i, vp, vp, vp, vp, i, vp]),
    "gsr_debug_list_constants": (i, [ip, i]),
    "gsr_debug_scan_excl_bytes": (ll, [ll]),
    "gsr_debug_scan_excl": (i, [vp, vp, ll, u, vp, u, vp, vp]),
    # densification
    "gsr_densify_workspace_bytes": (ll, [ll]),
    "gsr_densify_plan": (i, [ll] + [vp] * 5 + [f, f, f, vp, llp, fp, vp]),
    "gsr_densify_apply": (i, [ll, llp, vp, vp, i, vp, ll, vp, vp, i, POINTER(DensifyParam), vp]),
    "gsr_quantile_workspace_bytes": (ll, []),
    "gsr_quantile": (i, [ll] + [vp] * 5),
    "gsr_filter_3d": (i, [ll, vp, i, vp, f, vp, vp, vp]),
    "gsr_reset_opacity": (i, [ll] + [vp] * 7),
    # image-quality evaluation
    "gsr_image_quantize8": (i, [ll, i, i, i, vp, vp, vp]),
    "gsr_image_metrics": (i, A + [i] * 6 + [vp] * 6),
    # view preparation
    "gsr_resample_ksize": (i, [i, i]),
    "gsr_resample_coeffs": (i, [i, i, ip, ip]),
    "gsr_image_resample8": (i, [ll, i, i, i, i, i, vp, vp, vp, vp, vp]),
    "gsr_view_planes": (i, [ll, i, i] + [vp] * 6),
    # model files
    "gsr_model_row_floats": (i, [i, i]),
    "gsr_model_block_rows": (i, [i]),
    "gsr_model_unpack_block_rows": (i, [ll]),
    "gsr_model_pack_rows": (i, [ll, i, i] + [vp] * 12),
    "gsr_model_unpack_rows": (i, [ll, i, i, ll] + [vp] * 14),
    # status
    "gsr_last_error": (c_char_p, []),
    "gsr_abi_version": (i, []),
}
del vp, i, u, ll, sz, f, d, ip, llp, ullp, fp, dp, A

_lib = None


def load():
    """The one CDLL of libgsr.so, opened and bound on first use.  A function the loaded library does not
    export (an A/B build from before an additive entry point) is skipped: using it raises ctypes' own
    AttributeError."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(f"libgsr.so not built ({LIB_PATH}); run `make -C geometry-grounded-gaussian-splatting_amd` "
                           "or __graft_entry__.build()")
    L = ctypes.CDLL(LIB_PATH)
    L.gsr_abi_version.restype = c_int
    if L.gsr_abi_version() != ABI_VERSION:  # the table is written for this ABI
        raise RuntimeError(f"{LIB_PATH}: ABI {L.gsr_abi_version()}, expected {ABI_VERSION} (stale build? "
                           "run `make -C geometry-grounded-gaussian-splatting_amd`)")
    for name, (restype, argtypes) in SIGNATURES.items():
        fn = getattr(L, name, None)
        if fn is not None:
            fn.restype, fn.argtypes = restype, argtypes
    _lib = L
    return L


def loaded_library_path() -> str:
    load()
    return LIB_PATH


# ---- the idioms around a call ------------------------------------------------------------------------------------

def check(rc):
    if rc != 0:
        raise RuntimeError("gsr: " + _lib.gsr_last_error().decode())


def ptr(t):
    if t is None or t.numel() == 0:
        return None
    return c_void_p(t.data_ptr())


def f64ptr(a):
    """A contiguous float64 numpy array as the C ABI's host `double*`."""
    return a.ctypes.data_as(POINTER(c_double))


def f32ptr(a):
    """A contiguous float32 numpy array as the C ABI's host `float*`."""
    return a.ctypes.data_as(POINTER(c_float))


def stream(device):
    return c_void_p(torch.cuda.current_stream(device).cuda_stream)


def call(device, name, *args):
    """The library's function `name` on `args` with `device` current; a non-zero status raises.  The stream to
    launch on is one of `args` (stream(device))."""
    fn = getattr(_lib or load(), name)
    with torch.cuda.device(device):
        rc = fn(*args)
    if rc != 0:
        check(rc)


def dev32(t, name, who):
    """`t` contiguous, refused with `who`'s message unless it is a float32 device tensor."""
    if not t.is_cuda or t.dtype != torch.float32:
        raise RuntimeError(f"{who}: `{name}` must be a float32 HIP tensor")
    return t.contiguous()


# ---- callback allocators -----------------------------------------------------------------------------------------

class Out:
    """A device tensor of `dtype` handed to the C ABI as an allocation callback: allocated (zero-filled with
    `zero`) once the library knows its size (replaces resizeFunctional, DGR/rasterize_points.cu:27-37).
    Four of these are made per training forward: the constructor does no more than it must."""

    __slots__ = ("tensor", "cb")

    def __init__(self, device, dtype, zero=False):
        self.tensor = torch.empty(0, dtype=dtype, device=device)

        def _cb(_ctx, n):
            try:
                self.tensor = (torch.zeros if zero else torch.empty)(int(n) // dtype.itemsize, dtype=dtype,
                                                                     device=device)
                return self.tensor.data_ptr() or 1  # (a size of 0 is not a failure)
            except Exception:  # noqa: BLE001 - allocation failure is reported as NULL
                return None

        self.cb = _ALLOC(_cb)


class ScratchBlocks:
    """Forward-only scratch for gsr_rasterize_forward_ex: every block the
    callback hands out is kept until the forward returns, then dropped (the
    caching allocator reuses it in stream order), so it is not saved for the
    backward as the binning buffer is."""

    def __init__(self, device):
        self.device = device
        self.blocks = []

        def _cb(_ctx, n):
            try:
                t = torch.empty(max(int(n), 1), dtype=torch.uint8, device=self.device)
                self.blocks.append(t)
                return t.data_ptr()
            except Exception:  # noqa: BLE001 - allocation failure is reported as NULL
                return None

        self.cb = _ALLOC(_cb)


# ---- stage times (measurement hooks) -----------------------------------------------------------------------------

def stage_buffer(on):
    """The `stage_ms` argument of a call: 8 host floats when measuring (the call then synchronises), else NULL."""
    return (c_float * 8)() if on else None


def stage_stats(stages, ms, scratch=None, **extra):
    """The stats of one call as gsr_tnt returns them: stage_ms {stage: GPU ms} (None when not measured), the
    scratch_bytes of all blocks together, and `extra`."""
    return dict(stage_ms=None if ms is None else {k: float(ms[n]) for n, k in enumerate(stages)},
                scratch_bytes=sum(int(b.numel()) for b in scratch.blocks) if scratch is not None else 0, **extra)


def record_stats(hook, stages, ms, scratch, **extra):
    """The `last_call_stats` hooks of gsr_mesh, gsr_eval and gsr_tsdf: a dict `hook` is refilled with the
    stage times by name, scratch_bytes block by block, and `extra`; None is left alone."""
    if hook is not None:
        hook.clear()
        hook.update(stage_stats(stages, ms)["stage_ms"], scratch_bytes=[int(b.numel()) for b in scratch.blocks],
                    **extra)


# ---- tensor checks shared by the mesh, TSDF and evaluation modules ------------------------------------------------

def require(t, name, dtypes, ndim, who):
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise RuntimeError(f"{who}: `{name}` must be a HIP device tensor")
    if t.dtype not in dtypes:
        raise RuntimeError(f"{who}: `{name}` must be {' or '.join(str(d) for d in dtypes)} "
                           f"(got {t.dtype})")
    if t.dim() != ndim:
        raise RuntimeError(f"{who}: `{name}` must have {ndim} dimensions (got {tuple(t.shape)})")


def require_points(t, name, who):
    require(t, name, (torch.float64,), 2, who)
    if t.size(1) != 3:
        raise RuntimeError(f"{who}: `{name}` must have shape (N, 3) (got {tuple(t.shape)})")


def require_mesh(vertices, faces, who, vertices_optional=False):
    require(faces, "faces", (torch.int32, torch.int64), 2, who)
    if faces.size(1) != 3:
        raise RuntimeError(f"{who}: `faces` must have shape (F, 3) (got {tuple(faces.shape)})")
    if vertices is None and vertices_optional:
        return
    require(vertices, "vertices", (torch.float32,), 2, who)
    if vertices.size(1) != 3:
        raise RuntimeError(f"{who}: `vertices` must have shape (V, 3) (got {tuple(vertices.shape)})")
    if vertices.device != faces.device:
        raise RuntimeError(f"{who}: `vertices` and `faces` must be on one device")
