"""`_C` — the extension entry points of the reference, bound to libgsr.so.

Mirrors the pybind module of the reference (DGR/ext.cpp:15-23) with the same
names, argument order, return tuples and error behaviour:

  rasterize_gaussians(25 args)           -> (num_rendered, color, alpha, normal, mdepth, radii,
                                             geomBuffer, binningBuffer, imgBuffer, tileBuffer)
                                             (DGR/rasterize_points.cu:39-139)
  rasterize_gaussians_backward(35 args)  -> (dmeans2D, dcolors, dopacity, dmeans3D, dcov3D, dsh,
                                             dsg_axis, dsg_sharpness, dsg_color, dscales, drotations)
                                             (DGR/rasterize_points.cu:141-258)
  mark_visible(means3D, view, proj)      -> bool[P]  (DGR/rasterize_points.cu:260-277)
  sample_rasterized_depth(17 args)       -> (num_rendered, num_points, num_duplicated_tiles, output, inside,
                                             geomBuffer, binningBuffer, pointBuffer, pointBinningBuffer,
                                             tileBuffer, duplicatedTileBuffer)  (DGR/rasterize_points.cu:459-553)
  sample_rasterized_depth_backward(28)   -> (dopacity, dmeans3D, dcov3D, dscales, drotations, dpoints3D)
                                             (DGR/rasterize_points.cu:555-633)

The C ABI (include/gsr.h) takes raw device pointers and allocation callbacks;
here torch provides the memory (caching allocator), the current HIP stream and
the uint8 scratch tensors that autograd keeps alive between forward and
backward.  There is no CPU fallback: inputs must be HIP (cuda) tensors and the
shared library must load, otherwise these functions raise.
"""
from __future__ import annotations

import ctypes

import torch

# (the binding itself is _abi; its names are re-exported here under the ones callers and tests know, and
# this module's functions take _ScratchBlocks from these globals, where a test may replace it)
from ._abi import _ALLOC, _CHUNK, ABI_VERSION, LIB_PATH, AdamGroup, Out, call, loaded_library_path  # noqa: F401
from ._abi import ScratchBlocks as _ScratchBlocks, check as _check, load as _load, ptr as _ptr, stream as _stream

NUM_STAGES = 14
# debugging aid: keep the last backward's accumulator buffer (gsr_api.hip
# carve_bwd layout: 256-B aligned base, float acc[P][16], then float acc_abs[P])
KEEP_BWD_SCRATCH = False
last_bwd_scratch = None
# (ids 0, 2-4, 7, 8: retired variants and diagnostics, rejected by gsr_set_option)
OPT_RENDER_STATS = 1
OPT_NO_REFINE = 5
OPT_BWD_NO_CACHE = 6
OPT_ROCPRIM_DSORT = 9
OPT_PBWD_STAGE = 10


def backward_chunk_size(P: int, chunks: int) -> int:
    """The Gaussian range size of a backward run in `chunks` ranges
    (gsr_backward_chunk_size; host only, no GPU needed)."""
    n = _load().gsr_backward_chunk_size(int(P), int(chunks))
    if n < 0:
        raise RuntimeError(f"gsr: backward_chunk_size({P}, {chunks}): P must be >= 0 and chunks >= 1")
    return n


def debug_render_stats(reset: bool = True) -> list:
    """Counters of forward launches made with OPT_RENDER_STATS (render_fwd.hip)."""
    out = (ctypes.c_ulonglong * 20)()
    _check(_load().gsr_debug_render_stats(out, int(bool(reset))))
    return list(out)


def debug_binning(binningBuffer, tileBuffer, R: int, image_height: int, image_width: int, with_list: bool = True):
    """(point_list [R] uint32, ranges [tiles, 2] uint32) of a forward's buffers
    (gsr_debug_binning), as numpy arrays.  The per-tile lists hold only the
    instances that survive tile culling: their count is ranges[:, 1].max(),
    R (= num_rendered, the reference's K) is the capacity."""
    import numpy as np

    tiles = ((image_width + 15) // 16) * ((image_height + 15) // 16)
    plist = np.zeros(max(R, 0) if with_list else 0, np.uint32)
    ranges = np.zeros((tiles, 2), np.uint32)
    stream = torch.cuda.current_stream(binningBuffer.device).cuda_stream
    _check(_load().gsr_debug_binning(ctypes.c_void_p(binningBuffer.data_ptr()),
                                     ctypes.c_void_p(tileBuffer.data_ptr()), int(R), int(image_width),
                                     int(image_height), plist.ctypes.data_as(ctypes.c_void_p) if with_list else None,
                                     ranges.ctypes.data_as(ctypes.c_void_p), ctypes.c_void_p(stream)))
    return plist, ranges


def debug_n_contrib(imgBuffer, image_height: int, image_width: int):
    """Per-pixel last contributor [H, W] uint32 of a forward's image buffer
    (gsr_debug_image): 1-based positions in the culled per-tile lists of
    debug_binning."""
    import numpy as np

    out = np.zeros((image_height, image_width), np.uint32)
    stream = torch.cuda.current_stream(imgBuffer.device).cuda_stream
    _check(_load().gsr_debug_image(ctypes.c_void_p(imgBuffer.data_ptr()), int(image_width), int(image_height),
                                   out.ctypes.data_as(ctypes.c_void_p), ctypes.c_void_p(stream)))
    return out


def debug_max_contrib(tileBuffer, image_height: int, image_width: int):
    """Per-tile max contributor [tiles] uint32 of a forward's tile buffer
    (gsr_debug_tile_stats): how far into each culled tile list the forward's
    pixels blended, the range the backward walks."""
    import numpy as np

    tiles = ((image_width + 15) // 16) * ((image_height + 15) // 16)
    out = np.zeros(tiles, np.uint32)
    stream = torch.cuda.current_stream(tileBuffer.device).cuda_stream
    _check(_load().gsr_debug_tile_stats(ctypes.c_void_p(tileBuffer.data_ptr()), int(image_width), int(image_height),
                                        out.ctypes.data_as(ctypes.c_void_p), ctypes.c_void_p(stream)))
    return out


def debug_sample_points(pointBuffer, PN: int):
    """(median depth along the ray [PN] float32, last contributor [PN] uint32)
    of a sample_rasterized_depth forward's point buffer (gsr_debug_sample_points)."""
    import numpy as np

    md = np.zeros(PN, np.float32)
    last = np.zeros(PN, np.uint32)
    stream = torch.cuda.current_stream(pointBuffer.device).cuda_stream
    _check(_load().gsr_debug_sample_points(ctypes.c_void_p(pointBuffer.data_ptr()), int(PN),
                                           md.ctypes.data_as(ctypes.c_void_p), last.ctypes.data_as(ctypes.c_void_p),
                                           ctypes.c_void_p(stream)))
    return md, last


def debug_depth_sort_tile_keys(P: int) -> int:
    """Keys per workgroup tile of dsort.hip for P keys (gsr_debug_depth_sort_tile_keys;
    host only, no GPU needed)."""
    n = _load().gsr_debug_depth_sort_tile_keys(int(P))
    if n < 0:
        raise RuntimeError(f"gsr: debug_depth_sort_tile_keys({P}): P must be >= 0")
    return n


def debug_depth_sort_bytes(P: int) -> int:
    """Scratch bytes of debug_depth_sort for P keys (gsr_debug_depth_sort_bytes; host only)."""
    n = _load().gsr_debug_depth_sort_bytes(int(P))
    if n < 0:
        raise RuntimeError(f"gsr: debug_depth_sort_bytes({P}): P must be >= 0")
    return n


def debug_depth_sort(keys, prepared: bool = True):
    """(order [P] int32, keys_sorted [P]) = the depth sort of the render path
    (gsr_debug_depth_sort) on the caller's 32-bit keys, taken as unsigned bit
    patterns: the stable ascending order, values = index.  `prepared`: the
    state cleared and the histograms counted as the render path does, else by
    the sort's own kernels.  No host synchronisation."""
    bits32 = (torch.int32,) + ((torch.uint32,) if hasattr(torch, "uint32") else ())
    if not isinstance(keys, torch.Tensor) or not keys.is_cuda:
        raise RuntimeError("gsr debug_depth_sort: `keys` must be a HIP device tensor")
    if keys.dtype not in bits32 or keys.dim() != 1:
        raise RuntimeError(f"gsr debug_depth_sort: `keys` must be a 1-D int32 / uint32 tensor (got {keys.dtype}, "
                           f"{keys.dim()}-D)")
    if not keys.is_contiguous():
        raise RuntimeError("gsr debug_depth_sort: `keys` must be contiguous")
    P = keys.numel()
    if P >= 2 ** 31:
        raise RuntimeError("gsr debug_depth_sort: at most 2^31 - 1 keys")
    order = torch.empty(P, dtype=torch.int32, device=keys.device)
    keys_sorted = torch.empty_like(keys)
    if P == 0:
        return order, keys_sorted
    scratch = torch.empty(_load().gsr_debug_depth_sort_bytes(P), dtype=torch.uint8, device=keys.device)
    call(keys.device, "gsr_debug_depth_sort", P, _ptr(keys), _ptr(keys_sorted), _ptr(order), _ptr(scratch),
         int(bool(prepared)), _stream(keys.device))
    return order, keys_sorted


LIST_CONSTANTS = ("kRowSeg", "kRowSegBig", "kRowSegBigP", "kTileSeg", "kRecSpans", "kCoopCap", "kEmitCapW",
                  "kEmitPlanes", "kCoopMaxGx", "kCoopBlocks", "kTileBlocks", "kScanTile", "kScanItems", "kMaxGrid")


def debug_list_constants() -> dict:
    """The structural constants of csrc/tilelists.hip by name (gsr_debug_list_constants;
    host only, no GPU needed)."""
    out = (ctypes.c_int * len(LIST_CONSTANTS))()
    n = _load().gsr_debug_list_constants(out, len(LIST_CONSTANTS))
    if n != len(LIST_CONSTANTS):
        raise RuntimeError(f"gsr: debug_list_constants: the library has {n} constants, these bindings name "
                           f"{len(LIST_CONSTANTS)}")
    return dict(zip(LIST_CONSTANTS, out))


def debug_scan_excl_bytes(cap: int) -> int:
    """Scratch bytes of debug_scan_excl for a bound of `cap` words (gsr_debug_scan_excl_bytes; host only)."""
    n = _load().gsr_debug_scan_excl_bytes(int(cap))
    if n < 0:
        raise RuntimeError(f"gsr: debug_scan_excl_bytes({cap}): cap must be in [0, 2^31)")
    return n


def debug_scan_excl(inp, out, cap: int, n: int = 0, n_dev=None, mul: int = 1) -> None:
    """The tile lists' device-sized exclusive scan alone (gsr_debug_scan_excl), in place on the caller's
    tensors: out[0:N] = the exclusive prefix sums (mod 2^32) of inp[0:N], out[N] = their total, with
    N = `n`, or mul * n_dev[0] read on the device when the one-word tensor `n_dev` is given.  `cap` >= N is
    the host's bound that sizes the launch; inp holds at least cap words and is 16-byte aligned, out at
    least cap + 1.  Nothing of inp past N is read and nothing of out past N written."""
    bits32 = (torch.int32,) + ((torch.uint32,) if hasattr(torch, "uint32") else ())
    for name, t, words in (("inp", inp, int(cap)), ("out", out, int(cap) + 1)) + (
            (("n_dev", n_dev, 1),) if n_dev is not None else ()):
        if not isinstance(t, torch.Tensor) or not t.is_cuda:
            raise RuntimeError(f"gsr debug_scan_excl: `{name}` must be a HIP device tensor")
        if t.dtype not in bits32 or t.dim() != 1:
            raise RuntimeError(f"gsr debug_scan_excl: `{name}` must be a 1-D int32 / uint32 tensor (got {t.dtype}, "
                               f"{t.dim()}-D)")
        if not t.is_contiguous():
            raise RuntimeError(f"gsr debug_scan_excl: `{name}` must be contiguous")
        if t.numel() < words:
            raise RuntimeError(f"gsr debug_scan_excl: `{name}` holds {t.numel()} words, needs {words}")
    if inp.data_ptr() % 16:
        raise RuntimeError("gsr debug_scan_excl: `inp` must be 16-byte aligned")
    cap, mul = int(cap), int(mul)
    N = int(n) if n_dev is None else mul * (int(n_dev[0].item()) & 0xFFFFFFFF)  # (a test hook: one readback)
    if not 0 <= N <= cap or not 0 <= mul < 2 ** 32:
        raise RuntimeError(f"gsr debug_scan_excl: length {N} outside [0, cap = {cap}]")
    sums = torch.empty(debug_scan_excl_bytes(cap), dtype=torch.uint8, device=inp.device)
    call(inp.device, "gsr_debug_scan_excl", ctypes.c_void_p(inp.data_ptr()), ctypes.c_void_p(out.data_ptr()), cap,
         0 if n_dev is not None else N, None if n_dev is None else ctypes.c_void_p(n_dev.data_ptr()), mul, _ptr(sums),
         _stream(inp.device))


def set_option(opt: int, value: int) -> None:
    """Select an A/B kernel variant (gsr_set_option); variants are bit-identical."""
    _check(_load().gsr_set_option(int(opt), int(value)))


def timing_enable(on: bool = True) -> None:
    """Bracket every kernel stage with hipEvents on its stream (gsr_timing_enable)."""
    _load().gsr_timing_enable(int(bool(on)))


def timing_stages(names=None) -> None:
    """Time only the named stages (None: all), gsr_timing_stage_mask."""
    L = _load()
    if names is None:
        mask = 0xFFFFFFFF
    else:
        idx = {L.gsr_stage_name(k).decode(): k for k in range(NUM_STAGES)}
        mask = sum(1 << idx[n] for n in set(names))
    _check(L.gsr_timing_stage_mask(mask))


def timing_collect() -> dict:
    """{stage name: (total ms, launches)} since the last collect (gsr_timing_collect)."""
    L = _load()
    ms = (ctypes.c_double * NUM_STAGES)()
    n = (ctypes.c_int * NUM_STAGES)()
    _check(L.gsr_timing_collect(ms, n))
    return {L.gsr_stage_name(k).decode(): (ms[k], n[k]) for k in range(NUM_STAGES)}


def _ByteBuffer(device, zero: bool = False):
    """A resizable torch.uint8 device tensor handed to the C ABI as a callback
    (replaces resizeFunctional, DGR/rasterize_points.cu:27-37): Out for uint8,
    under the name callers outside this module know."""
    return Out(device, torch.uint8, zero)


def _dev_contig(t, name):
    if t is None:
        return None
    if t.numel() == 0:
        return t
    if not t.is_cuda:
        raise RuntimeError(f"gsr: `{name}` must be a HIP device tensor (got {t.device})")
    if t.dtype != torch.float32 and name not in ("radii",):
        raise RuntimeError(f"gsr: `{name}` must be float32 (got {t.dtype})")
    return t.contiguous()


def _split_rest(sh, sh_rest, P):
    """The rest rows of the split SH layout, checked, or None (one [P, M, 3] tensor)."""
    if sh_rest is None:
        return None
    if sh is None or sh.numel() == 0 or tuple(sh.shape) != (P, 1, 3) or sh_rest.dim() != 3 or \
            sh_rest.size(0) != P or sh_rest.size(2) != 3 or sh_rest.size(1) < 1:
        raise RuntimeError("gsr: split SH rows are sh [P, 1, 3] and sh_rest [P, M-1, 3]")
    return _dev_contig(sh_rest, "sh_rest")


def rasterize_gaussians(background, means3D, colors, opacity, scales, rotations, cov3D_precomp, sh, sg_axis,
                        sg_sharpness, sg_color, sh_degree, sg_degree, scale_modifier, viewmatrix, projmatrix,
                        tan_fovx, tan_fovy, kernel_size, image_height, image_width, campos, prefiltered,
                        require_depth, debug, sh_rest=None):
    """The reference's 25 arguments (rasterize_points.cu:36-139).  `sh_rest`
    (not in the reference): the split SH layout of training — `sh` the DC
    rows [P, 1, 3] and `sh_rest` the rest [P, M-1, 3] as GaussianModel keeps
    them, without their concatenation (gsr_rasterize_forward_ex2)."""
    if means3D.ndimension() != 2 or means3D.size(1) != 3:
        raise RuntimeError("means3D must have dimensions (num_points, 3)")
    P = means3D.size(0)
    H, W = int(image_height), int(image_width)
    dev = means3D.device
    fopt = dict(dtype=torch.float32, device=dev)
    if P == 0:  # rasterize_points.cu:77-95: zero outputs, nothing rendered
        bufs = [torch.empty(0, dtype=torch.uint8, device=dev) for _ in range(4)]
        return (0, torch.zeros(3, H, W, **fopt), torch.zeros(1, H, W, **fopt), torch.zeros(3, H, W, **fopt),
                torch.zeros(1, H, W, **fopt), torch.zeros(0, dtype=torch.int32, device=dev), *bufs)
    args = {k: _dev_contig(v, k) for k, v in dict(
        background=background, means3D=means3D, colors=colors, opacity=opacity, scales=scales,
        rotations=rotations, cov3D_precomp=cov3D_precomp, sh=sh, sg_axis=sg_axis, sg_sharpness=sg_sharpness,
        sg_color=sg_color, viewmatrix=viewmatrix, projmatrix=projmatrix, campos=campos).items()}
    SHM = sh.size(1) if sh is not None and sh.size(0) != 0 else 0
    SGM = sg_color.size(1) if sg_color is not None and sg_color.size(0) != 0 else 0
    rest = _split_rest(sh, sh_rest, P)
    if rest is not None:
        SHM = 1 + sh_rest.size(1)
    color = torch.empty(3, H, W, **fopt)
    mdepth = torch.empty(1, H, W, **fopt)
    alpha = torch.empty(1, H, W, **fopt)
    normal = torch.empty(3, H, W, **fopt)
    radii = torch.empty(P, dtype=torch.int32, device=dev)
    bufs = [Out(dev, torch.uint8) for _ in range(4)]
    scratch = _ScratchBlocks(dev)
    K = ctypes.c_int(0)
    call(dev, "gsr_rasterize_forward_ex2",
         bufs[0].cb, None, bufs[1].cb, None, bufs[2].cb, None, bufs[3].cb, None,
         P, int(sh_degree), SHM, int(sg_degree), SGM, _ptr(args["background"]), W, H, _ptr(args["means3D"]),
         _ptr(args["colors"]), _ptr(args["opacity"]), _ptr(args["scales"]), _ptr(args["rotations"]),
         _ptr(args["cov3D_precomp"]), _ptr(args["sh"]), _ptr(args["sg_axis"]), _ptr(args["sg_sharpness"]),
         _ptr(args["sg_color"]), float(scale_modifier), _ptr(args["viewmatrix"]), _ptr(args["projmatrix"]),
         _ptr(args["campos"]), float(tan_fovx), float(tan_fovy), float(kernel_size), int(bool(prefiltered)),
         _ptr(color), _ptr(mdepth), _ptr(alpha), _ptr(normal), _ptr(radii), int(bool(require_depth)),
         int(bool(debug)), _stream(dev), ctypes.byref(K), scratch.cb, None, _ptr(rest))
    del scratch
    return (K.value, color, alpha, normal, mdepth, radii, bufs[0].tensor, bufs[1].tensor, bufs[2].tensor,
            bufs[3].tensor)


def rasterize_gaussians_backward(background, means3D, colors, opacity, scales, rotations, cov3D_precomp, sh,
                                 sg_axis, sg_sharpness, sg_color, sh_degree, sg_degree, scale_modifier, viewmatrix,
                                 projmatrix, tan_fovx, tan_fovy, kernel_size, dL_dout_color, dL_dout_mdepth,
                                 dL_dout_alpha, dL_dout_normal, alphas, normalmap, mdepth, campos, radii,
                                 geomBuffer, R, binningBuffer, imageBuffer, tileBuffer, require_depth, debug,
                                 exchange=None, sh_rest=None):
    """The reference's 35 arguments and 11 gradients (rasterize_points.cu:141-258).
    `exchange` (not in the reference; gsr_dist.OverlappedViewGrads) runs the
    per-Gaussian backward in exchange.chunks Gaussian ranges through
    gsr_rasterize_backward_ex and calls exchange.on_chunk(begin, end, grads)
    after each range is queued; with exchange.dc_rows(...) a buffer, only the
    DC gradient rows are written there (the SH / SG rows are the exchange's to
    rebuild before the gradients are used).  `sh_rest` (the split SH layout,
    see rasterize_gaussians): dsh is then [P, 1, 3] and a 12th gradient,
    dsh_rest [P, M-1, 3], is returned (gsr_rasterize_backward_ex2)."""
    P = means3D.size(0)
    img = dL_dout_color if dL_dout_color is not None else alphas  # (a None upstream gradient is zero)
    H, W = img.size(1), img.size(2)
    SHM = sh.size(1) if sh is not None and sh.size(0) != 0 else 0
    SGM = sg_color.size(1) if sg_color is not None and sg_color.size(0) != 0 else 0
    rest = _split_rest(sh, sh_rest, P)
    dev = means3D.device
    fopt = dict(dtype=torch.float32, device=dev)
    alloc = torch.zeros if P == 0 else torch.empty  # the kernels overwrite every element
    outs = dict(dmeans3D=alloc(P, 3, **fopt), dmeans2D=alloc(P, 3, **fopt), dcolors=alloc(P, 3, **fopt),
                dopacity=alloc(P, 1, **fopt), dcov3D=alloc(P, 6, **fopt), dsh=alloc(P, SHM, 3, **fopt),
                dsg_axis=alloc(P, SGM, 3, **fopt), dsg_sharpness=alloc(P, SGM, **fopt),
                dsg_color=alloc(P, SGM, 3, **fopt), dscales=alloc(P, 3, **fopt), drotations=alloc(P, 4, **fopt))
    if rest is not None:
        outs["dsh_rest"] = alloc(*sh_rest.shape, **fopt)
        SHM = 1 + sh_rest.size(1)
    if P == 0:  # (SHM and SGM read 0 above: an empty gradient still has its input's shape, [0, M, 3])
        for k, t in (("dsh", sh), ("dsg_axis", sg_axis), ("dsg_sharpness", sg_sharpness), ("dsg_color", sg_color)):
            if t is not None and t.dim() == outs[k].dim():
                outs[k] = torch.zeros(t.shape, **fopt)
    if P != 0:
        a = {k: _dev_contig(v, k) for k, v in dict(
            background=background, means3D=means3D, colors=colors, opacity=opacity, scales=scales,
            rotations=rotations, cov3D_precomp=cov3D_precomp, sh=sh, sg_axis=sg_axis, sg_sharpness=sg_sharpness,
            sg_color=sg_color, viewmatrix=viewmatrix, projmatrix=projmatrix, campos=campos, alphas=alphas,
            normalmap=normalmap, mdepth=mdepth, dL_dout_color=dL_dout_color, dL_dout_mdepth=dL_dout_mdepth,
            dL_dout_alpha=dL_dout_alpha, dL_dout_normal=dL_dout_normal).items()}
        radii = radii.contiguous()
        scratch = Out(dev, torch.uint8)
        grads = (outs["dmeans2D"], outs["dcolors"], outs["dopacity"], outs["dmeans3D"], outs["dcov3D"], outs["dsh"],
                 outs["dsg_axis"], outs["dsg_sharpness"], outs["dsg_color"], outs["dscales"], outs["drotations"])
        chunks, dc = 1, None
        hook = _CHUNK()  # NULL
        if exchange is not None:
            chunks = max(1, int(exchange.chunks))
            dc = exchange.dc_rows(P, dev) if SHM else None
            cb = exchange.hook(grads)  # (errors held by the exchange, raised by settle below)
            hook = _CHUNK(lambda _ctx, b, e: cb(b, e))
        with torch.cuda.device(dev):  # (not call(): the exchange settles on the status before it is raised)
            rc = _load().gsr_rasterize_backward_ex2(
                scratch.cb, None, P, int(sh_degree), SHM, int(sg_degree), SGM, int(R), _ptr(a["background"]), W, H,
                _ptr(a["means3D"]), _ptr(a["colors"]), _ptr(a["opacity"]), _ptr(a["scales"]), _ptr(a["rotations"]),
                _ptr(a["cov3D_precomp"]), _ptr(a["sh"]), _ptr(a["sg_axis"]), _ptr(a["sg_sharpness"]),
                _ptr(a["sg_color"]), float(scale_modifier), _ptr(a["viewmatrix"]), _ptr(a["projmatrix"]),
                _ptr(a["campos"]), float(tan_fovx), float(tan_fovy), float(kernel_size), _ptr(radii),
                _ptr(a["alphas"]), _ptr(a["normalmap"]), _ptr(a["mdepth"]), _ptr(geomBuffer), _ptr(binningBuffer),
                _ptr(imageBuffer), _ptr(tileBuffer), _ptr(a["dL_dout_color"]), _ptr(a["dL_dout_mdepth"]),
                _ptr(a["dL_dout_alpha"]), _ptr(a["dL_dout_normal"]), _ptr(outs["dmeans3D"]), _ptr(outs["dmeans2D"]),
                _ptr(outs["dcolors"]), _ptr(outs["dopacity"]), _ptr(outs["dscales"]), _ptr(outs["drotations"]),
                _ptr(outs["dcov3D"]), _ptr(outs["dsh"]), _ptr(outs["dsg_axis"]), _ptr(outs["dsg_sharpness"]),
                _ptr(outs["dsg_color"]), int(bool(require_depth)), int(bool(debug)), chunks, hook, None,
                None if dc is None else _ptr(dc), _stream(dev), _ptr(rest), _ptr(outs.get("dsh_rest")))
        if exchange is not None:  # a failed backward still posts every range's collectives (no peer blocks)
            exchange.settle(rc == 0)
        _check(rc)
        if KEEP_BWD_SCRATCH:
            global last_bwd_scratch
            last_bwd_scratch = scratch.tensor
    g = (outs["dmeans2D"], outs["dcolors"], outs["dopacity"], outs["dmeans3D"], outs["dcov3D"], outs["dsh"],
         outs["dsg_axis"], outs["dsg_sharpness"], outs["dsg_color"], outs["dscales"], outs["drotations"])
    return g if rest is None else g + (outs["dsh_rest"],)


def mark_visible(means3D, viewmatrix, projmatrix):
    P = means3D.size(0)
    present = torch.zeros(P, dtype=torch.bool, device=means3D.device)
    if P != 0:
        m = _dev_contig(means3D, "means3D")
        v = _dev_contig(viewmatrix, "viewmatrix")
        p = _dev_contig(projmatrix, "projmatrix")
        call(means3D.device, "gsr_mark_visible", P, _ptr(m), _ptr(v), _ptr(p), _ptr(present),
             _stream(means3D.device))
    return present


def _point_query(fn, points3D, means3D, opacity, scales, rotations, scale_modifier, cov3D_precomp,
                 view2gaussian_precomp, viewmatrix, projmatrix, tan_fovx, tan_fovy, kernel_size, image_height,
                 image_width, campos, prefiltered, debug):
    """IntegrateGaussiansToPointsCUDA / evaluateSDFfromSingleView
    (DGR/rasterize_points.cu:279-457): outputs zero-filled (torch::full 0),
    the scratch buffers are local to the call."""
    if means3D.ndimension() != 2 or means3D.size(1) != 3:
        raise RuntimeError("means3D must have dimensions (num_points, 3)")
    if points3D.ndimension() != 2 or points3D.size(1) != 3:
        raise RuntimeError("points3D must have dimensions (num_points, 3)")
    PN, P = points3D.size(0), means3D.size(0)
    dev = means3D.device
    out0 = torch.zeros(PN, dtype=torch.float32, device=dev)
    out1 = torch.zeros(PN, dtype=torch.float32, device=dev)
    inside = torch.zeros(PN, dtype=torch.bool, device=dev)
    K = ctypes.c_int(0)
    if P != 0 and PN != 0:
        a = {k: _dev_contig(v, k) for k, v in dict(
            points3D=points3D, means3D=means3D, opacity=opacity, scales=scales, rotations=rotations,
            cov3D_precomp=cov3D_precomp, view2gaussian_precomp=view2gaussian_precomp, viewmatrix=viewmatrix,
            projmatrix=projmatrix, campos=campos).items()}
        bufs = [Out(dev, torch.uint8) for _ in range(6)]
        head = [bufs[0].cb, None, bufs[1].cb, None, bufs[2].cb, None, bufs[3].cb, None, bufs[4].cb, None,
                bufs[5].cb, None, PN, P, int(image_width), int(image_height), _ptr(a["points3D"]),
                _ptr(a["means3D"]), _ptr(a["opacity"]), _ptr(a["scales"]), float(scale_modifier),
                _ptr(a["rotations"]), _ptr(a["cov3D_precomp"]), _ptr(a["view2gaussian_precomp"]),
                _ptr(a["viewmatrix"]), _ptr(a["projmatrix"]), _ptr(a["campos"]), float(tan_fovx), float(tan_fovy),
                float(kernel_size), int(bool(prefiltered))]
        outs = [_ptr(out0)] if fn == "integrate" else [_ptr(out0), _ptr(out1)]
        call(dev, "gsr_integrate_forward" if fn == "integrate" else "gsr_evaluate_sdf_forward", *head, *outs,
             _ptr(inside), int(bool(debug)), _stream(dev), ctypes.byref(K))
    return K.value, out0, out1, inside


def integrate_gaussians_to_points(points3D, means3D, opacity, scales, rotations, scale_modifier, cov3D_precomp,
                                  view2gaussian_precomp, viewmatrix, projmatrix, tan_fovx, tan_fovy, kernel_size,
                                  image_height, image_width, campos, prefiltered, debug):
    """-> (num_rendered, transmittance [PN], inside [PN] bool), rasterize_points.cu:279-366."""
    K, T, _, inside = _point_query("integrate", points3D, means3D, opacity, scales, rotations, scale_modifier,
                                   cov3D_precomp, view2gaussian_precomp, viewmatrix, projmatrix, tan_fovx, tan_fovy,
                                   kernel_size, image_height, image_width, campos, prefiltered, debug)
    return K, T, inside


def evaluate_sdf_from_signle_view(points3D, means3D, opacity, scales, rotations, scale_modifier, cov3D_precomp,
                                  view2gaussian_precomp, viewmatrix, projmatrix, tan_fovx, tan_fovy, kernel_size,
                                  image_height, image_width, campos, prefiltered, debug):
    """-> (num_rendered, depth [PN], sdf [PN], inside [PN] bool), rasterize_points.cu:368-457
    (the reference's spelling of the binding name, DGR/ext.cpp)."""
    return _point_query("sdf", points3D, means3D, opacity, scales, rotations, scale_modifier, cov3D_precomp,
                        view2gaussian_precomp, viewmatrix, projmatrix, tan_fovx, tan_fovy, kernel_size,
                        image_height, image_width, campos, prefiltered, debug)


# (measurement hook, bench.py --e2e: the last sample_rasterized_depth call's points, camera and outputs, for
# the SAMPLE raster's algorithmic bytes)
CAPTURE_SAMPLE = False
last_sample = None


def sample_rasterized_depth(points3D, means3D, opacity, scales, rotations, scale_modifier, cov3D_precomp,
                            viewmatrix, projmatrix, tan_fovx, tan_fovy, kernel_size, image_height, image_width,
                            campos, prefiltered, debug):
    if means3D.ndimension() != 2 or means3D.size(1) != 3:
        raise RuntimeError("means3D must have dimensions (num_points, 3)")
    if points3D.ndimension() < 1 or points3D.size(-1) != 3:
        raise RuntimeError("points3D must have shape (..., 3) with last dimension == 3")
    PN = points3D.numel() // 3
    P = means3D.size(0)
    H, W = int(image_height), int(image_width)
    dev = means3D.device
    output = torch.zeros_like(points3D)
    inside = torch.zeros(points3D.shape[:-1], dtype=torch.bool, device=points3D.device)
    bufs = [Out(dev, torch.uint8) for _ in range(6)]
    scratch = _ScratchBlocks(dev)
    K, RN, TN = ctypes.c_int(0), ctypes.c_int(0), ctypes.c_int(0)
    if P != 0 and PN != 0:
        a = {k: _dev_contig(v, k) for k, v in dict(
            points3D=points3D, means3D=means3D, opacity=opacity, scales=scales, rotations=rotations,
            cov3D_precomp=cov3D_precomp, viewmatrix=viewmatrix, projmatrix=projmatrix, campos=campos).items()}
        call(dev, "gsr_sample_depth_forward_ex",
             bufs[0].cb, None, bufs[1].cb, None, bufs[2].cb, None, bufs[3].cb, None, bufs[4].cb, None,
             bufs[5].cb, None, PN, P, W, H, _ptr(a["points3D"]), _ptr(a["means3D"]), _ptr(a["opacity"]),
             _ptr(a["scales"]), float(scale_modifier), _ptr(a["rotations"]), _ptr(a["cov3D_precomp"]),
             _ptr(a["viewmatrix"]), _ptr(a["projmatrix"]), _ptr(a["campos"]), float(tan_fovx), float(tan_fovy),
             float(kernel_size), int(bool(prefiltered)), _ptr(output), _ptr(inside), int(bool(debug)),
             _stream(dev), ctypes.byref(K), ctypes.byref(RN), ctypes.byref(TN), scratch.cb, None)
        del scratch
    res = (K.value, RN.value, TN.value, output, inside, *[b.tensor for b in bufs])
    if CAPTURE_SAMPLE:
        global last_sample
        last_sample = dict(points3D=points3D, projmatrix=projmatrix, H=H, W=W, out=res)
    return res


def sample_rasterized_depth_backward(points3D, means3D, opacity, scales, rotations, scale_modifier, cov3D_precomp,
                                     viewmatrix, projmatrix, inside, dL_doutput, tan_fovx, tan_fovy, kernel_size,
                                     image_height, image_width, campos, geomBuffer, binningBuffer, pointBuffer,
                                     pointBinningBuffer, tileBuffer, duplicatedTileBuffer, R, RN, TN, prefiltered,
                                     debug):
    PN = points3D.numel() // 3
    P = means3D.size(0)
    dev = means3D.device
    fopt = dict(dtype=torch.float32, device=dev)
    alloc = torch.zeros if (P == 0 or PN == 0) else torch.empty  # the kernels overwrite every element
    outs = dict(dopacity=alloc(P, 1, **fopt), dmeans3D=alloc(P, 3, **fopt), dcov3D=alloc(P, 6, **fopt),
                dscales=alloc(P, 3, **fopt), drotations=alloc(P, 4, **fopt), dpoints3D=torch.zeros_like(points3D))
    if P != 0 and PN != 0:
        a = {k: _dev_contig(v, k) for k, v in dict(
            points3D=points3D, means3D=means3D, opacity=opacity, scales=scales, rotations=rotations,
            cov3D_precomp=cov3D_precomp, viewmatrix=viewmatrix, projmatrix=projmatrix, campos=campos,
            dL_doutput=dL_doutput).items()}
        ins = inside.contiguous()
        if not ins.is_cuda or ins.dtype != torch.bool:
            raise RuntimeError("gsr: `inside` must be the forward's bool device tensor")
        scratch = Out(dev, torch.uint8)
        call(dev, "gsr_sample_depth_backward",
             scratch.cb, None, PN, P, int(RN), int(R), int(TN), int(image_width), int(image_height),
             _ptr(a["points3D"]), _ptr(a["means3D"]), _ptr(a["opacity"]), _ptr(a["scales"]), float(scale_modifier),
             _ptr(a["rotations"]), _ptr(a["cov3D_precomp"]), _ptr(a["viewmatrix"]), _ptr(a["projmatrix"]),
             _ptr(a["campos"]), float(tan_fovx), float(tan_fovy), float(kernel_size), _ptr(geomBuffer),
             _ptr(binningBuffer), _ptr(pointBuffer), _ptr(pointBinningBuffer), _ptr(tileBuffer),
             _ptr(duplicatedTileBuffer), _ptr(ins), _ptr(a["dL_doutput"]), _ptr(outs["dopacity"]),
             _ptr(outs["dmeans3D"]), _ptr(outs["dcov3D"]), _ptr(outs["dscales"]), _ptr(outs["drotations"]),
             _ptr(outs["dpoints3D"]), int(bool(debug)), _stream(dev))
    return (outs["dopacity"], outs["dmeans3D"], outs["dcov3D"], outs["dscales"], outs["drotations"],
            outs["dpoints3D"])


MAX_ADAM_GROUPS = 16


def adam_step(tensors, lrs, step: float, beta1: float, beta2: float, eps: float) -> None:
    """One Adam update (gsr_adam_step) of up to 16 (param, grad, exp_avg,
    exp_avg_sq) fp32 device tensors, contiguous, each with its learning rate,
    all at step count `step` (after increment)."""
    if not tensors:
        return
    arr = (AdamGroup * len(tensors))()
    dev = None
    for k, ((p, g, m, v), lr) in enumerate(zip(tensors, lrs)):
        for t, name in ((p, "param"), (g, "grad"), (m, "exp_avg"), (v, "exp_avg_sq")):
            if not t.is_cuda or t.dtype != torch.float32 or not t.is_contiguous() or t.numel() != p.numel():
                raise RuntimeError(f"gsr adam: `{name}` must be a contiguous fp32 HIP tensor shaped like its param")
        dev = p.device
        arr[k] = AdamGroup(p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), p.numel(), float(lr))
    call(dev, "gsr_adam_step", len(tensors), arr, float(step), float(beta1), float(beta2), float(eps), _stream(dev))


def densify_stats(viewspace_grad, radii, max_radii2D, accum, accum_abs, denom) -> None:
    """add_densification_stats + max_radii2D (gsr_densify_stats), in place."""
    P = radii.numel()
    for t, name in ((viewspace_grad, "viewspace_grad"), (max_radii2D, "max_radii2D"), (accum, "accum"),
                    (accum_abs, "accum_abs"), (denom, "denom")):
        if not t.is_cuda or t.dtype != torch.float32 or not t.is_contiguous():
            raise RuntimeError(f"gsr densify_stats: `{name}` must be a contiguous fp32 HIP tensor")
    if radii.dtype != torch.int32 or not radii.is_cuda:
        raise RuntimeError("gsr densify_stats: `radii` must be an int32 HIP tensor")
    if viewspace_grad.numel() != 3 * P or max_radii2D.numel() != P or accum.numel() != P or accum_abs.numel() != P \
            or denom.numel() != P:
        raise RuntimeError("gsr densify_stats: shape mismatch")
    dev = radii.device
    r = radii.contiguous()
    call(dev, "gsr_densify_stats", P, _ptr(viewspace_grad), _ptr(r), _ptr(max_radii2D), _ptr(accum), _ptr(accum_abs),
         _ptr(denom), _stream(dev))


def view_color_grads_chunked(gathered, campos, n_views: int, chunk: int, means3D, sh_degree: int, dL_dsh,
                             sg_degree: int = 0, sg_axis=None, sg_sharpness=None, sg_color=None, dL_dsg_axis=None,
                             dL_dsg_sharpness=None, dL_dsg_color=None, dL_dsh_rest=None) -> None:
    """gsr_view_color_grads_chunked: view_color_grads for the range-by-range
    gathered layout (include/gsr.h): gathered [n_views * P * 3] DC rows in
    ranges of `chunk` Gaussians, campos [n_views, 4].  With `dL_dsh_rest` (the
    split SH layout) dL_dsh is the DC rows [P, 1, 3] and dL_dsh_rest the rest
    [P, SHM - 1, 3]."""
    P = means3D.shape[0]
    SHM = dL_dsh.shape[1] if dL_dsh_rest is None else 1 + dL_dsh_rest.shape[1]
    SGM = dL_dsg_color.shape[1] if dL_dsg_color is not None and dL_dsg_color.dim() == 3 else 0  # (P may be 0)
    want = {"means3D": (means3D, (P, 3)), "dL_dsh": (dL_dsh, (P, SHM, 3) if dL_dsh_rest is None else (P, 1, 3))}
    if dL_dsh_rest is not None:
        want["dL_dsh_rest"] = (dL_dsh_rest, (P, SHM - 1, 3))
    if SGM:
        want.update(dL_dsg_axis=(dL_dsg_axis, (P, SGM, 3)), dL_dsg_sharpness=(dL_dsg_sharpness, (P, SGM)),
                    dL_dsg_color=(dL_dsg_color, (P, SGM, 3)))
    if sg_degree:
        want.update(sg_axis=(sg_axis, (P, SGM, 3)), sg_sharpness=(sg_sharpness, (P, SGM)),
                    sg_color=(sg_color, (P, SGM, 3)))
    # (the checks of view_color_grads below, in its order and with its messages)
    for name, t in [("gathered", gathered), ("campos", campos)] + [(k, t) for k, (t, _) in want.items()]:
        if t is None or not t.is_cuda or t.dtype != torch.float32 or not t.is_contiguous():
            raise RuntimeError(f"gsr view_color_grads_chunked: `{name}` must be a contiguous fp32 HIP tensor")
    if gathered.numel() != n_views * P * 3 or campos.numel() != 4 * n_views or chunk < 1:
        raise RuntimeError("gsr view_color_grads_chunked: `gathered` must hold n_views * 3 P floats, `campos` "
                           "n_views * 4, chunk >= 1")
    if dL_dsh_rest is not None and SHM < 2:
        raise RuntimeError("gsr view_color_grads_chunked: the split SH layout needs SHM >= 2")
    for name, (t, shape) in want.items():
        if tuple(t.shape) != shape:
            raise RuntimeError(f"gsr view_color_grads_chunked: `{name}` has shape {tuple(t.shape)}, "
                               f"expected {shape}")
    if not 0 <= int(sh_degree) <= 3 or SHM < (int(sh_degree) + 1) ** 2 or not 0 <= int(sg_degree) <= SGM:
        raise RuntimeError(f"gsr view_color_grads_chunked: degrees (SH {sh_degree}, SG {sg_degree}) do not fit "
                           f"{SHM} SH rows and {SGM} SG lobes")
    dev = means3D.device
    p = lambda t: _ptr(t) if t is not None and t.numel() else None  # noqa: E731
    call(dev, "gsr_view_color_grads_chunked", P, int(sh_degree), SHM, int(sg_degree), SGM, int(n_views), int(chunk),
         _ptr(gathered), _ptr(campos), _ptr(means3D), p(sg_axis), p(sg_sharpness), p(sg_color), _ptr(dL_dsh),
         p(dL_dsg_axis), p(dL_dsg_sharpness), p(dL_dsg_color), p(dL_dsh_rest), _stream(dev))


def view_color_grads(gathered, n_views: int, means3D, sh_degree: int, dL_dsh, sg_degree: int = 0, sg_axis=None,
                     sg_sharpness=None, sg_color=None, dL_dsg_axis=None, dL_dsg_sharpness=None,
                     dL_dsg_color=None) -> None:
    """gsr_view_color_grads (view_grads.hip): the SH / SG gradient rows of a
    view-parallel step summed over `n_views` views, from the gathered
    [n_views, P * 3 + 4] DC rows + camera centres; outputs written in place."""
    P = means3D.shape[0]
    SHM = dL_dsh.shape[1]
    SGM = dL_dsg_color.shape[1] if dL_dsg_color is not None and dL_dsg_color.dim() == 3 else 0  # (P may be 0)
    need = [(gathered, "gathered"), (means3D, "means3D"), (dL_dsh, "dL_dsh")]
    if SGM:
        need += [(dL_dsg_axis, "dL_dsg_axis"), (dL_dsg_sharpness, "dL_dsg_sharpness"), (dL_dsg_color, "dL_dsg_color")]
    if sg_degree:
        need += [(sg_axis, "sg_axis"), (sg_sharpness, "sg_sharpness"), (sg_color, "sg_color")]
    for t, name in need:
        if t is None or not t.is_cuda or t.dtype != torch.float32 or not t.is_contiguous():
            raise RuntimeError(f"gsr view_color_grads: `{name}` must be a contiguous fp32 HIP tensor")
    if gathered.numel() != n_views * (3 * P + 4):
        raise RuntimeError("gsr view_color_grads: `gathered` must hold n_views * (3 P + 4) floats")
    want = {"means3D": (means3D, (P, 3)), "dL_dsh": (dL_dsh, (P, SHM, 3))}
    if SGM:
        want.update(dL_dsg_axis=(dL_dsg_axis, (P, SGM, 3)), dL_dsg_sharpness=(dL_dsg_sharpness, (P, SGM)),
                    dL_dsg_color=(dL_dsg_color, (P, SGM, 3)))
    if sg_degree:
        want.update(sg_axis=(sg_axis, (P, SGM, 3)), sg_sharpness=(sg_sharpness, (P, SGM)),
                    sg_color=(sg_color, (P, SGM, 3)))
    for name, (t, shape) in want.items():
        if tuple(t.shape) != shape:
            raise RuntimeError(f"gsr view_color_grads: `{name}` has shape {tuple(t.shape)}, expected {shape}")
    if not 0 <= int(sh_degree) <= 3 or SHM < (int(sh_degree) + 1) ** 2 or not 0 <= int(sg_degree) <= SGM:
        raise RuntimeError(f"gsr view_color_grads: degrees (SH {sh_degree}, SG {sg_degree}) do not fit "
                           f"{SHM} SH rows and {SGM} SG lobes")
    dev = means3D.device
    p = lambda t: _ptr(t) if t is not None and t.numel() else None  # noqa: E731
    call(dev, "gsr_view_color_grads", P, int(sh_degree), SHM, int(sg_degree), SGM, int(n_views), _ptr(gathered),
         _ptr(means3D), p(sg_axis), p(sg_sharpness), p(sg_color), _ptr(dL_dsh), p(dL_dsg_axis), p(dL_dsg_sharpness),
         p(dL_dsg_color), _stream(dev))
