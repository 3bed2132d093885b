"""Trained models across a process boundary: point_cloud.ply and checkpoints.

save_ply / load_ply — GaussianModel.save_ply and load_ply (scene/gaussian_model.py:450-493,
541-611).  A vertex row is the model's ten stored tensors interleaved, `f_rest` transposed; the
rows are formed and taken apart on the device, one launch each way and no temporaries (libgsr.so
gsr_model_pack_rows / gsr_model_unpack_rows, csrc/modelio.hip), and travel between the device and
the file in chunks through pinned host memory.  The header is the one `plyfile` writes for the
reference's structured array, so each side reads the other's files.

save_model / load_model — the `point_cloud/iteration_N/point_cloud.ply` layout of scene/__init__.py.

save_checkpoint / load_checkpoint — TrainGaussians.capture() with the iteration through torch.save.
The file is this project's own format (tensors, numbers, strings, lists and dicts only: it loads
with weights_only=True), not the reference's chkpnt.pth, which pickles an enum of its package.

There is no CPU path: tensors must be float32 HIP tensors.  The header parser is host code.
"""
from __future__ import annotations

import math
import os
import re
from dataclasses import dataclass

import numpy as np
import torch

import gsr_scene as S
from diff_gaussian_rasterization._abi import call, check, load, ptr, stream

# the stored tensors in the order the C ABI takes them, with TrainGaussians' attribute names
TENSORS = (("xyz", "_xyz"), ("features_dc", "_features_dc"), ("features_rest", "_features_rest"),
           ("opacity", "_opacity"), ("scaling", "_scaling"), ("rotation", "_rotation"), ("sg_axis", "_sg_axis"),
           ("sg_sharpness", "_sg_sharpness"), ("sg_color", "_sg_color"), ("filter_3D", "filter_3D"))
# PLY scalar types and their widths in bytes
PLY_TYPES = {"char": 1, "int8": 1, "uchar": 1, "uint8": 1, "short": 2, "int16": 2, "ushort": 2, "uint16": 2,
             "int": 4, "int32": 4, "uint": 4, "uint32": 4, "float": 4, "float32": 4, "double": 8, "float64": 8}
_FLOAT_CODE = {"float": 0, "float32": 0, "double": 1, "float64": 1}  # the type codes of gsr_model_unpack_rows
CHUNK_BYTES = 64 << 20  # of rows per chunk, unless chunk_rows says otherwise


def row_floats(M: int, G: int) -> int:
    """Floats per row for M SH coefficients and G spherical Gaussians: 18 + 3 (M - 1) + 7 G."""
    A = load().gsr_model_row_floats(int(M), int(G))
    if A <= 0:
        raise ValueError(f"gsr model: M = {M}, G = {G} are out of range")
    return A


def attribute_names(M: int, G: int, exclude_filter: bool = False) -> list:
    """construct_list_of_attributes (gaussian_model.py:450-470): the property names of a row, in order."""
    names = ["x", "y", "z", "nx", "ny", "nz"] + [f"f_dc_{k}" for k in range(3)]
    names += [f"f_rest_{k}" for k in range(3 * (M - 1))] + ["opacity"]
    names += [f"scale_{k}" for k in range(3)] + [f"rot_{k}" for k in range(4)]
    names += [f"sg_axis_{k}" for k in range(3 * G)] + [f"sg_sharpness_{k}" for k in range(G)]
    names += [f"sg_color_{k}" for k in range(3 * G)]
    return names if exclude_filter else names + ["filter_3D"]


def ply_header(P: int, M: int, G: int, exclude_filter: bool = False) -> bytes:
    """The header plyfile writes for PlyData([PlyElement.describe(elements, "vertex")]) with all-f4 fields."""
    lines = ["ply", "format binary_little_endian 1.0", f"element vertex {int(P)}"]
    lines += [f"property float {n}" for n in attribute_names(M, G, exclude_filter)]
    return ("\n".join(lines + ["end_header"]) + "\n").encode("ascii")


# ---- the model's tensors -----------------------------------------------------------------------------------------

def _tensors(gaussians):
    """The ten stored tensors of a TrainGaussians or a RawGaussians, checked; nothing is copied or cast."""
    out = []
    for name, attr in TENSORS:
        t = getattr(gaussians, attr if hasattr(gaussians, attr) else name, None)
        if not isinstance(t, torch.Tensor):
            raise ValueError(f"gsr model: `{name}` is missing")
        t = t.detach()
        if t.dtype != torch.float32:
            raise ValueError(f"gsr model: `{name}` must be float32 (got {t.dtype})")
        if not t.is_cuda:
            raise ValueError(f"gsr model: `{name}` must be on a HIP device (got {t.device})")
        if not t.is_contiguous():
            raise ValueError(f"gsr model: `{name}` must be contiguous")
        if out and t.device != out[0].device:
            raise ValueError(f"gsr model: `{name}` is on {t.device}, `xyz` on {out[0].device}")
        out.append(t)
    P = out[0].shape[0]
    M, G = out[2].shape[1] + 1 if out[2].dim() == 3 else -1, out[7].shape[1] if out[7].dim() == 2 else -1
    want = ((P, 3), (P, 1, 3), (P, M - 1, 3), (P, 1), (P, 3), (P, 4), (P, G, 3), (P, G), (P, G, 3), (P, 1))
    for (name, _), t, shape in zip(TENSORS, out, want):
        if tuple(t.shape) != shape:
            raise ValueError(f"gsr model: `{name}` must have shape {shape} (got {tuple(t.shape)})")
    return out, P, M, G


def _ptrs(tensors, r0, n):
    return [ptr(t[r0:r0 + n]) for t in tensors]


def pack_rows(tensors, M, G, r0=0, n=None, out=None):
    """Rows [r0, r0 + n) of the model as [n, A] float32 on the device (into `out` when given)."""
    P = tensors[0].shape[0]
    n = P - r0 if n is None else n
    dev = tensors[0].device
    A = row_floats(M, G)
    rows = torch.empty((n, A), dtype=torch.float32, device=dev) if out is None else out[:n * A].view(n, A)
    call(dev, "gsr_model_pack_rows", n, M, G, *_ptrs(tensors, r0, n), ptr(rows), stream(dev))
    return rows


def _chunk_rows(chunk_rows, row_bytes, block):
    if chunk_rows is None:  # sized in bytes, and a whole number of the kernel's blocks
        return max(CHUNK_BYTES // row_bytes // block * block, block)
    if int(chunk_rows) < 1:
        raise ValueError("gsr model: `chunk_rows` must be at least 1")
    return int(chunk_rows)


def save_ply(gaussians, path, chunk_rows=None):
    """GaussianModel.save_ply: `gaussians` (a TrainGaussians or a RawGaussians) as a binary little-endian
    PLY of float properties.  The rows are packed on the device chunk by chunk and copied to one of two
    pinned host buffers, so the copy of a chunk runs while the chunk before it is written."""
    tensors, P, M, G = _tensors(gaussians)
    A = row_floats(M, G)
    block = load().gsr_model_block_rows(A)
    if block <= 0:
        raise ValueError(f"gsr model: a row of {A} floats is too long for the pack kernel")
    dev = tensors[0].device
    if os.path.dirname(path):
        os.makedirs(os.path.dirname(path), exist_ok=True)
    C = min(_chunk_rows(chunk_rows, 4 * A, block), max(P, 1))
    with open(path, "wb") as f, torch.cuda.device(dev):
        f.write(ply_header(P, M, G))
        if P == 0:
            return
        staging = [torch.empty(C * A, dtype=torch.float32, device=dev) for _ in range(2)]
        pinned = [torch.empty(C * A, dtype=torch.float32, pin_memory=True) for _ in range(2)]
        events = [torch.cuda.Event() for _ in range(2)]
        pending = None  # (slot, floats) of the chunk whose copy is in flight
        for k, r0 in enumerate(range(0, P, C)):
            slot, n = k & 1, min(C, P - r0)
            pack_rows(tensors, M, G, r0, n, out=staging[slot])
            pinned[slot][:n * A].copy_(staging[slot][:n * A], non_blocking=True)
            events[slot].record()
            if pending is not None:
                events[pending[0]].synchronize()
                f.write(pinned[pending[0]].numpy()[:pending[1]].data)
            pending = (slot, n * A)
        events[pending[0]].synchronize()
        f.write(pinned[pending[0]].numpy()[:pending[1]].data)


# ---- reading ----------------------------------------------------------------------------------------------------

@dataclass
class PlyHeader:
    """The vertex element of a model file: `properties` are (name, PLY type, byte offset in a row)."""

    count: int
    properties: list
    stride: int
    payload_offset: int
    sh_degree: int
    sg_degree: int
    has_filter: bool

    @property
    def M(self) -> int:
        return (self.sh_degree + 1) ** 2

    def column_tables(self):
        """(byte offsets, type codes) of the canonical columns, the tables of gsr_model_unpack_rows:
        properties are found by name, so their order in the file is free and others are ignored."""
        at = {n: (o, t) for n, t, o in self.properties}
        off, code = [], []
        for n in attribute_names(self.M, self.sg_degree):
            o, t = at.get(n, (-1, "float"))
            if n in ("nx", "ny", "nz"):  # (not stored in any tensor)
                o, t = -1, "float"
            off.append(o)
            code.append(_FLOAT_CODE[t])
        return np.asarray(off, dtype=np.int32), np.asarray(code, dtype=np.int32)


def _family(names, prefix, path):
    """The suffixes of the properties `prefix`<k>, which must be exactly 0 .. n-1; returns n."""
    ks = sorted(int(n[len(prefix):]) for n in names if re.fullmatch(re.escape(prefix) + r"\d+", n))
    if ks != list(range(len(ks))):
        raise ValueError(f"{path}: the `{prefix}*` properties are not numbered 0 .. {len(ks) - 1}: {ks}")
    return len(ks)


def read_ply_header(path, allow_missing_filter: bool = False) -> PlyHeader:
    """Parse the header of a model file: little-endian binary, `vertex` the first element, scalar
    properties of any PLY type (their widths make up the stride).  ValueError, naming the cause,
    for anything else and for a property list that is not a model's."""
    size = os.path.getsize(path)
    with open(path, "rb") as f:
        head = f.read(1 << 20)
    end = head.find(b"end_header\n")
    if not head.startswith(b"ply") or end < 0:
        raise ValueError(f"{path}: not a PLY file (no `ply` ... `end_header`)")
    payload_offset = end + len(b"end_header\n")
    lines = [ln.strip() for ln in head[:end].decode("ascii", "replace").splitlines()]
    fmt = [ln.split() for ln in lines if ln.startswith("format")]
    if not fmt or len(fmt[0]) < 2:
        raise ValueError(f"{path}: no `format` line")
    if fmt[0][1] != "binary_little_endian":
        raise ValueError(f"{path}: format `{fmt[0][1]}` is not supported (binary_little_endian only)")
    count, props, element, n_elements = None, [], None, 0
    for ln in lines:
        tok = ln.split()
        if not tok:
            continue
        if tok[0] == "element":
            element = tok[1] if len(tok) == 3 else None
            n_elements += 1
            if element == "vertex":
                if n_elements != 1:
                    raise ValueError(f"{path}: element `vertex` must be the first element")
                count = int(tok[2])
        elif tok[0] == "property" and element == "vertex":
            if len(tok) >= 2 and tok[1] == "list":
                raise ValueError(f"{path}: list property `{tok[-1]}` in the vertex element")
            if len(tok) != 3 or tok[1] not in PLY_TYPES:
                raise ValueError(f"{path}: cannot read property line `{ln}`")
            props.append((tok[2], tok[1]))
    if count is None or count < 0:
        raise ValueError(f"{path}: no `element vertex`")
    names = [n for n, _ in props]
    if len(set(names)) != len(names):
        raise ValueError(f"{path}: duplicate property `{[n for n in names if names.count(n) > 1][0]}`")
    properties, stride = [], 0
    for n, t in props:
        properties.append((n, t, stride))
        stride += PLY_TYPES[t]
    if size - payload_offset < count * stride:
        raise ValueError(f"{path}: payload of {size - payload_offset} bytes is shorter than count x stride = "
                         f"{count} x {stride}")
    # a model's properties
    required = ["x", "y", "z", "opacity", "f_dc_0", "f_dc_1", "f_dc_2"]
    has_filter = "filter_3D" in names
    if not has_filter and not allow_missing_filter:
        required.append("filter_3D")
    for n in required:
        if n not in names:
            raise ValueError(f"{path}: required property `{n}` is missing")
    for prefix, want in (("scale_", 3), ("rot_", 4)):
        got = _family(names, prefix, path)
        if got != want:
            raise ValueError(f"{path}: {got} `{prefix}*` properties, {want} required")
    n_rest = _family(names, "f_rest_", path)
    degree = math.isqrt(n_rest // 3 + 1) - 1
    if n_rest != 3 * ((degree + 1) ** 2 - 1):
        raise ValueError(f"{path}: {n_rest} `f_rest_*` properties are not 3 (M - 1) for an integer SH degree")
    n_axis, G, n_color = (_family(names, p, path) for p in ("sg_axis_", "sg_sharpness_", "sg_color_"))
    if n_axis != 3 * G or n_color != 3 * G:
        raise ValueError(f"{path}: {n_axis} `sg_axis_*`, {G} `sg_sharpness_*` and {n_color} `sg_color_*` "
                         "properties disagree (3 G, G, 3 G expected)")
    M = (degree + 1) ** 2
    model = set(attribute_names(M, G)) - {"nx", "ny", "nz"}
    for n, t in props:
        if n in model and t not in _FLOAT_CODE:
            raise ValueError(f"{path}: property `{n}` is `{t}`; a model column must be float or double")
    return PlyHeader(count, properties, stride, payload_offset, degree, G, has_filter)


def load_ply(path, sh_degree=None, sg_degree=None, device="cuda", chunk_rows=None,
             allow_missing_filter: bool = False) -> S.RawGaussians:
    """GaussianModel.load_ply: the model of `path` as RawGaussians on `device`.  The degrees come from
    the header when None and are checked against it when given (the reference's assert, as a
    ValueError).  The file's bytes go up in chunks and are unpacked on the device."""
    h = read_ply_header(path, allow_missing_filter)
    if sh_degree is not None and int(sh_degree) != h.sh_degree:
        raise ValueError(f"{path}: holds SH degree {h.sh_degree} ({3 * (h.M - 1)} f_rest), not sh_degree = {sh_degree}")
    if sg_degree is not None and int(sg_degree) != h.sg_degree:
        raise ValueError(f"{path}: holds {h.sg_degree} spherical Gaussians, not sg_degree = {sg_degree}")
    dev = torch.device(device)
    if dev.type != "cuda":
        raise ValueError("gsr model: load_ply needs a HIP device")
    if dev.index is None:
        dev = torch.device("cuda", torch.cuda.current_device())
    P, M, G = h.count, h.M, h.sg_degree
    shapes = ((P, 3), (P, 1, 3), (P, M - 1, 3), (P, 1), (P, 3), (P, 4), (P, G, 3), (P, G), (P, G, 3), (P, 1))
    tensors = [torch.empty(s, dtype=torch.float32, device=dev) for s in shapes]
    if P:
        off, code = (torch.from_numpy(a).to(dev) for a in h.column_tables())
        L = load()
        C = min(_chunk_rows(chunk_rows, h.stride, 256), P)
        pinned = torch.empty(C * h.stride, dtype=torch.uint8, pin_memory=True)
        staging = torch.empty(C * h.stride, dtype=torch.uint8, device=dev)
        view = pinned.numpy()
        with open(path, "rb") as f, torch.cuda.device(dev):
            f.seek(h.payload_offset)
            for r0 in range(0, P, C):
                n = min(C, P - r0)
                if f.readinto(view[:n * h.stride]) != n * h.stride:
                    raise ValueError(f"{path}: payload ends inside row chunk {r0} .. {r0 + n}")
                staging[:n * h.stride].copy_(pinned[:n * h.stride], non_blocking=True)
                check(L.gsr_model_unpack_rows(n, M, G, h.stride, ptr(staging), ptr(off), ptr(code),
                                              *_ptrs(tensors, r0, n), stream(dev)))
                torch.cuda.current_stream(dev).synchronize()  # (the pinned buffer is refilled next)
    return S.RawGaussians(tensors[0], tensors[1], tensors[2], tensors[4], tensors[5], tensors[3], tensors[6],
                          tensors[7], tensors[8], tensors[9])


# ---- the model directory (scene/__init__.py:40-46, 133-135; utils/system_utils.py searchForMaxIteration) --------

def _ply_path(model_path, iteration):
    return os.path.join(model_path, "point_cloud", f"iteration_{int(iteration)}", "point_cloud.ply")


def save_model(gaussians, model_path, iteration, chunk_rows=None) -> str:
    """Scene.save: `model_path`/point_cloud/iteration_<iteration>/point_cloud.ply; returns the path."""
    path = _ply_path(model_path, iteration)
    save_ply(gaussians, path, chunk_rows)
    return path


def max_iteration(model_path) -> int:
    """searchForMaxIteration: the largest N with a point_cloud/iteration_N directory."""
    folder = os.path.join(model_path, "point_cloud")
    found = [int(m.group(1)) for m in (re.fullmatch(r"iteration_(\d+)", n) for n in
                                       (os.listdir(folder) if os.path.isdir(folder) else [])) if m]
    if not found:
        raise ValueError(f"{model_path}: no point_cloud/iteration_N directory")
    return max(found)


def load_model(model_path, iteration=-1, **kwargs):
    """Scene(..., load_iteration=): (RawGaussians, iteration); -1 picks the largest iteration present.
    `kwargs` are load_ply's."""
    it = max_iteration(model_path) if iteration == -1 else int(iteration)
    return load_ply(_ply_path(model_path, it), **kwargs), it


# ---- checkpoints (train.py:56-58, 265-270) -------------------------------------------------------------------------

def save_checkpoint(gaussians, iteration, path) -> None:
    """torch.save((gaussians.capture(), iteration), path) — `chkpnt<iteration>.pth` by convention."""
    if os.path.dirname(path):
        os.makedirs(os.path.dirname(path), exist_ok=True)
    torch.save((gaussians.capture(), int(iteration)), path)


def load_checkpoint(path, device="cuda"):
    """(TrainGaussians, iteration) of a file save_checkpoint wrote, restored on `device`."""
    from gsr_train import TrainGaussians

    state, iteration = torch.load(path, map_location=device, weights_only=True)
    raw = S.RawGaussians(state[2], state[3], state[4], state[5], state[6], state[7], state[8], state[9], state[10],
                         state[19])
    g = TrainGaussians(raw, spatial_lr_scale=state[15], sh_degree=state[0], sg_degree=state[1])
    g.restore(state)
    return g, int(iteration)
