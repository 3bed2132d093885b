"""Densification on gfx950: the consumer of the densification statistics.

densify_and_prune — GaussianModel.densify_and_prune (scene/gaussian_model.py:
797-816 over densify_and_clone, densify_and_split, prune_points and the
optimizer cat / prune helpers, :630-768) as one device-side plan and one gather
(libgsr.so gsr_densify_plan / gsr_densify_apply, csrc/densify.hip): every
parameter and Adam moment is copied once, there is one small readback (the
counts), the random draw is an explicit tensor, and the result is the same
bits on every run.  The final order is the reference's: [surviving originals |
surviving clones | children copy 0 | children copy 1].

compute_3D_filter / reset_3D_filter / reset_opacity — gaussian_model.py:220-262
and :521-539 (gsr_filter_3d, gsr_reset_opacity).

quantile — torch.quantile's linear rule by radix select (gsr_quantile), without
its 16,777,216-element limit.

All of these work on anything shaped like gsr_train.TrainGaussians: the nine
raw parameters `_xyz` ... `_sg_color`, `filter_3D`, the four statistics,
`percent_dense` and an `optimizer` whose groups are named and hold one
parameter each.  There is no CPU path: tensors must be float32 HIP tensors.
"""
from __future__ import annotations

import ctypes

import torch

from diff_gaussian_rasterization._abi import DensifyParam, call, check, load, ptr, stream

ROLE_COPY, ROLE_XYZ, ROLE_SCALING = 0, 1, 2
TIME_APPLY = False  # measurement (tools/bench_densify.py): last_densify["apply_ms"], adds a synchronisation
# optimizer group name, attribute, role (gaussian_model.py:342-351, densification_postfix)
PARAMS = (("xyz", "_xyz", ROLE_XYZ), ("f_dc", "_features_dc", ROLE_COPY), ("f_rest", "_features_rest", ROLE_COPY),
          ("opacity", "_opacity", ROLE_COPY), ("scaling", "_scaling", ROLE_SCALING), ("rotation", "_rotation", ROLE_COPY),
          ("sg_axis", "_sg_axis", ROLE_COPY), ("sg_sharpness", "_sg_sharpness", ROLE_COPY),
          ("sg_color", "_sg_color", ROLE_COPY))


def _f32(t, name, rows=None):
    if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype != torch.float32:
        raise RuntimeError(f"gsr densify: `{name}` must be a float32 HIP tensor")
    if not t.is_contiguous():
        raise RuntimeError(f"gsr densify: `{name}` must be contiguous")
    if rows is not None and (t.dim() == 0 or t.shape[0] != rows):
        raise RuntimeError(f"gsr densify: `{name}` must have {rows} rows, got {tuple(t.shape)}")
    return t


def _groups(optimizer):
    """name -> param group, for the groups densification edits (one parameter each)."""
    out = {}
    for group in optimizer.param_groups:
        name = group.get("name")
        if name in ("appearance_embeddings", "appearance_network") or name is None:
            continue
        if len(group["params"]) != 1:
            raise RuntimeError(f"gsr densify: optimizer group `{name}` must hold exactly one parameter")
        out[name] = group
    return out


def _replace(gaussians, optimizer, group, attr, new, moments):
    """cat_tensors_to_optimizer / _prune_optimizer's bookkeeping: a new nn.Parameter in the
    group, the optimizer state re-keyed to it with the new moments (no state stays no state)."""
    param = torch.nn.Parameter(new.requires_grad_(True))
    if group is not None:
        old = group["params"][0]
        st = optimizer.state.pop(old, None)
        group["params"][0] = param
        if st is not None:
            if moments is not None:
                st["exp_avg"], st["exp_avg_sq"] = moments
            optimizer.state[param] = st
    setattr(gaussians, attr, param)


@torch.no_grad()
def densify_and_prune(gaussians, max_grad, min_opacity, extent, max_screen_size=None, *, noise=None, generator=None):
    """GaussianModel.densify_and_prune; returns its triple (clone - before,
    split - clone, split - prune) = (clones, split selections, opacity-pruned
    points).  `noise` [C + 2 S, 3] is the standard-normal draw behind the
    reference's torch.normal calls (clones use rows [0, C), the children of the
    k-th selected point rows C + k and C + S + k); when None it is drawn with
    torch.randn((C + 2 S, 3), generator=generator) after the plan's readback.
    `max_screen_size` is accepted and unused, as in the reference.  filter_3D
    is left as it was (stale): call compute_3D_filter afterwards."""
    g = gaussians
    P = g._xyz.shape[0]
    dev = g._xyz.device
    srcs = {}
    for name, attr, role in PARAMS:
        srcs[attr] = _f32(getattr(g, attr).detach(), attr, P)
    stats = [_f32(getattr(g, a), a, P) for a in ("xyz_gradient_accum", "xyz_gradient_accum_abs", "denom")]
    if any(s.numel() != P for s in stats) or srcs["_opacity"].numel() != P or srcs["_scaling"].shape != (P, 3) \
            or srcs["_xyz"].shape != (P, 3) or srcs["_rotation"].shape != (P, 4):
        raise RuntimeError("gsr densify: statistics [P,1], _opacity [P,1], _scaling / _xyz [P,3], _rotation [P,4] expected")
    L = load()
    nbytes = L.gsr_densify_workspace_bytes(P)
    if nbytes < 0:
        raise RuntimeError(f"gsr densify: {P} points are out of range")
    groups = _groups(g.optimizer)
    with torch.cuda.device(dev):  # (one guard over both calls: the apply's timing events record on this device)
        strm = stream(dev)
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        counts = (ctypes.c_longlong * 4)()
        Q = ctypes.c_float()
        check(L.gsr_densify_plan(P, stats[0].data_ptr(), stats[1].data_ptr(), stats[2].data_ptr(),
                                 srcs["_scaling"].data_ptr(), srcs["_opacity"].data_ptr(), float(max_grad),
                                 float(min_opacity), float(g.percent_dense * extent), ws.data_ptr(), counts,
                                 ctypes.byref(Q), strm))
        C, S, pruned, N = (int(c) for c in counts)
        rows = C + 2 * S
        if noise is None:
            noise = torch.randn((rows, 3), generator=generator, dtype=torch.float32,
                                device=generator.device if generator is not None else dev).to(dev)
        elif not isinstance(noise, torch.Tensor) or tuple(noise.shape) != (rows, 3):
            raise RuntimeError(f"gsr densify: noise must be [C + 2 S, 3] = [{rows}, 3] for this call, got "
                               f"{tuple(noise.shape) if isinstance(noise, torch.Tensor) else type(noise)}")
        noise = _f32(noise, "noise")
        # Validate every moment before anything is replaced, then gather one parameter per launch and
        # hand it over at once: the source (and its moments) is released before the next output is
        # allocated, so the peak above the model's own bytes is one parameter with its two moments, not
        # the whole model.  xyz goes first (it reads the source _rotation and _scaling), then the largest.
        states = {}
        for name, attr, role in PARAMS:
            st = g.optimizer.state.get(groups[name]["params"][0]) if name in groups else None
            if st is not None and "exp_avg" in st:
                m, v = _f32(st["exp_avg"], name + ".exp_avg", P), _f32(st["exp_avg_sq"], name + ".exp_avg_sq", P)
                if m.shape != srcs[attr].shape or v.shape != srcs[attr].shape:
                    raise RuntimeError(f"gsr densify: the moments of `{name}` do not have the parameter's shape")
                states[attr] = st
        fmap = torch.empty(3 * max(N, 1), dtype=torch.int32, device=dev)
        rot_ptr, scl_ptr = srcs["_rotation"].data_ptr(), srcs["_scaling"].data_ptr()
        order = sorted(PARAMS, key=lambda t: (t[2] != ROLE_XYZ, -srcs[t[1]][0].numel()))
        apply_ms, first = (0.0 if TIME_APPLY else None), True
        for name, attr, role in order:
            src = srcs.pop(attr)
            width = src[0].numel()
            out = torch.empty((N,) + tuple(src.shape[1:]), dtype=torch.float32, device=dev)
            st = states.get(attr)
            moments = (torch.empty_like(out), torch.empty_like(out)) if st is not None else None
            if width and N:
                desc = DensifyParam(src.data_ptr(), st["exp_avg"].data_ptr() if st else None,
                                    st["exp_avg_sq"].data_ptr() if st else None, out.data_ptr(),
                                    moments[0].data_ptr() if st else None, moments[1].data_ptr() if st else None,
                                    width, role)
                if TIME_APPLY:
                    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
                    ev[0].record()
                check(L.gsr_densify_apply(P, counts, ws.data_ptr(), fmap.data_ptr(), int(first), ptr(noise), rows,
                                          rot_ptr if role == ROLE_XYZ else None,
                                          scl_ptr if role == ROLE_XYZ else None, 1, ctypes.byref(desc), strm))
                first = False
                if TIME_APPLY:
                    ev[1].record()
                    ev[1].synchronize()
                    apply_ms += ev[0].elapsed_time(ev[1])
            del src, st
            _replace(g, g.optimizer, groups.get(name), attr, out, moments)
    g.xyz_gradient_accum = torch.zeros((N, 1), device=dev)
    g.xyz_gradient_accum_abs = torch.zeros((N, 1), device=dev)
    g.denom = torch.zeros((N, 1), device=dev)
    g.max_radii2D = torch.zeros(N, device=dev)
    g.last_densify = {"C": C, "S": S, "pruned": pruned, "N": N, "Q": float(Q.value), "apply_ms": apply_ms}
    return C, S, pruned


def camera_records(cameras, device):
    """([n_cam, 14] float32 on `device`, max Fx): R (as the reference stores it), T and the two
    frustum bounds of every camera, the layout gsr_filter_3d reads."""
    cameras = list(cameras)
    if not cameras:
        raise RuntimeError("gsr densify: compute_3D_filter needs at least one camera")
    # three stacks and one copy, whatever the number of cameras
    R = torch.stack([torch.as_tensor(c.R, dtype=torch.float32).reshape(9) for c in cameras]).to(device)
    T = torch.stack([torch.as_tensor(c.T, dtype=torch.float32).reshape(3) for c in cameras]).to(device)
    b = torch.tensor([[c.image_width / c.Fx * 0.575, c.image_height / c.Fy * 0.575] for c in cameras],
                     dtype=torch.float32).to(device)
    return torch.cat([R, T, b], dim=1).contiguous(), max(float(c.Fx) for c in cameras)


@torch.no_grad()
def filter_3D(xyz, cameras):
    """gaussian_model.py:225-262 for `xyz` [P,3]: the [P,1] 3D filter."""
    xyz = _f32(xyz.detach(), "xyz")
    P = xyz.shape[0]
    if xyz.shape != (P, 3) or P == 0:
        raise RuntimeError("gsr densify: xyz [P,3] with P >= 1 expected")
    recs, focal = camera_records(cameras, xyz.device)
    out = torch.empty((P, 1), dtype=torch.float32, device=xyz.device)
    scratch = torch.empty(1, dtype=torch.int32, device=xyz.device)
    call(xyz.device, "gsr_filter_3d", P, xyz.data_ptr(), recs.shape[0], recs.data_ptr(), focal, out.data_ptr(),
         scratch.data_ptr(), stream(xyz.device))
    return out


def compute_3D_filter(gaussians, cameras):
    """GaussianModel.compute_3D_filter: sets gaussians.filter_3D [P,1]."""
    gaussians.filter_3D = filter_3D(gaussians._xyz, cameras)


@torch.no_grad()
def reset_3D_filter(gaussians):
    """GaussianModel.reset_3D_filter: a zero filter of the current size."""
    xyz = gaussians._xyz
    gaussians.filter_3D = torch.zeros((xyz.shape[0], 1), device=xyz.device)


@torch.no_grad()
def reset_opacity(gaussians):
    """GaussianModel.reset_opacity: the filtered opacity capped at 0.01, as a new `_opacity`
    parameter of the "opacity" group with zeroed moments (replace_tensor_to_optimizer)."""
    g = gaussians
    P = g._xyz.shape[0]
    s, o = _f32(g._scaling.detach(), "_scaling", P), _f32(g._opacity.detach(), "_opacity", P)
    f = _f32(g.filter_3D, "filter_3D", P)
    if s.shape != (P, 3) or o.numel() != P or f.numel() != P:
        raise RuntimeError("gsr densify: _scaling [P,3], _opacity [P,1], filter_3D [P,1] expected")
    group = _groups(g.optimizer).get("opacity")
    st = g.optimizer.state.get(group["params"][0]) if group is not None else None
    out = torch.empty_like(o)
    moments = (torch.empty_like(o), torch.empty_like(o)) if st is not None and "exp_avg" in st else None
    call(o.device, "gsr_reset_opacity", P, ptr(s), ptr(o), ptr(f), ptr(out), ptr(moments[0]) if moments else None,
         ptr(moments[1]) if moments else None, stream(o.device))
    _replace(g, g.optimizer, group, "_opacity", out, moments)


@torch.no_grad()
def quantile(values, q):
    """torch.quantile(values, q) (linear interpolation) for a flat float32 HIP tensor of
    non-negative values and a scalar q (float or 0-dim tensor), as a 0-dim device tensor."""
    v = _f32(values, "values").reshape(-1)
    if v.numel() == 0:
        raise RuntimeError("gsr densify: quantile of an empty tensor")
    qt = torch.as_tensor(q, dtype=torch.float32).to(v.device).reshape(1).contiguous()
    out = torch.empty((), dtype=torch.float32, device=v.device)
    ws = torch.empty(load().gsr_quantile_workspace_bytes(), dtype=torch.uint8, device=v.device)
    call(v.device, "gsr_quantile", v.numel(), v.data_ptr(), qt.data_ptr(), out.data_ptr(), ws.data_ptr(),
         stream(v.device))
    return out
