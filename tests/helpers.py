"""Shared test helpers: small seeded scenes and tolerance checks."""
from __future__ import annotations

import math

import numpy as np
import torch

import gsr_scene as S


def small_case(P=40, W=40, H=24, seed=0, sh_degree=3, sg_degree=0, sgm=None, log_scale=math.log(0.12),
               opacity_max_logit=2.0, z_range=(2.0, 4.0), kernel_size=0.0, require_depth=True, cam=None,
               bg=(0.0, 0.0, 0.0), flat=1.0, opacity_std=1.0, sh_max_degree=None):
    """A small random scene plus every argument of _C.rasterize_gaussians.

    Opacity logits are capped at `opacity_max_logit` (default 2: sigmoid(2) =
    0.88, so o*G < 0.99); the clamp cases raise the cap (logit 6: o = 0.9975)
    so alpha = min(0.99, o*G) clamps and the reference's pass-through gradient
    of the clamp (render_backward.cu:931-933, 1012) is exercised.
    `sh_max_degree` > `sh_degree` gives the SH warm-up layout: 16 SH rows
    rendered at a lower active degree (train.py:130)."""
    cam = cam or S.make_camera(W, H)
    raw = S.make_gaussians(P, sh_degree=sh_degree, sg_degree=sgm if sgm is not None else sg_degree, seed=seed,
                           aspect=H / W, z_range=z_range, log_scale_mean=log_scale, log_scale_std=0.3,
                           opacity_std=opacity_std, sh_max_degree=sh_max_degree)
    raw.opacity.clamp_(max=opacity_max_logit)
    if flat != 1.0:  # surfel-like Gaussians: one axis `flat` times thinner (steep vacancy steps)
        raw.scaling[:, 2] -= math.log(flat)
    inp = S.activated_inputs(raw)
    inp = {k: v.detach().contiguous() for k, v in inp.items()}
    return dict(
        bg=torch.tensor(bg, dtype=torch.float32), inp=inp, cam=cam, W=W, H=H, sh_degree=sh_degree,
        sg_degree=sg_degree, kernel_size=kernel_size, require_depth=require_depth,
        tanx=math.tan(cam.FoVx * 0.5), tany=math.tan(cam.FoVy * 0.5), raw=raw)


def oracle_args(c, colors_precomp=None):
    inp = c["inp"]
    return (c["bg"], inp["means3D"], colors_precomp, inp["opacities"], inp["scales"], inp["rotations"], None,
            None if colors_precomp is not None else inp["shs"], inp["sg_axis"], inp["sg_sharpness"],
            inp["sg_color"], c["sh_degree"], c["sg_degree"], 1.0, c["cam"].world_view_transform,
            c["cam"].full_proj_transform, c["tanx"], c["tany"], c["kernel_size"], c["H"], c["W"],
            c["cam"].camera_center, False, c["require_depth"])


def rel_err(a, b) -> float:
    """max|a-b| / max|b| (0 if both are zero)."""
    a = np.asarray(a, np.float64)
    b = np.asarray(b, np.float64)
    den = np.abs(b).max() if b.size else 0.0
    num = np.abs(a - b).max() if a.size else 0.0
    return 0.0 if den == 0 and num == 0 else float(num / max(den, 1e-30))


def record_margins(fields: dict, what: str = "") -> None:
    """Parity margins: {field: (value, bar)} of one test
    case.  Prints the worst field against its bar and appends one JSON line
    per case to $GSR_MARGIN_LOG (default gpurun_out/parity_margins.jsonl at
    the repository root, when that directory can be written)."""
    import json
    import os
    if not fields:
        return
    test = os.environ.get("PYTEST_CURRENT_TEST", "").rsplit(" ", 1)[0]  # (drops " (call)"; an id may hold spaces)
    worst = max(fields, key=lambda k: fields[k][0] / fields[k][1])
    v, bar = fields[worst]
    print(f"[margin] {test} {what}: worst {worst} {v:.3e} against {bar:.0e} ({bar / max(v, 1e-300):.1f}x headroom)")
    path = os.environ.get("GSR_MARGIN_LOG") or os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(
        __file__))), "gpurun_out", "parity_margins.jsonl")
    try:
        os.makedirs(os.path.dirname(path), exist_ok=True)
        with open(path, "a") as f:
            f.write(json.dumps({"test": test, "what": what, "worst": worst, "value": v, "bar": bar,
                                "headroom": bar / max(v, 1e-300),
                                "fields": {k: [float(a), float(b)] for k, (a, b) in fields.items()}}) + "\n")
    except OSError:
        pass


def max_err(a, ref) -> float:
    """max|a-ref| over the elements / max|ref| of the tensor; the absolute
    max|a-ref| where the reference is all zero (or empty: 0)."""
    a = torch.as_tensor(a).detach().cpu().double()
    ref = torch.as_tensor(ref).detach().cpu().double()
    if ref.numel() == 0:
        return 0.0
    num, den = float((a - ref).abs().max()), float(ref.abs().max())
    return num if den == 0.0 else num / den


def row_errs(a, ref) -> torch.Tensor:
    """max_err row by row (dim 0): max|a-ref| over a row's elements / max|ref|
    of that row, absolute where the row's reference is zero.  [len(ref)] float64;
    a non-finite element of `a` gives that row inf."""
    if torch.as_tensor(ref).numel() == 0:
        return torch.zeros(len(ref), dtype=torch.float64)
    a = torch.as_tensor(a).detach().cpu().double().reshape(len(ref), -1)
    ref = torch.as_tensor(ref).detach().cpu().double().reshape(len(ref), -1)
    num, den = (a - ref).abs().amax(dim=1), ref.abs().amax(dim=1)
    e = torch.where(den == 0.0, num, num / den.clamp_min(1e-300))
    return torch.where(torch.isfinite(a).all(dim=1), e, torch.full_like(e, float("inf")))


def row_err(a, ref) -> float:
    """The worst row of row_errs, so that a wrong row is not diluted by the
    largest row of the tensor."""
    e = row_errs(a, ref)
    return float(e.max()) if e.numel() else 0.0


class Yardstick:
    """The project's float64 yardstick: a GPU result may be no further from
    the exact float64 value than twice the error of the reference's own fp32
    arithmetic, e_gpu <= 2 e_fp32 + floor (`floor`: the measured e_gpu where
    the fp32 reference happens to be exact, rounded up to a power of ten).
    add() prints every figure; check() records the margins and asserts."""

    def __init__(self, what: str = ""):
        self.what, self.fields = what, {}

    def add(self, name: str, e_gpu: float, e_fp32: float, floor: float) -> None:
        assert math.isfinite(e_gpu) and math.isfinite(e_fp32), (name, e_gpu, e_fp32)  # an infinite bar checks nothing
        print(f"[yard] {self.what} {name}: e_gpu {e_gpu:.3e} e_fp32 {e_fp32:.3e} floor {floor:.0e}")
        self.fields[name] = (float(e_gpu), 2.0 * float(e_fp32) + floor)

    def check(self) -> None:
        record_margins({k: v for k, v in self.fields.items() if v[1] > 0.0}, self.what)  # (bar 0: exact, no margin)
        bad = {k: v for k, v in self.fields.items() if not v[0] <= v[1]}
        assert not bad, bad


def frac_bad(a, b, rtol, atol) -> float:
    a = np.asarray(a, np.float64)
    b = np.asarray(b, np.float64)
    if a.size == 0:
        return 0.0
    return float(np.mean(np.abs(a - b) > atol + rtol * np.abs(b)))


def gpu_n_contrib_for_oracle(out, o, H, W):
    """The GPU forward's per-pixel last contributors as positions in the
    oracle's per-tile lists.  The GPU lists are the oracle's (the reference's)
    minus the tile-culled instances, in the same order, so the
    last contributor's Gaussian is looked up in the oracle's list of its tile.
    With it (State.set_n_contrib) the oracle backward runs on exactly the GPU
    forward's state: its images and its contributor ranges."""
    from diff_gaussian_rasterization import _C

    plist, ranges = _C.debug_binning(out[7], out[9], out[0], H, W)
    last = _C.debug_n_contrib(out[8], H, W).astype(np.int64)
    ob = o["state"].binning()["point_list"].astype(np.int64)
    orng = o["state"].tile_state()["ranges"].astype(np.int64)
    gx = (W + 15) // 16
    ys, xs = np.mgrid[0:H, 0:W]
    tile = (ys // 16) * gx + (xs // 16)
    res = np.zeros((H, W), np.int64)
    has = last > 0
    g = plist.astype(np.int64)[ranges[tile[has], 0].astype(np.int64) + last[has] - 1]
    # per tile, the oracle positions of its Gaussians: search (tile, gaussian) keys in the oracle's list,
    # which is sorted per tile by depth, not id, so look up through a sorted copy
    otile = np.repeat(np.arange(orng.shape[0], dtype=np.int64), orng[:, 1] - orng[:, 0])
    okey = (otile << 32) | ob[np.concatenate([np.arange(a, b) for a, b in orng]) if len(ob) else np.zeros(0, np.int64)]
    opos = np.concatenate([np.arange(b - a) for a, b in orng]) if len(ob) else np.zeros(0, np.int64)
    srt = np.argsort(okey, kind="stable")
    want = (tile[has].astype(np.int64) << 32) | g
    at = np.searchsorted(okey[srt], want)
    assert np.array_equal(okey[srt][at], want), "GPU contributor missing from the oracle's tile list"
    res[has] = opos[srt][at] + 1
    return res.astype(np.uint32)


def check_binning(out, o, H, W, dead_sample=None):
    """Per-tile Gaussian lists against the oracle's (the reference's stable
    (tile, depth) sort order): ours is the oracle's list with the instances
    the tile test culls removed, in the same order, and every removed
    instance is dead — power > 0 or alpha < 1/255 at every pixel of its tile
    (checked for all of them, or for `dead_sample` random ones)."""
    from diff_gaussian_rasterization import _C

    plist, ranges = _C.debug_binning(out[7], out[9], out[0], H, W)
    ob = o["state"].binning()["point_list"].astype(np.int64)
    oranges = o["state"].tile_state()["ranges"].astype(np.int64)
    tiles = ranges.shape[0]

    def keys(pl, rg):
        tile = np.repeat(np.arange(tiles, dtype=np.int64), rg[:, 1] - rg[:, 0])
        ent = np.concatenate([pl[a:b] for a, b in rg]) if len(pl) else np.zeros(0, np.int64)
        return (tile << 32) | ent.astype(np.int64)

    ours = keys(plist.astype(np.int64), ranges.astype(np.int64))
    ref = keys(ob, oranges)
    assert len(ours) <= len(ref) == out[0]
    srt = np.argsort(ref, kind="stable")
    at = np.searchsorted(ref[srt], ours)
    assert np.all(at < len(ref)) and np.array_equal(ref[srt][np.minimum(at, len(ref) - 1)], ours)
    pos = srt[at]
    assert np.all(np.diff(pos) > 0)  # same relative order in every tile
    dropped = ref[~np.isin(ref, ours)]
    if dead_sample is not None and len(dropped) > dead_sample:
        dropped = np.random.default_rng(0).choice(dropped, dead_sample, replace=False)
    geo = o["state"].geometry()
    gx = (W + 15) // 16
    py, px = np.mgrid[0:16, 0:16]
    for k in dropped:
        t, g = int(k >> 32), int(k & 0xFFFFFFFF)
        ty, tx = divmod(t, gx)
        x = (tx * 16 + px).ravel().astype(np.float64)
        y = (ty * 16 + py).ravel().astype(np.float64)
        keep = (x < W) & (y < H)
        mx, my = geo["means2D"][g].astype(np.float64)
        a, b, c, op = geo["conic_opacity"][g].astype(np.float64)
        dx, dy = mx - x[keep], my - y[keep]
        power = -0.5 * (a * dx * dx + c * dy * dy) - b * dx * dy
        alpha = np.minimum(0.99, op * np.exp(np.minimum(power, 0.0)))
        assert np.all((power > 0) | (alpha < 1.0 / 255.0)), (t, g)


def with_depth_ties(c, n_tied):
    """Gaussians n_tied..2 n_tied-1 get the means of 0..n_tied-1: bit-identical
    depths, so the per-tile order of each pair is decided by the index alone
    (the reference's stable sort, rasterizer_impl.cu:403-412)."""
    m = c["inp"]["means3D"].clone()
    m[n_tied:2 * n_tied] = m[:n_tied]
    c["inp"]["means3D"] = m.contiguous()
    return c


def place(c, idx, px, py, z):
    """Gaussians `idx` moved to pixel centres (px, py) at depth z (identity camera:
    pixel = ((ndc + 1) size - 1) / 2)."""
    f32 = lambda v: torch.as_tensor(np.asarray(v), dtype=torch.float32)  # noqa: E731
    px, py, z = f32(px), f32(py), f32(z)
    m = c["inp"]["means3D"].clone()
    m[idx, 0] = ((2 * px + 1) / c["W"] - 1) * z * c["tanx"]
    m[idx, 1] = ((2 * py + 1) / c["H"] - 1) * z * c["tany"]
    m[idx, 2] = z
    c["inp"]["means3D"] = m.contiguous()


def reshape(c, idx, scale, opacity=0.8):
    """Gaussians `idx` axis-aligned with scales `scale` (x, y, z) and the given opacity."""
    s, r, op = (c["inp"][k].clone() for k in ("scales", "rotations", "opacities"))
    s[idx] = torch.tensor(scale, dtype=torch.float32)
    r[idx] = torch.tensor([1.0, 0.0, 0.0, 0.0])
    op[idx] = opacity
    c["inp"].update(scales=s.contiguous(), rotations=r.contiguous(), opacities=op.contiguous())


def surely_live_tiles(o, g, W, H):
    """Tiles that Gaussian g certainly keeps after tile culling, from the
    oracle's geometry: those holding a pixel of the row or the column through
    its centre with power <= 0 and alpha >= 2/255 (twice the cull's 1/255, so no
    rounding decides it).  A lower bound of its live tiles; set of (ty, tx)."""
    geo = o["state"].geometry()
    mx, my = geo["means2D"][g].astype(np.float64)
    a, b, cc, op = geo["conic_opacity"][g].astype(np.float64)
    x0, y0 = int(np.clip(round(mx), 0, W - 1)), int(np.clip(round(my), 0, H - 1))
    live = set()
    for xs, ys in ((np.arange(W, dtype=np.float64), np.full(W, float(y0))),
                   (np.full(H, float(x0)), np.arange(H, dtype=np.float64))):
        dx, dy = mx - xs, my - ys
        power = -0.5 * (a * dx * dx + cc * dy * dy) - b * dx * dy
        ok = (power <= 0) & (op * np.exp(np.minimum(power, 0.0)) >= 2.0 / 255.0)
        live |= set(zip((ys[ok] // 16).astype(int).tolist(), (xs[ok] // 16).astype(int).tolist()))
    return live


def gpu_entries_of(out, g, H, W):
    """How many per-tile list entries of the GPU forward name Gaussian g."""
    from diff_gaussian_rasterization import _C

    plist, ranges = _C.debug_binning(out[7], out[9], out[0], H, W)
    return int((plist[:int(ranges[:, 1].max())] == g).sum())


def parse_header(path):
    """The C ABI as include/gsr.h declares it, from the text of its extern "C" block (no compiler needed: the
    header is regular).  -> (prototypes, structs): prototypes {name: (return type, [parameter type, ...])} in
    the header's order, structs {name: [(member type, member name, array length or None), ...]}.  Types are
    normalised: no `const`, no parameter name, single spaces, the stars attached ("float*", "long long")."""
    import re

    text = open(path).read()
    text = text[text.index('extern "C" {'):text.rindex("#ifdef __cplusplus")]
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    text = "\n".join(ln for ln in text.split("\n")[1:] if not ln.lstrip().startswith("#"))

    def ctype(decl):
        """(type, name) of `const float* x`, `unsigned long long* counters`, `void* ctx`, `int key_bits[3]`."""
        m = re.fullmatch(r"\s*(.*?)(\w+)\s*((?:\[\w+\])?)\s*", decl, flags=re.S)
        t = re.sub(r"\bconst\b", " ", m.group(1))
        t = re.sub(r"\s*\*\s*", "*", " ".join(t.split()))
        return t, m.group(2), m.group(3)

    structs = {}
    for body, name in re.findall(r"typedef\s+struct\s*\w*\s*\{(.*?)\}\s*(\w+)\s*;", text, flags=re.S):
        members = []
        for stmt in filter(str.strip, body.split(";")):
            first, *more = stmt.split(",")  # `double bounds_min[3], bounds_max[3]`
            t, n, arr = ctype(first)
            for n, arr in [(n, arr)] + [ctype(t + " " + x)[1:] for x in more]:
                members.append((t, n, int(arr[1:-1]) if arr else None))
        structs[name] = members
    text = re.sub(r"typedef\s+struct\s*\w*\s*\{.*?\}\s*\w+\s*;", " ", text, flags=re.S)
    text = re.sub(r"enum\s+\w+\s*\{.*?\}\s*;", " ", text, flags=re.S)
    text = re.sub(r"typedef[^;]*;", " ", text)  # the two callback typedefs
    prototypes = {}
    for stmt in filter(str.strip, text.split(";")):
        m = re.fullmatch(r"\s*(.*?)\b(gsr_\w+)\s*\((.*)\)\s*", stmt, flags=re.S)
        assert m, f"not a prototype: {stmt.strip()[:80]!r}"
        ret = ctype(m.group(1) + " _")[0]
        params = [] if m.group(3).strip() == "void" else [ctype(p)[0] for p in m.group(3).split(",")]
        assert m.group(2) not in prototypes, m.group(2)
        prototypes[m.group(2)] = (ret, params)
    return prototypes, structs


def free_port() -> int:
    """A free TCP port for a process group's rendezvous, outside the kernel's ephemeral range: a port picked
    by binding to port 0 is an ephemeral one, and the gloo connections an earlier multi-rank test left in
    their last states take ephemeral ports too — one was taken again between the pick and the ranks' bind
    (EADDRINUSE at the C5 8-rank test's rendezvous, round 6)."""
    import random
    import socket
    lo = 32768
    try:
        with open("/proc/sys/net/ipv4/ip_local_port_range") as f:
            lo = int(f.read().split()[0])
    except (OSError, ValueError, IndexError):
        pass
    rng = random.Random()
    for _ in range(256):
        p = rng.randrange(10000, max(10001, lo))
        s = socket.socket()
        try:
            s.bind(("127.0.0.1", p))
            return p
        except OSError:
            continue
        finally:
            s.close()
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p
