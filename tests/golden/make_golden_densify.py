"""Generate tests/golden/densify.npz by running the reference's own
GaussianModel.densify_and_prune, compute_3D_filter and reset_opacity
(scene/gaussian_model.py) on the CPU.

Run where the reference checkout exists:
    python tests/golden/make_golden_densify.py
Only the data file written next to this script is committed.

The reference is CUDA-only in three places, patched here without touching
what it computes: `device="cuda"` is stripped from torch's factory functions,
torch.normal(mean, std) becomes mean + std * eps with eps drawn from a seeded
generator and stored (the HIP path and tests/densify_ref.py take eps as an
input), and torch.quantile is wrapped to store Q.  The optimizer is a real
torch.optim.Adam over the nine named groups that has taken one step, so the
moments are non-zero.  compute_3D_filter runs between densify_and_prune and
reset_opacity, as train.py does.

Cases (max SH degree 1, SG degree 1):
  mixed    P = 130: clones, splits, points that are cloned AND split, opacity
           prunes among survivors, clones and children;
  resplit  Q = 0: every original and every clone is split;
  nostats  denom == 0 everywhere: Q = 0, everything splits, no clones;
  quiet    no gradient reaches max_grad and no opacity is low.  The reference
           cannot select nothing: ratio = 0 gives Q = max(grads_abs), and the
           point that attains it satisfies grads_abs >= Q, so exactly that one
           point is split.
A tie margin is asserted: no point lies within 1e-5 (relative) of pd * extent,
max_grad, Q, min_opacity, z = 0.2 or a frustum bound, so the decisions do not
depend on whose exp / sigmoid / dot product is used.  Values that equal Q
exactly by construction (zeros when Q = 0, the maximum when Q is the maximum)
are exempt: the comparison is then between identical bits.
"""
from __future__ import annotations

import importlib
import math
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as MG  # noqa: E402  (the stubs of the reference's CUDA-only imports)

NAMES = {"xyz": "_xyz", "f_dc": "_features_dc", "f_rest": "_features_rest", "opacity": "_opacity",
         "scaling": "_scaling", "rotation": "_rotation", "sg_axis": "_sg_axis", "sg_sharpness": "_sg_sharpness",
         "sg_color": "_sg_color"}
LRS = {"xyz": 0.00016, "f_dc": 0.0013, "f_rest": 0.00011, "opacity": 0.05, "scaling": 0.005, "rotation": 0.001,
       "sg_axis": 0.002, "sg_sharpness": 0.095, "sg_color": 0.00064}
MARGIN = 1e-5
EXTENT, MAX_GRAD, MIN_OPACITY = 4.0, 0.0002, 0.05
LIMIT = 0.01 * EXTENT


def _strip_cuda(fn):
    def wrapped(*a, **k):
        if k.get("device") == "cuda":
            k.pop("device")
        return fn(*a, **k)
    return wrapped


class Cam:
    def __init__(self, R, T, W, H, Fx, Fy):
        self.R, self.T = torch.tensor(R, dtype=torch.float32), torch.tensor(T, dtype=torch.float32)
        self.image_width, self.image_height, self.Fx, self.Fy = W, H, Fx, Fy


def cameras(rng):
    cams = []
    for k, (W, H, F) in enumerate([(64, 48, 55.0), (80, 60, 70.0), (64, 64, 60.0)]):
        th = [0.0, 0.5, -0.6][k]
        R = np.array([[math.cos(th), 0, math.sin(th)], [0, 1, 0], [-math.sin(th), 0, math.cos(th)]])
        T = np.array([0.1 * k, -0.05 * k, 0.3 * k])
        cams.append(Cam(R, T, W, H, F, F * 1.02))
    return cams


def raw_params(rng, P):
    xyz = rng.standard_normal((P, 3)).astype(np.float32) * np.array([1.2, 0.9, 1.0], np.float32)
    xyz[:, 2] = rng.uniform(1.0, 6.0, P)
    xyz[:max(1, P // 16)] = rng.standard_normal((max(1, P // 16), 3)) * 0.3 + np.array([0, 0, -3.0])  # seen by no camera
    return dict(
        xyz=xyz.astype(np.float32),
        f_dc=rng.standard_normal((P, 1, 3)).astype(np.float32),
        f_rest=(rng.standard_normal((P, 3, 3)) * 0.1).astype(np.float32),
        opacity=(rng.standard_normal((P, 1)) * 1.5).astype(np.float32),
        scaling=(rng.standard_normal((P, 3)) * 0.6 + math.log(0.03)).astype(np.float32),
        rotation=rng.standard_normal((P, 4)).astype(np.float32),
        sg_axis=rng.standard_normal((P, 1, 3)).astype(np.float32),
        sg_sharpness=rng.standard_normal((P, 1)).astype(np.float32),
        sg_color=(rng.standard_normal((P, 1, 3)) * 0.1).astype(np.float32))


def stats_for(case, rng, P):
    denom = rng.integers(1, 30, P).astype(np.float32)
    denom[rng.random(P) < 0.1] = 0.0  # never visible: 0 / 0 -> NaN -> 0
    per_view = np.exp(rng.standard_normal(P) * 1.0 + math.log(MAX_GRAD * 0.6))
    per_view_abs = np.exp(rng.standard_normal(P) * 1.0 + math.log(MAX_GRAD * 2.0))
    if case == "resplit":  # more than 1 - ratio of grads_abs are zero -> Q = 0
        per_view_abs[rng.random(P) < 0.93] = 0.0
    if case == "nostats":
        denom[:] = 0.0
    if case == "quiet":
        per_view = np.minimum(per_view, MAX_GRAD * 0.5)
    accum = (per_view * denom).astype(np.float32)
    accum_abs = (per_view_abs * denom).astype(np.float32)
    if case == "nostats":
        accum[:] = 0.0
        accum_abs[:] = 0.0
    return accum, accum_abs, denom


def far(values, threshold, exempt=None):
    values = np.asarray(values, np.float64).reshape(-1)
    near = np.abs(values - threshold) <= MARGIN * max(abs(threshold), 1e-30)
    if exempt is not None:
        near &= ~exempt
    return not near.any()


def run_case(gm, case, P, seed, out):
    rng = np.random.default_rng(seed)
    raw = raw_params(rng, P)
    if case == "quiet":
        raw["opacity"] = np.abs(raw["opacity"]) + 0.5
    g = gm.GaussianModel(1, 1)
    for name, attr in NAMES.items():
        setattr(g, attr, torch.nn.Parameter(torch.tensor(raw[name])))
    g.percent_dense = 0.01
    g.optimizer = torch.optim.Adam([{"params": [getattr(g, attr)], "lr": LRS[name], "name": name}
                                    for name, attr in NAMES.items()], lr=0.0, eps=1e-15)
    tg = torch.Generator().manual_seed(seed)
    for attr in NAMES.values():
        p = getattr(g, attr)
        p.grad = torch.randn(p.shape, generator=tg) * 0.01
    g.optimizer.step()
    g.optimizer.zero_grad(set_to_none=True)
    accum, accum_abs, denom = stats_for(case, rng, P)
    g.xyz_gradient_accum = torch.tensor(accum)[:, None]
    g.xyz_gradient_accum_abs = torch.tensor(accum_abs)[:, None]
    g.denom = torch.tensor(denom)[:, None]
    g.max_radii2D = torch.zeros(P)
    g.filter_3D = torch.zeros(P, 1)

    pre = f"{case}_"
    for name, attr in NAMES.items():
        p = getattr(g, attr)
        out[pre + "in_" + name] = p.detach().numpy().copy()
        out[pre + "in_m_" + name] = g.optimizer.state[p]["exp_avg"].numpy().copy()
        out[pre + "in_v_" + name] = g.optimizer.state[p]["exp_avg_sq"].numpy().copy()
    out[pre + "accum"], out[pre + "accum_abs"], out[pre + "denom"] = accum, accum_abs, denom

    eps_rows, Qs = [], []

    def normal(mean, std):
        eps = torch.randn(std.shape, generator=tg)
        eps_rows.append(eps)
        return mean + std * eps

    real_quantile = torch.quantile

    def quantile(x, q, *a, **k):
        Q = real_quantile(x, q, *a, **k)
        Qs.append(float(Q))
        return Q

    torch.normal, torch.quantile = normal, quantile
    try:
        triple = g.densify_and_prune(MAX_GRAD, MIN_OPACITY, EXTENT, None)
    finally:
        torch.quantile = real_quantile
    Q = Qs[0]
    noise = torch.cat(eps_rows, dim=0).numpy()

    # ---- the tie margin, on the inputs
    with np.errstate(invalid="ignore", divide="ignore"):
        gr = np.nan_to_num(accum / denom, nan=0.0)
        ga = np.nan_to_num(accum_abs / denom, nan=0.0)
    assert far(gr, MAX_GRAD), case
    assert far(ga, Q, exempt=(ga == np.float32(Q))), case
    assert far(np.exp(out[pre + "in_scaling"].astype(np.float64)).max(axis=1), LIMIT), case
    assert far(1.0 / (1.0 + np.exp(-out[pre + "in_opacity"].astype(np.float64))), MIN_OPACITY), case

    for name, attr in NAMES.items():
        p = getattr(g, attr)
        out[pre + "out_" + name] = p.detach().numpy().copy()
        out[pre + "out_m_" + name] = g.optimizer.state[p]["exp_avg"].numpy().copy()
        out[pre + "out_v_" + name] = g.optimizer.state[p]["exp_avg_sq"].numpy().copy()
    N = g._xyz.shape[0]
    assert g.xyz_gradient_accum.shape == (N, 1) and g.max_radii2D.shape == (N,)
    assert float(g.xyz_gradient_accum.abs().sum() + g.denom.abs().sum() + g.max_radii2D.abs().sum()) == 0.0
    out[pre + "noise"] = noise
    out[pre + "triple"] = np.array(triple, np.int64)
    out[pre + "Q"] = np.array(Q, np.float32)
    out[pre + "scalars"] = np.array([MAX_GRAD, MIN_OPACITY, EXTENT], np.float64)

    # ---- 3D filter and opacity reset on the densified model
    cams = cameras(rng)
    xyz64 = g._xyz.detach().double().numpy()
    for c in cams:
        pc = xyz64 @ c.R.double().numpy() + c.T.double().numpy()
        assert far(pc[:, 2], 0.2), case
        front = pc[:, 2] > 0.2
        assert far(np.abs(pc[front, 0] / pc[front, 2]), c.image_width / c.Fx * 0.575), case
        assert far(np.abs(pc[front, 1] / pc[front, 2]), c.image_height / c.Fy * 0.575), case
    g.compute_3D_filter(cams)
    out[pre + "filter_3D"] = g.filter_3D.numpy().copy()
    g.reset_opacity()
    out[pre + "reset_opacity"] = g._opacity.detach().numpy().copy()
    st = g.optimizer.state[g._opacity]
    assert float(st["exp_avg"].abs().sum() + st["exp_avg_sq"].abs().sum()) == 0.0
    out[pre + "cam_R"] = np.stack([c.R.numpy() for c in cams])
    out[pre + "cam_T"] = np.stack([c.T.numpy() for c in cams])
    out[pre + "cam_WHF"] = np.array([[c.image_width, c.image_height, c.Fx, c.Fy] for c in cams], np.float64)
    return triple, Q, N


def main():
    MG._install_stubs()
    for fn in ("zeros", "ones", "full", "empty", "tensor", "rand", "randn", "arange"):
        setattr(torch, fn, _strip_cuda(getattr(torch, fn)))
    gm = importlib.import_module("scene.gaussian_model")
    out = {}
    for case, P, seed in (("mixed", 130, 11), ("resplit", 48, 12), ("nostats", 40, 13), ("quiet", 64, 14)):
        triple, Q, N = run_case(gm, case, P, seed, out)
        print(f"{case}: P={P} clone={triple[0]} split={triple[1]} pruned={triple[2]} N={N} Q={Q:.6g}")
    path = os.path.join(HERE, "densify.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")
    assert os.path.getsize(path) < 256 * 1024


if __name__ == "__main__":
    main()
