"""Densification on the HIP path against the plain-torch restatement
(tests/densify_ref.py: the reference's mask-index-and-cat formulation), on the
same GPU.

    python tools/bench_densify.py [--out profiles/densify_bench.json] [--quick]

Rows: 1M and 5M Gaussians with SH degree 3 (5M also with SG degree 7), about
5% and about 30% of the points selected.  Per row and path: the median of 5
calls after one warm-up call (every call on a fresh copy of the state, built
outside the timed region; wall time around the call with a device
synchronisation at both ends, since both paths synchronise inside), the peak of
torch.cuda.max_memory_allocated above the state's own bytes, and the host
synchronisations torch reports (set_sync_debug_mode) — the HIP path's single
readback happens inside libgsr.so and is added by hand.  For the HIP path also
the gather's time and its achieved bytes/s against its algorithmic bytes (each
output element written once, each source element of a surviving or copied row
read once).  Last: the 3D filter kernel against gsr_scene.compute_filter_3D at
1M points x 200 cameras.
"""
from __future__ import annotations

import argparse
import json
import math
import os
import statistics
import sys
import time
import warnings

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "geometry-grounded-gaussian-splatting_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

import densify_ref as R  # noqa: E402
import gsr_densify  # noqa: E402
import gsr_optim  # noqa: E402
import gsr_scene  # noqa: E402

DEV = torch.device("cuda", 0)
MAX_GRAD, MIN_OPACITY, EXTENT = 0.0002, 0.005, 4.0


def master_state(P, sg, rate, seed=0):
    gen = torch.Generator(device=DEV).manual_seed(seed)
    rn = lambda *s: torch.randn(*s, generator=gen, device=DEV)  # noqa: E731
    ru = lambda *s: torch.rand(*s, generator=gen, device=DEV)  # noqa: E731
    params = dict(xyz=rn(P, 3) * 2, f_dc=rn(P, 1, 3), f_rest=rn(P, 15, 3) * 0.1, opacity=rn(P, 1) * 2 + 1,
                  scaling=rn(P, 3) * 0.5 + math.log(0.03), rotation=rn(P, 4), sg_axis=rn(P, sg, 3),
                  sg_sharpness=rn(P, sg), sg_color=rn(P, sg, 3) * 0.1)
    moments = {n: (torch.randn_like(v) * 0.01, torch.rand_like(v) * 1e-4) for n, v in params.items() if v.numel()}
    denom = torch.full((P,), 10.0, device=DEV)
    hot = ru(P) < rate * 0.6  # the quantile of grads_abs selects about as many again
    accum = torch.where(hot, 2.0, 0.5) * MAX_GRAD * denom
    accum_abs = torch.exp(rn(P)) * MAX_GRAD * denom
    return params, moments, (accum, accum_abs, denom)


def fresh(master, optimizer_cls):
    params, moments, stats = master
    g = R.RefGaussians(params, device=DEV, optimizer_cls=optimizer_cls)
    g.set_moments(moments)
    g.set_stats(*stats)
    return g


def state_bytes(master):
    params, moments, _ = master
    return sum(v.numel() * 4 for v in params.values()) + sum(2 * m.numel() * 4 for m, _ in moments.values())


def run_hip(g, noise):
    return gsr_densify.densify_and_prune(g, MAX_GRAD, MIN_OPACITY, EXTENT, None, noise=noise)


def run_ref(g, noise):
    return R.densify_and_prune_ref(g, MAX_GRAD, MIN_OPACITY, EXTENT, noise, use_torch_quantile=False)[0]


def measure(master, optimizer_cls, run, noise, reps):
    times, peak, syncs, triple = [], 0, 0, None
    for k in range(reps + 2):
        g = fresh(master, optimizer_cls)
        torch.cuda.synchronize()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        count_syncs = k == 0  # the warm-up call also counts the synchronisations torch sees
        if count_syncs:
            torch.cuda.set_sync_debug_mode("warn")
        with warnings.catch_warnings(record=True) as w:
            warnings.simplefilter("always")
            t0 = time.perf_counter()
            triple = run(g, noise)
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
        if count_syncs:
            torch.cuda.set_sync_debug_mode("default")
            syncs = sum("synchroniz" in str(x.message) for x in w)
        if k >= 2:
            times.append(dt * 1e3)
            peak = max(peak, torch.cuda.max_memory_allocated() - base)
        last = g
        del g
    return {"ms": statistics.median(times), "ms_all": [round(t, 3) for t in times], "peak_extra_bytes": int(peak),
            "torch_visible_syncs": syncs, "triple": [int(x) for x in triple], "N": int(last._xyz.shape[0])}, last


def bench_row(P, sg, rate, reps):
    master = master_state(P, sg, rate)
    noise = torch.randn((5 * P, 3), generator=torch.Generator(device=DEV).manual_seed(1), device=DEV)
    ref, g_ref = measure(master, torch.optim.Adam, run_ref, noise, reps)
    used = ref["triple"][0] + 2 * ref["triple"][1]
    del g_ref
    hip, g_hip = measure(master, gsr_optim.FusedAdam, run_hip, noise[:used].contiguous(), reps)
    hip["host_syncs"] = hip.pop("torch_visible_syncs") + 1  # + the plan's readback inside the library
    ref["host_syncs"] = ref.pop("torch_visible_syncs")
    assert hip["triple"] == ref["triple"] and hip["N"] == ref["N"], (hip, ref)
    # the gather alone
    gsr_densify.TIME_APPLY = True
    ms = []
    for _ in range(reps):
        g = fresh(master, gsr_optim.FusedAdam)
        run_hip(g, noise[:used].contiguous())
        ms.append(g.last_densify["apply_ms"])
        ld = g.last_densify
        del g
    gsr_densify.TIME_APPLY = False
    apply_ms = statistics.median(ms)
    width = sum(v[0].numel() for v in master[0].values())
    # survivors keep their moments; count them as N minus the new rows that survived the prune: with
    # min_opacity pruning few points, new rows ~ C + 2 S (an upper bound on the bytes of at most pruned / N)
    survivors = max(hip["N"] - (ld["C"] + 2 * ld["S"]), 0)
    algo = 4 * width * (3 * hip["N"] + hip["N"] + 2 * survivors) + 24 * hip["N"] + 25 * P
    row = {"P": P, "sg_degree": sg, "target_rate": rate, "selected_fraction": (ld["C"] + ld["S"]) / P,
           "state_bytes": state_bytes(master), "hip": hip, "torch_ref": ref,
           "speedup": ref["ms"] / hip["ms"], "peak_ratio": hip["peak_extra_bytes"] / max(ref["peak_extra_bytes"], 1),
           "apply": {"ms": apply_ms, "algorithmic_bytes": int(algo), "GBps": algo / apply_ms / 1e6}}
    print(json.dumps(row), flush=True)
    return row


class _Cam:
    def __init__(self, R_, T, W, H, F):
        self.R, self.T, self.image_width, self.image_height, self.Fx, self.Fy = R_, T, W, H, F, F


def bench_filter(P, n_cam, reps):
    gen = torch.Generator().manual_seed(2)
    xyz = torch.randn(P, 3, generator=gen) * 2
    xyz[:, 2] += 6.0
    xyz = xyz.to(DEV)
    cams = []
    for k in range(n_cam):
        th = (k / max(n_cam - 1, 1) - 0.5) * 1.2
        Rm = torch.tensor([[math.cos(th), 0, math.sin(th)], [0, 1, 0], [-math.sin(th), 0, math.cos(th)]],
                          dtype=torch.float32, device=DEV)
        cams.append(_Cam(Rm, torch.tensor([0.01 * k, 0.0, 0.5], device=DEV), 1920, 1080, 1600.0 + k))
    out = {}
    for name, fn in (("hip", lambda: gsr_densify.filter_3D(xyz, cams)),
                     ("torch", lambda: gsr_scene.compute_filter_3D(xyz, cams))):
        ts = []
        for k in range(reps + 1):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            res = fn()
            torch.cuda.synchronize()
            if k:
                ts.append((time.perf_counter() - t0) * 1e3)
        out[name + "_ms"] = statistics.median(ts)
        out[name] = res
    diff = float((out.pop("hip") - out.pop("torch")).abs().max())
    row = {"P": P, "cameras": n_cam, **out, "speedup": out["torch_ms"] / out["hip_ms"], "max_abs_diff": diff}
    print(json.dumps(row), flush=True)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--quick", action="store_true", help="100k points only (a functional check)")
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    rows = []
    configs = [(100_000, 0)] if a.quick else [(1_000_000, 0), (5_000_000, 0), (5_000_000, 7)]
    for P, sg in configs:
        for rate in (0.05, 0.30):
            rows.append(bench_row(P, sg, rate, a.reps))
            torch.cuda.empty_cache()
    filt = bench_filter(100_000 if a.quick else 1_000_000, 200, a.reps)
    result = {"device": torch.cuda.get_device_name(0), "reps": a.reps, "densify": rows, "filter_3D": filt}
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(result, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
