"""Fused photometric loss timing (gsr_loss.rgb_loss, csrc/photoloss.hip) against the unfused torch + fused_ssim
formulation of the same loss on the same GPU, forward plus backward at 1920 x 1080:
  NO without a mask  (the unfused form is TrainStep's rgb_loss lines with fused_rgb_loss=False)
  PGSR with a mask   (train.py:159-169, 189: composite, exp / addcmul, L1, fused_ssim)
and one TrainStep iteration at the bench.py --e2e size (1M Gaussians, SH 3, 1920 x 1080) with
fused_rgb_loss True against False.  The two forms alternate in rounds of timed windows (device events around
`reps` calls each, after a warm-up of both); the figures are the median over the rounds with the min-max spread.
Also checks that both forms agree on the loss and the image gradient at the timed size.
Writes profiles/photoloss_bench.json and prints it as one JSON line.

    python tools/bench_photoloss.py [--rounds 7] [--reps 30] [--e2e-steps 10] [--no-e2e]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "geometry-grounded-gaussian-splatting_amd")]
import torch  # noqa: E402

import gsr_loss  # noqa: E402
from fused_ssim import fused_ssim  # noqa: E402

LAM = 0.2


def unfused(x, gt, mask, bg, emb):
    if mask is not None:
        m = (mask > 0.5).float().unsqueeze(0)
        gt = gt * m + bg.view(3, 1, 1) * (1 - m)
    t = x if emb is None else torch.addcmul(emb[1], torch.exp(emb[0]), x)
    l1 = torch.abs(t - gt).mean()
    return (1.0 - LAM) * l1 + LAM * (1.0 - fused_ssim(x.unsqueeze(0), gt.unsqueeze(0), padding="valid"))


def fused(x, gt, mask, bg, emb):
    return gsr_loss.rgb_loss(x, gt, mask=mask, bg=bg, app_model="no" if emb is None else "pgsr", embedding=emb,
                             lambda_dssim=LAM)[0]


def window(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def alternate(fns, rounds, reps, warmup=10):
    for fn in fns.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    t = {k: [] for k in fns}
    for _ in range(rounds):
        for k, fn in fns.items():
            t[k].append(window(fn, reps))
    return {k: {"median_ms": round(statistics.median(v), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4)}
            for k, v in t.items()}


def loss_case(name, masked, pgsr, rounds, reps, dev):
    H, W = 1080, 1920
    g = torch.Generator(device="cpu").manual_seed(0)
    a = torch.rand(3, H, W, generator=g).to(dev)
    gt = (a + 0.1 * torch.randn(3, H, W, generator=g).to(dev)).clamp(0, 1)
    mask = bg = emb = None
    if masked:
        ys, xs = torch.meshgrid(torch.arange(H, device=dev), torch.arange(W, device=dev), indexing="ij")
        mask = ((xs - W / 2) ** 2 + (ys - H / 2) ** 2 < (0.45 * H) ** 2).float()
        bg = torch.ones(3, device=dev)
    if pgsr:
        emb = torch.tensor([0.05, -0.02], device=dev, requires_grad=True)
    x = a.clone().requires_grad_(True)

    def call(fn):
        def go():
            x.grad = None
            if emb is not None:
                emb.grad = None
            fn(x, gt, mask, bg, emb).backward()
        return go

    vals = {}
    for k, fn in (("fused", fused), ("unfused", unfused)):
        call(fn)()
        vals[k] = (float(fn(x, gt, mask, bg, emb).detach()), x.grad.clone())
    res = alternate({"fused": call(fused), "unfused": call(unfused)}, rounds, reps)
    res["speedup"] = round(res["unfused"]["median_ms"] / res["fused"]["median_ms"], 3)
    res["loss_abs_diff"] = abs(vals["fused"][0] - vals["unfused"][0])
    res["dimage_rel_l2"] = float((vals["fused"][1] - vals["unfused"][1]).norm() / vals["unfused"][1].norm())
    res["what"] = name
    return res


def e2e_case(rounds, steps, dev):
    import gsr_train

    out = {}
    ts, view, nearest = gsr_train.synthetic_training_setup(1_000_000, 1920, 1080, 3, 0, device=dev)
    steppers = {"fused": gsr_train.TrainStep(ts.g, fused_rgb_loss=True), "unfused": ts}
    res = alternate({k: (lambda s=s: s.step(view, nearest)) for k, s in steppers.items()}, rounds, steps, warmup=3)
    for k, v in res.items():
        out[k] = dict(v, iterations_per_s=round(1000.0 / v["median_ms"], 3))
    out["what"] = "TrainStep, 1M Gaussians SH 3, 1920x1080 (both steppers share one model, alternating)"
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--e2e-steps", type=int, default=10)
    ap.add_argument("--no-e2e", action="store_true")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    out = {"device": torch.cuda.get_device_name(0), "size": "3x1080x1920, forward + backward",
           "no_without_mask": loss_case("NO, no mask", False, False, a.rounds, a.reps, dev),
           "pgsr_with_mask": loss_case("PGSR, mask", True, True, a.rounds, a.reps, dev)}
    if not a.no_e2e:
        out["e2e"] = e2e_case(a.rounds, a.e2e_steps, dev)
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "photoloss_bench.json"), "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
