"""Image-metric timing (gsr_metric.image_metrics, csrc/imgmetric.hip) against the torch formulation of the same
quantities on the same GPU, at 1920 x 1080, N = 1 and N = 8 image pairs:
  quantised  (render.py -> metric.py): bytes of both images, PSNR and per-image SSIM.  torch: the
             mul / add_ / clamp_ / to(uint8) chain on both images, / 255, the reference's psnr, and
             fused_ssim(padding="valid") per image;
  float      (training_report): L1 and PSNR of the clamped images.  torch: clamp, abs().mean(), psnr.
The two forms alternate in rounds of timed windows (device events around `reps` calls each, after a warm-up of
both); the figures are the median over the rounds with the min-max spread.  Both forms end in their
device-to-host copy, as a caller sees them.  Also records, at the timed size, whether the bytes agree exactly and
how far the numbers of the two forms are apart.  No speed-up is promised: the fused call's point is the
contract (separately rounded x * 255 + 0.5, exact integer sums, per-image SSIM in one read).
Writes profiles/imgmetric_bench.json and prints it as one JSON line.

    python tools/bench_imgmetric.py [--rounds 7] [--reps 20]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "geometry-grounded-gaussian-splatting_amd")]
import torch  # noqa: E402

import gsr_metric  # noqa: E402
from fused_ssim import fused_ssim  # noqa: E402

H, W = 1080, 1920


def psnr(img1, img2):  # utils/image_utils.py:18-20
    mse = ((img1 - img2) ** 2).view(img1.shape[0], -1).mean(1, keepdim=True)
    return 20 * torch.log10(1.0 / torch.sqrt(mse))


def torch_quantised(a, b):
    qa = a.mul(255).add_(0.5).clamp_(0, 255).permute(0, 2, 3, 1).to(torch.uint8)
    qb = b.mul(255).add_(0.5).clamp_(0, 255).permute(0, 2, 3, 1).to(torch.uint8)
    fa, fb = qa.permute(0, 3, 1, 2).float() / 255, qb.permute(0, 3, 1, 2).float() / 255  # to_tensor
    ss = torch.stack([fused_ssim(fa[i:i + 1], fb[i:i + 1], padding="valid", train=False) for i in range(a.shape[0])])
    return torch.cat([psnr(fa, fb)[:, 0], ss]).cpu(), qa, qb


def torch_float(a, b):
    ca, cb = a.clamp(0.0, 1.0), b.clamp(0.0, 1.0)
    l1 = torch.abs(ca - cb).view(a.shape[0], -1).mean(1)
    return torch.cat([l1, psnr(ca, cb)[:, 0]]).cpu()


def window(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def alternate(fns, rounds, reps, warmup=5):
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=20)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_imgmetric needs a HIP device"
    dev = torch.device("cuda", 0)
    out = {"device": torch.cuda.get_device_name(0), "size": f"3x{H}x{W}", "rounds": args.rounds, "reps": args.reps}
    for N in (1, 8):
        g = torch.Generator(device="cpu").manual_seed(N)
        a = torch.rand((N, 3, H, W), generator=g)
        b = (a + 0.1 * torch.randn((N, 3, H, W), generator=g))
        a, b = (a * 1.2 - 0.1).to(dev), b.to(dev)  # values outside [0, 1] on both sides
        # agreement at the timed size
        m, qa, qb = gsr_metric.image_metrics(a, b, return_bytes=True)
        t, ta, tb = torch_quantised(a, b)
        mf = gsr_metric.image_metrics(a, b, quantize=False, ssim=False)
        tf = torch_float(a, b)
        agree = {"bytes_equal": bool(torch.equal(qa, ta) and torch.equal(qb, tb)),
                 "psnr_abs_diff_db": float((m["PSNR"] - t[:N].double()).abs().max()),
                 "ssim_abs_diff": float((m["SSIM"] - t[N:].double()).abs().max()),
                 "float_l1_rel_diff": float(((mf["L1"] - tf[:N].double()).abs() / mf["L1"]).max()),
                 "float_psnr_abs_diff_db": float((mf["PSNR"] - tf[N:].double()).abs().max())}
        q = alternate({"fused": lambda: gsr_metric.image_metrics(a, b, return_bytes=True),
                       "fused_no_bytes": lambda: gsr_metric.image_metrics(a, b),
                       "torch": lambda: torch_quantised(a, b)}, args.rounds, args.reps)
        f = alternate({"fused": lambda: gsr_metric.image_metrics(a, b, quantize=False, ssim=False),
                       "torch": lambda: torch_float(a, b)}, args.rounds, args.reps)
        q8 = alternate({"fused": lambda: gsr_metric.quantize8(a),
                        "torch": lambda: a.mul(255).add_(0.5).clamp_(0, 255).permute(0, 2, 3, 1).to(torch.uint8)
                        .contiguous()}, args.rounds, args.reps)
        out[f"N{N}"] = {"quantised_bytes_psnr_ssim": dict(q, speedup=round(q["torch"]["median_ms"] /
                                                                         q["fused"]["median_ms"], 3)),
                        "float_l1_psnr": dict(f, speedup=round(f["torch"]["median_ms"] / f["fused"]["median_ms"], 3)),
                        "quantize8_alone": dict(q8, speedup=round(q8["torch"]["median_ms"] /
                                                                  q8["fused"]["median_ms"], 3)),
                        "agreement": agree}
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "imgmetric_bench.json"), "w") as fp:
        json.dump(out, fp, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
