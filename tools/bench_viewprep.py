"""View-preparation timing (gsr_data.resize_u8 + view_planes, csrc/viewprep.hip) at the start-up shape of a
mip360 scene: a batch of 5187 x 3361 RGB images scaled to 1600 wide (1600 x 1036).

  device    the two resample passes and the float planes on bytes already on the device (device events around
            `reps` calls, median over `rounds` windows with the min-max spread), per image, with each launch
            alone as well, and the share of the bytes-in roofline the whole chain reaches: the 52 MB of an
            image read once at the 6.3 TB/s a streaming read achieves on this part;
  upload    the copy of the full-size bytes from pageable host memory, per image (host clock, synchronised) —
            what the device path pays that the host path does not;
  pillow    the only baseline there is: PIL.Image.resize on the host, / 255.0 in torch, and the copy of the small
            float image to the device, per image (host clock), as PILtoTorch and Camera.__init__ do it.
Also records whether the device bytes equal Pillow's at this size.  No speed-up is promised; the point of the
device path is the byte contract with the start-up time it may save.
Writes profiles/viewprep_bench.json and prints it as one JSON line.

    python tools/bench_viewprep.py [--batch 4] [--rounds 5] [--reps 5]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "geometry-grounded-gaussian-splatting_amd")]
import numpy as np  # noqa: E402
import torch  # noqa: E402

import gsr_data  # noqa: E402

W0, H0 = 5187, 3361
STREAM_TBPS = 6.3  # achievable HBM streaming read


def spread(v, per):
    return {"median_ms": round(statistics.median(v) / per, 4), "min_ms": round(min(v) / per, 4),
            "max_ms": round(max(v) / per, 4)}


def device_windows(fn, rounds, reps, per, warmup=2):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t = []
    for _ in range(rounds):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        t.append(e0.elapsed_time(e1) / reps)
    return spread(t, per)


def host_windows(fn, rounds, per):
    fn()
    t = []
    for _ in range(rounds):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        t.append((time.perf_counter() - t0) * 1e3)
    return spread(t, per)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_viewprep needs a HIP device"
    dev = torch.device("cuda", 0)
    N = args.batch
    size = gsr_data.target_resolution(W0, H0, -1)
    host = np.random.default_rng(0).integers(0, 256, (N, H0, W0, 3), dtype=np.uint8)
    x = torch.from_numpy(host).to(dev)
    mid = gsr_data._resample(x, 1, size[0])
    small = gsr_data._resample(mid, 0, size[1])

    def chain():
        return gsr_data.view_planes(gsr_data.resize_u8(x, size))

    res = {"shape": {"batch": N, "in": [H0, W0, 3], "out": [size[1], size[0], 3]},
           "device_per_image": device_windows(chain, args.rounds, args.reps, N),
           "pass_w_per_image": device_windows(lambda: gsr_data._resample(x, 1, size[0]), args.rounds, args.reps, N),
           "pass_h_per_image": device_windows(lambda: gsr_data._resample(mid, 0, size[1]), args.rounds, args.reps, N),
           "planes_per_image": device_windows(lambda: gsr_data.view_planes(small), args.rounds, args.reps, N),
           "upload_per_image": host_windows(lambda: torch.from_numpy(host).to(dev), args.rounds, N)}
    roof_ms = H0 * W0 * 3 / (STREAM_TBPS * 1e12) * 1e3
    res["roofline"] = {"bytes_in_per_image": H0 * W0 * 3, "stream_tbps": STREAM_TBPS, "ms_per_image": round(roof_ms, 4),
                       "share_of_roofline": round(roof_ms / res["device_per_image"]["median_ms"], 4)}
    res["device_plus_upload_per_image_ms"] = round(res["device_per_image"]["median_ms"]
                                                   + res["upload_per_image"]["median_ms"], 4)
    try:
        from PIL import Image
    except ImportError:
        res["pillow_per_image"], res["bytes_equal_pillow"] = None, None
    else:
        im = Image.fromarray(host[0])

        def pillow():
            t = torch.from_numpy(np.array(im.resize(size))) / 255.0
            t = t.permute(2, 0, 1)
            gray = (0.299 * t[0] + 0.587 * t[1] + 0.114 * t[2])[None]
            return t.to(dev), gray.to(dev)

        res["pillow_per_image"] = host_windows(pillow, args.rounds, 1)
        res["bytes_equal_pillow"] = bool(np.array_equal(small[0].cpu().numpy(), np.asarray(im.resize(size))))
        res["pillow_over_device_plus_upload"] = round(res["pillow_per_image"]["median_ms"]
                                                      / res["device_plus_upload_per_image_ms"], 2)
    res["device"] = torch.cuda.get_device_name(0)
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "viewprep_bench.json"), "w") as fp:
        json.dump(res, fp, indent=1)
        fp.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
