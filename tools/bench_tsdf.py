#!/usr/bin/env python3
"""Times TSDF fusion and marching cubes (gsr_tsdf, csrc/tsdf.hip) at the scale
of the reference's DTU run: 49 and 64 views of 1200x1600, voxel_size 0.002,
blocks of 16^3, analytic depth maps of a sphere seen from a ring of cameras.
Writes profiles/tsdf_bench.json: per-stage GPU milliseconds (device events,
after one untimed warm-up fusion), the bytes each stage must move, and the
integrate kernel's achieved bandwidth.  Needs a HIP device; no fallback.

    python tools/bench_tsdf.py [--views 49 64] [--out profiles/tsdf_bench.json]
"""
from __future__ import annotations

import argparse
import json
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "geometry-grounded-gaussian-splatting_amd"))

import torch  # noqa: E402

H, W, FX = 1200, 1600, 1450.0
RADIUS, DIST, VOXEL = 0.25, 1.0, 0.002


def view(i, n, dev):
    """Camera i of n on a ring around the sphere (slightly tilted), its depth map by exact ray-sphere intersection."""
    th = 2 * math.pi * i / n
    eye = torch.tensor([DIST * math.cos(th), 0.3 * math.sin(2 * th), DIST * math.sin(th)], dtype=torch.float64)
    z = -eye / eye.norm()
    x = torch.linalg.cross(torch.tensor([0.0, 1.0, 0.0], dtype=torch.float64), z)
    x = x / x.norm()
    y = torch.linalg.cross(z, x)
    e = torch.eye(4, dtype=torch.float64)
    e[:3, :3] = torch.stack([x, y, z])
    e[:3, 3] = -e[:3, :3] @ eye
    k = (FX, FX, (W - 1) / 2, (H - 1) / 2)
    ys, xs = torch.meshgrid(torch.arange(H, device=dev, dtype=torch.float64),
                            torch.arange(W, device=dev, dtype=torch.float64), indexing="ij")
    d = torch.stack([(xs - k[2]) / FX, (ys - k[3]) / FX, torch.ones_like(xs)], -1)
    c = e[:3, 3].to(dev)  # the sphere's centre (the origin) in camera space
    a, b, q = (d * d).sum(-1), -2 * (d @ c), c @ c - RADIUS ** 2
    disc = b * b - 4 * a * q
    t = torch.where(disc > 0, (-b - disc.clamp(min=0).sqrt()) / (2 * a), torch.zeros_like(a))
    depth = t.clamp(min=0).float().contiguous()
    color = torch.stack([xs / W, ys / H, 0.5 * torch.ones_like(xs)], -1).float().contiguous()
    return depth, color, k, e


def fuse(views, dev, timed):
    import gsr_tsdf as T

    g = T.VoxelBlockGrid(VOXEL, 16, device=dev, block_count=4096)
    ev = lambda: torch.cuda.Event(enable_timing=True)  # noqa: E731
    touch_ms = integrate_ms = 0.0
    blocks_listed = updated = 0
    for depth, color, k, e in views:
        t0, t1, t2 = ev(), ev(), ev()
        before = float(g.weight.sum()) if timed else 0.0
        t0.record()
        blocks = g.compute_unique_block_coordinates(depth, k, e)
        t1.record()
        g.integrate(blocks, depth, color, k, e)
        t2.record()
        torch.cuda.synchronize()
        touch_ms += t0.elapsed_time(t1)
        integrate_ms += t1.elapsed_time(t2)  # includes the index rebuild when blocks are added
        blocks_listed += blocks.shape[0]
        if timed:
            updated += int(round(float(g.weight.sum()) - before))
    T.last_call_stats = {}
    t0, t1 = ev(), ev()
    t0.record()
    v, f, c = g.extract_triangle_mesh()
    t1.record()
    torch.cuda.synchronize()
    stats = dict(T.last_call_stats)
    T.last_call_stats = None
    # integrate reads tsdf, weight and colour of every listed voxel (20 B) and writes the updated ones back
    nbytes = blocks_listed * 4096 * 20 + updated * 20
    return {"views": len(views), "blocks": g.num_blocks, "blocks_listed": blocks_listed, "voxels_updated": updated,
            "touch_ms": touch_ms, "integrate_ms": integrate_ms, "integrate_bytes": nbytes,
            "integrate_GBps_including_host_side": nbytes / integrate_ms / 1e6,
            "extract_ms": t0.elapsed_time(t1), "extract_stage_ms": {k: stats[k] for k in T.EXTRACT_STAGES},
            "extract_scratch_bytes": stats["scratch_bytes"], "grid_bytes": g.num_blocks * 4096 * 20,
            "vertices": int(v.shape[0]), "faces": int(f.shape[0])}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--views", type=int, nargs="+", default=[49, 64])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tsdf_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_tsdf: needs a HIP device")
    dev = torch.device("cuda", 0)
    results = []
    for n in args.views:
        views = [view(i, n, dev) for i in range(n)]
        fuse(views[:4], dev, timed=False)  # warm-up: code objects, allocator
        results.append(fuse(views, dev, timed=True))
        print(json.dumps(results[-1]))
    with open(args.out, "w") as fh:
        json.dump({"device": torch.cuda.get_device_name(0), "image": [H, W], "voxel_size": VOXEL,
                   "block_resolution": 16, "results": results}, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
