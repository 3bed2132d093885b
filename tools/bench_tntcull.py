"""TnT mesh culling timing (development / DESIGN §6j numbers) -> profiles/tnt_cull_bench.json.

A bumpy height field of n x n cells over an 8 x 8 area (2 n^2 triangles; n = 1600: 5.1M) under a ring of
cameras that stand inside the area at eye height and look across it, at the reference's TnT image size and
intrinsics (1920 x 1080): most triangles are smaller than a pixel, the ground near each camera gives a few
large ones.  Measured: the per-stage GPU time of gsr_mesh_view_votes over all views (stage_ms: event pairs
around every stage of every view, summed), the host wall time of the same call without stage events (one
warm-up, then the median of 3), and in a run of its own with fewer views the counters (atomics issued, pixel
centres tested, triangles per class).  Derived: triangle-views per second, and the achieved fraction of two
ceilings of the MI355X: global atomics (1.3 TB/s of 4-byte operands; measured for float adds, taken here as
the yardstick for the integer minimum) over the two raster stages, and HBM streaming (6.3 TB/s) for the bytes
the set-up stage must move per triangle (three 8-byte ids, three gathered 12-byte corners, one 4-byte unit
count).  pyrender is not run: there is no speed-up over the reference in this file.

    python tools/bench_tntcull.py [n [views]]      (default 1600 200)
"""
import json, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "geometry-grounded-gaussian-splatting_amd")]
import numpy as np
import torch
import gsr_tnt as G

n = int(sys.argv[1]) if len(sys.argv) > 1 else 1600
views = int(sys.argv[2]) if len(sys.argv) > 2 else 200
dev = torch.device("cuda", 0)
H, W = 1080, 1920
K = dict(fx=1163.8678928442187, fy=1172.793101201448, cx=962.3120628412543, cy=542.0667209577691)
ATOMIC_BPS, HBM_BPS = 1.3e12, 6.3e12

ax = torch.linspace(-4.0, 4.0, n + 1, device=dev)
gx, gz = torch.meshgrid(ax, ax, indexing="ij")
gy = 0.15 * torch.sin(3.0 * gx) * torch.cos(2.3 * gz) + 0.03 * torch.sin(11.0 * gx + 7.0 * gz)
v = torch.stack([gx, gy, gz], -1).reshape(-1, 3).contiguous()
idx = torch.arange((n + 1) * (n + 1), device=dev).reshape(n + 1, n + 1)
a, b, c, d = (t.reshape(-1) for t in (idx[:-1, :-1], idx[1:, :-1], idx[:-1, 1:], idx[1:, 1:]))
f = torch.cat([torch.stack([a, b, c], 1), torch.stack([d, c, b], 1)]).contiguous()
F, V = f.size(0), v.size(0)
ang = 2 * np.pi * np.arange(views) / views


def look_at(eye, target):
    """Camera -> world 4x4 of an OpenCV camera (x right, y down, z forward) at `eye` looking at `target`."""
    eye, target = np.asarray(eye, float), np.asarray(target, float)
    zc = (target - eye) / np.linalg.norm(target - eye)
    xc = np.cross([0.0, 1.0, 0.0], zc)
    xc /= np.linalg.norm(xc)
    c2w = np.eye(4)
    c2w[:3, 0], c2w[:3, 1], c2w[:3, 2], c2w[:3, 3] = xc, np.cross(zc, xc), zc, eye
    return c2w


c2ws = np.stack([look_at((2.5 * np.cos(t), -0.6, 2.5 * np.sin(t)), (-1.0 * np.cos(t), 0.0, -1.0 * np.sin(t)))
                 for t in ang])
w2cs = np.linalg.inv(c2ws)


def call(count=False, m=w2cs):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    counts, st = G.mesh_view_votes(v, f, m, H, W, **K, count=count)
    torch.cuda.synchronize()
    return counts, st, (time.perf_counter() - t0) * 1e3


call()
G.measure_stages = True
counts, st, _ = call()
G.measure_stages = False
wall = statistics.median(call()[2] for _ in range(3))
sub = w2cs[:: max(1, views // 20)]
_, stc, _ = call(True, sub)
ctr = {k: int(x) for k, x in stc["counters"].items()}
t0 = time.perf_counter()
v2, f2 = G.cull_mesh(v, f, c2ws, H, W, **K)
torch.cuda.synchronize()
cull_ms = (time.perf_counter() - t0) * 1e3

ms = st["stage_ms"]
gpu_ms = sum(ms.values())
raster_ms = ms["setup_small"] + ms["wave_units"]
atomics_per_view = ctr["atomics"] / len(sub)
out = {
    "device": torch.cuda.get_device_name(0), "triangles": F, "vertices": V, "views": views, "image": [H, W],
    "stage_ms_all_views": ms, "gpu_ms_all_views": gpu_ms, "gpu_ms_per_view": gpu_ms / views,
    "wall_ms_votes_call": wall, "wall_ms_cull_mesh": cull_ms,
    "triangle_views_per_s": F * views / (gpu_ms * 1e-3),
    "scratch_bytes": st["scratch_bytes"],
    "counted_views": len(sub), "counters_counted_views": ctr, "atomics_per_view": atomics_per_view,
    "atomic_bytes_per_s": atomics_per_view * views * 4 / (raster_ms * 1e-3),
    "fraction_of_atomic_ceiling": atomics_per_view * views * 4 / (raster_ms * 1e-3) / ATOMIC_BPS,
    "setup_stream_bytes_per_view": F * (24 + 36 + 4),
    "fraction_of_hbm_ceiling_setup": F * (24 + 36 + 4) * views / (ms["setup_small"] * 1e-3) / HBM_BPS,
    "kept_vertices": int(v2.size(0)), "kept_faces": int(f2.size(0)),
    "votes_histogram": torch.bincount(counts.long().clamp(max=40), minlength=41).tolist(),
}
os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
with open(os.path.join(ROOT, "profiles", "tnt_cull_bench.json"), "w") as fh:
    json.dump(out, fh, indent=1)
print(json.dumps(out))
