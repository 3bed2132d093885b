"""TnT F-score evaluation timing (development / DESIGN §6i numbers) -> profiles/tnt_eval_bench.json.

A bumpy height field of n x n cells at 0.01 spacing as the mesh (its vertices
plus face centroids are the evaluated cloud: 3 n^2 points) and a denser
jittered copy of the same surface as the scanner cloud (30 n^2 points; n = 1000:
3M mesh-derived points against 30M), an L-shaped crop, tau = 0.01 and an
initial transform off by a small similarity.  Per size: the GPU time of every
stage of crop, voxel grid, index build and query (the stage_ms arrays of the C
calls: one warm-up call, then the median of `reps`), the ICP's time per
iteration, the whole of tnt_fscore (host wall time around a synchronised call,
one warm-up then the median of 3), the scratch bytes, and 20 queries against
one built index next to 20 calls of gsr_points_nearest on the same clouds.  The
baseline is the numpy / scipy restatement of the test suite
(tests/tnteval_ref.py, cKDTree with 16 workers) at a size it finishes in under
a minute; its counts are compared with the device's on the way.

    python tools/bench_tnt_eval.py [n ...]      (default 100 1000; the restatement runs for n <= 120)
"""
import json, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "geometry-grounded-gaussian-splatting_amd"), os.path.join(ROOT, "tests")]
import numpy as np
import torch
import gsr_eval as E
import gsr_tnt as G
import tnteval_ref as R

sizes = [int(a) for a in sys.argv[1:]] or [100, 1000]
dev = torch.device("cuda", 0)
reps, TAU, H = 3, 0.01, 0.01


def bumps(x, y):
    return 0.02 * torch.sin(40.0 * x) * torch.cos(33.0 * y) + 0.008 * torch.sin(90.0 * x + 60.0 * y)


def case(n):
    g = torch.Generator(device=dev)
    g.manual_seed(n)
    ax = torch.arange(n + 1, device=dev, dtype=torch.float64) * H
    gx, gy = torch.meshgrid(ax, ax, indexing="ij")
    v = torch.stack([gx, gy, bumps(gx, gy)], -1).reshape(-1, 3)
    idx = torch.arange((n + 1) * (n + 1), device=dev).reshape(n + 1, n + 1)
    a, b, c, d = idx[:-1, :-1].reshape(-1), idx[1:, :-1].reshape(-1), idx[:-1, 1:].reshape(-1), idx[1:, 1:].reshape(-1)
    f = torch.cat([torch.stack([a, b, c], 1), torch.stack([d, c, b], 1)])
    S = 30 * n * n
    xy = torch.rand(S, 2, generator=g, device=dev, dtype=torch.float64) * (H * n)
    gt = torch.cat([xy, bumps(xy[:, :1], xy[:, 1:])], 1) + 0.1 * TAU * torch.randn(S, 3, generator=g, device=dev,
                                                                                    dtype=torch.float64)
    L = H * n
    ell = np.array([(0.05, 0.05), (0.95, 0.05), (0.95, 0.45), (0.5, 0.45), (0.5, 0.95), (0.05, 0.95)]) * L
    poly = np.zeros((6, 3))
    poly[:, :2] = ell
    crop = {"orthogonal_axis": "Z", "axis_min": -1.0, "axis_max": 1.0, "bounding_polygon": poly}
    off = np.eye(4)
    th = np.radians(0.2)
    off[:3, :3] = 1.002 * np.array([[np.cos(th), -np.sin(th), 0], [np.sin(th), np.cos(th), 0], [0, 0, 1]])
    off[:3, 3] = [0.8 * TAU, -0.6 * TAU, 0.5 * TAU]
    v = torch.as_tensor(R.transform_ref(v.cpu().numpy(), off), device=dev)
    return v, f, gt, crop, np.linalg.inv(off)


def staged(fn):
    G.measure_stages = False
    fn()  # warm-up: first-call costs stay out of the numbers
    G.measure_stages = True
    runs = []
    for _ in range(reps):
        out = fn()
        runs.append(out[-1])
    G.measure_stages = False
    med = {k: round(statistics.median(r["stage_ms"][k] for r in runs), 4) for k in runs[0]["stage_ms"]}
    return out, med, runs[0]["scratch_bytes"]


def wall(fn, n=3):
    torch.cuda.synchronize()
    ts = []
    for _ in range(n + 1):
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return out, round(statistics.median(ts[1:]), 3)


rows = []
for n in sizes:
    v, f, gt, crop, init = case(n)
    pcd = torch.cat([v, ((v[f[:, 0]] + v[f[:, 1]]) + v[f[:, 2]]) / 3.0]).contiguous()
    (_, s_crop, _), ms_crop_s, sc_crop_s = staged(lambda: G.crop_points(pcd, crop, init))
    (_, t_crop, _), ms_crop_t, sc_crop_t = staged(lambda: G.crop_points(gt, crop))
    (s_vox, _), ms_vox_s, sc_vox_s = staged(lambda: G.voxel_down_sample(s_crop, TAU / 2))
    (t_vox, _), ms_vox_t, sc_vox_t = staged(lambda: G.voxel_down_sample(t_crop, TAU / 2))

    def build():
        ix = G.NearestIndex.build(t_vox)
        return ix, ix.build_stats
    (ix, _), ms_build, sc_build = staged(build)
    (_, _, _), ms_query, sc_query = staged(lambda: ix.query(s_vox, 2 * TAU))

    def twenty_indexed():
        one = G.NearestIndex.build(t_vox)
        for _ in range(20):
            d, _, _ = one.query(s_vox, 2 * TAU)
        return d

    def twenty_nearest():
        for _ in range(20):
            d = E.nearest_distance(s_vox, t_vox, 2 * TAU)
        return d
    d_a, ms20_indexed = wall(twenty_indexed)
    d_b, ms20_nearest = wall(twenty_nearest)
    assert torch.equal(d_a.view(torch.int64), d_b.view(torch.int64))
    icp, ms_icp = wall(lambda: G.registration_icp(s_vox, ix, 2 * TAU, 20), n=1)
    out, ms_whole = wall(lambda: G.tnt_fscore(v, f, gt, crop, init, TAU))
    row = {"what": f"TnT F-score evaluation, {n} x {n} height field at {H}, tau {TAU}",
           "mesh_points": int(pcd.shape[0]), "scanner_points": int(gt.shape[0]),
           "cropped": [int(s_crop.shape[0]), int(t_crop.shape[0])], "voxels": [int(s_vox.shape[0]), int(t_vox.shape[0])],
           "crop_stage_ms": {"source": ms_crop_s, "target": ms_crop_t},
           "voxel_stage_ms": {"source": ms_vox_s, "target": ms_vox_t},
           "index_build_stage_ms": ms_build, "index_query_stage_ms": ms_query,
           "icp_iterations": icp["iterations"], "icp_wall_ms_per_iteration": round(ms_icp / max(icp["iterations"], 1), 3),
           "tnt_fscore_wall_ms_median": ms_whole,
           "twenty_queries_one_index_wall_ms": ms20_indexed, "twenty_points_nearest_wall_ms": ms20_nearest,
           "ratio_nearest_over_indexed": round(ms20_nearest / ms20_indexed, 2),
           "scratch_bytes": {"crop": [sc_crop_s, sc_crop_t], "voxel": [sc_vox_s, sc_vox_t], "index_build": sc_build,
                             "index_query": sc_query, "index_bytes": ix.build_stats["index_bytes"]},
           "precision": out["precision"], "recall": out["recall"], "fscore": out["fscore"],
           "registration_iterations": [r["iterations"] for r in out["registrations"]]}
    if n <= 120:
        v_np, f_np, gt_np = v.cpu().numpy(), f.cpu().numpy(), gt.cpu().numpy()
        t0 = time.perf_counter()
        want = R.tnt_fscore_ref(v_np, f_np, gt_np, crop, init, TAU, nearest_factory=R.kdtree_nearest_factory(16))
        cpu_ms = (time.perf_counter() - t0) * 1e3
        same = all(out[k] == want[k] for k in ("n_source", "n_target", "n_precise", "n_recalled"))
        row.update(restatement_cpu_ms=round(cpu_ms, 1), equals_restatement=bool(same),
                   ratio_restatement_over_tnt_fscore=round(cpu_ms / ms_whole, 1))
    print(json.dumps(row), flush=True)
    rows.append(row)
    del pcd, s_crop, t_crop, s_vox, t_vox, ix, gt, out, icp, d_a, d_b
    torch.cuda.empty_cache()

out = os.path.join(ROOT, "profiles", "tnt_eval_bench.json")
try:
    with open(out, "w") as fh:
        json.dump(rows, fh, indent=1)
        fh.write("\n")
except OSError as e:
    print(f"not written: {out}: {e}", file=sys.stderr)
