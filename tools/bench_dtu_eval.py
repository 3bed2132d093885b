"""DTU Chamfer evaluation timing (development / DESIGN §6g numbers) -> profiles/dtu_eval_bench.json.

A bumpy height field of n x n cells at 1.3 spacing (n = 1000: 2M triangles,
about 27M sampled points at density 0.2) and a scanner cloud of 3M points
scattered around it.  Per size: the GPU time of every stage of
sample_mesh_points, downsample_points and of the two nearest_distance queries
(the stage_ms arrays of the three C calls: one warm-up call, then the median of
`reps` calls), the rounds of the thinning, the scratch bytes, and dtu_chamfer
as a whole (host wall time around a synchronised call, masking and readbacks
included).  The baseline is the numpy / scipy restatement of the test suite
(tests/dtueval_ref.py, CPU, 16 KD-tree workers) at a size it finishes in under
a minute; its kept set and distances are compared with the device's on the way.

    python tools/bench_dtu_eval.py [n ...]      (default 100 1000; the restatement runs for n <= 150)
"""
import json, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "geometry-grounded-gaussian-splatting_amd"), os.path.join(ROOT, "tests")]
import numpy as np
import torch
import gsr_eval as E
import dtueval_ref as R

sizes = [int(a) for a in sys.argv[1:]] or [100, 1000]
dev = torch.device("cuda", 0)
reps, DENSITY, MAX_DIST, SPACING = 3, 0.2, 20.0, 1.3


def case(n):
    g = torch.Generator(device=dev)
    g.manual_seed(n)
    ax = torch.arange(n + 1, device=dev, dtype=torch.float64) * SPACING
    gx, gy = torch.meshgrid(ax, ax, indexing="ij")
    gz = 2.0 * torch.sin(0.05 * gx) * torch.cos(0.04 * gy) + 0.05 * torch.randn(gx.shape, generator=g, device=dev,
                                                                               dtype=torch.float64)
    v = torch.stack([gx, gy, gz], -1).reshape(-1, 3).float()
    idx = torch.arange((n + 1) * (n + 1), device=dev).reshape(n + 1, n + 1)
    a, b, c, d = idx[:-1, :-1].reshape(-1), idx[1:, :-1].reshape(-1), idx[:-1, 1:].reshape(-1), idx[1:, 1:].reshape(-1)
    f = torch.cat([torch.stack([a, b, c], 1), torch.stack([d, c, b], 1)])
    S = max(3000, 3 * n * n)
    xy = torch.rand(S, 2, generator=g, device=dev, dtype=torch.float64) * (SPACING * n + 4) - 2
    z = 2.0 * torch.sin(0.05 * xy[:, 0]) * torch.cos(0.04 * xy[:, 1]) + 0.3 * torch.randn(S, generator=g, device=dev,
                                                                                        dtype=torch.float64)
    stl = torch.cat([xy, z[:, None]], 1).float()
    stl[: S // 50, 2] += 40.0
    bb = np.array([[-5.0, -5.0, -8.0], [SPACING * n + 5, SPACING * n + 5, 8.0]])
    obs = torch.ones(64, 64, 16, dtype=torch.bool, device=dev)
    res = float((bb[1] - bb[0]).max() / 63)
    return v, f, stl, obs, bb, res, np.array([0.0, 0.0, 1.0, 5.0])


def staged(fn):
    E.last_call_stats = None
    fn()  # warm-up: first-call costs stay out of the numbers
    runs = []
    for _ in range(reps):
        E.last_call_stats = {}
        out = fn()
        runs.append(dict(E.last_call_stats))
    E.last_call_stats = None
    med = {k: round(statistics.median(r[k] for r in runs), 4) for k in runs[0] if k not in ("scratch_bytes", "num_rounds")}
    return out, med, runs[0]


rows = []
for n in sizes:
    v, f, stl, obs, bb, res, plane = case(n)
    stl64 = stl.double()
    sampled, ms_sample, st_sample = staged(lambda: E.sample_mesh_points(v, f, DENSITY))
    perm = torch.randperm(sampled.shape[0], device=dev, generator=torch.Generator(device=dev).manual_seed(1))
    (down, kept), ms_thin, st_thin = staged(lambda: E.downsample_points(sampled, DENSITY, perm=perm))
    d2s, ms_d2s, st_d2s = staged(lambda: E.nearest_distance(down, stl64, MAX_DIST))
    s2d, ms_s2d, st_s2d = staged(lambda: E.nearest_distance(stl64, down, MAX_DIST))
    torch.cuda.synchronize()
    walls = []
    for _ in range(reps + 1):
        t0 = time.perf_counter()
        out = E.dtu_chamfer(v, f, stl, obs, bb, res, plane, density=DENSITY, max_dist=MAX_DIST, perm=perm)
        torch.cuda.synchronize()
        walls.append((time.perf_counter() - t0) * 1e3)
    row = {"what": f"DTU Chamfer evaluation, {n} x {n} height field at {SPACING}, density {DENSITY}, max_dist {MAX_DIST}",
           "triangles": int(f.shape[0]), "sampled": int(sampled.shape[0]), "kept": int(down.shape[0]),
           "stl": int(stl.shape[0]), "sample_stage_ms": ms_sample, "thin_stage_ms": ms_thin,
           "thin_rounds": st_thin["num_rounds"], "d2s_stage_ms": ms_d2s, "s2d_stage_ms": ms_s2d,
           "stage_ms_sum": round(sum(sum(m.values()) for m in (ms_sample, ms_thin, ms_d2s, ms_s2d)), 3),
           "scratch_bytes": {"sample": st_sample["scratch_bytes"], "thin": st_thin["scratch_bytes"],
                             "d2s": st_d2s["scratch_bytes"], "s2d": st_s2d["scratch_bytes"]},
           "dtu_chamfer_wall_ms_median": round(statistics.median(walls[1:]), 3),
           "mean_d2s": out["mean_d2s"], "mean_s2d": out["mean_s2d"]}
    if n <= 150:
        torch.set_num_threads(16)
        v_np, f_np, perm_np = v.cpu().numpy(), f.cpu().numpy(), perm.cpu().numpy()
        t0 = time.perf_counter()
        pcd = R.sample_mesh_points_ref(v_np, f_np, DENSITY)
        t1 = time.perf_counter()
        rdown, rkept = R.downsample_ref(pcd, DENSITY, perm_np, workers=16)
        t2 = time.perf_counter()
        stl_np = stl64.cpu().numpy()
        rd2s = R.nearest_ref(rdown, stl_np, MAX_DIST, workers=16)
        rs2d = R.nearest_ref(stl_np, rdown, MAX_DIST, workers=16)
        t3 = time.perf_counter()
        fin = np.isfinite(rd2s)
        same = bool(np.array_equal(rkept, kept.cpu().numpy()) and np.array_equal(pcd.shape, tuple(sampled.shape))
                    and np.array_equal(fin, torch.isfinite(d2s).cpu().numpy())
                    and np.allclose(rd2s[fin], d2s.cpu().numpy()[fin], rtol=1e-12, atol=0)
                    and np.allclose(rs2d[np.isfinite(rs2d)], s2d.cpu().numpy()[np.isfinite(rs2d)], rtol=1e-12, atol=0))
        row.update(restatement_cpu_ms={"sample": round((t1 - t0) * 1e3, 1), "thin": round((t2 - t1) * 1e3, 1),
                                       "nearest_both": round((t3 - t2) * 1e3, 1)},
                   restatement_cpu_total_ms=round((t3 - t0) * 1e3, 1), equals_restatement=same,
                   ratio_restatement_over_stage_sum=round((t3 - t0) * 1e3 / row["stage_ms_sum"], 1))
    print(json.dumps(row), flush=True)
    rows.append(row)
    del sampled, down, kept, d2s, s2d, out, perm
    torch.cuda.empty_cache()

out = os.path.join(ROOT, "profiles", "dtu_eval_bench.json")
try:
    with open(out, "w") as fh:
        json.dump(rows, fh, indent=1)
        fh.write("\n")
except OSError as e:
    print(f"not written: {out}: {e}", file=sys.stderr)
