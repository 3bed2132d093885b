"""Mesh clean-up timing (development / DESIGN §6f numbers) -> profiles/meshclean_bench.json.

The marching-tetrahedra mesh of a sphere plus a ripple over a structured grid
of n^3 cells (tests/tetmesh_ref.kuhn_grid; n = 384: about 3M triangles) with
4000 small floaters of 4 to 60 triangles added, triangle order shuffled.  Per
size: post_process_mesh as a whole (host wall time around a synchronised call,
size readbacks included), cluster_connected_triangles with areas, the GPU time
of each of its stages (gsr_mesh_clusters' stage_ms), the scratch bytes per
triangle, the edge sort's bytes against its time, and the numpy / scipy
restatement of the test suite (tests/meshclean_ref.py, CPU) on the same mesh:
the only baseline there is.  The restatement's clusters and filtered mesh are
compared with the device's on the way.

    python tools/bench_meshclean.py [n ...]      (default 96 192 384)
"""
import json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "geometry-grounded-gaussian-splatting_amd"), os.path.join(ROOT, "tests")]
import numpy as np
import torch
import gsr_mesh as M
import meshclean_ref as R
import tetmesh_ref as T

sizes = [int(a) for a in sys.argv[1:]] or [96, 192, 384]
dev = torch.device("cuda", 0)
steps = 5


def case(n):
    pts, tets = T.kuhn_grid(n, device=dev, dtype=torch.int32)
    sdf = pts.norm(dim=1) - 0.6 + 0.05 * torch.sin(8 * pts[:, 0]) * torch.sin(8 * pts[:, 1]) * torch.sin(8 * pts[:, 2])
    ids, faces = M.marching_tetrahedra_ids(tets, sdf.contiguous(), torch.ones(sdf.numel(), dtype=torch.bool, device=dev))
    verts = (pts[ids[:, 0]] + pts[ids[:, 1]]) * 0.5
    v, f = R.with_floaters(verts.cpu().numpy(), faces.cpu().numpy(), n=4000, seed=n)
    return torch.from_numpy(v).to(dev), torch.from_numpy(f).to(dev), v, f


def timed(fn, reps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps * 1e3, out


rows = []
for n in sizes:
    v, f, v_np, f_np = case(n)
    F, V = f.shape[0], v.shape[0]
    M.last_call_stats = None
    timed(lambda: M.post_process_mesh(v, f, 1), 2)
    ms_post, (pv, pf) = timed(lambda: M.post_process_mesh(v, f, 1), steps)
    ms_clusters, (labels, counts, area) = timed(lambda: M.cluster_connected_triangles(v, f), steps)
    M.last_call_stats = {}
    M.cluster_connected_triangles(v, f)
    st = dict(M.last_call_stats)
    M.last_call_stats = None
    t0 = time.perf_counter()
    ref = R.cluster_connected_triangles_ref(v_np, f_np)
    ref_ms = (time.perf_counter() - t0) * 1e3
    t0 = time.perf_counter()
    rv, rf = R.post_process_mesh_ref(v_np, f_np, 1)
    ref_post_ms = (time.perf_counter() - t0) * 1e3
    same = bool(np.array_equal(labels.cpu().numpy(), ref[0]) and np.array_equal(counts.cpu().numpy(), ref[1])
                and np.array_equal(pv.cpu().numpy(), rv) and np.array_equal(pf.cpu().numpy(), rf))
    bits = max(1, (V - 1).bit_length())
    passes = -(-2 * bits // 8)
    sort_bytes = 3 * F * (8 + 4) * 2 * passes  # keys and slots read and written once per 8-bit pass
    row = {"what": f"mesh clean-up, grid {n}^3 sphere + 4000 floaters, int64 faces", "F": F, "V": V,
           "clusters": int(counts.shape[0]), "F_kept": int(pf.shape[0]), "V_kept": int(pv.shape[0]),
           "post_process_mesh_ms": round(ms_post, 3), "cluster_connected_triangles_ms": round(ms_clusters, 3),
           "stage_ms": {k: round(st[k], 4) for k in M.CLEAN_STAGES},
           "stage_ms_sum": round(sum(st[k] for k in M.CLEAN_STAGES), 3),
           "scratch_bytes": st["scratch_bytes"], "scratch_bytes_per_triangle": round(sum(st["scratch_bytes"]) / F, 1),
           "sort_key_bits": 2 * bits, "sort_traffic_bytes_8bit_passes": sort_bytes,
           "sort_GBps": round(sort_bytes / (st["sort"] * 1e-3) / 1e9, 1) if st["sort"] > 0 else None,
           "restatement_cpu_clusters_ms": round(ref_ms, 1), "restatement_cpu_post_process_ms": round(ref_post_ms, 1),
           "equals_restatement": same}
    print(json.dumps(row), flush=True)
    rows.append(row)
    del v, f, labels, counts, area, pv, pf
    torch.cuda.empty_cache()

out = os.path.join(ROOT, "profiles", "meshclean_bench.json")
try:
    with open(out, "w") as fh:
        json.dump(rows, fh, indent=1)
        fh.write("\n")
except OSError as e:
    print(f"not written: {out}: {e}", file=sys.stderr)
