"""Marching tetrahedra timing (development / DESIGN §6e numbers), one JSON line per grid size.

A structured grid of n^3 cells, each split into 6 tets around its main
diagonal (n = 256: 100M tets, 17M vertices), sdf = a sphere plus a ripple.
Per size: the whole call (host wall time around a synchronised call, size
readbacks included), the GPU time of each stage (gsr_marching_tetrahedra's
stage_ms), E, F, the scratch bytes, and for the three stages that stream the
tets their bandwidth over 16 B x T (int32 tets).  Last line: the plain-torch
restatement of the test suite (tests/tetmesh_ref.py) on the same GPU at the
largest size where it fits.

    python tools/bench_tetmesh.py [n ...]      (default 64 128 256)
"""
import json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "geometry-grounded-gaussian-splatting_amd"), os.path.join(ROOT, "tests")]
import torch
import gsr_mesh as M
import tetmesh_ref as R

sizes = [int(a) for a in sys.argv[1:]] or [64, 128, 256]
dev = torch.device("cuda", 0)
steps = 5


def case(n, dtype):
    pts, tets = R.kuhn_grid(n, device=dev, dtype=dtype)
    sdf = pts.norm(dim=1) - 0.6 + 0.05 * torch.sin(8 * pts[:, 0]) * torch.sin(8 * pts[:, 1]) * torch.sin(8 * pts[:, 2])
    return tets, sdf.contiguous(), torch.ones(sdf.numel(), dtype=torch.bool, device=dev)


def timed(fn, reps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps * 1e3, out


for n in sizes:
    for dtype in (torch.int32, torch.int64):
        tets, sdf, valid = case(n, dtype)
        T, V = tets.shape[0], sdf.numel()
        M.last_call_stats = None
        timed(lambda: M.marching_tetrahedra_ids(tets, sdf, valid), 2)
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.memory_allocated()
        ms, (ids, faces) = timed(lambda: M.marching_tetrahedra_ids(tets, sdf, valid), steps)
        peak = torch.cuda.max_memory_allocated() - before
        M.last_call_stats = {}
        M.marching_tetrahedra_ids(tets, sdf, valid)
        st = dict(M.last_call_stats)
        M.last_call_stats = None
        E, F = ids.shape[0], faces.shape[0]
        row = {"what": f"marching tetrahedra, grid {n}^3, {str(dtype).replace('torch.', '')} tets", "T": T, "V": V,
               "E": E, "F": F, "ms_per_call": round(ms, 3),
               "stage_ms": {k: round(st[k], 4) for k in M.STAGES}, "stage_ms_sum": round(sum(st[k] for k in M.STAGES), 3),
               "scratch_bytes": st["scratch_bytes"],
               "peak_bytes_over_inputs": int(peak), "output_bytes": 16 * E + 24 * F,
               "tet_stream_GBps": {k: round(tets.element_size() * 4 * T / (st[k] * 1e-3) / 1e9, 1) for k in ("count", "emit", "faces") if st[k] > 0}}
        print(json.dumps(row), flush=True)
        del tets, sdf, valid, ids, faces
        torch.cuda.empty_cache()

# the restatement, largest size first; a size that does not fit is reported and skipped
R.marching_tetrahedra_ref(*case(16, torch.int64))  # warm-up of the torch kernels involved
for n in sorted(sizes, reverse=True):
    try:
        tets, sdf, valid = case(n, torch.int32)
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.memory_allocated()
        ms, (ids, faces) = timed(lambda: R.marching_tetrahedra_ref(tets, sdf, valid), 2)
        print(json.dumps({"what": f"torch restatement (tests/tetmesh_ref.py), grid {n}^3", "T": tets.shape[0],
                          "E": ids.shape[0], "F": faces.shape[0], "ms_per_call": round(ms, 3),
                          "peak_bytes_over_inputs": int(torch.cuda.max_memory_allocated() - before)}), flush=True)
        break
    except torch.cuda.OutOfMemoryError:
        print(json.dumps({"what": f"torch restatement, grid {n}^3", "error": "out of memory"}), flush=True)
        del tets, sdf, valid
        torch.cuda.empty_cache()
