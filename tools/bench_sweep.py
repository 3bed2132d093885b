"""The tetrahedral extraction sweep at full size (development / DESIGN §6k numbers) -> profiles/field_sweep_bench.json.

1M Gaussians (the C3 scene), one 1080p view, the 15M tetra points of
GaussianModel.get_tetra_points: one iteration of the per-view loop of
mesh_extract_tetrahedra.py:74-82 over all the points at once, with and without
a 1080p gt_mask (an ellipse).  Per view, each the median of `steps` runs after 2
warm-up runs, with the smallest and largest beside it:

  integrate        gaussian_renderer.integrate alone (host clock around a synchronised call);
  view_torch       integrate + the torch glue of gsr_mesh.alpha_cull_sdf (sweep="torch");
  view_hip         integrate + gsr_field_view_update (sweep="hip");
  glue_torch       the torch glue alone on held integrate outputs (device events);
  update_hip       gsr_field_view_update alone on the same outputs, the state reset before every run
                   so that every run writes what the first view of a sweep writes (device events),
                   with the bytes it must move (counted from the data, see `update_bytes`) over
                   its time against the 6.3 TB/s a copy reaches on this chip.

Then both sweeps end to end (alpha_cull_sdf over 6 views, every other one masked, the reference's
chunking: 2 chunks of 7.5M points) with their peak allocator bytes above what is resident before the
call, and one bisection step at E = 3M edges both ways.  The two sweeps' results are compared.

    python tools/bench_sweep.py [steps]      (default 10)
"""
import json, math, os, statistics, sys, time, types
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "geometry-grounded-gaussian-splatting_amd")]
import torch
import gsr_mesh as M
import gsr_scene as S
from diff_gaussian_rasterization._abi import call, f32ptr, ptr, stream
from gaussian_renderer import integrate

steps = int(sys.argv[1]) if len(sys.argv) > 1 else 10
dev = torch.device("cuda", 0)
W, H, P, E = 1920, 1080, 1_000_000, 3_000_000
COPY_BPS = 6.3e12
inp = {k: v.to(dev).contiguous() for k, v in S.activated_inputs(S.make_gaussians(P, aspect=H / W)).items()}
pc = types.SimpleNamespace(get_xyz=inp["means3D"], get_opacity_with_3D_filter=inp["opacities"],
                           get_scaling_with_3D_filter=inp["scales"], get_rotation=inp["rotations"],
                           active_sh_degree=3, active_sg_degree=0)
pipe = types.SimpleNamespace(debug=False, compute_cov3D_python=False)
pts = S.tetra_points(inp)
N = pts.shape[0]
yy, xx = torch.meshgrid(torch.arange(H, device=dev), torch.arange(W, device=dev), indexing="ij")
ellipse = ((((xx - W / 2) / (0.42 * W)) ** 2 + ((yy - H / 2) / (0.42 * H)) ** 2) < 1).float()[None]


def make_view(cam, mask):
    cam = cam.to(dev)
    wvt = cam.world_view_transform
    return types.SimpleNamespace(**{k: getattr(cam, k) for k in cam.__dataclass_fields__}, R=wvt[:3, :3], T=wvt[3, :3],
                                 Fx=W / (2 * math.tan(cam.FoVx / 2)), Fy=H / (2 * math.tan(cam.FoVy / 2)),
                                 Cx=(W - 1) / 2, Cy=(H - 1) / 2, gt_mask=mask)


def spread(ms):
    return {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4)}


def host_timed(fn):
    """ms of `steps` synchronised calls after 2 warm-up calls (host clock: `integrate` reads its count back)."""
    ms = []
    for k in range(steps + 2):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
    return spread(ms[2:])


def event_timed(fn, before=lambda: None):
    ms = []
    for k in range(steps + 2):
        before()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
    return spread(ms[2:])


def torch_glue(view, ret, weight, seen):
    ok = M._view_mask(view, pts, ret["inside"].bool())
    seen |= ok
    return torch.where(ok, torch.minimum(ret["alpha_integrated"], weight), weight)


def hip_update(cam, ret, weight, seen):
    if cam is None:
        call(dev, "gsr_field_view_update", N, None, ptr(ret["alpha_integrated"]), ptr(ret["inside"]), None, None, 0.0,
             0.0, 0.0, 0.0, 0, 0, None, ptr(weight), ptr(seen), stream(dev))
    else:
        R, T, Fx, Fy, Cx, Cy, w, h, plane = cam
        call(dev, "gsr_field_view_update", N, ptr(pts), ptr(ret["alpha_integrated"]), ptr(ret["inside"]), f32ptr(R),
             f32ptr(T), Fx, Fy, Cx, Cy, w, h, ptr(plane), ptr(weight), ptr(seen), stream(dev))


out = {"device": torch.cuda.get_device_name(0), "gaussians": P, "points": N, "image": [H, W], "steps": steps,
       "library": os.path.relpath(os.environ["GSR_LIB"], ROOT) if os.environ.get("GSR_LIB") else "libgsr.so",
       "per_view": {}}
for name, mask in (("no_mask", None), ("mask_1080p", ellipse)):
    view = make_view(S.make_camera(W, H), mask)
    cam = M._sweep_views([view], dev)[0][1]
    ret = integrate(pts, view, pc, pipe, 0.0)
    state = {"w": torch.ones(N, device=dev), "s": torch.zeros(N, dtype=torch.bool, device=dev)}

    def reset():
        state["w"].fill_(1)
        state["s"].zero_()

    def view_torch():
        r = integrate(pts, view, pc, pipe, 0.0)
        state["w"] = torch_glue(view, r, state["w"], state["s"])

    def view_hip():
        hip_update(cam, integrate(pts, view, pc, pipe, 0.0), state["w"], state["s"].view(torch.uint8))

    row = {"integrate": host_timed(lambda: integrate(pts, view, pc, pipe, 0.0))}
    reset()
    row["view_torch"] = host_timed(view_torch)
    want = (state["w"].clone(), state["s"].clone())
    reset()
    row["view_hip"] = host_timed(view_hip)
    # (at 1080p an ulp of the pixel coordinate moves the sample by ~1e-4: a few of the 15M points can sit that
    # close to the 0.5 bar, where the two formulations' roundings decide differently)
    row["points_that_differ"] = int(((want[0] != state["w"]) | (want[1] != state["s"])).sum())
    row["glue_torch"] = event_timed(lambda: torch_glue(view, ret, state["w"], state["s"]), reset)
    row["update_hip"] = event_timed(lambda: hip_update(cam, ret, state["w"], state["s"].view(torch.uint8)), reset)
    row["glue_by_difference_ms"] = round(row["view_torch"]["median_ms"] - row["integrate"]["median_ms"], 4)
    # what the update must move: `inside` of every point; alpha and weight of the points inside, with a mask their
    # three coordinates; of the points that pass, the `seen` byte and, alpha being below the 1 the state starts
    # at, the weight word (mask texels stay in L2 and are not counted)
    inside = ret["inside"].bool()
    ok = M._view_mask(view, pts, inside)
    n_in, n_ok = int(inside.sum()), int(ok.sum())
    n_upd = int((ok & (ret["alpha_integrated"] < 1)).sum())
    nbytes = N + n_in * (8 + (12 if mask is not None else 0)) + n_ok + 4 * n_upd
    row["update_bytes"] = {"points_inside": n_in, "points_ok": n_ok, "weights_written": n_upd, "bytes": nbytes,
                           "bytes_per_point": round(nbytes / N, 3),
                           "bytes_per_point_all_ok": 26 if mask is not None else 14}
    bps = nbytes / (row["update_hip"]["median_ms"] * 1e-3)
    row["update_bytes_per_s"] = bps
    row["update_fraction_of_copy_ceiling"] = round(bps / COPY_BPS, 4)
    out["per_view"][name] = row
    print(json.dumps({name: row}), flush=True)
    del ret, state, want, inside, ok

# both sweeps end to end, the reference's chunking, and their allocator peaks
views = [make_view(c, ellipse if k % 2 else None) for k, c in enumerate(S.orbit_cameras(6, W, H))]
sweeps = {}
for sweep in ("torch", "hip", "torch", "hip"):  # alternating; the first pair warms up
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats(dev)
    base = torch.cuda.memory_allocated(dev)
    t0 = time.perf_counter()
    res = M.alpha_cull_sdf(pts, views, pc, pipe, 0.0, sweep=sweep)
    torch.cuda.synchronize()
    sweeps[sweep] = {"ms": round((time.perf_counter() - t0) * 1e3, 3), "views": len(views),
                     "peak_bytes_above_resident": torch.cuda.max_memory_allocated(dev) - base,
                     "result_bytes": sum(t.numel() * t.element_size() for t in res)}
    sweeps[sweep + "_result"] = res
    del res
out["sweep"] = {k: v for k, v in sweeps.items() if not k.endswith("_result")}
out["sweep"]["points_that_differ"] = int(((sweeps["torch_result"][0] != sweeps["hip_result"][0])
                                          | (sweeps["torch_result"][1] != sweeps["hip_result"][1])).sum())
del sweeps

# one bisection step at E edges
g = torch.Generator(device=dev).manual_seed(0)
ends = [torch.randn(E, 3, device=dev, generator=g) for _ in range(2)]
sdfs = [torch.rand(E, 1, device=dev, generator=g) - 0.5 for _ in range(3)]


def torch_step():
    left_points, right_points, left_sdf, right_sdf, mid_sdf = b
    mid_points = (left_points + right_points) * 0.5
    low = ((mid_sdf < 0) & (left_sdf < 0)) | ((mid_sdf > 0) & (left_sdf > 0))
    left_sdf = torch.where(low, mid_sdf, left_sdf)
    right_sdf = torch.where(low, right_sdf, mid_sdf)
    left_points = torch.where(low, mid_points, left_points)
    right_points = torch.where(low, right_points, mid_points)
    return left_points, right_points, left_sdf, right_sdf, (left_points + right_points) * 0.5


b = [t.clone() for t in ends + sdfs]
mid = torch.empty(E, 3, device=dev)
out["bisect_step"] = {"edges": E}
torch.cuda.synchronize()
torch.cuda.reset_peak_memory_stats(dev)
base = torch.cuda.memory_allocated(dev)
want = torch_step()
out["bisect_step"]["torch_peak_bytes_above_resident"] = torch.cuda.max_memory_allocated(dev) - base
out["bisect_step"]["torch"] = event_timed(torch_step)


def restore():
    for t, src in zip(b, ends + sdfs):
        t.copy_(src)


out["bisect_step"]["hip"] = event_timed(lambda: M.bisect_step(b[0], b[1], b[2], b[3], b[4], mid), restore)
out["bisect_step"]["same_bits"] = bool(all(torch.equal(x, y) for x, y in zip(want, b[:4] + [mid])))
os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
path = os.path.join(ROOT, "profiles", "field_sweep_bench.json" if not os.environ.get("GSR_LIB") else
                    "field_sweep_bench_" + os.path.splitext(os.path.basename(os.environ["GSR_LIB"]))[0] + ".json")
with open(path, "w") as fh:
    json.dump(out, fh, indent=1)
print(json.dumps(out))
