"""GPU tests of the extraction sweep in HIP (csrc/fieldsweep.hip through the C ABI and gsr_mesh).

Yardstick: tests/fieldsweep_ref.py, the numpy float32 restatement in the
kernels' operation order, which tests/test_fieldsweep.py pins to the
reference's lines; the kernels must match it bit for bit.  The drivers with
sweep="hip" must return what the default torch formulation returns, bit for
bit.  The mask test compares against 0.5, so every tested point's float64
sample lies more than 1e-3 from it (fieldsweep_ref.draw_points for the kernel
cases; asserted here for the scene's tetra points); no point is left out.
"""
from __future__ import annotations

import ctypes
import math
import types

import numpy as np
import pytest
import torch

import fieldsweep_ref as R
import gsr_scene as S
from test_fieldsweep import _state, _with_points_behind, bisect_inputs
from test_tetmesh import SCENE_KW, group

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
SIZES = (0, 1, 63, 64, 65, 257, 70_001)
NMAX = SIZES[-1]
GSR_OK, GSR_ERR_ARGS = 0, 1
KINDS = (None,) + R.KINDS


def _abi():
    from diff_gaussian_rasterization import _abi

    _abi.load()
    return _abi


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _stream(s):
    return ctypes.c_void_p((s or torch.cuda.current_stream(DEV)).cuda_stream)


def _view_update(n, points, alpha, inside, view, weight, seen, stream=None):
    """gsr_field_view_update on device tensors -> the status code."""
    abi = _abi()
    if view is None:
        cam = (None, None, 0.0, 0.0, 0.0, 0.0, 0, 0, None)
    else:
        mask = _dev(view["mask"])
        cam = (abi.f32ptr(np.ascontiguousarray(view["R"])), abi.f32ptr(np.ascontiguousarray(view["T"])), view["Fx"],
               view["Fy"], view["Cx"], view["Cy"], view["W"], view["H"], abi.ptr(mask))
    with torch.cuda.device(DEV):
        return abi.load().gsr_field_view_update(n, abi.ptr(points), abi.ptr(alpha), abi.ptr(inside), *cam,
                                                abi.ptr(weight), abi.ptr(seen), _stream(stream))


def _finish(n, weight, seen, sdf, valid, stream=None):
    abi = _abi()
    with torch.cuda.device(DEV):
        return abi.load().gsr_field_finish(n, abi.ptr(weight), abi.ptr(seen), abi.ptr(sdf), abi.ptr(valid),
                                           _stream(stream))


def _bits(t):
    return t.cpu().numpy().view(np.uint32 if t.dtype == torch.float32 else np.uint64 if t.dtype == torch.float64
                                else np.uint8)


@pytest.fixture(scope="module")
def cases():
    """Per kind of view (None: no mask) NMAX points under the margin rule, 64 of them at or behind the camera
    plane with `inside` clear, shuffled so that every size holds some; the restatement's result computed once
    (it is elementwise: the first n elements are the result for the first n points)."""
    out = {}
    for k, kind in enumerate(KINDS):
        view = None if kind is None else R.make_view(kind)
        shape = view or R.make_view("grey")
        alpha, inside, weight, seen = _state(NMAX, 10 + k)
        points, inside = _with_points_behind(shape, R.draw_points(shape, NMAX - 64, seed=k), inside[:NMAX - 64], k)
        order = np.random.default_rng(k).permutation(NMAX)
        points, inside = np.ascontiguousarray(points[order]), inside[order]
        ref_w, ref_s = R.view_update(points, alpha, inside, view, weight, seen)
        out[kind] = types.SimpleNamespace(view=view, points=points, alpha=alpha, inside=inside, weight=weight,
                                          seen=seen, ref_w=ref_w, ref_s=ref_s)
    return out


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("kind", KINDS, ids=[k or "no_mask" for k in KINDS])
def test_view_update_matches_the_restatement(cases, kind, n):
    c = cases[kind]
    w, s = _dev(c.weight[:n]), _dev(c.seen[:n])
    rc = _view_update(n, _dev(c.points[:n]), _dev(c.alpha[:n]), _dev(c.inside[:n]), c.view, w, s)
    assert rc == GSR_OK
    assert np.array_equal(_bits(w), c.ref_w[:n].view(np.uint32)) and np.array_equal(_bits(s), c.ref_s[:n])
    changed = (c.ref_w[:n] != c.weight[:n]).sum(), (c.ref_s[:n] != c.seen[:n]).sum()
    if kind == "one_dark":  # the 1x1 plane below the bar: no point is on the mask
        assert changed == (0, 0)
    elif n >= 257:  # the case decides something: the state changed, and not everywhere
        assert 0 < changed[0] < n and 0 < changed[1] < n


def test_second_call_continues_the_running_minimum(cases):
    """Two views over the same buffers, the second on a stream of its own: the minimum runs on, `seen` only grows."""
    a, b = cases["binary"], cases["grey"]
    pts = _dev(a.points)
    w, s = torch.ones(NMAX, device=DEV), torch.zeros(NMAX, dtype=torch.uint8, device=DEV)
    assert _view_update(NMAX, pts, _dev(a.alpha), _dev(a.inside), a.view, w, s) == GSR_OK
    w1, s1 = R.view_update(a.points, a.alpha, a.inside, a.view, np.ones(NMAX, np.float32), np.zeros(NMAX, np.uint8))
    assert np.array_equal(_bits(w), w1.view(np.uint32)) and np.array_equal(_bits(s), s1)
    alpha2, inside2 = _dev(b.alpha), _dev(b.inside)
    sdf, valid = torch.empty(NMAX, device=DEV), torch.empty(NMAX, dtype=torch.bool, device=DEV)
    side = torch.cuda.Stream(DEV)
    side.wait_stream(torch.cuda.current_stream(DEV))
    assert _view_update(NMAX, pts, alpha2, inside2, None, w, s, stream=side) == GSR_OK
    assert _finish(NMAX, w, s, sdf, valid, stream=side) == GSR_OK
    side.synchronize()
    w2, s2 = R.view_update(a.points, b.alpha, b.inside, None, w1, s1)
    assert np.array_equal(_bits(w), w2.view(np.uint32)) and np.array_equal(_bits(s), s2)
    assert (w2 <= w1).all() and (w2 < w1).any() and (s2 >= s1).all() and (s2 > s1).any()
    ref_sdf, ref_valid = R.finish(w2, s2)
    assert np.array_equal(_bits(sdf), ref_sdf.view(np.uint32)) and np.array_equal(valid.cpu().numpy(), ref_valid)


@pytest.mark.parametrize("n", SIZES)
def test_finish_matches_the_restatement(cases, n):
    c = cases["odd"]
    ref_sdf, ref_valid = R.finish(c.ref_w[:n], c.ref_s[:n])
    w, s = _dev(c.ref_w[:n]), _dev(c.ref_s[:n])
    sdf, valid = torch.full((n,), 7.0, device=DEV), torch.zeros(n, dtype=torch.bool, device=DEV)
    assert _finish(n, w, s, sdf, valid) == GSR_OK
    assert np.array_equal(_bits(sdf), ref_sdf.view(np.uint32)) and np.array_equal(valid.cpu().numpy(), ref_valid)
    assert np.array_equal(_bits(w), c.ref_w[:n].view(np.uint32)) and np.array_equal(_bits(s), c.ref_s[:n])
    assert _finish(n, w, s, w, s) == GSR_OK  # in place, as the driver calls it
    assert np.array_equal(_bits(w), ref_sdf.view(np.uint32)) and np.array_equal(_bits(s), ref_valid.view(np.uint8))


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["float32", "float64"])
@pytest.mark.parametrize("E,stream", [(E, False) for E in SIZES] + [(65, True), (NMAX, True)])
def test_bisect_step_matches_the_restatement(E, dtype, stream):
    import gsr_mesh as M

    host = bisect_inputs(E, dtype, seed=E)
    ref = R.bisect_step(*host)
    left, right, lsdf, rsdf, msdf = (_dev(a) for a in host)
    mid = torch.full((E, 3), 9.0, dtype=left.dtype, device=DEV)
    side = torch.cuda.Stream(DEV) if stream else torch.cuda.current_stream(DEV)
    side.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(side):
        M.bisect_step(left, right, lsdf, rsdf, msdf, mid)
    side.synchronize()
    for got, want in zip((left, right, lsdf, rsdf, mid), ref):
        assert np.array_equal(_bits(got).reshape(-1), np.ascontiguousarray(want).view(_bits(got).dtype).reshape(-1))
    assert np.array_equal(_bits(msdf), host[4].view(np.uint32))
    if E >= 257:
        assert ((host[4] == 0) & (host[2] != 0)).any() and ((host[2] == 0) & (host[4] != 0)).any()


def test_argument_errors_leave_the_buffers_untouched(cases):
    abi = _abi()
    lib = abi.load()
    c, n = cases["binary"], 257
    pts, alpha, inside = _dev(c.points[:n]), _dev(c.alpha[:n]), _dev(c.inside[:n])
    w, s = _dev(c.weight[:n]), _dev(c.seen[:n])

    def untouched():
        torch.cuda.synchronize()
        return np.array_equal(_bits(w), c.weight[:n].view(np.uint32)) and np.array_equal(_bits(s), c.seen[:n])

    assert _view_update(-1, pts, alpha, inside, c.view, w, s) == GSR_ERR_ARGS and untouched()
    assert b"field_view_update" in lib.gsr_last_error()
    for missing in range(4):  # alpha, inside, weight, seen
        args = [alpha, inside, w, s]
        args[missing] = None
        assert _view_update(n, pts, args[0], args[1], None, args[2], args[3]) == GSR_ERR_ARGS and untouched()
    assert _view_update(n, None, alpha, inside, c.view, w, s) == GSR_ERR_ARGS and untouched()  # a mask needs points
    for bad in (dict(W=0), dict(H=0), dict(W=-3)):
        assert _view_update(n, pts, alpha, inside, dict(c.view, **bad), w, s) == GSR_ERR_ARGS and untouched()
    assert _view_update(n, None, alpha, inside, None, w, s) == GSR_OK  # no mask: points are not needed
    w.copy_(_dev(c.weight[:n])), s.copy_(_dev(c.seen[:n]))

    sdf, valid = torch.full((n,), 7.0, device=DEV), torch.zeros(n, dtype=torch.uint8, device=DEV)
    assert _finish(-1, w, s, sdf, valid) == GSR_ERR_ARGS
    for missing in range(4):
        args = [w, s, sdf, valid]
        args[missing] = None
        assert _finish(n, *args) == GSR_ERR_ARGS
    assert untouched() and bool((sdf == 7.0).all()) and not bool(valid.any())

    host = bisect_inputs(n, np.float32)
    bufs = [_dev(a) for a in host] + [torch.full((n, 3), 9.0, device=DEV)]

    def step(E, t):
        left, right, lsdf, rsdf, msdf, mid = (abi.ptr(x) if x is not None else None for x in t)
        with torch.cuda.device(DEV):
            return lib.gsr_field_bisect_step(E, left, right, 0, lsdf, rsdf, msdf, mid, _stream(None))

    assert step(-1, bufs) == GSR_ERR_ARGS
    for missing in range(6):
        assert step(n, [None if k == missing else b for k, b in enumerate(bufs)]) == GSR_ERR_ARGS
    torch.cuda.synchronize()
    for b, h in zip(bufs[:5], host):
        assert np.array_equal(_bits(b), h.view(np.uint32))
    assert bool((bufs[5] == 9.0).all())
    assert step(0, [None] * 6) == GSR_OK and step(n, bufs) == GSR_OK  # the library is fine afterwards


# ---- the drivers ------------------------------------------------------------------------------------------------
W, H = 64, 48


class _Pipe:
    debug = False
    compute_cov3D_python = False


class _Model:
    def __init__(self, inp):
        self.get_xyz = inp["means3D"]
        self.get_opacity_with_3D_filter = inp["opacities"]
        self.get_scaling_with_3D_filter = inp["scales"]
        self.get_rotation = inp["rotations"]
        self.active_sh_degree = 3
        self.active_sg_degree = 0


def _view(cam, mask):
    cam = cam.to(DEV)
    wvt = cam.world_view_transform
    return types.SimpleNamespace(**{k: getattr(cam, k) for k in cam.__dataclass_fields__}, R=wvt[:3, :3], T=wvt[3, :3],
                                 Fx=W / (2 * math.tan(cam.FoVx / 2)), Fy=H / (2 * math.tan(cam.FoVy / 2)),
                                 Cx=(W - 1) / 2, Cy=(H - 1) / 2, gt_mask=mask)


def _views(case):
    """Three 64x48 orbit views.  "one_mask" / "chunked": the middle one carries a disc mask; "blind_view": the
    last one, mask included, looks away from the scene and sees no point."""
    yy, xx = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
    disc = (((xx - W / 2) ** 2 + (yy - H / 2) ** 2) < (0.45 * H) ** 2).float()[None].to(DEV)
    cams = S.orbit_cameras(3, W, H)
    if case == "blind_view":
        cams[2] = S.make_camera(W, H, R=np.diag([-1.0, 1.0, -1.0]))
    masked = {"no_masks": (), "one_mask": (1,), "chunked": (1,), "blind_view": (1, 2)}[case]
    return [_view(cam, disc if i in masked else None) for i, cam in enumerate(cams)]


@pytest.fixture(scope="module")
def scene():
    g = group("scene")
    inp = S.activated_inputs(S.make_gaussians(**SCENE_KW))
    pc = _Model({k: v.detach().contiguous().to(DEV) for k, v in inp.items()})
    return types.SimpleNamespace(pc=pc, pts=torch.from_numpy(g["pts"]).to(DEV), host_pts=g["pts"],
                                 scale=torch.from_numpy(g["scale"]).to(DEV), cells=g["tets"].to(DEV))


def _assert_margin(views, pts):
    """The margin rule for the scene's tetra points, in float64: were a point to fall inside it, the mask's edge
    would have to move, not the point to leave the comparison."""
    for v in views:
        if v.gt_mask is not None:
            d = dict(R=v.R.cpu().numpy(), T=v.T.cpu().numpy(), Fx=v.Fx, Fy=v.Fy, Cx=v.Cx, Cy=v.Cy, W=W, H=H,
                     mask=v.gt_mask[0].cpu().numpy())
            front = (pts.astype(np.float64) @ d["R"].astype(np.float64) + d["T"])[:, 2] > 0  # (behind: never inside)
            assert np.abs(R.mask_sample(pts[front], d, np.float64) - 0.5).min(initial=1.0) > R.MARGIN


@pytest.mark.parametrize("case", ["no_masks", "one_mask", "blind_view", "chunked"])
def test_alpha_cull_sdf_hip_equals_the_default(scene, case, monkeypatch):
    import gsr_mesh as M

    views = _views(case)
    _assert_margin(views, scene.host_pts)
    kw = dict(chunk=700) if case == "chunked" else {}
    calls = []
    real = M.call
    monkeypatch.setattr(M, "call", lambda dev, name, *a: (calls.append(name), real(dev, name, *a))[1])
    want = M.alpha_cull_sdf(scene.pts, views, scene.pc, _Pipe(), 0.0, **kw)
    assert calls == []  # the default stays the torch formulation
    got = M.alpha_cull_sdf(scene.pts, views, scene.pc, _Pipe(), 0.0, sweep="hip", **kw)
    n = scene.pts.shape[0]
    chunks = len(torch.chunk(scene.pts, n // 700 + 1)) if case == "chunked" else 1
    assert calls.count("gsr_field_view_update") == 3 * chunks and calls.count("gsr_field_finish") == chunks
    assert got[0].dtype == torch.float32 and got[1].dtype == torch.bool and got[0].shape == (n,)
    assert torch.equal(got[0].view(torch.int32), want[0].view(torch.int32)) and torch.equal(got[1], want[1])
    assert 0.3 < float(got[1].float().mean()) and bool((got[0][~got[1]] == 0.5).all())
    if case == "chunked":
        assert chunks == 3
    if case == "blind_view":
        blind = M.alpha_cull_sdf(scene.pts, views[2:], scene.pc, _Pipe(), 0.0, sweep="hip")
        assert not bool(blind[1].any()) and bool((blind[0] == 0.5).all())
    if case == "one_mask":
        bare = M.alpha_cull_sdf(scene.pts, _views("no_masks"), scene.pc, _Pipe(), 0.0, sweep="hip")
        assert not torch.equal(bare[0], got[0])  # the mask removes a view from some points


@pytest.mark.parametrize("steps,keep", [(10, None), (4, 1), (0, None)], ids=["ten_steps", "cluster_to_keep", "no_steps"])
def test_extract_mesh_hip_equals_the_default(scene, steps, keep, monkeypatch):
    import gsr_mesh as M

    views = _views("one_mask")
    args = (scene.pts, scene.scale, scene.cells, views, scene.pc, _Pipe(), 0.0)
    want = M.extract_mesh(*args, n_binary_steps=steps, cluster_to_keep=keep)
    calls = []
    real = M.call
    monkeypatch.setattr(M, "call", lambda dev, name, *a: (calls.append(name), real(dev, name, *a))[1])
    got = M.extract_mesh(*args, n_binary_steps=steps, cluster_to_keep=keep, sweep="hip")
    assert calls.count("gsr_field_bisect_step") == steps and calls.count("gsr_field_view_update") == 3 * (steps + 1)
    assert got[0].dtype == torch.float32 and got[1].dtype == torch.int64 and (keep is not None or got[1].shape[0] > 0)
    assert torch.equal(got[0].view(torch.int32), want[0].view(torch.int32)) and torch.equal(got[1], want[1])
