"""CPU tests of the extraction sweep's restatement (no GPU needed).

tests/fieldsweep_ref.py restates the three kernels of csrc/fieldsweep.hip in
numpy float32, in the kernels' operation order; tests/test_gpu_fieldsweep.py
holds the kernels to it bit for bit.  Here the restatement is pinned to the
reference's own lines (mesh_extract_tetrahedra.py:44-61, 76-84, 155-163)
evaluated with torch's CPU ops — `points @ R + T`, `addcmul`,
`F.grid_sample(..., align_corners=True)`, `torch.min` / `where`, indexed
assignment: `seen`, `weight` and every bisection output must be equal.

torch's CPU `grid_sample` forms its weights differently from the kernel (1 -
(x - floor x) against (floor x + 1) - x) and `@` may fuse, so the sampled
values differ in their last bits, and `> 0.5` is discontinuous.  The inputs
are constrained, not the tolerance: every tested point's float64 sample lies
more than 1e-3 from 0.5 (fieldsweep_ref.draw_points drops and redraws the
others, fewer than 5% of the draws); masks are at most 64 px wide, so an ulp
of uv moves the sample by about 1e-5.  No point is left out of a comparison.
"""
from __future__ import annotations

import types

import numpy as np
import pytest
import torch

import fieldsweep_ref as R

N = 4000


def _torch_view(view):
    return types.SimpleNamespace(R=torch.from_numpy(view["R"]), T=torch.from_numpy(view["T"]), Fx=view["Fx"],
                                 Fy=view["Fy"], Cx=view["Cx"], Cy=view["Cy"], image_width=view["W"],
                                 image_height=view["H"], gt_mask=torch.from_numpy(view["mask"])[None])


def _reference_update(view, points, alpha, inside, weight, seen):
    """mesh_extract_tetrahedra.py:76-82 with :44-61 as gsr_mesh._view_mask transcribes it, on the CPU."""
    import gsr_mesh as M

    ns = types.SimpleNamespace(gt_mask=None) if view is None else _torch_view(view)
    ok = M._view_mask(ns, torch.from_numpy(points), torch.from_numpy(inside))
    seen = torch.logical_or(torch.from_numpy(seen).bool(), ok)
    weight = torch.from_numpy(weight)
    weight = torch.where(ok, torch.min(torch.from_numpy(alpha), weight), weight)
    return weight.numpy(), seen.numpy().astype(np.uint8)


def _state(n, seed):
    """alpha, inside, and a running state as earlier views leave it: weights in [0, 1] with untouched ones."""
    rng = np.random.default_rng([seed, 5])
    alpha = rng.random(n).astype(np.float32)
    alpha[rng.random(n) < 0.05] = 0.0
    weight = np.where(rng.random(n) < 0.3, 1.0, rng.random(n)).astype(np.float32)
    weight[::8] = alpha[::8]  # ties
    return alpha, rng.random(n) < 0.8, weight, (rng.random(n) < 0.4).astype(np.uint8)


def _with_points_behind(view, points, inside, seed):
    """Appends points at and behind the camera plane with `inside` clear (`integrate` never sets it there): the
    kernel must not evaluate them, whatever their division gives."""
    rng = np.random.default_rng([seed, 9])
    k = 64
    cam = np.concatenate([rng.uniform(-2, 2, (k, 2)), -rng.uniform(0.0, 3.0, (k, 1))], 1)
    cam[:8, 2] = 0.0
    back = ((cam - view["T"].astype(np.float64)) @ np.linalg.inv(view["R"].astype(np.float64))).astype(np.float32)
    return np.concatenate([points, back]), np.concatenate([inside, np.zeros(k, bool)])


@pytest.mark.parametrize("kind", R.KINDS)
def test_view_update_equals_the_reference_lines(kind):
    view = R.make_view(kind)
    points = R.draw_points(view, N)
    alpha, inside, weight, seen = _state(N + 64, 1)
    points, inside = _with_points_behind(view, points, inside[:N], 1)
    got_w, got_s = R.view_update(points, alpha, inside, view, weight, seen)
    ref_w, ref_s = _reference_update(view, points, alpha, inside, weight, seen)
    assert got_w.dtype == np.float32 and got_s.dtype == np.uint8
    assert np.array_equal(got_s, ref_s) and np.array_equal(got_w.view(np.uint32), ref_w.view(np.uint32))
    # the case is not trivial: the mask test decides, both ways, among the points inside
    sample = R.mask_sample(points[inside], view)
    on = sample > 0.5
    if kind not in ("one", "one_dark"):
        assert 0.1 < on.mean() < 0.9
        # zeros padding: samples in the one-texel band outside a border take part, some on, some off
        c, s = R.view_constants(view)
        cam = points[inside].astype(np.float64) @ view["R"].astype(np.float64) + view["T"].astype(np.float64)
        g = c + s * (cam[:, :2] / cam[:, 2:])
        outside = (np.abs(g) > 1).any(1)
        assert outside.sum() > N // 10 and (sample[outside] > 0).sum() > N // 40
        if kind in ("binary", "corners"):
            assert on[outside].any() and not on[outside].all()
    else:  # a 1x1 plane samples its one texel wherever the point projects
        assert np.all(sample == view["mask"][0, 0]) and on.all() == (kind == "one")


def test_view_update_without_a_mask_and_twice():
    view = R.make_view("grey")
    points = R.draw_points(view, N)
    alpha, inside, weight, seen = _state(N, 2)
    w1, s1 = R.view_update(points, alpha, inside, None, weight, seen)
    r1 = _reference_update(None, points, alpha, inside, weight, seen)
    assert np.array_equal(s1, r1[1]) and np.array_equal(w1, r1[0])
    assert np.array_equal(s1, seen | inside) and np.array_equal(w1, np.where(inside, np.minimum(alpha, weight), weight))
    alpha2, inside2, _, _ = _state(N, 3)
    w2, s2 = R.view_update(points, alpha2, inside2, view, w1, s1)
    r2 = _reference_update(view, points, alpha2, inside2, r1[0], r1[1])
    assert np.array_equal(s2, r2[1]) and np.array_equal(w2, r2[0])
    assert (w2 <= w1).all() and (s2 >= s1).all() and (w2 < w1).any()
    sdf, valid = R.finish(w2, s2)
    wt = torch.from_numpy(w2.copy())
    wt[torch.logical_not(torch.from_numpy(s2).bool())] = 0
    assert np.array_equal(sdf, (0.5 - wt).numpy()) and np.array_equal(valid, s2.astype(bool))
    assert sdf.dtype == np.float32 and valid.dtype == bool and (sdf[~valid] == 0.5).all()


def test_corner_texels_are_sampled_exactly():
    """uv = +-1 lands on the centre of a corner texel: its value with weight exactly 1, the neighbours outside
    the plane adding nothing."""
    view = R.make_view("corners")
    assert np.array_equal(R.view_constants(view)[0], [0, 0]) and np.array_equal(R.view_constants(view)[1], [1, 1])
    m, pts, want = view["mask"], [], []
    for z in (0.75, 1.0, 2.0, 3.0):
        for sx, col in ((-1, 0), (1, 7)):
            for sy, row in ((-1, 0), (1, 5)):
                pts.append([sx * z, sy * z, z])
                want.append(m[row, col])
    pts, want = np.array(pts, np.float32), np.array(want, np.float32)
    assert np.abs(want.astype(np.float64) - 0.5).min() > R.MARGIN
    assert np.array_equal(R.mask_sample(pts, view), want)
    n = len(pts)
    ones, zeros = np.ones(n, np.float32), np.zeros(n, np.uint8)
    got = R.view_update(pts, 0.25 * ones, np.ones(n, bool), view, ones, zeros)
    ref = _reference_update(view, pts, 0.25 * ones, np.ones(n, bool), ones, zeros)
    assert np.array_equal(got[1], (want > 0.5).astype(np.uint8)) and np.array_equal(got[1], ref[1])
    assert np.array_equal(got[0], ref[0]) and np.array_equal(got[0], np.where(want > 0.5, 0.25, 1.0))


def _reference_bisect(left_points, right_points, left_sdf, right_sdf, mid_sdf):
    """mesh_extract_tetrahedra.py:155-163: the reference's indexed assignments, [E,1] sdf columns."""
    left_points, right_points, left_sdf, right_sdf, mid_sdf = (
        torch.from_numpy(a.copy()) for a in (left_points, right_points, left_sdf, right_sdf, mid_sdf))
    mid_points = (left_points + right_points) * 0.5
    ind_low = ((mid_sdf < 0) & (left_sdf < 0)) | ((mid_sdf > 0) & (left_sdf > 0))
    left_sdf[ind_low] = mid_sdf[ind_low]
    right_sdf[~ind_low] = mid_sdf[~ind_low]
    left_points[ind_low.flatten()] = mid_points[ind_low.flatten()]
    right_points[~ind_low.flatten()] = mid_points[~ind_low.flatten()]
    points = (left_points + right_points) * 0.5
    return [t.numpy() for t in (left_points, right_points, left_sdf, right_sdf, points)]


def bisect_inputs(E, dtype, seed=0):
    """Edges with every sign pattern: left_sdf and mid_sdf negative, positive and exactly 0 (a tenth each)."""
    rng = np.random.default_rng([seed, 3])
    left, right = rng.standard_normal((E, 3)).astype(dtype), rng.standard_normal((E, 3)).astype(dtype)
    sdfs = []
    for k in range(3):
        s = (rng.random((E, 1)) - 0.5).astype(np.float32)
        s[rng.random(E) < 0.1] = 0.0
        sdfs.append(s)
    return (left, right, *sdfs)


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["float32", "float64"])
def test_bisect_step_equals_the_reference_lines(dtype):
    left, right, lsdf, rsdf, msdf = bisect_inputs(2000, dtype)
    assert ((msdf == 0) & (lsdf != 0)).sum() > 50 and ((lsdf == 0) & (msdf != 0)).sum() > 50
    assert ((lsdf == 0) & (msdf == 0)).sum() > 5
    for step in range(3):
        got = R.bisect_step(left, right, lsdf, rsdf, msdf)
        ref = _reference_bisect(left, right, lsdf, rsdf, msdf)
        for g, r in zip(got, ref):
            assert g.dtype == r.dtype and np.array_equal(g.reshape(r.shape), r)
        # a midpoint with sdf exactly 0 replaced the right end, whatever the left end's sign
        zero = (msdf == 0).reshape(-1)
        assert np.array_equal(got[0][zero], left[zero]) and (got[3][zero] == 0).all()
        left, right, lsdf, rsdf = got[0], got[1], got[2].reshape(-1, 1), got[3].reshape(-1, 1)
        msdf = np.where(np.arange(len(msdf))[:, None] % 3 == step, -msdf, msdf * 0.5).astype(np.float32)


def test_the_margin_rule_is_checked_at_generation():
    """draw_points keeps its promise, and a margin that would hide the border cases trips its own assertion."""
    view = R.make_view("binary")
    p = R.draw_points(view, 2000, seed=4)
    assert np.abs(R.mask_sample(p, view, np.float64) - 0.5).min() > R.MARGIN
    assert np.abs(R.mask_sample(p, view).astype(np.float64) - R.mask_sample(p, view, np.float64)).max() < 1e-4
    old, R.MARGIN = R.MARGIN, 0.2
    try:
        with pytest.raises(AssertionError):
            R.draw_points(R.make_view("grey"), 2000)
    finally:
        R.MARGIN = old


def test_sweep_keyword_and_cpu_tensors():
    """The module's rules hold for the new keyword: CPU tensors raise, there is no fallback, and only the two
    sweeps exist."""
    import gsr_mesh as M

    pts = torch.zeros(4, 3)
    for sweep in ("torch", "hip"):
        with pytest.raises(RuntimeError, match="HIP device tensor"):
            M.alpha_cull_sdf(pts, [], None, None, 0.0, sweep=sweep)
    with pytest.raises(RuntimeError, match="HIP device tensor"):
        M.extract_mesh(pts, torch.zeros(4, 1), torch.zeros(1, 4, dtype=torch.int64), [], None, None, 0.0, sweep="hip")
    with pytest.raises(ValueError, match="sweep"):
        M.alpha_cull_sdf(pts, [], None, None, 0.0, sweep="eager")
    with pytest.raises(ValueError, match="sweep"):
        M.extract_mesh(pts, torch.zeros(4, 1), torch.zeros(1, 4, dtype=torch.int64), [], None, None, 0.0, sweep=None)
    with pytest.raises(RuntimeError, match="HIP device tensor"):
        M.bisect_step(pts, pts.clone(), torch.zeros(4), torch.zeros(4), torch.zeros(4), pts.clone())


def test_abi_lists_the_sweep_entries():
    from diff_gaussian_rasterization import _abi

    for name, nargs in (("gsr_field_view_update", 16), ("gsr_field_finish", 6), ("gsr_field_bisect_step", 9)):
        assert len(_abi.SIGNATURES[name][1]) == nargs
