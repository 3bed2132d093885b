"""GPU tests of TSDF fusion and marching cubes in HIP (csrc/tsdf.hip through
gsr_tsdf and gsr_mesh.extract_mesh_tsdf).

Yardstick: tests/tsdf_ref.py, the numpy restatement of DESIGN §6h, which
tests/test_tsdf.py pins to answers known by construction.  open3d is not
involved anywhere.  Touch and integrate decide by float32 roundings (a floor,
a round to the nearest pixel, three comparisons); the restatement reports how
close each decision came to flipping, the comparisons leave out what lies
under a stated margin, and the share left out is bounded on the restatement
alone.  Extraction gets identical float32 inputs through from_arrays, so its
faces are compared exactly and its positions within 2^-21 relative.
"""
from __future__ import annotations

import json
import os
import types

import numpy as np
import pytest
import torch

import gsr_scene as S
import tsdf_ref as T
from test_tsdf import (IDENT, R8, VS, all_cases_field, single_pixel_case, sphere_case, sphere_field, torus_case,
                       translated, wall_case)

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _grid(R=R8, with_color=True, vs=VS):
    from gsr_tsdf import VoxelBlockGrid

    return VoxelBlockGrid(vs, R, with_color=with_color, device=DEV, block_count=2)


def _dev(a, dtype=torch.float32):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype).to(DEV)


def _touch(depth, k, e, R=R8, vs=VS, **kw):
    return _grid(R, vs=vs).compute_unique_block_coordinates(_dev(depth), k, e, **kw).cpu().numpy()


def _from_arrays(blocks, tsdf, weight, color=None, R=R8, vs=VS):
    from gsr_tsdf import VoxelBlockGrid

    return VoxelBlockGrid.from_arrays(_dev(blocks, torch.int32), _dev(tsdf), _dev(weight),
                                      None if color is None else _dev(color), voxel_size=vs, block_resolution=R)


def _record(name, **values):
    """One JSON line per case to the file $GSR_TSDF_MARGIN_LOG names, when it is set;
    profiles/tsdf_parity_margins.jsonl is a committed copy of one run."""
    path = os.environ.get("GSR_TSDF_MARGIN_LOG")
    if not path:
        return
    try:
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, "a") as fh:
            fh.write(json.dumps({"case": name, **values}) + "\n")
    except OSError:
        pass


def look_at(eye, target):
    """World -> camera of a camera at `eye` looking at `target` (+z forward, y down-ish)."""
    eye, target = np.asarray(eye, float), np.asarray(target, float)
    z = (target - eye) / np.linalg.norm(target - eye)
    x = np.cross([0.0, 1.0, 0.0] if abs(z[1]) < 0.9 else [1.0, 0.0, 0.0], z)
    x /= np.linalg.norm(x)
    y = np.cross(z, x)
    e = np.eye(4)
    e[:3, :3] = np.stack([x, y, z])
    e[:3, 3] = -e[:3, :3] @ eye
    return e


def sphere_depth(H, W, k, e, centre, radius):
    """The z-depth of the first intersection of every pixel's ray with a sphere, 0 where it misses."""
    fx, fy, cx, cy = k
    ys, xs = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    d = np.stack([(xs - cx) / fx, (ys - cy) / fy, np.ones_like(xs, float)], -1)
    c = e[:3, :3] @ np.asarray(centre) + e[:3, 3]
    a, b, q = (d * d).sum(-1), -2 * (d @ c), c @ c - radius ** 2
    disc = b * b - 4 * a * q
    t = np.where(disc > 0, (-b - np.sqrt(np.maximum(disc, 0))) / (2 * a), 0.0)
    return np.where(t > 0, t, 0.0).astype(np.float32)


# ---- touch -----------------------------------------------------------------------------------------

def test_touch_single_pixel_and_floor():
    depth, k = single_pixel_case()
    got = _touch(depth, k, IDENT)
    assert got.dtype == np.int32 and got.tolist() == [[0, 0, 11], [0, 0, 12], [0, 0, 13]]
    # samples at negative coordinates: floor, not truncation
    assert _touch(depth, k, translated(-0.001, -0.001, 0.0)).tolist() == [[-1, -1, 11], [-1, -1, 12], [-1, -1, 13]]


def test_touch_rejects_pixels():
    depth, k = single_pixel_case()
    for bad in (0.0, -1.0, 8.0, 9.0, float("nan"), float("inf")):
        d = np.zeros_like(depth)
        d[8, 4] = bad
        assert _touch(d, k, IDENT).shape == (0, 3)
    d = np.zeros_like(depth)  # valid depth only off the stride-4 lattice
    d[8, 5] = d[9, 4] = d[7, 7] = d[3, 3] = 1.0
    assert _touch(d, k, IDENT).shape == (0, 3)


def test_touch_clamps():
    depth, k = single_pixel_case()
    assert _touch(depth * 0.03, k, translated(0, 0, 0.004)).tolist() == [[0, 0, 0], [0, 0, 1]]
    assert _touch(depth * 7.98, k, translated(0, 0, -0.004))[:, 2].tolist() == [98, 99]
    assert _touch(depth * 7.98, k, translated(0, 0, 0.004))[:, 2].tolist() == [98, 99, 100]


@pytest.mark.parametrize("H,W", [(1, 9), (7, 10), (13, 5)])
def test_touch_odd_sizes(H, W):
    rng = np.random.default_rng(H * 100 + W)
    depth = rng.uniform(0.3, 0.6, (H, W)).astype(np.float32)
    k, e = (40.0, 40.0, (W - 1) / 2, (H - 1) / 2), translated(0.0113, -0.0071, 0.0037)
    ref = T.touch(depth, k, e, VS, R8)
    assert ref["pixels"].shape[0] == ((H + 3) // 4) * ((W + 3) // 4)
    assert ref["margin"].min() > 1e-4
    assert np.array_equal(_touch(depth, k, e), ref["coords"])


def test_touch_wall_one_block_and_order():
    # a wall whose samples all land in one block: z in [0.41, 0.47] of block 5, x and y in [0.002, 0.021] of block 0
    depth = np.full((8, 8), 0.44, np.float32)
    k = (100.0, 100.0, 0.0, 0.0)
    got = _touch(depth, k, translated(0.002, 0.002, 0.0), trunc_voxel_multiplier=3.0)
    assert got.tolist() == [[0, 0, 5]]
    depth, k = wall_case()
    got = _touch(depth, k, IDENT)
    keys = T.pack_keys(got)
    assert np.all(np.diff(keys) > 0)  # ascending and unique
    assert np.array_equal(got, T.touch(depth, k, IDENT, VS, R8)["coords"])


def test_touch_out_of_range_is_an_error():
    depth, k = single_pixel_case()
    with pytest.raises(RuntimeError, match="2\\^20"):
        _touch(depth * 7.0, k, IDENT, vs=1e-7)  # 7 / (8e-7) = 8.75e6 blocks along z
    with pytest.raises(RuntimeError, match="2\\^20"):
        _touch(depth, k, translated(0.0, -2000.0, 0.0), vs=1e-4)


def test_touch_random_view():
    rng = np.random.default_rng(11)
    H, W = 48, 64
    k = (70.0, 70.0, 31.5, 23.5)
    e = look_at((0.31, -0.22, -0.4), (0.02, 0.01, 0.3))
    depth = (0.75 + 0.1 * rng.standard_normal((H, W))).astype(np.float32)
    depth[rng.random((H, W)) < 0.1] = 0
    ref = T.touch(depth, k, e, VS, R8)
    margin, blocks = ref["margin"].reshape(-1), T.pack_keys(ref["blocks"].reshape(-1, 3))
    sure = margin > 1e-4
    assert (~sure).sum() <= 0.01 * sure.size  # on the restatement alone
    got = set(T.pack_keys(_touch(depth, k, e)).tolist())
    # a block is certain when a sample lands in it with margin
    assert len(set(blocks[sure].tolist())) > 20
    assert set(blocks[sure].tolist()) <= got, "a block every sample reaches with margin is missing"
    # the unsure samples may land in a neighbouring block: allow the 26 neighbours of their block
    near = set(blocks.tolist())
    for b in ref["blocks"].reshape(-1, 3)[~sure]:
        for dx in (-1, 0, 1):
            for dy in (-1, 0, 1):
                for dz in (-1, 0, 1):
                    near.add(int(T.pack_keys(b + np.array([dx, dy, dz]))[0]))
    assert got <= near, "a block appears that no sample reaches within the margin"


# ---- integrate -------------------------------------------------------------------------------------

def _voxels(R=R8):
    i = np.arange(R ** 3)
    return i % R, i // R % R, i // (R * R)


def test_integrate_wall_one_block():
    depth, k = wall_case()
    g = _grid()
    color = np.full((24, 32, 3), 0.25, np.float32)
    blk = _dev([[0, 0, 2]], torch.int32)
    g.integrate(blk, _dev(depth), _dev(color), k, IDENT)
    x, y, z = _voxels()
    wz = (2 * R8 + z) * VS  # 0.16 .. 0.23
    u, v = np.rint(100 * x * VS / wz + 15.5), np.rint(100 * y * VS / wz + 11.5)
    seen = (u < 32) & (v < 24)
    w, t, c = g.weight[0].cpu().numpy(), g.tsdf[0].cpu().numpy(), g.color[0].cpu().numpy()
    assert np.array_equal(w, seen.astype(np.float32))
    assert np.allclose(t[seen], (np.minimum(0.2 - wz, 0.08) / 0.08)[seen], atol=2e-6)
    assert np.all(t[~seen] == 0) and np.all(c[~seen] == 0) and np.allclose(c[seen], 0.25, atol=1e-7)
    # beyond -trunc behind the wall: block z = 3 holds z = 0.24 .. 0.31, untouched from 0.29 on
    g.integrate(_dev([[0, 0, 3]], torch.int32), _dev(depth), _dev(color), k, IDENT)
    wz3 = (3 * R8 + z) * VS
    w3 = g.weight[1].cpu().numpy()
    assert np.all(w3[wz3 > 0.2805] == 0) and np.all(w3[(wz3 < 0.2795) & (x == 0) & (y == 0)] == 1)
    # the same view twice, then views at other depths: the running mean in call order
    g.integrate(blk, _dev(depth), _dev(color), k, IDENT)
    assert np.array_equal(g.weight[0].cpu().numpy(), 2 * seen.astype(np.float32))
    assert np.allclose(g.tsdf[0].cpu().numpy(), t, atol=1e-7)
    g.integrate(blk, _dev(depth * 1.1), _dev(color * 2), k, IDENT)
    g.integrate(blk, _dev(depth * 0.9), _dev(color * 3), k, IDENT)
    lin = (2 * R8 + 1) * R8 + 1  # voxel (1, 1, 2): z = 0.18
    assert float(g.weight[0][lin]) == 4
    assert abs(float(g.tsdf[0][lin]) - (0.02 + 0.02 + 0.04 + 0.0) / 0.08 / 4) < 2e-6
    assert abs(float(g.color[0][lin][0]) - (0.25 + 0.25 + 0.5 + 0.75) / 4) < 1e-6


def test_integrate_untouched_voxels_and_blocks():
    depth, k = wall_case()
    depth = depth.copy()
    depth[:, :16] = 0  # zero depth over the left half: u < 15.5, i.e. x < 0
    g = _grid(with_color=False)
    blocks = _dev([[0, 0, 2], [-1, 0, 2], [0, 0, -1], [9, 0, 2]], torch.int32)
    g.integrate(blocks, _dev(depth), None, k, IDENT)
    assert g.color is None and g.block_coords.cpu().tolist() == [[-1, 0, 2], [0, 0, -1], [0, 0, 2], [9, 0, 2]]
    w = g.weight.cpu().numpy()
    assert np.all(w[0] == 0)  # over zero-depth pixels
    assert np.all(w[1] == 0)  # z_c <= 0
    assert np.all(w[3] == 0)  # projects outside the image
    assert w[2].sum() > 50
    # a block in the grid but not in the list is left alone, even in view
    before = g.tsdf.clone(), g.weight.clone()
    full = np.full((24, 32), 0.2, np.float32)
    g.integrate(_dev([[0, 0, 2]], torch.int32), _dev(full), None, k, IDENT)
    assert torch.equal(g.weight[0], before[1][0]) and torch.equal(g.tsdf[0], before[0][0])
    assert not torch.equal(g.weight[2], before[1][2])
    with pytest.raises(RuntimeError, match="twice"):
        g.integrate(_dev([[0, 0, 2], [0, 0, 2]], torch.int32), _dev(full), None, k, IDENT)


def test_integrate_growth_keeps_slots():
    depth, k = wall_case()
    g = _grid()  # capacity 2
    color = _dev(np.full((24, 32, 3), 0.5, np.float32))
    first = g.compute_unique_block_coordinates(_dev(depth), k, IDENT)
    g.integrate(first, _dev(depth), color, k, IDENT)
    n = g.num_blocks
    assert n > 2 and torch.equal(g.block_coords, first)
    keep = g.block_keys.clone(), g.tsdf.clone(), g.weight.clone(), g.color.clone()
    e = translated(0.3, 0.0, 0.0)  # a second view elsewhere: only new blocks
    second = g.compute_unique_block_coordinates(_dev(depth), k, e)
    g.integrate(second, _dev(depth), color, k, e)
    assert g.num_blocks == n + second.shape[0]
    assert torch.equal(g.block_keys[:n], keep[0]) and torch.equal(g.tsdf[:n], keep[1])
    assert torch.equal(g.weight[:n], keep[2]) and torch.equal(g.color[:n], keep[3])
    assert torch.equal(g.block_coords[n:], second)  # new blocks in ascending key order
    assert float(g.weight[n:].sum()) > 0


@pytest.mark.parametrize("R", [8, 16])
def test_integrate_random_view(R):
    rng = np.random.default_rng(3)
    H, W = 48, 64
    k = (70.0, 70.0, 31.5, 23.5)
    vs = 0.01 if R == 8 else 0.005
    views = []
    for eye in (((0.31, -0.22, -0.4),) if R == 8 else ((-0.2, 0.1, -0.45),)):
        e = look_at(eye, (0.02, 0.01, 0.3))
        depth = (0.75 + 0.05 * rng.standard_normal((H, W))).astype(np.float32)
        depth[rng.random((H, W)) < 0.1] = 0
        views.append((depth, rng.random((H, W, 3)).astype(np.float32), e))
    g = _grid(R, vs=vs)
    r64, r32 = T.Grid(vs, R, dtype=np.float64), T.Grid(vs, R, dtype=np.float32)
    sure = None
    for depth, color, e in views:
        blocks = T.touch(depth, k, e, vs, R)["coords"]
        out = r64.integrate(blocks, depth, color, k, e)
        r32.integrate(blocks, depth, color, k, e)
        g.integrate(_dev(blocks, torch.int32), _dev(depth), _dev(color), k, e)
        ok = np.ones(r64.tsdf.shape, bool) if sure is None else np.concatenate(
            [sure, np.ones((r64.tsdf.shape[0] - sure.shape[0], R ** 3), bool)])
        ok[out["slots"]] &= out["margin"] > 1e-3
        sure = ok
    assert np.array_equal(g.block_coords.cpu().numpy(), r64.coords)
    updated = r64.weight > 0
    assert updated.sum() > 5000
    assert (updated & ~sure).sum() <= 0.01 * updated.sum()  # on the restatement alone
    # the restatement's own float32 run against its float64 run, where both made the same decisions
    same = sure & (r32.weight == r64.weight)
    dev_t = float(np.abs(r32.tsdf - r64.tsdf)[same].max())
    dev_c = float(np.abs(r32.color - r64.color)[same].max())
    tol_t, tol_c = max(4 * dev_t, 1e-6), max(4 * dev_c, 1e-6)
    w, t, c = g.weight.cpu().numpy(), g.tsdf.cpu().numpy(), g.color.cpu().numpy()
    err_t, err_c = float(np.abs(t - r64.tsdf)[sure].max()), float(np.abs(c - r64.color)[sure].max())
    print(f"R={R}: ref32-ref64 tsdf {dev_t:.3e} colour {dev_c:.3e}; gpu-ref64 tsdf {err_t:.3e} colour {err_c:.3e}")
    _record(f"integrate_random_R{R}", ref32_tsdf=dev_t, ref32_color=dev_c, tol_tsdf=tol_t, tol_color=tol_c,
            gpu_tsdf=err_t, gpu_color=err_c, excluded=int((updated & ~sure).sum()), updated=int(updated.sum()))
    assert np.array_equal(w[sure], r64.weight[sure])
    assert err_t <= tol_t and err_c <= tol_c


# ---- extract ---------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def sphere():
    blocks, tsdf, weight = sphere_case()
    rng = np.random.default_rng(9)
    color = rng.random(tsdf.shape + (3,)).astype(np.float32)
    order = rng.permutation(blocks.shape[0])  # slots in no particular order
    blocks, tsdf, weight, color = blocks[order], tsdf[order], weight[order], color[order]
    return {"in": (blocks, tsdf, weight, color), "ref": T.extract(blocks, tsdf, weight, color, VS, R8)}


def _close(v, rv, vs=VS):
    tol = 2.0 ** -21 * np.maximum(np.abs(rv), vs)
    return bool(np.all(np.abs(v.astype(np.float64) - rv) <= tol))


def test_extract_sphere(sphere):
    blocks, tsdf, weight, color = sphere["in"]
    rv, rf, rc, n_edges = sphere["ref"]
    g = _from_arrays(blocks, tsdf, weight, color)
    v, f, c = g.extract_triangle_mesh()
    v2, f2, c2 = g.extract_triangle_mesh()
    assert torch.equal(v, v2) and torch.equal(f, f2) and torch.equal(c, c2)  # the same bits on every run
    assert v.dtype == torch.float32 and f.dtype == torch.int64 and c.dtype == torch.float32
    v, f, c = v.cpu().numpy(), f.cpu().numpy(), c.cpu().numpy()
    assert np.array_equal(f, rf)  # order included
    assert v.shape[0] == n_edges and np.unique(f).size == v.shape[0]
    assert _close(v, rv)
    assert np.abs(c - rc).max() <= 4e-7  # one interpolation of values in [0, 1]
    assert T.is_closed_oriented(f) and T.euler(f) == 2
    vol, rvol = T.signed_volume(v, f), T.signed_volume(rv, rf)
    assert vol > 0 and abs(vol - rvol) <= 1e-5 * rvol


def test_extract_torus():
    blocks, tsdf, weight = torus_case()
    v, f, c = _from_arrays(blocks, tsdf, weight).extract_triangle_mesh()
    rv, rf, _, _ = T.extract(blocks, tsdf, weight, None, VS, R8)
    assert c is None and np.array_equal(f.cpu().numpy(), rf) and _close(v.cpu().numpy(), rv)
    assert T.is_closed_oriented(rf) and T.euler(f.cpu().numpy()) == 0


def test_extract_all_256_patterns():
    blocks, tsdf, weight = all_cases_field()
    v, f, _ = _from_arrays(blocks, tsdf, weight).extract_triangle_mesh()
    rv, rf, _, n_edges = T.extract(blocks, tsdf, weight, None, VS, R8)
    assert rf.shape[0] == sum(len(r) // 3 for r in T.MC_ROWS)
    assert np.array_equal(f.cpu().numpy(), rf) and v.shape[0] == n_edges and _close(v.cpu().numpy(), rv)


@pytest.mark.parametrize("R", [8, 16])
def test_extract_threshold_missing_block_and_zero(R):
    vs = 0.004
    blocks = np.array([(x, y, z) for x in (-1, 0) for y in (-1, 0) for z in (-1, 0)])
    blocks, tsdf, weight = sphere_field((0.0005, -0.0007, 0.0003), 0.6 * R * vs, blocks, R=R, vs=vs)
    full = T.extract(blocks, tsdf, weight, None, vs, R)
    assert T.is_closed_oriented(full[1])
    # a corner with weight == weight_threshold suppresses its 8 cubes (strictly greater counts): a corner
    # inside block (0, 0, 0) next to a sign change along x
    t = tsdf[7].reshape(R, R, R)  # [z, y, x]
    z, y, x = np.argwhere((t[1:-1, 1:-1, 1:-2] < 0) != (t[1:-1, 1:-1, 2:-1] < 0))[0] + 1
    w = weight.copy()
    w[7, (z * R + y) * R + x] = 3.0
    rv, rf, _, n = T.extract(blocks, tsdf, w, None, vs, R)
    v, f, _ = _from_arrays(blocks, tsdf, w, R=R, vs=vs).extract_triangle_mesh()
    assert np.array_equal(f.cpu().numpy(), rf) and _close(v.cpu().numpy(), rv, vs)
    assert rf.shape[0] < full[1].shape[0] and len(T.boundary_edges(rf)) > 0
    w[7, (z * R + y) * R + x] = np.nextafter(np.float32(3.0), np.float32(4.0))
    assert _from_arrays(blocks, tsdf, w, R=R, vs=vs).extract_triangle_mesh()[1].shape[0] == full[1].shape[0]
    # a missing neighbour block: an open boundary there and nothing across it
    keep = np.arange(8) != 0  # drop block (-1, -1, -1)
    rv, rf, _, _ = T.extract(blocks[keep], tsdf[keep], weight[keep], None, vs, R)
    v, f, _ = _from_arrays(blocks[keep], tsdf[keep], weight[keep], R=R, vs=vs).extract_triangle_mesh()
    f, v = f.cpu().numpy(), v.cpu().numpy()
    assert np.array_equal(f, rf) and _close(v, rv, vs)
    assert len(T.boundary_edges(f)) > 0 and not np.any(np.all(v < -1e-9, axis=1))
    # tsdf == 0 exactly at corners: no NaN, the vertex sits on the corner
    t0 = tsdf.copy()
    lin = np.argmin(np.abs(t0[7]))
    t0[7, lin] = 0.0
    v, f, _ = _from_arrays(blocks, t0, weight, R=R, vs=vs).extract_triangle_mesh()
    rv, rf, _, _ = T.extract(blocks, t0, weight, None, vs, R)
    v = v.cpu().numpy()
    assert np.isfinite(v).all() and np.array_equal(f.cpu().numpy(), rf) and _close(v, rv, vs)
    p0 = np.array([lin % R, lin // R % R, lin // (R * R)]) * np.float32(vs)
    assert np.any(np.all(v == p0.astype(np.float32), axis=1))


def test_extract_nothing():
    blocks, tsdf, weight = sphere_field((0, 0, 0), 10.0, np.array([[0, 0, 0], [1, 0, 0]]))  # all inside
    for out in (_from_arrays(blocks, tsdf, weight).extract_triangle_mesh(), _grid().extract_triangle_mesh(),
                _from_arrays(np.zeros((0, 3)), np.zeros((0, R8 ** 3)), np.zeros((0, R8 ** 3))).extract_triangle_mesh()):
        assert tuple(out[0].shape) == (0, 3) and tuple(out[1].shape) == (0, 3)
        assert out[0].dtype == torch.float32 and out[1].dtype == torch.int64


def test_extract_feeds_the_clean_up(sphere):
    import gsr_mesh as M

    blocks, tsdf, weight, _ = sphere["in"]
    far = np.array([(x, y, 9) for x in (0, 1) for y in (0, 1)])
    b2, t2, w2 = sphere_field((0.08, 0.08, 0.76), 0.025, far)
    g = _from_arrays(np.concatenate([blocks, b2]), np.concatenate([tsdf, t2]), np.concatenate([weight, w2]))
    v, f, _ = g.extract_triangle_mesh()
    labels, counts, _ = M.cluster_connected_triangles(v, f)
    assert counts.numel() == 2 and int(counts.min()) >= 50
    pv, pf = M.post_process_mesh(v, f, cluster_to_keep=1)
    assert pf.shape[0] == sphere["ref"][1].shape[0] and pv.shape[0] == sphere["ref"][0].shape[0]
    assert T.is_closed_oriented(pf.cpu().numpy())


# ---- end to end ------------------------------------------------------------------------------------

def test_fuse_sphere_from_depth_maps():
    import gsr_mesh as M

    # 8 cameras on the corners of a cube around the sphere.  Fusion from depth maps leaves thin
    # artefacts at silhouettes (a voxel behind a thin cap reads as inside), so whether the fused
    # surface closes depends on the case: this one was chosen on the CPU, where the restatement's
    # fusion of the same views has no boundary edge
    centre, radius, vs, R = np.array([0.02, -0.01, 0.03]), 0.06, 0.005, 8
    H, W, k = 48, 64, (100.0, 100.0, 31.5, 23.5)
    g = _grid(R, with_color=False, vs=vs)
    eyes = [0.4 * np.array(d) / np.sqrt(3.0) for d in ((1, 1, 1), (1, 1, -1), (1, -1, 1), (1, -1, -1), (-1, 1, 1),
                                                        (-1, 1, -1), (-1, -1, 1), (-1, -1, -1))]
    for eye in eyes:
        e = look_at(centre + np.array(eye), centre)
        depth = _dev(sphere_depth(H, W, k, e, centre, radius))
        for _ in range(4):  # weight must exceed 3
            g.integrate(g.compute_unique_block_coordinates(depth, k, e), depth, None, k, e)
    v, f, _ = g.extract_triangle_mesh()
    assert f.shape[0] > 500
    d = np.linalg.norm(v.cpu().numpy() - centre, axis=1)
    assert np.abs(d - radius).max() <= 8 * vs + vs  # sdf_trunc + voxel_size
    pv, pf = M.post_process_mesh(v, f, cluster_to_keep=1)
    labels, counts, _ = M.cluster_connected_triangles(pv, pf)
    assert counts.numel() == 1 and T.is_closed_oriented(pf.cpu().numpy())


def test_driver_matches_the_three_stages():
    import gsr_mesh as M
    from gaussian_renderer import render
    from gsr_tsdf import VoxelBlockGrid
    from test_gpu_tetmesh import _Pipe, _views
    from test_tetmesh import SCENE_KW

    W, H = 64, 48
    inp = {k: v.detach().contiguous().to(DEV) for k, v in S.activated_inputs(S.make_gaussians(**SCENE_KW)).items()}
    pc = types.SimpleNamespace(get_xyz=inp["means3D"], get_rotation=inp["rotations"], get_features=inp["shs"],
                               get_scaling_n_opacity_with_3D_filter=(inp["scales"], inp["opacities"]),
                               get_sg_axis=inp["sg_axis"], get_sg_sharpness=inp["sg_sharpness"],
                               get_sg_color=inp["sg_color"], active_sh_degree=3, active_sg_degree=0)
    views = _views(W, H)
    bg = torch.ones(3, device=DEV)
    kw = dict(voxel_size=0.05, block_resolution=8, weight_threshold=0.5)
    v, f, c, (pv, pf) = M.extract_mesh_tsdf(views, pc, _Pipe(), bg, 0.0, cluster_to_keep=1, **kw)
    assert f.shape[0] > 0 and c.shape == v.shape and float(c.min()) >= 0 and float(c.max()) <= 1
    g = VoxelBlockGrid(0.05, 8, device=DEV)
    for view in views:
        pkg = render(view, pc, _Pipe(), bg, 0.0)
        color = pkg["render"].clamp(0, 1).permute(1, 2, 0).contiguous()
        depth = pkg["median_depth"].clone()
        if view.gt_mask is not None:
            depth[view.gt_mask < 0.5] = 0
        intr, extr = M._view_camera(view)
        blocks = g.compute_unique_block_coordinates(depth[0], intr, extr)
        g.integrate(blocks, depth[0], color, intr, extr)
    hv, hf, hc = g.extract_triangle_mesh(0.5)
    assert torch.equal(v, hv) and torch.equal(f, hf) and torch.equal(c, hc)
    qv, qf = M.post_process_mesh(v, f, 1)
    assert torch.equal(pv, qv) and torch.equal(pf, qf)
    # the mask is respected: without it the middle view adds measurements
    bare = [types.SimpleNamespace(**{**vars(x), "gt_mask": None}) for x in views]
    uv, uf, uc = M.extract_mesh_tsdf(bare, pc, _Pipe(), bg, 0.0, **kw)
    assert uv.shape != v.shape or not torch.equal(uv, v)


def test_write_ply_colors(tmp_path):
    import gsr_mesh as M

    v = torch.tensor([[0.0, 0, 0], [1, 0, 0], [0, 1, 0]])
    f = torch.tensor([[0, 1, 2]])
    M.write_ply(tmp_path / "a.ply", v, f)
    M.write_ply(tmp_path / "b.ply", v, f, colors=torch.tensor([[0.0, 0.5, 1.0]] * 3))
    a, b = (tmp_path / "a.ply").read_bytes(), (tmp_path / "b.ply").read_bytes()
    assert b"red" not in a and a.endswith(np.array([3], "u1").tobytes() + np.array([0, 1, 2], "<i4").tobytes())
    assert len(a) == a.index(b"end_header\n") + 11 + 36 + 13
    assert b"property uchar blue\n" in b and len(b) - b.index(b"end_header\n") == 11 + 3 * 15 + 13
