"""CPU tests that pin the numpy restatement of the TnT mesh culling (tests/tntcull_ref.py, the yardstick of
tests/test_gpu_tntcull.py).

depth_ref (float32, the contract's order) against depth_f64 (Moller-Trumbore, float64): equal coverage and
depth within 1e-5 relative at every pixel, except pixels whose centre lies within 1e-3 px of an edge of a
triangle that decides the pixel (the winner of either map); those may be at most 1 % of the image, asserted.
votes_ref against a literal transcription of cull_mesh.py's point_masks on torch's CPU grid_sample: equal
counts, except vertices with |z - (d + eps)| <= 1e-5 z in some view or (u, v) within 1e-4 px of the frustum
border; at most 1 % of the vertices, asserted.
"""
from __future__ import annotations

import numpy as np
import pytest
import torch

import tntcull_ref as R

H, W = 45, 70
K = dict(fx=62.0, fy=61.0, cx=34.6, cy=22.3)


def _scenes():
    sv, sf = R.icosphere(3)
    tv, tf = R.terrain(24, 24)
    plane_v = np.array([[-9, 0.4, -9], [9, 0.4, -9], [9, 0.4, 9], [-9, 0.4, 9]], np.float32)  # through z = 0
    plane_f = np.array([[0, 1, 2], [0, 2, 3]])
    return {
        "sphere_outside": (sv, sf, np.linalg.inv(R.look_at((0.3, -0.4, -3.0), (0, 0, 0)))),
        "sphere_centre": (sv, sf, np.linalg.inv(R.look_at((0.0, 0.0, 0.0), (0.3, 0.2, 1.0)))),
        "terrain": (tv, tf, np.linalg.inv(R.look_at((2.5, -1.5, 2.0), (0, 0, 0)))),
        "floor_through_camera_plane": (plane_v, plane_f, np.linalg.inv(R.look_at((0, 0, 0), (0, 0.2, 1.0)))),
    }


@pytest.mark.parametrize("name", list(_scenes()))
def test_depth_ref_matches_float64_ray_cast(name):
    v, f, w2c = _scenes()[name]
    d32, w32 = R.depth_ref(v, f, w2c, H, W, **K, return_winner=True)
    d64, w64 = R.depth_f64(v, f, w2c, H, W, **K)
    near = np.fmin(R.edge_distance_px(v, f, w2c, w32, **K), R.edge_distance_px(v, f, w2c, w64, **K)) <= 1e-3
    assert near.mean() <= 0.01, f"{name}: {near.sum()} pixels within 1e-3 px of a deciding edge"
    assert (d64 > 0).sum() > 0.2 * H * W
    ok = ~near
    assert np.array_equal((d32 > 0)[ok], (d64 > 0)[ok])
    both = ok & (d64 > 0)
    rel = np.abs(d32.astype(np.float64) - d64)[both] / d64[both]
    assert rel.max() <= 1e-5, f"{name}: depth off by {rel.max():.3e} relative"


def point_masks_transcribed(points, depths, c2ws, H, W, fx, fy, cx, cy, eps=0.005):
    """cull_mesh.py:96-183 line for line on the CPU (the forecast branch left out) -> valid_num [V] int32."""
    pnts = torch.from_numpy(np.asarray(points)).clone().detach().float()
    valid_num = torch.zeros(pnts.shape[0]).int()
    for i in range(len(c2ws)):
        c2w = torch.from_numpy(np.asarray(c2ws[i])).float()
        depth = torch.from_numpy(np.asarray(depths[i])).float()
        w2c = torch.inverse(c2w).float()
        ones = torch.ones_like(pnts[:, 0]).reshape(-1, 1)
        homo_points = torch.cat([pnts, ones], dim=1).reshape(-1, 4, 1).float()
        cam_cord = (w2c @ homo_points)[:, :3, :]
        Km = np.eye(3)
        Km[0, 0], Km[0, 2], Km[1, 1], Km[1, 2] = fx, cx, fy, cy
        uv = torch.from_numpy(Km).float() @ cam_cord.float()
        z = uv[:, -1:] + 1e-8
        uv = uv[:, :2] / z
        u, v = uv[:, 0, 0].float(), uv[:, 1, 0].float()
        z = z[:, 0, 0].float()
        in_frustum = (u >= 0) & (u <= W - 1) & (v >= 0) & (v <= H - 1) & (z > 0)
        vgrid = uv.reshape(1, 1, -1, 2).clone()
        vgrid[..., 0] = vgrid[..., 0] / (W - 1) * 2.0 - 1.0
        vgrid[..., 1] = vgrid[..., 1] / (H - 1) * 2.0 - 1.0
        sample = torch.nn.functional.grid_sample(depth.reshape(1, 1, H, W), vgrid, padding_mode="border",
                                                 align_corners=True).reshape(-1)
        front = torch.where(sample > 0.0, z < (sample + eps), torch.ones_like(z).bool())
        valid_num = valid_num + (in_frustum & front).int()
    return valid_num.numpy()


def _nested():
    ov, of = R.icosphere(2, 1.0)
    iv, fi = R.icosphere(2, 0.5)
    return np.concatenate([ov, iv]), np.concatenate([of, fi + ov.shape[0]]), ov.shape[0]


@pytest.mark.parametrize("scene", ["nested", "terrain"])
def test_votes_ref_matches_point_masks(scene):
    if scene == "nested":
        v, f, _ = _nested()
        c2ws = R.orbit(8, 3.0, -0.7)
    else:
        v, f = R.terrain(24, 24)
        c2ws = R.orbit(8, 3.2, -1.6)
    w2cs = np.linalg.inv(c2ws)
    depths = [R.depth_ref(v, f, m, H, W, **K) for m in w2cs]
    counts = np.zeros(v.shape[0], np.int32)
    fragile = np.zeros(v.shape[0], bool)
    for m, d in zip(w2cs, depths):
        vote, g = R.votes_view_ref(v, d, m, H, W, **K)
        counts += vote
        with np.errstate(all="ignore"):
            z, dd, u, vv = (g[k].astype(np.float64) for k in ("z", "d", "u", "v"))
            fragile |= g["in_frustum"] & (dd > 0) & (np.abs(z - (dd + 0.005)) <= 1e-5 * np.abs(z))
            for x, hi in ((u, W - 1), (vv, H - 1)):
                fragile |= (np.abs(x) <= 1e-4) | (np.abs(x - hi) <= 1e-4)
    assert fragile.mean() <= 0.01
    want = point_masks_transcribed(v, depths, c2ws, H, W, **K)
    assert counts.max() > 0 and np.array_equal(counts[~fragile], want[~fragile])
    assert np.array_equal(counts, R.votes_ref(v, f, w2cs, H, W, **K))


def test_fronto_parallel_plane_is_exactly_two():
    v = np.array([[-1.5, -1.25, 2], [1.75, -1.0, 2], [1.5, 1.5, 2], [-1.25, 1.0, 2]], np.float32)
    f = np.array([[0, 1, 2], [0, 2, 3]])
    d = R.depth_ref(v, f, np.eye(4), H, W, **K)
    d64, _ = R.depth_f64(v, f, np.eye(4), H, W, **K)
    assert (d > 0).sum() > 0.5 * H * W and np.array_equal(d > 0, d64 > 0)
    assert np.all(d[d > 0] == np.float32(2.0))


def test_nested_spheres_lose_the_inner_one():
    v, f, n_outer = _nested()
    # eps 0.05: at 70 x 45 the half-pixel shift of the bilinear sample moves the depth of a slanted surface
    # by more than the default 0.005; the inner sphere lies 0.5 behind the outer one
    c2ws = R.around(3.0)
    v2, f2 = R.cull_ref(v, f, c2ws, H, W, **K, min_views=6, eps=0.05)
    assert v2.shape[0] == n_outer and np.array_equal(v2, v[:n_outer])
    assert np.array_equal(f2, f[:f.shape[0] // 2])


def test_winding_and_rotation_leave_the_bits_alone():
    v, f = R.icosphere(2)
    w2c = np.linalg.inv(R.look_at((0.3, -0.4, -3.0), (0, 0, 0)))
    a = R.depth_ref(v, f, w2c, H, W, **K)
    assert np.array_equal(a.view(np.uint32), R.depth_ref(v, f[:, [0, 2, 1]], w2c, H, W, **K).view(np.uint32))
    assert np.array_equal(a.view(np.uint32), R.depth_ref(v, f[:, [1, 2, 0]], w2c, H, W, **K).view(np.uint32))
