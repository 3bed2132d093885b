"""The tile-list binning (csrc/tilelists.hip) at its structural edges, through
the real forward, against the C oracle.

The rule is helpers.check_binning, as in tests/test_gpu_parity.py: per tile,
ours is the oracle's list (the reference's stable (tile, depth, index) order)
with the culled instances removed, in the same order (which also catches
duplicates), and every removed instance is dead at every pixel of its tile.
K and the radii are exact.  Everything compared is an integer; there is no
tolerance.  The runner checks the lists only: no image audit, no backward.

Every structural size comes from _C.debug_list_constants(), so the scenes move
with the constants, and each scene first asserts, from the oracle's output
alone, that it reaches the edge it is for (a moved constant fails there
instead of silently testing something else).  Scenes built from "pinned"
Gaussians — centre on a tile centre, radius <= 7 px, opacity 0.8: exactly one
tile, never culled — also require that nothing was culled at all, so their
lists are fully determined by the oracle's.

  A  tile-pass segment counts: a row of kTileSeg - 1 ... 2 kTileSeg + 1 entries
     between an empty row and a row of one.
  B  row-pass segment edges: P around kRowSeg and 2 kRowSeg.
  C  the row record: Gaussians of kRecSpans - 1 ... kRecSpans + 2 live rows, one
     over all 40 rows, one rotated (its column span changes from row to row
     past the record).
  D  the coop kernel's direct writes: a first segment of more than kCoopCap
     instances, a second that is staged.
  E  grid width: the widest coop grid, the narrowest and the widest grid of
     tiles_emit_wide_kernel + list_ranges_kernel; on the two wide grids a
     chunk over kEmitCapW (direct writes; D pins the coop kernel's direct
     branch), span end kMaxGrid - 1 in the 16-bit packing.
  F  1 x kMaxGrid tiles with more than kCoopBlocks segments: the lockstep
     stride, the rows scan over several scan tiles, build_seg_table's carry
     over kMaxGrid / 64 rounds, the rows kernels' largest LDS.
  G  no live instance with P > 0: by opacity (the reference's K, the rect
     tiles, stays above 0) and with every Gaussian behind the camera (K = 0).

Not reached at test size, and not tested: the wide kernel's stride (more than
kTileBlocks segments: about 4M row entries); the coop_lds_bytes > 65536
fallback to the wide kernel on a narrow grid (needs more than kMaxGrid rows);
kRowSegBig (equal to kRowSeg, and used above kRowSegBigP = 2M Gaussians only).
"""
from __future__ import annotations

import math

import numpy as np
import pytest
import torch

import gsr_scene as S
import helpers as Hh
from oracle import gsr_oracle as O

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)

# alpha >= 2/255 at opacity 0.8 out to this many sigmas: sqrt(2 ln(0.8 * 255 / 2))
SURE_SIGMAS = math.sqrt(2.0 * math.log(0.8 * 255.0 / 2.0))


def _k():
    from diff_gaussian_rasterization import _C

    return _C.debug_list_constants()


def _case(P, W, H, seed, sigma_px=4.0):
    """P random Gaussians of about sigma_px pixels on a W x H image whose wider
    side spans 60 degrees (so neither half-angle's tangent exceeds tan 30)."""
    tan30 = math.tan(math.radians(30.0))
    fovx = 60.0 if W >= H else math.degrees(2.0 * math.atan(tan30 * W / H))
    cam = S.make_camera(W, H, fovx_deg=fovx)
    fx = W / (2.0 * math.tan(cam.FoVx * 0.5))
    c = Hh.small_case(P=P, W=W, H=H, seed=seed, cam=cam, log_scale=math.log(sigma_px * 3.0 / fx))
    # (small_case spreads the centres over a 60-degree frustum: bring them into this camera's)
    m = c["inp"]["means3D"].clone()
    m[:, 0] *= c["tanx"] / tan30
    m[:, 1] *= c["tany"] / (tan30 * H / W)
    c["inp"]["means3D"] = m.contiguous()
    c["fx"] = fx
    return c


def _shape(c, idx, px, py, z, sx, sy, angle_deg=0.0):
    """Gaussians idx at pixel centres (px, py), depth z, opacity 0.8, flat in
    depth, with sigmas (sx, sy) pixels along their own axes, rotated by
    angle_deg about the view axis."""
    idx = list(idx)
    z = np.broadcast_to(np.asarray(z, np.float64), (len(idx),))
    z = z.copy()
    Hh.place(c, idx, np.broadcast_to(px, (len(idx),)).copy(), np.broadcast_to(py, (len(idx),)).copy(), z)
    s, r, op = (c["inp"][k].clone() for k in ("scales", "rotations", "opacities"))
    w = torch.as_tensor(z / c["fx"], dtype=torch.float32)
    s[idx, 0] = torch.as_tensor(np.broadcast_to(sx, (len(idx),)).copy(), dtype=torch.float32) * w
    s[idx, 1] = torch.as_tensor(np.broadcast_to(sy, (len(idx),)).copy(), dtype=torch.float32) * w
    s[idx, 2] = 0.02 * w
    half = math.radians(angle_deg) / 2.0
    r[idx] = torch.tensor([math.cos(half), 0.0, 0.0, math.sin(half)])
    op[idx] = 0.8
    c["inp"].update(scales=s.contiguous(), rotations=r.contiguous(), opacities=op.contiguous())


def _pin(c, idx, tx, ty, z):
    """Pinned Gaussians: on the centre of tile (tx, ty), sigma 2 px."""
    _shape(c, idx, 16.0 * np.asarray(tx) + 7.5, 16.0 * np.asarray(ty) + 7.5, z, 2.0, 2.0)


def _span(t0, w):
    """(centre, sigma) in pixels of a Gaussian whose alpha >= 2/255 reach covers
    tiles t0 .. t0 + w - 1 of an axis and ends 4 px inside them."""
    return 16.0 * t0 + 8.0 * w - 0.5, (8.0 * w - 4.0) / SURE_SIGMAS


def _oracle(c):
    o = O.forward(*Hh.oracle_args(c))
    if o["state"] is not None:
        o["ranges"] = o["state"].tile_state()["ranges"].astype(np.int64)
        o["list"] = o["state"].binning()["point_list"].astype(np.int64)
    return o


def _tile_of_entry(o):
    return np.repeat(np.arange(len(o["ranges"])), o["ranges"][:, 1] - o["ranges"][:, 0])


def _row_entries(o, gx, gy):
    """Per tile row, the Gaussians with a rect tile in it (the oracle's
    instances; an upper bound of the row pass's entries, exact when nothing
    is culled)."""
    tile = _tile_of_entry(o)
    return [np.unique(o["list"][tile // gx == y]) for y in range(gy)]


def _assert_pinned(o, idx, gx):
    """Gaussians idx each touch exactly one tile with radius <= 7 and centre alpha 0.8."""
    idx = np.asarray(list(idx))
    geo = o["state"].geometry()
    assert np.all(o["radii"][idx] > 0) and np.all(o["radii"][idx] <= 7), np.unique(o["radii"][idx])
    assert np.all(geo["tiles_touched"][idx] == 1)
    assert np.all(geo["conic_opacity"][idx, 3] * 255.0 >= 2.0)
    frac = geo["means2D"][idx] / 16.0 - np.floor(geo["means2D"][idx] / 16.0)
    assert np.all(np.abs(frac - 7.5 / 16.0) < 0.01)  # on a tile centre


def _live_tiles(o, g, W, H):
    """Tiles Gaussian g certainly keeps: those with a pixel of power <= 0 and
    alpha >= 2/255 (helpers.surely_live_tiles' criterion, over every pixel).
    Set of (ty, tx)."""
    geo = o["state"].geometry()
    mx, my = geo["means2D"][g].astype(np.float64)
    a, b, cc, op = geo["conic_opacity"][g].astype(np.float64)
    dx = (mx - np.arange(W, dtype=np.float64))[None, :]
    dy = (my - np.arange(H, dtype=np.float64))[:, None]
    power = -0.5 * (a * dx * dx + cc * dy * dy) - b * dx * dy
    ok = (power <= 0) & (op * np.exp(np.minimum(power, 0.0)) >= 2.0 / 255.0)
    ys, xs = np.nonzero(ok)
    return set(zip((ys // 16).tolist(), (xs // 16).tolist()))


def _gpu_lists(c, o, dead_sample=None, pinned=False):
    """The lists-only runner: K, radii and every tile's list against the oracle."""
    from diff_gaussian_rasterization import _C

    H, W = c["H"], c["W"]
    ga = [x.to(DEV) if isinstance(x, torch.Tensor) else (torch.Tensor([]) if x is None else x)
          for x in Hh.oracle_args(c)] + [False]
    out = _C.rasterize_gaussians(*ga)
    assert out[0] == o["num_rendered"]
    assert np.array_equal(out[5].cpu().numpy(), o["radii"])
    Hh.check_binning(out, o, H, W, dead_sample=dead_sample)
    _, ranges = _C.debug_binning(out[7], out[9], out[0], H, W, with_list=False)
    empty = ranges[:, 1] == ranges[:, 0]
    assert not np.any(ranges[empty]) and not np.any(o["ranges"][o["ranges"][:, 1] == o["ranges"][:, 0]])  # (0, 0)
    if pinned:
        assert int((ranges[:, 1].astype(np.int64) - ranges[:, 0]).sum()) == o["num_rendered"]  # nothing culled
    return out


def _depths(n, seed, lo=2.0, hi=4.0):
    return np.random.default_rng(seed).uniform(lo, hi, n)


def _tie(c, n):
    """helpers.with_depth_ties for shaped Gaussians: n..2 n-1 become copies of 0..n-1 in place, size and
    orientation too (their sizes were set in pixels at their own depth), so each pair has bit-identical depths
    and the same tiles, and the index alone orders it."""
    Hh.with_depth_ties(c, n)
    for key in ("scales", "rotations"):
        t = c["inp"][key].clone()
        t[n:2 * n] = t[:n]
        c["inp"][key] = t.contiguous()


# ------------------------------------------------------------------ A
@pytest.mark.parametrize("n_of", ["T-1", "T", "T+1", "2T", "2T+1"])
def test_tile_pass_segment_counts(n_of):
    """A 4 x 3 grid: row 0 empty, row 1 exactly N pinned Gaussians (N - 1 to
    2 N + 1 around the tile pass's segment size: a last segment of kTileSeg - 1,
    kTileSeg and 1 entries, one and two full segments), row 2 one; with depth
    ties in row 1."""
    T = _k()["kTileSeg"]
    N = {"T-1": T - 1, "T": T, "T+1": T + 1, "2T": 2 * T, "2T+1": 2 * T + 1}[n_of]
    W, H, gx, gy = 64, 48, 4, 3
    c = _case(N + 1, W, H, seed=100 + N % 7)
    rng = np.random.default_rng(N)
    _pin(c, range(N), rng.integers(0, gx, N), np.ones(N), _depths(N, N))
    _pin(c, [N], [2], [2], 3.0)
    _tie(c, N // 3)
    o = _oracle(c)
    _assert_pinned(o, range(N + 1), gx)
    rows = _row_entries(o, gx, gy)
    assert [len(r) for r in rows] == [0, N, 1] and o["num_rendered"] == N + 1
    per_tile = o["ranges"][:, 1] - o["ranges"][:, 0]
    assert np.all(per_tile[gx:2 * gx] > 0)  # every tile of the row, and more than one entry per 64-entry chunk
    depth_bits = o["state"].geometry()["depths"].view(np.uint32)
    assert len(np.unique(depth_bits[:N])) <= N - N // 3
    _gpu_lists(c, o, pinned=True)


# ------------------------------------------------------------------ B
@pytest.mark.parametrize("n_of", ["S-1", "S", "S+1", "2S-1", "2S", "2S+1"])
def test_row_pass_segment_edges(n_of):
    """P around one and two row-pass segments, every Gaussian live (pinned),
    spread over all rows of a 5 x 4 grid."""
    Sg = _k()["kRowSeg"]
    P = {"S-1": Sg - 1, "S": Sg, "S+1": Sg + 1, "2S-1": 2 * Sg - 1, "2S": 2 * Sg, "2S+1": 2 * Sg + 1}[n_of]
    assert P <= _k()["kRowSegBigP"]  # (the row pass cuts by kRowSeg at these sizes)
    W, H, gx, gy = 80, 64, 5, 4
    c = _case(P, W, H, seed=200 + P)
    rng = np.random.default_rng(P)
    _pin(c, range(P), rng.integers(0, gx, P), np.arange(P) % gy, _depths(P, P))
    o = _oracle(c)
    _assert_pinned(o, range(P), gx)
    rows = _row_entries(o, gx, gy)
    assert sum(len(r) for r in rows) == P == o["num_rendered"] and all(len(r) >= P // gy for r in rows)
    _gpu_lists(c, o, pinned=True)


# ------------------------------------------------------------------ C
def test_row_record_length():
    """A 4 x 40 grid.  Thin upright Gaussians whose live rows number
    kRecSpans - 1, kRecSpans, kRecSpans + 1 and kRecSpans + 2 (the last row of
    the 32-B row record, and one and two rows past it, where rows_count and
    rows_emit recompute the span from the footprint), one over all 40 rows, and
    a tall one rotated by 30 degrees, whose column span differs from row to
    row past the record; among 120 pinned ones."""
    R = _k()["kRecSpans"]
    W, H, gx, gy = 64, 640, 4, 40
    nfill = 120
    c = _case(nfill + 6, W, H, seed=300)
    rng = np.random.default_rng(300)
    _pin(c, range(nfill), rng.integers(0, gx, nfill), rng.integers(0, gy, nfill), _depths(nfill, 301))
    tall = list(range(nfill, nfill + 4))
    want_rows = [R - 1, R, R + 1, R + 2]
    for g, n, y0, tx in zip(tall, want_rows, (2, 11, 20, 29), (0, 1, 2, 3)):
        cy, sy = _span(y0, n)
        _shape(c, [g], 16.0 * tx + 7.5, cy, 2.5 + 0.1 * n, 1.5, sy)
    full, rot = nfill + 4, nfill + 5
    _shape(c, [full], 39.5, 319.5, 2.2, 1.5, 200.0)
    _shape(c, [rot], 31.5, 330.0, 3.1, 1.5, 70.0, angle_deg=30.0)
    o = _oracle(c)
    _assert_pinned(o, range(nfill), gx)
    tile = _tile_of_entry(o)
    live = {g: _live_tiles(o, g, W, H) for g in tall + [full, rot]}
    for g, n in zip(tall, want_rows):
        rows_live = sorted({ty for ty, _ in live[g]})
        rect_rows = np.unique(tile[o["list"] == g] // gx)
        assert len(rows_live) == n and rows_live == list(range(rows_live[0], rows_live[0] + n)), (g, rows_live)
        assert rect_rows[0] == rows_live[0], (g, rect_rows, rows_live)  # the record starts at the first live row
    assert {ty for ty, _ in live[full]} == set(range(gy))
    rot_rows = sorted({ty for ty, _ in live[rot]})
    rot_rect0 = int((tile[o["list"] == rot] // gx).min())
    past = [ty for ty in rot_rows if ty >= rot_rect0 + R]
    spans_past = {tuple(sorted(tx for y, tx in live[rot] if y == ty)) for ty in past}
    assert len(past) > R and len(spans_past) >= 3, (past, spans_past)  # different spans in the rows past the record
    out = _gpu_lists(c, o)
    for g in tall + [full, rot]:
        assert Hh.gpu_entries_of(out, g, H, W) >= len(live[g]), g


# ------------------------------------------------------------------ D
def test_coop_direct_writes():
    """A 16 x 2 grid.  Row 0 holds kTileSeg + 88 wide Gaussians, each with at
    least ceil(kCoopCap / kTileSeg) + 1 live tiles, and 30 pinned ones: its
    first tile-pass segment (kTileSeg entries in depth order) carries more than
    kCoopCap instances and is written directly, the second fits the staging
    buffer.  Row 1 holds 50 pinned ones.  With depth ties."""
    k = _k()
    T, cap = k["kTileSeg"], k["kCoopCap"]
    W, H, gx, gy = 256, 32, 16, 2
    assert gx <= k["kCoopMaxGx"]
    nwide, n0, n1 = T + 88, 30, 50
    wmin = -(-cap // T) + 1
    assert wmin <= gx // 2
    P = nwide + n0 + n1
    c = _case(P, W, H, seed=400)
    rng = np.random.default_rng(400)
    w = rng.integers(wmin, gx // 2 + 3, nwide)
    t0 = (rng.random(nwide) * (gx - w + 1)).astype(int)
    cx, sx = _span(t0, w)
    wide = np.arange(nwide)
    _shape(c, wide, cx, 7.5, _depths(nwide, 401), sx, 1.5)
    row0 = np.arange(nwide, nwide + n0)
    row1 = np.arange(nwide + n0, P)
    _pin(c, row0, rng.integers(0, gx, n0), np.zeros(n0), _depths(n0, 402))
    _pin(c, row1, rng.integers(0, gx, n1), np.ones(n1), _depths(n1, 403))
    _tie(c, 100)  # wide Gaussians 100..199 become copies of 0..99
    o = _oracle(c)
    _assert_pinned(o, np.concatenate([row0, row1]), gx)
    assert len(np.unique(o["state"].geometry()["depths"].view(np.uint32)[wide])) <= nwide - 100  # depth ties
    # the instance arithmetic, from the oracle: row 0's entries in (depth bits, index) order, cut at kTileSeg
    geo = o["state"].geometry()
    in_row0 = np.concatenate([wide, row0])
    order = in_row0[np.lexsort((in_row0, geo["depths"].view(np.uint32)[in_row0]))]
    sure0 = {int(g): len([1 for ty, _ in _live_tiles(o, g, W, H) if ty == 0]) for g in wide}
    for g in row0:
        sure0[int(g)] = 1
    assert min(sure0[int(g)] for g in wide) >= wmin
    tile = _tile_of_entry(o)
    rect0 = {int(g): int(((o["list"] == g) & (tile // gx == 0)).sum()) for g in in_row0}
    first, second = order[:T], order[T:]
    assert len(second) == 88 + n0
    assert sum(sure0[int(g)] for g in first) > cap  # the first segment is written directly, whatever is culled
    assert sum(rect0[int(g)] for g in second) <= cap  # the second is staged, whatever is culled
    # (row 1's rect instances of the wide Gaussians are dead there: sigma_y 1.5 px, 8.5 px above the row)
    out = _gpu_lists(c, o)
    for g in wide[:50]:
        assert Hh.gpu_entries_of(out, int(g), H, W) >= sure0[int(g)]


# ------------------------------------------------------------------ E
@pytest.mark.parametrize("gx_of", ["kCoopMaxGx", "kCoopMaxGx+1", "kMaxGrid"])
def test_grid_width(gx_of):
    """gx = the widest coop grid, the narrowest grid of tiles_emit_wide_kernel
    (with list_ranges_kernel) and the widest tile-list grid, each 3 rows tall
    (H = 40: a last row of 8 pixels): 600 random small Gaussians with depth
    ties; pinned ones in tile columns 0, kCoopMaxGx - 1, kCoopMaxGx and gx - 1
    and one clipped by the right image edge; row 1 with more than kTileSeg
    entries, its chunks under the staging cap; and, nearest to the camera,
    flat Gaussians over every column of row 0 (span end gx - 1): on the two
    wide grids enough of them that the chunk they share exceeds kEmitCapW
    instances and is written directly; on the coop grid the same Gaussians
    alone stay under kCoopCap, and whether their segment is written directly
    depends on the entries that share it (scene D pins the coop kernel's
    direct branch)."""
    k = _k()
    coop_max, T = k["kCoopMaxGx"], k["kTileSeg"]
    gx = {"kCoopMaxGx": coop_max, "kCoopMaxGx+1": coop_max + 1, "kMaxGrid": k["kMaxGrid"]}[gx_of]
    W, H, gy = 16 * gx, 40, 3
    nrand, nrow1 = 600, T + 8
    nflat = k["kEmitCapW"] // gx + 1
    cols = sorted({0, coop_max - 1, min(coop_max, gx - 1), gx - 1})
    P = nrand + nrow1 + len(cols) + 1 + nflat
    c = _case(P, W, H, seed=500 + gx % 11, sigma_px=3.0)
    Hh.with_depth_ties(c, 150)  # among the random ones
    rng = np.random.default_rng(gx)
    row1 = np.arange(nrand, nrand + nrow1)
    _pin(c, row1, rng.integers(0, gx, nrow1), np.ones(nrow1), _depths(nrow1, gx + 1))
    edge = np.arange(row1[-1] + 1, row1[-1] + 1 + len(cols))
    _pin(c, edge, cols, np.arange(len(cols)) % 2 * 2, _depths(len(cols), gx + 2))
    clipped = int(edge[-1]) + 1
    _shape(c, [clipped], W - 3.0, 20.0, 2.7, 5.0, 5.0)
    flat = np.arange(clipped + 1, P)
    _shape(c, flat, (W - 1) / 2.0, 7.5, 1.5 + 0.01 * np.arange(nflat), W / 5.0, 1.5)
    o = _oracle(c)
    _assert_pinned(o, np.concatenate([row1, edge]), gx)
    geo = o["state"].geometry()
    tile = _tile_of_entry(o)
    rows = _row_entries(o, gx, gy)
    assert len(rows[1]) > T and len(rows[0]) > 0 and len(rows[2]) > 0
    edge_tiles = {int(tile[o["list"] == g][0]) % gx for g in edge}
    assert edge_tiles == set(cols)
    assert geo["means2D"][clipped, 0] + o["radii"][clipped] > W and (gy // 2, gx - 1) in _live_tiles(o, clipped, W, H)
    # the flat Gaussians: first in depth order (so they share row 0's first chunk) and live in every column of row 0
    depth_bits = geo["depths"].view(np.uint32)
    seen = np.flatnonzero(o["radii"] > 0)
    assert set(seen[np.argsort(depth_bits[seen], kind="stable")[:nflat]].tolist()) == set(flat.tolist())
    assert nflat <= 64 * k["kEmitPlanes"]
    for g in flat:
        assert {tx for ty, tx in _live_tiles(o, int(g), W, H) if ty == 0} == set(range(gx))
    if gx > coop_max:
        assert nflat * gx > k["kEmitCapW"]  # the wide kernel's direct branch
    else:
        assert nflat * gx <= k["kCoopCap"]  # the coop grid's flats alone do not force its direct branch
    # the other chunks stay under the staging cap: no other Gaussian's rect is wider than this many tiles
    others = np.setdiff1d(seen, flat)
    widest = int(np.ceil((2 * o["radii"][others].max() + 16) / 16.0))
    if gx > coop_max:
        assert 64 * k["kEmitPlanes"] * widest <= k["kEmitCapW"]
    out = _gpu_lists(c, o, dead_sample=3000)
    for g in flat:
        assert Hh.gpu_entries_of(out, int(g), H, W) >= gx


# ------------------------------------------------------------------ F
def test_many_rows_many_segments():
    """A 1 x kMaxGrid grid (16 x 16384 pixels): every row one pinned Gaussian,
    9 rows kTileSeg + 1 of them (two segments, the second of one entry), so
    the tile pass has more segments than the coop kernel has blocks and some
    XCD's blocks take a second, strided segment.  Also: the rows scan over
    many scan tiles, build_seg_table's carry over kMaxGrid / 64 rounds, the
    rows kernels' largest LDS (24 B per row)."""
    k = _k()
    gy, T = k["kMaxGrid"], k["kTileSeg"]
    nbig = 9
    W, H, gx = 16, 16 * gy, 1
    P = gy + nbig * T
    assert P == gy + nbig * T and 5000 < P < 6500
    nseg = gy + nbig
    assert nseg > k["kCoopBlocks"]  # some XCD's share exceeds its kCoopBlocks / 8 blocks
    assert gy * -(-P // k["kRowSeg"]) > 2 * k["kScanTile"]  # the rows scan: several blocks
    big_rows = (np.arange(nbig) * (gy // nbig) + 37) % gy  # spread over the XCDs' shares
    ty = np.concatenate([np.arange(gy), np.repeat(big_rows, T)])
    c = _case(P, W, H, seed=600)
    _pin(c, range(P), np.zeros(P), ty, _depths(P, 601))
    o = _oracle(c)
    _assert_pinned(o, range(P), gx)
    per_row = o["ranges"][:, 1] - o["ranges"][:, 0]
    want = np.ones(gy, np.int64)
    want[big_rows] = T + 1
    assert np.array_equal(per_row, want) and o["num_rendered"] == P
    assert int(np.ceil(per_row / T).sum()) == nseg
    _gpu_lists(c, o, pinned=True)


# ------------------------------------------------------------------ G
@pytest.mark.parametrize("how", ["opacity", "behind"])
def test_no_live_instance_with_gaussians(how):
    """No live instance with P > 0: every row empty, zero tile-pass segments, a
    scan of length 0.  Every range is (0, 0) and the image is the background.
    "opacity": every Gaussian inside the frustum with opacity below 1/255.  The
    reference's preprocess does not look at the opacity, so its K (num_rendered,
    the rect tiles) stays above 0 and the binning buffer has that capacity; the
    tile test culls every instance.  "behind": every Gaussian behind the
    camera, K = 0 itself."""
    from diff_gaussian_rasterization import _C

    W, H = 80, 48
    c = _case(200, W, H, seed=700)
    if how == "opacity":
        c["inp"]["opacities"] = torch.full_like(c["inp"]["opacities"], 1.0 / 300.0)
    else:
        c["inp"]["means3D"] = (c["inp"]["means3D"] * torch.tensor([1.0, 1.0, -1.0])).contiguous()
    o = _oracle(c)
    if how == "opacity":
        assert o["num_rendered"] > 0 and int((o["radii"] > 0).sum()) > 150
        assert np.all(o["state"].geometry()["conic_opacity"][:, 3] * 255.0 < 1.0)
    else:
        assert o["num_rendered"] == 0 and not np.any(o["radii"])
    ga = [x.to(DEV) if isinstance(x, torch.Tensor) else (torch.Tensor([]) if x is None else x)
          for x in Hh.oracle_args(c)] + [False]
    out = _C.rasterize_gaussians(*ga)
    assert out[0] == o["num_rendered"] and np.array_equal(out[5].cpu().numpy(), o["radii"])
    _, ranges = _C.debug_binning(out[7], out[9], out[0], H, W, with_list=False)
    assert ranges.shape == (15, 2) and not np.any(ranges)
    if how == "opacity":
        Hh.check_binning(out, o, H, W, dead_sample=500)  # (ours is empty: every oracle instance is dead)
    assert float(out[1].abs().max()) == 0.0 and float(out[2].abs().max()) == 0.0
