"""The contracts of csrc/gsr_wave.h's block primitives, restated in NumPy.

block_excl_scan<WAVES>: every wave takes a 64-lane inclusive scan by doubling
(lane l adds the value of lane l - o for o = 1, 2, ..., 32 where l >= o),
lane 63 of wave w leaves the wave's total in slot w of the scratch, and after
the one barrier every lane adds the totals of the waves before its own, in
wave order, and subtracts its own input.  The result is the exclusive scan in
thread order modulo 2^32, and the total is the sum of every lane, the last
one included.  The scratch is left holding the wave totals: nothing in the
primitive waits for the other waves to have read it, so a caller that runs it
again owns the barrier in between.

block_minmax6: min of the first three and max of the last three values per
lane, by a xor butterfly (32, 16, ..., 1) in each wave, then the four waves'
results paired (w0, w1), (w2, w3).

These are plain arithmetic over a lane index; no device is involved (the
kernels that call the header are held at their edges by the gpu tests).
"""
from __future__ import annotations

import numpy as np
import pytest

SIZES = (1, 63, 64, 65, 255, 256, 1024)
M32 = 0xFFFFFFFF


def wave_incl_scan(x):
    """uint32 [waves, 64] -> the inclusive scan of each row, by doubling."""
    x = x.copy()
    lane = np.arange(64)
    for o in (1, 2, 4, 8, 16, 32):
        y = np.roll(x, o, axis=1)  # __shfl_up: lane l reads lane l - o (its own value below o: unused)
        x = np.where(lane >= o, x + y, x)
    return x


def block_excl_scan(v):
    """uint32 [n] (n lanes, padded with zeros to whole waves as an idle lane's 0) ->
    (exclusive scan [n], total, scratch as the primitive leaves it)."""
    n = v.size
    waves = (n + 63) // 64
    x = np.zeros(waves * 64, np.uint32)
    x[:n] = v
    x = x.reshape(waves, 64)
    incl = wave_incl_scan(x)
    s_w = incl[:, 63].copy()  # lane 63 of each wave
    before = np.zeros(waves, np.uint32)
    total = np.uint32(0)
    for w in range(waves):  # the combine, in wave order
        before[w + 1:] += s_w[w]
        total = np.uint32((int(total) + int(s_w[w])) & M32)
    out = before[:, None] + incl - x
    return out.reshape(-1)[:n], total, s_w


def _inputs(n):
    rng = np.random.default_rng(n)
    last = np.zeros(n, np.uint32)
    last[-1] = 7
    return {"zero": np.zeros(n, np.uint32), "ones32": np.full(n, M32, np.uint32), "last": last,
            "random": rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)}


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("kind", ("zero", "ones32", "last", "random"))
def test_block_excl_scan_is_exclusive_cumsum_mod_2_32(n, kind):
    v = _inputs(n)[kind]
    with np.errstate(over="ignore"):
        out, total, s_w = block_excl_scan(v)
    incl = np.cumsum(v.astype(np.uint64)) & M32  # (64-bit sums of < 2^42: exact, then wrapped)
    want = np.concatenate([[0], incl[:-1]]).astype(np.uint32)
    assert out.dtype == np.uint32 and np.array_equal(out, want)
    assert out[0] == 0  # exclusive: lane 0 gets nothing, not its own value
    assert int(total) == int(incl[-1])  # the total includes the last lane
    assert int(total) == (int(out[-1]) + int(v[-1])) & M32
    # the scratch still holds every wave's total after the call: a second call overwrites words
    # that a slower wave may not have read yet, which is why the trailing barrier is the caller's
    w = np.zeros(s_w.size * 64, np.uint64)
    w[:n] = v
    assert np.array_equal(s_w, (w.reshape(-1, 64).sum(axis=1) & M32).astype(np.uint32))


def test_block_excl_scan_wraps_at_the_sizes_that_overflow():
    # n lanes of 0xFFFFFFFF: lane i gets -i mod 2^32, the total -n mod 2^32
    for n in SIZES:
        with np.errstate(over="ignore"):
            out, total, _ = block_excl_scan(np.full(n, M32, np.uint32))
        assert np.array_equal(out, (-np.arange(n, dtype=np.int64) & M32).astype(np.uint32))
        assert int(total) == (-n) & M32


def test_block_excl_scan_single_last_lane():
    for n in SIZES:
        v = np.zeros(n, np.uint32)
        v[-1] = 7
        out, total, _ = block_excl_scan(v)
        assert not out.any() and int(total) == 7  # no lane sees it before it; the total does


def wave_butterfly(x, op):
    """[waves, 64] -> every lane of a row holds op over the row (partners l ^ 32, ..., l ^ 1)."""
    lane = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        x = op(x, x[:, lane ^ o])
    return x


def block_minmax6(v):
    """[256, 6] -> [6]: min of columns 0..2, max of columns 3..5 over the block."""
    out = np.empty(6, v.dtype)
    for k in range(6):
        op = np.minimum if k < 3 else np.maximum
        w = wave_butterfly(v[:, k].reshape(4, 64), op)
        assert (w == w[:, :1]).all()  # every lane of a wave agrees
        s = w[:, 0]  # lane 0 of each wave to the scratch
        out[k] = op(op(s[0], s[1]), op(s[2], s[3]))
    return out


@pytest.mark.parametrize("dtype", (np.float32, np.float64))
@pytest.mark.parametrize("n", SIZES[:-1])  # a 256-lane block: up to 256 live lanes
def test_block_minmax6_is_min_and_max(n, dtype):
    rng = np.random.default_rng(100 + n)
    big = np.finfo(dtype).max
    v = np.empty((256, 6), dtype)
    v[:, :3], v[:, 3:] = big, -big  # an idle lane holds the identities
    pts = rng.normal(size=(n, 3)).astype(dtype)
    v[:n, :3] = pts
    v[:n, 3:] = pts
    out = block_minmax6(v)
    assert np.array_equal(out[:3], pts.min(axis=0)) and np.array_equal(out[3:], pts.max(axis=0))
    # the extreme in the last live lane alone is found
    v[n - 1, :3], v[n - 1, 3:] = -5e3, 5e3
    out = block_minmax6(v)
    assert (out[:3] == -5e3).all() and (out[3:] == 5e3).all()
