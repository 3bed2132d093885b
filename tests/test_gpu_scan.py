"""The tile lists' device-sized exclusive scan (csrc/tilelists.hip,
launch_scan_excl) alone, through _C.debug_scan_excl, against numpy.

Every comparison is exact: the reference is np.cumsum in uint64 reduced mod
2^32.  Every run asserts four things: out[0:n] is the exclusive prefix,
out[n] the total, out[n+1:] still holds the sentinel written beforehand, and
the input past n, filled with 0xffffffff beforehand, changed nothing (no input
beyond n is read, so the count arrays need no clearing).

The lengths follow the scan's own structure and are derived from
_C.debug_list_constants, so they move with the constants: I = kScanItems words
per thread (one 16-B-vector branch for a thread whose I words lie below n, a
scalar branch for the thread that holds index n, whether it straddles n or
starts exactly at it), T = kScanTile words per block (the block holding
index n writes the total, even when it holds no input; later blocks add the
earlier blocks' sums).  The total at out[n] always comes from the scalar
branch of the thread holding index n; the vector branch's thread that ends
exactly at n stores the same word a second time, so the lengths that are
multiples of I are there for the switch between the two branches, not for
a second way of writing the total.

Each length runs with the launch sized for n itself and for 6 n + T (blocks
past n, as the tile pass's bound is ~6x its live length), with n on the host
and with n = mul * *n_dev read on the device (mul 1 and 7, as the tile pass
scans gx * segbase[gy] counts).
"""
from __future__ import annotations

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)

SENTINEL = 0xA5A5A5A5
POISON = 0xFFFFFFFF
GUARD = 64  # sentinel words kept past out[cap]


def _consts():
    from diff_gaussian_rasterization import _C

    c = _C.debug_list_constants()
    T, I = c["kScanTile"], c["kScanItems"]
    assert T == 256 * I and 2 <= I < T - I  # what the lengths below are built on
    return T, I


def _length(spec):
    """spec = (a, b, c): a * T + b * I + c words."""
    T, I = _consts()
    a, b, c = spec
    n = a * T + b * I + c
    assert n >= 0
    return n


def _spec_id(spec):
    a, b, c = spec
    s = "".join(f"{v:+d}{u}" for v, u in ((a, "T"), (b, "I")) if v) + (f"{c:+d}" if c else "")
    return s.lstrip("+") or "0"


# 0, 1, I-1, I, I+1; T-I, T-1, T, T+1, T+I, 2T; 3T+5; one length near 200,000 (48 T + 3 I + 7 at T = 4096)
LENGTHS = [(0, 0, 0), (0, 0, 1), (0, 1, -1), (0, 1, 0), (0, 1, 1), (1, -1, 0), (1, 0, -1), (1, 0, 0), (1, 0, 1),
           (1, 1, 0), (2, 0, 0), (3, 0, 5), (48, 3, 7)]
# (where n comes from, multiplier, bound): the bound is n itself or 6 n + T
MODES = [("host", 1, "tight"), ("host", 1, "loose"), ("device", 1, "tight"), ("device", 1, "loose"),
         ("device", 7, "loose")]

PATTERNS = {
    "zero": lambda rng, n: np.zeros(n, np.uint32),
    "one": lambda rng, n: np.ones(n, np.uint32),
    "below_4096": lambda rng, n: rng.integers(0, 2 ** 12, n, dtype=np.uint32),
    # every value >= 2^32 - 16: the running sum wraps 2^32 at every step from the second on
    "wraps": lambda rng, n: (np.uint32(0xFFFFFFF0) | rng.integers(0, 16, n, dtype=np.uint32)).astype(np.uint32),
}


def _run(values, cap, n_dev_mul):
    """One scan of `values` (n words) with bound cap; n on the host, or on the
    device as mul * word when n_dev_mul = (word, mul).  Asserts the four
    properties against numpy."""
    from diff_gaussian_rasterization import _C

    n = len(values)
    assert cap >= n
    host_in = np.full(cap, POISON, np.uint32)
    host_in[:n] = values
    inp = torch.from_numpy(host_in.view(np.int32)).to(DEV)
    out = torch.from_numpy(np.full(cap + 1 + GUARD, SENTINEL, np.uint32).view(np.int32)).to(DEV)
    assert inp.data_ptr() % 16 == 0
    if n_dev_mul is None:
        _C.debug_scan_excl(inp, out, cap, n)
    else:
        word, mul = n_dev_mul
        assert word * mul == n
        n_dev = torch.tensor([word], dtype=torch.int32, device=DEV)
        _C.debug_scan_excl(inp, out, cap, 0, n_dev=n_dev, mul=mul)
    got = out.cpu().numpy().view(np.uint32)
    incl = np.cumsum(values.astype(np.uint64))
    want = np.concatenate([np.zeros(1, np.uint64), incl]) & np.uint64(0xFFFFFFFF)  # [n + 1]: prefix, then total
    bad = np.flatnonzero(got[:n] != want[:n])
    assert bad.size == 0, ("prefix", n, cap, f"{bad.size} differ", "first", int(bad[0]), int(got[bad[0]]),
                           int(want[bad[0]]))
    assert int(got[n]) == int(want[n]), ("total at out[n]", n, cap, int(got[n]), int(want[n]))
    past = np.flatnonzero(got[n + 1:] != SENTINEL)
    assert past.size == 0, ("written past out[n]", n, cap, "first", n + 1 + int(past[0]))
    assert np.array_equal(inp.cpu().numpy().view(np.uint32), host_in), ("input changed", n, cap)
    return int(incl[-1]) if n else 0


@pytest.mark.parametrize("mode", MODES, ids=lambda m: f"{m[0]}-x{m[1]}-{m[2]}")
@pytest.mark.parametrize("spec", LENGTHS, ids=_spec_id)
def test_scan_excl(spec, mode):
    T, I = _consts()
    where, mul, bound = mode
    n = _length(spec)
    if mul > 1:
        n = -(-n // mul) * mul  # the next multiple: n = mul * word
    cap = n if bound == "tight" else 6 * n + T
    if bound == "loose":
        assert cap // T > n // T  # blocks lie past the one that holds index n
    for k, (name, make) in enumerate(PATTERNS.items()):
        values = make(np.random.default_rng([n, k]), n)
        assert values.dtype == np.uint32 and values.shape == (n,)
        total = _run(values, cap, None if where == "host" else (n // mul, mul))
        if name == "wraps" and n >= 2:
            assert total >= 2 ** 32  # the pattern does what it is for


def test_scan_excl_multiplier_carries_across_a_tile():
    """n_dev below one scan tile, mul * n_dev above it: the length the kernels
    work with is the product, not the word."""
    T, I = _consts()
    word = T // 7 + 1
    assert word < T < 7 * word
    values = PATTERNS["below_4096"](np.random.default_rng(11), 7 * word)
    _run(values, 7 * word, (word, 7))
    _run(values, 6 * 7 * word + T, (word, 7))
    # and across several tiles, ending one word past a thread's vector
    word = (3 * T + I + 1 + 6) // 7
    values = PATTERNS["wraps"](np.random.default_rng(12), 7 * word)
    assert 7 * word > 3 * T and word < T
    _run(values, 7 * word + 5, (word, 7))


def test_scan_excl_same_bits_on_two_runs_and_in_place_offsets():
    """Two runs give the same words; a 16-B-aligned view at an offset into a
    larger buffer (how the binning buffer's arrays are carved) scans the same."""
    from diff_gaussian_rasterization import _C

    T, I = _consts()
    n = 2 * T + I + 3
    values = PATTERNS["below_4096"](np.random.default_rng(13), n)
    want = np.concatenate([np.zeros(1, np.uint64), np.cumsum(values.astype(np.uint64))]) & np.uint64(0xFFFFFFFF)
    buf = torch.full((n + 8,), -1, dtype=torch.int32, device=DEV)
    inp = buf[4:4 + n]
    assert inp.data_ptr() % 16 == 0
    inp.copy_(torch.from_numpy(values.view(np.int32)))
    outs = []
    for _ in range(2):
        out = torch.zeros(n + 1, dtype=torch.int32, device=DEV)
        _C.debug_scan_excl(inp, out, n, n)
        outs.append(out)
    assert torch.equal(outs[0], outs[1])
    assert np.array_equal(outs[0].cpu().numpy().view(np.uint32), want.astype(np.uint32))
    assert int((buf[:4] != -1).sum()) == 0 and int((buf[4 + n:] != -1).sum()) == 0
