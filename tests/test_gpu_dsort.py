"""The depth sort (csrc/dsort.hip, and rocPRIM's under OPT_ROCPRIM_DSORT) on
chosen keys, through _C.debug_depth_sort, against numpy's stable argsort.

Every comparison is exact: order == argsort(keys, kind="stable") and
keys_sorted == keys[argsort].  Each case runs once.

The sizes follow the sort's own structure and are derived from
_C.debug_depth_sort_tile_keys, so they move with the constants: t keys per
workgroup tile (tb above 2,000,000 keys); the look-back reads 32 status words
per lane with 4 lanes per digit, so parts 1 to 3 of a quad see a real word
from tiles 33, 65 and 97 on, and a second look-back round starts at tile 129;
the last tile pads with key 0xffffffff and takes the padding out of digit
255's count.

Key patterns (PATTERNS): uniform 32-bit; fp32 bits of [2, 4) (what a scene
gives: one digit in the top byte); all keys equal (the order must be the
identity); all keys 0xffffffff (real keys equal to the padding key); three
distinct values (ties across tiles); strictly descending, and descending with
runs of ties; random in one byte and 0xff in the other three (digit 255
dominates three passes); uniform with low byte 0xff in the keys of the last,
partial tile (the padding correction).
"""
from __future__ import annotations

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)

BIG_FROM = 2_000_001  # the first size on the larger tile (asserted in _tiles)


def _tiles():
    """(t, tb): keys per tile at and below 2,000,000 keys, and above."""
    from diff_gaussian_rasterization import _C

    t, tb = _C.debug_depth_sort_tile_keys(1), _C.debug_depth_sort_tile_keys(BIG_FROM)
    assert t != tb and _C.debug_depth_sort_tile_keys(2_000_000) == t, (t, tb)  # a moved threshold fails here
    return t, tb


def _size(spec):
    """spec = (m, a, big): m * tile + a keys, tile = tb if big else t."""
    m, a, big = spec
    t, tb = _tiles()
    return m * (tb if big else t) + a


def _spec_id(spec):
    m, a, big = spec
    if m == 0:
        return str(a)
    return f"{m}{'tb' if big else 't'}" + (f"{a:+d}" if a else "")


def _descending(P, run):
    stride = max(1, 0xFFFFFFFF // max(P, 1))  # spread over all four bytes
    return (((P - 1 - np.arange(P, dtype=np.uint64)) // run) * stride).astype(np.uint32)


def _one_byte(rng, P, b):
    return (np.uint32(0xFFFFFFFF) ^ (rng.integers(0, 256, P, dtype=np.uint32) << np.uint32(8 * b))).astype(np.uint32)


def _last_tile_ff(rng, P, tile):
    k = rng.integers(0, 2 ** 32, P, dtype=np.uint32)
    n = P % tile
    if n:
        k[P - n:] |= np.uint32(0xFF)
    return k


PATTERNS = {
    "uniform": lambda rng, P, tile: rng.integers(0, 2 ** 32, P, dtype=np.uint32),
    "fp32_2_4": lambda rng, P, tile: rng.uniform(2.0, 4.0, P).astype(np.float32).view(np.uint32),
    "equal": lambda rng, P, tile: np.full(P, 0x40490FDB, np.uint32),
    "all_ff": lambda rng, P, tile: np.full(P, 0xFFFFFFFF, np.uint32),
    "three_values": lambda rng, P, tile: rng.choice(np.array([0x00000000, 0x40490FDB, 0xFFFFFFFF], np.uint32), P),
    "descending": lambda rng, P, tile: _descending(P, 1),
    "descending_ties": lambda rng, P, tile: _descending(P, 7),
    "byte0": lambda rng, P, tile: _one_byte(rng, P, 0),
    "byte1": lambda rng, P, tile: _one_byte(rng, P, 1),
    "byte2": lambda rng, P, tile: _one_byte(rng, P, 2),
    "byte3": lambda rng, P, tile: _one_byte(rng, P, 3),
    "last_tile_ff": _last_tile_ff,
}
ALL = tuple(PATTERNS)
LARGE = ("uniform", "equal", "all_ff", "three_values", "last_tile_ff")  # (numpy's argsort dominates at 2M keys)

_REF = {"P": None}


def _ref(name, P):
    """(keys, stable argsort as int32) of a pattern at P keys, computed once
    for the cases of one size (they run back to back) and never written to."""
    from diff_gaussian_rasterization import _C

    if _REF["P"] != P:
        _REF.clear()
        _REF["P"] = P
    if name not in _REF:
        rng = np.random.default_rng([P, ALL.index(name)])
        keys = np.ascontiguousarray(PATTERNS[name](rng, P, _C.debug_depth_sort_tile_keys(P)), np.uint32)
        assert keys.shape == (P,)
        order = np.argsort(keys, kind="stable").astype(np.int32)
        keys.setflags(write=False)
        order.setflags(write=False)
        _REF[name] = (keys, order)
    return _REF[name]


def _sort(keys, prepared):
    from diff_gaussian_rasterization import _C

    order, ks = _C.debug_depth_sort(torch.from_numpy(keys.view(np.int32).copy()).to(DEV), prepared)
    return order, ks


def _mismatch(name, P, prepared):
    """None, or what differs from the stable argsort for this pattern."""
    keys, want = _ref(name, P)
    order, ks = _sort(keys, prepared)
    order, ks = order.cpu().numpy(), ks.cpu().numpy().view(np.uint32)
    if name == "equal":
        assert np.array_equal(want, np.arange(P, dtype=np.int32))
    bad = np.flatnonzero(order != want)
    if bad.size:
        return (name, "order", f"{bad.size} of {P}", "first", int(bad[0]), int(order[bad[0]]), int(want[bad[0]]))
    bad = np.flatnonzero(ks != keys[want])
    if bad.size:
        return (name, "keys_sorted", f"{bad.size} of {P}", "first", int(bad[0]))
    return None


def _check(names, P, prepared):
    """Every pattern runs once; the failure names all that differ."""
    failed = [m for m in (_mismatch(name, P, prepared) for name in names) if m is not None]
    assert not failed, (P, "prepared" if prepared else "own-hist", failed)


# the small tile: below, at and past one tile; the first real word of quad parts 1, 2 and 3; the second
# look-back round; the last size on the small tile
SMALL_ALL = [(0, 1, False), (0, 63, False), (0, 64, False), (0, 65, False), (1, -1, False), (1, 0, False),
             (1, 1, False), (32, 0, False), (32, 1, False), (33, 1, False)]
SMALL_LARGE = [(64, 1, False), (96, 1, False), (128, 0, False), (128, 1, False), (129, 1, False),
               (0, 2_000_000, False)]
# the large tile: its first size, an exact multiple (no padding) and one key more
BIG = [(0, BIG_FROM, True), (163, 0, True), (163, 1, True)]


@pytest.mark.parametrize("prepared", [True, False], ids=["prepared", "own-hist"])
@pytest.mark.parametrize("spec", SMALL_ALL, ids=_spec_id)
def test_dsort_small_tile_every_pattern(spec, prepared):
    P = _size(spec)
    _check(ALL, P, prepared)


@pytest.mark.parametrize("prepared", [True, False], ids=["prepared", "own-hist"])
@pytest.mark.parametrize("spec", SMALL_LARGE, ids=_spec_id)
def test_dsort_small_tile_lookback(spec, prepared):
    from diff_gaussian_rasterization import _C

    P = _size(spec)
    assert _C.debug_depth_sort_tile_keys(P) == _tiles()[0]
    _check(LARGE, P, prepared)


@pytest.mark.parametrize("spec", BIG, ids=_spec_id)
def test_dsort_big_tile(spec):
    """The 12-keys-per-lane instantiation, as the render path runs it (the
    sort's own histogram kernel never runs at these sizes in production)."""
    from diff_gaussian_rasterization import _C

    P = _size(spec)
    assert P >= BIG_FROM and _C.debug_depth_sort_tile_keys(P) == _tiles()[1]
    _check(LARGE, P, True)


@pytest.mark.parametrize("spec", [(1, 1, False), (129, 1, False), (0, BIG_FROM, True)], ids=_spec_id)
def test_rocprim_depth_sort(spec):
    """The A/B reference other tests lean on (OPT_ROCPRIM_DSORT), checked by itself."""
    from diff_gaussian_rasterization import _C

    P = _size(spec)
    _C.set_option(_C.OPT_ROCPRIM_DSORT, 1)
    try:
        for prepared in ((True,) if spec[2] else (True, False)):
            _check(("uniform", "equal", "three_values"), P, prepared)
    finally:
        _C.set_option(_C.OPT_ROCPRIM_DSORT, 0)


def test_dsort_same_bits_on_two_runs():
    P = _size((129, 1, False))
    keys, _ = _ref("three_values", P)
    a, b = _sort(keys, True), _sort(keys, True)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def test_debug_depth_sort_binding():
    """uint32 and int32 inputs give the same unsigned order; P == 0 works;
    non-contiguous input and other dtypes are refused on the device too."""
    from diff_gaussian_rasterization import _C

    keys = np.random.default_rng(7).integers(0, 2 ** 32, 1000, dtype=np.uint32)
    want = np.argsort(keys, kind="stable").astype(np.int32)
    o_u, k_u = _C.debug_depth_sort(torch.from_numpy(keys.copy()).to(DEV), True)
    assert k_u.dtype == torch.uint32 and o_u.dtype == torch.int32
    assert np.array_equal(o_u.cpu().numpy(), want) and np.array_equal(k_u.cpu().numpy(), keys[want])
    o_i, k_i = _C.debug_depth_sort(torch.from_numpy(keys.view(np.int32).copy()).to(DEV), False)
    assert k_i.dtype == torch.int32
    assert np.array_equal(o_i.cpu().numpy(), want) and np.array_equal(k_i.cpu().numpy().view(np.uint32), keys[want])
    for prepared in (True, False):
        o, k = _C.debug_depth_sort(torch.zeros(0, dtype=torch.int32, device=DEV), prepared)
        assert o.numel() == 0 and k.numel() == 0
    with pytest.raises(RuntimeError, match="must be contiguous"):
        _C.debug_depth_sort(torch.zeros(16, dtype=torch.int32, device=DEV)[::2], True)
    for dt in (torch.float32, torch.int64, torch.int16):
        with pytest.raises(RuntimeError, match="1-D int32 / uint32"):
            _C.debug_depth_sort(torch.zeros(8, dtype=dt, device=DEV), True)
    with pytest.raises(RuntimeError, match="1-D int32 / uint32"):
        _C.debug_depth_sort(torch.zeros(4, 2, dtype=torch.int32, device=DEV), True)
