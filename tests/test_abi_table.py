"""The ctypes signature table against include/gsr.h (CPU, no library needed).

diff_gaussian_rasterization/_abi.py writes every prototype of the C ABI down
once (SIGNATURES) with the three structures the prototypes name.  A scalar of
the wrong width is silent on this ABI until the argument is large, so the
table is held to the header here: the same functions, the same number of
arguments, every scalar and return type the exact ctypes class of its C type,
every pointer c_void_p or a POINTER to the pointee's class, the callbacks
their CFUNCTYPEs, and the structures' members in order.
"""
from __future__ import annotations

import ctypes
import os

import pytest

from helpers import parse_header

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROTOTYPES, STRUCTS = parse_header(os.path.join(ROOT, "include", "gsr.h"))

# C scalar -> the ctypes classes that are that type (c_uint32 is c_uint here; both are named for the reader)
SCALARS = {"int": (ctypes.c_int,), "unsigned int": (ctypes.c_uint,), "uint32_t": (ctypes.c_uint32, ctypes.c_uint),
           "int32_t": (ctypes.c_int32, ctypes.c_int), "uint8_t": (ctypes.c_uint8,),
           "long long": (ctypes.c_longlong,), "unsigned long long": (ctypes.c_ulonglong,),
           "size_t": (ctypes.c_size_t,), "float": (ctypes.c_float,), "double": (ctypes.c_double,)}


def _abi():
    from diff_gaussian_rasterization import _abi

    return _abi


def _structures():
    abi = _abi()
    return {"gsr_adam_group": abi.AdamGroup, "gsr_point_index": abi.PointIndex, "gsr_densify_param": abi.DensifyParam}


def _matches(ctype, c, returns=False):
    """Whether the ctypes class `ctype` binds the C type `c` of the header."""
    abi = _abi()
    if c in ("gsr_alloc_fn", "gsr_chunk_fn"):
        return ctype is {"gsr_alloc_fn": abi._ALLOC, "gsr_chunk_fn": abi._CHUNK}[c]
    if c == "char*":
        return returns and ctype is ctypes.c_char_p
    if c.endswith("*"):
        if ctype is ctypes.c_void_p:
            return True
        pointee = c[:-1]
        if pointee == "void" or not (isinstance(ctype, type) and issubclass(ctype, ctypes._Pointer)):
            return False
        want = (_structures()[pointee],) if pointee in _structures() else SCALARS[pointee]
        return ctype._type_ in want
    return ctype in SCALARS[c]


def test_header_parses_to_the_known_shape():
    """The parser sees the header as it is: its first and last prototypes, a multi-line one, the host-only size
    queries and the three structures (a parser that silently lost declarations would let the table lose them)."""
    names = list(PROTOTYPES)
    assert names[0] == "gsr_rasterize_forward" and names[-1] == "gsr_abi_version" and len(names) >= 75
    assert PROTOTYPES["gsr_abi_version"] == ("int", []) and PROTOTYPES["gsr_last_error"] == ("char*", [])
    assert PROTOTYPES["gsr_points_index_bytes"] == ("size_t", ["long long"])
    assert PROTOTYPES["gsr_debug_scan_excl"] == ("int", ["uint32_t*", "uint32_t*", "long long", "uint32_t",
                                                         "uint32_t*", "uint32_t", "void*", "void*"])
    assert len(PROTOTYPES["gsr_rasterize_backward_ex2"][1]) == 60
    assert PROTOTYPES["gsr_mesh_depth"][1][-3:] == ["unsigned long long*", "float*", "void*"]
    assert set(STRUCTS) == set(_structures())
    assert STRUCTS["gsr_point_index"][2:4] == [("double", "bounds_min", 3), ("double", "bounds_max", 3)]


def test_table_names_every_function_of_the_header():
    assert set(_abi().SIGNATURES) == set(PROTOTYPES)


@pytest.mark.parametrize("name", sorted(PROTOTYPES))
def test_signature_matches_the_header(name):
    ret, params = PROTOTYPES[name]
    restype, argtypes = _abi().SIGNATURES[name]
    assert _matches(restype, ret, returns=True), f"{name} returns {ret}, the table says {restype}"
    assert len(argtypes) == len(params), f"{name} takes {len(params)} arguments, the table lists {len(argtypes)}"
    for k, (a, c) in enumerate(zip(argtypes, params)):
        assert _matches(a, c), f"{name} argument {k} is {c}, the table says {a}"


@pytest.mark.parametrize("name", sorted(STRUCTS))
def test_structure_matches_the_header(name):
    fields = _structures()[name]._fields_
    members = STRUCTS[name]
    assert [f[0] for f in fields] == [m[1] for m in members]
    for (fname, ftype), (c, _, length) in zip(fields, members):
        if length is not None:
            assert issubclass(ftype, ctypes.Array) and ftype._length_ == length, f"{name}.{fname} is {c}[{length}]"
            ftype = ftype._type_
        assert _matches(ftype, c), f"{name}.{fname} is {c}, the structure says {ftype}"
