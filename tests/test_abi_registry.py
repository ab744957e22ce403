# coding=utf-8
"""The uniform checks of the C ABI, one table-driven pass over _lib.ABIS (no GPU needed): every header under include/ compiles
as C and C++, declares exactly the names of its ctypes table with types the rule of tests/abi_header.py accepts, carries the
version the package binds and the library reports; the library exports exactly the union of the tables; every ctypes struct has
its header's layout; _lib.bind refuses a library whose version or constant differs; and the checker rejects planted errors."""
import ctypes
import inspect
import os

import pytest

import abi_header as H
from tf_geometric_amd import _lib as L

VERSIONS = {"tfgx.h": 114}          # pinned here so that a bump is deliberate; every other header is at 1
HEADERS = pytest.mark.parametrize("abi", L.ABIS, ids=[a.header for a in L.ABIS])


def _version_macro(abi):
    """tfgx_version -> TFGX_ABI_VERSION, tfgx_h16_version -> TFGX_H16_ABI_VERSION."""
    assert abi.version_fn.startswith("tfgx_") and abi.version_fn.endswith("version")
    return abi.version_fn[:-len("version")].upper() + "ABI_VERSION"


def test_the_registry_covers_include():
    assert L.ABIS[0].header == "tfgx.h" and L.ABIS[0].signatures is L.SIGNATURES
    assert sorted(a.header for a in L.ABIS) == sorted(set(os.listdir(H.INCLUDE)) - {"tfgx_dist.h"})
    tables = [v for k, v in vars(L).items() if k.endswith("SIGNATURES")]
    assert len(tables) == len(L.ABIS) and all(any(a.signatures is t for a in L.ABIS) for t in tables)


@HEADERS
def test_header_declares_what_the_table_binds(abi):
    lib = L.load_library()
    declared = H.declarations(abi.header)
    assert H.mismatches(declared, abi.signatures, L.STRUCTS) == []
    assert set(declared) == set(abi.signatures) <= H.exported_symbols()
    assert abi.version_fn in declared and all(fn in declared for fn, _ in abi.constants)
    for name, (res, args) in abi.signatures.items():
        assert name.startswith("tfgx_")
        fn = getattr(lib, name)
        assert fn.restype is res and list(fn.argtypes) == list(args), name


@HEADERS
def test_header_version_is_the_bound_and_the_built_one(abi):
    lib = L.load_library()
    pinned = VERSIONS.get(abi.header, 1)
    assert H.macro(abi.header, _version_macro(abi)) == abi.version == getattr(lib, abi.version_fn)() == pinned
    for fn, bound in abi.constants:
        assert getattr(lib, fn)() == bound > 0
        assert H.macro(abi.header, fn.upper()) in (bound, None)          # where the header has the macro of that name


@HEADERS
def test_header_compiles_as_c_and_cxx(abi, tmp_path):
    H.compiles_as_c_and_cxx(abi.header, tmp_path)


def test_tables_are_disjoint_and_nothing_undeclared_is_exported():
    names = [n for a in L.ABIS for n in a.signatures]
    assert len(names) == len(set(names)), sorted(n for n in set(names) if names.count(n) > 1)
    assert H.exported_symbols() == set(names)


@pytest.mark.parametrize("c_struct", sorted(L.STRUCTS))
def test_struct_has_the_header_layout(c_struct, tmp_path):
    header = [a.header for a in L.ABIS if "typedef struct %s {" % c_struct in H.source(a.header)]
    assert len(header) == 1, header
    H.struct_layout(header[0], c_struct, L.STRUCTS[c_struct], tmp_path)


def test_every_ctypes_struct_is_registered():
    classes = [c for c in vars(L).values() if inspect.isclass(c) and issubclass(c, ctypes.Structure) and c.__module__ == L.__name__]
    assert sorted(classes, key=id) == sorted(L.STRUCTS.values(), key=id)


# ---- bind() refuses a library built for another version ----------------------------------------------------------------
def _bind_fresh(abis):
    return L.bind(ctypes.CDLL(L.LIB_PATH), abis)          # a handle of its own: the cached library is not touched


def test_the_unmodified_registry_binds_cleanly():
    cached = L.load_library()
    lib = _bind_fresh(L.ABIS)
    assert lib is not cached and L.load_library() is cached
    assert lib.tfgx_version() == L.ABI_VERSION and lib.tfgx_last_error.restype is ctypes.c_char_p


@HEADERS
def test_bind_refuses_another_version(abi):
    abis = tuple(a._replace(version=a.version + 1) if a is abi else a for a in L.ABIS)
    with pytest.raises(L.TfgxError) as e:
        _bind_fresh(abis)
    msg = str(e.value)
    assert "include/" + abi.header in msg and abi.version_fn in msg and L.LIB_PATH in msg and "__graft_entry__.build()" in msg
    assert "= {} ".format(abi.version) in msg and "binds {} ".format(abi.version + 1) in msg


@pytest.mark.parametrize("header, fn", [(a.header, fn) for a in L.ABIS for fn, _ in a.constants])
def test_bind_refuses_another_constant(header, fn):
    bump = lambda a: a._replace(constants=tuple((f, v + (f == fn)) for f, v in a.constants))      # noqa: E731
    abis = tuple(bump(a) if a.header == header else a for a in L.ABIS)
    bound = dict(c for a in L.ABIS for c in a.constants)[fn]
    with pytest.raises(L.TfgxError) as e:
        _bind_fresh(abis)
    msg = str(e.value)
    assert "include/" + header in msg and fn in msg and L.LIB_PATH in msg and "__graft_entry__.build()" in msg
    assert "= {} ".format(bound) in msg and "binds {} ".format(bound + 1) in msg


def test_both_constants_are_registered():
    assert [(a.header, c) for a in L.ABIS for c in a.constants] == [
        ("tfgx_seggram.h", ("tfgx_seggram_block", L.SEGGRAM_BLOCK)), ("tfgx_collate.h", ("tfgx_collate_tile", L.COLLATE_TILE))]


# ---- the checker rejects planted errors --------------------------------------------------------------------------------
PLANTED_HEADER = """
#ifndef TFGX_PLANTED_H
#define TFGX_PLANTED_H
#ifdef __cplusplus
extern "C" {
#endif
#define TFGX_PLANTED_ABI_VERSION 3
#define TFGX_PLANTED_BAD ((int32_t)0x80000000)
typedef void* tfgx_stream_t; /* a stream */
typedef struct tfgx_planted_args {
    const float* x;   /* tfgx_not_a_function(int) in a comment */
    int64_t n;
} tfgx_planted_args;
typedef struct tfgx_other_args { int32_t k; } tfgx_other_args;
int tfgx_planted_version(void);
const char* tfgx_planted_error(void);
void tfgx_planted_draw(uint64_t seed, uint32_t slot, int32_t* u);
size_t tfgx_planted_bytes(int64_t n, size_t have);
int tfgx_planted_run(const tfgx_planted_args* args, const float* x, int64_t n, float scale /* > 0 */,
                     int64_t* total, char* buf, size_t buf_bytes, tfgx_stream_t stream);
#ifdef __cplusplus
}
#endif
#endif
"""


class _PlantedArgs(ctypes.Structure):
    _fields_ = [("x", ctypes.c_void_p), ("n", ctypes.c_int64)]


class _OtherArgs(ctypes.Structure):
    _fields_ = [("k", ctypes.c_int32)]


PLANTED_STRUCTS = {"tfgx_planted_args": _PlantedArgs, "tfgx_other_args": _OtherArgs}
_P, _I64, _SZ = ctypes.c_void_p, ctypes.c_int64, ctypes.c_size_t
RUN = [ctypes.POINTER(_PlantedArgs), _P, _I64, ctypes.c_float, ctypes.POINTER(_I64), ctypes.c_char_p, _SZ, _P]


def _planted_table(**changes):
    table = {"tfgx_planted_version": (ctypes.c_int, []), "tfgx_planted_error": (ctypes.c_char_p, []),
             "tfgx_planted_draw": (None, [ctypes.c_uint64, ctypes.c_uint32, ctypes.POINTER(ctypes.c_int32)]),
             "tfgx_planted_bytes": (_SZ, [_I64, _SZ]), "tfgx_planted_run": (ctypes.c_int, list(RUN))}
    table.update(changes)
    return {k: v for k, v in table.items() if v is not None}


def _run_with(i, ctype):
    return (ctypes.c_int, RUN[:i] + [ctype] + RUN[i + 1:])


def test_the_parser_reads_the_planted_header():
    d = H.declarations(PLANTED_HEADER)
    assert sorted(d) == ["tfgx_planted_bytes", "tfgx_planted_draw", "tfgx_planted_error", "tfgx_planted_run", "tfgx_planted_version"]
    assert d["tfgx_planted_version"] == (("val", "int"), []) and d["tfgx_planted_error"] == (("ptr", "char"), [])
    assert d["tfgx_planted_draw"] == (("val", "void"), [("val", "uint64_t"), ("val", "uint32_t"), ("ptr", "int32_t")])
    assert d["tfgx_planted_run"][1] == [("ptr", "tfgx_planted_args"), ("ptr", "float"), ("val", "int64_t"), ("val", "float"),
                                        ("ptr", "int64_t"), ("ptr", "char"), ("val", "size_t"), ("val", "tfgx_stream_t")]
    assert H.macro(PLANTED_HEADER, "TFGX_PLANTED_ABI_VERSION") == 3 and H.macro(PLANTED_HEADER, "TFGX_PLANTED_BAD") is None
    assert H.macro(PLANTED_HEADER, "TFGX_PLANTED") is None


def test_the_rule_accepts_the_right_table():
    d = H.declarations(PLANTED_HEADER)
    assert H.mismatches(d, _planted_table(), PLANTED_STRUCTS) == []
    # every pointer may be an untyped one
    assert H.mismatches(d, _planted_table(tfgx_planted_run=(ctypes.c_int, [_P, _P, _I64, ctypes.c_float, _P, _P, _SZ, _P])),
                        PLANTED_STRUCTS) == []


@pytest.mark.parametrize("what, changes, word", [
    ("a missing argument", dict(tfgx_planted_run=(ctypes.c_int, RUN[:-1])), "8 parameters declared, 7 bound"),
    ("c_int32 for int64_t", dict(tfgx_planted_run=_run_with(2, ctypes.c_int32)), "tfgx_planted_run: argument 2"),
    ("c_int32 for size_t", dict(tfgx_planted_run=_run_with(6, ctypes.c_int32)), "tfgx_planted_run: argument 6"),
    ("c_int64 for size_t", dict(tfgx_planted_bytes=(_SZ, [_I64, _I64])), "tfgx_planted_bytes: argument 1"),
    ("POINTER(c_int32) for int64_t*", dict(tfgx_planted_run=_run_with(4, ctypes.POINTER(ctypes.c_int32))), "argument 4"),
    ("the wrong struct class", dict(tfgx_planted_run=_run_with(0, ctypes.POINTER(_OtherArgs))), "argument 0"),
    ("an unregistered struct class", dict(tfgx_planted_run=_run_with(0, ctypes.POINTER(L.HubLists))), "argument 0"),
    ("c_char_p for float*", dict(tfgx_planted_run=_run_with(1, ctypes.c_char_p)), "argument 1"),
    ("a pointer for a value", dict(tfgx_planted_run=_run_with(3, _P)), "argument 3"),
    ("a value for a stream", dict(tfgx_planted_run=_run_with(7, _I64)), "argument 7"),
    ("a wrong return type", dict(tfgx_planted_bytes=(ctypes.c_int, [_I64, _SZ])), "tfgx_planted_bytes: returns"),
    ("a result for void", dict(tfgx_planted_draw=(ctypes.c_int, _planted_table()["tfgx_planted_draw"][1])), "tfgx_planted_draw: returns"),
    ("a name missing from the table", dict(tfgx_planted_error=None), "tfgx_planted_error: only in the header"),
    ("a name missing from the header", dict(tfgx_planted_more=(ctypes.c_int, [])), "tfgx_planted_more: only in the table"),
])
def test_the_rule_rejects_a_planted_error(what, changes, word):
    bad = H.mismatches(H.declarations(PLANTED_HEADER), _planted_table(**changes), PLANTED_STRUCTS)
    assert len(bad) == 1 and word in bad[0], (what, bad)
