# coding=utf-8
"""include/tfgx_rows3d.h (node rows -> the dense [G, k, F] tensor) without a GPU: its names and macros, every argument refusal
and every zero-size success of its entry point — argument checks on the host, before any device work.  (The header / table /
version checks are tests/test_abi_registry.py's.)"""
from abi_header import declarations, macro, refused
from sortpool3d_mirror import MAX_GRAPH_NODES, TOO_LONG

HEADER = "tfgx_rows3d.h"
FN = "tfgx_segment_rows_3d_f32"
OK = dict(seg_ptr=1 << 30, seg_node=2 << 30, G=8, N=100, x=3 << 30, ldx=16, n_rows=100, F=16, k=30, key=(3 << 30) + 60, ldkey=16,
          out=4 << 30, ldo=16, slot_node=5 << 30, node_slot=6 << 30, flags=7 << 30, stream=None)


def test_rows3d_names_and_constants():
    from tf_geometric_amd import _lib as L
    assert sorted(declarations(HEADER)) == sorted(L.ROWS3D_SIGNATURES) == ["tfgx_rows3d_version", FN]
    assert list(OK) == ["seg_ptr", "seg_node", "G", "N", "x", "ldx", "n_rows", "F", "k", "key", "ldkey", "out", "ldo", "slot_node",
                        "node_slot", "flags", "stream"] and len(OK) == len(L.ROWS3D_SIGNATURES[FN][1])
    for abi in L.ABIS:
        assert abi.signatures is L.ROWS3D_SIGNATURES or not any("rows3d" in n or "rows_3d" in n for n in abi.signatures), abi.header
    assert macro(HEADER, "TFGX_ROWS3D_ABI_VERSION") == L.ROWS3D_ABI_VERSION == 1
    assert macro(HEADER, "TFGX_ROWS3D_TOO_LONG") == L.ROWS3D_TOO_LONG == L.STATIC_POOL_TOO_LONG == TOO_LONG == 8
    assert L.ROWS3D_MAX_GRAPH_NODES == macro("tfgx_pool_static.h", "TFGX_STATIC_POOL_MAX_GRAPH_NODES") == MAX_GRAPH_NODES == 4096
    assert not L.ROWS3D_TOO_LONG & (L.COLLATE_STATIC_BAD_ID | L.COLLATE_STATIC_OVERFLOW | L.STATIC_POOL_CLAMPED)
    assert macro("tfgx.h", "TFGX_ABI_VERSION") == L.ABI_VERSION == 114


def test_rows3d_argument_validation_without_gpu():
    """Every refusal returns TFGX_ERR_INVALID_ARG (1) on the host (the pointers are not memory), with the entry point and the
    argument named."""
    for name in ("G", "N", "n_rows", "F"):
        refused(FN, OK, {name: -1}, "negative size (" + name)
        refused(FN, OK, {name: 1 << 31}, name + " = 2147483648 does not fit int32")
    refused(FN, OK, dict(k=0), "k must be at least 1")
    refused(FN, OK, dict(k=-3), "k must be at least 1")
    refused(FN, OK, dict(k=1 << 31), "k = 2147483648 does not fit int32")
    refused(FN, OK, dict(G=1 << 20, k=1 << 11), "G * k = 2147483648 slots do not fit int32")
    refused(FN, OK, dict(ldx=15), "ldx is smaller than F")
    refused(FN, OK, dict(ldo=15), "ldo is smaller than F")
    refused(FN, OK, dict(ldkey=0), "ldkey must be at least 1")
    refused(FN, OK, dict(N=101), "N = 101 positions are more than n_rows = 100")
    refused(FN, OK, dict(N=99), "N = 99 is not n_rows = 100")
    for name in ("seg_ptr", "x", "out", "slot_node", "node_slot", "flags"):
        refused(FN, OK, {name: None}, name + " is null")


def test_rows3d_zero_size_calls_succeed_without_gpu():
    from tf_geometric_amd import _lib as L
    lib = L.load_library()
    call = lambda **kw: lib.tfgx_segment_rows_3d_f32(*dict(OK, **kw).values())      # noqa: E731
    assert call(G=0, N=0, n_rows=0) == 0
    assert call(G=0, N=0, n_rows=0, seg_ptr=None, seg_node=None, x=None, key=None, out=None, slot_node=None, node_slot=None,
                flags=None) == 0
    assert call(G=0, N=0, n_rows=0, F=0) == 0
    # an identity plan may cover fewer positions than x has rows; the plain mode needs no flag word (neither is refused: the
    # next check, node_slot, is what answers)
    refused(FN, OK, dict(seg_node=None, N=60, key=None, flags=None, node_slot=None), "node_slot is null")
