# coding=utf-8
"""Host-side contract of the device-side plan builders (no GPU needed): every entry point is declared, exported and bound;
the two policy functions agree with the Python policies they replace; argument errors come back before any launch; and the
ReduceArgs ctypes mirror INTEGRATION.md tells a host to paste has the header's layout."""
import ctypes
import os
import re

import abi_header
from conftest import ROOT

NEW_SYMBOLS = ["tfgx_hub_policy", "tfgx_gat_source_block_count", "tfgx_plan_row_order_workspace_bytes", "tfgx_plan_row_order",
               "tfgx_plan_hub_lists_workspace_bytes", "tfgx_plan_hub_lists_count", "tfgx_plan_hub_lists_emit",
               "tfgx_plan_hub_order_slot", "tfgx_plan_source_blocks"]
ERR_INVALID_ARG, ERR_WORKSPACE = 1, 3
FAKE = ctypes.c_void_p(256)          # a non-NULL address that is never dereferenced: every call below fails its host checks


def _lib():
    from tf_geometric_amd import _lib
    return _lib.load_library()


def test_builders_declared_exported_and_bound():
    from tf_geometric_amd import _lib as L
    lib = _lib()
    declared = abi_header.declarations("tfgx.h")
    for name in NEW_SYMBOLS:
        assert name in declared, name
        assert hasattr(lib, name), name
        assert name in L.SIGNATURES, name


def _py_source_block_count(n_dst, n_src, E, A, W, block_bytes=6 << 20, min_edges=32):
    """nn/conv/gat.py:source_block_count as it was written in Python (the statement the library now holds)."""
    if n_dst == 0 or E == 0:
        return 1
    table = n_src * (int(A) + int(W)) * 4
    kb = min(int(round(table / float(block_bytes))), int(E / float(n_dst) / min_edges), 16)
    return kb if kb >= 2 else 1


def test_hub_policy_matches_python():
    from tf_geometric_amd import plan as P
    lib = _lib()
    thr, chunk = ctypes.c_int32(0), ctypes.c_int32(0)
    cases = [(0, 0), (0, 5), (5, 0), (1, 1)]
    for n in (1, 7, 1000, 233000, 2 ** 21, 2400000):
        for avg in (0.5, 1, 16, 31.9, 32, 32.1, 63.99, 64, 64.01, 127, 128, 129, 255, 256, 257, 489, 511, 512, 513, 4000):
            cases.append((int(avg * n), n))
            cases.append((int(avg * n) + 1, n))
    assert P.HUB_THRESHOLD is None
    for E, n in cases:
        assert lib.tfgx_hub_policy(E, n, ctypes.byref(thr), ctypes.byref(chunk)) == 0
        assert (thr.value, chunk.value) == P.hub_policy(E, n), (E, n)


def test_source_block_count_matches_python():
    lib = _lib()
    B = 6 << 20
    cases = [(0, 10, 100, 8, 64, 0, 0), (10, 10, 0, 8, 64, 0, 0), (0, 0, 0, 0, 0, 0, 0),
             (233000, 233000, 114000000, 8, 64, 0, 0), (2400000, 2400000, 123000000, 8, 64, 0, 0), (600, 600, 30000, 8, 64, 0, 0),
             (233000, 233000, 114000000, 8, 0, 0, 0), (233000, 233000, 114000000, 64, 0, 0, 0)]
    # table / block_bytes exactly k + 0.5: Python's round() goes to the even neighbour
    for k in range(0, 20):
        n_src = (2 * k + 1) * B // (2 * 64 * 4)          # n_src * 64 * 4 = (k + 0.5) * B exactly
        assert n_src * 64 * 4 * 2 == (2 * k + 1) * B
        cases.append((1000, n_src, 1000 * 10000, 8, 56, 0, 0))
        cases.append((1000, n_src, 1000 * 10000, 8, 56, B, 32))
        cases.append((1000, 2 * k + 1, 1000 * 10000, 1, 1, 8, 0))      # table / 8 = 2k + 1: an integer
        cases.append((1000, 2 * k + 1, 1000 * 10000, 1, 0, 8, 0))      # table / 8 = k + 0.5: a tie
    # E / n_dst just below, at and above multiples of min_edges
    for m in range(1, 20):
        for d in (-1, 0, 1):
            for n_dst in (1000, 233000, 7):
                cases.append((n_dst, 233000, 32 * m * n_dst + d, 8, 64, 0, 0))
                cases.append((n_dst, 10 ** 7, 32 * m * n_dst + d, 8, 64, 0, 0))
                cases.append((n_dst, 10 ** 7, 17 * m * n_dst + d, 8, 64, B, 17))
    # the cap at 16
    for n_src in (10 ** 6, 5 * 10 ** 6, 10 ** 8):
        cases.append((1000, n_src, 1000 * 2000, 16, 128, 0, 0))
    for n_dst, n_src, E, A, W, bb, me in cases:
        got = lib.tfgx_gat_source_block_count(n_dst, n_src, E, A, W, bb, me)
        want = _py_source_block_count(n_dst, n_src, E, A, W, bb or B, me or 32)
        assert got == want, (n_dst, n_src, E, A, W, bb, me, got, want)
    assert lib.tfgx_gat_source_block_count(1000, 10 ** 7, 1000 * 2000, 16, 128, 0, 0) == 16
    assert lib.tfgx_gat_source_block_count(-1, 10, 10, 8, 64, 0, 0) == 0 and b"negative" in lib.tfgx_last_error()


def test_source_block_count_python_delegates_to_library():
    from tf_geometric_amd.nn.conv import gat as G

    class _P(object):
        def __init__(self, n_dst, n_src, e):
            self.n_dst, self.n_src, self.num_edges = n_dst, n_src, e
    lib = _lib()
    saved = G.SOURCE_BLOCK_BYTES, G.SOURCE_BLOCK_MIN_EDGES
    try:
        for bb, me in ((6 << 20, 32), (3 << 20, 32), (12 << 20, 8)):
            G.SOURCE_BLOCK_BYTES, G.SOURCE_BLOCK_MIN_EDGES = bb, me
            for p in (_P(233000, 233000, 114000000), _P(2400000, 2400000, 123000000), _P(50000, 80000, 50000 * 600), _P(0, 5, 0)):
                assert G.source_block_count(p, 8, 64) == _py_source_block_count(p.n_dst, p.n_src, p.num_edges, 8, 64, bb, me)
                assert G.source_block_count(p, 8, 64) == lib.tfgx_gat_source_block_count(p.n_dst, p.n_src, p.num_edges, 8, 64,
                                                                                          bb, me)
        G.SOURCE_BLOCKS = 5
        assert G.source_block_count(_P(10, 10, 10), 8, 64) == 5
    finally:
        G.SOURCE_BLOCK_BYTES, G.SOURCE_BLOCK_MIN_EDGES = saved
        G.SOURCE_BLOCKS = None


def _fails(rc, code, lib, words=()):
    assert rc == code, (rc, lib.tfgx_last_error())
    msg = lib.tfgx_last_error()
    assert msg, "no message"
    for w in words:
        assert w in msg, (w, msg)


def test_builders_check_arguments_before_any_launch():
    """Without a GPU a launch would fail with TFGX_ERR_HIP (4): the exact codes below show that nothing was launched."""
    lib = _lib()
    i32 = ctypes.c_int32(0)
    nh, nc = ctypes.c_int64(0), ctypes.c_int64(0)
    # policies
    _fails(lib.tfgx_hub_policy(10, 5, None, ctypes.byref(i32)), ERR_INVALID_ARG, lib, [b"null"])
    _fails(lib.tfgx_hub_policy(-1, 5, ctypes.byref(i32), ctypes.byref(i32)), ERR_INVALID_ARG, lib, [b"negative"])
    # walk order
    ws = lib.tfgx_plan_row_order_workspace_bytes(1000)
    assert ws >= 3 * 4 * 1000 and lib.tfgx_plan_row_order_workspace_bytes(-1) == 0
    _fails(lib.tfgx_plan_row_order(FAKE, 1000, 5000, FAKE, None, FAKE, ws, None), ERR_INVALID_ARG, lib, [b"skewed"])
    _fails(lib.tfgx_plan_row_order(FAKE, -3, 5000, FAKE, ctypes.byref(i32), FAKE, ws, None), ERR_INVALID_ARG, lib, [b"negative"])
    _fails(lib.tfgx_plan_row_order(None, 1000, 5000, FAKE, ctypes.byref(i32), FAKE, ws, None), ERR_INVALID_ARG, lib, [b"null"])
    _fails(lib.tfgx_plan_row_order(FAKE, 1000, 5000, None, ctypes.byref(i32), FAKE, ws, None), ERR_INVALID_ARG, lib, [b"null"])
    _fails(lib.tfgx_plan_row_order(FAKE, 1000, 5000, FAKE, ctypes.byref(i32), None, ws, None), ERR_INVALID_ARG, lib,
           [b"workspace"])
    _fails(lib.tfgx_plan_row_order(FAKE, 1000, 5000, FAKE, ctypes.byref(i32), FAKE, ws - 1, None), ERR_WORKSPACE, lib,
           [b"workspace too small"])
    i32.value = 7      # an empty plan is "not skewed" without touching the device
    assert lib.tfgx_plan_row_order(None, 0, 0, None, ctypes.byref(i32), None, 0, None) == 0 and i32.value == 0
    # hub lists
    ws = lib.tfgx_plan_hub_lists_workspace_bytes(1000)
    assert ws >= 2 * 4 * 1000 + 2 * 8 * 1000 and lib.tfgx_plan_hub_lists_workspace_bytes(-1) == 0
    good = (FAKE, FAKE, 1, 1000, 128, 64)
    _fails(lib.tfgx_plan_hub_lists_count(*good, None, ctypes.byref(nc), FAKE, ws, None), ERR_INVALID_ARG, lib, [b"host"])
    for bad in ((None, FAKE, 1, 1000, 128, 64), (FAKE, FAKE, 0, 1000, 128, 64), (FAKE, FAKE, 1, -1, 128, 64),
                (FAKE, FAKE, 1, 1000, -1, 64), (FAKE, FAKE, 1, 1000, 128, 0)):
        _fails(lib.tfgx_plan_hub_lists_count(*bad, ctypes.byref(nh), ctypes.byref(nc), FAKE, ws, None), ERR_INVALID_ARG, lib)
    _fails(lib.tfgx_plan_hub_lists_count(*good, ctypes.byref(nh), ctypes.byref(nc), None, ws, None), ERR_INVALID_ARG, lib,
           [b"null"])
    _fails(lib.tfgx_plan_hub_lists_count(*good, ctypes.byref(nh), ctypes.byref(nc), FAKE, ws - 1, None), ERR_WORKSPACE, lib,
           [b"workspace too small"])
    outs = (FAKE,) * 5
    _fails(lib.tfgx_plan_hub_lists_emit(*good, 1001, 10, *outs, FAKE, ws, None), ERR_INVALID_ARG, lib, [b"n_hub_rows"])
    _fails(lib.tfgx_plan_hub_lists_emit(*good, 0, 3, *outs, FAKE, ws, None), ERR_INVALID_ARG, lib, [b"chunks"])
    _fails(lib.tfgx_plan_hub_lists_emit(*good, 2, 3, None, FAKE, FAKE, FAKE, FAKE, FAKE, ws, None), ERR_INVALID_ARG, lib,
           [b"null"])
    _fails(lib.tfgx_plan_hub_lists_emit(*good, 2, 3, *outs, FAKE, ws - 1, None), ERR_WORKSPACE, lib)
    assert lib.tfgx_plan_hub_lists_emit(*good, 0, 0, None, None, None, None, None, FAKE, ws, None) == 0    # nothing to write
    # hub_order_slot
    _fails(lib.tfgx_plan_hub_order_slot(FAKE, -1, FAKE, FAKE, None), ERR_INVALID_ARG, lib)
    _fails(lib.tfgx_plan_hub_order_slot(FAKE, 5, None, FAKE, None), ERR_INVALID_ARG, lib, [b"null"])
    assert lib.tfgx_plan_hub_order_slot(None, 0, None, None, None) == 0
    # source blocks: 1 <= KB <= 64
    for kb in (0, -1, 65, 1000):
        _fails(lib.tfgx_plan_source_blocks(FAKE, FAKE, 10, 10, 100, kb, FAKE, FAKE, None), ERR_INVALID_ARG, lib, [b"KB"])
    _fails(lib.tfgx_plan_source_blocks(FAKE, FAKE, -1, 10, 100, 4, FAKE, FAKE, None), ERR_INVALID_ARG, lib, [b"negative"])
    _fails(lib.tfgx_plan_source_blocks(FAKE, FAKE, 10, -10, 100, 4, FAKE, FAKE, None), ERR_INVALID_ARG, lib, [b"negative"])
    _fails(lib.tfgx_plan_source_blocks(FAKE, FAKE, 10, 10, 1 << 31, 4, FAKE, FAKE, None), ERR_INVALID_ARG, lib, [b"int32"])
    _fails(lib.tfgx_plan_source_blocks(FAKE, None, 10, 10, 100, 4, FAKE, FAKE, None), ERR_INVALID_ARG, lib, [b"null"])
    _fails(lib.tfgx_plan_source_blocks(FAKE, FAKE, 10, 10, 100, 4, None, FAKE, None), ERR_INVALID_ARG, lib, [b"null"])
    _fails(lib.tfgx_plan_source_blocks(FAKE, FAKE, 10, 10, 100, 4, FAKE, None, None), ERR_INVALID_ARG, lib, [b"null"])


def _integration_reduce_args():
    """The ReduceArgs class of INTEGRATION.md's binding example, executed as a host would paste it."""
    text = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    m = re.search(r"^class ReduceArgs\(ctypes\.Structure\):.*?\]\s*\n(?=\s*#|\S)", text, flags=re.S | re.M)
    assert m, "INTEGRATION.md has no ReduceArgs mirror"
    ns = {"ctypes": ctypes}
    exec(compile(m.group(0), "INTEGRATION.md", "exec"), ns)
    return ns["ReduceArgs"]


def test_integration_reduce_args_mirror_has_the_header_layout(tmp_path):
    from tf_geometric_amd import _lib as L
    mirror = _integration_reduce_args()
    abi_header.struct_layout("tfgx.h", "tfgx_reduce_args", mirror, tmp_path)
    assert ctypes.sizeof(mirror) == ctypes.sizeof(L.ReduceArgs)
    assert [f for f, _ in mirror._fields_] == [f for f, _ in L.ReduceArgs._fields_]


def test_gat_demo_uses_only_the_c_abi():
    src = open(os.path.join(ROOT, "examples", "c_abi_gat_demo.cpp")).read()
    includes = re.findall(r'#include\s*[<"]([^>"]+)[>"]', src)
    assert "tfgx.h" in includes
    assert not any("torch" in i or "python" in i.lower() or "tfgx_common" in i for i in includes), includes
    for fn in ("tfgx_plan_row_order", "tfgx_plan_hub_lists_count", "tfgx_plan_hub_lists_emit", "tfgx_plan_source_blocks",
               "tfgx_gat_source_block_count", "tfgx_hub_policy", "tfgx_gat_fused_f32", "tfgx_build_csr_by_dst"):
        assert fn in src, fn
