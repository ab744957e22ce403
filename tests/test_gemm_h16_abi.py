# coding=utf-8
"""include/tfgx_gemm_h16.h (the dense GEMM and its weight gradient reading a 16-bit table) without a GPU: every declared symbol
pinned by the exact list of its names (the uniform header / table / version checks are tests/test_abi_registry.py's), every
refusal names its member before any device work (launch and describe), describe honours its buffer, and for every shape of the route table
(and a seeded sweep of random shapes) the 16-bit call on a table of either stride takes the route of the float32 call on the
dense widened matrix: tfgx_gemm_h16_describe == dtype tag + tfgx_gemm_describe(lda = K)."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np

from abi_header import declarations
from conftest import ROOT

HEADER = "tfgx_gemm_h16.h"
BF16, F16 = 1, 2
TAG = {BF16: "bf16 ", F16: "f16 "}
A_PTR, B_PTR, C_PTR, WS_PTR = 1 << 30, 2 << 30, 3 << 30, 4 << 30      # 16-byte aligned; describe never dereferences them

# (M, K, N, workspace lent, the route of the float32 call on the dense matrix as a regular expression).  "[^>]*" stands for
# the load-width flags of a generic-kernel instantiation where the table of routes leaves them open.
ROUTES = [
    (32805, 32, 16, False, r"gemm_rows_kernel<1,bv4> fixed"),
    (32805, 36, 40, False, r"gemm_rows_kernel<2,bv4> fixed"),
    (32805, 44, 64, False, r"gemm_rows_kernel<2,bv4> fixed"),
    (32805, 60, 100, False, r"gemm_rows_kernel<4,bv4> fixed"),
    (32805, 100, 47, False, r"gemm_rows_kernel<2,b1> fixed"),
    (32805, 128, 256, False, r"gemm_rows_kernel<8,bv4> fixed"),
    (32768, 100, 256, False, r"gemm_rows_kernel<8,bv4> fixed"),
    (32805, 256, 128, False, r"gemm_rows_kernel<4,bv4> fixed"),
    (262181, 100, 64, True, r"gemm_rows_kernel<2,bv4> claimed"),
    (32805, 256, 384, False, r"slices\(3\) x gemm_rows_kernel<4,bv4> fixed"),
    (32805, 256, 160, False, r"remainder: gemm_rows_kernel<4,bv4> fixed \+ gemm_rows_kernel<1,bv4> fixed"),
    (4100, 256, 144, False, r"remainder: gemm_kernel<128,128,64,64,[^>]*,ahead> \+ gemm_kernel<256,32,64,32,[^>]*,step>"),
    (32805, 65, 7, False, r"gemm_skinny_kernel<1>"),
    (32805, 602, 16, False, r"gemm_skinny_kernel<1>"),
    (32805, 1433, 16, False, r"gemm_skinny_kernel<1>"),
    (32805, 101, 24, False, r"gemm_skinny_kernel<2>"),
    (32805, 79, 33, False, r"gemm_skinny_kernel<3>"),
    (32805, 602, 40, False, r"gemm_skinny_kernel<3>"),
    (32805, 101, 48, False, r"gemm_skinny_kernel<3>"),
    (1, 1, 1, False, r"gemm_kernel<256,32,64,32,a1,b1,step>"),
    (37, 7, 5, False, r"gemm_kernel<256,32,64,32,a1,b1,step>"),
    (32805, 30, 20, False, r"gemm_kernel<256,32,64,32,a1,bv4,step>"),
    (513, 100, 47, False, r"gemm_kernel<128,64,32,64,av4,b1,step>"),
    (32805, 1433, 64, False, r"gemm_kernel<128,64,32,64,av4,bv4,step>"),
    (32805, 101, 256, False, r"gemm_kernel<128,128,64,64,av4,bv4,step>"),
    (32805, 128, 300, False, r"gemm_kernel<128,128,64,64,av4,bv4,step>"),
    (2708, 1433, 16, True, r"split-K\(10\) gemm_kernel<[^>]*>"),
    (2708, 1433, 7, True, r"split-K\(10\) gemm_kernel<[^>]*>"),
    (2708, 1433, 64, True, r"split-K\(10\) gemm_kernel<[^>]*>"),
    (2708, 1433, 256, True, r"split-K\(5\) gemm_kernel<[^>]*>"),
    (1000, 602, 128, True, r"split-K\(4\) gemm_kernel<128,128,64,64,[^>]*,step>"),
]


def roundup8(k):
    return (k + 7) // 8 * 8


def f32_route(lib, M, K, N, lent, a=A_PTR, b=B_PTR, c=C_PTR, ldb=None, ldc=None, ws=WS_PTR):
    """tfgx_gemm_describe for a dense float32 A (lda = K)."""
    buf = ctypes.create_string_buffer(200)
    wsb = lib.tfgx_gemm_workspace_bytes(M, K, N) if lent else 0
    assert lib.tfgx_gemm_describe(a, K, b, N if ldb is None else ldb, None, 0, 0, c, N if ldc is None else ldc, M, K, N,
                                  ws if wsb else None, wsb, buf, 200) == 0, lib.tfgx_last_error()
    return buf.value.decode()


def h16_route(lib, dt, lda, M, K, N, lent, a=A_PTR, b=B_PTR, c=C_PTR, ldb=None, ldc=None, ws=WS_PTR):
    buf = ctypes.create_string_buffer(200)
    wsb = lib.tfgx_gemm_workspace_bytes(M, K, N) if lent else 0
    assert lib.tfgx_gemm_h16_describe(a, dt, lda, b, N if ldb is None else ldb, None, 0, 0, c, N if ldc is None else ldc, M, K, N,
                                      ws if wsb else None, wsb, buf, 200) == 0, lib.tfgx_last_error()
    return buf.value.decode()


def test_gemm_h16_symbols_and_versions():
    from tf_geometric_amd import _lib
    names = sorted(declarations(HEADER))
    assert names == sorted(_lib.GEMM_H16_SIGNATURES) == [
        "tfgx_gemm_bias_act_cols_ws_h16", "tfgx_gemm_h16_describe", "tfgx_gemm_h16_version", "tfgx_gemm_tn_gated_h16"]
    assert not any("h16" in n for n in _lib.SIGNATURES)
    # the workspace sizes are the float32 entries': no new size function
    assert not [n for n in names if "workspace" in n]


def test_gemm_h16_refusals_without_gpu():
    """Every refusal returns TFGX_ERR_INVALID_ARG on the host with its member named, from the launch AND from describe."""
    from tf_geometric_amd import _lib
    lib = _lib.load_library()
    buf = ctypes.create_string_buffer(200)
    M, K, N = 64, 100, 16

    def refused(word, a=A_PTR, dt=BF16, lda=104, b=B_PTR, ldb=N, act=0, act_cols=0, c=C_PTR, ldc=N, m=M, k=K, n=N):
        assert lib.tfgx_gemm_bias_act_cols_ws_h16(a, dt, lda, b, ldb, None, act, act_cols, c, ldc, m, k, n, None, 0, None) == 1
        assert word in lib.tfgx_last_error(), (word, lib.tfgx_last_error())
        buf.value = b"x"
        assert lib.tfgx_gemm_h16_describe(a, dt, lda, b, ldb, None, act, act_cols, c, ldc, m, k, n, None, 0, buf, 200) == 1
        assert buf.value == b"" and word in lib.tfgx_last_error(), (word, lib.tfgx_last_error())

    for bad in (0, 3, -1):
        refused(b"dtype", dt=bad)
    refused(b"multiple of 8", lda=100)
    refused(b"multiple of 8", lda=1436, k=1433)
    refused(b"16-byte aligned", a=A_PTR + 8)
    refused(b"16-byte aligned", a=A_PTR + 2, dt=F16)
    refused(b"smaller than K", lda=96)
    # the float32 entry's own checks
    refused(b"act_cols", act_cols=N + 1)
    refused(b"bad act", act=9)
    refused(b"null pointer", b=None)
    refused(b"null pointer", a=None)
    refused(b"leading dimension", ldb=N - 1)
    refused(b"leading dimension", ldc=N - 1)
    refused(b"bad M / K / N", k=0, lda=8)
    # the weight gradient's entry: the table's layout, then the float32 entry's checks
    G, DW = 5 << 30, 6 << 30

    def tn(x=A_PTR, dt=BF16, ldx=104, ldg=N, ka=K, ldw=N, dw=DW, gate=None, ldt=0, ws=None, wsb=0):
        return lib.tfgx_gemm_tn_gated_h16(x, dt, ldx, G, ldg, gate, ldt, M, ka, N, dw, ldw, None, ws, wsb, None)

    for kw, word in ((dict(dt=0), b"dtype"), (dict(ldx=100), b"multiple of 8"), (dict(x=A_PTR + 4), b"16-byte aligned"),
                     (dict(ldx=96), b"smaller than K"), (dict(dw=None), b"bad dW"), (dict(ldw=N - 1), b"bad dW"),
                     (dict(gate=7 << 30, ldt=N - 1), b"gate"), (dict(ldg=N - 1), b"leading dimension"),
                     (dict(), b"workspace too small")):
        assert tn(**kw) == 1 and word in lib.tfgx_last_error(), (kw, lib.tfgx_last_error())
    # M == 0 on the forward entry: OK, nothing launched (no device is touched)
    assert lib.tfgx_gemm_bias_act_cols_ws_h16(None, F16, 104, None, N, None, 0, 0, None, N, 0, K, N, None, 0, None) == 0
    assert lib.tfgx_gemm_h16_describe(None, F16, 104, None, N, None, 0, 0, None, N, 0, K, N, None, 0, buf, 200) == 0
    assert buf.value == b"f16 nothing (M = 0)"


def test_gemm_tn_h16_refuses_the_lds_staged_kernel_by_name():
    """TFGX_TN_DIRECT=0 (the float32-only kernel kept for A/B runs) is read once per process: a fresh process."""
    code = ("import ctypes, sys; sys.path.insert(0, {!r}); from tf_geometric_amd import _lib; lib = _lib.load_library(); "
            "rc = lib.tfgx_gemm_tn_gated_h16(1 << 30, 1, 104, 5 << 30, 16, None, 0, 64, 100, 16, 6 << 30, 16, None, None, 0, None); "
            "print(rc, lib.tfgx_last_error().decode())").format(ROOT)
    out = subprocess.check_output([sys.executable, "-c", code], env=dict(os.environ, TFGX_TN_DIRECT="0")).decode()
    assert out.startswith("1 ") and "TFGX_TN_DIRECT" in out, out


def test_gemm_h16_describe_buffer_rules():
    from tf_geometric_amd import _lib
    lib = _lib.load_library()
    args = (A_PTR, BF16, 128, B_PTR, 256, None, 0, 0, C_PTR, 256, 1 << 18, 128, 256)
    big = ctypes.create_string_buffer(b"\xff" * 200, 200)
    assert lib.tfgx_gemm_h16_describe(*args, None, 0, big, 200) == 0 and big.value == b"bf16 gemm_rows_kernel<8,bv4> fixed"
    assert lib.tfgx_gemm_h16_describe(*args, WS_PTR, 4096, big, 200) == 0 and big.value == b"bf16 gemm_rows_kernel<8,bv4> claimed"
    n = len(big.value) + 1
    small = ctypes.create_string_buffer(b"\xff" * 64, 64)
    assert lib.tfgx_gemm_h16_describe(*args, None, 0, small, 8) == 1 and b"buffer too small" in lib.tfgx_last_error()
    assert small.raw[0:1] == b"\x00" and small.raw[8:] == b"\xff" * 56             # empty string, nothing past buf_bytes
    exact = ctypes.create_string_buffer(b"\xff" * 64, 64)
    assert lib.tfgx_gemm_h16_describe(*args, WS_PTR, 4096, exact, n) == 0 and exact.raw[n:] == b"\xff" * (64 - n)
    assert lib.tfgx_gemm_h16_describe(*args, WS_PTR, 4096, exact, n - 1) == 1 and exact.raw[0:1] == b"\x00"
    assert lib.tfgx_gemm_h16_describe(*args, None, 0, None, 200) == 1 and lib.tfgx_gemm_h16_describe(*args, None, 0, big, 0) == 1


def test_gemm_h16_takes_the_float32_route_of_the_dense_matrix():
    """The route table, both dtypes, with and without workspace, both table strides; then ~200 seeded random shapes."""
    from tf_geometric_amd import _lib
    lib = _lib.load_library()
    for M, K, N, lent, pattern in ROUTES:
        ref = f32_route(lib, M, K, N, lent)
        assert re.fullmatch(pattern, ref), (M, K, N, lent, ref)
        for ws in (False, True):
            ref = f32_route(lib, M, K, N, ws)
            for dt in (BF16, F16):
                for lda in (roundup8(K), int(lib.tfgx_h16_friendly_ld(K))):
                    assert lda % 8 == 0 and lda >= K
                    assert h16_route(lib, dt, lda, M, K, N, ws) == TAG[dt] + ref, (M, K, N, ws, dt, lda)
    rng = np.random.default_rng(20260)
    seen = set()
    for i in range(200):
        M = int(np.exp(rng.uniform(0.0, np.log(400000.0))))
        K = int(rng.integers(1, 1500)) if i % 3 else 4 * int(rng.integers(8, 80))
        N = int(rng.integers(1, 400)) if i % 4 else int(rng.choice([16, 40, 64, 128, 256, 384, 160]))
        ws, dt = bool(i % 2), (BF16, F16)[(i // 2) % 2]
        # B and C as column blocks of wider buffers too (their alignment and strides are part of the route)
        ldb, ldc = N + int(rng.integers(0, 3)), N + 4 * int(rng.integers(0, 3))
        b = B_PTR + 4 * int(rng.integers(0, 4))
        ref = f32_route(lib, M, K, N, ws, b=b, ldb=ldb, ldc=ldc)
        for lda in (roundup8(K), int(lib.tfgx_h16_friendly_ld(K))):
            assert h16_route(lib, dt, lda, M, K, N, ws, b=b, ldb=ldb, ldc=ldc) == TAG[dt] + ref, (M, K, N, ws, dt, lda)
        seen.add(ref.split("<")[0].split("(")[0])
    assert {"gemm_rows_kernel", "gemm_skinny_kernel", "gemm_kernel", "split-K"} <= seen, seen
