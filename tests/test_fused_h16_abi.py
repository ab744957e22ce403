# coding=utf-8
"""include/tfgx_fused_h16.h (the fused aggregate -> project launch over a 16-bit table) without a GPU: the exact list of its
names (the uniform header / table / version checks are tests/test_abi_registry.py's), every refusal names its member before any
device work (launch and describe), describe names the instantiation the dispatch mirror predicts, and the draws of
tests/test_gpu_fused_h16.py reach every (DT, G, WEIGHTED) instantiation with resident and streamed B, hub and non-hub plans."""
import ctypes
import os
import re

import numpy as np

from abi_header import declarations
from test_gpu_fuzz_backward import _graph, _rng
from test_h16_abi import BF16, F16, _rmat, _roundup8

HEADER = "tfgx_fused_h16.h"
_SCALE = int(os.environ.get("TFGX_FUZZ_SCALE", "1"))

# the issue's lists: tile edges; the G switch (F <= 64 -> 8 lanes, F % 8 == 4 leaves a half-valid last lane); job counts
FH_NDST = [1, 63, 64, 65, 129, 300]
FH_F = [4, 8, 12, 60, 64, 68, 100, 124, 128]
FH_N = [1, 16, 64, 65, 128, 129, 192, 256]
FH_SETTINGS = ("plain", "out_block", "hub_order", "hub_noorder", "skew_order", "skew_noorder", "rect", "no_edges", "hub_order_noslot")
FH_TARGETS = [(dt, g, w) for dt in (BF16, F16) for g in (8, 16) for w in (False, True)]
N_FH = 72


def fused_h16_kernel_name(dt, F, weighted):
    """Mirror of group_lanes + tfgx_aggregate_gemm_h16_describe (tfgx_fused_h16.hip)."""
    return "agg_gemm_h16_kernel<{}, {}, {}>".format(dt, 8 if F <= 64 else 16, "true" if weighted else "false")


def resident_cols(F, N):
    """Mirror of fused_resident_cols: columns of B held in LDS beside the two tiles (160 KB); < N: the rest is streamed."""
    kp, np_ = (F + 1) // 2 * 2, (N + 127) // 128 * 128
    for nl in range(np_, 63, -64):
        if 4 * (kp * (nl + 8) + 2 * kp * 65) + 4 * (16 + 2 * 64) <= 160 * 1024:
            return nl
    return 0


def _target_of(name):
    t = re.match(r"agg_gemm_h16_kernel<(\d+), (\d+), (\w+)>$", name).groups()
    return int(t[0]), int(t[1]), t[2] == "true"


def draw_fused_h16(seed):
    """One seed of the sweep.  F, N, n_dst and the setting cycle with the seed (every listed value is reached whatever the
    generator does); the rest is drawn."""
    from tf_geometric_amd import plan as P
    rng = _rng(31000, seed)
    F = FH_F[seed % len(FH_F)]
    N = FH_N[(seed // len(FH_F) + 3 * seed) % len(FH_N)]
    setting = FH_SETTINGS[(seed + seed // len(FH_SETTINGS)) % len(FH_SETTINGS)]
    n_dst = FH_NDST[(seed + seed // 7) % len(FH_NDST)]
    dt = BF16 if (seed // 2 + seed // 9) % 2 == 0 else F16
    weighted = bool((seed + seed // 4) % 2)
    n_src = n_dst + int(rng.integers(1, 80)) if setting == "rect" else n_dst
    e = 0 if setting == "no_edges" else int(rng.integers(1, 12 * n_dst + 40))
    skew = setting.startswith("skew")
    ei = _rmat(rng, n_dst, n_src, e) if (skew or seed % 4 == 0) else _graph(rng, n_dst, n_src, e, spare_sources=n_dst < n_src)
    hub = None
    if setting.startswith("hub") or skew:
        thr = int(rng.choice([8, 32, 100]))
        r0, m = int(rng.integers(0, n_dst)), thr + int(rng.integers(1, 3 * thr))
        ei = np.concatenate([ei, np.stack([np.full(m, r0, np.int32), rng.integers(0, n_src, m).astype(np.int32)])], 1)
        if setting.startswith("hub"):
            hub = (thr, int(rng.choice([8, 16, 64])))
    friendly = bool((seed + seed // 3) % 2)
    d = dict(seed=seed, F=F, N=N, n_dst=n_dst, n_src=n_src, ei=ei, setting=setting, dt=dt, weighted=weighted, hub=hub,
             ldx=P.h16_friendly_ld(F) if friendly else _roundup8(F), friendly=friendly,
             row_order=setting in ("hub_order", "skew_order", "hub_order_noslot"), slot=setting == "hub_order",
             mean=bool(rng.random() < 0.5), self=bool(rng.random() < 0.5), bias=bool(rng.random() < 0.5),
             relu=bool(rng.random() < 0.5), side=bool(rng.random() < 0.7) or setting == "out_block")
    d["count_extra"] = bool(d["mean"] and rng.random() < 0.6)
    d["c_off"], d["c_pad"], d["s_off"], d["s_pad"] = (4 * int(rng.integers(0, 3)), int(rng.choice([1, 3, 4])), 4 * int(rng.integers(1, 3)),
                                                      4 * int(rng.integers(0, 2))) if setting == "out_block" else (0, 0, 0, 0)
    d["target"] = (dt, 8 if F <= 64 else 16, weighted)
    d["streamed"] = resident_cols(F, N) < N
    return d


def test_fused_h16_symbols_and_versions():
    from tf_geometric_amd import _lib
    names = sorted(declarations(HEADER))
    assert names == sorted(_lib.FUSED_H16_SIGNATURES) == [
        "tfgx_aggregate_gemm_h16", "tfgx_aggregate_gemm_h16_describe", "tfgx_fused_h16_version"]
    # the envelope is the float32 launch's, reused and not redeclared
    assert "tfgx_aggregate_gemm_fits" not in names and "tfgx_aggregate_gemm_fits" in _lib.SIGNATURES


def _args(F=100, ldx=104, n_dst=4, op=0):
    from tf_geometric_amd import _lib
    a = _lib.ReduceArgs()
    a.F, a.ldx, a.n_dst, a.op, a.rp_stride = F, ldx, n_dst, op, 1
    a.x, a.row_begin, a.row_end, a.col = 1 << 30, 3 << 30, (3 << 30) + 4, 4 << 30
    return a


def test_fused_h16_argument_validation_without_gpu():
    """Every refusal returns TFGX_ERR_INVALID_ARG on the host, with the member named, from the launch AND from describe."""
    from tf_geometric_amd import _lib
    lib = _lib.load_library()
    buf = ctypes.create_string_buffer(160)
    B, C = 5 << 30, 6 << 30

    def refused(a, xdt, word, N=256):
        p = None if a is None else ctypes.byref(a)
        assert lib.tfgx_aggregate_gemm_h16(p, xdt, B, N, None, 0, C, N, N, None) == 1
        assert word in lib.tfgx_last_error(), (word, lib.tfgx_last_error())
        assert lib.tfgx_aggregate_gemm_h16_describe(p, xdt, N, buf, 160) == 1 and buf.value == b""
        assert word in lib.tfgx_last_error(), (word, lib.tfgx_last_error())

    refused(None, BF16, b"args is null")
    for bad in (0, 3, -1):
        refused(_args(), bad, b"x_dtype")
    for member in ("x_tail", "edge_tail", "track", "add_x"):
        a = _args()
        setattr(a, member, 7 << 30)
        refused(a, BF16, member.encode())
    for member in ("verify", "accumulate"):
        a = _args()
        setattr(a, member, 1)
        refused(a, F16, member.encode())
    # explicit spans: a row_end that is not row_begin + 1, a stride
    a = _args()
    a.row_end = (3 << 30) + 8
    refused(a, BF16, b"row_end")
    a = _args()
    a.rp_stride = 2
    refused(a, BF16, b"rp_stride")
    refused(_args(op=2), BF16, b"op:")
    refused(_args(ldx=100), BF16, b"ldx")
    a = _args()
    a.x = (1 << 30) + 8
    refused(a, BF16, b"x:")
    # the envelope of tfgx_aggregate_gemm_fits
    refused(_args(F=132, ldx=136), BF16, b"tfgx_aggregate_gemm_fits")
    refused(_args(F=6, ldx=8), BF16, b"tfgx_aggregate_gemm_fits")
    refused(_args(), BF16, b"tfgx_aggregate_gemm_fits", N=257)
    a = _args()
    a.out, a.ldo = (2 << 30) + 4, 100
    refused(a, BF16, b"out")
    # launch-only checks
    a = _args()
    assert lib.tfgx_aggregate_gemm_h16(ctypes.byref(a), BF16, B, 256, None, 9, C, 256, 256, None) == 1 and b"act" in lib.tfgx_last_error()
    assert lib.tfgx_aggregate_gemm_h16(ctypes.byref(a), BF16, None, 256, None, 0, C, 256, 256, None) == 1 and b"B / C" in lib.tfgx_last_error()
    assert lib.tfgx_aggregate_gemm_h16(ctypes.byref(a), BF16, B, 255, None, 0, C, 256, 256, None) == 1 and b"ldb" in lib.tfgx_last_error()
    # n_dst == 0: OK, nothing launched (no device is touched)
    a = _args(n_dst=0)
    assert lib.tfgx_aggregate_gemm_h16(ctypes.byref(a), F16, B, 256, None, 0, C, 256, 256, None) == 0


def test_fused_h16_describe_buffer_and_names():
    from tf_geometric_amd import _lib
    lib = _lib.load_library()
    big = ctypes.create_string_buffer(b"\xff" * 160, 160)
    for dt in (BF16, F16):
        for F in FH_F:
            for w in (0, 4 << 30):
                a = _args(F=F, ldx=_roundup8(F))
                a.w = w
                assert lib.tfgx_aggregate_gemm_h16_describe(ctypes.byref(a), dt, 256, big, 160) == 0, lib.tfgx_last_error()
                assert big.value.decode() == fused_h16_kernel_name(dt, F, bool(w))
    a = _args()
    assert lib.tfgx_aggregate_gemm_h16_describe(ctypes.byref(a), BF16, 256, big, 160) == 0
    assert big.value == b"agg_gemm_h16_kernel<1, 16, false>"
    small = ctypes.create_string_buffer(b"\xff" * 32, 32)
    assert lib.tfgx_aggregate_gemm_h16_describe(ctypes.byref(a), BF16, 256, small, 8) == 1
    assert b"buffer too small" in lib.tfgx_last_error()
    assert small.raw[0:1] == b"\x00" and small.raw[8:] == b"\xff" * 24
    n = len(big.value) + 1
    assert n <= 48
    exact = ctypes.create_string_buffer(b"\xff" * 64, 64)
    assert lib.tfgx_aggregate_gemm_h16_describe(ctypes.byref(a), BF16, 256, exact, n) == 0 and exact.raw[n:] == b"\xff" * (64 - n)
    assert lib.tfgx_aggregate_gemm_h16_describe(ctypes.byref(a), BF16, 256, exact, n - 1) == 1
    assert lib.tfgx_aggregate_gemm_h16_describe(ctypes.byref(a), BF16, 256, None, 160) == 1
    assert lib.tfgx_aggregate_gemm_h16_describe(ctypes.byref(a), BF16, 256, big, 0) == 1


def test_fused_h16_default_seeds_reach_every_instantiation():
    """The draws of test_gpu_fused_h16.py through the mirror and the host-only describe entry point: every instantiation, with
    B resident and streamed, on hub and non-hub plans; every listed n_dst / F / N; every setting; both strides."""
    from tf_geometric_amd import _lib as L
    from test_gpu_fuzz_backward import _thr
    lib = L.load_library()
    seen, combos = set(), set()
    for seed in range(N_FH):
        d = draw_fused_h16(seed)
        a = _args(F=d["F"], ldx=d["ldx"], n_dst=d["n_dst"], op=int(d["mean"]))
        a.w = (4 << 30) if d["weighted"] else 0
        buf = ctypes.create_string_buffer(160)
        assert lib.tfgx_aggregate_gemm_fits(d["F"], d["N"]) == 1
        assert lib.tfgx_aggregate_gemm_h16_describe(ctypes.byref(a), d["dt"], d["N"], buf, 160) == 0, lib.tfgx_last_error()
        name = buf.value.decode()
        assert name == fused_h16_kernel_name(d["dt"], d["F"], d["weighted"]) and _target_of(name) == d["target"], seed
        deg = np.bincount(d["ei"][0], minlength=d["n_dst"])
        E = d["ei"].shape[1]
        hub_d = bool(d["hub"]) and int(deg.max(initial=0)) > _thr(d["hub"][0], d["hub"][1], E, d["n_dst"])
        assert hub_d == d["setting"].startswith("hub"), (seed, d["setting"])
        seen.add(d["target"])
        combos.update([("tgt_stream", d["target"][1:], d["streamed"]), ("tgt_hub", d["target"], hub_d), ("setting", d["setting"]),
                       ("F", d["F"]), ("N", d["N"]), ("n_dst", d["n_dst"]), ("friendly", d["friendly"], d["dt"]),
                       ("empty_rows", bool((deg == 0).any()) and E > 0), ("half_lane", d["F"] % 8 == 4, d["dt"])])
        for k in ("mean", "self", "bias", "relu", "side", "count_extra"):
            combos.add((k, d[k]))
        assert d["ei"][0].max(initial=0) < d["n_dst"] and d["ei"][1].max(initial=0) < d["n_src"]
        assert d["ldx"] % 8 == 0 and d["ldx"] >= _roundup8(d["F"])
    assert seen == set(FH_TARGETS) and len(FH_TARGETS) == 8
    for t in FH_TARGETS:
        assert ("tgt_hub", t, True) in combos and ("tgt_hub", t, False) in combos, t
    for w in (False, True):
        assert ("tgt_stream", (16, w), True) in combos and ("tgt_stream", (16, w), False) in combos and ("tgt_stream", (8, w), False) in combos
    assert resident_cols(128, 256) == 128 and resident_cols(100, 256) == 256 and resident_cols(128, 128) == 128
    assert {c[1] for c in combos if c[0] == "F"} == set(FH_F) and {c[1] for c in combos if c[0] == "N"} == set(FH_N)
    assert {c[1] for c in combos if c[0] == "n_dst"} == set(FH_NDST) and {c[1] for c in combos if c[0] == "setting"} == set(FH_SETTINGS)
    for dt in (BF16, F16):
        assert ("friendly", True, dt) in combos and ("friendly", False, dt) in combos and ("half_lane", True, dt) in combos
    assert ("empty_rows", True) in combos
    for k in ("mean", "self", "bias", "relu", "side", "count_extra"):
        assert (k, True) in combos and (k, False) in combos, k
