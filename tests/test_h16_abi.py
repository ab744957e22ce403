# coding=utf-8
"""include/tfgx_h16.h (16-bit feature tables) without a GPU: the exact list of its names, of which tfgx.h knows none (the uniform
header / table / version checks are tests/test_abi_registry.py's), the host argument checks name the refused member
before any device work, the describe entry point honours its buffer, tfgx_h16_friendly_ld keeps its promises, and the draws
of tests/test_gpu_h16.py reach every seg_reduce_h16_kernel instantiation the dispatcher can name."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from abi_header import declarations, source
from test_gpu_fuzz_backward import _graph, _hubs, _rng

HEADER = "tfgx_h16.h"
_SCALE = int(os.environ.get("TFGX_FUZZ_SCALE", "1"))
BF16, F16 = 1, 2

# (G, CH, U) the dispatcher of tfgx_reduce_h16.hip can pick, with the widths (of the issue's list) that select each:
# lanes = ceil(F / 8); (16, 1, 16) = column blocks of 128 elements, taken only with wide_blocks = +1 on whole-line rows
H16_SHAPES = {(4, 1, 0): [1, 3, 7, 8, 20], (8, 1, 0): [47], (16, 1, 0): [100, 128], (32, 1, 0): [172, 256],
              (64, 1, 0): [384, 512], (64, 2, 0): [1030], (16, 1, 16): [256, 384, 512]}
# (DT, G, CH, IS_MAX, WEIGHTED, U)
H16_TARGETS = [(dt,) + s[:2] + (m, w, s[2]) for s in H16_SHAPES for dt in (BF16, F16) for m in (False, True) for w in (False, True)]
H16_SETTINGS = ("plain", "out_block", "hub_order", "hub_noorder", "spans", "n_dst", "plain")
N_H16 = 2 * len(H16_TARGETS)


def _roundup8(F):
    return (F + 7) // 8 * 8


def _avg_lines(F, ld):
    """128-byte lines per row of roundup8(F) 16-bit elements at a stride of ld elements, averaged over the row phases."""
    import math
    row, stride = 2 * _roundup8(F), 2 * ld
    period = 128 // math.gcd(stride, 128)
    return sum(((i * stride) % 128 + row - 1) // 128 + 1 for i in range(period)) / period


def h16_kernel_name(dt, F, ldx, x_ptr, is_max, weighted, wide_blocks):
    """Mirror of group_shape + tfgx_segment_reduce_h16_describe (tfgx_reduce_h16.hip)."""
    lanes = -(-F // 8)
    if F >= 256 and F % 64 == 0 and ldx % 64 == 0 and x_ptr % 128 == 0 and wide_blocks > 0:
        g, ch, u = 16, 1, 16
    else:
        u = 0
        g, ch = next(((g, 1) for g in (4, 8, 16, 32, 64) if lanes <= g), (64, 2))
    b = lambda v: "true" if v else "false"      # noqa: E731
    return "seg_reduce_h16_kernel<{}, {}, {}, {}, {}, {}>".format(dt, g, ch, b(is_max), b(weighted), u)


def _target_of(name):
    t = re.match(r"seg_reduce_h16_kernel<(\d+), (\d+), (\d+), (\w+), (\w+), (\d+)>$", name).groups()
    return (int(t[0]), int(t[1]), int(t[2]), t[3] == "true", t[4] == "true", int(t[5]))


def _rmat(rng, n_dst, n_src, e):
    """A small R-MAT edge list (quadrant probabilities 0.57 / 0.19 / 0.19 / 0.05): a power-law plan."""
    bits = max(1, int(np.ceil(np.log2(max(n_dst, n_src, 2)))))
    row, col = np.zeros(e, np.int64), np.zeros(e, np.int64)
    for _ in range(bits):
        q = rng.choice(4, size=e, p=[0.57, 0.19, 0.19, 0.05])
        row, col = row * 2 + q // 2, col * 2 + q % 2
    return np.stack([row % n_dst, col % n_src]).astype(np.int32)


def draw_h16(seed):
    """One seed of the 16-bit sweep: built for H16_TARGETS[seed % T] under a setting that cycles with the seed."""
    from tf_geometric_amd import plan as P
    rng = _rng(21000, seed)
    T = len(H16_TARGETS)
    tgt, visit = H16_TARGETS[seed % T], seed // T
    dt, g, ch, is_max, weighted, u = tgt
    Fs = H16_SHAPES[(g, ch, u)]
    setting = H16_SETTINGS[(seed % T + 3 * visit) % len(H16_SETTINGS)]
    F = int(Fs[int(rng.integers(0, len(Fs)))])
    n_src = int(rng.integers(2, 300))
    rect = bool(((seed % T) // 2 + (seed % T) // 4 + visit) % 2)
    n_dst = (1 if rng.random() < 0.2 else int(rng.integers(1, n_src))) if rect else n_src
    e = 0 if (rng.random() < 0.06 and not weighted) else int(rng.integers(1, 3000 if F <= 512 else 1200))
    rmat = bool((seed % T + visit) % 3 == 0)
    ei = _rmat(rng, n_dst, n_src, e) if rmat else _graph(rng, n_dst, n_src, e, spare_sources=n_dst < n_src)
    hub = None
    if setting in ("hub_order", "hub_noorder"):
        hub = (int(rng.choice([8, 32, 100])), int(rng.choice([8, 16, 64])))
        r0, m = int(rng.integers(0, n_dst)), hub[0] + int(rng.integers(1, 3 * hub[0]))
        ei = np.concatenate([ei, np.stack([np.full(m, r0, np.int32), rng.integers(0, n_src, m).astype(np.int32)])], 1)
    friendly = bool((seed % T + visit) % 2)
    d = dict(seed=seed, target=tgt, setting=setting, F=F, n_src=n_src, n_dst=n_dst, ei=ei, hub=hub, rect=n_dst < n_src, rmat=rmat,
             dt=dt, op=2 if is_max else int(rng.integers(0, 2)), weighted=weighted, row_order=setting != "hub_noorder",
             ldx=P.h16_friendly_ld(F) if friendly else _roundup8(F), friendly=friendly)
    d["out_off"], d["out_pad"] = (int(rng.choice([1, 2, 3, 4, 8])), int(rng.choice([1, 3, 4, 8]))) if setting == "out_block" else (0, 0)
    d["self"] = bool(rng.random() < 0.5)
    d["bias"] = bool(rng.random() < 0.4)
    d["add_x"] = bool(rng.random() < 0.3)
    d["relu"] = bool(rng.random() < 0.5)
    d["k1"] = int(rng.choice([2, 3, 4])) if setting == "spans" else 0
    d["count_extra"] = bool(d["op"] == 1 and setting in ("hub_order", "hub_noorder", "plain") and rng.random() < 0.7)
    d["n_run"] = int(rng.integers(1, n_dst + 1)) if setting == "n_dst" else n_dst
    d["wide_blocks"] = 1 if u == 16 else -1
    d["quant"] = bool(is_max and rng.random() < 0.6)
    d["half_out"] = bool(setting in ("plain", "out_block", "hub_order", "hub_noorder", "n_dst") and visit % 2 == seed % 2)
    return d


def test_h16_symbols_and_versions():
    from tf_geometric_amd import _lib
    assert sorted(declarations(HEADER)) == sorted(_lib.H16_SIGNATURES) == [
        "tfgx_h16_friendly_ld", "tfgx_h16_version", "tfgx_rows_f32_to_h16", "tfgx_rows_h16_to_f32", "tfgx_segment_reduce_h16",
        "tfgx_segment_reduce_h16_describe"]
    assert not any("h16" in n for n in _lib.SIGNATURES)
    assert "h16" not in source("tfgx.h") and "TFGX_DT_" not in source("tfgx.h")


def _args(F=100, ldx=104, n_dst=4, op=0):
    from tf_geometric_amd import _lib
    a = _lib.ReduceArgs()
    a.F, a.ldx, a.ldo, a.n_dst, a.op, a.rp_stride = F, ldx, F, n_dst, op, 1
    a.x, a.out, a.row_begin, a.row_end, a.col = 1 << 30, 2 << 30, 3 << 30, (3 << 30) + 4, 4 << 30
    return a


def test_h16_argument_validation_without_gpu():
    """Every refusal returns TFGX_ERR_INVALID_ARG on the host, with the member named, from the launch AND from describe."""
    from tf_geometric_amd import _lib
    lib = _lib.load_library()
    buf = ctypes.create_string_buffer(160)

    def refused(a, xdt, odt, word):
        p = None if a is None else ctypes.byref(a)
        assert lib.tfgx_segment_reduce_h16(p, xdt, odt, None) == 1
        assert word in lib.tfgx_last_error(), (word, lib.tfgx_last_error())
        assert lib.tfgx_segment_reduce_h16_describe(p, xdt, odt, buf, 160) == 1 and buf.value == b""
        assert word in lib.tfgx_last_error(), (word, lib.tfgx_last_error())

    refused(None, BF16, 0, b"args is null")
    refused(_args(), 0, 0, b"x_dtype")
    refused(_args(), 3, 0, b"x_dtype")
    refused(_args(), BF16, 3, b"out_dtype")
    refused(_args(), F16, -1, b"out_dtype")
    refused(_args(ldx=100), BF16, 0, b"ldx")
    a = _args()
    a.x = (1 << 30) + 8
    refused(a, BF16, 0, b"x:")
    for member in ("x_tail", "edge_tail", "track"):
        a = _args()
        setattr(a, member, 5 << 30)
        refused(a, BF16, 0, member.encode())
    a = _args()
    a.verify = 1
    refused(a, F16, 0, b"verify")
    a = _args()
    a.accumulate = 1
    refused(a, BF16, BF16, b"accumulate")
    assert lib.tfgx_segment_reduce_h16_describe(ctypes.byref(a), BF16, 0, buf, 160) == 0      # float32 output: allowed
    refused(_args(op=7), BF16, 0, b"bad op")
    refused(_args(F=0), BF16, 0, b"bad n_dst / F")
    # converters
    for fn, args in ((lib.tfgx_rows_f32_to_h16, lambda n, F, dt: (1 << 30, 8, n, F, 2 << 30, 8, dt, None)),
                     (lib.tfgx_rows_h16_to_f32, lambda n, F, dt: (1 << 30, 8, dt, n, F, 2 << 30, 8, None))):
        assert fn(*args(-1, 4, BF16)) == 1 and b"negative" in lib.tfgx_last_error()
        assert fn(*args(4, -1, BF16)) == 1 and b"negative" in lib.tfgx_last_error()
        assert fn(*args(4, 4, 0)) == 1 and b"dtype" in lib.tfgx_last_error()
        assert fn(*args(4, 9, F16)) == 1 and b"leading dimension" in lib.tfgx_last_error()
        assert fn(*args(0, 4, F16)) == 0


def test_h16_describe_buffer_and_names():
    from tf_geometric_amd import _lib
    lib = _lib.load_library()
    big = ctypes.create_string_buffer(b"\xff" * 160, 160)
    names = {}
    for op in (0, 2):
        for w in (0, 4 << 30):
            a = _args(op=op)
            a.w = w
            assert lib.tfgx_segment_reduce_h16_describe(ctypes.byref(a), BF16, 0, big, 160) == 0
            names[(op, bool(w))] = big.value.decode()
            assert big.value.startswith(b"seg_reduce_h16_kernel<")
    assert len(set(names.values())) == 4
    assert names[(0, True)] == "seg_reduce_h16_kernel<1, 16, 1, false, true, 0>"
    a = _args()
    assert lib.tfgx_segment_reduce_h16_describe(ctypes.byref(a), F16, 0, big, 160) == 0
    assert big.value == b"seg_reduce_h16_kernel<2, 16, 1, false, false, 0>"
    small = ctypes.create_string_buffer(b"\xff" * 32, 32)
    assert lib.tfgx_segment_reduce_h16_describe(ctypes.byref(a), F16, 0, small, 8) == 1
    assert b"buffer too small" in lib.tfgx_last_error()
    assert small.raw[0:1] == b"\x00" and small.raw[8:] == b"\xff" * 24
    n = len(big.value) + 1
    exact = ctypes.create_string_buffer(b"\xff" * 64, 64)
    assert lib.tfgx_segment_reduce_h16_describe(ctypes.byref(a), F16, 0, exact, n) == 0 and exact.raw[n:] == b"\xff" * (64 - n)
    assert lib.tfgx_segment_reduce_h16_describe(ctypes.byref(a), F16, 0, exact, n - 1) == 1
    assert lib.tfgx_segment_reduce_h16_describe(ctypes.byref(a), F16, 0, None, 160) == 1
    assert lib.tfgx_segment_reduce_h16_describe(ctypes.byref(a), F16, 0, big, 0) == 1


def test_h16_friendly_ld_properties():
    from tf_geometric_amd import _lib
    from tf_geometric_amd import plan as P
    lib = _lib.load_library()
    for F in range(1, 1101):
        ld = lib.tfgx_h16_friendly_ld(F)
        assert ld % 8 == 0 and ld >= F, (F, ld)
        assert _avg_lines(F, ld) <= _avg_lines(F, _roundup8(F)) + 1e-9, (F, ld)
        assert ld == P.h16_friendly_ld(F), (F, ld, P.h16_friendly_ld(F))
        assert not (ld >= 256 and ld & (ld - 1) == 0), (F, ld)
    assert lib.tfgx_h16_friendly_ld(100) == 128 and _avg_lines(100, 128) == 2.0 and _avg_lines(100, 104) == 2.5
    assert [lib.tfgx_h16_friendly_ld(F) for F in (8, 47, 128, 256, 512)] == [8, 64, 128, 320, 576]


def test_h16_product_path_needs_a_gpu():
    import tf_geometric_amd as tfg
    if torch.cuda.is_available():
        pytest.skip("a GPU is present: the refusal cannot be observed")
    with pytest.raises(tfg._lib.TfgxError):
        tfg.prepare_half_features(torch.zeros(4, 8))
    with pytest.raises(tfg._lib.TfgxError):
        tfg.half_features_to_f32(tfg.HalfRows(torch.zeros(4, 8, dtype=torch.bfloat16), 8))


def test_h16_default_seeds_reach_every_instantiation():
    """The draws of test_gpu_h16.py, the mirror and the host-only describe entry point, no device: every instantiation of
    seg_reduce_h16_kernel the dispatcher can name is reached by the default seeds, each setting on square and rectangular
    plans, uniform and R-MAT graphs, dense and friendly strides, both dtypes."""
    from tf_geometric_amd import _lib as L
    lib = L.load_library()
    seen, combos = set(), set()
    for seed in range(N_H16):
        d = draw_h16(seed)
        a = L.ReduceArgs()
        a.F, a.ldx, a.ldo, a.x, a.out, a.op, a.n_dst, a.rp_stride = d["F"], d["ldx"], d["F"] + d["out_off"] + d["out_pad"], 1 << 30, \
            (2 << 30) + 4 * d["out_off"], d["op"], d["n_run"], 1
        a.w = (4 << 30) if d["weighted"] else 0
        a.wide_blocks = d["wide_blocks"]
        buf = ctypes.create_string_buffer(160)
        assert lib.tfgx_segment_reduce_h16_describe(ctypes.byref(a), d["dt"], 0, buf, 160) == 0, lib.tfgx_last_error()
        name = buf.value.decode()
        assert name == h16_kernel_name(d["dt"], d["F"], d["ldx"], 1 << 30, d["op"] == 2, d["weighted"], d["wide_blocks"]), d["seed"]
        assert _target_of(name) == d["target"], "draw misses its target {}: {}".format(d["target"], name)
        seen.add(_target_of(name))
        hub_d = bool(_hubs(d)[0])
        assert hub_d or d["setting"] not in ("hub_order", "hub_noorder")
        combos.update([("setting", d["setting"], d["rect"]), ("rmat", d["rmat"]), ("friendly", d["friendly"]), ("dt", d["dt"]),
                       ("half_out", d["half_out"], d["dt"]), ("hub", hub_d), ("F", d["F"])])
        for k in ("self", "bias", "add_x", "relu", "count_extra"):
            combos.add((k, d[k]))
        assert d["ei"][0].max(initial=0) < d["n_dst"] and d["ei"][1].max(initial=0) < d["n_src"]
        assert d["ldx"] % 8 == 0 and d["ldx"] >= d["F"]
    assert seen == set(H16_TARGETS) and len(H16_TARGETS) == 2 * 7 * 4, sorted(set(H16_TARGETS) - seen)
    for s in set(H16_SETTINGS):
        assert ("setting", s, True) in combos and ("setting", s, False) in combos, s
    for key in [("rmat", True), ("rmat", False), ("friendly", True), ("friendly", False), ("dt", BF16), ("dt", F16), ("hub", True),
                ("hub", False), ("half_out", True, BF16), ("half_out", True, F16)]:
        assert key in combos, key
    for k in ("self", "bias", "add_x", "relu", "count_extra"):
        assert (k, True) in combos and (k, False) in combos, k
    assert {c[1] for c in combos if c[0] == "F"} == {1, 3, 7, 8, 20, 47, 100, 128, 172, 256, 384, 512, 1030}
