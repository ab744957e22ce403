# coding=utf-8
"""Seeded random sweeps of the FORWARD kernels against float64, route by route — the counterpart of
test_gpu_fuzz_backward.py for tfgx_segment_reduce_f32 and tfgx_gemm_bias_act_cols_ws_f32.

Every seed is BUILT FOR one route (a kernel instantiation of the segment reduce, a route of the GEMM dispatcher) and one
setting of the argument surface, and asserts before it launches that the library's own `describe` entry point names that
route: tfgx_segment_reduce_describe against a Python mirror of vector_width + group_shape (seg_kernel_name), tfgx_gemm_describe
against the route class of the draw.  Both describe functions are host code, so test_default_seeds_reach_every_forward_route
runs the draws and the mirrors without a device (made-up pointers with the alignment of the draw) and asserts that the default
seed counts reach every instantiation and every route.

Bars.  MAX is a selection: compared BIT FOR BIT with numpy on float32-rounded messages (the float64 product of two float32
numbers is exact, so np.float32(x64 * w64) is the kernel's message; bias / add_x add one float32 rounding each).  Sums:
assert_parity with 1e-5 * sqrt(max column sum of |messages|), the bar of test_gpu_fuzz.py.  GEMM: 2e-5 with B scaled by
1 / sqrt(K), as test_fuzz_gemm.  Bit identities asserted: row order on = off, wide_blocks +1 = -1, split rows (with and
without the per-edge tail) = dense, MAX span by span = MAX whole row (values and the packed winner table), GEMM with =
without a workspace on the row kernel (claimed = fixed tiles), and every launch run to run.  Outputs are filled with NaN
before each launch; columns / rows outside the launch must keep that fill bit for bit.

The verified-layout route (test_gpu_verified_layout.py is its own file) has one setting here: a table promoted by two
sightings, the served result bit for bit against the plain route, describe naming seg_reduce_verify_kernel.

GAT forward (tfgx_gat_fused_f32): settings plain / forced hub lists / SOURCE_BLOCKS 2, 3, 5 (one state buffer, the two-buffer
rotation) / attention dropout, with bias, activation, add_self_loop=False, scale_d and the stats_ml side output drawn on
top, against f64_layers.gat_attention_f64 at 2e-5 (the bar of test_fuzz_gat_attention; source blocks only reorder a row's
softmax terms, so they get the same bar, not a bit identity).  Witness: SOURCE_BLOCK_STATS["launches"], plan.hub_info(),
plan.row_order() against gat_forward_route.

Deliberate deviation from the issue's table: in the spans setting the MEAN divisor (mean_count = the whole row's count) and
the epilogue travel with the LAST launch only and the earlier launches run as SUM — a MEAN launch divides what it stores, so
"mean_count on every launch" would divide the earlier partial sums again; dist/sharded.py chains its passes this way."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from conftest import assert_parity
from test_gpu_fuzz_backward import _degrees, _graph, _hubs, _rng, _skewed

# soak runs: TFGX_FUZZ_SCALE=10 multiplies the number of seeds of every sweep
_SCALE = int(os.environ.get("TFGX_FUZZ_SCALE", "1"))
_FLT_MAX = np.float32(3.4028234663852886e38)
_NAN_BITS = 0x7FC00000

# ------------------------------------------------------------------------------------------ segment reduce: the instantiations
# (VEC, G, CH, U) that launch_vec can dispatch (tfgx_reduce.hip: vector_width never leaves fewer than 8 lanes per row at
# VEC > 1, so (2, 4) and (4, 4) do not occur), each with the widths F that select it on 16-byte aligned rows with ldx = F
SEG_SHAPES = {
    (1, 4, 1, 0): [1, 2, 3, 4], (1, 8, 1, 0): [5, 7, 8], (1, 16, 1, 0): [9, 12, 15], (1, 32, 1, 0): [17, 31],
    (1, 64, 1, 0): [33, 63], (1, 64, 2, 0): [65, 127], (1, 64, 4, 0): [129, 301],
    (2, 8, 1, 0): [16], (2, 16, 1, 0): [18, 20, 30], (2, 32, 1, 0): [34, 50, 62], (2, 64, 1, 0): [66, 102],
    (2, 64, 2, 0): [130, 250], (2, 64, 4, 0): [258, 1102],
    (4, 8, 1, 0): [32], (4, 16, 1, 0): [36, 48, 64], (4, 32, 1, 0): [68, 96, 100], (4, 64, 1, 0): [132, 200, 252],
    (4, 64, 2, 0): [260, 300, 500], (4, 64, 4, 0): [520, 1100],
    (4, 16, 1, 16): [128, 160, 192, 384, 512, 1024], (4, 32, 1, 16): [256],
}
SPLIT_SHAPES = {(4, 16, 1, 0): [36, 40, 60], (4, 32, 1, 0): [68, 100, 124], (4, 64, 1, 0): [132, 200, 252]}
TRACK_SHAPES = [(4, 8, 1, 0), (4, 16, 1, 0), (4, 32, 1, 0), (4, 64, 1, 0), (4, 16, 1, 16), (4, 32, 1, 16)]
# every instantiation the census must see: (VEC, G, CH, IS_MAX, WEIGHTED, SPLIT, TRACK, U)
SEG_TARGETS = ([s[:3] + (m, w, False, False, s[3]) for s in SEG_SHAPES for m in (False, True) for w in (False, True)] +
               [s[:3] + (m, w, True, False, 0) for s in SPLIT_SHAPES for m in (False, True) for w in (False, True)] +
               [s[:3] + (True, w, False, True, s[3]) for s in TRACK_SHAPES for w in (False, True)])
PLAIN_SETTINGS = ("plain", "strided_x", "out_block", "hub_order", "hub_noorder", "spans", "n_dst")
N_SEG = 2 * len(SEG_TARGETS)

GEMM_ROUTES = (["rows%d" % t for t in range(1, 9)] + ["claimed", "skinny1", "skinny2", "skinny3", "slices", "remainder", "splitk",
                                                       "ahead", "g32", "g64", "g128"])
N_GEMM = 3 * len(GEMM_ROUTES)
N_VERIFY = 8
GAT_SETTINGS = ("plain", "hub", "blocks2", "blocks3", "blocks5", "dropout")
N_GAT = 36
_FLAGS = r"(av4|a1),(bv4|b1)"
GEMM_PATTERNS = dict(
    [("rows%d" % t, r"^gemm_rows_kernel<%d,(bv4|b1)> fixed$" % t) for t in range(1, 9)] +
    [("skinny%d" % t, r"^gemm_skinny_kernel<%d>$" % t) for t in (1, 2, 3)],
    claimed=r"^gemm_rows_kernel<[1-8],(bv4|b1)> claimed$", slices=r"^slices\([234]\) x gemm_rows_kernel<4,(bv4|b1)> fixed$",
    remainder=r"^remainder: gemm_kernel<128,128,64,64,%s,ahead> \+ gemm_kernel<(256,32,64,32|128,64,32,64),%s,step>$" % (_FLAGS, _FLAGS),
    splitk=r"^split-K\(([2-9]|1[0-6])\) gemm_kernel<(256,32,64,32|128,64,32,64|128,128,64,64),%s,(ahead|step)>$" % _FLAGS,
    ahead=r"^gemm_kernel<128,128,64,64,%s,ahead>$" % _FLAGS, g32=r"^gemm_kernel<256,32,64,32,%s,step>$" % _FLAGS,
    g64=r"^gemm_kernel<128,64,32,64,%s,step>$" % _FLAGS, g128=r"^gemm_kernel<128,128,64,64,%s,step>$" % _FLAGS)


# ------------------------------------------------------------------------------------------------------------------ mirrors
def seg_kernel_name(F, ldx, ldo, x_ptr, out_ptr, is_max, weighted, add=None, bias_ptr=None, split=False, track=False,
                    wide_blocks=0):
    """Mirror of vector_width + group_shape + tfgx_segment_reduce_describe (tfgx_reduce.hip) for a plain / split / tracked
    launch: pointers and leading dimensions in, kernel symbol out.  add = (ld_add, add_x pointer) or None."""
    def ok(v):
        al = 4 * v
        good = F % v == 0 and ldx % v == 0 and ldo % v == 0 and x_ptr % al == 0 and out_ptr % al == 0
        if add is not None:
            good = good and add[0] % v == 0 and add[1] % al == 0
        if bias_ptr is not None:
            good = good and bias_ptr % al == 0
        return good
    vec = 4 if ok(4) else (2 if ok(2) else 1)
    while vec > 1 and F // vec < 8:
        vec //= 2
    lanes = -(-F // vec)
    if (vec == 4 and F >= 128 and F % 32 == 0 and ldx % 32 == 0 and x_ptr % 128 == 0 and not split and wide_blocks >= 0
            and (wide_blocks > 0 or os.environ.get("TFGX_REDUCE_WIDE_BLOCKS", "1") != "0")):
        g, ch, u = (32 if F == 256 else 16), 1, 16
    else:
        u = 0
        g, ch = next((g, 1) for g in (4, 8, 16, 32, 64, 1 << 30) if lanes <= g)
        if g > 64:
            g, ch = 64, (2 if lanes <= 128 else 4)
    b = lambda v: "true" if v else "false"      # noqa: E731
    return "seg_reduce_kernel<{}, {}, {}, {}, {}, {}, {}, {}>".format(vec, g, ch, b(is_max), b(weighted),
                                                                      b(split and vec == 4 and ch == 1), b(track), u)


def _target_of(name):
    t = re.match(r"seg_reduce_kernel<(\d+), (\d+), (\d+), (\w+), (\w+), (\w+), (\w+), (\d+)>$", name).groups()
    return (int(t[0]), int(t[1]), int(t[2]), t[3] == "true", t[4] == "true", t[5] == "true", t[6] == "true", int(t[7]))


# -------------------------------------------------------------------------------------------------------------------- draws
def draw_segment(seed):
    """One seed of the segment-reduce sweep: built for SEG_TARGETS[seed % T] under a setting that cycles with the seed."""
    rng = _rng(11000, seed)
    T = len(SEG_TARGETS)
    tgt, visit = SEG_TARGETS[seed % T], seed // T
    vec, g, ch, is_max, weighted, split, track, u = tgt
    shape = (vec, g, ch, u)
    if split:
        setting, Fs = "split", SPLIT_SHAPES[shape]
    elif track:
        setting, Fs = ("track", "track_spans")[(seed + visit) % 2], SEG_SHAPES[shape]
    else:
        menu = PLAIN_SETTINGS + (("wide_blocks",) * 2 if u == 16 else ())
        setting, Fs = menu[(seed % T + 3 * visit) % len(menu)], SEG_SHAPES[shape]
    F = int(Fs[int(rng.integers(0, len(Fs)))])
    n_src = int(rng.integers(2, 300))
    rect = bool(((seed % T) // 2 + (seed % T) // 4 + visit) % 2)      # alternates within every (shape, setting) family
    if setting == "wide_blocks":
        rect = bool((seed % T + visit) % 2)
    n_dst = (1 if rng.random() < 0.2 else int(rng.integers(1, n_src))) if rect else n_src
    dense = u == 16 and setting not in ("wide_blocks", "spans", "track_spans")     # E >= 32 n_dst: the hint allows column blocks
    if dense:
        n_dst = min(n_dst, 24)
        n_src = max(n_dst, min(n_src, 64)) if not rect else n_src
        e = 32 * n_dst + int(rng.integers(0, 200))
    else:
        e = 0 if (rng.random() < 0.06 and not weighted) else int(rng.integers(1, 3000 if F <= 512 else 1200))
    ei = _graph(rng, n_dst, n_src, e, spare_sources=n_dst < n_src)
    hub = None
    if setting in ("hub_order", "hub_noorder") or (setting == "split" and visit % 2 == 1):
        hub = (int(rng.choice([8, 32, 100])), int(rng.choice([8, 16, 64])))
        r0, m = int(rng.integers(0, n_dst)), hub[0] + int(rng.integers(1, 3 * hub[0]))    # one destination far past the threshold
        ei = np.concatenate([ei, np.stack([np.full(m, r0, np.int32), rng.integers(0, n_src, m).astype(np.int32)])], 1)
    # leading-dimension pads / column offsets that keep the target's vector width: multiples of VEC floats, odd ones at VEC = 1
    unit = {1: [1, 2, 3, 5], 2: [2, 6], 4: [4, 8]}[vec]
    d = dict(seed=seed, target=tgt, setting=setting, F=F, n_src=n_src, n_dst=n_dst, ei=ei, hub=hub, rect=n_dst < n_src,
             op=2 if is_max else int(rng.integers(0, 2)), weighted=weighted, row_order=setting != "hub_noorder")
    d["pad_x"] = int(rng.choice(unit)) if setting == "strided_x" else 0
    d["out_off"], d["out_pad"] = (int(rng.choice(unit)), int(rng.choice(unit))) if setting == "out_block" else (0, 0)
    if u == 16 and d["pad_x"]:
        d["pad_x"] = 32                              # column blocks need whole 128-byte lines between rows
    epi = not track
    d["self"] = bool(epi and rng.random() < 0.5)
    d["bias"] = bool(epi and rng.random() < 0.4)
    d["add_x"] = bool(epi and rng.random() < 0.3)
    d["relu"] = bool(epi and rng.random() < 0.5)
    d["k1"] = int(rng.choice([2, 3, 4])) if setting in ("spans", "track_spans") else 0
    d["count_extra"] = bool(d["op"] == 1 and setting in ("hub_order", "hub_noorder", "plain") and rng.random() < 0.7)
    d["n_run"] = int(rng.integers(1, n_dst + 1)) if setting == "n_dst" else n_dst
    d["wide_blocks"] = 1 if setting == "wide_blocks" else (-1 if (u == 0 and F >= 128 and F % 32 == 0) else None)
    d["quant"] = bool(is_max and rng.random() < 0.6)     # quantised features: exact ties between different edges
    if u == 16 and d["wide_blocks"] is None and _hint(d) < 0:
        d["wide_blocks"] = 1                             # the policy says one burst per row here: the column blocks are forced
    return d


def _hint(d):
    """Mirror of plan.wide_blocks_hint for the seed's primary launch (the census holds it to the function itself)."""
    spans = d["setting"] in ("spans", "track_spans")
    ldx = d["F"] + d["pad_x"]
    hub_d = bool(_hubs(d)[0] and not spans and d["setting"] != "track" and d["n_run"] == d["n_dst"])
    if spans or (not hub_d and d["ei"].shape[1] < 32 * max(d["n_run"], 1)):
        return -1
    return -1 if (hub_d and not (ldx >= 128 and ldx & (ldx - 1) == 0)) else 0


def segment_primary(d, hint):
    """(mirror arguments, has hub lists) of the seed's primary launch for made-up, allocation-aligned pointers; `hint` =
    plan.wide_blocks_hint."""
    F, s = d["F"], d["setting"]
    spans = s in ("spans", "track_spans")
    ldx = F + d["pad_x"]
    ldo = F + d["out_off"] + d["out_pad"]
    hub_d = bool(_hubs(d)[0] and not spans and s != "track" and d["n_run"] == d["n_dst"])
    split = s == "split"
    if split:
        ldx = (F // 32) * 32
    wb = d["wide_blocks"]
    if wb is None:
        wb = hint(spans, hub_d, ldx, d["ei"].shape[1], d["n_run"])
        assert split or wb == _hint(d)
    kw = dict(F=F, ldx=ldx, ldo=ldo, x_ptr=1 << 30, out_ptr=(2 << 30) + 4 * d["out_off"], is_max=d["op"] == 2,
              weighted=d["weighted"], add=(F + d["pad_x"], 1 << 30) if d["add_x"] else None,
              bias_ptr=(3 << 30) if d["bias"] else None, split=split, track=s in ("track", "track_spans"), wide_blocks=wb)
    if spans and not kw["track"]:      # the epilogue operands travel with the LAST launch only; the first one is witnessed
        kw["add"], kw["bias_ptr"] = None, None
    return kw, hub_d


def draw_gemm(seed):
    """One seed of the GEMM sweep: built for GEMM_ROUTES[seed % R]; the operand layouts (lda, ldb, ldc, column offsets into
    wider A / B / C, bias, act, act_cols) are drawn on top, within what keeps the route."""
    rng = _rng(12000, seed)
    R = len(GEMM_ROUTES)
    route, visit = GEMM_ROUTES[seed % R], seed // R
    pick = lambda xs: int(xs[int(rng.integers(0, len(xs)))])      # noqa: E731
    tall = lambda: int(rng.integers(32768, 34000))                # noqa: E731
    a_aligned = True                                               # A rows 16-byte aligned with lda % 4 == 0
    if route.startswith("rows"):
        tn = int(route[4:])
        M, N = tall(), int(rng.integers(max(2, 32 * tn - 31), 32 * tn + 1))
        K = pick([k for k in (32, 36, 64, 100, 128, 152, 256, 300) if 4 * k * (32 * tn + 8) <= 160 * 1024])
    elif route == "claimed":
        M, K, N = (1 << 18) + int(rng.integers(0, 70)), pick([32, 36]), pick([32, 64, 100])
    elif route.startswith("skinny"):
        nt = int(route[6:])
        M, N = tall(), int(rng.integers(max(2, 16 * nt - 15), 16 * nt + 1))
        K = pick([65, 101, 130, 601]) if visit % 3 == 0 else pick([64, 100, 256, 600])
        a_aligned = visit % 3 == 0
    elif route == "slices":
        N = pick([256, 384, 512])
        M, K = tall(), pick([160, 200, 256, 300] if N == 256 else [32, 64, 100, 160, 256, 300])
    elif route == "remainder":
        M, K, N = int(rng.integers(4096, 6000)), pick([256, 300, 400]), pick([130, 160, 192, 260, 320])
    elif route == "splitk":
        M, K, N = int(rng.integers(1, 1500)), pick([512, 602, 1433]), pick([7, 16, 40, 64, 100, 256])
    elif route == "ahead":
        M, K, N = int(rng.integers(1000, 4000)), pick([256, 300, 500]), pick([65, 100, 128, 200])
    else:
        N = pick({"g32": [2, 7, 16, 32], "g64": [33, 40, 64], "g128": [65, 100, 128, 200, 300]}[route])
        M, K = int(rng.integers(1, 3000)), pick([1, 3, 16, 36, 60, 100, 200])
    d = dict(seed=seed, route=route, M=M, K=K, N=N)
    needs_rows = route.startswith("rows") or route in ("claimed", "slices")
    if needs_rows or (route.startswith("skinny") and a_aligned):
        d["oa"], d["pad_a"] = pick([0, 4]), pick([0, 4, 8])
        d["pad_a"] += d["oa"] + ((-(K + d["pad_a"] + d["oa"])) % 4 if needs_rows else 0)
    elif route.startswith("skinny"):
        # K % 4 == 0 here: keep the row kernel out through a misaligned first row (visit 1) or an odd leading dimension (visit 2)
        d["oa"] = pick([1, 2, 3]) if visit % 3 == 1 else 0
        d["pad_a"] = d["oa"] + (pick([0, 4]) if visit % 3 == 1 else pick([1, 3, 5]))
        if visit % 3 == 2 and (K + d["pad_a"]) % 4 == 0:
            d["pad_a"] += 1
    else:
        d["oa"] = pick([0, 0, 1, 2, 3, 4])
        d["pad_a"] = d["oa"] + pick([0, 0, 1, 3, 4])
    d["ob"] = pick([0, 0, 1, 2, 3, 4])
    d["pad_b"] = d["ob"] + pick([0, 0, 1, 2, 4])
    if visit % 3 == 1:       # every route once with B on 16-byte rows (the row kernel's 16-byte staging path) ...
        d["ob"] = pick([0, 4])
        d["pad_b"] = d["ob"] + (-(N + d["ob"])) % 4
    elif visit % 3 == 2:     # ... and once off them (dword staging)
        d["ob"] = pick([1, 2, 3])
        d["pad_b"] = d["ob"] + pick([0, 1, 4])
    # first visit of every route: C off the 16-byte boundary inside a wider buffer, ReLU on a strict sub-range of the columns
    d["oc"] = pick([1, 2, 3]) if visit % 3 == 0 else pick([0, 0, 1, 4])
    d["pad_c"] = d["oc"] + (pick([0, 1, 2]) if visit % 3 == 0 else pick([0, 0, 3, 4]))
    d["bias"] = bool(rng.random() < 0.6)
    d["act"] = 1 if visit % 3 == 0 else int(rng.integers(0, 2))
    cols = [int(rng.integers(1, N)), 1, N - 1, min(N - 1, 128), min(N - 1, 100), max(1, N - N % 128), max(1, N - 3)]
    d["act_cols"] = pick(cols) if (visit % 3 == 0 or rng.random() < 0.5) else pick([0, N])
    d["workspace"] = route != "g128" or visit % 2 == 0
    return d


def draw_verified(seed):
    """The verified-layout setting: a table the plan-level entry promotes on its second sighting (widths SplitRows takes once
    the size gate is lowered), no hub rows (a promoted table is never served on a plan with hub lists)."""
    from test_gpu_fuzz_backward import _cap
    rng = _rng(13000, seed)
    F = int(rng.choice([36, 60, 68, 100, 124]))
    n_src = int(rng.integers(2, 300))
    n_dst = n_src if seed % 2 == 0 else int(rng.integers(1, n_src))
    ei = _cap(_graph(rng, n_dst, n_src, int(rng.integers(1, 3000)), spare_sources=n_dst < n_src), 0, 100)
    return dict(seed=seed, F=F, n_src=n_src, n_dst=n_dst, ei=ei, hub=None, op=(seed // 2) % 3, weighted=bool(seed % 4 < 2),
                self=bool(seed % 8 < 4), bias=bool(rng.random() < 0.5), relu=bool(rng.random() < 0.5))


def verified_name(d):
    """Mirror of tfgx_segment_reduce_describe on the verified route (16-byte aligned table, F <= 128: VEC = 4, CH = 1)."""
    lanes = d["F"] // 4
    g = next(g for g in (4, 8, 16, 32, 64) if lanes <= g)
    fused = d["self"] and d["n_src"] == d["n_dst"]
    return "{}seg_reduce_verify_kernel<4, {}, 1, {}, {}, 0> + seg_reduce_repair_kernel".format(
        "" if fused else "split_rows_compare_kernel + ", g, "true" if d["op"] == 2 else "false", "true" if d["weighted"] else "false")


def draw_gat_forward(seed):
    """One seed of the GAT forward sweep: the setting cycles with the seed, the epilogue / side-output options with seed // 6."""
    rng = _rng(14000, seed)
    setting, visit = GAT_SETTINGS[seed % len(GAT_SETTINGS)], seed // len(GAT_SETTINGS)
    H = int(rng.choice([1, 2, 4, 8]))
    d_ = int(rng.choice([1, 2, 3, 4, 8, 16, 5]))
    dv = int(rng.choice([1, 2, 4, 8, 16, 6, 32]))
    n_src = int(rng.integers(2, 300))
    rect = bool((visit // 2 + seed % len(GAT_SETTINGS)) % 2)
    n_dst = int(rng.integers(1, n_src)) if rect else n_src
    hub = None
    if setting.startswith("blocks"):               # dense, near-regular graph: no hub, no skewed walk order
        e = n_dst * int(rng.integers(8, 40))
        ei = np.stack([rng.integers(0, n_dst, e), rng.integers(0, n_src, e)]).astype(np.int32)
    else:
        ei = _graph(rng, n_dst, n_src, int(rng.integers(0, 3000)), spare_sources=rect)
    if setting == "hub":                           # a destination far past the threshold
        hub = (int(rng.choice([4, 8, 32])), int(rng.choice([4, 8, 16])))
        r0, m = int(rng.integers(0, n_dst)), 2 * hub[0] + int(rng.integers(1, 40))
        ei = np.concatenate([ei, np.stack([np.full(m, r0, np.int32), rng.integers(0, n_src, m).astype(np.int32)])], 1)
    return dict(seed=seed, setting=setting, H=H, d=d_, dv=dv, n_src=n_src, n_dst=n_dst, ei=ei, hub=hub, rect=rect,
                source_blocks=int(setting[6:]) if setting.startswith("blocks") else None,
                rate=float(rng.uniform(0.1, 0.8)) if setting == "dropout" else 0.0, drop_seed=int(rng.integers(1, 1 << 62)),
                bias=bool(visit % 2 == 0 or rng.random() < 0.3), relu=bool(visit % 3 == 0 or rng.random() < 0.3),
                self_loop=bool(visit % 3 != 1), scale_d=int(rng.choice([1, 2, 3, 7])) if visit % 2 == 1 else None,
                stats=bool(visit % 3 != 2))


def gat_forward_route(g):
    """Mirror of nn.conv.gat.gat_attention's dispatch: (chained source-block launches, hub lists attached, walk order attached)."""
    E = g["ei"].shape[1]
    indeg, _ = _degrees(g["ei"], g["n_dst"], g["n_src"])
    hub_d, skew = _hubs(g)[0], _skewed(indeg, E)
    sb = g["source_blocks"] or 1                   # without the override the library's policy says 1 at these sizes
    blocks = sb if (g["rate"] <= 0.0 and not skew and not hub_d and sb >= 2) else 0
    return blocks, bool(hub_d and g["rate"] <= 0.0 and not blocks), bool(skew and not blocks)


def gemm_describe(lib, d, a_ptr, b_ptr, c_ptr, ws_ptr, ws_bytes):
    buf = ctypes.create_string_buffer(200)
    rc = lib.tfgx_gemm_describe(a_ptr, d["K"] + d["pad_a"], b_ptr, d["N"] + d["pad_b"], None, d["act"], d["act_cols"], c_ptr,
                                d["N"] + d["pad_c"], d["M"], d["K"], d["N"], ws_ptr, ws_bytes, buf, 200)
    assert rc == 0, lib.tfgx_last_error()
    return buf.value.decode()


def _desc(d, *drop):
    return " ".join("{}={}".format(k, v) for k, v in d.items() if k not in ("ei",) + drop)


# ------------------------------------------------------------------------------------------------------------- the census (CPU)
def test_default_seeds_reach_every_forward_route():
    """Draws, mirrors and the two host-only describe entry points, no device: every seg_reduce_kernel instantiation that
    launch_vec / launch_cfg can dispatch is reached (and the Python mirror agrees with the library on every default draw);
    every setting meets rectangular and square plans, hub lists and none; every GEMM route is reached, each with ldc > N, with
    a C off the 16-byte boundary and with 0 < act_cols < N."""
    from tf_geometric_amd import _lib as L
    from tf_geometric_amd import plan as P
    lib = L.load_library()
    seen, combos = set(), set()
    for seed in range(N_SEG):
        d = draw_segment(seed)
        kw, hub_d = segment_primary(d, P.wide_blocks_hint)
        name = seg_kernel_name(**kw)
        a = L.ReduceArgs()
        a.F, a.ldx, a.ldo, a.x, a.out, a.op, a.n_dst = kw["F"], kw["ldx"], kw["ldo"], kw["x_ptr"], kw["out_ptr"], d["op"], d["n_run"]
        a.w = (4 << 30) if kw["weighted"] else 0
        if kw["add"] is not None:
            a.ld_add, a.add_x = kw["add"]
        a.bias = kw["bias_ptr"] or 0
        a.wide_blocks = kw["wide_blocks"]
        if kw["split"]:
            a.x_tail, a.ld_tail, a.f_main = 5 << 30, d["F"] % 32, kw["ldx"]
        if kw["track"]:
            a.track, a.ld_track = 6 << 30, d["F"]
        buf = ctypes.create_string_buffer(160)
        assert lib.tfgx_segment_reduce_describe(ctypes.byref(a), buf, 160) == 0
        assert buf.value.decode() == name, "mirror != library: " + _desc(d)
        assert _target_of(name) == d["target"], "draw misses its target {}: {} | {}".format(d["target"], name, _desc(d))
        seen.add(_target_of(name))
        combos.add((d["setting"], d["rect"], hub_d))
        assert d["ei"][0].max(initial=0) < d["n_dst"] and d["ei"][1].max(initial=0) < d["n_src"]
    assert seen == set(SEG_TARGETS), sorted(set(SEG_TARGETS) - seen)
    assert len(SEG_TARGETS) == 4 * 21 + 4 * 3 + 2 * 6
    settings = set(PLAIN_SETTINGS) | {"wide_blocks", "split", "track", "track_spans"}
    assert {c[0] for c in combos} == settings
    for s in settings:
        assert (s, True) in {c[:2] for c in combos} and (s, False) in {c[:2] for c in combos}, s + ": rectangular and square"
    for s in ("plain", "strided_x", "out_block", "split", "wide_blocks"):      # settings that attach hub lists when the plan has hubs
        assert {c[2] for c in combos if c[0] == s} == {True, False}, s + ": with and without hub lists"
    assert all(c[2] for c in combos if c[0] in ("hub_order", "hub_noorder"))
    assert not any(c[2] for c in combos if c[0] in ("spans", "track", "track_spans"))

    for seed in range(N_VERIFY):                      # the verified-layout setting: mirror == library, fused and compare-first
        d = draw_verified(seed)
        a = L.ReduceArgs()
        a.F, a.ldx, a.ldo, a.x, a.out, a.op, a.n_dst = d["F"], (d["F"] // 32) * 32, d["F"], 1 << 30, 2 << 30, d["op"], d["n_dst"]
        a.w = (4 << 30) if d["weighted"] else 0
        a.self_coef = (7 << 30) if d["self"] else 0
        a.x_tail, a.ld_tail, a.f_main, a.verify, a.n_verify = 5 << 30, d["F"] % 32, a.ldx, 1, d["n_src"]
        buf = ctypes.create_string_buffer(160)
        assert lib.tfgx_segment_reduce_describe(ctypes.byref(a), buf, 160) == 0
        assert buf.value.decode() == verified_name(d), _desc(d)
        assert not _hubs(d)[0]
        combos.add(("verify", d["n_dst"] < d["n_src"], d["self"] and d["n_dst"] == d["n_src"]))
    assert {c[1:] for c in combos if c[0] == "verify"} == {(False, True), (False, False), (True, False)}

    gat = set()
    for seed in range(N_GAT):
        g = draw_gat_forward(seed)
        blocks, hub_d, order = gat_forward_route(g)
        assert blocks == (g["source_blocks"] or 0), "blocks draw is not dense / regular enough: " + _desc(g)
        assert hub_d == (g["setting"] == "hub") or g["setting"] in ("plain",), _desc(g)
        assert lib.tfgx_gat_source_block_count(g["n_dst"], g["n_src"], g["ei"].shape[1], g["H"] * g["d"], g["H"] * g["dv"],
                                               6 << 20, 32) == 1
        gat.add((g["setting"], g["rect"]))
        for k in ("bias", "relu", "self_loop", "stats"):
            gat.add((g["setting"], k, g[k]))
        gat.add((g["setting"], "scale_d", g["scale_d"] is not None))
        gat.add(("d fast", g["d"] in (1, 2, 4, 8, 16, 32)))
    for st in GAT_SETTINGS:
        assert (st, True) in gat and (st, False) in gat, st + ": rectangular and square"
        for k in ("bias", "relu", "self_loop", "stats", "scale_d"):
            assert (st, k, True) in gat and (st, k, False) in gat, (st, k)
    assert ("d fast", True) in gat and ("d fast", False) in gat

    marks = {r: set() for r in GEMM_ROUTES}
    for seed in range(N_GEMM):
        d = draw_gemm(seed)
        ws_bytes = lib.tfgx_gemm_workspace_bytes(d["M"], d["K"], d["N"]) if d["workspace"] else 0
        name = gemm_describe(lib, d, (1 << 30) + 4 * d["oa"], (2 << 30) + 4 * d["ob"], (3 << 30) + 4 * d["oc"],
                             (4 << 30) if ws_bytes else None, ws_bytes)
        assert re.match(GEMM_PATTERNS[d["route"]], name), "draw misses its route: {} | {}".format(name, _desc(d))
        assert d["pad_a"] >= d["oa"] and d["pad_b"] >= d["ob"] and d["pad_c"] >= d["oc"] and 0 <= d["act_cols"] <= d["N"]
        m = marks[d["route"]]
        m.update(re.findall(r"bv4|b1", name) if "rows" in name else ["bv4", "b1"])     # the row kernel's two B staging paths
        m.update(["ldc"] * (d["pad_c"] > 0) + ["c_off16"] * (d["oc"] % 4 != 0) + ["act_cols"] * (d["act"] == 1 and 0 < d["act_cols"] < d["N"]))
    for r, m in marks.items():
        assert m == {"ldc", "c_off16", "act_cols", "bv4", "b1"}, (r, m)


# ------------------------------------------------------------------------------------------------------------ segment reduce
def _nan(shape, dtype=torch.float32):
    if dtype == torch.int32:
        return torch.full(shape, 0x7FFFFFFF, dtype=torch.int32, device="cuda")
    return torch.full(shape, float("nan"), dtype=torch.float32, device="cuda")


def _still_nan(t):
    return bool((t.contiguous().view(torch.int32) == _NAN_BITS).all())


def _segment_reference(d, x, w, ei, sc, bias, count, n_rows):
    """(float64 reference for sums | bit-exact float32 reference for MAX, sqrt-bar scale) for rows [0, n_rows)."""
    F = d["F"]
    keep = ei[0] < n_rows
    row, col = ei[0][keep], ei[1][keep]
    msg = x[col].astype(np.float64) * (w[keep][:, None].astype(np.float64) if w is not None else 1.0)
    if d["op"] == 2:
        ref = np.full((n_rows, F), -_FLT_MAX, np.float32)
        np.maximum.at(ref, row, msg.astype(np.float32))
        if sc is not None:
            ref = np.maximum(ref, sc[:n_rows, None] * x[:n_rows])                   # float32 product: one rounding, as the kernel
        if d["add_x"]:
            ref = x[:n_rows] + ref
        if bias is not None:
            ref = ref + bias
        if d["relu"]:
            ref = np.maximum(ref, np.float32(0))
        assert ref.dtype == np.float32
        return ref, 1.0
    ref = np.zeros((n_rows, F))
    np.add.at(ref, row, msg)
    if sc is not None:
        ref += sc[:n_rows, None].astype(np.float64) * x[:n_rows]
    if d["op"] == 1:
        ref /= np.maximum(count[:n_rows], 1)[:, None]
    if d["add_x"]:
        ref = x[:n_rows] + ref
    if bias is not None:
        ref = ref + bias
    if d["relu"]:
        ref = np.maximum(ref, 0)
    return ref, max(1.0, float(np.abs(msg).sum(0).max()) if msg.shape[0] else 1.0)


def _check_values(d, got, ref, scale, what):
    got = got.cpu().numpy()
    if d["op"] == 2:
        same = got.view(np.int32) == ref.view(np.int32)
        if not same.all():
            i = tuple(np.argwhere(~same)[0])
            raise AssertionError("{}: MAX differs in {} elements, first at {}: got {!r} ref {!r}".format(
                what, int((~same).sum()), i, got[i], ref[i]))
    else:
        assert np.isfinite(got).all(), what + ": unwritten elements"
        assert_parity(got, ref.astype(np.float32), tol=1e-5 * scale ** 0.5, what=what)


def _partition(rp, col, n_src, k1):
    """numpy statement of plan.source_blocks(k1): (rpk, permutation of the CSR positions)."""
    n = rp.shape[0] - 1
    per = -(-n_src // k1)
    row = np.repeat(np.arange(n), np.diff(rp))
    blk = col // max(per, 1)
    order = np.lexsort((np.arange(col.shape[0]), blk, row))
    cnt = np.zeros(n * k1 + 1, np.int64)
    np.add.at(cnt, row * k1 + blk + 1, 1)
    return np.cumsum(cnt).astype(np.int32), order


def _track_reference(rp, msg32):
    """tie count << 16 | row-relative position of the first maximal edge, per (row, column); an empty row: 0x0000FFFF."""
    n, F = rp.shape[0] - 1, msg32.shape[1]
    out = np.full((n, F), 0xFFFF, np.int64)
    for r in range(n):
        seg = msg32[rp[r]:rp[r + 1]]
        if seg.shape[0]:
            eq = seg == seg.max(0)
            out[r] = (np.minimum(eq.sum(0), 65535) << 16) | eq.argmax(0)
    return out


@pytest.mark.gpu
def test_track_refuses_every_epilogue_operand(tfg):
    from tf_geometric_amd import plan as P
    L = tfg._lib
    ei = np.array([[0, 1, 2, 2], [1, 2, 0, 1]], np.int32)
    plan = P.CsrPlan.build(L.as_i32(ei), 3, 3)
    x = torch.randn(3, 32, device="cuda")
    pk = _nan((3, 32), torch.int32)
    for kw in (dict(self_coef=torch.ones(3, device="cuda")), dict(bias=torch.ones(32, device="cuda")), dict(add_x=x), dict(act=L.ACT_RELU)):
        with pytest.raises(L.TfgxError, match="track: plain TFGX_MAX launches only"):
            P.segment_reduce(plan, x, L.MAX, track=pk, **kw)
    with pytest.raises(L.TfgxError, match="track: plain TFGX_MAX launches only"):
        P.segment_reduce(plan, x, L.SUM, track=pk)


@pytest.mark.gpu
@pytest.mark.parametrize("seed", range(N_SEG * _SCALE))
def test_fuzz_segment_reduce_forward(tfg, oracle, seed):
    """tfgx_segment_reduce_f32 over its argument surface (see the module docstring for settings, bars and identities)."""
    from tf_geometric_amd import plan as P
    L = tfg._lib
    d = draw_segment(seed)
    what = "fuzz forward seg_reduce " + _desc(d)
    rng = _rng(11500, seed)
    F, n_src, n_dst, ei, s = d["F"], d["n_src"], d["n_dst"], d["ei"], d["setting"]
    E = ei.shape[1]
    x = rng.standard_normal((n_src, F)).astype(np.float32)
    if d["quant"]:
        x = np.round(x * 2) / 2 + np.float32(0)      # (+ 0: no -0.0 — which zero max(+0, -0) returns is not specified)
    w = None
    if d["weighted"]:
        w = (rng.integers(1, 4, size=E) * 0.5).astype(np.float32) if d["quant"] else rng.uniform(-1.5, 1.5, size=E).astype(np.float32)
    sc = rng.uniform(0.1, 1.0, size=n_dst).astype(np.float32) if d["self"] else None
    bias = rng.standard_normal(F).astype(np.float32) if d["bias"] else None
    deg = np.bincount(ei[0], minlength=n_dst)
    count = deg + (rng.integers(0, 4, size=n_dst) if d["count_extra"] else 0)
    old = P.HUB_THRESHOLD, P.HUB_CHUNK, P.USE_ROW_ORDER
    try:
        if d["hub"]:
            P.HUB_THRESHOLD, P.HUB_CHUNK = d["hub"]
        plan = P.CsrPlan.build(L.as_i32(ei), n_dst, n_src)
        spans = s in ("spans", "track_spans")
        # witnesses of the plan-level routes against the backward sweep's mirrors
        indeg, _ = _degrees(ei, n_dst, n_src)
        assert (plan.hub_info() is not None) == _hubs(d)[0], what
        assert (plan.row_order() is not None) == _skewed(indeg, E), what
        xd = L.as_f32(x)
        if d["pad_x"]:
            big = _nan((n_src, F + d["pad_x"]))
            big[:, :F] = xd
            xd = big[:, :F]
        wd = None if w is None else plan.edge_attr_to_csr(w)
        n_run = d["n_run"]
        wide_out = _nan((n_dst, F + d["out_off"] + d["out_pad"]))
        out = wide_out[:, d["out_off"]:d["out_off"] + F]
        epi = dict(self_coef=None if sc is None else L.as_f32(sc), bias=None if bias is None else L.as_f32(bias),
                   add_x=xd if d["add_x"] else None, act=L.ACT_RELU if d["relu"] else L.ACT_NONE)
        cnt_d = L.as_i32(count) if (d["op"] == 1 and (d["count_extra"] or spans)) else None

        def ld_of(t, width):
            return int(t.stride(0)) if t.shape[0] > 1 else max(int(width), 1)

        def launch(xin, op, o, primary=False, **kw):
            """describe == mirror (on the real pointers), then the launch."""
            kw.setdefault("wide_blocks", d["wide_blocks"])
            name = P.segment_reduce(plan, xin, op, out=o, describe=True, **kw)
            x2 = xin.main if isinstance(xin, P.SplitRows) else xin
            explicit = kw.get("row_begin") is not None
            nr = int(kw.get("n_dst", n_dst))
            has_hub = plan.hub_info() is not None and not explicit and kw.get("track") is None and nr == n_dst
            wb = kw["wide_blocks"]
            if wb is None:
                wb = P.wide_blocks_hint(explicit, has_hub, ld_of(x2, x2.shape[1]), E, nr)
            ax = kw.get("add_x")
            exp = seg_kernel_name(F, ld_of(x2, x2.shape[1]), ld_of(o, F), x2.data_ptr(), o.data_ptr(), op == L.MAX,
                                  kw.get("w_csr") is not None and kw["w_csr"].data_ptr() != 0, add=None if ax is None else (ld_of(ax, F), ax.data_ptr()),
                                  bias_ptr=None if kw.get("bias") is None else kw["bias"].data_ptr(),
                                  split=isinstance(xin, P.SplitRows), track=kw.get("track") is not None, wide_blocks=wb)
            assert name == exp, "{}: describe {} != mirror {}".format(what, name, exp)
            if primary:
                assert _target_of(name) == d["target"], "{}: ran {} instead of the target".format(what, name)
            return P.segment_reduce(plan, xin, op, out=o, **kw)

        ref, scale = _segment_reference(d, x, w, ei, sc, bias, count, n_run)
        if s in ("track", "track_spans"):
            rp = plan.row_ptr.cpu().numpy().astype(np.int64)
            col = plan.col.cpu().numpy().astype(np.int64)
            w_csr = None if wd is None else wd.cpu().numpy()
            if s == "track":
                pk = _nan((n_dst, F), torch.int32)
                launch(xd, L.MAX, out, primary=True, w_csr=wd, track=pk)
                msg32 = (x[col].astype(np.float64) * (w_csr[:, None] if w_csr is not None else 1.0)).astype(np.float32)
                tref = _track_reference(rp, msg32)
            else:
                k1 = d["k1"]
                rpk_np, order = _partition(rp, col, n_src, k1)
                rpk_t, col_k = plan.source_blocks(k1)
                assert np.array_equal(rpk_t.cpu().numpy(), rpk_np) and np.array_equal(col_k.cpu().numpy(), col[order]), what
                wk = None if w_csr is None else L.as_f32(w_csr[order])
                one, pk1 = _nan((n_dst, F)), _nan((n_dst, F), torch.int32)
                launch(xd, L.MAX, one, w_csr=wk, track=pk1, row_begin=rpk_t, row_end=rpk_t[k1:], rp_stride=k1, col=col_k)
                pk = _nan((n_dst, F), torch.int32)
                for b in range(k1):
                    launch(xd, L.MAX, out, primary=b == 0, w_csr=wk, track=pk, accumulate=b > 0, row_begin=rpk_t[b:],
                           row_end=rpk_t[b + 1:], rp_stride=k1, col=col_k, track_row_begin=rpk_t)
                assert torch.equal(one, out) and torch.equal(pk1, pk), what + ": span by span != whole row"
                msg32 = (x[col[order]].astype(np.float64) * (w_csr[order][:, None] if w_csr is not None else 1.0)).astype(np.float32)
                tref = _track_reference(rpk_np[::k1].astype(np.int64), msg32)
            _check_values(d, out, ref, scale, what)
            got_t = pk.cpu().numpy().astype(np.int64) & 0xFFFFFFFF
            assert np.array_equal(got_t, tref), "{}: packed winner table differs in {} elements".format(what, int((got_t != tref).sum()))
            return
        if s == "spans":
            k1 = d["k1"]
            rp = plan.row_ptr.cpu().numpy().astype(np.int64)
            col = plan.col.cpu().numpy().astype(np.int64)
            rpk_np, order = _partition(rp, col, n_src, k1)
            rpk_t, col_k = plan.source_blocks(k1)
            assert np.array_equal(rpk_t.cpu().numpy(), rpk_np) and np.array_equal(col_k.cpu().numpy(), col[order]), what
            wk = None if wd is None else L.as_f32(wd.cpu().numpy()[order])
            for b in range(k1):          # the way dist/sharded.py chains them: the epilogue and the mean divisor on the last launch
                kw = dict(w_csr=wk, accumulate=b > 0, row_begin=rpk_t[b:], row_end=rpk_t[b + 1:], rp_stride=k1, col=col_k)
                if b == k1 - 1:
                    launch(xd, d["op"], out, mean_count=cnt_d, **dict(kw, **epi))
                else:
                    launch(xd, L.SUM if d["op"] == 1 else d["op"], out, primary=b == 0, **kw)
            _check_values(d, out, ref, scale, what)
            if d["op"] == 2:             # MAX span by span = MAX whole row
                whole = _nan((n_dst, F))
                launch(xd, L.MAX, whole, w_csr=wd, **epi)
                assert torch.equal(whole, out), what + ": span by span != whole row"
            return
        kw = dict(w_csr=wd, mean_count=cnt_d, **epi)
        if s == "n_dst":
            kw["n_dst"] = n_run
        if s == "split":
            dense = launch(xd, d["op"], _nan((n_dst, F)), **kw)
            rows = P.SplitRows.from_dense(xd)
            launch(rows, d["op"], out, primary=True, **kw)
            assert torch.equal(out, dense), what + ": split rows != dense"
            if E:
                rows.with_edge_tail(plan)
                again = launch(rows, d["op"], _nan((n_dst, F)), **kw)
                assert torch.equal(again, dense), what + ": split rows + edge tail != dense"
        else:
            P.USE_ROW_ORDER = d["row_order"]
            launch(xd, d["op"], out, primary=True, **kw)
        _check_values(d, out[:n_run], ref, scale, what)
        if n_run < n_dst:
            assert _still_nan(out[n_run:]), what + ": rows past n_dst were written"
        if d["out_off"] or d["out_pad"]:
            assert _still_nan(wide_out[:, :d["out_off"]]) and _still_nan(wide_out[:, d["out_off"] + F:]), \
                what + ": columns outside the block were written"
        # bit identities: run to run; walk order on = off; column blocks = one burst per row
        first = out.clone()
        if s != "split":
            again = _nan((n_dst, F))
            P.USE_ROW_ORDER = not d["row_order"]
            launch(xd, d["op"], again, **kw)
            assert torch.equal(again[:n_run], first[:n_run]), what + ": row order on != off"
            P.USE_ROW_ORDER = d["row_order"]
            launch(xd, d["op"], out, **kw)
            assert torch.equal(out[:n_run], first[:n_run]), what + ": run to run"
        if s == "wide_blocks":
            burst = launch(xd, d["op"], _nan((n_dst, F)), **dict(kw, wide_blocks=-1))
            assert torch.equal(burst, first), what + ": wide_blocks +1 != -1"
    finally:
        P.HUB_THRESHOLD, P.HUB_CHUNK, P.USE_ROW_ORDER = old


# ---------------------------------------------------------------------------------------------------------------------- GEMM
@pytest.mark.gpu
@pytest.mark.parametrize("seed", range(N_GEMM * _SCALE))
def test_fuzz_gemm_forward(tfg, oracle, seed):
    """tfgx_gemm_bias_act_cols_ws_f32 on every route of its dispatcher with A, B and C as column blocks of wider buffers."""
    L = tfg._lib
    lib = L.require_gpu()
    d = draw_gemm(seed)
    what = "fuzz forward gemm " + _desc(d)
    rng = _rng(12500, seed)
    M, K, N = d["M"], d["K"], d["N"]
    a = rng.standard_normal((M, K)).astype(np.float32)
    b = (rng.standard_normal((K, N)) / np.sqrt(K)).astype(np.float32)
    bias = rng.standard_normal(N).astype(np.float32) if d["bias"] else None
    wa, wb = _nan((M, K + d["pad_a"])), _nan((K, N + d["pad_b"]))
    ad, bd = wa[:, d["oa"]:d["oa"] + K], wb[:, d["ob"]:d["ob"] + N]
    ad.copy_(torch.from_numpy(a))
    bd.copy_(torch.from_numpy(b))
    bias_d = None if bias is None else L.as_f32(bias)
    ws_bytes = lib.tfgx_gemm_workspace_bytes(M, K, N) if d["workspace"] else 0
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device="cuda") if ws_bytes else None

    def run(ws_t, nbytes):
        wc = _nan((M, N + d["pad_c"]))
        cd = wc[:, d["oc"]:d["oc"] + N]
        name = gemm_describe(lib, d, ad.data_ptr(), bd.data_ptr(), cd.data_ptr(), None if ws_t is None else ws_t.data_ptr(), nbytes)
        L.check(lib.tfgx_gemm_bias_act_cols_ws_f32(L.ptr(ad), K + d["pad_a"], L.ptr(bd), N + d["pad_b"], L.ptr(bias_d), d["act"],
                                                   d["act_cols"], L.ptr(cd), N + d["pad_c"], M, K, N, L.ptr(ws_t), nbytes,
                                                   L.stream_ptr()), "tfgx_gemm_bias_act_cols_ws_f32")
        assert _still_nan(wc[:, :d["oc"]]) and _still_nan(wc[:, d["oc"] + N:]), what + ": padding columns of C were written"
        return name, cd

    name, got = run(ws, ws_bytes)
    assert re.match(GEMM_PATTERNS[d["route"]], name), "{}: describe says {}".format(what, name)
    ref = a.astype(np.float64) @ b.astype(np.float64)
    if bias is not None:
        ref = ref + bias
    if d["act"]:
        ref[:, :d["act_cols"]] = np.maximum(ref[:, :d["act_cols"]], 0)
    g = got.cpu().numpy()
    assert np.isfinite(g).all(), what + ": unwritten elements of C"
    assert_parity(g, ref.astype(np.float32), tol=2e-5, what=what + " [" + name + "]")
    name2, again = run(ws, ws_bytes)
    assert name2 == name and torch.equal(again, got), what + ": run to run"
    if d["route"].startswith("rows") or d["route"] in ("claimed", "slices"):
        name3, plain = run(None, 0)         # claimed tiles = fixed tiles: a tile's arithmetic does not depend on who runs it
        assert name3.endswith("fixed") and torch.equal(plain, got), what + ": with != without a workspace"


# ------------------------------------------------------------------------------------------- segment reduce, verified layout
@pytest.mark.gpu
@pytest.mark.parametrize("seed", range(N_VERIFY * _SCALE))
def test_fuzz_segment_reduce_verified_layout(tfg, monkeypatch, seed):
    """Two sightings of an unchanged table promote it; the third call is served from the split + edge-tail layout through
    seg_reduce_verify_kernel and must equal the plain route bit for bit (and the float64 restatement under the sweep's bars)."""
    from tf_geometric_amd import plan as P
    L = tfg._lib
    d = draw_verified(seed)
    d.update(add_x=False, setting="verify")
    what = "fuzz forward verified layout " + _desc(d)
    rng = _rng(13500, seed)
    F, n_src, n_dst, ei = d["F"], d["n_src"], d["n_dst"], d["ei"]
    x = rng.standard_normal((n_src, F)).astype(np.float32)
    w = rng.uniform(-1.5, 1.5, size=ei.shape[1]).astype(np.float32) if d["weighted"] else None
    sc = rng.uniform(0.1, 1.0, size=n_dst).astype(np.float32) if d["self"] else None
    bias = rng.standard_normal(F).astype(np.float32) if d["bias"] else None
    monkeypatch.setattr(P.SplitRows, "wanted", staticmethod(lambda n, F: F % 4 == 0 and 32 < F <= 128 and F % 32 != 0))
    monkeypatch.setattr(P, "AUTO_STATIC_LAYOUT", True)
    stats = dict(P.VERIFIED_STATS)
    plan = P.CsrPlan.build(L.as_i32(ei), n_dst, n_src)
    try:
        assert plan.hub_info() is None, what
        xd = L.as_f32(x)
        kw = dict(w_csr=None if w is None else plan.edge_attr_to_csr(w), self_coef=None if sc is None else L.as_f32(sc),
                  bias=None if bias is None else L.as_f32(bias), act=L.ACT_RELU if d["relu"] else L.ACT_NONE)
        with P.no_auto_promotion():
            plain = P.segment_reduce(plan, xd, d["op"], out=_nan((n_dst, F)), **kw)
            assert "verify" not in P.segment_reduce(plan, xd, d["op"], describe=True, **kw)
        outs = [P.segment_reduce(plan, xd, d["op"], out=_nan((n_dst, F)), **kw) for _ in range(3)]   # sighting, promotion, served
        assert P.VERIFIED_STATS["promotions"] == stats["promotions"] + 1 and P.VERIFIED_STATS["served"] >= stats["served"] + 1, what
        assert P.segment_reduce(plan, xd, d["op"], describe=True, **kw) == verified_name(d), what
        for o in outs:
            assert torch.equal(o, plain), what + ": served != plain route"
        ref, scale = _segment_reference(d, x, w, ei, sc, bias, np.bincount(ei[0], minlength=n_dst), n_dst)
        _check_values(d, plain, ref, scale, what)
        torch.cuda.synchronize()
        assert P.VERIFIED_STATS["demotions"] == stats["demotions"], what
    finally:
        plan.__dict__.pop("_verified", None)           # the layout memo of this plan


# ------------------------------------------------------------------------------------------------------------- GAT forward
@pytest.mark.gpu
@pytest.mark.parametrize("seed", range(N_GAT * _SCALE))
def test_fuzz_gat_forward(tfg, oracle, seed):
    """tfgx_gat_fused_f32 on every route (one pass, hub merge, walk order, chained source blocks, dropout) and epilogue."""
    from f64_layers import gat_attention_f64
    from test_gpu_backward import _keep_mask_host
    from tf_geometric_amd import plan as P
    from tf_geometric_amd.nn.conv import gat as G
    L = tfg._lib
    g = draw_gat_forward(seed)
    what = "fuzz forward gat " + _desc(g)
    rng = _rng(14500, seed)
    H, dd, dv, n_src, n_dst, ei = g["H"], g["d"], g["dv"], g["n_src"], g["n_dst"], g["ei"]
    E = ei.shape[1]
    Q = rng.standard_normal((n_dst, H * dd)).astype(np.float32)
    K = rng.standard_normal((n_src, H * dd)).astype(np.float32)
    V = rng.standard_normal((n_src, H * dv)).astype(np.float32)
    bias = rng.standard_normal(H * dv).astype(np.float32) if g["bias"] else None
    old = P.HUB_THRESHOLD, P.HUB_CHUNK, G.SOURCE_BLOCKS
    try:
        if g["hub"]:
            P.HUB_THRESHOLD, P.HUB_CHUNK = g["hub"]
        G.SOURCE_BLOCKS = g["source_blocks"]
        plan = P.CsrPlan.build(L.as_i32(ei), n_dst, n_src)
        blocks, hub_d, order = gat_forward_route(g)
        indeg, _ = _degrees(ei, n_dst, n_src)
        assert (plan.hub_info() is not None) == _hubs(g)[0] and (plan.row_order() is not None) == _skewed(indeg, E), what
        assert blocks == (g["source_blocks"] or 0), what

        def run():
            st = _nan((n_dst, 2 * H)) if g["stats"] else None
            before = G.SOURCE_BLOCK_STATS["launches"]
            out = G.gat_attention(plan, L.as_f32(Q), L.as_f32(K), L.as_f32(V), H, add_self_loop=g["self_loop"],
                                  bias=None if bias is None else L.as_f32(bias), act=L.ACT_RELU if g["relu"] else L.ACT_NONE,
                                  stats_ml=st, drop_rate=g["rate"], drop_seed=g["drop_seed"], scale_d=g["scale_d"])
            assert G.SOURCE_BLOCK_STATS["launches"] - before == blocks, what + ": source-block launches"
            return out, st

        out, st = run()
        rp, col = plan.row_ptr.cpu().numpy().astype(np.int64), plan.col.cpu().numpy().astype(np.int64)
        keep = _keep_mask_host(g["drop_seed"], (E + n_dst) * H, g["rate"]).reshape(E + n_dst, H) if g["rate"] > 0 else None
        if keep is not None:
            lib = L.require_gpu()
            for item in (0, (E + n_dst) * H - 1, E * H):
                assert bool(keep.reshape(-1)[item]) == bool(lib.tfgx_dropout_keep(g["drop_seed"], int(item), g["rate"])), what
        t64 = lambda a: torch.from_numpy(a.astype(np.float64))      # noqa: E731
        ref, ml = gat_attention_f64(t64(Q), t64(K), t64(V), rp, col, H, keep=keep, rate=g["rate"], add_self_loop=g["self_loop"],
                                    scale_d=g["scale_d"], stats=True)
        ref = ref.numpy()
        if bias is not None:
            ref = ref + bias
        if g["relu"]:
            ref = np.maximum(ref, 0)
        got = out.cpu().numpy()
        assert np.isfinite(got).all(), what
        assert_parity(got, ref.astype(np.float32), tol=2e-5, what=what)
        if st is not None:
            s_np, ml = st.cpu().numpy(), ml.numpy()
            assert np.isfinite(s_np[:, 1::2]).all(), what + ": stats_ml not written"
            assert_parity(s_np[:, 1::2], ml[:, 1::2], tol=2e-5, what=what + " (stats_ml: denominator)")
            has = ml[:, 1::2] > 0                      # rows with at least one term: the row maximum is defined
            assert_parity(np.where(has, s_np[:, 0::2], 0.0), np.where(has, ml[:, 0::2], 0.0), tol=2e-5, what=what + " (stats_ml: maximum)")
        out2, st2 = run()
        assert torch.equal(out, out2) and (st is None or torch.equal(st, st2)), what + ": run to run"
    finally:
        P.HUB_THRESHOLD, P.HUB_CHUNK, G.SOURCE_BLOCKS = old
