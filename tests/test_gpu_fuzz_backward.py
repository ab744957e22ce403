# coding=utf-8
"""Seeded random sweeps of the BACKWARD kernels against float64 torch autograd of a plain index / dense restatement — the
counterpart of test_gpu_fuzz.py.  autograd.py picks a backward route from host-side conditions (width, alignment, leading
dimension, hub lists on the forward or the transposed plan, the max-gradient mode, which inputs want a gradient); the draws
below force every route in turn, and each seed asserts which C-ABI entry points it actually reached (the route witness:
tf_geometric_amd._lib.require_gpu is wrapped for the duration of the call by a proxy that logs every tfgx_* lookup) against
what a small Python mirror of those conditions predicts from the draw.  test_default_seeds_reach_every_route runs the
draws and the mirrors alone (numpy, no device) and asserts that the default seed counts cover every route.

Tolerances follow the conditioning of each sum: assert_parity's bar floor * (1 + |ref|), or — for long sums — 8 * 2^-24 *
sqrt(k) * sum|terms| per element, with sum|terms| from the same float64 restatement run on absolute values.  Max ties are
decided on float32-rounded messages (as the device decides them); a ReLU epilogue's mask is the device output's (> 0), so
that an output within rounding of the kink cannot flip a whole gradient entry — the forward values themselves are checked
against float64 first."""
import contextlib
import os

import numpy as np
import pytest
import torch

# soak runs: TFGX_FUZZ_SCALE=10 multiplies the number of seeds of every sweep
_SCALE = int(os.environ.get("TFGX_FUZZ_SCALE", "1"))
_FLT_MAX = 3.4028234663852886e38
_EPS = 2.0 ** -24

N_AGG, N_MAX, N_FUSED, N_DENSE, N_GAT, N_POOL = 40, 35, 30, 24, 24, 20
MAX_ROUTES = ("packed", "argpos", "push", "pull", "hub_dst", "hub_src", "packed_fallback")
FUSED_KINDS = ("aggregate_project", "sage_wide", "sage_narrow", "linear", "dual_linear")


# ------------------------------------------------------------------------------------------------------------------ draws
def _rng(base, seed):
    return np.random.Generator(np.random.PCG64(base + seed))


def _graph(rng, n_dst, n_src, e, spare_sources=False):
    """test_gpu_fuzz._random_graph on an n_dst x n_src operator: a long row, duplicate edges, self-loops, empty rows;
    spare_sources: the last quarter of the sources is never referenced."""
    hi = max(1, n_src - max(1, n_src // 4)) if spare_sources else n_src
    row = rng.integers(0, n_dst, size=e).astype(np.int32)
    col = rng.integers(0, hi, size=e).astype(np.int32)
    if e > 8 and rng.random() < 0.5:
        k = e // 3
        row[:k] = row[0]
        col[k:k + 4] = col[k]
        v = rng.integers(0, min(n_dst, hi), size=4).astype(np.int32)
        row[k + 4:k + 8] = v
        col[k + 4:k + 8] = v
    if rng.random() < 0.5 and n_dst > 3:
        row[row == 1] = 0
    return np.stack([row, col])


def _cap(ei, axis, k):
    """Keep the first k edges of every destination (axis 0) or source (axis 1)."""
    key = ei[axis]
    order = np.argsort(key, kind="stable")
    sk = key[order]
    first = np.searchsorted(sk, sk, side="left")
    rank = np.empty(key.shape[0], np.int64)
    rank[order] = np.arange(key.shape[0]) - first
    return ei[:, rank < k]


def _thr(T, C, E, n):
    """plan.hub_policy's threshold under the override (T, C) — the module globals are set for the call only."""
    from tf_geometric_amd import plan as P
    old = P.HUB_THRESHOLD, P.HUB_CHUNK
    P.HUB_THRESHOLD, P.HUB_CHUNK = T, C
    try:
        return P.hub_policy(E, n)[0]
    finally:
        P.HUB_THRESHOLD, P.HUB_CHUNK = old


def _degrees(ei, n_dst, n_src):
    return np.bincount(ei[0], minlength=n_dst), np.bincount(ei[1], minlength=n_src)


def _skewed(deg, E):
    """plan.row_order's test: longest row more than 8 * max(E / n, 1) edges."""
    n = deg.shape[0]
    return n > 0 and E > 0 and float(deg.max()) > 8.0 * max(float(E) / n, 1.0)


def _hubs(d):
    """(hub destinations on the plan, hub sources on the transposed plan) for a draw."""
    indeg, outdeg = _degrees(d["ei"], d["n_dst"], d["n_src"])
    E = d["ei"].shape[1]
    T, C = d["hub"] if d["hub"] else (None, None)
    return (int(indeg.max(initial=0)) > _thr(T, C, E, d["n_dst"]),
            int(outdeg.max(initial=0)) > _thr(T, C, E, d["n_src"]))


def draw_aggregate(seed):
    rng = _rng(5000, seed)
    n_src = int(rng.integers(1, 400))
    rect = rng.random() < 0.5 and n_src > 1
    n_dst = (1 if rng.random() < 0.25 else int(rng.integers(1, n_src))) if rect else n_src
    e = int(rng.integers(0, 4000))
    F = int(rng.choice([1, 2, 3, 4, 5, 7, 8, 12, 16, 20, 31, 32, 33, 48, 64, 65, 96, 100, 128, 130, 192, 256, 260, 300,
                        512, 520, 1100]))
    ei = _graph(rng, n_dst, n_src, e, spare_sources=rect)
    d = dict(seed=seed, n_dst=n_dst, n_src=n_src, F=F, ei=ei, mean=bool(rng.random() < 0.4))
    d["weighted"] = bool(rng.random() < 0.6)
    d["self"] = bool(rng.random() < 0.45)
    d["bias"] = bool(rng.random() < 0.4)
    d["relu"] = bool(rng.random() < 0.5)
    d["pad"] = int(rng.integers(1, 5)) if (rng.random() < 0.3 and F > 1) else 0
    d["hub"] = (int(rng.choice([8, 32, 100])), int(rng.choice([8, 16, 64]))) if rng.random() < 0.4 else None
    d["row_order"] = bool(rng.random() < 0.7)
    want = rng.random(4) < 0.55
    d["need"] = dict(x=bool(want[0]), w=bool(want[1] and d["weighted"]), s=bool(want[2] and d["self"]),
                     b=bool(want[3] and d["bias"]))
    if not any(d["need"].values()):
        d["need"]["x"] = True
    return d


def aggregate_labels(d):
    hub_d, hub_s = _hubs(d)
    nd = d["need"]
    lab = {k for k, v in nd.items() if v}
    if d["mean"] and (nd["w"] or nd["s"]) and not nd["x"]:
        lab.add("mean_without_x")
    if d["self"]:
        lab.add("square_self" if d["n_dst"] == d["n_src"] else ("rect_self_n1" if d["n_dst"] == 1 else "rect_self"))
    if d["n_dst"] < d["n_src"]:
        lab.add("unreferenced_sources")
    if hub_s and nd["x"]:
        lab.add("hub_sources")
    if hub_d:
        lab.add("hub_destinations")
    if d["pad"]:
        lab.add("strided")
    if d["relu"]:
        lab.add("relu")
    if d["F"] & (d["F"] - 1) == 0:
        lab.add("pow2")
    return lab


def draw_max(seed):
    rng = _rng(6000, seed)
    route = MAX_ROUTES[seed % len(MAX_ROUTES)]
    hubby = route in ("hub_dst", "hub_src", "packed_fallback")
    T = int(rng.choice([8, 16, 32])) if hubby else None
    C = int(rng.choice([4, 8, 16])) if hubby else None
    trackable = [32, 36, 48, 64, 100, 128, 132, 192, 256]
    F = int(rng.choice({"packed": trackable, "packed_fallback": trackable,
                        "argpos": [4, 8, 12, 16, 20, 28, 260, 300, 520, 1100],
                        "push": [4, 8, 16, 32, 64, 100, 128, 260],
                        "pull": [1, 2, 3, 4, 5, 7, 12, 31, 33, 64, 65, 100, 130],
                        "hub_dst": [1, 3, 4, 8, 12, 32, 64, 100, 130, 256],
                        "hub_src": [3, 4, 5, 8, 12, 16, 20, 28, 260, 300]}[route]))
    n_src = int(rng.integers(2, 300))
    rect = rng.random() < 0.5
    n_dst = (1 if rng.random() < 0.2 else int(rng.integers(1, n_src))) if rect else n_src
    if route in ("hub_src", "packed_fallback"):
        n_dst = max(n_dst, T + 2 + int(rng.integers(0, 8)))
        n_src = max(n_src, n_dst)
        rect = n_dst < n_src
    e = int(rng.integers(0, 3000))
    ei = _graph(rng, n_dst, n_src, e, spare_sources=rect)
    if route == "hub_dst":                        # one destination far past the threshold
        r0 = int(rng.integers(0, n_dst))
        m = T + int(rng.integers(1, 3 * T))
        ei = np.concatenate([ei, np.stack([np.full(m, r0, np.int32), rng.integers(0, n_src, m).astype(np.int32)])], 1)
    elif route in ("hub_src", "packed_fallback"):  # one source far past the threshold, every destination within it
        ei = _cap(ei, 0, T - 1)
        s = int(rng.integers(0, n_src))
        rows = rng.choice(n_dst, size=min(n_dst, T + 1 + int(rng.integers(0, T))), replace=False).astype(np.int32)
        ei = np.concatenate([ei, np.stack([rows, np.full(rows.shape[0], s, np.int32)])], 1)
    else:                                         # the default policy's threshold is >= 128: no hub on either side
        ei = _cap(_cap(ei, 0, 128), 1, 128)
    d = dict(seed=seed, route=route, n_dst=n_dst, n_src=n_src, F=F, ei=ei, hub=(T, C) if hubby else None)
    d["mode"] = {"push": "push", "pull": "pull"}.get(route, "mask")
    d["pad"] = int(rng.choice([1, 2, 3, 4, 8])) if (route in ("pull", "hub_dst") and rng.random() < 0.4) else 0
    d["weighted"] = bool((seed // len(MAX_ROUTES)) % 4 != 3)
    d["quant_w"] = bool(rng.random() < 0.5)
    d["relu_x"] = bool(rng.random() < 0.5)
    return d


def max_route(d):
    """Mirror of _AggregateMax's dispatch for a draw whose x is a fresh torch allocation (16- and 128-byte aligned) with
    leading dimension F + pad: (route, forward tfgx_segment_max_* entry points, backward ones, hub dst, hub src)."""
    F, ldx, E, n_dst = d["F"], d["F"] + d["pad"], d["ei"].shape[1], d["n_dst"]
    hub_d, hub_s = _hubs(d)
    T, C = d["hub"] if d["hub"] else (None, None)
    wide = F % 32 == 0 and ldx % 32 == 0 and E >= 32 * max(n_dst, 1)
    track = (F % 4 == 0 and F >= 32 and (F <= 256 or wide) and ldx % 4 == 0 and not hub_d
             and _thr(T, C, E, n_dst) < 65536)
    mode = d["mode"]
    if mode == "mask" and track:
        fwd = "packed"
    elif not hub_d:
        fwd = "arg" if (mode in ("mask", "push") and F % 4 == 0 and ldx % 4 == 0) else "count"
    else:
        fwd = "hub"
    aligned = fwd in ("packed", "arg") and not hub_s
    if aligned and fwd == "packed":
        bwd = "mask_phases"
    elif aligned and mode == "mask":
        bwd = "mask"
    elif aligned:
        bwd = "push"
    else:
        bwd = "pull"
    if fwd == "hub":
        route = "hub_dst"
    elif fwd == "packed":
        route = "packed" if bwd == "mask_phases" else "packed_fallback"
    elif hub_s:
        route = "hub_src"
    else:
        route = {"mask": "argpos", "push": "push", "pull": "pull"}[bwd]
    pre = "tfgx_segment_max_"
    f_names = {"packed": set(), "arg": {pre + "with_arg_f32"}, "count": {pre + "with_count_f32"}, "hub": set()}[fwd]
    b_names = {"mask_phases": {pre + "backward_mask_phases_f32", pre + "backward_mask_workspace_bytes"},
               "mask": {pre + "backward_mask_f32", pre + "backward_mask_workspace_bytes"},
               "push": {pre + "backward_push_f32"}, "pull": {pre + "backward_hub_f32"}}[bwd]
    if fwd == "hub":
        b_names = b_names | {pre + "count_hub_f32"}
    if d["weighted"]:
        b_names = b_names | {pre + "backward_w_f32"}
    return route, f_names, b_names, hub_d, hub_s


def draw_fused(seed):
    rng = _rng(7000, seed)
    kind = FUSED_KINDS[seed % len(FUSED_KINDS)]
    n = int(rng.integers(1, 1500))
    e = int(rng.integers(0, 20000))
    if kind in ("aggregate_project", "sage_wide"):
        F = 4 * int(rng.integers(1, 33))
        units = int(rng.choice([1, 7, 16, 40, 64, 65, 100, 128, 129, 192, 200, 256]))
    else:
        F = int(rng.choice([1, 3, 4, 16, 17, 32, 48, 64, 100, 128, 200, 300]))
        units = int(rng.choice([1, 7, 16, 40, 64, 65, 100, 128, 200]))
    mean = bool(rng.random() < 0.4)
    d = dict(seed=seed, kind=kind, n=n, F=F, units=units, ei=_graph(rng, n, n, e), mean=mean,
             bias=bool(rng.random() < 0.6), relu=bool(rng.random() < 0.7), weighted=bool(rng.random() < 0.5),
             self=bool(kind == "aggregate_project" and not mean and rng.random() < 0.5))
    d["units2"] = int(rng.choice([1, 8, 16, 33, 64])) if kind in ("sage_wide", "sage_narrow", "dual_linear") else 0
    d["F2"] = int(rng.choice([3, 16, 20, 64])) if kind == "dual_linear" else 0
    want = rng.random(5) < 0.5
    # x, the first kernel, the second kernel, dual_linear's second input r, the bias.  Layer 0 (x without a gradient)
    # on about half of the seeds, so that the gated reductions run
    d["need"] = dict(x=bool(want[0]), k=bool(want[1]), k2=bool(want[2] and d["units2"]),
                     r=bool(want[3] and kind == "dual_linear"), b=bool(want[4] and d["bias"]))
    if not any(d["need"].values()):
        d["need"]["k"] = True
    return d


def fused_gated(d, flag):
    """Mirror of the gating condition of each autograd.Function for one value of its module flag."""
    nd = d["need"]
    if not d["relu"] or not flag:
        return False
    if d["kind"] == "aggregate_project":
        return nd["k"] and not nd["x"]
    if d["kind"] == "sage_wide":
        return nd["k2"] and not nd["x"]
    if d["kind"] == "linear":
        return not nd["x"]
    if d["kind"] == "dual_linear":
        return not nd["x"] and not nd["r"]
    return False


def draw_dense(seed):
    rng = _rng(8000, seed)
    M = {0: 100003, 1: int(rng.integers(90000, 100000)), 2: 0, 3: 1}.get(seed, int(rng.integers(2, 5000)))
    big = M > 50000
    Ka = int(rng.choice([16, 36, 64, 100, 128] if big else [1, 3, 7, 16, 17, 32, 48, 64, 100, 128, 256, 602]))
    N = int(rng.choice([16, 41, 64, 128] if big else [1, 7, 16, 40, 47, 48, 64, 65, 100, 128, 200, 256]))
    ld = N + int(rng.choice([0, 1, 2, 3, 4, 5, 8, 13]))
    c0 = int(rng.integers(0, ld - N + 1))
    return dict(seed=seed, M=M, Ka=Ka, N=N, ld=ld, c0=c0, bias=bool(seed % 2 == 0 or rng.random() < 0.3),
                gated=bool(seed % 4 in (1, 2) or rng.random() < 0.3), xpad=int(rng.choice([0, 0, 3, 4])))


def draw_gat(seed):
    rng = _rng(9000, seed)
    H = int(rng.choice([1, 2, 4, 8]))
    d_ = 1 if seed % 4 == 0 else int(rng.choice([1, 2, 3, 4, 8, 16, 5]))
    dv = int(rng.choice([1, 2, 4, 8, 16, 6, 32]))
    setting = ["plain", "hub", "blocks", "plain"][(seed // 4) % 4] if seed % 4 else ["plain", "blocks"][(seed // 4) % 2]
    n_src = int(rng.integers(1, 300))
    rect = rng.random() < 0.5 and n_src > 1
    n_dst = int(rng.integers(1, n_src)) if rect else n_src
    if setting == "blocks":                        # dense, near-regular graph: no hub, no skewed walk order
        e = n_dst * int(rng.integers(8, 40))
        ei = np.stack([rng.integers(0, n_dst, e), rng.integers(0, n_src, e)]).astype(np.int32)
        if d_ not in (1, 2, 4, 8, 16, 32):
            d_ = 4
        if dv % 4:
            dv = 8
    else:
        ei = _graph(rng, n_dst, n_src, int(rng.integers(0, 3000)), spare_sources=rect)
    hub = (int(rng.choice([4, 8, 32])), int(rng.choice([4, 8, 16]))) if setting == "hub" else None
    if hub:                                        # a source far past the threshold: the source pass walks it chunk-wise
        m = 2 * hub[0] + int(rng.integers(1, 40))
        ei = np.concatenate([ei, np.stack([rng.integers(0, n_dst, m).astype(np.int32),
                                           np.full(m, int(rng.integers(0, n_src)), np.int32)])], 1)
    return dict(seed=seed, H=H, d=d_, dv=dv, n_dst=n_dst, n_src=n_src, ei=ei, setting=setting, hub=hub,
                source_blocks=int(rng.choice([2, 3, 5])) if setting == "blocks" else None,
                destination_blocks=(int(rng.choice([2, 4])) if rng.random() < 0.5 else None) if setting == "blocks" else None,
                query_sums=bool(rng.random() < 0.6) if d_ == 1 else True)


def gat_route(g):
    """Mirror of _GatAttention.backward's dispatch: (query sums, destination-pass launches, source-pass launches,
    hub sources)."""
    E = g["ei"].shape[1]
    indeg, outdeg = _degrees(g["ei"], g["n_dst"], g["n_src"])
    hub_d, hub_s = _hubs(g)
    d, dv, H = g["d"], g["dv"], g["H"]
    qs = g["query_sums"] and d == 1 and dv % 4 == 0 and g["n_dst"] > 0 and not hub_d
    ok = (not hub_d and not _skewed(indeg, E) and not _skewed(outdeg, E) and d in (1, 2, 4, 8, 16, 32) and dv % 4 == 0
          and dv // 4 <= 64 and ((dv // 4) & (dv // 4 - 1) == 0 or H == 1))
    sb = max(g["source_blocks"], 1) if g["source_blocks"] is not None else 1   # the library's policy: 1 at these sizes
    kb_d = sb if ok else 1
    kb_s = sb if (ok and not hub_s) else 1
    if kb_s >= 2 and g["destination_blocks"] is not None:
        kb_s = max(int(g["destination_blocks"]), 1)
    return qs, (0 if qs else kb_d), kb_s, hub_s


def pool_chunk(F_in, Fp):
    """Edges per LDS chunk of tfgx_pool_mlp_max_wgrad_f32: min(kPoolChunk, kPoolSlots * Fp / (F_in / 4))."""
    return min(96, (4 * Fp) // (F_in // 4))


def draw_pool(seed):
    rng = _rng(10000, seed)
    F_in = 4 * int(rng.integers(1, 32))
    Fp = int(rng.choice([128, 256, 512]))
    n = 1 if seed % 5 == 0 else int(rng.integers(2, 40))
    c = pool_chunk(F_in, Fp)
    menu = [0, 1, c - 1, c, c + 1, 2 * c, 2 * c + 1, 3 * c, int(rng.integers(0, 2 * c + 1))]
    deg = rng.choice(menu, size=n)
    last = ["empty", "long", "random"][seed % 3]
    if last == "empty":
        deg[-1] = 0
    elif last == "long":
        deg[-1] = 3 * c + int(rng.integers(1, c + 1))
    if deg.sum() == 0:                              # a plan without edges: tests/test_gpu_regressions.py covers it
        deg[0] = c
    if Fp == 512 and deg.sum() < 32 * n:            # the tracked forward takes 512 columns only on dense plans
        Fp = 256
        c = pool_chunk(F_in, Fp)
    row = np.repeat(np.arange(n, dtype=np.int32), deg)
    col = rng.integers(0, n, size=row.shape[0]).astype(np.int32)
    if row.shape[0] > 8:                            # duplicate edges: exact ties between copies of one edge
        col[1:8:2] = col[0:7:2]
        row[1:8:2] = row[0:7:2]
    perm = rng.permutation(row.shape[0])
    return dict(seed=seed, F_in=F_in, Fp=Fp, n=n, chunk=c, deg=np.bincount(row, minlength=n), last=last,
                ei=np.stack([row[perm], col[perm]]), bias=bool(rng.random() < 0.6), quant=bool(rng.random() < 0.75))


# ---------------------------------------------------------------------------------------------------------------- helpers
def _what(d, *keys):
    return " ".join("{}={}".format(k, d[k]) for k in keys)


def _close(got, ref, absref, k, what, floor=1e-5):
    """|got - ref| <= max(floor * (1 + |ref|), 8 * 2^-24 * sqrt(k) * sum|terms|) per element; a non-finite element (an
    unwritten row of a poisoned output) always fails."""
    got = got.detach().double().cpu().numpy() if isinstance(got, torch.Tensor) else np.asarray(got, np.float64)
    ref, absref = np.asarray(ref, np.float64), np.asarray(absref, np.float64)
    assert got.shape == ref.shape, "{}: shape {} vs {}".format(what, got.shape, ref.shape)
    assert np.isfinite(got).all(), "{}: {} non-finite elements (unwritten rows?), first at {}".format(
        what, int((~np.isfinite(got)).sum()), np.argwhere(~np.isfinite(got))[:4].tolist())
    bound = np.maximum(floor * (1.0 + np.abs(ref)), 8.0 * _EPS * np.sqrt(max(k, 1)) * absref)
    bad = np.abs(got - ref) > bound
    if bad.any():
        i = tuple(np.argwhere(bad)[0])
        raise AssertionError("{}: {} of {} elements off; first at {}: got {!r} ref {!r} bound {:.3e}".format(
            what, int(bad.sum()), bad.size, i, float(got[i]), float(ref[i]), float(bound[i])))


def _f64(fn, inputs, gout, absolute=False):
    """float64 autograd of fn(**leaves) with output gradient gout -> ({name: grad}, output).  absolute=True runs the same
    restatement on |inputs| and |gout|: for the functions here (linear in each input once masks and tie shares are fixed)
    its gradients are the sums of |terms| of the gradients' sums."""
    leaves = {}
    for k, v in inputs.items():
        t = torch.as_tensor(v, dtype=torch.float64)
        leaves[k] = (t.abs() if absolute else t).clone().requires_grad_(True)
    out = fn(**leaves)
    go = torch.as_tensor(gout, dtype=torch.float64)
    out.backward(go.abs() if absolute else go)
    return {k: v.grad for k, v in leaves.items()}, out.detach()


def _poison(*shapes):
    """Fill blocks of torch's caching allocator with NaN and free them, so that a gradient buffer (torch.empty) that a route
    leaves partly unwritten shows NaN instead of a stale zero.  A heuristic, not a guarantee: whether the allocator hands
    exactly these blocks to the backward's outputs depends on what else is allocated first."""
    bufs = [torch.full(tuple(int(v) for v in s), float("nan"), dtype=torch.float32, device="cuda")
            for s in shapes if all(int(v) > 0 for v in s)]
    del bufs


class _Proxy(object):
    def __init__(self, lib, log):
        self._lib, self._log = lib, log

    def __getattr__(self, name):
        if name.startswith("tfgx_"):
            self._log.append(name)
        return getattr(self._lib, name)


@contextlib.contextmanager
def _witness(monkeypatch):
    """Log of every tfgx_* entry point looked up through _lib.require_gpu() while the block runs."""
    from tf_geometric_amd import _lib as L
    log = []
    proxy = _Proxy(L.require_gpu(), log)
    with monkeypatch.context() as m:
        m.setattr(L, "require_gpu", lambda: proxy)
        yield log


@contextlib.contextmanager
def _settings(**kw):
    """Set module globals of plan (P__NAME), autograd (AG__NAME) and nn.conv.gat (G__NAME) for the block."""
    from tf_geometric_amd import plan as P, autograd as AG
    from tf_geometric_amd.nn.conv import gat as G
    mods = dict(P=P, AG=AG, G=G)
    old = []
    try:
        for key, v in kw.items():
            mod, name = key.split("__")
            old.append((mods[mod], name, getattr(mods[mod], name)))
            setattr(mods[mod], name, v)
        yield
    finally:
        for mod, name, v in reversed(old):
            setattr(mod, name, v)


def _csr(plan):
    """(row of every CSR position, col) of a plan as int64 CPU tensors."""
    rp = plan.row_ptr.cpu().numpy().astype(np.int64)
    row = torch.from_numpy(np.repeat(np.arange(plan.n_dst), np.diff(rp)))
    return row, torch.from_numpy(plan.col.cpu().numpy().astype(np.int64))


def _table(x32, pad):
    """x32 on the device; pad > 0: a column view of a wider buffer (leading dimension F + pad)."""
    from tf_geometric_amd import _lib as L
    if not pad:
        return L.as_f32(x32)
    big = torch.zeros((x32.shape[0], x32.shape[1] + pad), device="cuda")
    big[:, :x32.shape[1]] = L.as_f32(x32)
    return big[:, :x32.shape[1]]


def _tie_shares(msg32, out32, row, n_dst, F):
    """TF's unsorted_segment_max gradient: 1 / (number of tied maxima) on every edge that attains its row's maximum —
    decided on the float32 messages — else 0."""
    tie = (msg32 == out32[row]).astype(np.float64)
    cnt = np.zeros((n_dst, F))
    np.add.at(cnt, row, tie)
    return torch.from_numpy(tie / np.maximum(cnt[row], 1.0))


# ---------------------------------------------------------------------------------------------------------------- CPU
def test_default_seeds_reach_every_route():
    """The draws alone, through the dispatch mirrors (numpy, no device): the default seed counts reach every route."""
    routes = set()
    for s in range(N_MAX):
        d = draw_max(s)
        got = max_route(d)[0]
        assert got == d["route"], "max seed {}: drawn for {} but the dispatch takes {}".format(s, d["route"], got)
        routes.add(got)
        if d["weighted"]:
            routes.add("w:" + got)
    assert routes >= set(MAX_ROUTES) | {"w:" + r for r in MAX_ROUTES}, sorted(routes)
    labels = set()
    for s in range(N_AGG):
        labels |= aggregate_labels(draw_aggregate(s))
    assert labels >= {"x", "w", "s", "b", "mean_without_x", "square_self", "rect_self", "rect_self_n1",
                      "unreferenced_sources", "hub_sources", "hub_destinations", "strided", "relu", "pow2"}, sorted(labels)
    fused = set()
    for s in range(N_FUSED):
        d = draw_fused(s)
        fused.add((d["kind"], fused_gated(d, True)))
    assert fused >= ({(k, False) for k in FUSED_KINDS} | {(k, True) for k in FUSED_KINDS if k != "sage_narrow"}), sorted(fused)
    dense = set()
    for s in range(N_DENSE):
        d = draw_dense(s)
        dense |= {("M", min(d["M"], 2) if d["M"] < 50000 else "big"), ("ld%4", d["ld"] % 4 == 0),
                  ("Ka%16", d["Ka"] % 16 == 0), ("N%16", d["N"] % 16 == 0), ("bias", d["bias"]), ("gated", d["gated"])}
    assert dense >= {("M", 0), ("M", 1), ("M", 2), ("M", "big"), ("ld%4", True), ("ld%4", False), ("Ka%16", True),
                     ("Ka%16", False), ("N%16", True), ("N%16", False), ("bias", True), ("bias", False), ("gated", True),
                     ("gated", False)}, sorted(dense, key=str)
    gat = set()
    for s in range(N_GAT):
        g = draw_gat(s)
        qs, nd, ns, hub_s = gat_route(g)
        gat |= {"query_sums"} if qs else set()
        gat |= {"destination_blocks"} if nd >= 2 else set()
        gat |= {"source_pass_blocks"} if ns >= 2 else set()
        gat |= {"hub_sources"} if hub_s and g["hub"] else set()
        gat |= {"rectangular"} if g["n_dst"] < g["n_src"] else set()
        gat |= {"d1_without_sums"} if g["d"] == 1 and not qs else set()
    assert gat >= {"query_sums", "destination_blocks", "source_pass_blocks", "hub_sources", "rectangular",
                   "d1_without_sums"}, sorted(gat)
    pool = set()
    for s in range(N_POOL):
        p = draw_pool(s)
        c = p["chunk"]
        for v in p["deg"]:
            pool |= {"c-1"} if v == c - 1 else set()
            pool |= {"c"} if v == c else set()
            pool |= {"c+1"} if v == c + 1 else set()
            pool |= {"kc"} if v >= 2 * c and v % c == 0 else set()
        pool |= {"last_empty"} if p["n"] > 1 and p["deg"][-1] == 0 else set()
        pool |= {"last_long"} if p["deg"][-1] > 3 * c else set()
        pool |= {"bias" if p["bias"] else "no_bias", "Fp{}".format(p["Fp"])}
        pool |= {"n1"} if p["n"] == 1 else set()
    assert pool >= {"c-1", "c", "c+1", "kc", "last_empty", "last_long", "bias", "no_bias", "n1", "Fp128", "Fp256",
                    "Fp512"}, sorted(pool)


# ---------------------------------------------------------------------------------------------------------------- 1. sum / mean
@pytest.mark.gpu
@pytest.mark.parametrize("seed", range(N_AGG * _SCALE))
def test_fuzz_aggregate_backward(tfg, monkeypatch, seed):
    """_Aggregate (sum / mean): weights, self-loop term (square and n_dst < n_src, n_dst = 1 included), bias and ReLU
    epilogue, strided x, a random subset of {x, w, self_coef, bias} wanting a gradient, forced hub lists, walk order."""
    from tf_geometric_amd import plan as P, autograd as AG
    L = tfg._lib
    d = draw_aggregate(seed)
    rng = _rng(50000, seed)
    n_dst, n_src, F, ei, nd = d["n_dst"], d["n_src"], d["F"], d["ei"], d["need"]
    hub_d, hub_s = _hubs(d)
    what = "fuzz aggregate backward seed {} {} E={} need={} hub={} row_order={} (hub dst={} src={})".format(
        seed, _what(d, "n_dst", "n_src", "F", "mean", "weighted", "self", "bias", "relu", "pad"), ei.shape[1], nd,
        d["hub"], d["row_order"], hub_d, hub_s)
    x32 = rng.standard_normal((n_src, F)).astype(np.float32)
    w32 = rng.uniform(-1.5, 1.5, size=ei.shape[1]).astype(np.float32)
    sc32 = rng.uniform(0.1, 1.0, size=n_dst).astype(np.float32)
    b32 = rng.standard_normal(F).astype(np.float32)
    g32 = rng.standard_normal((n_dst, F)).astype(np.float32)
    T, C = d["hub"] if d["hub"] else (None, None)
    with _settings(P__HUB_THRESHOLD=T, P__HUB_CHUNK=C, P__USE_ROW_ORDER=d["row_order"]):
        plan = P.CsrPlan.build(L.as_i32(ei), n_dst, n_src)
        x = _table(x32, d["pad"]).requires_grad_(nd["x"])
        w = plan.edge_attr_to_csr(L.as_f32(w32)).detach().requires_grad_(nd["w"]) if d["weighted"] else None
        sc = L.as_f32(sc32).requires_grad_(nd["s"]) if d["self"] else None
        b = L.as_f32(b32).requires_grad_(nd["b"]) if d["bias"] else None
        act = L.ACT_RELU if d["relu"] else L.ACT_NONE
        with _witness(monkeypatch) as fwd:
            out = AG.aggregate(plan, x, L.MEAN if d["mean"] else L.SUM, w_csr=w, self_coef=sc, bias=b, act=act)
        _poison((n_src, F), (n_dst, F), (ei.shape[1],), (n_dst,), (F,))
        with _witness(monkeypatch) as bwd:
            out.backward(L.as_f32(g32))
        # the witness: forward launch, transposed pass (its hub lists built on demand), d/dw, d/db, the ReLU mask
        assert fwd.count("tfgx_segment_reduce_f32") == 1, what
        assert fwd.count("tfgx_plan_hub_lists_emit") == int(hub_d), what + " (hub destinations)"
        assert bwd.count("tfgx_segment_reduce_f32") == int(nd["x"]), what + " (transposed pass)"
        assert bwd.count("tfgx_plan_hub_lists_emit") == int(nd["x"] and hub_s), what + " (hub sources)"
        assert ("tfgx_sddmm_hub_f32" in bwd) == nd["w"], what
        assert ("tfgx_column_sum_f32" in bwd) == nd["b"], what
        assert ("tfgx_relu_backward_f32" in bwd) == d["relu"], what
        row, col = _csr(plan)
        wcsr = w.detach().cpu().numpy() if w is not None else None
    mask = (out.detach().cpu() > 0).double() if d["relu"] else None
    cnt = torch.bincount(row, minlength=n_dst).clamp(min=1).double()

    def f(x, w=None, s=None, b=None):
        msg = x[col] * w[:, None] if w is not None else x[col]
        agg = torch.zeros(n_dst, F, dtype=torch.float64).index_add(0, row, msg)
        if s is not None:
            agg = agg + s[:, None] * x[:n_dst]
        if d["mean"]:
            agg = agg / cnt[:, None]
        if b is not None:
            agg = agg + b
        return agg * mask if mask is not None else agg
    ins = dict(x=x32)
    if d["weighted"]:
        ins["w"] = wcsr
    if d["self"]:
        ins["s"] = sc32
    if d["bias"]:
        ins["b"] = b32
    ref, ref_out = _f64(f, ins, g32)
    ab, ab_out = _f64(f, ins, g32, absolute=True)
    indeg, outdeg = _degrees(ei, n_dst, n_src)
    _close(out, ref_out.numpy(), ab_out.numpy(), int(indeg.max(initial=0)) + 2, what + " forward")
    k = {"x": int(outdeg.max(initial=0)) + 2, "w": F, "s": F, "b": n_dst}
    for name, t in (("x", x), ("w", w), ("s", sc), ("b", b)):
        if t is None:
            continue
        if nd[name]:
            _close(t.grad, ref[name].numpy(), ab[name].numpy(), k[name], what + " d/d" + name)
        else:
            assert t.grad is None, what + " d/d" + name + " computed but not wanted"


# ---------------------------------------------------------------------------------------------------------------- 2. max
@pytest.mark.gpu
@pytest.mark.parametrize("seed", range(N_MAX * _SCALE))
def test_fuzz_max_backward(tfg, monkeypatch, seed):
    """_AggregateMax, one route per seed in turn: packed mask, argpos mask, push, pull, hub destinations (count pass), hub
    sources (pull, chunked) and the packed -> pull fall-back; d/dx and d/dw; ties from quantised features, duplicate edges
    and ReLU zero plateaus; negative and inexact weights; rectangular plans with unreferenced sources."""
    from tf_geometric_amd import plan as P, autograd as AG
    L = tfg._lib
    d = draw_max(seed)
    route, f_names, b_names, hub_d, hub_s = max_route(d)
    rng = _rng(60000, seed)
    n_dst, n_src, F, ei = d["n_dst"], d["n_src"], d["F"], d["ei"]
    what = "fuzz max backward seed {} route={} {} E={} hub={} (hub dst={} src={})".format(
        seed, route, _what(d, "n_dst", "n_src", "F", "mode", "pad", "weighted", "quant_w", "relu_x"), ei.shape[1], d["hub"],
        hub_d, hub_s)
    x32 = (np.round(rng.standard_normal((n_src, F)) * 2) / 2).astype(np.float32)       # quantised: exact ties
    if d["relu_x"]:
        x32 = np.maximum(x32, 0).astype(np.float32)                                      # zero plateaus
    if d["quant_w"]:
        w32 = rng.choice(np.float32([-1.0, -0.5, 0.5, 1.0, 2.0]), size=ei.shape[1]).astype(np.float32)
    else:
        w32 = rng.uniform(-1.5, 1.5, size=ei.shape[1]).astype(np.float32)                # inexact products
    g32 = rng.standard_normal((n_dst, F)).astype(np.float32)
    T, C = d["hub"] if d["hub"] else (None, None)

    def run(plan, mode, backward=True):
        with _settings(AG__MAX_GRADIENT_MODE=mode):
            x = _table(x32, d["pad"]).requires_grad_(True)
            w = plan.edge_attr_to_csr(L.as_f32(w32)).detach().requires_grad_(True) if d["weighted"] else None
            with _witness(monkeypatch) as fwd:
                out = AG.aggregate(plan, x, L.MAX, w_csr=w)
            if not backward:
                return out.detach(), None, None, fwd, None
            _poison((n_src, F), (ei.shape[1],))
            with _witness(monkeypatch) as bwd:
                out.backward(L.as_f32(g32))
            return out.detach(), x.grad, (w.grad if w is not None else None), fwd, bwd

    with _settings(P__HUB_THRESHOLD=T, P__HUB_CHUNK=C):
        plan = P.CsrPlan.build(L.as_i32(ei), n_dst, n_src)
        out, gx, gw, fwd, bwd = run(plan, d["mode"])
        assert {s for s in fwd if s.startswith("tfgx_segment_max_")} == f_names, what + " forward {}".format(sorted(set(fwd)))
        assert ("tfgx_segment_reduce_f32" in fwd) == (route in ("packed", "packed_fallback", "hub_dst")), what
        assert {s for s in bwd if s.startswith("tfgx_segment_max_")} == b_names, what + " backward {}".format(sorted(set(bwd)))
        assert ("tfgx_plan_hub_lists_emit" in bwd) == hub_s, what + " (hub sources)"
        # every route's training forward gives the same maxima; the mask routes give the same bits when run again
        for mode in ("mask", "push", "pull"):
            assert torch.equal(run(plan, mode, backward=False)[0], out), what + " forward of mode " + mode
        if route in ("packed", "argpos"):
            _, gx2, gw2, _, _ = run(plan, d["mode"])
            assert torch.equal(gx2.view(torch.int32), gx.view(torch.int32)), what + " d/dx not reproducible"
            assert gw is None or torch.equal(gw2.view(torch.int32), gw.view(torch.int32)), what + " d/dw not reproducible"
        row, col = _csr(plan)
        wcsr = plan.edge_attr_to_csr(L.as_f32(w32)).cpu().numpy() if d["weighted"] else None
    # maxima and ties decided on the float32-rounded messages (as the device decides them), derivatives in float64
    rown, coln = row.numpy(), col.numpy()
    msg32 = (x32[coln] * wcsr[:, None]).astype(np.float32) if wcsr is not None else x32[coln]
    out32 = np.full((n_dst, F), -_FLT_MAX, np.float32)
    np.maximum.at(out32, rown, msg32)
    assert np.array_equal(out.cpu().numpy(), out32), what + " forward maxima (empty rows: -FLT_MAX)"
    coef = _tie_shares(msg32, out32, rown, n_dst, F)

    def f(x, w=None):
        msg = x[col] * w[:, None] if w is not None else x[col]
        return torch.zeros(n_dst, F, dtype=torch.float64).index_add(0, row, msg * coef)
    ins = dict(x=x32, w=wcsr) if wcsr is not None else dict(x=x32)
    ref, _ = _f64(f, ins, g32)
    ab, _ = _f64(f, ins, g32, absolute=True)
    _close(gx, ref["x"].numpy(), ab["x"].numpy(), int(np.bincount(ei[1], minlength=n_src).max(initial=0)) + 1, what + " d/dx")
    if wcsr is not None:
        _close(gw, ref["w"].numpy(), ab["w"].numpy(), F, what + " d/dw")


# ---------------------------------------------------------------------------------------------------------------- 3. fused layers
@pytest.mark.gpu
@pytest.mark.parametrize("seed", range(N_FUSED * _SCALE))
def test_fuzz_fused_layer_backward(tfg, monkeypatch, seed):
    """_AggregateProject / _SageWide with GATED_AGGREGATE_PROJECT on and off, _SageNarrow, _Linear / _DualLinear with
    GATED_WEIGHT_GRADIENTS on and off: gated and un-gated agree with each other and with float64."""
    from tf_geometric_amd import plan as P, autograd as AG
    L = tfg._lib
    d = draw_fused(seed)
    rng = _rng(70000, seed)
    kind, n, F, U, U2, nd = d["kind"], d["n"], d["F"], d["units"], d["units2"], d["need"]
    what = "fuzz fused backward seed {} {} E={} need={}".format(
        seed, _what(d, "kind", "n", "F", "units", "units2", "F2", "mean", "bias", "relu", "weighted", "self"),
        d["ei"].shape[1], nd)
    ei = d["ei"]
    F2 = d["F2"] if kind == "dual_linear" else F
    x32 = rng.standard_normal((n, F)).astype(np.float32)
    k32 = (rng.standard_normal((F, U)) / np.sqrt(F)).astype(np.float32)
    k232 = (rng.standard_normal((F2, U2)) / np.sqrt(F2)).astype(np.float32) if U2 else None
    r32 = rng.standard_normal((n, F2)).astype(np.float32) if kind == "dual_linear" else None
    w32 = rng.uniform(0.2, 1.5, size=ei.shape[1]).astype(np.float32)
    sc32 = rng.uniform(0.1, 1.0, size=n).astype(np.float32)
    width = U + U2
    b32 = (rng.standard_normal(width) * 0.3).astype(np.float32)
    g32 = rng.standard_normal((n, width)).astype(np.float32)
    act = L.ACT_RELU if d["relu"] else L.ACT_NONE
    op = L.MEAN if d["mean"] else L.SUM
    plan = P.CsrPlan.build(L.as_i32(ei), n, n)
    w_csr = plan.edge_attr_to_csr(L.as_f32(w32)) if d["weighted"] else None
    flag = "AG__GATED_WEIGHT_GRADIENTS" if kind in ("linear", "dual_linear") else "AG__GATED_AGGREGATE_PROJECT"

    def run(gated_flag):
        t = dict(x=L.as_f32(x32).requires_grad_(nd["x"]), k=L.as_f32(k32).requires_grad_(nd["k"]))
        if U2:
            t["k2"] = L.as_f32(k232).requires_grad_(nd["k2"])
        if r32 is not None:
            t["r"] = L.as_f32(r32).requires_grad_(nd["r"])
        if d["bias"]:
            t["b"] = L.as_f32(b32).requires_grad_(nd["b"])
        b = t.get("b")
        with _settings(**{flag: gated_flag}):
            if kind == "aggregate_project":
                sc = L.as_f32(sc32) if d["self"] else None
                out = AG.aggregate_project(plan, t["x"], op, t["k"], w_csr=w_csr, self_coef=sc, bias=b, act=act)
                assert out is not None, what + ": the fused launch declined"
            elif kind == "sage_wide":
                out = AG.sage_wide(plan, op, t["x"], t["k"], t["k2"], w_csr=w_csr, bias=b, act=act)
                assert out is not None, what + ": the fused launch declined"
            elif kind == "sage_narrow":
                out = AG.sage_narrow(plan, op, t["x"], t["k"], t["k2"], w_csr=w_csr, bias=b, act=act)
            elif kind == "linear":
                out = AG.linear(t["x"], t["k"], bias=b, act=act)
            else:
                out = AG.dual_linear(t["x"], t["k"], t["r"], t["k2"], bias=b, act=act)
            _poison((n, F), (F, U), (F2, U2), (width,), (n, F2))
            with _witness(monkeypatch) as bwd:
                out.backward(L.as_f32(g32))
        return out.detach(), {kk: v.grad for kk, v in t.items()}, bwd

    out_g, grads_g, log_g = run(True)
    out_u, grads_u, log_u = run(False)
    assert torch.equal(out_g, out_u), what
    for flag_v, log in ((True, log_g), (False, log_u)):
        gated = fused_gated(d, flag_v)
        assert ("tfgx_relu_backward_f32" in log) == (d["relu"] and not gated), what + " flag={} gated={} {}".format(
            flag_v, gated, sorted(set(log)))
    row, col = _csr(plan)
    cnt = torch.bincount(row, minlength=n).clamp(min=1).double()
    wc = torch.from_numpy(w_csr.cpu().numpy()).double() if w_csr is not None else None
    mask = (out_g.cpu() > 0).double() if d["relu"] else None

    def agg(v, s=None):
        msg = v[col] * wc[:, None] if wc is not None else v[col]
        a = torch.zeros(n, v.shape[1], dtype=torch.float64).index_add(0, row, msg)
        if s is not None:
            a = a + s[:, None] * v
        return a / cnt[:, None] if d["mean"] else a

    def f(x, k, k2=None, r=None, b=None):
        if kind == "aggregate_project":
            h = agg(x, torch.from_numpy(sc32).double() if d["self"] else None) @ k
        elif kind == "sage_wide":
            h = torch.cat([x @ k, agg(x) @ k2], 1)
        elif kind == "sage_narrow":
            h = torch.cat([x @ k, agg(x @ k2)], 1)
        elif kind == "linear":
            h = x @ k
        else:
            h = torch.cat([x @ k, r @ k2], 1)
        if b is not None:
            h = h + b
        return h * mask if mask is not None else h
    ins = dict(x=x32, k=k32)
    if U2:
        ins["k2"] = k232
    if r32 is not None:
        ins["r"] = r32
    if d["bias"]:
        ins["b"] = b32
    ref, ref_out = _f64(f, ins, g32)
    ab, ab_out = _f64(f, ins, g32, absolute=True)
    deg = int(np.bincount(ei[1], minlength=n).max(initial=0)) + 2
    _close(out_g, ref_out.numpy(), ab_out.numpy(), (F + F2) * deg, what + " forward")
    k = dict(x=width * deg, k=n * deg, k2=n * deg, r=width, b=n * deg)
    for name in ins:
        for tag, grads in (("gated", grads_g), ("un-gated", grads_u)):
            gv = grads.get(name)
            if nd[name]:
                _close(gv, ref[name].numpy(), ab[name].numpy(), k[name], what + " d/d{} ({})".format(name, tag))
            else:
                assert gv is None, what + " d/d{} ({}) computed but not wanted".format(name, tag)
        if nd[name]:                  # gated and un-gated: the same sums, within rounding of each other
            _close(grads_g[name], grads_u[name].double().cpu().numpy(), ab[name].numpy(), k[name],
                   what + " d/d{} gated vs un-gated".format(name))


# ---------------------------------------------------------------------------------------------------------------- 4. dense pieces
@pytest.mark.gpu
@pytest.mark.parametrize("seed", range(N_DENSE * _SCALE))
def test_fuzz_dense_weight_gradient_pieces(tfg, monkeypatch, seed):
    """plan.gemm_tn (plain and gated by a ReLU output with exact zeros), relu_backward, column_sums and transpose, with g a
    column slice of a wider buffer; M from 0 to ~10^5."""
    from tf_geometric_amd import plan as P, autograd as AG
    d = draw_dense(seed)
    M, Ka, N, ld, c0 = d["M"], d["Ka"], d["N"], d["ld"], d["c0"]
    what = "fuzz dense seed {} {}".format(seed, _what(d, "M", "Ka", "N", "ld", "c0", "bias", "gated", "xpad"))
    gen = torch.Generator(device="cuda")
    gen.manual_seed(80000 + seed)
    x = torch.randn(M, Ka + d["xpad"], generator=gen, device="cuda")[:, :Ka]
    g = torch.randn(M, ld, generator=gen, device="cuda")[:, c0:c0 + N]                  # a column slice
    gate = torch.relu(torch.round(torch.randn(M, ld, generator=gen, device="cuda") * 2))[:, ld - N:]   # exact zeros
    gm = torch.where(gate > 0, g, torch.zeros_like(g)) if d["gated"] else g
    _poison((Ka, N), (N,))
    with _witness(monkeypatch) as log:
        dW, db = P.gemm_tn(x, g, want_bias=d["bias"], gate=gate if d["gated"] else None)
    assert log.count("tfgx_gemm_tn_gated_f32") == 1, what
    xd, gd = x.double(), gm.double()
    _close(dW, (xd.t() @ gd).cpu().numpy(), (xd.abs().t() @ gd.abs()).cpu().numpy(), M, what + " dW")
    if d["bias"]:
        _close(db, gd.sum(0).cpu().numpy(), gd.abs().sum(0).cpu().numpy(), M, what + " db")
    else:
        assert db is None, what
    if d["gated"]:                    # gated == the product with the masked gradient, bit for bit
        dWm, dbm = P.gemm_tn(x, gm, want_bias=d["bias"])
        assert torch.equal(dW, dWm) and (dbm is None or torch.equal(db, dbm)), what + " gated vs masked"
    rb = AG.relu_backward(g, gate)
    assert torch.equal(rb, torch.where(gate > 0, g, torch.zeros_like(g))), what + " relu_backward"
    cs = P.column_sums(g)
    _close(cs, g.double().sum(0).cpu().numpy(), g.double().abs().sum(0).cpu().numpy(), M, what + " column_sums")
    if M <= 20000:
        assert torch.equal(P.transpose(x), x.t().contiguous()), what + " transpose"
        assert torch.equal(P.transpose(g), g.t().contiguous()), what + " transpose of the slice"


# ---------------------------------------------------------------------------------------------------------------- 5. GAT
@pytest.mark.gpu
@pytest.mark.parametrize("seed", range(N_GAT * _SCALE))
def test_fuzz_gat_attention_backward(tfg, monkeypatch, seed):
    """AG.gat_attention on random ragged graphs with n_src >= n_dst: forced hub lists, forced source / destination blocks,
    the query-gradient sums on and off for d = 1; dQ, dK, dV against float64."""
    from tf_geometric_amd import plan as P, autograd as AG
    from f64_layers import gat_attention_f64
    L = tfg._lib
    gd = draw_gat(seed)
    qs, n_dpass, n_spass, hub_s = gat_route(gd)
    rng = _rng(90000, seed)
    H, dd, dv, n_dst, n_src, ei = gd["H"], gd["d"], gd["dv"], gd["n_dst"], gd["n_src"], gd["ei"]
    what = "fuzz gat backward seed {} {} hub={} E={} -> query_sums={} dst_launches={} src_launches={} hub_src={}".format(
        seed, _what(gd, "H", "d", "dv", "n_dst", "n_src", "setting", "source_blocks", "destination_blocks", "query_sums"),
        gd["hub"], ei.shape[1], qs, n_dpass, n_spass, hub_s)
    Q32 = rng.standard_normal((n_dst, H * dd)).astype(np.float32)
    K32 = rng.standard_normal((n_src, H * dd)).astype(np.float32)
    V32 = rng.standard_normal((n_src, H * dv)).astype(np.float32)
    g32 = rng.standard_normal((n_dst, H * dv)).astype(np.float32)
    T, C = gd["hub"] if gd["hub"] else (None, None)
    with _settings(P__HUB_THRESHOLD=T, P__HUB_CHUNK=C, G__SOURCE_BLOCKS=gd["source_blocks"],
                   G__DESTINATION_BLOCKS=gd["destination_blocks"], G__QUERY_GRAD_SUMS=gd["query_sums"]):
        plan = P.CsrPlan.build(L.as_i32(ei), n_dst, n_src)
        t = [L.as_f32(a).requires_grad_(True) for a in (Q32, K32, V32)]
        out = AG.gat_attention(plan, t[0], t[1], t[2], H)
        _poison((n_dst, H * dd), (n_src, H * dd), (n_src, H * dv))
        with _witness(monkeypatch) as bwd:
            out.backward(L.as_f32(g32))
        assert ("tfgx_gat_query_grad_d1_f32" in bwd) == qs, what + " {}".format(sorted(set(bwd)))
        assert bwd.count("tfgx_gat_backward_dst_hub_f32") == n_dpass, what
        assert bwd.count("tfgx_gat_backward_src_hub_f32") == n_spass, what
        rp, col = plan.row_ptr.cpu().numpy(), plan.col.cpu().numpy()
    leaves = [torch.tensor(a, dtype=torch.float64, requires_grad=True) for a in (Q32, K32, V32)]
    ref = gat_attention_f64(leaves[0], leaves[1], leaves[2], rp, col, H)
    _close(out, ref.detach().numpy(), np.zeros(ref.shape), 1, what + " forward", floor=2e-5)
    ref.backward(torch.from_numpy(g32).double())
    indeg, outdeg = _degrees(ei, n_dst, n_src)
    tol = 5e-5 * max(1.0, np.sqrt(max(int(indeg.max(initial=0)), int(outdeg.max(initial=0))) / 64.0))
    for name, got, r in zip(("dQ", "dK", "dV"), t, leaves):
        _close(got.grad, r.grad.numpy(), np.zeros(r.shape), 1, what + " " + name, floor=tol)


# ---------------------------------------------------------------------------------------------------------------- 6. pool MLP
@pytest.mark.gpu
@pytest.mark.parametrize("seed", range(N_POOL * _SCALE))
def test_fuzz_pool_mlp_max_weight_gradient(tfg, monkeypatch, seed):
    """AG.pool_mlp_max (tfgx_pool_mlp_max_wgrad_f32): in-degrees at, one below and one above the LDS chunk length and at
    multiples of it, the last row empty or long, n_dst down to 1; dW, db against float64 autograd of
    max_j relu(x W + b)[col_j] with ties split evenly, decided on the float32 hidden rows."""
    from tf_geometric_amd import plan as P, autograd as AG
    L = tfg._lib
    p = draw_pool(seed)
    rng = _rng(100000, seed)
    F_in, Fp, n, ei = p["F_in"], p["Fp"], p["n"], p["ei"]
    what = "fuzz pool-mlp wgrad seed {} {} E={} deg={}".format(
        seed, _what(p, "F_in", "Fp", "n", "chunk", "last", "bias", "quant"), ei.shape[1], p["deg"].tolist())
    if p["quant"]:                    # exact products: ties between different sources and at the ReLU's zero plateau
        x32 = (np.round(rng.standard_normal((n, F_in)) * 2) / 2).astype(np.float32)
        k32 = (np.round(rng.standard_normal((F_in, Fp)) / np.sqrt(F_in) * 8) / 8).astype(np.float32)
        b32 = (np.round(rng.standard_normal(Fp)) * 0.25).astype(np.float32)
    else:
        x32 = rng.standard_normal((n, F_in)).astype(np.float32)
        k32 = (rng.standard_normal((F_in, Fp)) / np.sqrt(F_in)).astype(np.float32)
        b32 = (rng.standard_normal(Fp) * 0.1).astype(np.float32)
    g32 = rng.standard_normal((n, Fp)).astype(np.float32)
    with _settings(P__HUB_THRESHOLD=4096, P__HUB_CHUNK=None):       # long rows stay rows: the tracked forward takes them
        plan = P.CsrPlan.build(L.as_i32(ei), n, n)
        x = L.as_f32(x32)
        k = L.as_f32(k32).requires_grad_(True)
        b = L.as_f32(b32).requires_grad_(True) if p["bias"] else None
        assert AG.pool_mlp_max_applies(plan, x, k), what + ": pool_mlp_max_applies declined"
        red = AG.pool_mlp_max(plan, x, k, b)
        _poison((F_in, Fp), (Fp,))
        with _witness(monkeypatch) as bwd:
            red.backward(L.as_f32(g32))
        assert bwd.count("tfgx_pool_mlp_max_wgrad_f32") == 1, what
        h32 = P.gemm_bias_act(x, L.as_f32(k32), bias=L.as_f32(b32) if p["bias"] else None, act=L.ACT_RELU).cpu().numpy()
        row, col = _csr(plan)
    rown, coln = row.numpy(), col.numpy()
    red32 = np.full((n, Fp), -_FLT_MAX, np.float32)
    np.maximum.at(red32, rown, h32[coln])
    assert np.array_equal(red.detach().cpu().numpy(), red32), what + " forward maxima"
    coef = _tie_shares(h32[coln], red32, rown, n, Fp)
    gate = torch.from_numpy((h32 > 0).astype(np.float64))            # the ReLU decided on the float32 hidden rows

    def f(x, k, b=None):
        h = x @ k
        if b is not None:
            h = h + b
        return torch.zeros(n, Fp, dtype=torch.float64).index_add(0, row, (h * gate)[col] * coef)
    ins = dict(x=x32, k=k32, b=b32) if p["bias"] else dict(x=x32, k=k32)
    ref, _ = _f64(f, ins, g32)
    ab, _ = _f64(f, ins, g32, absolute=True)
    E = max(ei.shape[1], 1)
    _close(k.grad, ref["k"].numpy(), ab["k"].numpy(), E, what + " dW")
    if p["bias"]:
        _close(b.grad, ref["b"].numpy(), ab["b"].numpy(), E, what + " db")
