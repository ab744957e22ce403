# coding=utf-8
"""Planted NaN / +inf / -inf in the operands of the FORWARD kernels, route by route, against float64.

The seeds, drawers and mirrors are those of test_gpu_fuzz_forward.py (same finite data: unit-variance features, B / sqrt(K));
every case is one route.  After a clean launch the case walks its PLANTS (a site of one operand + one of the three values),
launches again on the same buffers with the plant written in, takes it out again, and holds the pair to one oracle:

  route     the describe string / mirror is the one the seed was built for, in both launches
  T         the reach set: the output elements whose float64 restatement changes under the plant (restated only on the rows /
            columns the plant can reach; NaN != NaN, so every NaN of the planted restatement is in T)
  outside T bit for bit the clean launch (fixed arithmetic order per element: an untouched element has no excuse to move)
  inside T  the class (NaN, +inf, -inf, finite) of the restatement; a finite element (ReLU of -inf, a row renormalised after a
            -inf score, a new maximum) under the forward sweep's bar for the operator: GEMM 2e-5, sums 1e-5 * sqrt(max column
            sum of |messages|), MAX bit for bit, GAT 2e-5, edge softmax 1e-5
  padding   NaN-filled columns / rows outside the launch still NaN

The pattern belongs to the operation, not to the precision: every plant is restated in float64 AND in numpy float32, and the
classes on T must agree (an underflowed exp turning tiny * inf into 0 * inf would make a seed unusable; the cap on unusable
seeds is zero).  test_default_plants_reach_every_route_and_site asserts that, and the coverage of routes and sites, without a
device.  Not drawn: NaN messages under MAX, softmax rows whose scores are all -inf, MAX rows whose messages
are all -inf.

Where the drawn seed cannot carry a plant (all asserted by the census): g128's first visit draws K = 1, so it has no second K
step for the +inf / -inf pair; a -inf under MAX reaches the output only where the planted element was a row's ONLY maximum, so
seeds with quantised (tied) features may carry +inf alone; a plant that reaches a row of a one-row launch (n_dst = 1) reaches
the whole output.  A site is the first of its candidates at which every value changes the float64 restatement (a -inf under a
ReLU that already clamps to 0 changes nothing).  The split-K route carries one plant more: a +inf in B over a zero row of A
(every split's partial then starts with an exact 0: a dead split must not be skipped, and 0 * inf is NaN)."""
import ctypes
import math
import re

import numpy as np
import pytest
import torch

from test_gpu_fuzz_backward import _degrees, _graph, _hubs, _rng, _skewed, _thr
from test_gpu_fuzz_forward import (GAT_SETTINGS, GEMM_PATTERNS, GEMM_ROUTES, PLAIN_SETTINGS, SEG_TARGETS, _desc, _nan, _partition,
                                   _segment_reference, _still_nan, _target_of, _track_reference, draw_gat_forward, draw_gemm,
                                   draw_segment, gat_forward_route, gemm_describe, seg_kernel_name, segment_primary)

VALUES = (("nan", np.nan), ("+inf", np.inf), ("-inf", -np.inf))
ORDERED = VALUES[1:]                      # MAX: infinities are ordinary ordered values; NaN under MAX is not drawn
SOFTMAX_WIDE = 1024                       # kSoftmaxWide (tfgx_attn.hip)


# ---------------------------------------------------------------------------------------------------------------- the oracle
def _cls(a):
    a = np.asarray(a)
    return np.where(np.isnan(a), 1, np.where(a == np.inf, 2, np.where(a == -np.inf, 3, 0))).astype(np.int8)


def reach_set(what, ref0, ref1, ref1_f32):
    """T of one plant from the restatements alone; asserts that float64 and float32 agree on its classes and that it is not
    empty."""
    assert ref0.shape == ref1.shape == ref1_f32.shape, what
    T = ~(np.asarray(ref0, np.float64) == np.asarray(ref1, np.float64))
    assert T.any(), what + ": the plant reaches nothing"
    c64, c32 = _cls(ref1), _cls(ref1_f32)
    assert (c64[T] == c32[T]).all(), what + ": float64 and float32 disagree on the non-finite pattern (unusable seed)"
    return T


def hold(what, got0, got1, ref0, ref1, ref1_f32, tol=None):
    """The oracle on one region (numpy arrays of one shape).  tol None: finite elements of T bit for bit ref1 (MAX)."""
    T = reach_set(what, ref0, ref1, ref1_f32)
    moved = (got0.view(np.int32) != got1.view(np.int32)) & ~T
    if moved.any():
        i = tuple(np.argwhere(moved)[0])
        raise AssertionError("{}: {} elements outside the reach set moved, first at {}: {!r} -> {!r}".format(
            what, int(moved.sum()), i, got0[i], got1[i]))
    cg, cr = _cls(got1), _cls(ref1)
    bad = T & (cg != cr)
    if bad.any():
        i = tuple(np.argwhere(bad)[0])
        raise AssertionError("{}: {} of {} reached elements in the wrong class, first at {}: got {!r} (clean {!r}), float64 says {!r}".format(
            what, int(bad.sum()), int(T.sum()), i, got1[i], got0[i], ref1[i]))
    fin = T & (cr == 0)
    if fin.any():
        if tol is None:
            assert (got1[fin].view(np.int32) == np.asarray(ref1, np.float32)[fin].view(np.int32)).all(), what + ": finite reached elements"
        else:
            g, r = got1[fin].astype(np.float64), np.asarray(ref1, np.float64)[fin]
            worst = float((np.abs(g - r) - tol * np.abs(r)).max())
            assert worst <= tol, "{}: finite reached elements off by {:.3e} > {:.1e}".format(what, worst, tol)
    return T


def _bits_equal(a, b):
    return a.shape == b.shape and (a.numel() == 0 or torch.equal(a.view(torch.int32), b.view(torch.int32)))


def _np_err():
    return np.errstate(all="ignore")


# ---------------------------------------------------------------------------------------------------------------------- GEMM
def gemm_data(d):
    rng = _rng(12500, d["seed"])                   # the forward sweep's stream
    a = rng.standard_normal((d["M"], d["K"])).astype(np.float32)
    b = (rng.standard_normal((d["K"], d["N"])) / np.sqrt(d["K"])).astype(np.float32)
    bias = rng.standard_normal(d["N"]).astype(np.float32) if d["bias"] else None
    return a, b, bias


def gemm_plants(d):
    """[(site label, operand, [(index, value)], reach)] of a first-visit GEMM seed; reach = ("row", i) or ("col", j)."""
    M, K, N, ac = d["M"], d["K"], d["N"], d["act_cols"]
    where, row = (("first", 0), ("last", M - 1), ("interior", M // 2 + 1))[d["seed"] % 3]
    row = min(row, M - 1)
    out = []
    for tag, k in (("k_first", 0), ("k_last", K - 1)):
        for vn, v in VALUES:
            out.append(("A:%s:%s:%s" % (where, tag, vn), "a", [((row, k), v)], ("row", row)))
    cols = [("relu", ac - 1), ("plain", ac)]
    if d["route"] == "slices":
        cols.append(("slice2", 128 + (ac % 97)))
    if d["route"] == "remainder":
        cols.append(("remainder", N - 1))
    elif N - 1 not in (ac - 1, ac):
        cols.append(("last", N - 1))
    for tag, j in cols:
        for vn, v in VALUES:
            out.append(("B:%s:%s" % (tag, vn), "b", [((K // 3, j), v)], ("col", j)))
    if d["bias"]:
        for vn, v in VALUES:
            out.append(("bias:%s" % vn, "bias", [((0,), v)], ("col", 0)))
    if K >= 2:
        out.append(("A:double", "a", [((row, 0), np.inf), ((row, K - 1), -np.inf)], ("row", row)))
    return out


def gemm_restate(d, a, b, bias, reach):
    """act(A B + bias) on one row or one column, in the dtype of a."""
    kind, i = reach
    with _np_err():
        if kind == "row":
            r = a[i:i + 1] @ b
            if bias is not None:
                r = r + bias
            r[:, :d["act_cols"]] = np.maximum(r[:, :d["act_cols"]], 0) if d["act"] else r[:, :d["act_cols"]]
        else:
            r = a @ b[:, i:i + 1]
            if bias is not None:
                r = r + bias[i]
            if d["act"] and i < d["act_cols"]:
                r = np.maximum(r, 0)
    return r


def gemm_dead_split(d, hosts):
    """The split-K route's extra plant: (zeros for row 0 of A, +inf in one element of B outside column 0, whole-output
    restatements without / with the +inf in float64 and with it in float32)."""
    K, N = d["K"], d["N"]
    zero = [((0, k), 0.0) for k in range(K)]
    plant = [((K - 1, N - 1), np.inf)]
    (a32, a64), (b32, b64), (bias32, bias64) = hosts["a"], hosts["b"], hosts["bias"]

    def whole(a, b, bias):
        with _np_err():
            r = a @ b
            if bias is not None:
                r = r + bias
            if d["act"]:
                r[:, :d["act_cols"]] = np.maximum(r[:, :d["act_cols"]], 0)
        return r

    with _Planted(hosts["a"], zero):
        ref0 = whole(a64, b64, bias64)
        with _Planted(hosts["b"], plant):
            ref1, ref32 = whole(a64, b64, bias64), whole(a32, b32, bias32)
    return zero, plant, ref0, ref1, ref32


class _Planted(object):
    """Writes a plant into the named host arrays (every precision) and, when given, the device tensor; restores on exit."""

    def __init__(self, hosts, entries, dev=None):
        self.hosts, self.entries, self.dev = hosts, entries, dev

    def __enter__(self):
        self.saved = [[h[idx].copy() for h in self.hosts] for idx, _ in self.entries]
        for idx, v in self.entries:
            for h in self.hosts:
                h[idx] = v
            if self.dev is not None:
                self.dev[idx] = float(v)
        return self

    def __exit__(self, *exc):
        for (idx, _), old in zip(self.entries, self.saved):
            for h, o in zip(self.hosts, old):
                h[idx] = o
            if self.dev is not None:
                self.dev[idx] = float(old[0])
        return False


def _gemm_refs(d, a, b, bias, reach, clean):
    """(ref0, ref1, ref1 in float32) of the plant that is currently written into the host arrays; clean: cache of ref0."""
    a32, a64 = a
    b32, b64 = b
    bias32, bias64 = bias
    return clean[reach], gemm_restate(d, a64, b64, bias64, reach), gemm_restate(d, a32, b32, bias32, reach)


def _gemm_hosts(d):
    a, b, bias = gemm_data(d)
    hosts = dict(a=(a, a.astype(np.float64)), b=(b, b.astype(np.float64)),
                 bias=(bias, None if bias is None else bias.astype(np.float64)))
    plants = gemm_plants(d)
    clean = {}
    for _, _, _, reach in plants:
        if reach not in clean:
            clean[reach] = gemm_restate(d, hosts["a"][1], hosts["b"][1], hosts["bias"][1], reach)
    return hosts, plants, clean


@pytest.mark.gpu
@pytest.mark.parametrize("route", GEMM_ROUTES)
def test_nonfinite_gemm(tfg, route):
    """tfgx_gemm_bias_act_cols_ws_f32, the route's first visit (ReLU on a strict sub-range of the columns): one element of A
    (T = its row), of B (T = its column), of bias, and +inf / -inf in one row of A at the two ends of K."""
    L = tfg._lib
    lib = L.require_gpu()
    d = draw_gemm(GEMM_ROUTES.index(route))
    what = "nonfinite gemm " + _desc(d)
    hosts, plants, clean_ref = _gemm_hosts(d)
    M, K, N = d["M"], d["K"], d["N"]
    wa, wb = _nan((M, K + d["pad_a"])), _nan((K, N + d["pad_b"]))
    ad, bd = wa[:, d["oa"]:d["oa"] + K], wb[:, d["ob"]:d["ob"] + N]
    ad.copy_(torch.from_numpy(hosts["a"][0]))
    bd.copy_(torch.from_numpy(hosts["b"][0]))
    bias_d = None if hosts["bias"][0] is None else L.as_f32(hosts["bias"][0])
    dev = dict(a=ad, b=bd, bias=bias_d)
    ws_bytes = lib.tfgx_gemm_workspace_bytes(M, K, N) if d["workspace"] else 0
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device="cuda") if ws_bytes else None

    def run():
        wc = _nan((M, N + d["pad_c"]))
        cd = wc[:, d["oc"]:d["oc"] + N]
        name = gemm_describe(lib, d, ad.data_ptr(), bd.data_ptr(), cd.data_ptr(), None if ws is None else ws.data_ptr(), ws_bytes)
        L.check(lib.tfgx_gemm_bias_act_cols_ws_f32(L.ptr(ad), K + d["pad_a"], L.ptr(bd), N + d["pad_b"], L.ptr(bias_d), d["act"],
                                                   d["act_cols"], L.ptr(cd), N + d["pad_c"], M, K, N, L.ptr(ws), ws_bytes,
                                                   L.stream_ptr()), "tfgx_gemm_bias_act_cols_ws_f32")
        assert _still_nan(wc[:, :d["oc"]]) and _still_nan(wc[:, d["oc"] + N:]), what + ": padding columns of C were written"
        return name, cd

    name0, clean = run()
    assert re.match(GEMM_PATTERNS[route], name0), "{}: describe says {}".format(what, name0)
    assert bool(torch.isfinite(clean).all()), what + ": clean launch"
    for label, operand, entries, reach in plants:
        w2 = "{} [{}] plant {}".format(what, name0, label)
        with _Planted(hosts[operand], entries, dev[operand]):
            name1, got = run()
            ref0, ref1, ref32 = _gemm_refs(d, hosts["a"], hosts["b"], hosts["bias"], reach, clean_ref)
        assert name1 == name0, w2 + ": the route depends on the values"
        kind, i = reach
        if kind == "row":
            assert _bits_equal(got[:i], clean[:i]) and _bits_equal(got[i + 1:], clean[i + 1:]), w2 + ": another row moved"
            g0, g1 = clean[i:i + 1].cpu().numpy(), got[i:i + 1].cpu().numpy()
        else:
            assert _bits_equal(got[:, :i], clean[:, :i]) and _bits_equal(got[:, i + 1:], clean[:, i + 1:]), w2 + ": another column moved"
            g0, g1 = clean[:, i:i + 1].cpu().numpy(), got[:, i:i + 1].cpu().numpy()
        hold(w2, g0, g1, ref0, ref1, ref32, tol=2e-5)
    if route == "splitk":
        # a dead split is not skipped: with row 0 of A at zero every split's partial starts with an exact 0, and the +inf in
        # B still has to reach its column (and 0 * inf = NaN the first row)
        zero, plant, ref0, ref1, ref32 = gemm_dead_split(d, hosts)
        with _Planted(hosts["a"], zero, ad):
            name3, base = run()
            base = base.cpu().numpy()
            with _Planted(hosts["b"], plant, bd):
                name4, got = run()
        assert name3 == name0 and name4 == name0, what + ": the route depends on the values"
        T = hold(what + " plant dead split", base, got.cpu().numpy(), ref0, ref1, ref32, tol=2e-5)
        assert T[:, plant[0][0][1]].all() and not T.all()
    name2, again = run()
    assert name2 == name0 and _bits_equal(again, clean), what + ": the operands were not restored"


# ------------------------------------------------------------------------------------------------------------ segment reduce
def segment_seeds():
    """Every SEG_TARGETS entry under its first-visit setting, plus the first later seed of every PLAIN_SETTINGS entry."""
    seeds = list(range(len(SEG_TARGETS)))
    for s in PLAIN_SETTINGS:
        seeds.append(next(i for i in range(len(SEG_TARGETS), 40 * len(SEG_TARGETS)) if draw_segment(i)["setting"] == s))
    return seeds


SEG_SEEDS = segment_seeds()


def segment_data(d):
    rng = _rng(11500, d["seed"])                   # the forward sweep's stream
    F, n_src, n_dst, E = d["F"], d["n_src"], d["n_dst"], d["ei"].shape[1]
    x = rng.standard_normal((n_src, F)).astype(np.float32)
    if d["quant"]:
        x = np.round(x * 2) / 2 + np.float32(0)
    w = None
    if d["weighted"]:
        w = (rng.integers(1, 4, size=E) * 0.5).astype(np.float32) if d["quant"] else rng.uniform(-1.5, 1.5, size=E).astype(np.float32)
    sc = rng.uniform(0.1, 1.0, size=n_dst).astype(np.float32) if d["self"] else None
    bias = rng.standard_normal(F).astype(np.float32) if d["bias"] else None
    deg = np.bincount(d["ei"][0], minlength=n_dst)
    count = deg + (rng.integers(0, 4, size=n_dst) if d["count_extra"] else 0)
    return dict(x=x, add=x.copy() if d["add_x"] else None, w=w, sc=sc, bias=bias, count=count)


def segment_restate(d, h, cols, row=None, edge=None, dt=np.float64):
    """The kernel's contract on the columns `cols` of rows [0, n_run) (row None) or of the one row `row`, in dtype dt (MAX:
    float32-rounded messages, a selection, as _segment_reference).  edge = (original edge index, value): that edge's gathered
    element (the per-edge tail stream) is replaced."""
    ei, n_rows = d["ei"], d["n_run"]
    cols = np.asarray(cols)
    keep = (ei[0] < n_rows) if row is None else (ei[0] == row)
    rr = ei[0][keep] if row is None else np.zeros(int(keep.sum()), np.int64)
    rsel = np.arange(n_rows) if row is None else np.array([row])
    is_max = d["op"] == 2
    mt = np.float64 if is_max else dt
    with _np_err():
        g = h["x"][ei[1][keep]][:, cols].astype(mt)
        if edge is not None:
            g[int(np.searchsorted(np.flatnonzero(keep), edge[0])), 0] = edge[1]
        msg = g * (h["w"][keep][:, None].astype(mt) if h["w"] is not None else mt(1))
        x_self = h["x"][rsel][:, cols]
        if is_max:
            ref = np.full((rsel.shape[0], cols.shape[0]), -np.float32(3.4028234663852886e38), np.float32)
            np.maximum.at(ref, rr, msg.astype(np.float32))
            if h["sc"] is not None:
                ref = np.maximum(ref, h["sc"][rsel][:, None] * x_self)
            dt = np.float32
        else:
            ref = np.zeros((rsel.shape[0], cols.shape[0]), dt)
            np.add.at(ref, rr, msg)
            if h["sc"] is not None:
                ref += h["sc"][rsel][:, None].astype(dt) * x_self.astype(dt)
            if d["op"] == 1:
                ref /= np.maximum(h["count"][rsel], 1)[:, None].astype(dt)
        if h["add"] is not None:
            ref = h["add"][rsel][:, cols].astype(dt) + ref
        if h["bias"] is not None:
            ref = ref + h["bias"][cols].astype(dt)
        if d["relu"]:
            ref = np.maximum(ref, dt(0))
    assert ref.dtype == dt
    return ref


def _hub_chunk(d):
    """plan.hub_policy's chunk length under the seed's override."""
    from tf_geometric_amd import plan as P
    old = P.HUB_THRESHOLD, P.HUB_CHUNK
    P.HUB_THRESHOLD, P.HUB_CHUNK = d["hub"] if d["hub"] else (None, None)
    try:
        return int(P.hub_policy(d["ei"].shape[1], d["n_dst"])[1])
    finally:
        P.HUB_THRESHOLD, P.HUB_CHUNK = old


def _reaches(d, h, operand, idx, reach, vals):
    """Does every value planted at this site change the float64 restatement somewhere?  (ReLU of a -inf over a clamped 0, or a
    -inf below the running maximum, changes nothing: such a site is passed over.)"""
    kind, i = reach
    kw = dict(cols=[i]) if kind == "col" else dict(cols=np.arange(d["F"]), row=i)
    clean = segment_restate(d, h, **kw)
    for _, v in vals:
        if operand == "edge_tail":
            r = segment_restate(d, h, edge=(idx[0], v), **kw)
        else:
            with _Planted((h[operand],), [(idx, v)]):
                r = segment_restate(d, h, **kw)
        if (r == clean).all():
            return False
        if d["op"] == 2 and v == -np.inf and operand == "x":
            # not drawn: a row whose messages in this column are ALL -inf — it returns the empty row's value and a
            # winner count of 0 (test_gpu_regressions.test_max_row_of_only_neg_inf_messages_is_an_empty_row pins that)
            live = d["ei"][0] < d["n_run"]
            with _Planted((h["x"],), [(idx, v)]), _np_err():
                msg = h["x"][d["ei"][1][live], idx[1]] * (h["w"][live] if h["w"] is not None else np.float32(1))
            top = np.full(d["n_run"], -np.inf, np.float32)
            np.maximum.at(top, d["ei"][0][live], msg)
            if (top[np.unique(d["ei"][0][live])] == -np.inf).any():
                return False
    return True


def segment_plants(d, h):
    """[(site label, operand, [(index, value)], reach, variant)].  The planted source is gathered by a hub row when the seed
    has one and, where the graph allows it, by the fewest destinations; a site is the first of its candidates at which all
    the values reach the output."""
    ei, F, n_run = d["ei"], d["F"], d["n_run"]
    is_max = d["op"] == 2
    vals = ORDERED if is_max else VALUES
    live = ei[0] < n_run
    indeg = np.bincount(ei[0][live], minlength=n_run)
    hub_d = bool(_hubs(d)[0] and d["setting"] not in ("spans", "track", "track_spans") and n_run == d["n_dst"])   # as segment_primary
    r0 = int(indeg.argmax())
    out = []

    def site(tag, operand, cands, variant="primary"):
        # sums: one site for the three values.  MAX: +inf and -inf each at the first site where it reaches the output; -inf
        # reaches it only where the planted element was a row's ONLY maximum, which quantised (tied) seeds may not have
        for group in ([vals] if not is_max else [vals[:1], vals[1:]]):
            for idx, reach in (cands if is_max else cands[:48]):
                if _reaches(d, h, operand, idx, reach, group):
                    out.extend(("%s:%s" % (tag, vn), operand, [(idx, v)], reach, variant) for vn, v in group)
                    break
            else:
                assert is_max and group[0][0] == "-inf", "no usable {} site: {}".format(tag, _desc(d))

    srcs = []
    if live.any():
        # hub lists: a source of the longest row's FIRST chunk (the CSR keeps a row's edges in their original order), so the
        # poisoned partial is the one the fold starts from
        cand = np.unique(ei[1][np.flatnonzero(ei[0] == r0)[:_hub_chunk(d)]]) if hub_d else np.unique(ei[1][live])
        fan = [len(set(ei[0][live & (ei[1] == s)].tolist())) for s in cand]
        srcs = [int(cand[i]) for i in np.argsort(fan, kind="stable")]
    elif (d["self"] or d["add_x"]) and not is_max:
        srcs = list(range(n_run))                  # no edge reaches the launch: the self term carries the plant
    fm = (F // 32) * 32                            # the last column first (the ragged end of a row), then those below it
    cols = [("x_main", range(fm - 1, -1, -1)), ("x_tail", range(F - 1, fm - 1, -1))] if d["setting"] == "split" else [("x", range(F - 1, -1, -1))]
    if srcs:
        for tag, cs in cols:
            site(tag, "x", [((s, c), ("col", c)) for c in list(cs)[:8] for s in (srcs if is_max else srcs[:6])])
        if d["setting"] == "split" and live.any():
            site("edge_tail", "edge_tail", [((int(e), c), ("col", c)) for c in list(cols[1][1])[:4] for e in np.flatnonzero(live & (ei[0] == r0))[:12]], "edge_tail")
    if not is_max:
        rows = [int(r) for r in np.argsort(-indeg, kind="stable")]
        if d["weighted"] and live.any():
            site("w", "w", [((int(e),), ("row", int(ei[0][e]))) for e in np.flatnonzero(live & (ei[0] == r0))])
        if d["self"]:
            site("self_coef", "sc", [((r,), ("row", r)) for r in rows])
        if d["bias"]:
            site("bias", "bias", [(((F // 2 + c) % F,), ("col", (F // 2 + c) % F)) for c in range(F)])
        if d["add_x"]:
            site("add_x", "add", [((r, c), ("col", c)) for r in rows[:4] for c in range(min(F, 6))])
    return out


def _segment_refs(d, h, reach, edge, clean):
    """Full-size (ref0, ref1, ref1 float32) with only the reached row / column restated."""
    kind, i = reach
    kw = dict(cols=[i]) if kind == "col" else dict(cols=np.arange(d["F"]), row=i)
    kw["edge"] = edge
    r64 = segment_restate(d, h, dt=np.float64, **kw)      # (MAX: one statement, on float32-rounded messages)
    r32 = segment_restate(d, h, dt=np.float32, **kw)
    ref1, ref32 = clean.copy(), clean.astype(np.float32)
    if kind == "col":
        ref1[:, i], ref32[:, i] = r64[:, 0], r32[:, 0]
    else:
        ref1[i], ref32[i] = r64[0], r32[0]
    return clean, ref1, ref32


def _segment_hosts(d):
    h32 = segment_data(d)                          # (segment_restate casts every operand itself)
    clean = segment_restate(d, h32, np.arange(d["F"]))
    ref, scale = _segment_reference(d, h32["x"], h32["w"], d["ei"], h32["sc"], h32["bias"], h32["count"], d["n_run"])
    assert np.array_equal(clean, ref), "the restatement of this file != _segment_reference on clean data: " + _desc(d)
    return h32, clean, scale


@pytest.mark.gpu
@pytest.mark.parametrize("seed", SEG_SEEDS)
def test_nonfinite_segment_reduce(tfg, seed):
    """tfgx_segment_reduce_f32: one element of a gathered source row of x (main part, tail and per-edge tail stream with split
    rows), one edge weight, one self_coef, bias and add_x entry; MAX: +-inf in x only, the winner table still held."""
    from tf_geometric_amd import plan as P
    L = tfg._lib
    d = draw_segment(seed)
    what = "nonfinite seg_reduce " + _desc(d)
    h32, clean_ref, scale = _segment_hosts(d)
    F, n_src, n_dst, ei, s, n_run = d["F"], d["n_src"], d["n_dst"], d["ei"], d["setting"], d["n_run"]
    is_max = d["op"] == 2
    old = P.HUB_THRESHOLD, P.HUB_CHUNK, P.USE_ROW_ORDER
    try:
        if d["hub"]:
            P.HUB_THRESHOLD, P.HUB_CHUNK = d["hub"]
        P.USE_ROW_ORDER = d["row_order"]
        plan = P.CsrPlan.build(L.as_i32(ei), n_dst, n_src)
        indeg, _ = _degrees(ei, n_dst, n_src)
        assert (plan.hub_info() is not None) == _hubs(d)[0] and (plan.row_order() is not None) == _skewed(indeg, ei.shape[1]), what
        perm = plan.perm.cpu().numpy().astype(np.int64)
        rp = plan.row_ptr.cpu().numpy().astype(np.int64)
        col = plan.col.cpu().numpy().astype(np.int64)
        spans = s in ("spans", "track_spans")
        track = s in ("track", "track_spans")

        def table(a):
            if d["pad_x"]:
                big = _nan((n_src, F + d["pad_x"]))
                big[:, :F] = L.as_f32(a)
                return big[:, :F]
            return L.as_f32(a).clone()

        dev = dict(x=table(h32["x"]), add=table(h32["add"]) if d["add_x"] else None,
                   sc=None if h32["sc"] is None else L.as_f32(h32["sc"]).clone(),
                   bias=None if h32["bias"] is None else L.as_f32(h32["bias"]).clone())
        cnt_d = L.as_i32(h32["count"]) if (d["op"] == 1 and (d["count_extra"] or spans)) else None
        if spans:
            k1 = d["k1"]
            rpk_np, order = _partition(rp, col, n_src, k1)
            rpk_t, col_k = plan.source_blocks(k1)

        def run(variant, edge=None):
            """The seed's launches on the current operands -> (describe strings, out rows [0, n_run), winner table or None)."""
            names = []
            wd = None if h32["w"] is None else plan.edge_attr_to_csr(h32["w"])
            epi = dict(self_coef=dev["sc"], bias=dev["bias"], add_x=dev["add"], act=L.ACT_RELU if d["relu"] else L.ACT_NONE)
            wide_out = _nan((n_dst, F + d["out_off"] + d["out_pad"]))
            out = wide_out[:, d["out_off"]:d["out_off"] + F]
            pk = _nan((n_dst, F), torch.int32) if track else None

            def launch(xin, op, **kw):
                kw.setdefault("wide_blocks", d["wide_blocks"])
                names.append(P.segment_reduce(plan, xin, op, out=out, describe=True, **kw))
                P.segment_reduce(plan, xin, op, out=out, **kw)

            if s == "track":
                launch(dev["x"], L.MAX, w_csr=wd, track=pk)
            elif spans:
                wk = None if wd is None else L.as_f32(wd.cpu().numpy()[order])
                for b in range(k1):
                    kw = dict(w_csr=wk, accumulate=b > 0, row_begin=rpk_t[b:], row_end=rpk_t[b + 1:], rp_stride=k1, col=col_k)
                    if track:
                        launch(dev["x"], L.MAX, track=pk, track_row_begin=rpk_t, **kw)
                    elif b == k1 - 1:
                        launch(dev["x"], d["op"], mean_count=cnt_d, **dict(kw, **epi))
                    else:
                        launch(dev["x"], L.SUM if d["op"] == 1 else d["op"], **kw)
            else:
                kw = dict(w_csr=wd, mean_count=cnt_d, **epi)
                if s == "n_dst":
                    kw["n_dst"] = n_run
                xin = dev["x"]
                if s == "split":
                    xin = P.SplitRows.from_dense(dev["x"])
                    if variant == "edge_tail":
                        xin.with_edge_tail(plan)
                        if edge is not None:
                            (e, c), v = edge
                            pos = int(np.flatnonzero(perm == e)[0])
                            assert col[pos] == ei[1][e]
                            xin.edge_tail[pos, c - int(xin.main.shape[1])] = float(v)
                launch(xin, d["op"], **kw)
            assert _target_of(names[0]) == d["target"], "{}: ran {} instead of the target".format(what, names[0])
            if n_run < n_dst:
                assert _still_nan(out[n_run:]), what + ": rows past n_dst were written"
            if d["out_off"] or d["out_pad"]:
                assert _still_nan(wide_out[:, :d["out_off"]]) and _still_nan(wide_out[:, d["out_off"] + F:]), \
                    what + ": columns outside the block were written"
            return names, out[:n_run].cpu().numpy(), (None if pk is None else pk.cpu().numpy().astype(np.int64) & 0xFFFFFFFF)

        def winners(hh):
            if s == "track":
                o, rows = np.arange(col.shape[0]), rp
            else:
                o, rows = order, rpk_np[::d["k1"]].astype(np.int64)
            w_csr = None if hh["w"] is None else hh["w"][perm][o]
            with _np_err():
                msg32 = (hh["x"][col[o]].astype(np.float64) * (w_csr[:, None].astype(np.float64) if w_csr is not None else 1.0)).astype(np.float32)
            return _track_reference(rows, msg32)

        clean = {}
        tol = None if is_max else 1e-5 * scale ** 0.5
        plants = segment_plants(d, h32)
        assert plants, what + ": no plant"
        for label, operand, entries, reach, variant in plants:
            if variant not in clean:
                clean[variant] = run(variant)
                if track:
                    assert np.array_equal(clean[variant][2], winners(h32)), what + ": clean winner table"
            names0, got0, pk0 = clean[variant]
            w2 = "{} [{}] plant {}".format(what, names0[0], label)
            if operand == "edge_tail":
                names1, got1, pk1 = run(variant, edge=entries[0])
                ref0, ref1, ref32 = _segment_refs(d, h32, reach, (entries[0][0][0], entries[0][1]), clean_ref)
            else:
                with _Planted((h32[operand],), entries, dev.get(operand)):
                    names1, got1, pk1 = run(variant)
                    ref0, ref1, ref32 = _segment_refs(d, h32, reach, None, clean_ref)
                    tref = winners(h32) if track else None
            assert names1 == names0, w2 + ": the route depends on the values"
            hold(w2, got0, got1, ref0, ref1, ref32, tol=tol)
            if track:
                assert np.array_equal(pk1, tref), w2 + ": packed winner table"
                other = np.arange(F) != reach[1]
                assert np.array_equal(pk1[:, other], pk0[:, other]), w2 + ": winner table of another column moved"
        for variant, (names0, got0, pk0) in clean.items():
            names2, got2, pk2 = run(variant)
            assert names2 == names0 and np.array_equal(got2.view(np.int32), got0.view(np.int32)), what + ": the operands were not restored"
    finally:
        P.HUB_THRESHOLD, P.HUB_CHUNK, P.USE_ROW_ORDER = old


# ----------------------------------------------------------------------------------------------------------------------- GAT
def _csr_host(ei, n_dst):
    """(row_ptr, col, perm) of the plan's CSR: destinations ascending, edges of a row in their original order."""
    perm = np.argsort(ei[0], kind="stable")
    rp = np.concatenate([[0], np.cumsum(np.bincount(ei[0], minlength=n_dst))]).astype(np.int64)
    return rp, ei[1][perm].astype(np.int64), perm


def gat_data(g):
    rng = _rng(14500, g["seed"])                   # the forward sweep's stream
    H = g["H"]
    Q = rng.standard_normal((g["n_dst"], H * g["d"])).astype(np.float32)
    K = rng.standard_normal((g["n_src"], H * g["d"])).astype(np.float32)
    V = rng.standard_normal((g["n_src"], H * g["dv"])).astype(np.float32)
    bias = rng.standard_normal(H * g["dv"]).astype(np.float32) if g["bias"] else None
    return dict(Q=Q, K=K, V=V, bias=bias)


def gat_restate(g, h, rp, col, keep, dt):
    """numpy statement of f64_layers.gat_attention_f64 + bias + ReLU in dtype dt -> (out, some (row, head) has only -inf scores)."""
    n, H, d_, dv = g["n_dst"], g["H"], g["d"], g["dv"]
    ar = np.arange(n)
    row = np.repeat(ar, np.diff(rp))
    if g["self_loop"]:
        row, col = np.concatenate([row, ar]), np.concatenate([col, ar])
    Q, K, V = (h[k].astype(dt) for k in "QKV")
    out = np.zeros((n, H * dv), dt)
    dead = False
    with _np_err():
        for hd in range(H):
            sl = slice(hd * d_, (hd + 1) * d_)
            s = (Q[row, sl] * K[col, sl]).sum(-1) / dt(math.sqrt(d_ if g["scale_d"] is None else g["scale_d"]))
            m = np.full(n, -np.inf, dt)
            np.maximum.at(m, row, s)
            dead = dead or bool((m[np.unique(row)] == -np.inf).any())
            p = np.exp(s - m[row])
            den = np.zeros(n, dt)
            np.add.at(den, row, p)
            a = p / (den[row] + dt(1e-8))
            if keep is not None:
                a = a * keep[:a.shape[0], hd].astype(dt) / dt(1.0 - g["rate"])
            np.add.at(out[:, hd * dv:(hd + 1) * dv], row, a[:, None] * V[col, hd * dv:(hd + 1) * dv])
        if h["bias"] is not None:
            out = out + h["bias"].astype(dt)
        if g["relu"]:
            out = np.maximum(out, dt(0))
    return out, dead


def gat_seeds():
    """First visit of every setting whose draw has d_head == 1 ("plain") or d_head > 1 (the others) and some edges."""
    seeds = []
    for i, st in enumerate(GAT_SETTINGS):
        for sd in range(i, 1200, len(GAT_SETTINGS)):
            g = draw_gat_forward(sd)
            if (g["d"] == 1) == (st == "plain") and g["ei"].shape[1] > 50 and g["dv"] > 1 and g["relu"] == (i % 2 == 0):
                seeds.append(sd)
                break
    return seeds


GAT_SEEDS = gat_seeds()


def gat_plants(g, h, rp, col, keep):
    """[(site label, operand, [(index, value)])] and the planted source.  The source is gathered by a destination that also has
    other terms; on source blocks it lies before the last block, on hub lists in the hub row's first chunk (of several)."""
    n_dst, n_src, H, d_, dv = g["n_dst"], g["n_src"], g["H"], g["d"], g["dv"]
    row = np.repeat(np.arange(n_dst), np.diff(rp))
    blocks, hub_d, _ = gat_forward_route(g)
    if blocks:
        per = -(-n_src // blocks)
        cand = [int(s) for s in np.unique(col) if s // per < blocks - 1 and (col[row == row[np.flatnonzero(col == s)[0]]] // per).max() > s // per]
    elif hub_d:
        r0 = int(np.diff(rp).argmax())
        chunk = g["hub"][1]
        assert rp[r0 + 1] - rp[r0] > chunk, "the hub row has one chunk only"
        cand = [int(s) for s in col[rp[r0]:rp[r0] + chunk]]
    else:
        cand = [int(s) for s in np.unique(col)]
    j, c = H * d_ - 1, H * dv - 1
    for s in cand:
        ok = True
        for v in (np.inf, -np.inf):
            with _Planted((h["K"],), [((s, j), v)]):
                ok = ok and not gat_restate(g, h, rp, col, keep, np.float64)[1]
        if ok:
            break
    else:
        raise AssertionError("no usable source: " + _desc(g))
    r = int(row[np.flatnonzero(col == s)[0]])
    plants = [("V:%s" % vn, "V", [((s, c), v)]) for vn, v in VALUES]
    plants += [("K:%s" % vn, "K", [((s, j), v)]) for vn, v in VALUES]
    plants.append(("Q:nan", "Q", [((r, j), np.nan)]))
    return plants, s


def _gat_keep(g, E):
    if g["rate"] <= 0:
        return None
    from test_gpu_backward import _keep_mask_host
    return _keep_mask_host(g["drop_seed"], (E + g["n_dst"]) * g["H"], g["rate"]).reshape(E + g["n_dst"], g["H"])


@pytest.mark.gpu
@pytest.mark.parametrize("seed", GAT_SEEDS)
def test_nonfinite_gat(tfg, seed):
    """tfgx_gat_fused_f32 on the one-pass route, the hub merge, chained source blocks and dropout: one element of V (each
    value), NaN in a K row and a Q row, +-inf in a K row (the score is +-inf by the sign of q: +inf poisons the (row, head),
    -inf drops the edge and the row is renormalised)."""
    from tf_geometric_amd import plan as P
    from tf_geometric_amd.nn.conv import gat as G
    L = tfg._lib
    g = draw_gat_forward(seed)
    what = "nonfinite gat " + _desc(g)
    h = gat_data(g)
    H, n_src, n_dst, ei = g["H"], g["n_src"], g["n_dst"], g["ei"]
    E = ei.shape[1]
    old = P.HUB_THRESHOLD, P.HUB_CHUNK, G.SOURCE_BLOCKS
    try:
        if g["hub"]:
            P.HUB_THRESHOLD, P.HUB_CHUNK = g["hub"]
        G.SOURCE_BLOCKS = g["source_blocks"]
        plan = P.CsrPlan.build(L.as_i32(ei), n_dst, n_src)
        blocks, hub_d, order = gat_forward_route(g)
        rp, col = plan.row_ptr.cpu().numpy().astype(np.int64), plan.col.cpu().numpy().astype(np.int64)
        rp_h, col_h, _ = _csr_host(ei, n_dst)
        assert np.array_equal(rp, rp_h) and np.array_equal(col, col_h), what + ": the plan's CSR is not the stable sort the census assumes"
        assert (plan.hub_info() is not None) == _hubs(g)[0] and blocks == (g["source_blocks"] or 0), what
        keep = _gat_keep(g, E)
        dev = {k: L.as_f32(h[k]).clone() for k in "QKV"}
        bias_d = None if h["bias"] is None else L.as_f32(h["bias"])

        def run():
            st = _nan((n_dst, 2 * H)) if g["stats"] else None
            before = G.SOURCE_BLOCK_STATS["launches"]
            out = G.gat_attention(plan, dev["Q"], dev["K"], dev["V"], H, add_self_loop=g["self_loop"], bias=bias_d,
                                  act=L.ACT_RELU if g["relu"] else L.ACT_NONE, stats_ml=st, drop_rate=g["rate"],
                                  drop_seed=g["drop_seed"], scale_d=g["scale_d"])
            assert G.SOURCE_BLOCK_STATS["launches"] - before == blocks, what + ": source-block launches"
            return out.cpu().numpy()

        got0 = run()
        ref0 = gat_restate(g, h, rp, col, keep, np.float64)[0]
        assert np.isfinite(got0).all(), what
        plants, _ = gat_plants(g, h, rp, col, keep)
        for label, operand, entries in plants:
            w2 = "{} plant {}".format(what, label)
            with _Planted((h[operand],), entries, dev[operand]):
                got1 = run()
                ref1, dead = gat_restate(g, h, rp, col, keep, np.float64)
                ref32 = gat_restate(g, h, rp, col, keep, np.float32)[0]
            assert not dead, w2 + ": a row with all scores at -inf is not drawn"
            hold(w2, got0, got1, ref0, ref1, ref32, tol=2e-5)
        assert np.array_equal(run().view(np.int32), got0.view(np.int32)), what + ": the operands were not restored"
    finally:
        P.HUB_THRESHOLD, P.HUB_CHUNK, G.SOURCE_BLOCKS = old


# ------------------------------------------------------------------------------------------------- fused aggregate -> GEMM
# (F, N, weighted, mean, self_coef, bias, relu, hub): G = 16 (F <= 64) and 32, B fully and partly resident, hub rows + walk order
FUSED_CASES = ((36, 40, True, False, True, True, True, None), (64, 256, False, False, True, True, False, None),
               (100, 64, True, False, True, False, True, None), (128, 256, False, False, True, True, True, None),
               (128, 256, True, True, False, True, True, (32, 16)), (60, 129, False, True, False, True, True, (8, 8)),
               (96, 200, True, False, True, True, True, (100, 64)), (8, 7, False, False, True, True, True, None))


def draw_fused(i):
    F, N, weighted, mean, self_, bias, relu, hub = FUSED_CASES[i]
    rng = _rng(15000, i)
    n = int(rng.integers(150, 400))
    e = int(rng.integers(1500, 4000))
    ei = _graph(rng, n, n, e) if hub else np.stack([rng.integers(1, n, e), rng.integers(0, n, e)]).astype(np.int32)   # (row 0: empty)
    if hub:
        r0, m = int(rng.integers(0, n)), hub[0] + int(rng.integers(1, 3 * hub[0]))
        ei = np.concatenate([ei, np.stack([np.full(m, r0, np.int32), rng.integers(0, n, m).astype(np.int32)])], 1)
    d = dict(seed=i, F=F, N=N, n_src=n, n_dst=n, n_run=n, ei=ei, hub=hub, weighted=weighted, op=1 if mean else 0, self=self_,
             bias=bias, relu=relu)
    E = ei.shape[1]
    d["x"] = rng.standard_normal((n, F)).astype(np.float32)
    d["k"] = (rng.standard_normal((F, N)) / np.sqrt(F)).astype(np.float32)
    d["w"] = rng.uniform(-1.5, 1.5, size=E).astype(np.float32) if weighted else None
    d["sc"] = rng.uniform(0.1, 1.0, size=n).astype(np.float32) if self_ else None
    d["b"] = rng.standard_normal(N).astype(np.float32) if bias else None
    return d


def fused_restate(d, h, dt):
    """(aggregate, act(aggregate @ kernel + bias)) in dtype dt."""
    ei, n = d["ei"], d["n_dst"]
    with _np_err():
        msg = h["x"][ei[1]].astype(dt) * (h["w"][:, None].astype(dt) if h["w"] is not None else dt(1))
        agg = np.zeros((n, d["F"]), dt)
        np.add.at(agg, ei[0], msg)
        if h["sc"] is not None:
            agg += h["sc"][:, None].astype(dt) * h["x"].astype(dt)
        if d["op"] == 1:
            agg /= np.maximum(np.bincount(ei[0], minlength=n), 1)[:, None].astype(dt)
        out = agg @ h["k"].astype(dt)
        if h["b"] is not None:
            out = out + h["b"].astype(dt)
        if d["relu"]:
            out = np.maximum(out, dt(0))
    return agg, out, max(1.0, float(np.abs(msg).sum(0).max()))


def fused_plants(d):
    ei, F, N = d["ei"], d["F"], d["N"]
    indeg = np.bincount(ei[0], minlength=d["n_dst"])
    r0 = int(indeg.argmax())
    cand = np.unique(ei[1][ei[0] == r0])
    fan = [len(set(ei[0][ei[1] == s].tolist())) for s in cand]
    src = int(cand[int(np.argmin(fan))])
    out = [("x:%s" % vn, "x", [((src, F - 1), v)]) for vn, v in VALUES]
    out += [("B:%s:%s" % (tag, vn), "k", [((F // 2, j), v)]) for tag, j in (("resident", 0), ("last", N - 1)) for vn, v in VALUES]
    if d["bias"]:
        out += [("bias:%s" % vn, "b", [((N // 2,), v)]) for vn, v in VALUES]
    if d["self"]:
        out += [("self_coef:%s" % vn, "sc", [((r0,), v)]) for vn, v in VALUES]
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("case", range(len(FUSED_CASES)))
def test_nonfinite_aggregate_gemm(tfg, case):
    """tfgx_aggregate_gemm_f32 with the aggregate as a side output: one element of x (T = every output column of every
    destination that gathers it, and that (row, column) set of the side output), of B, of bias and of self_coef."""
    from tf_geometric_amd import plan as P
    L = tfg._lib
    d = draw_fused(case)
    what = "nonfinite fused " + _desc(d, "x", "k", "w", "sc", "b")
    h = {k: d[k] for k in ("x", "k", "w", "sc", "b")}
    n, F, N = d["n_dst"], d["F"], d["N"]
    old = P.HUB_THRESHOLD, P.HUB_CHUNK
    try:
        if d["hub"]:
            P.HUB_THRESHOLD, P.HUB_CHUNK = d["hub"]
        plan = P.CsrPlan.build(L.as_i32(d["ei"]), n, n)
        assert (plan.hub_info() is not None) == (d["hub"] is not None), what
        assert (plan.row_order() is not None) == _skewed(np.bincount(d["ei"][0], minlength=n), d["ei"].shape[1]), what
        assert L.require_gpu().tfgx_aggregate_gemm_fits(F, N) == 1
        dev = {k: (None if h[k] is None else L.as_f32(h[k]).clone()) for k in ("x", "k", "sc", "b")}

        def run():
            side, wide = _nan((n, F)), _nan((n, N + 3))
            w_csr = None if h["w"] is None else plan.edge_attr_to_csr(h["w"])
            got = P.aggregate_gemm(plan, dev["x"], d["op"], dev["k"], w_csr=w_csr, self_coef=dev["sc"], bias=dev["b"],
                                   act=L.ACT_RELU if d["relu"] else L.ACT_NONE, out=wide[:, 3:], agg_out=side)
            assert got is not None, what + ": the fused launch declined"
            assert _still_nan(wide[:, :3]), what + ": padding columns were written"
            return got.cpu().numpy(), side.cpu().numpy()

        out0, side0 = run()
        agg_ref0, ref0, scale = fused_restate(d, h, np.float64)
        assert np.isfinite(out0).all() and np.isfinite(side0).all(), what
        tol = 2e-5 * scale ** 0.5                                  # the bars of test_fuzz_fused_aggregate_gemm
        for label, operand, entries in fused_plants(d):
            w2 = "{} plant {}".format(what, label)
            with _Planted((h[operand],), entries, dev[operand]):
                out1, side1 = run()
                agg_ref1, ref1, _ = fused_restate(d, h, np.float64)
                agg32, ref32, _ = fused_restate(d, h, np.float32)
            hold(w2, out0, out1, ref0, ref1, ref32, tol=tol * max(1.0, float(np.abs(d["k"]).sum(0).max())))
            if operand in ("x", "sc"):
                hold(w2 + " (side output)", side0, side1, agg_ref0, agg_ref1, agg32, tol=tol)
            else:
                assert np.array_equal(side0.view(np.int32), side1.view(np.int32)), w2 + ": the side output moved"
        out2, side2 = run()
        assert np.array_equal(out2.view(np.int32), out0.view(np.int32)) and np.array_equal(side2.view(np.int32), side0.view(np.int32)), \
            what + ": the operands were not restored"
    finally:
        P.HUB_THRESHOLD, P.HUB_CHUNK = old


# -------------------------------------------------------------------------------------------------------------- edge softmax
SOFTMAX_H = (1, 3, 8, 65)


def draw_softmax(H):
    """~60 destinations with in-degrees 0 .. 40 and one row past the wide launch's limit; scores in the original edge order."""
    rng = _rng(16000, H)
    n = 60
    deg = rng.integers(0, 41, size=n)
    deg[:3] = (0, 2, 40)
    long_row = int(rng.integers(3, n))
    deg[long_row] = SOFTMAX_WIDE + int(rng.integers(1, 101))
    dst = rng.permutation(np.repeat(np.arange(n), deg))
    ei = np.stack([dst, rng.integers(0, n, dst.shape[0])]).astype(np.int32)
    score = (3.0 * rng.standard_normal((dst.shape[0], H))).astype(np.float32)
    short_row = int(next(r for r in rng.permutation(n) if 2 <= deg[r] <= 40))
    return dict(H=H, n=n, ei=ei, score=score, long_row=long_row, short_row=short_row)


def softmax_restate(score, row, n, dt):
    """exp(s - segment max) / (segment sum + 1e-8) per (destination, head), in dtype dt."""
    s = score.astype(dt)
    with _np_err():
        m = np.full((n, s.shape[1]), -np.inf, dt)
        np.maximum.at(m, row, s)
        p = np.exp(s - m[row])
        den = np.zeros((n, s.shape[1]), dt)
        np.add.at(den, row, p)
        return p / (den[row] + dt(1e-8))


def softmax_plants(c):
    out = []
    for tag, r in (("short", c["short_row"]), ("long", c["long_row"])):
        edges = np.flatnonzero(c["ei"][0] == r)
        e, hd = int(edges[len(edges) // 2]), c["H"] // 2
        out += [("%s:%s" % (tag, vn), (e, hd), v) for vn, v in VALUES]
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["perm", "csr", "hub"])
@pytest.mark.parametrize("H", SOFTMAX_H)
def test_nonfinite_edge_softmax(tfg, H, mode):
    """tfgx_edge_softmax_f32 with and without perm (grouped, serial at H = 65, and the wide launch on the long row) and
    tfgx_edge_softmax_hub_f32 with a forced low threshold: clean against float64 at 1e-5, then one planted score in a short
    row and in the long row (T = that (row, head): the other heads of the edge are outside it)."""
    from tf_geometric_amd import plan as P
    L = tfg._lib
    lib = L.require_gpu()
    c = draw_softmax(H)
    n, ei = c["n"], c["ei"]
    what = "nonfinite edge softmax H={} {}".format(H, mode)
    old = P.HUB_THRESHOLD, P.HUB_CHUNK
    try:
        if mode == "hub":
            P.HUB_THRESHOLD, P.HUB_CHUNK = 64, 48
        plan = P.CsrPlan.build(L.as_i32(ei), n, n)
        hub, nc = L.hub_lists(plan) if mode == "hub" else (None, 0)
    finally:
        P.HUB_THRESHOLD, P.HUB_CHUNK = old
    assert (hub is not None) == (mode == "hub")
    perm = plan.perm.cpu().numpy().astype(np.int64)
    use_perm = mode != "csr"
    host = c["score"].copy() if use_perm else c["score"][perm].copy()        # the layout the kernel reads
    row = ei[0].astype(np.int64) if use_perm else ei[0][perm].astype(np.int64)
    where = (lambda e: e) if use_perm else (lambda e: int(np.flatnonzero(perm == e)[0]))
    dev = L.as_f32(host).clone()
    E = host.shape[0]
    hp = 1
    while hp < H:
        hp <<= 1

    def run():
        out = _nan((E, H))
        if hub is not None:
            scratch = _nan((max(nc * 2 * hp, 1),))
            L.check(lib.tfgx_edge_softmax_hub_f32(L.ptr(plan.row_ptr), L.ptr(plan.perm if use_perm else None), L.ptr(dev), H, n,
                                                  L.ptr(out), ctypes.byref(hub), L.ptr(scratch), L.stream_ptr()), "tfgx_edge_softmax_hub_f32")
        else:
            L.check(lib.tfgx_edge_softmax_f32(L.ptr(plan.row_ptr), L.ptr(plan.perm if use_perm else None), L.ptr(dev), H, n,
                                              L.ptr(out), L.stream_ptr()), "tfgx_edge_softmax_f32")
        return out.cpu().numpy()

    got0 = run()
    ref0 = softmax_restate(host, row, n, np.float64)
    assert np.isfinite(got0).all(), what + ": unwritten elements"
    worst = float((np.abs(got0 - ref0) - 1e-5 * np.abs(ref0)).max())
    assert worst <= 1e-5, "{}: clean launch off by {:.3e}".format(what, worst)
    for label, (e, hd), v in softmax_plants(c):
        w2 = "{} plant {}".format(what, label)
        with _Planted((host,), [((where(e), hd), v)], dev):
            got1 = run()
            ref1 = softmax_restate(host, row, n, np.float64)
            ref32 = softmax_restate(host, row, n, np.float32)
        T = hold(w2, got0, got1, ref0, ref1, ref32, tol=1e-5)
        assert set(row[np.argwhere(T)[:, 0]].tolist()) == {int(ei[0][e])} and set(np.argwhere(T)[:, 1].tolist()) == {hd}, w2
    assert np.array_equal(run().view(np.int32), got0.view(np.int32)), what + ": the scores were not restored"


# ------------------------------------------------------------------------------------------------------------- the census (CPU)
def test_default_plants_reach_every_route_and_site():
    """No device: the default seeds reach every GEMM route, every SEG_TARGETS entry and setting, every GAT setting and every
    plant site; for every default (seed, plant) the float64 and float32 restatements agree on the non-finite pattern, and the
    reach set is neither empty nor the whole output.  No seed is skipped."""
    from f64_layers import gat_attention_f64
    from tf_geometric_amd import _lib as L
    from tf_geometric_amd import plan as P
    lib = L.load_library()

    # GEMM
    sites = set()
    for i, route in enumerate(GEMM_ROUTES):
        d = draw_gemm(i)
        assert d["route"] == route and d["act"] == 1 and 0 < d["act_cols"] < d["N"], _desc(d)
        ws_bytes = lib.tfgx_gemm_workspace_bytes(d["M"], d["K"], d["N"]) if d["workspace"] else 0
        name = gemm_describe(lib, d, (1 << 30) + 4 * d["oa"], (2 << 30) + 4 * d["ob"], (3 << 30) + 4 * d["oc"],
                             (4 << 30) if ws_bytes else None, ws_bytes)
        assert re.match(GEMM_PATTERNS[route], name), name
        hosts, plants, clean = _gemm_hosts(d)
        for label, operand, entries, reach in plants:
            with _Planted(hosts[operand], entries):
                T = reach_set("gemm {} {}".format(route, label), *_gemm_refs(d, hosts["a"], hosts["b"], hosts["bias"], reach, clean))
            assert T.size < d["M"] * d["N"]
            if operand == "a":
                assert 0 <= entries[0][0][0] < d["M"]
            if operand == "b":
                assert entries[0][0][1] < d["N"] and ("relu" in label) <= (entries[0][0][1] < d["act_cols"]), label
                assert ("plain" in label) <= (entries[0][0][1] >= d["act_cols"]), label
            sites.add(label.rsplit(":", 1)[0] if label != "A:double" else label)
            sites.add((route, label.split(":")[0]))
        assert ("A:double" in [p[0] for p in plants]) == (d["K"] >= 2)        # (g128's first visit draws K = 1: one K step only)
        sites.add(("double", route))
        if route == "splitk":
            zero, plant, ref0, ref1, ref32 = gemm_dead_split(d, hosts)
            T = reach_set("gemm dead split", ref0, ref1, ref32)
            assert plant[0][0][1] > 0 and T[:, plant[0][0][1]].all() and not T.all() and np.isnan(ref1[0, plant[0][0][1]])
            sites.add("dead split")
            m = re.match(r"^split-K\((\d+)\)", name)
            assert d["K"] // int(m.group(1)) >= 1                   # k = 0 and k = K - 1 lie in the first and the last split
    for r in GEMM_ROUTES:
        assert (r, "A") in sites and (r, "B") in sites, r
    assert [r for r in GEMM_ROUTES if draw_gemm(GEMM_ROUTES.index(r))["K"] < 2] == ["g128"]
    assert {"A:first:k_first", "A:first:k_last", "A:last:k_first", "A:last:k_last", "A:interior:k_first", "A:interior:k_last",
            "B:relu", "B:plain", "B:slice2", "B:remainder", "bias", "A:double", "dead split"} <= sites, sites

    # segment reduce
    seen, settings, sites = set(), set(), set()
    for seed in SEG_SEEDS:
        d = draw_segment(seed)
        kw, hub_d = segment_primary(d, P.wide_blocks_hint)
        assert _target_of(seg_kernel_name(**kw)) == d["target"], _desc(d)
        seen.add(d["target"])
        settings.add((d["setting"], hub_d))
        h32, clean, _ = _segment_hosts(d)
        plants = segment_plants(d, h32)
        assert plants, "no plant: " + _desc(d)
        live = d["ei"][0] < d["n_run"]
        for label, operand, entries, reach, variant in plants:
            w2 = "seg_reduce seed {} {}".format(seed, label)
            if operand == "edge_tail":
                T = reach_set(w2, *_segment_refs(d, h32, reach, (entries[0][0][0], entries[0][1]), clean))
            else:
                with _Planted((h32[operand],), entries):
                    T = reach_set(w2, *_segment_refs(d, h32, reach, None, clean))
            # (a launch of one row is all there is for a plant that reaches a row, one of one column for one that reaches a column)
            assert not T.all() or (d["n_run"] if reach[0] == "row" else d["F"]) == 1, w2 + ": the plant reaches the whole output"
            if operand == "x" and live.any():
                s_ = entries[0][0][0]
                gathers = set(d["ei"][0][live & (d["ei"][1] == s_)].tolist())
                assert gathers, w2
                if hub_d:
                    assert int(np.bincount(d["ei"][0][live]).argmax()) in gathers, w2 + ": no hub row gathers the planted source"
                sites.add(("spared", len(gathers) < d["n_run"]))
            sites.add(label.split(":")[0])
            sites.add((d["setting"], label.split(":")[0]))
            sites.add(("max" if d["op"] == 2 else "sum", label.split(":")[0], label.split(":")[1]))
    assert seen == set(SEG_TARGETS)
    assert {s for s, _ in settings} == set(PLAIN_SETTINGS) | {"wide_blocks", "split", "track", "track_spans"}
    assert ("hub_order", True) in settings and ("hub_noorder", True) in settings and ("split", True) in settings
    assert {"x", "x_main", "x_tail", "edge_tail", "w", "self_coef", "bias", "add_x", ("spared", True)} <= sites, sites
    for s in ("spans", "n_dst", "wide_blocks", "track", "track_spans", "hub_order", "hub_noorder"):
        assert (s, "x") in sites, s
    assert not any(k[0] == "max" and (k[1] not in ("x", "x_main", "x_tail", "edge_tail") or k[2] == "nan") for k in sites if len(k) == 3)

    # GAT
    assert [draw_gat_forward(s)["setting"] for s in GAT_SEEDS] == list(GAT_SETTINGS)
    assert [draw_gat_forward(s)["d"] == 1 for s in GAT_SEEDS] == [True] + [False] * 5
    acts = set()
    for seed in GAT_SEEDS:
        g = draw_gat_forward(seed)
        blocks, hub_d, _ = gat_forward_route(g)
        assert blocks == (g["source_blocks"] or 0) and hub_d == (g["setting"] == "hub"), _desc(g)
        acts.add(g["relu"])
        h = gat_data(g)
        rp, col, _ = _csr_host(g["ei"], g["n_dst"])
        keep = _gat_keep(g, g["ei"].shape[1])
        ref0 = gat_restate(g, h, rp, col, keep, np.float64)[0]
        t64 = lambda a: torch.from_numpy(a.astype(np.float64))      # noqa: E731
        f64 = gat_attention_f64(t64(h["Q"]), t64(h["K"]), t64(h["V"]), rp, col, g["H"], keep=keep, rate=g["rate"],
                                add_self_loop=g["self_loop"], scale_d=g["scale_d"]).numpy()
        f64 = f64 + (h["bias"] if h["bias"] is not None else 0)
        f64 = np.maximum(f64, 0) if g["relu"] else f64
        assert np.allclose(ref0, f64, rtol=1e-12, atol=1e-12), "gat_restate != gat_attention_f64: " + _desc(g)
        plants, src = gat_plants(g, h, rp, col, keep)
        if blocks:
            assert src // -(-g["n_src"] // blocks) < blocks - 1
        classes = set()
        for label, operand, entries in plants:
            w2 = "gat seed {} {}".format(seed, label)
            with _Planted((h[operand],), entries):
                ref1, dead = gat_restate(g, h, rp, col, keep, np.float64)
                ref32 = gat_restate(g, h, rp, col, keep, np.float32)[0]
            assert not dead, w2
            T = reach_set(w2, ref0, ref1, ref32)
            assert not T.all(), w2 + ": the plant reaches the whole output"
            if operand == "K" and "inf" in label:
                classes |= set(_cls(ref1)[T].tolist())
        assert 1 in classes, "seed {}: no +inf score".format(seed)
    assert acts == {True, False}

    # fused aggregate -> GEMM
    marks = set()
    for i in range(len(FUSED_CASES)):
        d = draw_fused(i)
        assert lib.tfgx_aggregate_gemm_fits(d["F"], d["N"]) == 1
        marks |= {("G", 16 if d["F"] <= 64 else 32, d["weighted"]), ("hub", _hubs(d)[0]), ("shape", d["F"], d["N"])}
        marks.add(("hub + walk order", bool(_hubs(d)[0] and _skewed(np.bincount(d["ei"][0], minlength=d["n_dst"]), d["ei"].shape[1]))))
        assert _hubs(d)[0] == (d["hub"] is not None)
        h = {k: d[k] for k in ("x", "k", "w", "sc", "b")}
        agg0, ref0, _ = fused_restate(d, h, np.float64)
        for label, operand, entries in fused_plants(d):
            with _Planted((h[operand],), entries):
                agg1, ref1, _ = fused_restate(d, h, np.float64)
                agg32, ref32, _ = fused_restate(d, h, np.float32)
            T = reach_set("fused {} {}".format(i, label), ref0, ref1, ref32)
            assert not T.all()
            if operand in ("x", "sc"):
                assert not reach_set("fused {} {} side".format(i, label), agg0, agg1, agg32).all()
            marks.add(label.split(":")[0])
    assert {("G", 16, True), ("G", 16, False), ("G", 32, True), ("G", 32, False), ("hub", True), ("hub", False),
            ("shape", 128, 256), ("hub + walk order", True), "x", "B", "bias", "self_coef"} <= marks, marks

    # edge softmax
    for H in SOFTMAX_H:
        c = draw_softmax(H)
        deg = np.bincount(c["ei"][0], minlength=c["n"])
        assert deg.min() == 0 and SOFTMAX_WIDE < deg.max() <= SOFTMAX_WIDE + 100 and 2 <= deg[c["short_row"]] <= 40
        assert _thr(64, 48, c["ei"].shape[1], c["n"]) < deg.max()
        row = c["ei"][0].astype(np.int64)
        ref0 = softmax_restate(c["score"], row, c["n"], np.float64)
        for label, idx, v in softmax_plants(c):
            with _Planted((c["score"],), [(idx, v)]):
                T = reach_set("softmax H={} {}".format(H, label), ref0, softmax_restate(c["score"], row, c["n"], np.float64),
                              softmax_restate(c["score"], row, c["n"], np.float32))
            assert not T.all()
