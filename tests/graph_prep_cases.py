# coding=utf-8
"""Draws, float64 references and comparators for the once-per-graph kernels: the forward GCN normalisation
(csrc/tfgx_norm.hip) and the duplicate-edge merge (csrc/tfgx_plan.hip).  No device: tests/test_graph_prep_cases.py runs the
census and the comparator checks on the CPU, tests/test_gpu_graph_prep.py holds the kernels to what is stated here.

A. Normalisation.  Reference: normgrad_mirror.restatement in float64 on the float32 weights.  A result is a dict
   ``row_deg [n_rows]``, ``col_deg [n_cols] or None``, ``w_out [E + GUARD]`` in the CALLER's edge order, ``self_coef
   [n_rows + GUARD]``, all float32, the GUARD tail still holding the NaN of NAN_BITS.  Bars (eps = 2^-24):
     exact weights (quantised, unweighted): every degree sum is exact in float32 in any order, so degrees are bit-equal to the
       float64 sums and values lie within 16 eps |ref|: two reciprocal (square) roots and two products are at most six half-ulp
       roundings, 16 leaves room for a 1-ulp rsqrt or reciprocal.  No absolute floor; a reference of exactly 0 demands exactly 0.
     uniform weights: a degree within b = 8 eps sqrt(k) sum|w| (k = edges of the row or column + 1, the diagonal a term), the
       project's long-sum bar.  A value is a product of degree powers d^e: to first order its relative error is sum |e| b/|d|
       — e = -1/2 twice under "both", -1 once under "left" / "right" — so the bar is |ref| (sum |e| b/|d| + 16 eps).  Draws keep
       |d| >= sum|w| / 4 wherever d != 0: b/|d| <= 32 eps sqrt(k) < 1.4e-4 at k = 5120, and the second-order term 3/8 (b/d)^2
       < 8e-9 sits inside the 16 eps.
B. Merge.  Reference: test_gpu_aggregate._np_merge (first-occurrence order, float64 merges); indices bit for bit."""
import functools

import numpy as np
import torch

import normgrad_mirror as nm
from asap_mirror import _Ops

EPS = 2.0 ** -24
K_LONG = 2048            # tfgx_norm.hip kLongRow: longer rows are walked by the whole workgroup
BLOCK = 256              # kBlock
TILE = 32                # kRowsPerBlock: rows of one trip of one workgroup
GRID_CAP = 8191          # kGridCap
GUARD = 64
NAN_BITS = 0x7FC05A5A
SHORT_LENGTHS = (0, 1, 7, 8, 9, 24, 25, 31, 32, 33, 40)
LONG_LENGTHS = (2048, 2049, 2049 + 255, 3072, 3073, 4096 + 1023, 5000)
WEIGHT_MODES = ("quantised", "uniform", "unweighted")
SQUARE_DRAWS = ("short", "long", "tile", "grid2", "degenerate", "empty")
RECT_DRAWS = ("rect7x11", "rect300x40", "rect40x30")
NORM_DRAWS = SQUARE_DRAWS + RECT_DRAWS
SMALL_DRAWS = ("short", "degenerate", "empty", "rect7x11")        # compared as dense matrices too
IDENTITY_DRAWS = ("short", "long", "tile", "degenerate")          # edge permutation / node relabelling


# ---- A. draws ------------------------------------------------------------------------------------------------------------------
def _graph(name, seed, n_rows, n_cols, lengths, paths, long_col=None):
    rng = np.random.Generator(np.random.PCG64(seed))
    lengths = np.asarray(lengths, np.int64)
    assert lengths.size == n_rows
    row = np.repeat(np.arange(n_rows), lengths)
    col = rng.integers(0, n_cols, row.size)
    if long_col is not None:
        c, m = long_col
        col[rng.choice(row.size, m, replace=False)] = c
    order = rng.permutation(row.size)
    return dict(name=name, seed=seed, n_rows=n_rows, n_cols=n_cols, row=row[order].astype(np.int32),
                col=col[order].astype(np.int32), paths=tuple(paths), sign=None, unit=None)


def _degenerate():
    """n = 24.  Node 20 heads no edge and is a column of rows 0..9 (isolated as a row); row 21 holds +1 and -1 into column 22,
    which nothing else reaches (row AND column degree exactly 0); row 23 holds 16 negative weights, all into column 19, which
    nothing else reaches (negative row and column degree)."""
    rng = np.random.Generator(np.random.PCG64(404))
    n = 24
    row, col = [], []
    for r in range(19):
        k = int(rng.integers(1, 7))
        row += [r] * k
        col += list(rng.integers(0, 19, k))
    for r in range(10):
        row.append(r), col.append(20)
    row += [22, 22, 22]
    col += list(rng.integers(0, 19, 3))
    base = len(row)
    row += [21, 21] + [23] * 16
    col += [22, 22] + [19] * 16
    sign = np.ones(len(row))
    unit = np.zeros(len(row), bool)
    sign[base + 1] = -1.0
    unit[base:base + 2] = True
    sign[base + 2:] = -1.0
    order = rng.permutation(len(row))
    return dict(name="degenerate", seed=404, n_rows=n, n_cols=n, row=np.asarray(row, np.int32)[order],
                col=np.asarray(col, np.int32)[order], sign=sign[order], unit=unit[order],
                paths=("isolated-column-only", "cancelled-row", "negative-row"))


@functools.lru_cache(maxsize=None)
def norm_draw(name):
    rng = np.random.Generator(np.random.PCG64(11))
    if name == "short":
        n = 48
        return _graph(name, 1, n, n, list(SHORT_LENGTHS) + list(rng.integers(0, 13, n - len(SHORT_LENGTHS))),
                      ["short-%d" % k for k in SHORT_LENGTHS])
    if name == "long":
        n = 300
        lengths = rng.integers(0, 9, n)
        # (2560 on top of LONG_LENGTHS: the one remainder-loop trip count, 2, that those lengths do not produce)
        fixed = {0: 2049, 5: 2048, 40: 3072, 50: 3073, 100: 4096 + 1023, 150: 2560, 200: 5000, n - 1: 2049 + 255}
        for r, k in fixed.items():
            lengths[r] = k
        return _graph(name, 2, n, n, lengths, ["long-%d" % k for k in LONG_LENGTHS] +
                      ["long-row-0", "long-row-last", "two-long-in-tile", "long-column", "unroll-remainders"], long_col=(7, 2100))
    if name == "tile":
        n = 40
        return _graph(name, 3, n, n, [2049 + 17 * i for i in range(TILE)] + list(rng.integers(0, 9, n - TILE)), ["whole-tile-long"])
    if name == "grid2":
        n = GRID_CAP * TILE + 40
        lengths = rng.integers(0, 9, n)
        lengths[n - 5] = 2049
        return _graph(name, 4, n, n, lengths, ["second-grid-trip"])
    if name == "degenerate":
        return _degenerate()
    if name == "empty":
        return _graph(name, 5, 1, 1, [0], ["empty"])
    if name == "rect7x11":
        return _graph(name, 6, 7, 11, [9, 0, 8, 7, 1, 12, 3], ["rectangular"])
    if name == "rect300x40":
        lengths = rng.integers(0, 5, 300)
        lengths[3] = 2100
        return _graph(name, 7, 300, 40, lengths, ["rectangular", "rectangular-right", "rectangular-long-row"])
    if name == "rect40x30":
        lengths = rng.integers(0, 12, 40)
        lengths[2] = 2060
        return _graph(name, 8, 40, 30, lengths, ["rectangular", "rectangular-right", "rectangular-long-row"])
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def _weights(name, mode):
    d = norm_draw(name)
    E = d["row"].size
    rng = np.random.Generator(np.random.PCG64(1000 + d["seed"]))
    if mode == "unweighted":
        return None
    w = rng.integers(1, 8, E) * 0.25 if mode == "quantised" else rng.uniform(0.5, 1.5, E)
    if d["sign"] is not None:
        w = np.where(d["unit"], 1.0, w) * d["sign"]
    w = w.astype(np.float32)
    w.setflags(write=False)
    return w


def weights(d, mode):
    """float32 [E], or None for the unweighted operator.  Signs only on the degenerate draw."""
    return _weights(d["name"], mode)


def exact_mode(mode):
    return mode != "uniform"


def configs_for(d):
    """All 24 on a square draw; on a rectangular one the legal ones (no self-loop, sym=False; "right" needs n_cols <= n_rows)."""
    if d["n_rows"] == d["n_cols"]:
        return nm.configs()
    out = [("both", False, False, renorm, imp) for renorm in (True, False) for imp in (True, False)]
    out += [("left", False, False, True, False)]
    if d["n_cols"] <= d["n_rows"]:
        out += [("right", False, False, True, False)]
    return out


def fill_diag(cfg):
    norm, sym, asl, renorm, improved = cfg
    fill = 2.0 if improved else 1.0
    if norm == "both":
        return fill, (fill if (asl and renorm) else 0.0)
    return fill, (fill if asl else 0.0)


def permuted_edges(d, seed=0):
    """(draw with its edge list shuffled, q): new edge k is old edge q[k]."""
    q = np.random.Generator(np.random.PCG64(77 + seed)).permutation(d["row"].size)
    out = dict(d, name=d["name"] + "/edges", row=np.ascontiguousarray(d["row"][q]), col=np.ascontiguousarray(d["col"][q]),
               sign=None if d["sign"] is None else d["sign"][q], unit=None if d["unit"] is None else d["unit"][q])
    return out, q


def relabelled(d, seed=0):
    """(draw with node v renamed p[v], p) — square draws."""
    assert d["n_rows"] == d["n_cols"]
    p = np.random.Generator(np.random.PCG64(88 + seed)).permutation(d["n_rows"]).astype(np.int32)
    return dict(d, name=d["name"] + "/nodes", row=p[d["row"]], col=p[d["col"]]), p


# ---- A. reference ----------------------------------------------------------------------------------------------------------------
def _sums(idx, w64, n):
    cnt = np.bincount(idx, minlength=n)[:n]
    return cnt, np.bincount(idx, weights=w64, minlength=n)[:n], np.bincount(idx, weights=np.abs(w64), minlength=n)[:n]


def reference(d, w, cfg):
    """float64: degrees, their bars, values (zeros where the operator has no diagonal) and the first-order sensitivities."""
    norm, sym, asl, renorm, improved = cfg
    fill, diag = fill_diag(cfg)
    n_rows, n_cols = d["n_rows"], d["n_cols"]
    row, col = d["row"].astype(np.int64), d["col"].astype(np.int64)
    w64 = np.ones(row.size) if w is None else np.asarray(w, np.float64)

    def degree(idx, n):
        cnt, s, a = _sums(idx, w64, n)
        deg = s + diag
        bar = 8.0 * EPS * np.sqrt(cnt + 1.0) * (a + abs(diag))
        with np.errstate(all="ignore"):
            rel = np.where(deg != 0.0, bar / np.abs(deg), 0.0)
        return deg, bar, rel, a + abs(diag)
    row_deg, row_bar, rel_r, abs_r = degree(row, n_rows)
    col_deg = col_bar = abs_c = None
    rel_c = rel_r
    if norm == "both" and not sym:
        col_deg, col_bar, rel_c, abs_c = degree(col, n_cols)
    w_out, sc = nm.restatement(_Ops(False), torch.from_numpy(row), torch.from_numpy(col), torch.from_numpy(w64), n_rows,
                               n_cols, cfg)
    if norm == "both":
        sens = 0.5 * (rel_r[row] + rel_c[col])
        sens_sc = 0.5 * (rel_r + rel_c[:n_rows]) if (asl and renorm) else np.zeros(n_rows)
    else:
        sens = rel_r[row] if norm == "left" else rel_r[col]
        sens_sc = rel_r if asl else np.zeros(n_rows)
    return dict(row_deg=row_deg, row_deg_bar=row_bar, col_deg=col_deg, col_deg_bar=col_bar, abs_r=abs_r, abs_c=abs_c,
                w_out=w_out.numpy(), self_coef=np.zeros(n_rows) if sc is None else sc.numpy(), has_self_coef=sc is not None,
                sens=sens, sens_sc=sens_sc)


def dense_reference(d, ref, exact):
    """(dense float64 operator, per-element bar): duplicates add up, the diagonal on top."""
    A, B = np.zeros((d["n_rows"], d["n_cols"])), np.zeros((d["n_rows"], d["n_cols"]))
    np.add.at(A, (d["row"], d["col"]), ref["w_out"])
    np.add.at(B, (d["row"], d["col"]), _bar(ref["w_out"], ref["sens"], exact))
    if ref["has_self_coef"]:
        ar = np.arange(d["n_rows"])
        np.add.at(A, (ar, ar), ref["self_coef"])
        np.add.at(B, (ar, ar), _bar(ref["self_coef"], ref["sens_sc"], exact))
    return A, B


# ---- A. the same formulas in float32 numpy -----------------------------------------------------------------------------------------
_SUM32 = {}


def _sum32(idx, w32, n, key=None):
    """Sequential float32 accumulation in the caller's edge order; memoised for the module's own (read-only) weight arrays."""
    if key is not None and key in _SUM32:
        return _SUM32[key]
    out = np.zeros(n, np.float32)
    np.add.at(out, idx, w32)
    if key is not None:
        _SUM32[key] = out
    return out


def f32_degrees(d, w, cfg):
    fill, diag = fill_diag(cfg)
    w32 = np.ones(d["row"].size, np.float32) if w is None else w
    key = (d["name"], "ones" if w is None else id(w)) if (w is None or not w.flags.writeable) else None
    row_deg = _sum32(d["row"], w32, d["n_rows"], key and key + ("row",)) + np.float32(diag)
    col_deg = None
    if cfg[0] == "both" and not cfg[1]:
        col_deg = _sum32(d["col"], w32, d["n_cols"], key and key + ("col",)) + np.float32(diag)
    return row_deg, col_deg


def _inv_pow32(deg, half):
    one = np.float32(1.0)
    with np.errstate(all="ignore"):
        v = one / np.sqrt(deg) if half else one / deg
    return np.where(np.isfinite(v), v, np.float32(0.0)).astype(np.float32)


def _padded(values):
    out = np.full(values.size + GUARD, np.nan, np.float32)
    out.view(np.uint32)[:] = NAN_BITS
    out[:values.size] = values
    return out


def f32_from_degrees(d, w, cfg, row_deg, col_deg):
    """What tfgx_gcn_norm_edges_f32 writes, operation for operation in float32 numpy."""
    norm, sym, asl, renorm, improved = cfg
    fill = np.float32(fill_diag(cfg)[0])
    row, col = d["row"], d["col"]
    w32 = np.ones(row.size, np.float32) if w is None else w
    cdeg = row_deg if col_deg is None else col_deg
    zeros = np.zeros(d["n_rows"], np.float32)
    if norm == "both":
        pr, pc = _inv_pow32(row_deg, True), _inv_pow32(cdeg, True)
        w_out = (pr[row] * w32) * pc[col]
        sc = zeros if not asl else ((pr * fill) * pc[:d["n_rows"]] if renorm else np.full(d["n_rows"], fill, np.float32))
    elif norm == "left":
        q = _inv_pow32(row_deg, False)
        w_out, sc = q[row] * w32, (q * fill if asl else zeros)
    else:
        q = _inv_pow32(row_deg, False)
        w_out, sc = w32 * q[col], (fill * q if asl else zeros)
    return dict(row_deg=row_deg.copy(), col_deg=None if col_deg is None else col_deg.copy(),
                w_out=_padded(w_out.astype(np.float32)), self_coef=_padded(sc.astype(np.float32)))


def f32_eval(d, w, cfg):
    return f32_from_degrees(d, w, cfg, *f32_degrees(d, w, cfg))


# ---- A. comparators ----------------------------------------------------------------------------------------------------------------
def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _bar(ref, sens, exact):
    return np.abs(ref) * ((0.0 if exact else sens) + 16.0 * EPS)


def _ratio(err, bar):
    with np.errstate(all="ignore"):
        r = np.where(bar > 0.0, err / bar, 0.0)
    return float(r.max()) if r.size else 0.0


def _check_values(what, got, ref, sens, exact):
    got = np.asarray(got, np.float32)
    assert got.shape == ref.shape, "{}: shape {} for {}".format(what, got.shape, ref.shape)
    assert np.isfinite(got).all(), "{}: {} elements are NaN or inf".format(what, int((~np.isfinite(got)).sum()))
    zero = ref == 0.0
    assert (got[zero] == 0.0).all(), "{}: {} elements differ from a reference of exactly 0".format(
        what, int((got[zero] != 0.0).sum()))
    err, bar = np.abs(got.astype(np.float64) - ref), _bar(ref, sens, exact)
    worst = _ratio(err, bar)
    assert (err <= bar).all(), "{}: worst error / bar = {:.3f} ({} elements outside)".format(what, worst, int((err > bar).sum()))
    return worst


def _check_degree(what, got, ref, bar, exact):
    got = np.asarray(got, np.float32)
    assert got.shape == ref.shape, "{}: shape {} for {}".format(what, got.shape, ref.shape)
    assert np.isfinite(got).all(), "{}: NaN or inf".format(what)
    if exact:
        ref32 = ref.astype(np.float32)
        assert (ref32.astype(np.float64) == ref).all(), "{}: the draw's degree sums are not exact in float32".format(what)
        bad = _bits(got) != _bits(ref32)
        assert not bad.any(), "{}: {} degrees differ in bits from the float64 sums (first at {})".format(
            what, int(bad.sum()), int(np.flatnonzero(bad)[0]))
        return 0.0
    err = np.abs(got.astype(np.float64) - ref)
    assert (err <= bar).all(), "{}: worst error / bar = {:.3f}".format(what, _ratio(err, bar))
    return _ratio(err, bar)


def compare(res, ref, exact, what="", guard=True):
    """Hold one result to the reference; -> dict of the worst error / bar ratios.  guard=False: w_out [E] and self_coef
    ([n_rows], or None where the operator has no diagonal) without the NaN tail and without degrees (the public route)."""
    E, n = ref["w_out"].size, ref["self_coef"].size
    w_out, sc = res["w_out"], res["self_coef"]
    stats = {}
    if guard:
        for name, arr, m in (("w_out", w_out, E), ("self_coef", sc, n)):
            assert arr.shape == (m + GUARD,), "{} {}: shape {}".format(what, name, arr.shape)
            assert (_bits(arr[m:]) == NAN_BITS).all(), "{} {}: the guard behind the array was written".format(what, name)
        w_out, sc = w_out[:E], sc[:n]
        stats["row_deg"] = _check_degree(what + " row_deg", res["row_deg"], ref["row_deg"], ref["row_deg_bar"], exact)
        assert (res["col_deg"] is None) == (ref["col_deg"] is None), what + " col_deg"
        if ref["col_deg"] is not None:
            stats["col_deg"] = _check_degree(what + " col_deg", res["col_deg"], ref["col_deg"], ref["col_deg_bar"], exact)
    stats["w_out"] = _check_values(what + " w_out", w_out, ref["w_out"], ref["sens"], exact)
    if guard or ref["has_self_coef"]:
        assert sc is not None, what + " self_coef is missing"
        stats["self_coef"] = _check_values(what + " self_coef", sc, ref["self_coef"], ref["sens_sc"], exact)
    else:
        assert sc is None, what + " self_coef on an operator without a diagonal"
    return stats


def bit_differences(res, other):
    """Elements of (w_out, self_coef, degrees) whose bits differ between two results of the same layout."""
    total = 0
    for k in ("w_out", "self_coef", "row_deg", "col_deg"):
        if res.get(k) is not None and other.get(k) is not None:
            total += int((_bits(res[k]) != _bits(other[k])).sum())
    return total


# ---- A. planted errors, applied to the float32 evaluation -----------------------------------------------------------------------------
def row_lengths(d):
    return np.bincount(d["row"], minlength=d["n_rows"])


def long_rows(d):
    return np.flatnonzero(row_lengths(d) > K_LONG)


def csr_edges(d, r):
    """Caller positions of row r's edges in CSR order (the plan's sort is stable)."""
    return np.flatnonzero(d["row"] == r)


PLANTS = ("degree-drops-last-edge", "remainder-edge-unwritten", "row-degree-for-column", "guard-written", "zero-factor-inf")


def planted(d, w, cfg, kind):
    """The float32 evaluation with one error of `kind` in it."""
    row_deg, col_deg = f32_degrees(d, w, cfg)
    if kind == "degree-drops-last-edge":
        r = long_rows(d)[-1]
        last = csr_edges(d, r)[-1]
        row_deg = row_deg.copy()
        row_deg[r] -= np.float32(1.0) if w is None else w[last]
        return f32_from_degrees(d, w, cfg, row_deg, col_deg)
    if kind == "row-degree-for-column":
        assert cfg[0] == "both" and not cfg[1] and d["n_rows"] == d["n_cols"]
        out = f32_from_degrees(d, w, cfg, row_deg, row_deg)
        out["col_deg"] = col_deg
        return out
    out = f32_from_degrees(d, w, cfg, row_deg, col_deg)
    E = d["row"].size
    if kind == "remainder-edge-unwritten":
        rows = [r for r in long_rows(d) if row_lengths(d)[r] % (4 * BLOCK) != 0]
        out["w_out"][csr_edges(d, rows[0])[-1]] = np.float32(np.nan)
    elif kind == "guard-written":
        out["w_out"][E + 3] = np.float32(0.0)
    elif kind == "zero-factor-inf":
        ref = reference(d, w, cfg)
        zeroed = np.flatnonzero(ref["w_out"] == 0.0)
        assert zeroed.size, "no zeroed factor in this draw / configuration"
        out["w_out"][zeroed[0]] = np.float32(np.inf)
    else:
        raise KeyError(kind)
    return out


# ---- A. census -------------------------------------------------------------------------------------------------------------------
def remainder_trips(length):
    """The remainder-loop trip counts (0..3) that the 256 threads of a workgroup see on a long row of `length` edges."""
    t = np.arange(min(length, BLOCK))
    iters = -(-(length - t) // BLOCK)
    return set((iters % 4).tolist())


def norm_paths(d):
    """The named paths this draw reaches, recomputed from its edge list."""
    out = set()
    n_rows, n_cols = d["n_rows"], d["n_cols"]
    lens = row_lengths(d)
    clens = np.bincount(d["col"], minlength=n_cols)
    longs = np.flatnonzero(lens > K_LONG)
    if n_rows != n_cols:
        out.add("rectangular")
        if n_cols <= n_rows:
            out.add("rectangular-right")
        if longs.size:
            out.add("rectangular-long-row")
        return out
    out.update("short-%d" % k for k in SHORT_LENGTHS if (lens == k).any())
    out.update("long-%d" % k for k in LONG_LENGTHS if (lens == k).any())
    if longs.size:
        if longs[0] == 0:
            out.add("long-row-0")
        if longs[-1] == n_rows - 1:
            out.add("long-row-last")
        per_tile = np.bincount(longs // TILE)
        if ((per_tile >= 2) & (per_tile < TILE)).any():
            out.add("two-long-in-tile")
        if (per_tile == TILE).any():
            out.add("whole-tile-long")
        trips = set()
        for r in longs:
            trips |= remainder_trips(int(lens[r]))
        if trips == {0, 1, 2, 3}:
            out.add("unroll-remainders")
        if n_rows > GRID_CAP * TILE and (longs >= GRID_CAP * TILE).any():
            out.add("second-grid-trip")
    if (clens > K_LONG).any():
        out.add("long-column")
    if ((lens == 0) & (clens > 0)).any():
        out.add("isolated-column-only")
    if d["sign"] is not None:
        w = _weights(d["name"], "quantised").astype(np.float64)
        s = np.bincount(d["row"], weights=w, minlength=n_rows)
        a = np.bincount(d["row"], weights=np.abs(w), minlength=n_rows)
        if ((s == 0.0) & (a > 0.0)).any():
            out.add("cancelled-row")
        if (s < 0.0).any():
            out.add("negative-row")
    if d["row"].size == 0 and n_rows == 1:
        out.add("empty")
    return out


REQUIRED_NORM_PATHS = (["short-%d" % k for k in SHORT_LENGTHS] + ["long-%d" % k for k in LONG_LENGTHS] +
                       ["long-row-0", "long-row-last", "two-long-in-tile", "whole-tile-long", "unroll-remainders", "long-column",
                        "second-grid-trip", "rectangular", "rectangular-right", "rectangular-long-row", "isolated-column-only",
                        "cancelled-row", "negative-row", "empty"])


# ---- B. merge --------------------------------------------------------------------------------------------------------------------
HASH_N = (1, 2, 3, 46340, 46341, 65535, 65536, 65537, 2 ** 20 + 1, 2 ** 31 - 1)
EDGE_COUNTS = (1, 2, 255, 256, 257, 70001, 1000003)
MIXES = ("no-duplicates", "all-same", "half-duplicated", "self-loops")
MODES = ["sum", "mean", "max", "min"]
HUB_COPIES = 3000


@functools.lru_cache(maxsize=None)
def hash_draw(n):
    """300 edges over at most 12 ids of [0, n), 0 and n - 1 among them; (n - 1, n - 1) twice."""
    rng = np.random.Generator(np.random.PCG64(n % 9973))
    pool = np.unique(np.concatenate([[0, n - 1], rng.integers(0, n, 10)]))
    ei = pool[rng.integers(0, pool.size, (2, 300))]
    ei[:, 5] = ei[:, 177] = n - 1
    return ei.astype(np.int32)


@functools.lru_cache(maxsize=None)
def edge_draw(E, mix):
    rng = np.random.Generator(np.random.PCG64(E + 31 * MIXES.index(mix)))
    n = int(np.sqrt(E)) + 2

    def distinct(k):
        h = rng.permutation(n * n)[:k]
        return np.stack([h // n, h % n])
    if mix == "no-duplicates":
        ei = distinct(E)
    elif mix == "all-same":
        ei = np.stack([np.full(E, 3), np.full(E, 5)])
    elif mix == "half-duplicated":
        U = max(1, E // 2)
        idx = np.concatenate([np.arange(U), rng.integers(0, U, E - U)])
        ei = distinct(U)[:, rng.permutation(idx)]
    else:
        m = n // 2 + 2
        row = rng.integers(0, m, E)
        ei = np.stack([row, np.where(rng.random(E) < 0.5, row, rng.integers(0, m, E))])
    return ei.astype(np.int32)


@functools.lru_cache(maxsize=None)
def hub_draw():
    """HUB_COPIES copies of the edge (2, 7) among 500 random edges over 40 nodes."""
    rng = np.random.Generator(np.random.PCG64(3000))
    ei = np.concatenate([np.tile(np.array([[2], [7]]), (1, HUB_COPIES)), rng.integers(0, 40, (2, 500))], axis=1)
    return ei[:, rng.permutation(ei.shape[1])].astype(np.int32)


def props_for(ei, width=None, seed=0):
    rng = np.random.Generator(np.random.PCG64(ei.shape[1] + seed))
    shape = (ei.shape[1],) if width is None else (ei.shape[1], width)
    return rng.uniform(-1.5, 1.5, shape).astype(np.float32)


def _np_merge(ei, props, modes):
    from test_gpu_aggregate import _np_merge as merge
    return merge(ei, props, modes)


def merge_reference(ei, prop, modes):
    """(unique edges int32 [2, U], [merged prop per mode], [tolerance per mode]) for one property [E] or [E, k]: float64
    merges; sums and means at 1e-5 sqrt(max column sum of |terms|), None (bit for bit) for max / min."""
    cols = [prop] if prop.ndim == 1 else [prop[:, j] for j in range(prop.shape[1])]
    merged, terms = [], []
    for c in cols:
        u, out = _np_merge(ei, [c] * len(modes), modes)
        merged.append(out)
        _, t = _np_merge(ei, [np.abs(c)] * len(modes), modes)
        terms.append([float(np.abs(x).max()) for x in t])
    res, tol = [], []
    for m, mode in enumerate(modes):
        res.append(merged[0][m] if prop.ndim == 1 else np.stack([merged[j][m] for j in range(len(cols))], axis=1))
        tol.append(1e-5 * np.sqrt(max(t[m] for t in terms)) if mode in ("sum", "mean") else None)
    return u.astype(np.int32), res, tol


def check_merged(what, u, ref_u):
    u = np.asarray(u)
    assert u.dtype == np.int32 and u.shape == ref_u.shape, "{}: {} {} for {}".format(what, u.dtype, u.shape, ref_u.shape)
    assert np.array_equal(u, ref_u), "{}: unique edges differ (first at {})".format(
        what, int(np.flatnonzero((u != ref_u).any(0))[0]))


def check_props(what, got, ref, tol):
    from conftest import assert_parity
    for g, r, t, mode in zip(got, ref, tol, MODES):
        g = np.asarray(g)
        assert g.dtype == np.float32 and g.shape == r.shape, "{} {}: {} {}".format(what, mode, g.dtype, g.shape)
        if t is None:
            assert np.array_equal(_bits(g), _bits(r)), "{} {}: not bit for bit".format(what, mode)
        else:
            assert_parity(g, r, tol=t, what="{} {}".format(what, mode))


def wrong_merge(ei):
    """The merge with col = key % (n - 1): the planted error of the hash recovery."""
    n = int(ei.max()) + 1
    key = ei[0].astype(np.int64) * n + ei[1]
    _, first = np.unique(key, return_index=True)
    k = key[np.sort(first)]
    return np.stack([k // n, k % max(n - 1, 1)]).astype(np.int32)


def upper_reference(ei, w):
    """convert_edge_to_upper / convert_edge_to_directed restated as in test_edge_preprocessing_on_device: (upper edges, their
    summed weights, directed edges or None when every edge is a self-loop, their weights, the tolerance of the sums)."""
    upper = np.stack([ei.min(0), ei.max(0)])
    up, (uw,) = _np_merge(upper, [w], ["sum"])
    _, (terms,) = _np_merge(upper, [np.abs(w)], ["sum"])
    tol = 1e-5 * np.sqrt(float(terms.max()))
    m = up[0] != up[1]
    if not m.any():
        return up.astype(np.int32), uw, None, None, tol
    return (up.astype(np.int32), uw, np.concatenate([up, up[::-1][:, m]], axis=1).astype(np.int32),
            np.concatenate([uw, uw[m]]), tol)


def hash_class(n):
    """Where n * n falls against the hash widths the kernel has to get right."""
    nn = n * n
    if nn < 2 ** 31:
        return "below-2^31"
    if nn < 2 ** 32:
        return "2^31-to-2^32"
    if nn == 2 ** 32:
        return "exactly-2^32"
    if nn <= 2 ** 61:
        return "above-2^32"
    return "62-bits"


def edge_count_class(E):
    return "below-block" if E < BLOCK else "one-block" if E == BLOCK else "block+1" if E == BLOCK + 1 else "many-blocks"
