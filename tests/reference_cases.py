# coding=utf-8
"""
One table of parity cases, three executors.

Every case builds seeded inputs and knows how to run them through
  * ``ref``  — the reference's OWN Python, loaded unmodified from /root/reference by oracle/ref_harness (only in this
               container: tests/golden/make_golden_from_reference.py and tests/test_oracle_vs_reference.py),
  * ``orc``  — the CPU oracle restatement (oracle/tfg_oracle.py),
  * ``hip``  — the product (tf_geometric_amd, HIP kernels through the C ABI; ``-m gpu`` tests).
Each executor returns ``{output name: numpy array}``.  The reference's outputs are committed as
tests/golden/reference_cases.npz (key ``<case>::<output>``) so the GPU box — where /root/reference does not exist —
still checks the product against what the reference itself produced.

``exact`` lists the outputs that must be bit-identical (index work, max/min reductions); everything else is held to
|a - b| <= tol + tol*|b| with tol = 1e-5 (BASELINE.json north_star) unless the case widens it and says why.
"""
import numpy as np

TOL = 1e-5


class Case(object):
    def __init__(self, name, inputs, ref, orc=None, hip=None, exact=(), tol=TOL, key_tol=None, note=""):
        self.name, self.inputs, self.ref, self.orc, self.hip = name, inputs, ref, orc, hip
        self.exact, self.tol, self.key_tol, self.note = set(exact), tol, dict(key_tol or {}), note

    def tol_of(self, key):
        return self.key_tol.get(key, self.tol)

    def __repr__(self):
        return "Case({})".format(self.name)


CASES = []


def _add(*a, **k):
    CASES.append(Case(*a, **k))


# ---------------------------------------------------------------------------------------------------------------------
# seeded inputs
# ---------------------------------------------------------------------------------------------------------------------
def graph(n, e, f, seed, self_loops=0, isolated=0, weighted=True, forbid_self_loops=False):
    """Random multigraph: duplicates allowed, ``self_loops`` explicit (i,i) edges, the last ``isolated`` nodes receive
    no edge (empty segments).  ``forbid_self_loops`` also removes the (i,i) pairs the uniform draw produces by chance, so
    the graph holds NO diagonal entry at all (cases whose result must not depend on how ``SparseMatrix.add_diag`` treats
    an existing diagonal: add-to vs replace)."""
    rng = np.random.Generator(np.random.PCG64(seed))
    hi = n - isolated
    row = rng.integers(0, hi, size=e, dtype=np.int32)
    col = rng.integers(0, n, size=e, dtype=np.int32)
    if forbid_self_loops:
        assert not self_loops
        col = np.where(col == row, (col + 1) % n, col).astype(np.int32)
        assert not (col == row).any()
    if self_loops:
        d = rng.integers(0, hi, size=self_loops, dtype=np.int32)
        row, col = np.concatenate([row, d]), np.concatenate([col, d])
        p = rng.permutation(row.size)
        row, col = row[p], col[p]
    ei = np.stack([row, col]).astype(np.int32)
    x = rng.standard_normal((n, f), dtype=np.float32)
    w = rng.uniform(0.5, 1.5, size=ei.shape[1]).astype(np.float32) if weighted else None
    return dict(n=n, f=f, x=x, ei=ei, w=w, rng=rng)


def glorot(rng, a, b):
    lim = np.sqrt(6.0 / (a + b))
    return rng.uniform(-lim, lim, size=(a, b)).astype(np.float32)


def small_bias(rng, n):
    return (rng.standard_normal(n) * 0.1).astype(np.float32)


def sym_graph(n, e, f, seed):
    """Undirected graph without duplicates or self-loops (what sym=True assumes)."""
    rng = np.random.Generator(np.random.PCG64(seed))
    a = rng.integers(0, n, size=e)
    b = rng.integers(0, n, size=e)
    keep = a != b
    lo, hi = np.minimum(a, b)[keep], np.maximum(a, b)[keep]
    _, first = np.unique(lo * n + hi, return_index=True)
    lo, hi = lo[np.sort(first)], hi[np.sort(first)]
    ei = np.stack([np.concatenate([lo, hi]), np.concatenate([hi, lo])]).astype(np.int32)
    wu = rng.uniform(0.5, 1.5, size=lo.size).astype(np.float32)
    x = rng.standard_normal((n, f), dtype=np.float32)
    return dict(n=n, f=f, x=x, ei=ei, w=np.concatenate([wu, wu]), rng=rng)


def _np(v):
    """tensor-like (reference Tensor / torch tensor / ndarray) -> ndarray."""
    if v is None:
        return None
    if hasattr(v, "detach"):
        return v.detach().cpu().numpy()
    if hasattr(v, "numpy") and not isinstance(v, np.ndarray):
        return np.asarray(v.numpy())
    return np.asarray(v)


def _dense(index, value, shape):
    out = np.zeros(shape, dtype=np.float64)
    index = _np(index)
    np.add.at(out, (index[0], index[1]), _np(value).astype(np.float64))
    return out.astype(np.float32)


def _ract(R, a):
    return None if a is None else R.tf.nn.relu


def _hact(T, a):
    return None if a is None else T.relu


# ---------------------------------------------------------------------------------------------------------------------
# (a1-a5) aggregate_neighbors and its mappers / reducers / updaters   — nn/kernel/map_reduce.py:7-73
# ---------------------------------------------------------------------------------------------------------------------
def _agg_inputs():
    return graph(150, 1400, 13, seed=101, self_loops=9, isolated=7)


def _agg_all(ns, mapper_of, reducer_of, updater_of, call, g):
    out = {}
    for m in ("identity", "gcn"):
        for r in ("sum", "mean", "max"):
            for u in ("sum", "identity"):
                out["{}-{}-{}".format(m, r, u)] = _np(call(g["x"], g["ei"], g["w"], mapper_of(m), reducer_of(r),
                                                           updater_of(u)))
    return out


def _agg_ref(R, g):
    nn = R.tfg.nn
    gm = R.tfg.nn.conv.gcn.gcn_mapper
    return _agg_all(nn, lambda m: gm if m == "gcn" else nn.identity_mapper,
                    lambda r: getattr(nn, r + "_reducer"), lambda u: getattr(nn, u + "_updater"),
                    lambda x, ei, w, m, r, u: nn.aggregate_neighbors(x, ei, w, m, r, u), g)


def _agg_orc(o, g):
    return _agg_all(o, lambda m: getattr(o, m + "_mapper"), lambda r: getattr(o, r + "_reducer"),
                    lambda u: getattr(o, u + "_updater"),
                    lambda x, ei, w, m, r, u: o.aggregate_neighbors(x, ei, w, m, r, u), g)


def _agg_hip(T, g):
    nn = T.nn
    return _agg_all(nn, lambda m: getattr(nn, m + "_mapper"), lambda r: getattr(nn, r + "_reducer"),
                    lambda u: getattr(nn, u + "_updater"),
                    lambda x, ei, w, m, r, u: nn.aggregate_neighbors(x, ei, w, m, r, u), g)


_add("aggregate_neighbors", _agg_inputs, _agg_ref, _agg_orc, _agg_hip,
     exact=["identity-max-identity", "gcn-max-identity"],
     note="max over w*x: products are single fp32 roundings, so identity-updater outputs are bit-exact")


def _count_ref(R, g):
    nn = R.tfg.nn
    return {"count": _np(nn.aggregate_neighbors(g["x"], g["ei"], None, nn.neighbor_count_mapper, nn.sum_reducer,
                                                nn.identity_updater)),
            "max_rows_default": _np(nn.max_reducer(R.tf.gather(g["x"], g["ei"][1]), g["ei"][0])),
            "segment_count": _np(R.tfg.nn.kernel.segment.segment_count(g["ei"][0], g["n"]))}


def _count_orc(o, g):
    return {"count": o.aggregate_neighbors(g["x"], g["ei"], None, o.neighbor_count_mapper, o.sum_reducer,
                                           o.identity_updater),
            "max_rows_default": o.max_reducer(g["x"][g["ei"][1]], g["ei"][0]),
            "segment_count": o.segment_count(g["ei"][0], g["n"])}


def _count_hip(T, g):
    nn = T.nn
    return {"count": _np(nn.aggregate_neighbors(g["x"], g["ei"], None, nn.neighbor_count_mapper, nn.sum_reducer,
                                                nn.identity_updater)),
            "max_rows_default": _np(nn.max_reducer(g["x"][g["ei"][1]], g["ei"][0])),
            "segment_count": _np(nn.segment_count(g["ei"][0], g["n"]))}


_add("neighbor_count_and_defaults", _agg_inputs, _count_ref, _count_orc, _count_hip,
     exact=["count", "max_rows_default", "segment_count"],
     note="max_reducer(num_nodes=None) has max(row)+1 rows (map_reduce.py:38-42); the isolated tail nodes drop out")


def _empty_inputs():
    g = graph(9, 20, 5, seed=111)
    g["ei"], g["w"] = np.zeros((2, 0), np.int32), np.zeros((0,), np.float32)
    return g


def _empty_ref(R, g):
    out = _agg_ref(R, g)
    out["no_edges_as_empty_list"] = _np(R.tfg.nn.aggregate_neighbors(g["x"], np.zeros((0,), np.int32)))
    return out


def _empty_orc(o, g):
    out = _agg_orc(o, g)
    out["no_edges_as_empty_list"] = o.aggregate_neighbors(g["x"], np.zeros((0,), np.int32))
    return out


def _empty_hip(T, g):
    out = _agg_hip(T, g)
    out["no_edges_as_empty_list"] = _np(T.nn.aggregate_neighbors(g["x"], np.zeros((0,), np.int32)))
    return out


_add("aggregate_neighbors_no_edges", _empty_inputs, _empty_ref, _empty_orc, _empty_hip,
     exact=["{}-{}-{}".format(m, r, u) for m in ("identity", "gcn") for r in ("sum", "mean", "max")
            for u in ("sum", "identity")] + ["no_edges_as_empty_list"],
     note="map_reduce.py:57 tests tf.shape(edge_index)[0]: a [2, 0] index is NOT the early return")


# ---------------------------------------------------------------------------------------------------------------------
# (a6) segment_softmax   — nn/kernel/segment.py:26-33
# ---------------------------------------------------------------------------------------------------------------------
def _softmax_inputs():
    g = graph(90, 1100, 4, seed=102, isolated=5)
    g["s1"] = (g["rng"].standard_normal(g["ei"].shape[1]) * 3).astype(np.float32)
    g["s2"] = (g["rng"].standard_normal((g["ei"].shape[1], 6)) * 3).astype(np.float32)
    return g


_add("segment_softmax", _softmax_inputs,
     lambda R, g: {"1d": _np(R.tfg.nn.kernel.segment.segment_softmax(g["s1"], g["ei"][0], g["n"])),
                   "2d": _np(R.tfg.nn.kernel.segment.segment_softmax(g["s2"], g["ei"][0], g["n"]))},
     lambda o, g: {"1d": o.segment_softmax(g["s1"], g["ei"][0], g["n"]),
                   "2d": o.segment_softmax(g["s2"], g["ei"][0], g["n"])},
     lambda T, g: {"1d": _np(T.nn.segment_softmax(g["s1"], g["ei"][0], g["n"])),
                   "2d": _np(T.nn.segment_softmax(g["s2"], g["ei"][0], g["n"]))})


# ---------------------------------------------------------------------------------------------------------------------
# (a7) gcn_norm_adj — nn/conv/gcn.py:32-130 — compared as dense matrices (the stored entry order is not part of the
# contract: tf_sparse merges coordinates, the product keeps the diagonal implicit)
# ---------------------------------------------------------------------------------------------------------------------
NORM_CFGS = [dict(), dict(renorm=False), dict(improved=True), dict(renorm=False, improved=True), dict(norm="left"),
             dict(norm="right"), dict(sym=False), dict(add_self_loop=False), dict(norm="left", add_self_loop=False),
             dict(norm="right", add_self_loop=False), dict(sym=False, add_self_loop=False)]


def _cfg_name(cfg):
    return ",".join("{}={}".format(k, v) for k, v in sorted(cfg.items())) or "default"


def _norm_inputs():
    return graph(70, 500, 3, seed=103, self_loops=6, isolated=4)


def _norm_ref(R, g):
    out = {}
    for cfg in NORM_CFGS:
        adj = R.tfs.SparseMatrix(g["ei"], g["w"], [g["n"], g["n"]])
        nadj = R.tfg.nn.gcn_norm_adj(adj, **cfg)
        out[_cfg_name(cfg)] = _dense(nadj.index, nadj.value, (g["n"], g["n"]))
    ei, w = R.tfg.nn.gcn_norm_edge(g["ei"], g["n"], g["w"])
    out["gcn_norm_edge"] = _dense(ei, w, (g["n"], g["n"]))
    return out


def _norm_orc(o, g):
    out = {}
    for cfg in NORM_CFGS:
        ei, w = o.gcn_norm_adj(g["ei"], g["w"], g["n"], **cfg)
        out[_cfg_name(cfg)] = _dense(ei, w, (g["n"], g["n"]))
    ei, w = o.gcn_norm_adj(g["ei"], g["w"], g["n"])
    out["gcn_norm_edge"] = _dense(ei, w, (g["n"], g["n"]))
    return out


def _norm_hip(T, g):
    out = {}
    for cfg in NORM_CFGS:
        adj = T.SparseMatrix(g["ei"], g["w"], [g["n"], g["n"]])
        nadj = T.nn.gcn_norm_adj(adj, **cfg).to_sparse_matrix()
        out[_cfg_name(cfg)] = _dense(nadj.index, nadj.value, (g["n"], g["n"]))
    ei, w = T.nn.gcn_norm_edge(g["ei"], g["n"], g["w"])
    out["gcn_norm_edge"] = _dense(ei, w, (g["n"], g["n"]))
    return out


_add("gcn_norm_adj", _norm_inputs, _norm_ref, _norm_orc, _norm_hip)


def _norm_inputs_nodiag():
    return graph(70, 500, 3, seed=113, isolated=4, forbid_self_loops=True)


_add("gcn_norm_adj_no_diagonal", _norm_inputs_nodiag, _norm_ref, _norm_orc, _norm_hip,
     note="same 11 configurations on a graph with NO diagonal entry: independent of whether tf_sparse's add_diag adds "
          "to or replaces an existing diagonal (the one [external] semantic that changes numbers, SURVEY.md 8c; call "
          "sites nn/conv/gcn.py:72-98)")


# ---------------------------------------------------------------------------------------------------------------------
# (a8-a10) gcn functional + SparseMatrix surface — nn/conv/gcn.py:225-290
# ---------------------------------------------------------------------------------------------------------------------
def _gcn_inputs():
    g = graph(200, 1800, 24, seed=104, self_loops=5, isolated=6)
    g["kernel"], g["bias"] = glorot(g["rng"], 24, 10), small_bias(g["rng"], 10)
    g["wide_kernel"], g["wide_bias"] = glorot(g["rng"], 24, 40), small_bias(g["rng"], 40)
    g["bias_f"] = small_bias(g["rng"], 24)
    return g


def _gcn_ref(R, g):
    tfg, tf, tfs = R.tfg, R.tf, R.tfs
    adj = lambda: tfs.SparseMatrix(g["ei"], g["w"], [g["n"], g["n"]])       # noqa: E731
    out = {}
    for cfg in NORM_CFGS:
        out[_cfg_name(cfg)] = _np(tfg.nn.gcn(g["x"], adj(), g["kernel"], g["bias"], activation=tf.nn.relu, **cfg))
    out["wide"] = _np(tfg.nn.gcn(g["x"], adj(), g["wide_kernel"], g["wide_bias"], activation=tf.nn.relu))
    out["no_kernel"] = _np(tfg.nn.gcn(g["x"], adj(), None, g["bias_f"]))
    out["no_bias_no_act"] = _np(tfg.nn.gcn(g["x"], adj(), g["kernel"]))
    out["splits"] = _np(tfg.nn.gcn(g["x"], adj(), g["kernel"], g["bias"], num_or_size_splits=[3, 3, 4]))
    out["unweighted"] = _np(tfg.nn.gcn(g["x"], tfs.SparseMatrix(g["ei"], shape=[g["n"], g["n"]]), g["kernel"]))
    out["cached_twice"] = _np((lambda c: (tfg.nn.gcn(g["x"], adj(), g["kernel"], cache=c),
                                          tfg.nn.gcn(g["x"], adj(), g["kernel"], cache=c))[1])({}))
    a = adj()
    out["spmm"] = _np(a @ g["x"])
    out["row_sum"], out["col_sum"] = _np(a.segment_sum(axis=-1)), _np(a.segment_sum(axis=0))
    out["add_diag_dense"] = _np(a.add_diag(2.0).to_dense())
    sm = a.segment_softmax(axis=-1)
    out["softmax_spmm"] = _np(sm @ g["x"])
    out["transpose_spmm"] = _np(a.transpose() @ g["x"])
    return out


def _gcn_orc(o, g):
    n = g["n"]
    out = {}
    for cfg in NORM_CFGS:
        out[_cfg_name(cfg)] = o.gcn(g["x"], g["ei"], g["w"], g["kernel"], g["bias"], "relu", **cfg)
    out["wide"] = o.gcn(g["x"], g["ei"], g["w"], g["wide_kernel"], g["wide_bias"], "relu")
    out["no_kernel"] = o.gcn(g["x"], g["ei"], g["w"], None, g["bias_f"])
    out["no_bias_no_act"] = o.gcn(g["x"], g["ei"], g["w"], g["kernel"])
    out["splits"] = o.gcn(g["x"], g["ei"], g["w"], g["kernel"], g["bias"])
    out["unweighted"] = o.gcn(g["x"], g["ei"], None, g["kernel"])
    out["cached_twice"] = out["no_bias_no_act"]
    out["spmm"] = o.spmm(g["ei"], g["w"], (n, n), g["x"])
    out["row_sum"] = o.unsorted_segment_sum(g["w"], g["ei"][0], n)
    out["col_sum"] = o.unsorted_segment_sum(g["w"], g["ei"][1], n)
    ei2, w2 = o.add_self_loop_edge(g["ei"], n, g["w"], fill_weight=2.0)
    out["add_diag_dense"] = _dense(ei2, w2, (n, n))
    out["softmax_spmm"] = o.spmm(g["ei"], o.segment_softmax(g["w"], g["ei"][0], n), (n, n), g["x"])
    out["transpose_spmm"] = o.spmm(g["ei"][::-1], g["w"], (n, n), g["x"])
    return out


def _gcn_hip(T, g):
    n = g["n"]
    adj = lambda: T.SparseMatrix(g["ei"], g["w"], [n, n])       # noqa: E731
    out = {}
    for cfg in NORM_CFGS:
        out[_cfg_name(cfg)] = _np(T.nn.gcn(g["x"], adj(), g["kernel"], g["bias"], activation=T.relu, **cfg))
    out["wide"] = _np(T.nn.gcn(g["x"], adj(), g["wide_kernel"], g["wide_bias"], activation=T.relu))
    out["no_kernel"] = _np(T.nn.gcn(g["x"], adj(), None, g["bias_f"]))
    out["no_bias_no_act"] = _np(T.nn.gcn(g["x"], adj(), g["kernel"]))
    out["splits"] = _np(T.nn.gcn(g["x"], adj(), g["kernel"], g["bias"], num_or_size_splits=[3, 3, 4]))
    out["unweighted"] = _np(T.nn.gcn(g["x"], T.SparseMatrix(g["ei"], shape=[n, n]), g["kernel"]))
    c = {}
    T.nn.gcn(g["x"], adj(), g["kernel"], cache=c)
    out["cached_twice"] = _np(T.nn.gcn(g["x"], adj(), g["kernel"], cache=c))
    a = adj()
    out["spmm"] = _np(a @ g["x"])
    out["row_sum"], out["col_sum"] = _np(a.segment_sum(axis=-1)), _np(a.segment_sum(axis=0))
    d = a.add_diag(2.0)
    out["add_diag_dense"] = _dense(d.index, d.value, (n, n))
    out["softmax_spmm"] = _np(a.segment_softmax(axis=-1) @ g["x"])
    out["transpose_spmm"] = _np(a.transpose() @ g["x"])
    return out


_add("gcn", _gcn_inputs, _gcn_ref, _gcn_orc, _gcn_hip)


def _gcn_inputs_nodiag():
    g = graph(200, 1800, 24, seed=114, isolated=6, forbid_self_loops=True)
    g["kernel"], g["bias"] = glorot(g["rng"], 24, 10), small_bias(g["rng"], 10)
    g["wide_kernel"], g["wide_bias"] = glorot(g["rng"], 24, 40), small_bias(g["rng"], 40)
    g["bias_f"] = small_bias(g["rng"], 24)
    return g


_add("gcn_no_diagonal", _gcn_inputs_nodiag, _gcn_ref, _gcn_orc, _gcn_hip,
     note="the gcn case on a graph with NO diagonal entry (add_diag reading-independent twin)")


# ---------------------------------------------------------------------------------------------------------------------
# (a11-a12) gat + add_self_loop_edge — nn/conv/gat.py:13-122
# ---------------------------------------------------------------------------------------------------------------------
GAT_CFGS = [dict(H=1, A=4, U=6), dict(H=4, A=8, U=16), dict(H=8, A=8, U=64), dict(H=8, A=64, U=64),
            dict(H=2, A=6, U=10, qact=None, kact=None, act=None), dict(H=4, A=8, U=5, split=False),
            dict(H=3, A=12, U=9, bias=False),
            # head geometries that reach the fast kernels zero-padded / in blocks (nn/conv/gat._kernel_widths)
            dict(H=1, A=1, U=41), dict(H=8, A=256, U=64), dict(H=2, A=2, U=82), dict(H=1, A=8, U=300, act=None),
            dict(H=4, A=12, U=20), dict(H=4, A=20, U=10, split=False)]


def _gat_name(c):
    return "H{H}-A{A}-U{U}".format(**c) + ("-nosplit" if not c.get("split", True) else "") + \
        ("-linearqk" if "qact" in c else "") + ("-nobias" if not c.get("bias", True) else "")


def _gat_inputs():
    g = graph(130, 1500, 20, seed=105, self_loops=7, isolated=5)
    rng = g["rng"]
    g["gat"] = []
    for c in GAT_CFGS:
        uw = c["U"] if c.get("split", True) else c["U"] * c["H"]
        g["gat"].append(dict(wq=glorot(rng, 20, c["A"]), bq=small_bias(rng, c["A"]), wk=glorot(rng, 20, c["A"]),
                             bk=small_bias(rng, c["A"]), wv=glorot(rng, 20, uw),
                             b=small_bias(rng, c["U"]) if c.get("bias", True) else None))
    return g


def _gat_run(fn, act_of, g):
    out = {}
    for c, p in zip(GAT_CFGS, g["gat"]):
        out[_gat_name(c)] = _np(fn(g["x"], g["ei"], p["wq"], p["bq"], act_of(c.get("qact", "relu")), p["wk"], p["bk"],
                                   act_of(c.get("kact", "relu")), p["wv"], p["b"], act_of(c.get("act", "relu")),
                                   num_heads=c["H"], split_value_heads=c.get("split", True)))
    return out


def _selfloop_ref(R, g):
    ei, w = R.tfg.utils.graph_utils.add_self_loop_edge(g["ei"], g["n"], g["w"], fill_weight=2.0)
    ei2, w2 = R.tfg.utils.graph_utils.add_self_loop_edge(g["ei"], g["n"])
    assert w2 is None
    return {"self_loop_index": _np(ei), "self_loop_weight": _np(w), "self_loop_index_noweight": _np(ei2)}


def _gat_ref(R, g):
    out = _gat_run(R.tfg.nn.gat, lambda a: _ract(R, a), g)
    out.update(_selfloop_ref(R, g))
    return out


def _gat_orc(o, g):
    out = _gat_run(o.gat, lambda a: a, g)
    ei, w = o.add_self_loop_edge(g["ei"], g["n"], g["w"], fill_weight=2.0)
    out.update({"self_loop_index": ei, "self_loop_weight": w,
                "self_loop_index_noweight": o.add_self_loop_edge(g["ei"], g["n"])[0]})
    return out


def _gat_hip(T, g):
    out = _gat_run(T.nn.gat, lambda a: _hact(T, a), g)
    ei, w = T.utils.add_self_loop_edge(g["ei"], g["n"], g["w"], fill_weight=2.0)
    out.update({"self_loop_index": _np(ei), "self_loop_weight": _np(w),
                "self_loop_index_noweight": _np(T.utils.add_self_loop_edge(g["ei"], g["n"])[0])})
    return out


_add("gat", _gat_inputs, _gat_ref, _gat_orc, _gat_hip,
     exact=["self_loop_index", "self_loop_weight", "self_loop_index_noweight"])


# ---------------------------------------------------------------------------------------------------------------------
# (a13-a15) GraphSAGE — nn/conv/graph_sage.py:9-287
# ---------------------------------------------------------------------------------------------------------------------
def _sage_inputs():
    g = graph(160, 1500, 18, seed=106, self_loops=4, isolated=6)
    rng = g["rng"]
    g.update(ws=glorot(rng, 18, 7), wn=glorot(rng, 18, 7), b14=small_bias(rng, 14), b7=small_bias(rng, 7),
             wmlp=glorot(rng, 18, 28), bmlp=small_bias(rng, 28), wpn=glorot(rng, 28, 7),
             wg=glorot(rng, 18, 9), bg=small_bias(rng, 9))
    # the pooling variants run on a copy where every node has an in-edge: max over an EMPTY neighbourhood is float32
    # lowest (covered bit-exactly by the aggregate_neighbors case) and lowest @ W overflows to inf/NaN in the reference
    iso = np.arange(g["n"] - 6, g["n"], dtype=np.int32)
    g["ei_full"] = np.concatenate([g["ei"], np.stack([iso, (iso * 7) % g["n"]])], axis=1).astype(np.int32)
    g["w_full"] = np.concatenate([g["w"], np.ones(6, np.float32)])
    return g


def _sage_run(ns, act, g, gcn_cache):
    out = {}
    for name in ("mean", "sum"):
        fn = getattr(ns, name + "_graph_sage")
        for concat in (True, False):
            for weighted in (True, False):
                for normalize in (False, True):
                    key = "{}-concat{}-w{}-l2{}".format(name, int(concat), int(weighted), int(normalize))
                    out[key] = _np(fn(g["x"], g["ei"], g["w"] if weighted else None, g["ws"], g["wn"],
                                      g["b14"] if concat else g["b7"], act, concat=concat, normalize=normalize))
    for name in ("mean_pool", "max_pool"):
        fn = getattr(ns, name + "_graph_sage")
        for concat in (True, False):
            key = "{}-concat{}".format(name, int(concat))
            out[key] = _np(fn(g["x"], g["ei_full"], g["w_full"], g["ws"], g["wmlp"], g["wpn"], g["bmlp"],
                              g["b14"] if concat else g["b7"], act, concat=concat, normalize=True))
    out["gcn-cacheNone"] = _np(ns.gcn_graph_sage(g["x"], g["ei"], g["w"], g["wg"], g["bg"], act, normalize=True))
    out["gcn-cacheDict"] = _np(ns.gcn_graph_sage(g["x"], g["ei"], g["w"], g["wg"], g["bg"], act, cache=gcn_cache()))
    out["gcn-unweighted"] = _np(ns.gcn_graph_sage(g["x"], g["ei"], None, g["wg"], g["bg"], act))
    return out


_add("graph_sage", _sage_inputs,
     lambda R, g: _sage_run(R.tfg.nn, R.tf.nn.relu, g, dict),
     lambda o, g: _sage_run(o, "relu", g, dict),
     lambda T, g: _sage_run(T.nn, T.relu, g, dict))


# ---------------------------------------------------------------------------------------------------------------------
# (b) the layer classes: constructor kwargs, weight names and shapes, call signature — layers/conv/*.py
# The reference layer is built first; ITS variables (by the names it registered) are loaded into the product layer.
# ---------------------------------------------------------------------------------------------------------------------
LAYER_SPECS = [
    ("GCN", dict(units=9, activation="relu"), "xew", dict(cache=True)),
    ("GCN", dict(units=9, use_bias=False, renorm=False, improved=True), "xe", dict()),
    ("GCN", dict(units=9, use_kernel=False, norm="left"), "xew", dict()),
    ("GAT", dict(units=16, attention_units=8, num_heads=4, activation="relu"), "xe", dict()),
    ("GAT", dict(units=64, attention_units=8, num_heads=8), "xew", dict()),
    ("GAT", dict(units=6, num_heads=3, split_value_heads=False, use_bias=False), "xe", dict()),
    ("MeanGraphSage", dict(units=12), "xew", dict()),
    ("MeanGraphSage", dict(units=12, concat=False, normalize=True, use_bias=False), "xe", dict()),
    ("SumGraphSage", dict(units=10), "xew", dict()),
    ("GCNGraphSage", dict(units=10, normalize=True), "xew", dict()),
    ("MeanPoolGraphSage", dict(units=8), "xew", dict()),
    ("MaxPoolGraphSage", dict(units=8, concat=False), "xew", dict()),
]


def _layer_key(i):
    return "{:02d}-{}".format(i, LAYER_SPECS[i][0])


def _layer_inputs():
    return graph(110, 1000, 15, seed=107, self_loops=3, isolated=0)   # empty rows + max-pool overflow: see graph_sage case


def _layer_kwargs(kw, act):
    kw = dict(kw)
    if "activation" in kw:
        kw["activation"] = act
    return kw


def _layer_ref(R, g):
    R.tf.random.set_seed(1234)
    out = {}
    for i, (cls, kw, sig, opts) in enumerate(LAYER_SPECS):
        layer = getattr(R.tfg.layers, cls)(**_layer_kwargs(kw, R.tf.nn.relu))
        inputs = [g["x"], g["ei"]] + ([g["w"]] if sig == "xew" else [])
        y = layer(inputs, cache={}) if opts.get("cache") else layer(inputs)
        out[_layer_key(i)] = _np(y)
        for v in layer.trainable_variables:
            val = np.array(_np(v))
            if v.name.endswith("bias"):          # zero-initialised in the reference; make them matter
                val = (np.sin(np.arange(val.size, dtype=np.float32)) * 0.1).astype(np.float32)
                v.assign(val)
            out["{}::{}".format(_layer_key(i), v.name)] = val
        y = layer(inputs, cache={}) if opts.get("cache") else layer(inputs)
        out[_layer_key(i)] = _np(y)
    return out


def layer_weights(golden, i):
    """{variable name: value} the reference layer registered for spec i (read back from the golden file)."""
    pre = "layers::{}::".format(_layer_key(i))
    return {k[len(pre):]: v for k, v in golden.items() if k.startswith(pre)}


def _layer_hip(T, g, golden):
    out = {}
    for i, (cls, kw, sig, opts) in enumerate(LAYER_SPECS):
        layer = getattr(T.layers, cls)(**_layer_kwargs(kw, T.relu))
        inputs = [g["x"], g["ei"]] + ([g["w"]] if sig == "xew" else [])
        layer._maybe_build(inputs)
        ref_w = layer_weights(golden, i)
        mine = {k: tuple(v.shape) for k, v in layer.weights.items()}
        theirs = {k: tuple(v.shape) for k, v in ref_w.items()}
        assert mine == theirs, "{}: weight names/shapes {} differ from the reference's {}".format(cls, mine, theirs)
        layer.set_weights(**ref_w)
        out[_layer_key(i)] = _np(layer(inputs, cache={}) if opts.get("cache") else layer(inputs))
        out.update({"{}::{}".format(_layer_key(i), k): v for k, v in ref_w.items()})
    return out


_add("layers", _layer_inputs, _layer_ref, None, _layer_hip,
     note="the hip executor takes the golden dict as third argument (weights come from the reference's own variables)")


# ---------------------------------------------------------------------------------------------------------------------
# BASELINE.json configs[0] and configs[1]: the 2-layer GCN MODEL of demo/demo_gcn.py:18-32 (GCN(16, relu) -> GCN(classes),
# Dropout between them: identity at inference) at Cora shape and at ogbn-arxiv shape, through the reference's own
# tfg.layers.GCN with a shared graph cache.  Synthetic inputs per SURVEY.md 8d (no dataset downloads here).
# ---------------------------------------------------------------------------------------------------------------------
MODEL_SHAPES = {"model_gcn_cora": dict(n=2708, e=10556, f=1433, hidden=16, classes=7, seed=301, bow=True, rows=None),
                "model_gcn_arxiv": dict(n=170000, e=1200000, f=128, hidden=256, classes=40, seed=302, bow=False,
                                        rows=2000)}


def directed_pairs(rng, n, e):
    """E/2 uniform pairs, a == b dropped, emitted [all (a,b) | all (b,a)] (utils/graph_utils.py:186-190)."""
    a = rng.integers(0, n, size=e // 2, dtype=np.int64)
    b = rng.integers(0, n, size=e // 2, dtype=np.int64)
    keep = a != b
    a, b = a[keep], b[keep]
    return np.stack([np.concatenate([a, b]), np.concatenate([b, a])]).astype(np.int32)


def _model_inputs(name):
    def make():
        c = MODEL_SHAPES[name]
        rng = np.random.Generator(np.random.PCG64(c["seed"]))
        ei = directed_pairs(rng, c["n"], c["e"])
        if c["bow"]:        # Cora-like: ~17 active words of 1433 per node, rows normalised to sum 1
            x = (rng.random((c["n"], c["f"])) < 0.012).astype(np.float32)
            x = x / np.maximum(x.sum(1, keepdims=True), 1.0)
        else:
            x = rng.standard_normal((c["n"], c["f"]), dtype=np.float32)
        g = dict(n=c["n"], f=c["f"], x=x, ei=ei, w=np.ones(ei.shape[1], np.float32),    # Graph default: data/graph.py:53-56
                 k0=glorot(rng, c["f"], c["hidden"]), b0=small_bias(rng, c["hidden"]),
                 k1=glorot(rng, c["hidden"], c["classes"]), b1=small_bias(rng, c["classes"]),
                 hidden=c["hidden"], classes=c["classes"])
        g["rows"] = None if c["rows"] is None else np.sort(rng.permutation(c["n"])[:c["rows"]]).astype(np.int32)
        return g
    return make


def _model_outputs(g, hidden, logits):
    """What is stored / compared: the full logits at Cora shape; at arxiv shape (27 MB of logits) the sampled rows plus
    float64 column sums of |.| over ALL rows of both layers' outputs (no cancellation: held to the same 1e-5 relative)."""
    hidden, logits = _np(hidden), _np(logits)
    out = {"hidden_col_abs_sum": np.abs(hidden.astype(np.float64)).sum(0),
           "logits_col_abs_sum": np.abs(logits.astype(np.float64)).sum(0)}
    if g["rows"] is None:
        out["logits"] = logits
    else:
        out["rows"] = g["rows"]
        out["logits_rows"] = logits[g["rows"]]
        out["hidden_rows_head"] = hidden[g["rows"][:100]]
    return out


def _model_ref(R, g):
    tf, tfg = R.tf, R.tfg

    class GCNModel(tf.keras.Model):                   # demo/demo_gcn.py:18-32, verbatim structure

        def __init__(self, *args, **kwargs):
            super().__init__(*args, **kwargs)
            self.gcn0 = tfg.layers.GCN(g["hidden"], activation=tf.nn.relu)
            self.gcn1 = tfg.layers.GCN(g["classes"])
            self.dropout = tf.keras.layers.Dropout(0.5)

        def call(self, inputs, training=None, mask=None, cache=None):
            x, edge_index, edge_weight = inputs
            h = self.dropout(x, training=training)
            h = self.gcn0([h, edge_index, edge_weight], cache=cache)
            self.hidden = h
            h = self.dropout(h, training=training)
            h = self.gcn1([h, edge_index, edge_weight], cache=cache)
            return h

    model = GCNModel()
    cache = {}
    inputs = [g["x"], g["ei"], g["w"]]
    model(inputs, cache=cache)                        # builds the variables and the cached normalised adjacency
    for layer, k, b in ((model.gcn0, g["k0"], g["b0"]), (model.gcn1, g["k1"], g["b1"])):
        layer.kernel.assign(k)
        layer.bias.assign(b)
    logits = model(inputs, cache=cache)
    return _model_outputs(g, model.hidden, logits)


def _model_orc(o, g):
    h = o.gcn(g["x"], g["ei"], g["w"], g["k0"], g["b0"], "relu")
    return _model_outputs(g, h, o.gcn(h, g["ei"], g["w"], g["k1"], g["b1"]))


def _model_hip(T, g):
    gcn0, gcn1 = T.layers.GCN(g["hidden"], activation=T.relu), T.layers.GCN(g["classes"])
    cache = {}
    x = T._lib.as_f32(g["x"])
    gcn0._maybe_build([x])
    gcn0.set_weights(kernel=g["k0"], bias=g["b0"])
    h = gcn0([x, g["ei"], g["w"]], cache=cache)
    gcn1._maybe_build([h])
    gcn1.set_weights(kernel=g["k1"], bias=g["b1"])
    return _model_outputs(g, h, gcn1([h, g["ei"], g["w"]], cache=cache))


for _name in MODEL_SHAPES:
    _add(_name, _model_inputs(_name), _model_ref, _model_orc, _model_hip, exact=["rows"],
         note="BASELINE.json configs[{}]: 2-layer GCN model of demo/demo_gcn.py".format(0 if "cora" in _name else 1))


# ---------------------------------------------------------------------------------------------------------------------
# The other two demo MODELS, end to end through the reference's own layer classes:
#   * demo/demo_gat.py:18-42 — GAT(64, relu, num_heads=8, attention_units=8) -> GAT(classes, num_heads=1, attention_units=1)
#     at Cora shape (dropout / edge dropout: identity at inference);
#   * demo/demo_graph_sage.py:22-60 — MeanGraphSage(256, relu, concat) x 2 over two SAMPLED neighbourhoods (25 / 10 incoming
#     edges per node, as RandomNeighborSampler.sample(k) hands them over: an edge list plus per-edge weights) -> Dense, at a
#     PPI-like shape (50 features, 121 labels).  The sampled lists are inputs of the case (drawn once, seeded): the sampler
#     itself is random by contract and has its own distributional test.
# ---------------------------------------------------------------------------------------------------------------------
def _gat_model_inputs():
    rng = np.random.Generator(np.random.PCG64(311))
    n, f, classes = 2708, 1433, 7
    ei = directed_pairs(rng, n, 10556)
    x = (rng.random((n, f)) < 0.012).astype(np.float32)
    x = x / np.maximum(x.sum(1, keepdims=True), 1.0)
    return dict(n=n, f=f, x=x, ei=ei, classes=classes,
                w0=dict(query_kernel=glorot(rng, f, 8), query_bias=small_bias(rng, 8), key_kernel=glorot(rng, f, 8),
                        key_bias=small_bias(rng, 8), kernel=glorot(rng, f, 64), bias=small_bias(rng, 64)),
                w1=dict(query_kernel=glorot(rng, 64, 1), query_bias=small_bias(rng, 1), key_kernel=glorot(rng, 64, 1),
                        key_bias=small_bias(rng, 1), kernel=glorot(rng, 64, classes), bias=small_bias(rng, classes)))


def _gat_model_ref(R, g):
    tf, tfg = R.tf, R.tfg

    class GATModel(tf.keras.Model):                   # demo/demo_gat.py:18-42, verbatim structure

        def __init__(self, *args, **kwargs):
            super().__init__(*args, **kwargs)
            self.gat0 = tfg.layers.GAT(64, activation=tf.nn.relu, num_heads=8, attention_units=8, edge_drop_rate=0.6)
            self.gat1 = tfg.layers.GAT(g["classes"], num_heads=1, attention_units=1, edge_drop_rate=0.6)
            self.dropout = tf.keras.layers.Dropout(0.6)

        def call(self, inputs, training=None, mask=None, cache=None):
            x, edge_index = inputs
            h = self.dropout(x, training=training)
            h = self.gat0([h, edge_index], training=training)
            self.hidden = h
            h = self.dropout(h, training=training)
            h = self.gat1([h, edge_index], training=training)
            return h

    model = GATModel()
    model([g["x"], g["ei"]])
    for layer, ws in ((model.gat0, g["w0"]), (model.gat1, g["w1"])):
        for k, v in ws.items():
            getattr(layer, k).assign(v)
    logits = model([g["x"], g["ei"]], training=False)
    return {"hidden": _np(model.hidden), "logits": _np(logits)}


def _gat_model_orc(o, g):
    a, b = g["w0"], g["w1"]
    h = o.gat(g["x"], g["ei"], a["query_kernel"], a["query_bias"], "relu", a["key_kernel"], a["key_bias"], "relu",
              a["kernel"], a["bias"], "relu", num_heads=8)
    out = o.gat(h, g["ei"], b["query_kernel"], b["query_bias"], "relu", b["key_kernel"], b["key_bias"], "relu",
                b["kernel"], b["bias"], None, num_heads=1)
    return {"hidden": h, "logits": out}


def _gat_model_hip(T, g):
    gat0 = T.layers.GAT(64, activation=T.relu, num_heads=8, attention_units=8, edge_drop_rate=0.6)
    gat1 = T.layers.GAT(g["classes"], num_heads=1, attention_units=1, edge_drop_rate=0.6)
    x = T._lib.as_f32(g["x"])
    gat0._maybe_build([x])
    gat0.set_weights(**g["w0"])
    h = gat0([x, g["ei"]], training=False)
    gat1._maybe_build([h])
    gat1.set_weights(**g["w1"])
    return {"hidden": _np(h), "logits": _np(gat1([h, g["ei"]], training=False))}


_add("model_gat_cora", _gat_model_inputs, _gat_model_ref, _gat_model_orc, _gat_model_hip,
     note="the 2-layer GAT model of demo/demo_gat.py at Cora shape (8 heads x 8 attention units, then the d_head = 1 output layer)")


def _sampled_in_edges(rng, ei, n, k):
    """At most k incoming edges per destination, drawn without replacement, each weighted 1 / (number kept) — the shape of
    what RandomNeighborSampler.sample(k) returns (utils/graph_utils.py: sampled edge_index + edge_weight)."""
    order = np.argsort(ei[0], kind="stable")
    row, col = ei[0][order], ei[1][order]
    starts = np.searchsorted(row, np.arange(n + 1))
    keep_r, keep_c, keep_w = [], [], []
    for r in range(n):
        nb = col[starts[r]:starts[r + 1]]
        if nb.size > k:
            nb = rng.permutation(nb)[:k]
        if nb.size:
            keep_r.append(np.full(nb.size, r, np.int32))
            keep_c.append(nb.astype(np.int32))
            keep_w.append(np.full(nb.size, 1.0 / nb.size, np.float32))
    return np.stack([np.concatenate(keep_r), np.concatenate(keep_c)]), np.concatenate(keep_w)


def _sage_model_inputs():
    rng = np.random.Generator(np.random.PCG64(312))
    n, f, units, classes = 1500, 50, 256, 121
    ei = directed_pairs(rng, n, 45000)
    x = rng.standard_normal((n, f), dtype=np.float32)
    e25, w25 = _sampled_in_edges(rng, ei, n, 25)
    e10, w10 = _sampled_in_edges(rng, ei, n, 10)
    return dict(n=n, f=f, x=x, units=units, classes=classes, e25=e25, w25=w25, e10=e10, w10=w10,
                s0=dict(self_kernel=glorot(rng, f, units // 2), neighbor_kernel=glorot(rng, f, units // 2),
                        bias=small_bias(rng, units)),
                s1=dict(self_kernel=glorot(rng, units, units // 2), neighbor_kernel=glorot(rng, units, units // 2),
                        bias=small_bias(rng, units)),
                dk=glorot(rng, units, classes), db=small_bias(rng, classes))


def _sage_model_ref(R, g):
    tf, tfg = R.tf, R.tfg
    sages = [tfg.layers.MeanGraphSage(units=g["units"], activation=tf.nn.relu, concat=True),       # demo_graph_sage.py:29-30
             tfg.layers.MeanGraphSage(units=g["units"], activation=tf.nn.relu, concat=True)]
    lists = [(g["e25"], g["w25"]), (g["e10"], g["w10"])]                                            # :47, :53-55
    for run in range(2):
        h = g["x"]
        for sage, (e_s, w_s), ws in zip(sages, lists, (g["s0"], g["s1"])):
            if run == 1:
                for k, v in ws.items():
                    getattr(sage, k).assign(v)
            h = sage([h, e_s, w_s], training=False)
    logits = _np(h) @ g["dk"] + g["db"]              # tf.keras.layers.Dense(num_classes), :44 — a plain affine map
    return {"hidden": _np(h), "logits": logits.astype(np.float32)}


def _sage_model_orc(o, g):
    h = g["x"]
    for (e_s, w_s), ws in zip([(g["e25"], g["w25"]), (g["e10"], g["w10"])], (g["s0"], g["s1"])):
        h = o.mean_graph_sage(h, e_s, w_s, ws["self_kernel"], ws["neighbor_kernel"], ws["bias"], "relu", concat=True)
    return {"hidden": h, "logits": (h.astype(np.float64) @ g["dk"] + g["db"]).astype(np.float32)}


def _sage_model_hip(T, g):
    h = T._lib.as_f32(g["x"])
    for (e_s, w_s), ws in zip([(g["e25"], g["w25"]), (g["e10"], g["w10"])], (g["s0"], g["s1"])):
        sage = T.layers.MeanGraphSage(units=g["units"], activation=T.relu, concat=True)
        sage._maybe_build([h])
        sage.set_weights(**ws)
        h = sage([h, e_s, w_s], training=False)
    from tf_geometric_amd.plan import gemm_bias_act
    return {"hidden": _np(h), "logits": _np(gemm_bias_act(h, T._lib.as_f32(g["dk"]), bias=T._lib.as_f32(g["db"])))}


_add("model_sage_sampled", _sage_model_inputs, _sage_model_ref, _sage_model_orc, _sage_model_hip,
     note="the sampled 2-layer MeanGraphSage model of demo/demo_graph_sage.py (25 / 10 sampled in-edges, weights 1 / kept)")


# ---------------------------------------------------------------------------------------------------------------------
# (f3) edge preprocessing — utils/graph_utils.py:14-212, 252-269 — index work, bit-exact
# ---------------------------------------------------------------------------------------------------------------------
def _edge_inputs():
    rng = np.random.Generator(np.random.PCG64(108))
    ei = rng.integers(0, 40, size=(2, 900), dtype=np.int32)        # many duplicates and self-loops
    w = rng.uniform(0.5, 1.5, 900).astype(np.float32)
    return dict(ei=ei, w=w, doc=np.array([[1, 3, 5], [2, 1, 4]], np.int32))


def _edge_run(U, g):
    out = {}
    d, _ = U.convert_edge_to_directed(g["doc"])
    out["doc_directed"] = _np(d)
    u, props = U.merge_duplicated_edge(g["ei"], [g["w"]] * 4, ["sum", "mean", "max", "min"])
    out["merged_index"] = _np(u)
    for m, p in zip(["sum", "mean", "max", "min"], props):
        out["merged_" + m] = _np(p)
    up, (uw,) = U.convert_edge_to_upper(g["ei"], [g["w"]])
    out["upper_index"], out["upper_w"] = _np(up), _np(uw)
    de, (dw,) = U.convert_edge_to_directed(g["ei"], [g["w"]])
    out["directed_index"], out["directed_w"] = _np(de), _np(dw)
    e2, w2 = U.remove_self_loop_edge(g["ei"], g["w"])
    out["noself_index"], out["noself_w"] = _np(e2), _np(w2)
    return out


_add("edge_preprocessing", _edge_inputs,
     lambda R, g: _edge_run(R.tfg.utils.graph_utils, g), None, lambda T, g: _edge_run(T.utils, g),
     exact=["doc_directed", "merged_index", "merged_max", "merged_min", "upper_index", "directed_index", "noself_index",
            "noself_w"])


def _gutil_inputs():
    g = sym_graph(90, 500, 4, seed=208)                              # undirected, no self-loops, weighted
    rng = np.random.Generator(np.random.PCG64(209))
    loops = graph(60, 400, 3, seed=210, self_loops=25)               # directed multigraph WITH self-loops and duplicates
    sampled_nodes = rng.permutation(90)[:40].astype(np.int32)
    sub = rng.integers(0, 90, size=(2, 300), dtype=np.int32)        # some endpoints were not sampled -> -1
    return dict(g=g, loops=loops, sampled_nodes=sampled_nodes, sub=sub)


def _gutil_run(U, d):
    g, lp = d["g"], d["loops"]
    out = {}
    for nt in ("sym", "rw", None):
        for tag, gg in (("sym_graph", g), ("loops", lp)):
            ei, w = U.get_laplacian(gg["ei"], gg["n"], gg["w"], nt, fill_weight=1.5 if tag == "loops" else 1.0)
            out["laplacian-{}-{}-index".format(nt, tag)], out["laplacian-{}-{}-w".format(nt, tag)] = _np(ei), _np(w)
    for asl in (False, True):
        ei, w = U.adj_norm_edge(lp["ei"], lp["n"], lp["w"], add_self_loop=asl)
        out["adj_norm-{}-index".format(asl)], out["adj_norm-{}-w".format(asl)] = _np(ei), _np(w)
    ei, w = U.adj_norm_edge(g["ei"], g["n"], None)
    out["adj_norm-unweighted-w"] = _np(w)
    cache = {}
    first = U.adj_norm_edge(g["ei"], g["n"], g["w"], cache=cache)
    again = U.adj_norm_edge(lp["ei"], lp["n"], lp["w"], cache=cache)          # the cache wins over the arguments (:916-920)
    out["adj_norm-cache-hit"] = np.array([_np(first[1]).shape[0] == _np(again[1]).shape[0], "adj_normed_edge" in cache])
    out["reindexed"] = _np(U.reindex_sampled_edge_index(d["sub"], d["sampled_nodes"]))
    out["lambda_max-sym"] = np.float32(U.LaplacianMaxEigenvalue(g["ei"], g["n"], g["w"])("sym"))
    out["lambda_max-unweighted-sym"] = np.float32(U.LaplacianMaxEigenvalue(g["ei"], g["n"], None)("sym"))
    return out


_add("graph_utils_laplacian_reindex", _gutil_inputs,
     lambda R, d: _gutil_run(R.tfg.utils.graph_utils, d), None, lambda T, d: _gutil_run(T.utils, d),
     exact=["reindexed", "adj_norm-cache-hit"] + ["laplacian-{}-{}-index".format(nt, t) for nt in ("sym", "rw", None)
                                                  for t in ("sym_graph", "loops")]
           + ["adj_norm-{}-index".format(a) for a in (False, True)])


# ---------------------------------------------------------------------------------------------------------------------
# (f2) the other SpMM-shaped convolutions — nn/conv/{sgc,tagcn,appnp,ssgc,chebynet,gin,le_conv}.py
# ---------------------------------------------------------------------------------------------------------------------
def _prop_inputs():
    g = sym_graph(140, 700, 14, seed=109)
    rng = g["rng"]
    g.update(k9=glorot(rng, 14, 9), b9=small_bias(rng, 9), tk=glorot(rng, 14 * 4, 7), tb=small_bias(rng, 7),
             ks=[glorot(rng, 14, 16), glorot(rng, 16, 6)], bs=[small_bias(rng, 16), small_bias(rng, 6)],
             ck=[glorot(rng, 14, 5) for _ in range(3)], cb=small_bias(rng, 5),
             lk=[glorot(rng, 14, 6) for _ in range(3)], lb=[small_bias(rng, 6) for _ in range(3)],
             gin_w=glorot(rng, 14, 8))
    g.update(kw30=glorot(rng, 14, 30), bw30=small_bias(rng, 30))      # drawn last: earlier arrays keep their values
    return g


def _prop_ref(R, g):
    nn, relu = R.tfg.nn, R.tf.nn.relu
    x, ei, w = g["x"], g["ei"], g["w"]
    out = {}
    for k in (1, 3):
        out["sgc-k{}".format(k)] = _np(nn.sgc(x, ei, w, k, g["k9"], g["b9"], relu))
    out["sgc-widening"] = _np(nn.sgc(x, ei, w, 2, g["kw30"], g["bw30"], relu))
    out["tagcn"] = _np(nn.tagcn(x, ei, w, 3, g["tk"], g["tb"], relu))
    out["appnp"] = _np(nn.appnp(x, ei, w, g["ks"], g["bs"], relu, None, k=6, alpha=0.15))
    out["ssgc"] = _np(nn.ssgc(x, ei, w, g["ks"], g["bs"], k=5, alpha=0.2))
    out["ssgc-plain"] = _np(nn.ssgc(x, ei, None, None, None, k=4))
    for norm in ("sym", "rw", None):
        out["chebynet-{}".format(norm)] = _np(nn.chebynet(x, ei, w, 3, g["ck"], g["cb"], relu, norm))
    out["chebynet-sym-dynamic"] = _np(nn.chebynet(x, ei, w, 3, g["ck"], g["cb"], relu, "sym", use_dynamic_lambda_max=True))
    out["lambda_max-sym"] = np.float32(R.tfg.utils.graph_utils.LaplacianMaxEigenvalue(ei, g["n"], w)("sym"))
    out["lambda_max-None"] = np.float32(R.tfg.utils.graph_utils.LaplacianMaxEigenvalue(ei, g["n"], w)(None))
    mlp = lambda h, training=None: relu(h @ g["gin_w"])      # noqa: E731
    out["gin"] = _np(nn.gin(x, ei, mlp, eps=0.3))
    out["le_conv"] = _np(nn.le_conv(x, ei, w, g["lk"][0], g["lb"][0], g["lk"][1], g["lb"][1], g["lk"][2], g["lb"][2],
                                    relu))
    return out


def _prop_orc(o, g):
    x, ei, w = g["x"], g["ei"], g["w"]
    out = {}
    for k in (1, 3):
        out["sgc-k{}".format(k)] = o.sgc(x, ei, w, k, g["k9"], g["b9"], "relu")
    out["sgc-widening"] = o.sgc(x, ei, w, 2, g["kw30"], g["bw30"], "relu")
    out["tagcn"] = o.tagcn(x, ei, w, 3, g["tk"], g["tb"], "relu")
    out["appnp"] = o.appnp(x, ei, w, g["ks"], g["bs"], "relu", None, k=6, alpha=0.15)
    out["ssgc"] = o.ssgc(x, ei, w, g["ks"], g["bs"], k=5, alpha=0.2)
    out["ssgc-plain"] = o.ssgc(x, ei, None, None, None, k=4)
    for norm in ("sym", "rw", None):
        out["chebynet-{}".format(norm)] = o.chebynet(x, ei, w, 3, g["ck"], g["cb"], "relu", norm)
    out["chebynet-sym-dynamic"] = o.chebynet(x, ei, w, 3, g["ck"], g["cb"], "relu", "sym", use_dynamic_lambda_max=True)
    out["lambda_max-sym"] = np.float32(o.laplacian_max_eigenvalue(ei, g["n"], w, "sym"))
    out["lambda_max-None"] = np.float32(o.laplacian_max_eigenvalue(ei, g["n"], w, None))
    out["gin"] = np.maximum(o.matmul(o.gin(x, ei, lambda h: h, eps=0.3), g["gin_w"]), 0)
    out["le_conv"] = o.le_conv(x, ei, w, g["lk"][0], g["lb"][0], g["lk"][1], g["lb"][1], g["lk"][2], g["lb"][2], "relu")
    return out


def _prop_hip(T, g):
    import torch
    nn, relu = T.nn, T.relu
    x, ei, w = g["x"], g["ei"], g["w"]
    out = {}
    for k in (1, 3):
        out["sgc-k{}".format(k)] = _np(nn.sgc(x, ei, w, k, g["k9"], g["b9"], relu))
    out["sgc-widening"] = _np(nn.sgc(x, ei, w, 2, g["kw30"], g["bw30"], relu))
    out["tagcn"] = _np(nn.tagcn(x, ei, w, 3, g["tk"], g["tb"], relu))
    out["appnp"] = _np(nn.appnp(x, ei, w, g["ks"], g["bs"], relu, None, k=6, alpha=0.15))
    out["ssgc"] = _np(nn.ssgc(x, ei, w, g["ks"], g["bs"], k=5, alpha=0.2))
    out["ssgc-plain"] = _np(nn.ssgc(x, ei, None, None, None, k=4))
    for norm in ("sym", "rw", None):
        out["chebynet-{}".format(norm)] = _np(nn.chebynet(x, ei, w, 3, g["ck"], g["cb"], relu, norm))
    out["chebynet-sym-dynamic"] = _np(nn.chebynet(x, ei, w, 3, g["ck"], g["cb"], relu, "sym", use_dynamic_lambda_max=True))
    from tf_geometric_amd.nn.conv.propagation import chebynet_norm_edge, laplacian_max_eigenvalue
    for nt in ("sym", None):       # the unscaled Laplacian: chebynet_norm_edge with lambda_max = 2 has scale 1
        out["lambda_max-{}".format(nt)] = np.float32(laplacian_max_eigenvalue(chebynet_norm_edge(ei, g["n"], w, nt), nt))
    gw = T._lib.as_f32(g["gin_w"])
    out["gin"] = _np(nn.gin(x, ei, lambda h, training=None: torch.relu(h @ gw), eps=0.3))
    out["le_conv"] = _np(nn.le_conv(x, ei, w, g["lk"][0], g["lb"][0], g["lk"][1], g["lb"][1], g["lk"][2], g["lb"][2],
                                    relu))
    return out


_add("propagation_convs", _prop_inputs, _prop_ref, _prop_orc, _prop_hip, key_tol={"chebynet-None": 2e-4},
     note="ONE widened output: chebynet(normalization_type=None) applies the UN-normalised Laplacian twice — terms of "
          "magnitude 1e4 cancel, and the reference's OWN fp32 output is 8x the 1e-5 band away from the float64 value "
          "(tests/test_oracle_vs_reference.py::test_the_one_widened_tolerance_is_inherent_to_fp32).  Everything else, "
          "k-hop chains included, is held to the plain band (round 2's blanket 2e-5 was not needed: the HIP path sits at "
          "<= 0.11 of the band on every other output, profiles/r03_golden_margin.jsonl)")


# ---------------------------------------------------------------------------------------------------------------------
# (f4) readouts + topk_pool — nn/pool/common_pool.py:7-52, nn/pool/topk_pool.py:6-87
# ---------------------------------------------------------------------------------------------------------------------
def _pool_inputs():
    rng = np.random.Generator(np.random.PCG64(110))
    x = rng.standard_normal((700, 9), dtype=np.float32)
    gid = np.sort(rng.integers(0, 30, size=700, dtype=np.int32))
    gid[gid == 20] = 21                                             # graph 20 is empty
    score = rng.standard_normal(700).astype(np.float32)
    score[::50] = score[1::50]                                       # ties
    return dict(x=x, gid=gid, score=score)


def _pool_run(nn, g):
    out = {}
    for name in ("sum", "mean", "max", "min"):
        out[name] = _np(getattr(nn, name + "_pool")(g["x"], g["gid"], 33))
        out[name + "-default"] = _np(getattr(nn, name + "_pool")(g["x"], g["gid"]))
    out["topk-k5"] = _np(nn.topk_pool(g["gid"], g["score"], k=5))
    out["topk-ratio"] = _np(nn.topk_pool(g["gid"], g["score"], ratio=0.3))
    return out


_add("pooling", _pool_inputs, lambda R, g: _pool_run(R.tfg.nn, g), None, lambda T, g: _pool_run(T.nn, g),
     exact=["max", "min", "max-default", "min-default", "topk-k5", "topk-ratio"])


# ---------------------------------------------------------------------------------------------------------------------
# segment_op_with_pad — nn/kernel/segment.py:5-23 (the TF1 route of max_reducer / max_pool / min_pool: a SORTED segment op
# on rows sorted by id, zero rows appended up to num_segments)
# ---------------------------------------------------------------------------------------------------------------------
def _pad_inputs():
    rng = np.random.Generator(np.random.PCG64(120))
    ids = rng.integers(0, 40, size=900, dtype=np.int32)             # unsorted; ids 7 and 23 never occur, 40..44 are padding
    ids[ids == 7] = 8
    ids[ids == 23] = 22
    x = rng.standard_normal((900, 6), dtype=np.float32)
    x[::37] = x[1::37][:x[::37].shape[0]]                            # ties
    return dict(x=x, ids=ids, v=rng.standard_normal(900).astype(np.float32))


def _pad_run(pad, op_of, g):
    out = {}
    for kind in ("sum", "mean", "max", "min"):
        out[kind] = _np(pad(op_of(kind), g["x"], g["ids"], 45))
        out[kind + "-1d"] = _np(pad(op_of(kind), g["v"], g["ids"], 41))
    return out


def _pad_orc(o, g):
    import functools
    return _pad_run(o.segment_op_with_pad, lambda k: functools.partial(o.sorted_segment, k), g)


_add("segment_op_with_pad", _pad_inputs,
     lambda R, g: _pad_run(R.tfg.nn.kernel.segment.segment_op_with_pad, lambda k: getattr(R.tf.math, "segment_" + k), g),
     _pad_orc,
     lambda T, g: _pad_run(T.nn.kernel.segment.segment_op_with_pad, lambda k: getattr(T.nn.kernel.segment, "segment_" + k), g),
     exact=["max", "min", "max-1d", "min-1d"])


# ---------------------------------------------------------------------------------------------------------------------
# fuzz: the core hot-path functions on six more seeded graphs each (sizes, widths, head counts, normalisation configs
# and graph irregularities vary with the seed) — reference outputs in the same golden file
# ---------------------------------------------------------------------------------------------------------------------
def _fuzz_inputs(seed):
    def make():
        g = graph(80 + 37 * seed, 700 + 260 * seed, 8 + 4 * seed, seed=500 + seed, self_loops=2 * seed,
                  isolated=(seed * 3) % 5)
        rng, f = g["rng"], g["f"]
        u = 6 + 2 * seed
        H = [1, 2, 4, 8, 2, 4][seed]
        A, U = H * (1 + seed % 3), H * (2 + seed % 2)
        g.update(kernel=glorot(rng, f, u), bias=small_bias(rng, u), cfg=NORM_CFGS[(seed * 2 + 1) % len(NORM_CFGS)], H=H,
                 wq=glorot(rng, f, A), bq=small_bias(rng, A), wk=glorot(rng, f, A), bk=small_bias(rng, A),
                 wv=glorot(rng, f, U), b=small_bias(rng, U), ws=glorot(rng, f, u), wn=glorot(rng, f, u),
                 b2=small_bias(rng, 2 * u), normalize=bool(seed % 2))
        return g
    return make


def _fuzz_run(nn, adj_of, gcn_mapper, act, g):
    out = {}
    x, ei, w = g["x"], g["ei"], g["w"]
    for red in ("sum", "mean", "max"):
        out["agg-" + red] = _np(nn.aggregate_neighbors(x, ei, w, gcn_mapper, getattr(nn, red + "_reducer"),
                                                       nn.identity_updater))
    out["gcn"] = _np(nn.gcn(x, adj_of(g), g["kernel"], g["bias"], activation=act, **g["cfg"]))
    out["gat"] = _np(nn.gat(x, ei, g["wq"], g["bq"], act, g["wk"], g["bk"], act, g["wv"], g["b"], act, num_heads=g["H"]))
    for name in ("mean", "sum"):
        out["sage-" + name] = _np(getattr(nn, name + "_graph_sage")(x, ei, w, g["ws"], g["wn"], g["b2"], act,
                                                                    normalize=g["normalize"]))
    return out


def _fuzz_orc(o, g):
    out = {}
    x, ei, w = g["x"], g["ei"], g["w"]
    for red in ("sum", "mean", "max"):
        out["agg-" + red] = o.aggregate_neighbors(x, ei, w, o.gcn_mapper, getattr(o, red + "_reducer"), o.identity_updater)
    out["gcn"] = o.gcn(x, ei, w, g["kernel"], g["bias"], "relu", **g["cfg"])
    out["gat"] = o.gat(x, ei, g["wq"], g["bq"], "relu", g["wk"], g["bk"], "relu", g["wv"], g["b"], "relu", num_heads=g["H"])
    for name in ("mean", "sum"):
        out["sage-" + name] = getattr(o, name + "_graph_sage")(x, ei, w, g["ws"], g["wn"], g["b2"], "relu",
                                                               normalize=g["normalize"])
    return out


for _seed in range(6):
    _add("fuzz-{}".format(_seed), _fuzz_inputs(_seed),
         lambda R, g: _fuzz_run(R.tfg.nn, lambda g_: R.tfs.SparseMatrix(g_["ei"], g_["w"], [g_["n"], g_["n"]]),
                                R.tfg.nn.conv.gcn.gcn_mapper, R.tf.nn.relu, g),
         _fuzz_orc,
         lambda T, g: _fuzz_run(T.nn, lambda g_: T.SparseMatrix(g_["ei"], g_["w"], [g_["n"], g_["n"]]), T.nn.gcn_mapper,
                                T.relu, g),
         exact=["agg-max"])


def by_name(name):
    for c in CASES:
        if c.name == name:
            return c
    raise KeyError(name)


# ---------------------------------------------------------------------------------------------------------------------
# checks that run the reference live where it exists; tests/golden/reference_checks.npz holds what it returned, so the
# same checks run on a machine without the reference checkout (tests/golden/make_golden_from_reference.py writes it)
# ---------------------------------------------------------------------------------------------------------------------
REFERENCE_FILES = ("nn/kernel/map_reduce.py", "nn/kernel/segment.py", "nn/conv/gcn.py", "nn/conv/gat.py",
                   "nn/conv/graph_sage.py", "utils/graph_utils.py", "layers/conv/gcn.py", "layers/conv/gat.py",
                   "layers/conv/graph_sage.py")
FUZZ_SEEDS = range(6)
NUM_SPLITS_F = (1, 7, 12, 100, 128, 602, 1433)
NUM_SPLITS_K = (None, 1, 2, 3, 4, 5, 7, 8, 16, 100)


def inputs_digest(value):
    """sha256 of a case's inputs (arrays by dtype, shape and bytes; generators by their state): names the exact inputs the
    committed golden vectors were computed from."""
    import hashlib
    import json
    h = hashlib.sha256()

    def walk(v):
        if isinstance(v, dict):
            h.update(b"{")
            for k in sorted(v):
                h.update(repr(k).encode())
                walk(v[k])
            h.update(b"}")
        elif isinstance(v, (list, tuple)):
            h.update(b"[")
            for x in v:
                walk(x)
            h.update(b"]")
        elif isinstance(v, np.ndarray):
            h.update("{}{}".format(v.dtype.str, v.shape).encode())
            h.update(np.ascontiguousarray(v).tobytes())
        elif isinstance(v, np.random.Generator):
            h.update(json.dumps(v.bit_generator.state, sort_keys=True).encode())
        else:
            h.update(repr(v).encode())
    walk(value)
    return h.hexdigest()


def fuzz_check_inputs(seed):
    """Fresh graph (duplicates, self-loops, isolated nodes) and parameters of one seed of the oracle-vs-live-reference fuzz."""
    g = graph(60 + 17 * seed, 400 + 90 * seed, 5 + seed, seed=900 + seed, self_loops=seed, isolated=seed % 3)
    rng = g["rng"]
    f, u = g["x"].shape[1], 4 + seed
    p = dict(g, f=f, u=u, cfg=NORM_CFGS[seed % len(NORM_CFGS)], normalize=bool(seed % 2))
    p["kernel"], p["bias"] = glorot(rng, f, u), small_bias(rng, u)
    H = [1, 2, 4, 8, 2, 4][seed]
    A, U = H * (1 + seed % 3), H * 3
    p["H"] = H
    p["wq"], p["wk"], p["wv"] = glorot(rng, f, A), glorot(rng, f, A), glorot(rng, f, U)
    p["bq"], p["bk"], p["b"] = small_bias(rng, A), small_bias(rng, A), small_bias(rng, U)
    p["ws"], p["wn"], p["b2"] = glorot(rng, f, u), glorot(rng, f, u), small_bias(rng, 2 * u)
    p["s"] = (rng.standard_normal(g["ei"].shape[1]) * 4).astype(np.float32)
    return p


def fuzz_check_ref(R, p):
    nn, tf = R.tfg.nn, R.tf
    x, ei, w, n = p["x"], p["ei"], p["w"], p["n"]
    out = {}
    for red in ("sum", "mean", "max"):
        out["aggregate-" + red] = nn.aggregate_neighbors(x, ei, w, R.tfg.nn.conv.gcn.gcn_mapper, getattr(nn, red + "_reducer"),
                                                         nn.identity_updater).numpy()
    adj = R.tfs.SparseMatrix(ei, w, [n, n])
    out["gcn"] = nn.gcn(x, adj, p["kernel"], p["bias"], activation=tf.nn.relu, **p["cfg"]).numpy()
    out["gat"] = nn.gat(x, ei, p["wq"], p["bq"], tf.nn.relu, p["wk"], p["bk"], tf.nn.relu, p["wv"], p["b"], tf.nn.relu,
                        num_heads=p["H"]).numpy()
    for name in ("mean", "sum"):
        out[name + "-sage"] = getattr(nn, name + "_graph_sage")(x, ei, w, p["ws"], p["wn"], p["b2"], tf.nn.relu,
                                                                normalize=p["normalize"]).numpy()
    out["segment_softmax"] = R.tfg.nn.kernel.segment.segment_softmax(p["s"], ei[0], n).numpy()
    return out


def fuzz_check_orc(o, p):
    x, ei, w, n = p["x"], p["ei"], p["w"], p["n"]
    out = {}
    for red in ("sum", "mean", "max"):
        out["aggregate-" + red] = o.aggregate_neighbors(x, ei, w, o.gcn_mapper, getattr(o, red + "_reducer"),
                                                        o.identity_updater)
    out["gcn"] = o.gcn(x, ei, w, p["kernel"], p["bias"], "relu", **p["cfg"])
    out["gat"] = o.gat(x, ei, p["wq"], p["bq"], "relu", p["wk"], p["bk"], "relu", p["wv"], p["b"], "relu", num_heads=p["H"])
    for name in ("mean", "sum"):
        out[name + "-sage"] = getattr(o, name + "_graph_sage")(x, ei, w, p["ws"], p["wn"], p["b2"], "relu",
                                                               normalize=p["normalize"])
    out["segment_softmax"] = o.segment_softmax(p["s"], ei[0], n)
    return out


def num_splits_table(fn):
    """[[f, k, split sizes or "raises"], ...] of compute_num_or_size_splits over the grid."""
    rows = []
    for f in NUM_SPLITS_F:
        for k in NUM_SPLITS_K:
            try:
                got = fn(f, k)
            except Exception:
                got = "raises"
            if isinstance(got, (list, tuple)):
                got = [int(v) for v in got]
            elif got is not None and not isinstance(got, str):
                got = int(got)
            rows.append([f, k, got])
    return rows


def check_loaded_unmodified(tfg, root):
    """The package the harness loaded is the one under `root`, and each of REFERENCE_FILES is imported byte for byte as
    it lies on disk there."""
    import hashlib
    import importlib
    import os
    assert os.path.realpath(tfg.__file__).startswith(os.path.realpath(root)), tfg.__file__
    for rel in REFERENCE_FILES:
        m = importlib.import_module("tf_geometric." + rel[:-3].replace("/", "."))
        with open(os.path.join(root, "tf_geometric", rel), "rb") as f:
            on_disk = hashlib.sha1(f.read()).hexdigest()
        with open(m.__file__, "rb") as f:
            assert hashlib.sha1(f.read()).hexdigest() == on_disk, rel
