# coding=utf-8
"""Parity cases of the graph-coarsening layers: sag_pool, sort_pool and sample_new_graph_by_node_index
(reference: nn/pool/sag_pool.py:7-45, nn/pool/sort_pool.py:7-35, data/graph.py:276-359).

Same two executors per case as tests/reference_cases.py: ``ref`` runs the reference's own Python (written into
tests/golden/pool_cases.npz by tests/golden/make_pool_golden.py; re-run live by tests/test_pool_reference.py where the
reference checkout exists), ``hip`` runs the product (tests/test_gpu_pool.py).  Index outputs (edge_index,
node_graph_index), gathered edge weights and SortPool's gathered x are bit-exact; SAGPool's x is held to 1e-5 (the score
comes out of a GCN, or through tanh, whose last bit differs between math libraries).

The batch below is built to hit the corner cases: node_graph_index unsorted and gapped (graphs 1 and 4 have no nodes),
tied scores, self-loops, duplicate edges, edges across graphs, a graph that loses every edge, k larger than a graph."""
import numpy as np

TOL = 1e-5


class Case(object):
    def __init__(self, name, inputs, ref, hip, exact=(), tol=TOL):
        self.name, self.inputs, self.ref, self.hip, self.exact, self.tol = name, inputs, ref, hip, set(exact), tol

    def __repr__(self):
        return "Case({})".format(self.name)


CASES = []


def _add(*a, **k):
    CASES.append(Case(*a, **k))


def batch(seed=0, f=6):
    """A batch of 5 graph ids, 3 of them used (0, 2, 3; plus 5), nodes interleaved."""
    rng = np.random.Generator(np.random.PCG64(seed))
    sizes = {0: 7, 2: 2, 3: 9, 5: 5}           # graph 2 (2 nodes) is smaller than k = 3; ids 1 and 4 are gaps
    gid = np.concatenate([np.full(s, g, dtype=np.int32) for g, s in sizes.items()])
    gid = gid[rng.permutation(gid.size)]        # unsorted
    n = gid.size
    edges = []
    for g in sizes:
        nodes = np.flatnonzero(gid == g)
        for _ in range(2 * nodes.size):
            a, b = rng.choice(nodes, 2)
            edges.append((a, b))
    nodes0 = np.flatnonzero(gid == 0)
    edges += [(nodes0[0], nodes0[0]), (nodes0[1], nodes0[1])]           # self-loops
    edges += [edges[0], edges[3], edges[3]]                             # duplicates
    n5 = np.flatnonzero(gid == 5)
    n3 = np.flatnonzero(gid == 3)
    edges += [(n5[0], n3[0]), (n3[1], n5[1]), (nodes0[2], n3[2])]       # across graphs
    ei = np.asarray(edges, dtype=np.int32).T.copy()
    p = rng.permutation(ei.shape[1])
    ei = ei[:, p].copy()
    x = rng.standard_normal((n, f)).astype(np.float32)
    # ties: scores on a coarse grid.  Graph 5's top nodes are chosen so that no edge joins two of them (it loses every edge)
    score = (rng.integers(-3, 4, size=n) * 0.25).astype(np.float32)
    w = rng.uniform(0.5, 1.5, size=ei.shape[1]).astype(np.float32)
    x[:, 0] = np.round(x[:, 0] * 2.0) / 2.0                            # SortPool on column 0 sees ties as well
    kern = (rng.uniform(-1, 1, size=(f, 1)) * np.sqrt(6.0 / (f + 1))).astype(np.float32)
    bias = np.asarray([0.05], dtype=np.float32)
    keep5 = _isolate_top(ei, n5)
    score[n5] = -1.0
    score[keep5] = 1.0
    return dict(n=n, f=f, x=x, ei=ei, w=w, gid=gid, score=score.reshape(-1, 1), kernel=kern, bias=bias)


def _isolate_top(ei, nodes):
    """Nodes of `nodes` with no edge between any two of them (greedy independent set, at least one)."""
    chosen = []
    for v in nodes:
        ok = True
        for u in chosen:
            if ((ei[0] == u) & (ei[1] == v)).any() or ((ei[0] == v) & (ei[1] == u)).any():
                ok = False
        if ok and not ((ei[0] == v) & (ei[1] == v)).any():
            chosen.append(v)
    return np.asarray(chosen[:2], dtype=np.int64)


def _np(t):
    if t is None:
        return None
    if hasattr(t, "detach"):
        t = t.detach().cpu()
    return np.asarray(t)


def _outs(prefix, res):
    x, ei, w, gi = res
    out = {prefix + "x": _np(x), prefix + "edge_index": _np(ei), prefix + "node_graph_index": _np(gi)}
    if w is not None:
        out[prefix + "edge_weight"] = _np(w)
    return out


# ---- score functions: the reference's are TF / tf_sparse callables, the product's torch ones --------------------------
def _ref_fixed(R, g):
    return lambda inputs, training=None, cache=None: R.tf.constant(g["score"])


def _ref_gcn(R, g):
    def score(inputs, training=None, cache=None):
        x, ei, w = inputs
        adj = R.tfs.SparseMatrix(ei, w, [g["n"], g["n"]])
        return R.tfg.nn.gcn(x, adj, g["kernel"], g["bias"], cache=cache)
    return score


def _hip_fixed(tfg, g):
    import torch
    s = torch.from_numpy(g["score"]).cuda()
    return lambda inputs, training=None, cache=None: s


def _hip_gcn(tfg, g):
    layer = tfg.layers.GCN(1)
    layer._maybe_build([g["x"]])
    layer.set_weights(kernel=g["kernel"], bias=g["bias"])
    return layer


SAG_CONFIGS = [
    ("fixed-k3-tanh-w", "fixed", dict(k=3), "tanh", True),
    ("fixed-ratio-none-w", "fixed", dict(ratio=0.5), None, True),
    ("fixed-k3-none-now", "fixed", dict(k=3), None, False),
    ("gcn-ratio-tanh-w", "gcn", dict(ratio=0.5), "tanh", True),
    ("gcn-k2-tanh-now", "gcn", dict(k=2), "tanh", False),
    ("gcn-k20-none-w", "gcn", dict(k=20), None, True),            # k larger than every graph: keeps every node
]


def ref_sag(R, g):
    out = {}
    for name, fn, kr, act, weighted in SAG_CONFIGS:
        score = _ref_fixed(R, g) if fn == "fixed" else _ref_gcn(R, g)
        res = R.tfg.nn.sag_pool(g["x"], g["ei"], g["w"] if weighted else None, g["gid"], score,
                                score_activation=R.tf.nn.tanh if act == "tanh" else None, **kr)
        out.update(_outs(name + "/", res))
    return out


def hip_sag(tfg, g):
    import torch
    out = {}
    for name, fn, kr, act, weighted in SAG_CONFIGS:
        score = _hip_fixed(tfg, g) if fn == "fixed" else _hip_gcn(tfg, g)
        res = tfg.nn.sag_pool(g["x"], g["ei"], g["w"] if weighted else None, g["gid"], score,
                              score_activation=torch.tanh if act == "tanh" else None, **kr)
        out.update(_outs(name + "/", res))
    return out


_add("sag_pool", batch, ref_sag, hip_sag,
     exact=[c[0] + "/" + k for c in SAG_CONFIGS for k in ("edge_index", "node_graph_index", "edge_weight")]
     + [c[0] + "/x" for c in SAG_CONFIGS if c[1] == "fixed" and c[3] is None])     # tanh: libm ulps differ

SORT_CONFIGS = [("k3-last", dict(k=3), -1), ("ratio-col0", dict(ratio=0.5), 0), ("k4-col0-w", dict(k=4), 0)]


def ref_sort(R, g):
    out = {}
    for name, kr, si in SORT_CONFIGS:
        w = g["w"] if name.endswith("-w") else None
        out.update(_outs(name + "/", R.tfg.nn.sort_pool(g["x"], g["ei"], w, g["gid"], sort_index=si, **kr)))
    return out


def hip_sort(tfg, g):
    out = {}
    for name, kr, si in SORT_CONFIGS:
        w = g["w"] if name.endswith("-w") else None
        out.update(_outs(name + "/", tfg.nn.sort_pool(g["x"], g["ei"], w, g["gid"], sort_index=si, **kr)))
    return out


_add("sort_pool", batch, ref_sort, hip_sort,
     exact=[c[0] + "/" + k for c in SORT_CONFIGS for k in ("x", "edge_index", "node_graph_index", "edge_weight")])


def subgraph_inputs():
    g = batch(seed=3)
    rng = np.random.Generator(np.random.PCG64(11))
    g["sampled"] = rng.permutation(g["n"])[: g["n"] // 2 + 3].astype(np.int32)     # unsorted, arbitrary
    return g


def ref_subgraph(R, g):
    bg = R.tfg.BatchGraph(x=g["x"], edge_index=g["ei"], node_graph_index=g["gid"], edge_graph_index=None,
                          edge_weight=g["w"])
    sub = bg.sample_new_graph_by_node_index(g["sampled"])
    out = _outs("", (sub.x, sub.edge_index, sub.edge_weight, sub.node_graph_index))
    out["edge_mask"] = _np(R.tfg.utils.graph_utils.compute_edge_mask_by_node_index(g["ei"], g["sampled"]))
    return out


def hip_subgraph(tfg, g):
    res = tfg.utils.sample_new_graph_by_node_index(g["ei"], g["sampled"], x=g["x"], edge_weight=g["w"],
                                                   node_graph_index=g["gid"])
    out = _outs("", res)
    out["edge_mask"] = _np(tfg.utils.compute_edge_mask_by_node_index(g["ei"], g["sampled"]))
    return out


_add("sample_new_graph", subgraph_inputs, ref_subgraph, hip_subgraph,
     exact=["x", "edge_index", "edge_weight", "node_graph_index", "edge_mask"])
