# coding=utf-8
"""Parity cases of DiffPool and MinCutPool (reference: nn/pool/diff_pool.py:8-105, nn/pool/min_cut_pool.py:18-232).

Same two executors as tests/asap_cases.py: ``ref`` runs the reference's own Python, unmodified (written into
tests/golden/densepool_cases.npz by tests/golden/make_densepool_golden.py; re-run live by tests/test_densepool_reference.py
where the reference checkout exists), ``hip`` runs the product (tests/test_gpu_densepool.py).  The two GNNs are GCN layers with
fixed weights.

On the numpy stand-ins for TensorFlow the two coarsen functions and diff_pool run as they are.  The LOSS needs three adapters
ON THE STAND-INS (``install_adapters``; nothing in the reference and nothing under oracle/ changes; with real TensorFlow none
is installed):
  1. ``SparseTensor.__mul__(dense)``: the values times ``dense`` at the indices (min_cut_pool.py:11);
  2. ``tf.eye(..., batch_shape=)`` (min_cut_pool.py:86);
  3. ``tf.norm`` taking a list for ``axis`` (min_cut_pool.py:82, :89).

The batch: five graphs, node_graph_index unsorted, one graph without edges, one single-node graph, a node without edges
inside a graph that has some; no self-loops, no duplicate edges (tf.sparse.to_dense of the loss does not add duplicates up)
and no edge between two graphs.  The set of non-zero pooled entries must not be a float32 accident: edge weights in
[0.5, 1.5], |logits| <= 4 (checked by the generator), so every in-block entry of a graph that has an edge is far from zero
(``checks``: at least 1e-12 is the generator's condition)."""
import numpy as np

import densepool_mirror as dm

TOL = 1e-5
MAX_LOGIT = 4.0
MIN_ENTRY = 1e-12
K = 3
UNITS = 5
SIZES = [5, 1, 4, 7, 3]          # graph 1: a single node; graph 2: no edges
EDGELESS = (1, 2)


class Case(object):
    def __init__(self, name, inputs, ref, hip, configs):
        self.name, self.inputs, self.ref, self.hip, self.configs = name, inputs, ref, hip, configs

    def __repr__(self):
        return "Case({})".format(self.name)


def _np(t):
    if t is None:
        return None
    if hasattr(t, "detach"):
        t = t.detach().cpu()
    return np.asarray(t)


def batch(seed=3, f=6):
    rng = np.random.Generator(np.random.PCG64(seed))
    n = int(sum(SIZES))
    gid_sorted = np.repeat(np.arange(len(SIZES)), SIZES)
    place = rng.permutation(n)                       # sorted position -> node id
    gid = np.empty(n, np.int32)
    gid[place] = gid_sorted
    start = np.concatenate([[0], np.cumsum(SIZES)])
    edges = []
    for g, size in enumerate(SIZES):
        if g in EDGELESS or size < 2:
            continue
        members = place[start[g]:start[g + 1]][:size - 1] if size > 4 else place[start[g]:start[g + 1]]    # one isolated node
        pairs = [(a, b) for a in members for b in members if a != b]
        pick = rng.choice(len(pairs), size=min(len(pairs), 2 * len(members)), replace=False)
        for p in pick:
            edges.append(pairs[p])
        edges.append((pairs[pick[0]][1], pairs[pick[0]][0]))          # at least one edge in both directions
    edges = sorted(set((int(a), int(b)) for a, b in edges))
    ei = np.asarray(edges, np.int32)[rng.permutation(len(edges))].T.copy()
    g = dict(n=n, f=f, ei=ei, gid=gid,
             x=rng.uniform(-1, 1, (n, f)).astype(np.float32),
             w=rng.uniform(0.5, 1.5, ei.shape[1]).astype(np.float32),
             assign_kernel=(rng.uniform(-1, 1, (f, K)) * 1.5).astype(np.float32),
             assign_bias=rng.uniform(-0.5, 0.5, K).astype(np.float32),
             feature_kernel=(rng.uniform(-1, 1, (f, UNITS)) * np.sqrt(6.0 / (f + UNITS))).astype(np.float32),
             feature_bias=rng.uniform(-0.3, 0.3, UNITS).astype(np.float32),
             bias=rng.uniform(-0.3, 0.3, UNITS).astype(np.float32))
    logits = rng.uniform(-MAX_LOGIT, MAX_LOGIT, (n, K)).astype(np.float32)
    ex = np.exp(logits - logits.max(axis=1, keepdims=True))
    g["assign"] = (ex / ex.sum(axis=1, keepdims=True)).astype(np.float32)
    return g


# (name, weighted, bias, activation)
DIFF_CONFIGS = [("w-bias-relu", True, True, "relu"), ("now-plain", False, False, None)]
# (name, weighted, bias, gnn_use_normed_edge)
MINCUT_CONFIGS = [("w-normed-bias", True, True, True), ("now-raw", False, False, False)]
COARSEN_CONFIGS = [("w", True), ("now", False)]


def checks(g):
    """(largest |assign logit| of any configuration, smallest in-block pooled entry of a graph that has an edge), from the
    float64 mirror: the generator's two conditions."""
    big, small = 0.0, np.inf
    has_edge = np.setdiff1d(np.arange(len(SIZES)), EDGELESS)
    blocks = lambda P: [P[q * K:(q + 1) * K, q * K:(q + 1) * K].abs().min().item() for q in has_edge]     # noqa: E731
    fg, ag = (g["feature_kernel"], g["feature_bias"]), (g["assign_kernel"], g["assign_bias"])
    for _, weighted, _, _ in DIFF_CONFIGS:
        m = dm.diff_pool_mirror(g["x"], g["ei"], g["w"] if weighted else None, g["gid"], _f64(fg), _f64(ag))
        big, small = max(big, m["logits"].abs().max().item()), min([small] + blocks(m["P"]))
    for _, weighted, _, normed in MINCUT_CONFIGS:
        m = dm.min_cut_pool_mirror(g["x"], g["ei"], g["w"] if weighted else None, g["gid"], _f64(fg), _f64(ag),
                                   gnn_use_normed_edge=normed)
        big, small = max(big, m["logits"].abs().max().item()), min([small] + blocks(m["P"]))
    for _, weighted in COARSEN_CONFIGS:
        w = g["w"] if weighted else None
        small = min([small] + blocks(dm.diff_pool_coarsen_mirror(g["x"], g["ei"], w, g["gid"], g["assign"])["P"]))
        small = min([small] + blocks(dm.min_cut_pool_coarsen_mirror(g["x"], g["ei"], w, g["gid"], g["assign"])["P"]))
    return big, small


def _f64(pair):
    import torch
    return tuple(torch.from_numpy(np.asarray(a)).double() for a in pair)


def install_adapters(R):
    """The three adapters of the module docstring, on the numpy stand-ins only."""
    tf = R.tf
    if getattr(tf, "_tfgx_densepool_adapters", False) or getattr(R, "backend", "numpy-stub") != "numpy-stub":
        return
    sparse_tensor = tf.SparseTensor

    def sparse_times_dense(self, dense):
        idx = np.asarray(self.indices)
        return sparse_tensor(idx, np.asarray(self.values) * np.asarray(dense)[tuple(idx.T)], self.dense_shape)

    plain_eye, plain_norm = tf.eye, tf.norm

    def eye(num_rows, num_columns=None, batch_shape=None, dtype=tf.float32):
        out = plain_eye(num_rows, num_columns, dtype=dtype)
        if batch_shape is None:
            return out
        lead = [int(b) for b in np.asarray(batch_shape).reshape(-1)]
        return tf.constant(np.broadcast_to(np.asarray(out), lead + list(out.shape)).copy())

    def norm(tensor, ord="euclidean", axis=None, keepdims=False):      # noqa: A002
        return plain_norm(tensor, ord=ord, axis=tuple(axis) if isinstance(axis, list) else axis, keepdims=keepdims)

    sparse_tensor.__mul__ = sparse_times_dense
    tf.eye, tf.norm = eye, norm
    tf._tfgx_densepool_adapters = True


def _outs(prefix, res):
    x, ei, w, gi = res
    return {prefix + "x": _np(x), prefix + "edge_index": _np(ei), prefix + "edge_weight": _np(w),
            prefix + "node_graph_index": _np(gi)}


def _loss_outs(prefix, losses):
    cut, orth = losses
    return {prefix + "cut_loss": np.asarray(_np(cut), np.float32).reshape(()),
            prefix + "orth_loss": np.asarray(_np(orth), np.float32).reshape(())}


def _ref_gcn(R, g, which):
    def gnn(inputs, training=None, cache=None):
        x, ei, w = inputs
        adj = R.tfs.SparseMatrix(ei, w, [g["n"], g["n"]])
        return R.tfg.nn.gcn(x, adj, g[which + "_kernel"], g[which + "_bias"], cache=cache)
    return gnn


def hip_gcn(tfg, g, which):
    layer = tfg.layers.GCN(int(g[which + "_kernel"].shape[1]))
    layer._maybe_build([g["x"]])
    layer.set_weights(kernel=g[which + "_kernel"], bias=g[which + "_bias"])
    return layer


def _run(nn, g, feature_gnn, assign_gnn, relu):
    out = {}
    for name, weighted, bias, act in DIFF_CONFIGS:
        res = nn.diff_pool(g["x"], g["ei"], g["w"] if weighted else None, g["gid"], feature_gnn, assign_gnn, K,
                           bias=g["bias"] if bias else None, activation=relu if act == "relu" else None)
        out.update(_outs("diff_pool/{}/".format(name), res))
    for name, weighted, bias, normed in MINCUT_CONFIGS:
        res, losses = nn.min_cut_pool(g["x"], g["ei"], g["w"] if weighted else None, g["gid"], feature_gnn, assign_gnn, K,
                                      bias=g["bias"] if bias else None, gnn_use_normed_edge=normed, return_losses=True)
        out.update(_outs("min_cut_pool/{}/".format(name), res))
        out.update(_loss_outs("min_cut_pool/{}/".format(name), losses))
    for name, weighted in COARSEN_CONFIGS:
        w = g["w"] if weighted else None
        out.update(_outs("diff_pool_coarsen/{}/".format(name), nn.diff_pool_coarsen(g["x"], g["ei"], w, g["gid"], g["assign"])))
        out.update(_outs("min_cut_pool_coarsen/{}/".format(name),
                         nn.min_cut_pool_coarsen(g["x"], g["ei"], w, g["gid"], g["assign"])))
        out.update(_loss_outs("min_cut_pool_compute_losses/{}/".format(name),
                              nn.min_cut_pool_compute_losses(g["ei"], w, g["gid"], g["assign"])))
    return out


def ref_all(R, g):
    install_adapters(R)
    return _run(R.tfg.nn, g, _ref_gcn(R, g, "feature"), _ref_gcn(R, g, "assign"), R.tf.nn.relu)


def hip_all(tfg, g):
    import torch
    return _run(tfg.nn, g, hip_gcn(tfg, g, "feature"), hip_gcn(tfg, g, "assign"), torch.relu)


ALL_CONFIGS = ([("diff_pool/" + c[0]) for c in DIFF_CONFIGS] + [("min_cut_pool/" + c[0]) for c in MINCUT_CONFIGS]
               + [("diff_pool_coarsen/" + c[0]) for c in COARSEN_CONFIGS]
               + [("min_cut_pool_coarsen/" + c[0]) for c in COARSEN_CONFIGS])
LOSS_CONFIGS = ([("min_cut_pool/" + c[0]) for c in MINCUT_CONFIGS]
                + [("min_cut_pool_compute_losses/" + c[0]) for c in COARSEN_CONFIGS])

CASES = [Case("densepool", batch, ref_all, hip_all, ALL_CONFIGS)]
