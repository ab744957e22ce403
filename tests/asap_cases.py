# coding=utf-8
"""Parity cases of ASAP and cluster_pool (reference: nn/pool/asap.py:19-131, nn/pool/cluster_pool.py:9-46).

Same two executors per case as tests/pool_cases.py: ``ref`` runs the reference's own Python (written into
tests/golden/asap_cases.npz by tests/golden/make_asap_golden.py; re-run live by tests/test_asap_reference.py where the
reference checkout exists), ``hip`` runs the product (tests/test_gpu_asap.py).

The reference's asap() does not run as written against its own current code; the generator installs exactly two adapters on
its asap module and runs its body otherwise unmodified (``install_adapters``):
  1. ``gcn``: a wrapper with the argument order asap.py:54 uses (x, edge_index, edge_weight, kernel, bias, cache=) around the
     reference's own gcn(x, SparseMatrix, kernel, bias, cache=);
  2. ``cluster_pool``: swaps the two rows of assign_edge_index ([cluster; node] -> [node; cluster]) before the reference's own
     cluster_pool.

The batch is the one of tests/pool_cases.py: node_graph_index unsorted and gapped, self-loops, duplicate edges, edges across
graphs, k larger than a graph.  Edge weights are positive, so no pooled entry cancels to zero by re-association."""
import sys

import numpy as np

import pool_cases as pc
from asap_mirror import WEIGHT_NAMES, make_weights

TOL = 1e-5
MIN_SCORE_GAP = 1e-3          # adjacent sorted node scores inside a graph: the selection must not hang on a last bit


class Case(object):
    def __init__(self, name, inputs, ref, hip, configs):
        self.name, self.inputs, self.ref, self.hip, self.configs = name, inputs, ref, hip, configs

    def __repr__(self):
        return "Case({})".format(self.name)


CASES = []

# (name, k / ratio, le_conv_activation, weighted, attention units)
ASAP_CONFIGS = [
    ("ratio-sigmoid-w", dict(ratio=0.5), "sigmoid", True, 6),
    ("ratio-sigmoid-now", dict(ratio=0.5), "sigmoid", False, 6),
    ("k3-sigmoid-w", dict(k=3), "sigmoid", True, 6),
    ("k3-sigmoid-now", dict(k=3), "sigmoid", False, 6),
    ("ratio-none-w", dict(ratio=0.5), None, True, 6),
    ("k3-none-a4-now", dict(k=3), None, False, 4),           # attention_units != F
]
BATCH_SEED = 1            # pool_cases.batch(seed=0) holds a two-node graph whose nodes are structurally tied without weights
WEIGHT_SEED = 8


def asap_inputs():
    g = pc.batch(seed=BATCH_SEED)
    for cfg in ASAP_CONFIGS:
        rng = np.random.Generator(np.random.PCG64(WEIGHT_SEED + cfg[4]))
        for name, v in make_weights(rng, g["f"], cfg[4]).items():
            g["{}/{}".format(cfg[0], name)] = v
    return g


def config_weights(g, cfg_name):
    return [g["{}/{}".format(cfg_name, n)] for n in WEIGHT_NAMES]


def install_adapters(R):
    """The two adapters (see the module docstring) on the reference's asap module; returns that module."""
    mod = sys.modules["tf_geometric.nn.pool.asap"]
    if getattr(mod, "_tfgx_adapters", False):
        return mod
    ref_gcn, ref_cluster_pool = mod.gcn, mod.cluster_pool

    def gcn_old_signature(x, edge_index, edge_weight, kernel, bias=None, cache=None):
        n = int(np.shape(x)[0])
        return ref_gcn(x, R.tfs.SparseMatrix(edge_index, edge_weight, [n, n]), kernel, bias, cache=cache)

    def cluster_pool_node_first(x, edge_index, edge_weight, assign_edge_index, assign_edge_weight, num_clusters,
                                num_nodes=None):
        swapped = R.tf.stack([assign_edge_index[1], assign_edge_index[0]], axis=0)
        return ref_cluster_pool(x, edge_index, edge_weight, swapped, assign_edge_weight, num_clusters, num_nodes=num_nodes)

    mod.gcn, mod.cluster_pool = gcn_old_signature, cluster_pool_node_first
    mod._tfgx_adapters = True
    return mod


def _outs(prefix, res):
    x, ei, w, gi = res
    return {prefix + "x": pc._np(x), prefix + "edge_index": pc._np(ei), prefix + "edge_weight": pc._np(w),
            prefix + "node_graph_index": pc._np(gi)}


def ref_asap(R, g):
    mod = install_adapters(R)
    out = {}
    for name, kr, act, weighted, _ in ASAP_CONFIGS:
        res = mod.asap(g["x"], g["ei"], g["w"] if weighted else None, g["gid"], *config_weights(g, name), None,
                       le_conv_activation=R.tf.nn.sigmoid if act == "sigmoid" else None, **kr)
        out.update(_outs(name + "/", res))
    return out


def hip_asap(tfg, g):
    import torch
    out = {}
    for name, kr, act, weighted, _ in ASAP_CONFIGS:
        res = tfg.nn.asap(g["x"], g["ei"], g["w"] if weighted else None, g["gid"], *config_weights(g, name), None,
                          le_conv_activation=torch.sigmoid if act == "sigmoid" else None, **kr)
        out.update(_outs(name + "/", res))
    return out


CASES.append(Case("asap", asap_inputs, ref_asap, hip_asap, ASAP_CONFIGS))


# ---- cluster_pool --------------------------------------------------------------------------------------------------------
# (name, with x, assign weights: "w" | "zero" (one weight exactly 0.0: an entry must be dropped) | None, edge weights)
CLUSTER_CONFIGS = [("x-w", True, "w", True), ("x-zero", True, "zero", True), ("nox-w", False, "w", True),
                   ("x-ones", True, None, False)]


def cluster_inputs():
    g = pc.batch(seed=2)
    rng = np.random.Generator(np.random.PCG64(21))
    n, K = g["n"], 7
    node = np.concatenate([np.arange(n), rng.integers(0, n, 9)]).astype(np.int32)        # several clusters per node ...
    node = node[node != 4]                                                               # ... and a node in no cluster
    cluster = rng.integers(0, K - 1, node.size).astype(np.int32)                         # cluster K - 1 stays empty
    p = rng.permutation(node.size)
    g["assign"] = np.stack([node[p], cluster[p]])
    g["assign_w"] = rng.uniform(0.2, 1.0, node.size).astype(np.float32)
    # "zero": cluster 5 is reached through ONE assignment only and that weight is exactly 0.0 -> row / column 5 must vanish
    a0 = g["assign"].copy()
    w0 = g["assign_w"].copy()
    a0[1, a0[1] == 5] = 0
    a0[1, 0] = 5
    w0[0] = 0.0
    g["assign_zero"], g["assign_zero_w"] = a0, w0
    g["K"] = np.asarray(K)
    return g


def _cluster_args(g, cfg):
    name, with_x, aw, ew = cfg
    assign = g["assign_zero"] if aw == "zero" else g["assign"]
    w = g["assign_zero_w"] if aw == "zero" else (g["assign_w"] if aw == "w" else None)
    return (g["x"] if with_x else None, g["ei"], g["w"] if ew else None, assign, w, int(g["K"])), dict(num_nodes=g["n"])


def _cluster_outs(prefix, res):
    x, ei, w = res
    out = {prefix + "edge_index": pc._np(ei), prefix + "edge_weight": pc._np(w)}
    if x is not None:
        out[prefix + "x"] = pc._np(x)
    return out


def ref_cluster(R, g):
    out = {}
    for cfg in CLUSTER_CONFIGS:
        a, kw = _cluster_args(g, cfg)
        out.update(_cluster_outs(cfg[0] + "/", R.tfg.nn.cluster_pool(*a, **kw)))
    return out


def hip_cluster(tfg, g):
    out = {}
    for cfg in CLUSTER_CONFIGS:
        a, kw = _cluster_args(g, cfg)
        out.update(_cluster_outs(cfg[0] + "/", tfg.nn.cluster_pool(*a, **kw)))
    return out


CASES.append(Case("cluster_pool", cluster_inputs, ref_cluster, hip_cluster, CLUSTER_CONFIGS))
