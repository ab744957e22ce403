# coding=utf-8
"""Parity cases of utils.convert_x_to_3d and of the DGCNN readout sort_pool -> convert_x_to_3d (reference:
utils/graph_utils.py:215-249, nn/pool/sort_pool.py:7-35, demo/demo_sort_pool.py:94-96).

``ref`` runs the reference's own Python (written into tests/golden/sortpool3d_cases.npz by
tests/golden/make_sortpool3d_golden.py; re-run live by tests/test_sortpool3d_reference.py where the reference checkout exists).
Every output only moves values, so every comparison is exact.

The sort column holds DISTINCT values within every graph: the reference's descending argsort is not stable, so ties are pinned
to nn.topk_pool by the GPU tests instead.  The batches cover: k None / below / equal / above the largest group, each with pad
True and False; an empty graph in the middle; a trailing empty graph (the reference's first axis stops at the last graph that
has a node: num_sources= appends zero graphs); unsorted, interleaved source_index; F = 1 and F = 3."""
import numpy as np


class Case(object):
    def __init__(self, name, inputs, configs):
        self.name, self.inputs, self.configs = name, inputs, configs

    def __repr__(self):
        return "Case({})".format(self.name)

    def ref(self, R, g):
        """{config/convert: [G_ref, k', F], config/sort: [G_ref, k, F]} — the second only for configs with an int k and
        pad=True (sort_pool_3d has no pad=)."""
        convert = R.tfg.utils.graph_utils.convert_x_to_3d
        out = {}
        for name, k, pad, si in self.configs:
            out[name + "/convert"] = _np(convert(g["x"], g["gid"], k=k, pad=pad))
            if k is not None and pad:
                px, _, _, pgi = R.tfg.nn.sort_pool(g["x"], g["ei"], None, g["gid"], k=k, sort_index=si)
                out[name + "/sort"] = _np(convert(px, pgi, k=k, pad=pad))
        return out


def _np(t):
    if hasattr(t, "numpy"):
        t = t.numpy()
    return np.asarray(t)


def _batch(sizes, f, seed, interleave=True):
    rng = np.random.Generator(np.random.PCG64(seed))
    gid = np.concatenate([np.full(s, g, dtype=np.int32) for g, s in sizes.items()])
    if interleave:
        gid = gid[rng.permutation(gid.size)]
    n = gid.size
    x = rng.standard_normal((n, f)).astype(np.float32)
    for c in range(f):          # every column distinct within the whole batch: any sort_index ranks without ties
        x[:, c] = (rng.permutation(n) - n // 2).astype(np.float32) * 0.25
    edges = []
    for g in sizes:
        nodes = np.flatnonzero(gid == g)
        for _ in range(nodes.size):
            edges.append(tuple(rng.choice(nodes, 2)))
    ei = np.asarray(edges, dtype=np.int32).T.copy()
    return dict(x=x, gid=gid, ei=ei)


def interleaved():
    """5 graph ids, graph 2 empty, nodes interleaved; the largest group has 9 nodes; F = 3."""
    return _batch({0: 7, 1: 2, 3: 9, 4: 5}, 3, seed=0)


def trailing():
    """Graphs 0-3 used, in order, one feature; the tests ask for num_sources = 6 (two trailing empty graphs) as well."""
    return _batch({0: 4, 1: 1, 2: 6, 3: 3}, 1, seed=1, interleave=False)


def _configs(largest, sort_indices):
    out = []
    for label, k in (("none", None), ("below", 3), ("equal", largest), ("above", largest + 3), ("one", 1)):
        for pad in (True, False):
            for si in sort_indices:
                out.append(("k{}-{}-pad{}-col{}".format(label, k, int(pad), si), k, pad, si))
    return out


CASES = [Case("interleaved", interleaved, _configs(9, (-1, 0, 1))), Case("trailing", trailing, _configs(6, (-1,)))]
NUM_SOURCES = {"interleaved": (None, 5, 7), "trailing": (None, 4, 6)}      # what the tests pass as num_sources / num_graphs
