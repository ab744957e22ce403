# coding=utf-8
"""Writes tests/golden/link_cases.npz: the outputs of the reference's OWN extract_unique_edge,
convert_edge_index_to_edge_hash, convert_edge_hash_to_edge_index and convert_edge_to_upper(..., ["max"]) (the
deterministic part of edge_train_test_split, utils/graph_utils.py:510), run unmodified through oracle/ref_harness (on the
numpy stand-ins for TensorFlow where it is not installed; the backend is recorded as ``__backend__``).  The inputs are
stored next to the outputs (``<case>::edge_index``, ``<case>::edge_weight``), so the tests need nothing else.

Cases: ``mixed`` holds duplicates, both directions of an edge, self-loops and weights; ``empty`` holds no edge (there the
reference's convert_edge_to_upper fails on an empty maximum, so only the other three functions are recorded).

    python tests/golden/make_link_golden.py          # regenerate (needs the reference checkout)
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

from oracle.ref_harness import load_reference   # noqa: E402

OUT = os.path.join(HERE, "link_cases.npz")


def cases():
    rng = np.random.Generator(np.random.PCG64(2024))
    base = rng.integers(0, 12, size=(2, 40)).astype(np.int32)
    flipped = base[::-1, :15]                                     # both directions
    repeats = base[:, 5:25]                                       # exact duplicates
    loops = np.stack([np.arange(0, 12, 3), np.arange(0, 12, 3)]).astype(np.int32)
    ei = np.concatenate([base, flipped, loops, repeats, loops[:, :2]], axis=1)
    ei = ei[:, rng.permutation(ei.shape[1])]
    w = rng.uniform(0.1, 2.0, size=ei.shape[1]).astype(np.float32)
    return {"mixed": (ei, w, 12), "empty": (np.zeros((2, 0), np.int32), np.zeros(0, np.float32), 5)}


def run_reference():
    tfg, tf, tfs, backend = load_reference()
    from tf_geometric.utils import graph_utils as gu
    blob = {"__backend__": np.array(backend)}
    for name, (ei, w, n) in cases().items():
        put = lambda k, v: blob.__setitem__("{}::{}".format(name, k), np.asarray(v))      # noqa: E731
        put("edge_index", ei)
        put("edge_weight", w)
        put("num_nodes", n)
        for mode in ("undirected", "directed"):
            u_ei, u_w = gu.extract_unique_edge(ei, w, mode=mode)
            put("unique_{}_index".format(mode), np.asarray(u_ei, dtype=np.int32).reshape(2, -1))
            put("unique_{}_weight".format(mode), u_w)
        edge_hash, n_out = gu.convert_edge_index_to_edge_hash(ei, n)
        put("hash", edge_hash)
        put("hash_num_nodes", n_out)
        put("hash_to_index", gu.convert_edge_hash_to_edge_index(edge_hash, n))
        if ei.shape[1] > 0:
            edge_hash, n_out = gu.convert_edge_index_to_edge_hash(ei)
            put("hash_inferred", edge_hash)
            put("hash_inferred_num_nodes", n_out)
            upper, [upper_w] = gu.convert_edge_to_upper(ei, [w], merge_modes=["max"])
            put("upper_index", upper)
            put("upper_weight", upper_w)
    return blob


if __name__ == "__main__":
    blob = run_reference()
    np.savez_compressed(OUT, **blob)
    print("wrote {} ({} arrays, {} bytes)".format(OUT, len(blob), os.path.getsize(OUT)))
