# coding=utf-8
"""Hierarchical MinCutPool graph classification — the MI355X counterpart of the reference's demo/demo_min_cut_pool.py.

The model of examples/demo_diff_pool.py with MinCutPool layers (20 and 5 clusters per graph); the loss is the classification
loss plus, per level, the cut loss and the orthogonality loss that the layer's loss callable returns.  Data: the seeded
NCI1-shaped stand-in of examples/demo_sag_pool_h.py.

    python examples/demo_min_cut_pool.py [--steps 40] [--graphs 600] [--static] [--capture]

--static / --capture: the fixed-shape route of examples/demo_diff_pool.py with MinCutPool.pool_static; the two losses of every
level are means over the live slots and are part of the replayed step.

Unlike the DiffPool demo, the pooled edge weights are detached before they enter the next level
(detach_pooled_weights=True): MinCutPool normalises its edge weights with raw kernel launches (adj_norm_edge) and still
refuses an edge_weight that requires grad, although the GCNs inside it would differentiate one.
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import tf_geometric_amd as tfg   # noqa: E402
from demo_diff_pool import run   # noqa: E402

if __name__ == "__main__":
    run(tfg.layers.MinCutPool, True, "MinCutPool on an NCI1-shaped synthetic set", detach_pooled_weights=True)
