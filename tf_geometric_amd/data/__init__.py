# coding=utf-8
"""The data layer: the reference's Graph / BatchGraph containers (tf_geometric/data/graph.py) and GraphStore, a dataset held
on the device that assembles minibatches — features, index arrays and CSR plans — in one kernel launch."""
from .graph import Graph, BatchGraph, StaticBatchGraph
from .graph_store import GraphStore, StaticLoader, StaticBatchCapacities, COLLATE_TILE
