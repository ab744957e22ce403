# coding=utf-8
"""The case table of tests/golden/batch_graph_cases.npz: constructor arguments of small graphs — (nodes, edges) = (3, 4),
(0, 0), (5, 0), (2, 6) and (1, 1: a self-loop) — as lists, float64 and float32 / int64 and int32 arrays, with weights on some,
all or none of the graphs and y absent, int64 [1] or float32 [1, 3].  `run` builds them with a Graph / BatchGraph pair — the
reference's (tests/golden/make_batch_graph_golden.py) or this package's (tests/test_graph_data.py) — and returns every array
the casts and BatchGraph.from_graphs produce."""
import numpy as np

F = 3
SHAPES = [(3, 4), (0, 0), (5, 0), (2, 6), (1, 1)]
EDGES = [[[0, 1, 2, 0], [1, 2, 0, 2]], None, None, [[0, 1, 0, 1, 0, 0], [1, 0, 1, 0, 0, 1]], [[0], [0]]]


def _x(rng, n, kind):
    x = rng.standard_normal((n, F))
    if kind == "list" and n > 0:
        return x.round(3).tolist()
    return x.astype(np.float32) if kind == "f32" else x


def _edges(i, kind):
    if EDGES[i] is None:
        return np.zeros((2, 0), dtype=np.int32 if kind != "i64" else np.int64)
    return EDGES[i] if kind == "list" else np.asarray(EDGES[i], dtype=np.int64 if kind == "i64" else np.int32)


def _weights(rng, e, kind):
    w = rng.uniform(0.5, 2.0, e)
    return w.round(3).tolist() if kind == "list" else (w.astype(np.float32) if kind == "f32" else w)


def _graphs(seed, x_kinds, e_kinds, w_kinds, y_kind):
    """One constructor-argument dict per graph.  w kind None = no weights given."""
    rng = np.random.Generator(np.random.PCG64(seed))
    graphs = []
    for i, (n, e) in enumerate(SHAPES):
        g = {"x": _x(rng, n, x_kinds[i]), "edge_index": _edges(i, e_kinds[i])}
        if w_kinds[i] is not None:
            g["edge_weight"] = _weights(rng, e, w_kinds[i])
        if y_kind == "i64":
            g["y"] = np.asarray([i % 2], dtype=np.int64)
        elif y_kind == "f32":
            g["y"] = rng.standard_normal((1, 3)).astype(np.float32)
        elif y_kind == "list":
            g["y"] = [i % 3]
        graphs.append(g)
    return graphs


CASES = {
    "f32_no_weights_no_y": lambda: _graphs(1, ["f32"] * 5, ["i32"] * 5, [None] * 5, None),
    "lists_f64_some_weights_y_i64": lambda: _graphs(2, ["list", "f64", "f64", "list", "f64"], ["list", "i32", "i64", "i64", "list"],
                                                    ["list", None, None, "f64", None], "i64"),
    "all_weights_y_f32": lambda: _graphs(3, ["f64", "f32", "f32", "f64", "list"], ["i64", "i32", "i32", "list", "i32"],
                                         ["f32", "f32", "f64", "list", "f32"], "f32"),
    "y_list": lambda: _graphs(4, ["f32"] * 5, ["list", "i32", "i32", "list", "list"], [None] * 5, "list"),
}


def run(Graph, BatchGraph, graphs):
    """{name: array} of everything the casts and from_graphs make of `graphs` (constructor-argument dicts)."""
    built = [Graph(**g) for g in graphs]
    out = {}
    for i, g in enumerate(built):
        out["g{}.x".format(i)] = g.x
        out["g{}.edge_index".format(i)] = g.edge_index
        out["g{}.edge_weight".format(i)] = g.edge_weight
        if g.y is not None:
            out["g{}.y".format(i)] = g.y
        out["g{}.sizes".format(i)] = np.asarray([g.num_nodes, g.num_edges, g.num_features], dtype=np.int64)
    b = BatchGraph.from_graphs(built)
    for key in ("x", "edge_index", "node_graph_index", "edge_graph_index", "edge_weight", "y"):
        if getattr(b, key) is not None:
            out["batch." + key] = getattr(b, key)
    out["batch.sizes"] = np.asarray([b.num_nodes, b.num_edges, b.num_features], dtype=np.int64)
    for k, v in out.items():
        assert isinstance(v, np.ndarray), "{} is {}: numpy graphs must stay numpy".format(k, type(v))
    return out
