# coding=utf-8
"""Measures the graph-coarsening path (SAGPool / SortPool) and writes one JSON under profiles/.

(a) products shape (N = 2.4 M, E = 123 M from synthetic_edges, node_graph_index = 64 contiguous blocks, random scores,
    ratio 0.5): induced subgraph + DERIVED plan  vs  induced subgraph + CsrPlan.build of the pooled edge list.  Wall times
    per call (events around the host calls: both include the one host read of the kept-edge count), algorithmic bytes
    computed from the shapes, and their share of the 8 TB/s HBM peak.
(b) one training step of the hierarchical SAGPool model (examples/demo_sag_pool_h.py) on a batch of 512 synthetic graphs:
    ms per step and host syncs per step (torch-side synchronising calls counted by torch's sync debug mode, library-side
    ones by counting the entry points that synchronise: tfgx_build_csr_by_dst, tfgx_segment_topk,
    tfgx_induced_subgraph_count).

    python tools/bench_graph_pool.py [--reps 10] [--out profiles/graph_pool.json]
    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/bench_graph_pool.py --reps 3 --out <dir>/run.json
"""
import argparse
import json
import os
import sys
import time
import warnings

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "examples"))
import tf_geometric_amd as tfg                                    # noqa: E402
from tf_geometric_amd.synthetic import synthetic_edges            # noqa: E402
from tf_geometric_amd.utils.subgraph import induced_subgraph      # noqa: E402

PEAK_BYTES_PER_S = 8.0e12
SYNCING = ("tfgx_build_csr_by_dst", "tfgx_segment_topk", "tfgx_induced_subgraph_count")


def timed(fn, reps):
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b))
    return float(np.median(ts)), [round(t, 4) for t in ts]


def products(reps):
    n, e = 2449029, 123718280
    dev = torch.device("cuda")
    ei = torch.from_numpy(synthetic_edges(n, e, seed=0)).to(dev)
    E = int(ei.shape[1])
    gid = (torch.arange(n, device=dev, dtype=torch.int64) * 64 // n).to(torch.int32)
    score = torch.rand(n, generator=torch.Generator(device="cpu").manual_seed(5)).to(dev)
    keep = tfg.nn.topk_pool(gid, score, ratio=0.5)
    m = int(keep.shape[0])
    parent = tfg.CsrPlan.build(ei, n)
    sub = induced_subgraph(ei, keep, n, parent_plan=parent)
    K = sub.plan.num_edges
    deg = parent.in_degree()
    e_rows = int(deg[keep.long()].sum().item())        # parent edges in the kept rows: what the derivation walks

    derive_ms, derive_all = timed(lambda: induced_subgraph(ei, keep, n, parent_plan=parent), reps)
    plain_ms, _ = timed(lambda: induced_subgraph(ei, keep, n), reps)
    pooled = sub.edge_index
    build_ms, _ = timed(lambda: tfg.CsrPlan.build(pooled, m), reps)
    # algorithmic bytes (each array once): count = row, col + node_map writes + node_index reads; emit = row, col again +
    # (row', col', edge id, rank) writes; derivation = row_ptr pairs of the kept rows, parent col of the kept rows (twice:
    # count + emit), parent perm + rank of the kept edges, (row_ptr', col', perm') writes
    count_b = 8 * E + 4 * n + 4 * m
    emit_b = 8 * E + 16 * K
    derive_b = 2 * 8 * m + 2 * 4 * e_rows + 8 * K + 4 * (m + 1) + 8 * K
    res = {
        "shape": {"n": n, "E": E, "kept_nodes": m, "kept_edges": K, "parent_edges_in_kept_rows": e_rows, "ratio": 0.5,
                  "graphs": 64},
        "induced_subgraph_with_derived_plan_ms": round(derive_ms, 4),
        "induced_subgraph_with_derived_plan_all_ms": derive_all,
        "induced_subgraph_without_plan_ms": round(plain_ms, 4),
        "csr_plan_build_of_pooled_ms": round(build_ms, 4),
        "induced_subgraph_plus_rebuild_ms": round(plain_ms + build_ms, 4),
        "derivation_ms": round(derive_ms - plain_ms, 4),
        "algorithmic_bytes": {"count": count_b, "emit": emit_b, "derive": derive_b, "total": count_b + emit_b + derive_b},
    }
    res["share_of_8TBs_peak"] = {
        "induced_subgraph_with_derived_plan": round((count_b + emit_b + derive_b) / (derive_ms * 1e-3) / PEAK_BYTES_PER_S, 4),
        "derivation_alone": round(derive_b / max((derive_ms - plain_ms) * 1e-3, 1e-9) / PEAK_BYTES_PER_S, 4),
    }
    return res


class _Counter(object):
    def __init__(self):
        self.calls = {k: 0 for k in SYNCING}
        lib = tfg._lib.load_library()
        self._orig = {}
        for name in SYNCING:
            fn = getattr(lib, name)
            self._orig[name] = fn

            def wrap(*a, _fn=fn, _name=name):
                self.calls[_name] += 1
                return _fn(*a)
            setattr(lib, name, wrap)

    def restore(self):
        lib = tfg._lib.load_library()
        for name, fn in self._orig.items():
            setattr(lib, name, fn)


def sag_pool_h_step(reps):
    import demo_sag_pool_h as demo
    data = demo.make_dataset(num_graphs=512, seed=0)
    batch = demo.make_batch(data, list(range(512)))
    model = demo.SAGPoolHModel(data.num_features, data.num_classes, seed=0)
    opt = torch.optim.Adam(model.parameters(), lr=5e-4)
    for _ in range(3):
        demo.train_step(model, opt, batch)
    ms, all_ms = timed(lambda: demo.train_step(model, opt, batch), reps)
    counter = _Counter()
    torch_syncs = None
    try:
        with warnings.catch_warnings(record=True) as caught:
            warnings.simplefilter("always")
            torch.cuda.set_sync_debug_mode("warn")
            try:
                demo.train_step(model, opt, batch)
            finally:
                torch.cuda.set_sync_debug_mode("default")
        torch_syncs = sum(1 for w in caught if "synchroniz" in str(w.message).lower())
    finally:
        counter.restore()
    return {"graphs": 512, "nodes": int(batch[0].shape[0]), "edges": int(batch[1].shape[1]),
            "ms_per_step": round(ms, 4), "ms_all": all_ms,
            "library_syncs_per_step": dict(counter.calls), "torch_syncs_per_step": torch_syncs}


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--reps", type=int, default=10)
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "graph_pool.json"))
    p.add_argument("--skip-products", action="store_true")
    args = p.parse_args()
    tfg._lib.require_gpu()
    res = {"device": torch.cuda.get_device_name(0), "time": time.strftime("%Y-%m-%d %H:%M:%S")}
    if not args.skip_products:
        res["products"] = products(args.reps)
        torch.cuda.empty_cache()
    res["sag_pool_h_step"] = sag_pool_h_step(args.reps)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
