# coding=utf-8
"""The SortPool readout of DGCNN (node rows -> [B, k, F], k = 30, F = 128) alone, and one whole training step of
examples/demo_sort_pool.py (3 x GCN(128) -> SortPool(30) -> Conv1D(128, 5) -> MLP, Adam) on its dataset (4000 graphs of 10-50
nodes, F = 37), batches of 128 and 512 graphs.

The readout alone, forward, on the rows of one collated batch:
  fused    : nn.sort_pool_3d with a warm cache — one launch of tfgx_segment_rows_3d_f32, no host read
  static   : nn.sort_pool_static on the collate_static batch of the same graphs — the same launch over graph_row_ptr
  composed : nn.sort_pool (global radix sort, two host reads, the induced edge list and its plan) + utils.convert_x_to_3d
  torch    : a pure-torch restatement (two stable argsorts, bincount, cumsum, a mask, an indexed scatter; the mask reads a size back)
and the fused kernel by itself between two device events, against its byte floor: 4 B k F written, 4 F sum_g min(n_g, k) read,
and one 128-byte line per node for the key (the key is one float out of a 512-byte row).

The step, three ways and the fused readout on ordinary batches beside them:
  collate          : GraphStore.collate of host-drawn ids + SortPool.call + convert_x_to_3d (the reference's model as written)
  collate_fused    : the same batches + SortPool.pool_3d
  static           : StaticLoader.next_ids + collate_static + SortPool.pool_static, issued launch by launch
  replayed         : `static` recorded once by tfg.CapturedTrainStep and replayed from one hipGraph

Method (that of tools/bench_sag_pool_static.py): a host clock around work that ends in a device synchronise; the variants
alternate step by step in one process, after a warm-up; the whole comparison is repeated (--repeats) so the spread between the
repeats' medians is known.  A variant counts as ahead of another only when its median is below the other's by more than the SUM
of the two spreads.  Each step variant trains a model of its own.  Not measured: where inside a step the time goes (no kernel
trace); the backward of the readout by itself.

    python tools/bench_sort_pool_3d.py [--out profiles/sort_pool_3d_bench.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "examples"))

K, UNITS = 30, 128


def torch_route(h, ngi, k, G):
    """sort_pool_3d in torch indexing, what a user without the helper writes."""
    import torch
    n = h.shape[0]
    by_key = torch.argsort(h.detach()[:, -1], descending=True, stable=True)
    perm = by_key[torch.argsort(ngi[by_key], stable=True)]
    g = ngi[perm].long()
    counts = torch.bincount(g, minlength=G)
    pos = torch.arange(n, device=h.device) - (torch.cumsum(counts, 0) - counts)[g]
    mask = pos < k
    out = torch.zeros((G, k, h.shape[1]), dtype=h.dtype, device=h.device)
    out[g[mask], pos[mask]] = h[perm[mask]]
    return out


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--graphs", type=int, default=4000)
    p.add_argument("--batch-sizes", type=int, nargs="+", default=[128, 512])
    p.add_argument("--steps", type=int, default=60, help="timed steps per variant and repeat (at least 50)")
    p.add_argument("--warmup", type=int, default=8)
    p.add_argument("--repeats", type=int, default=3)
    p.add_argument("--out", default=None)
    args = p.parse_args()

    import torch
    import tf_geometric_amd as tfg
    from demo_sort_pool import SortPoolModel, graph_store, make_dataset, static_loss
    assert torch.cuda.is_available(), "bench_sort_pool_3d needs a GPU: there is nothing to time without one"

    data = make_dataset(args.graphs, 0)
    store = graph_store(data, range(len(data.graphs)))
    F, G = store.num_features, len(store)
    rng = np.random.Generator(np.random.PCG64(7))

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, out

    def summary(medians):
        med = {k: float(np.median(v)) for k, v in medians.items()}
        spread = {k: float(max(v) - min(v)) for k, v in medians.items()}
        return {"median_ms": med, "repeat_medians_ms": medians, "spread_ms": spread}

    def ahead(s, a, b):
        """a ahead of b beyond the sum of the two spreads"""
        return bool(s["median_ms"][b] - s["median_ms"][a] > s["spread_ms"][a] + s["spread_ms"][b])

    def collate_loss(model, b):
        logits = model([b.x, b.edge_index, b.node_graph_index, b.num_graphs], training=True)
        return torch.nn.functional.cross_entropy(logits, b.y.reshape(-1))

    def eager_step(opt, loss_fn):
        def step():
            opt.zero_grad(set_to_none=True)
            loss = loss_fn()
            loss.backward()
            opt.step()
            return loss
        return step

    result = {"dataset": {"graphs": G, "nodes": int(store.node_ptr[-1]), "edges": int(store.edge_ptr[-1]), "F": F},
              "readout": {"k": K, "F": UNITS},
              "method": "host clock around work ending in a device synchronise; variants alternate step by step; ms",
              "batch_sizes": {}}
    for bs in args.batch_sizes:
        cap = store.static_capacities(bs)
        torch.manual_seed(0)
        pool = [rng.choice(G, bs, replace=False) for _ in range(256)]
        turn = iter(range(1 << 30))

        def host_ids():
            return pool[next(turn) % len(pool)]

        models = [SortPoolModel(F, 2, seed=0, fused=f) for f in (False, True, True, True)]
        loader_b = store.static_loader(bs, shuffle=True, seed=1)
        loader_c = store.static_loader(bs, shuffle=True, seed=1)
        steps = {"collate": eager_step(torch.optim.Adam(models[0].parameters(), lr=5e-4),
                                       lambda: collate_loss(models[0], store.collate(host_ids()))),
                 "collate_fused": eager_step(torch.optim.Adam(models[1].parameters(), lr=5e-4),
                                             lambda: collate_loss(models[1], store.collate(host_ids()))),
                 "static": eager_step(torch.optim.Adam(models[2].parameters(), lr=5e-4),
                                      lambda: static_loss(models[2], store.collate_static(loader_b.next_ids(), cap))),
                 "replayed": tfg.CapturedTrainStep(lambda: static_loss(models[3], store.collate_static(loader_c.next_ids(), cap)),
                                                   torch.optim.Adam(models[3].parameters(), lr=5e-4, capturable=True))}
        # the readout alone: the rows of one batch, F = 128, as the third GCN leaves them (random values: the kernel moves rows)
        ids = pool[0]
        plain = store.collate(ids)
        batch = store.collate_static(torch.from_numpy(ids.astype(np.int32)).cuda(), cap)
        n = int(plain.x.shape[0])
        h = torch.randn(n, UNITS, device="cuda")
        h_static = torch.zeros(cap.n_cap, UNITS, device="cuda")
        h_static[:n] = h
        ngi, ei = plain.node_graph_index, plain.edge_index

        def composed():
            px, _, _, pgi = tfg.nn.sort_pool(h, ei, None, ngi, k=K)
            return tfg.utils.convert_x_to_3d(px, pgi, k=K, num_sources=bs)

        alone = {"fused": lambda: tfg.nn.sort_pool_3d(h, ngi, K, num_graphs=bs, cache=plain.cache),
                 "static": lambda: tfg.nn.sort_pool_static(h_static, batch, K),
                 "composed": composed,
                 "torch": lambda: torch_route(h, ngi, K, bs)}
        ref = alone["fused"]()
        assert torch.equal(ref, alone["static"]()) and torch.equal(ref, alone["composed"]()) and torch.equal(ref, alone["torch"]())
        entry = {"capacities": cap._asdict(), "batch_nodes": n}
        for what, variants in (("step", steps), ("readout_alone", alone)):
            for _ in range(args.warmup):
                for fn in variants.values():
                    fn()
            medians = {k: [] for k in variants}
            for _ in range(args.repeats):
                t = {k: [] for k in variants}
                for _ in range(max(args.steps, 50)):
                    for k, fn in variants.items():
                        t[k].append(timed(fn)[0])
                for k in t:
                    medians[k].append(float(np.median(t[k])))
            entry[what] = summary(medians)
        s, a = entry["step"], entry["readout_alone"]
        entry["ahead_beyond_spreads"] = {"step: replayed vs collate": ahead(s, "replayed", "collate"),
                                         "step: static vs collate": ahead(s, "static", "collate"),
                                         "step: collate_fused vs collate": ahead(s, "collate_fused", "collate"),
                                         "readout: fused vs composed": ahead(a, "fused", "composed"),
                                         "readout: fused vs torch": ahead(a, "fused", "torch")}
        # the kernel by itself: `reps` launches recorded in one hipGraph (no host between them), replayed between two device events
        deg = np.diff(store.node_ptr)[ids]
        floor = 4 * bs * K * UNITS + 4 * UNITS * int(np.minimum(deg, K).sum()) + 128 * n
        reps, per_launch = 50, []
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            kept = [alone["fused"]() for _ in range(reps)]
        for _ in range(4):
            start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            start.record()
            graph.replay()
            end.record()
            torch.cuda.synchronize()
            per_launch.append(start.elapsed_time(end) * 1e3 / reps)
        assert torch.equal(kept[-1], ref)
        del kept, graph
        us = float(np.median(per_launch[1:]))
        entry["kernel"] = {"us_per_launch": us, "repeat_us": per_launch[1:], "floor_bytes": int(floor),
                           "floor_GB_per_s_reached": float(floor / us / 1e3),
                           "note": "{} launches replayed from one hipGraph between two device events (the first replay dropped); "
                                   "every launch writes an output of its own, the rows it reads stay cache resident".format(reps)}
        result["batch_sizes"][str(bs)] = entry
        print("batch {:4d}: step  collate {:.3f}  collate_fused {:.3f}  static {:.3f}  replayed {:.3f} ms  (spreads {:.3f} / {:.3f} / "
              "{:.3f} / {:.3f})".format(bs, *(s["median_ms"][k] for k in steps), *(s["spread_ms"][k] for k in steps)), flush=True)
        print("            readout alone: fused {:.3f}  static {:.3f}  composed {:.3f}  torch {:.3f} ms  (spreads {:.3f} / {:.3f} / "
              "{:.3f} / {:.3f})".format(*(a["median_ms"][k] for k in alone), *(a["spread_ms"][k] for k in alone)), flush=True)
        print("            kernel: {:.1f} us per launch, floor {} bytes -> {:.0f} GB/s;  ahead beyond spreads: {}".format(
            us, floor, entry["kernel"]["floor_GB_per_s_reached"], entry["ahead_beyond_spreads"]), flush=True)
    print(json.dumps(result))
    if args.out:
        with open(args.out, "w") as fh:
            json.dump(result, fh, indent=1)


if __name__ == "__main__":
    main()
