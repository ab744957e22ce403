# coding=utf-8
"""Times the segmented product S_g^T Y_g (include/tfgx_seggram.h) and the DiffPool layer built on it against routes made only
of operators that existed before it: a padded [G, n_max, .] torch.bmm, and — where its expansion fits — the sparse S^T A S
of cluster_pool (expand - sort - compress) on the dense assignment.

Shapes: NCI1-shaped batches (graphs of 10-50 nodes, a random tree plus n / 8 extra bonds, both directions) of 512 and 4096
graphs, and one single graph of --single-nodes nodes, for K in {5, 20, 64} clusters per graph; h is [N, 128].
Method: every variant of a shape is warmed up, then the variants are timed in turn, --rounds times over (device events
around one call each); the medians are reported.  One JSON line per (shape, K) goes to --out.

    python tools/bench_dense_pool.py [--out profiles/dense_pool_bench.jsonl] [--rounds 9]
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import tf_geometric_amd as tfg                                    # noqa: E402
from tf_geometric_amd import _lib as L, autograd as AG             # noqa: E402
from tf_geometric_amd.nn.pool.cluster_pool import sparse_sas       # noqa: E402
from tf_geometric_amd.nn.pool.common_pool import _graph_plan       # noqa: E402
from tf_geometric_amd.nn.pool.diff_pool import _pooled_edges       # noqa: E402
from tf_geometric_amd.plan import CsrPlan                          # noqa: E402

UNITS = 128
SPARSE_SAS_MAX_PRODUCTS = 1.5e8          # 32 bytes each in the expansion's workspace


def _graph(rng, n):
    parent = (rng.random(n - 1) * np.arange(1, n)).astype(np.int64)
    a = np.concatenate([np.arange(1, n), rng.integers(0, n, n // 8)])
    b = np.concatenate([parent, rng.integers(0, n, n // 8)])
    keep = a != b
    return a[keep], b[keep]


def make_batch(sizes, seed):
    rng = np.random.Generator(np.random.PCG64(seed))
    rows, cols, gids, off = [], [], [], 0
    for j, n in enumerate(sizes):
        a, b = _graph(rng, int(n))
        rows += [a + off, b + off]
        cols += [b + off, a + off]
        gids.append(np.full(int(n), j, np.int32))
        off += int(n)
    dev = L.device()
    ei = torch.from_numpy(np.stack([np.concatenate(rows), np.concatenate(cols)]).astype(np.int32)).to(dev)
    return ei, torch.from_numpy(np.concatenate(gids)).to(dev), off


def timed(fn):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    fn()
    end.record()
    end.synchronize()
    return start.elapsed_time(end)


def measure(variants, rounds, warmup=2):
    """{name: callable} -> {name: median ms}; the variants alternate inside every round."""
    for fn in variants.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    times = {name: [] for name in variants}
    for _ in range(rounds):
        for name, fn in variants.items():
            times[name].append(timed(fn))
    return {name: round(statistics.median(v), 4) for name, v in times.items()}


def padded_index(gid, G):
    """(graph, slot) of every node for the padded route and n_max; gid is sorted here."""
    counts = torch.bincount(gid.long(), minlength=G)
    start = torch.cumsum(counts, 0) - counts
    slot = torch.arange(gid.shape[0], device=gid.device) - start[gid.long()]
    return gid.long(), slot, int(counts.max().item())


def bmm_gram(S, Y, gl, slot, G, n_max):
    """The padded route: scatter both operands into [G, n_max, .], one torch.bmm; -> [G K, W]."""
    Sp = torch.zeros((G, n_max, S.shape[1]), dtype=S.dtype, device=S.device).index_put((gl, slot), S)
    Yp = torch.zeros((G, n_max, Y.shape[1]), dtype=Y.dtype, device=Y.device).index_put((gl, slot), Y)
    return torch.bmm(Sp.transpose(1, 2), Yp).reshape(G * S.shape[1], Y.shape[1])


def bench_shape(name, sizes, K, rounds, seed):
    dev = L.device()
    ei, gid, N = make_batch(sizes, seed)
    G, E = len(sizes), int(ei.shape[1])
    gen = torch.Generator(device="cpu").manual_seed(seed)
    S0 = torch.softmax(torch.randn((N, K), generator=gen), dim=-1).to(dev)
    h0 = torch.randn((N, UNITS), generator=gen).to(dev)
    gplan = _graph_plan(gid, G, N, None)
    plan = CsrPlan.build(ei, N, N)
    AS0 = AG.aggregate(plan, S0, L.SUM)
    gl, slot, n_max = padded_index(gid, G)
    rec = dict(shape=name, graphs=G, nodes=N, edges=E, K=K, units=UNITS, n_max=n_max, seggram_block=L.SEGGRAM_BLOCK)

    def leaf(t):
        return t.detach().clone().requires_grad_(True)

    def train(gram):
        def step():
            S, AS, h = leaf(S0), leaf(AS0), leaf(h0)
            (gram(S, AS).sum() + gram(S, h).sum()).backward()
        return step
    ours = lambda S, Y: AG.segment_gram(gplan, gid, S, Y)                  # noqa: E731
    padded = lambda S, Y: bmm_gram(S, Y, gl, slot, G, n_max)              # noqa: E731
    err = float((ours(S0, h0) - padded(S0, h0)).abs().max())
    assert err < 1e-3 * max(1.0, float(n_max) ** 0.5), err                # the two routes compute the same thing
    variants = {
        "gram_fwd_ms": lambda: (ours(S0, AS0), ours(S0, h0)),
        "bmm_fwd_ms": lambda: (padded(S0, AS0), padded(S0, h0)),
        "gram_fwd_bwd_ms": train(ours),
        "bmm_fwd_bwd_ms": train(padded),
    }
    if float(E) * K * K <= SPARSE_SAS_MAX_PRODUCTS:
        s_row_ptr = (torch.arange(N + 1, dtype=torch.int64, device=dev) * K).to(torch.int32)
        s_col = (gid.reshape(-1, 1) * K + torch.arange(K, dtype=torch.int32, device=dev)).reshape(-1).contiguous()
        a_row, a_col = ei[0].contiguous(), ei[1].contiguous()
        # S^T A S alone, against aggregate + one segmented product
        variants["sparse_sas_fwd_ms"] = lambda: sparse_sas(s_row_ptr, s_col, S0.reshape(-1), N, G * K, a_row, a_col, None)
        variants["gram_sas_fwd_ms"] = lambda: ours(S0, AG.aggregate(plan, S0, L.SUM))
    rec.update(measure(variants, rounds))

    # the whole layer: DiffPool over two GCNs, warm cache, against the same layer with the padded products
    feature, assign = tfg.layers.GCN(UNITS, seed=seed + 1), tfg.layers.GCN(K, seed=seed + 2)
    layer = tfg.layers.DiffPool(feature, assign, UNITS, K)
    x0 = torch.randn((N, 37), generator=gen).to(dev)
    cache = {}
    layer([x0, ei, None, gid], cache=cache, num_graphs=G)
    layer.trainable(True)

    def layer_ours(x):
        return layer([x, ei, None, gid], cache=cache, num_graphs=G)

    def layer_padded(x):
        S = torch.softmax(assign([x, ei, None], cache=cache), dim=-1)
        hh = feature([x, ei, None], cache=cache)
        P = padded(S, AG.aggregate(plan, S, L.SUM))
        pei, pw = _pooled_edges(P, G, K, False)
        return [AG.bias_add(padded(S, hh), layer.bias), pei, pw, None]

    def layer_train(fn):
        def step():
            out = fn(x0)
            (out[0].sum() + out[2].sum()).backward()
        return step

    def no_grad(fn):
        def step():
            with torch.no_grad():
                fn(x0)
        return step
    a, b = layer_ours(x0), layer_padded(x0)
    assert torch.equal(a[1], b[1]) and float((a[0] - b[0]).abs().max()) < 1e-3 * max(1.0, float(n_max) ** 0.5)
    rec.update(measure({"layer_fwd_ms": no_grad(layer_ours), "layer_bmm_fwd_ms": no_grad(layer_padded),
                        "layer_fwd_bwd_ms": layer_train(layer_ours), "layer_bmm_fwd_bwd_ms": layer_train(layer_padded)}, rounds))
    return rec


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                                 "dense_pool_bench.jsonl"))
    p.add_argument("--rounds", type=int, default=9)
    p.add_argument("--single-nodes", type=int, default=1000000)
    p.add_argument("--clusters", type=int, nargs="*", default=[5, 20, 64])
    p.add_argument("--seed", type=int, default=0)
    args = p.parse_args()
    L.require_gpu()
    rng = np.random.Generator(np.random.PCG64(args.seed))
    shapes = [("nci1x512", rng.integers(10, 51, 512)), ("nci1x4096", rng.integers(10, 51, 4096)),
              ("single", np.asarray([args.single_nodes]))]
    box = "{} (torch {})".format(torch.cuda.get_device_name(0), torch.__version__)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        for name, sizes in shapes:
            for K in args.clusters:
                rec = bench_shape(name, sizes, K, args.rounds, args.seed)
                rec["box"] = box
                line = json.dumps(rec)
                print(line, flush=True)
                f.write(line + "\n")
                f.flush()


if __name__ == "__main__":
    main()
