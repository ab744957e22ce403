# coding=utf-8
"""ASAP pooling on NCI1-shaped batches (the synthetic set of examples/demo_sag_pool_h.py, 64 hidden features): the layer
forward and forward + backward, and its two new pieces beside routes made ONLY of operators that were in the package before
them:

  attention   the fused launch (tfgx_asap_attend_f32 / _backward_f32) vs autograd.asap_attend_composed: two scalar gathers,
              leaky_relu, the segment-softmax kernel over explicit row ids, and the weighted aggregation;
  S^T A S     tfgx_spasp_count / _emit / _reduce vs torch dense matmul S^T (A S) followed by nonzero(), where [N, N] fits
              (--dense-limit nodes; the reference's own route).

    python tools/bench_asap.py [--graphs 512 4096] [--features 64] [--rounds 10] [--out FILE]

A and B alternate inside one process, medians of --rounds after a warm-up.  The layer is timed with a warm `cache`.  A
measurement tool: it has no pass / fail ratio.  One JSON line."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples"))
import tf_geometric_amd as tfg   # noqa: E402
from tf_geometric_amd import autograd as AG   # noqa: E402
from tf_geometric_amd.nn.pool.cluster_pool import sparse_sas   # noqa: E402
import demo_sag_pool_h as demo   # noqa: E402


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def alternate(fa, fb, rounds):
    fa(), fb()
    ta, tb = [], []
    for _ in range(rounds):
        ta.append(event_ms(fa))
        tb.append(event_ms(fb))
    return round(float(np.median(ta)), 4), round(float(np.median(tb)), 4)


def kernel_launches(fn):
    """Device kernels launched by fn (torch's profiler sees the launches of libtfgx.so too); None when it cannot tell."""
    try:
        from torch.profiler import profile, ProfilerActivity
        fn()
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        n = sum(1 for e in prof.events() if str(getattr(e, "device_type", "")).endswith("CUDA"))
        return n or None
    except Exception:      # noqa: BLE001 - a count is optional
        return None


def batch_of(num_graphs, F, seed=0):
    data = demo.make_dataset(num_graphs=num_graphs, seed=seed)
    x, ei, gid, _, _ = demo.make_batch(data, list(range(num_graphs)))
    g = torch.Generator().manual_seed(seed)
    return torch.randn(int(x.shape[0]), F, generator=g).to(x.device), ei, gid


def bench_batch(num_graphs, F, rounds, dense_limit):
    x, ei, gid = batch_of(num_graphs, F)
    n, E = int(x.shape[0]), int(ei.shape[1])
    dev = x.device
    res = dict(graphs=num_graphs, nodes=n, edges=E, features=F)

    # ---- the attention alone
    plan = tfg.CsrPlan.build(ei, n)
    g = torch.Generator().manual_seed(1)
    sq, sh = torch.randn(n, generator=g).to(dev), torch.randn(n, generator=g).to(dev)
    b = torch.zeros(1, device=dev)
    with torch.no_grad():
        f_ms, c_ms = alternate(lambda: AG.asap_attend(plan, x, sq, sh, b), lambda: AG.asap_attend_composed(plan, x, sq, sh, b), rounds)
        diff = float((AG.asap_attend(plan, x, sq, sh, b)[0] - AG.asap_attend_composed(plan, x, sq, sh, b)[0]).abs().max())
        launches = (kernel_launches(lambda: AG.asap_attend(plan, x, sq, sh, b)),
                    kernel_launches(lambda: AG.asap_attend_composed(plan, x, sq, sh, b)))
    leaves = [t.clone().requires_grad_(True) for t in (x, sq, sh, b)]

    def train(fn):
        for t in leaves:
            t.grad = None
        fn(plan, *leaves)[0].sum().backward()
    f_fb, c_fb = alternate(lambda: train(AG.asap_attend), lambda: train(AG.asap_attend_composed), rounds)
    res["attention"] = dict(fused_forward_ms=f_ms, composed_forward_ms=c_ms, fused_forward_backward_ms=f_fb,
                            composed_forward_backward_ms=c_fb, max_abs_difference=diff, fused_forward_launches=launches[0],
                            composed_forward_launches=launches[1])

    # ---- the layer, warm cache: fused attention (the default) and the composed attention
    layer = tfg.layers.ASAP(ratio=0.5, seed=1)
    cache = {}
    inputs = [x, ei, None, gid]
    layer(inputs, cache=cache)

    def fwd(fused):
        AG.ASAP_FUSED = fused
        try:
            with torch.no_grad():
                return layer(inputs, cache=cache)
        finally:
            AG.ASAP_FUSED = True
    f_ms, c_ms = alternate(lambda: fwd(True), lambda: fwd(False), rounds)
    out = fwd(True)
    res["layer_forward"] = dict(fused_attention_ms=f_ms, composed_attention_ms=c_ms, pooled_nodes=int(out[0].shape[0]),
                                pooled_edges=int(out[1].shape[1]), launches=kernel_launches(lambda: fwd(True)))
    layer.trainable(True)

    def step(fused):
        AG.ASAP_FUSED = fused
        try:
            for p in layer.parameters():
                p.grad = None
            layer(inputs, cache=cache)[0].sum().backward()
        finally:
            AG.ASAP_FUSED = True
    f_ms, c_ms = alternate(lambda: step(True), lambda: step(False), rounds)
    res["layer_forward_backward"] = dict(fused_attention_ms=f_ms, composed_attention_ms=c_ms)
    layer.trainable(False)

    # ---- S^T A S alone: a top-half assignment with the 1-hop weights of a uniform attention
    with torch.no_grad():
        K = n // 2
        node_map = torch.full((n,), -1, dtype=torch.int32, device=dev)
        node_map[torch.randperm(n, generator=g)[:K].to(dev)] = torch.arange(K, dtype=torch.int32, device=dev)
        from tf_geometric_amd.nn.pool.asap import _assignment
        AG._transposed(plan)
        pw = torch.rand(E, generator=g).to(dev)
        pws = torch.rand(n, generator=g).to(dev)
        s_row_ptr, s_col, s_val = _assignment(plan, pw, pws, node_map)
        arn = torch.arange(n, dtype=torch.int32, device=dev)
        a_row, a_col = torch.cat([AG.plan_rows(plan).to(torch.int32), arn]), torch.cat([plan.col, arn])

        def sparse():
            return sparse_sas(s_row_ptr, s_col, s_val, n, K, a_row, a_col, None, drop_diagonal=True)
        sas = dict(clusters=K, pooled_entries=int(sparse()[0].shape[0]), launches=kernel_launches(sparse))
        if n <= dense_limit:
            rows_s = torch.repeat_interleave(torch.arange(n, device=dev), (s_row_ptr[1:] - s_row_ptr[:-1]).long())
            ok = s_col >= 0

            def dense():
                S = torch.zeros((n, K), device=dev).index_put((rows_s[ok], s_col[ok].long()), s_val[ok], accumulate=True)
                A = torch.zeros((n, n), device=dev).index_put((a_row.long(), a_col.long()), torch.ones(E + n, device=dev),
                                                              accumulate=True)
                P = S.t() @ (A @ S)
                P.fill_diagonal_(0.0)
                idx = torch.nonzero(P)
                return idx, P[idx[:, 0], idx[:, 1]]
            sas["sparse_ms"], sas["dense_ms"] = alternate(sparse, dense, max(rounds // 2, 3))
            sas["dense_bytes"] = 4 * (n * n + 2 * n * K + K * K)
            sas["same_structure"] = bool(torch.equal(torch.stack([sparse()[0], sparse()[1]]).long(), dense()[0].t()))
        else:
            sparse()
            sas["sparse_ms"] = round(float(np.median([event_ms(sparse) for _ in range(rounds)])), 4)
            sas["dense_ms"] = None      # [N, N] float32 does not fit: 4 N^2 bytes
            sas["dense_bytes"] = 4 * (n * n + 2 * n * K + K * K)
        res["sas"] = sas
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--graphs", type=int, nargs="+", default=[512, 4096])
    ap.add_argument("--features", type=int, default=64)
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--dense-limit", type=int, default=40000)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    res = dict(tool="bench_asap", device=torch.cuda.get_device_name(0),
               batches=[bench_batch(g, args.features, args.rounds, args.dense_limit) for g in args.graphs])
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
