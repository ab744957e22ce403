# coding=utf-8
"""Times the backward of the GCN normalisation (include/tfgx_normgrad.h) at the products shape (N = 2.4 M, E = 123 M; the
uniform graph and the R-MAT graph of tf_geometric_amd/synthetic.py), for the layer's default configuration (norm both,
symmetric, renormalised unit self-loops):

  each of its three launches alone (the `passes` argument of tfgx_gcn_norm_backward_f32) and all three together;
  the normalisation forward (two launches);
  the same formulas composed of torch operators (index_add_ / gathers) on the same inputs: the comparison baseline, whose
  float atomics the kernels avoid; the two routes' outputs are compared at the timed size;
  one weighted F = 100 segment-sum pass over the same plan, for scale;
  a 2-layer GCN training step (100 -> 256 -> 47) with the edge weights tracked and untracked.

Method: every variant is warmed up, then the variants are timed in turn, --rounds times over (device events around one call
each); the medians are reported.  Algorithmic bytes come from the shapes: per edge the row pass reads G, w, col and writes t,
the column pass reads t2d and gathers t, the edge pass reads G, col and writes dL/dw; per node the arrays each pass touches.
One JSON record per graph goes to --out.

    python tools/bench_gcn_norm_grad.py [--out profiles/normgrad_bench.json] [--rounds 9] [--graphs uniform rmat]
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import tf_geometric_amd as tfg                                    # noqa: E402
from tf_geometric_amd import _lib as L, autograd as AG             # noqa: E402
from tf_geometric_amd.plan import CsrPlan, segment_reduce          # noqa: E402
from tf_geometric_amd.synthetic import synthetic_edges, rmat_edges, WORKLOADS   # noqa: E402

NORM, FILL, DIAG, LOOP, RENORM = "both", 1.0, 1.0, True, True
HIDDEN, CLASSES = 256, 47


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


def composed_backward(row, col, w, row_deg, G, S):
    """The formulas of include/tfgx_normgrad.h (BOTH, symmetric, renormalised self-loops) from torch operators; row / col are
    int64 [E] in CSR order.  index_add_ adds with float atomics: its bits change from run to run."""
    p = row_deg.pow(-0.5)
    p = torch.where(torch.isfinite(p), p, torch.zeros_like(p))
    dp = -0.5 * p * p * p
    gw = G * w
    pr, pc = p[row], p[col]
    A = torch.zeros_like(row_deg).index_add_(0, row, gw * pc) + S * FILL * p
    B = torch.zeros_like(row_deg).index_add_(0, col, gw * pr) + S * FILL * p
    D = (A + B) * dp
    return G * pr * pc + D[row]


def algorithmic_bytes(n, e):
    """Bytes each launch has to move, from the shapes alone (gathers of node arrays by column id are served by the caches and
    are not counted; the 4-byte gather of t is counted as 4 bytes, whatever line it arrives in)."""
    row = 4 * e * 4 + n * (4 + 4 + 4 + 4)            # G, w, col read, t written; row_ptr, row_deg, S read, A written
    col = 4 * e * 2 + n * (4 + 4 + 4 + 4 + 4)        # t2d read, t gathered; t_row_ptr, A, row_deg, S read, D written
    edge = 4 * e * 3 + n * (4 + 4 + 4)               # G, col read, dL/dw written; row_ptr, row_deg, D read
    return dict(row_pass=row, col_pass=col, edge_pass=edge, total=row + col + edge)


def bench_graph(name, ei, n, rounds, seed):
    dev = L.device()
    plan = CsrPlan.build(ei, n, n)
    E = plan.num_edges
    gen = torch.Generator(device=dev).manual_seed(seed)
    w = torch.rand(E, generator=gen, device=dev) + 0.5                       # CSR order, U(0.5, 1.5)
    G = torch.randn(E, generator=gen, device=dev)
    S = torch.randn(n, generator=gen, device=dev)
    AG._transposed(plan)                                                     # built once per plan, as in training
    w_out, self_coef, row_deg, _ = AG.gcn_norm_forward(plan, w, None, False, NORM, FILL, DIAG, LOOP, RENORM)
    new = lambda k: torch.empty(k, dtype=torch.float32, device=dev)          # noqa: E731
    scratch = (new(n), new(n), new(E), new(E))
    backward = lambda passes: AG.gcn_norm_backward(plan, w, row_deg, None, NORM, FILL, LOOP, RENORM, G, S, passes=passes,   # noqa: E731
                                                   scratch=scratch)
    ours = backward(L.NORMGRAD_ALL).clone()
    rec = dict(graph=name, nodes=n, edges=E, max_row=int(plan.in_degree().max().item()),
               max_col=int(plan.transposed().in_degree().max().item()), config="both/sym/self-loop/renorm")

    variants = {
        "row_pass_ms": lambda: backward(L.NORMGRAD_ROW_PASS),
        "col_pass_ms": lambda: backward(L.NORMGRAD_COL_PASS),
        "edge_pass_ms": lambda: backward(L.NORMGRAD_EDGE_PASS),
        "backward_ms": lambda: backward(L.NORMGRAD_ALL),
        "forward_ms": lambda: AG.gcn_norm_forward(plan, w, None, False, NORM, FILL, DIAG, LOOP, RENORM),
    }
    rec.update(measure(variants, rounds))
    assert torch.equal(ours, backward(L.NORMGRAD_ALL)), "two runs of the kernels differ"

    # the torch-composed baseline on the same inputs (its int64 index arrays are built outside the timed region)
    row = torch.repeat_interleave(torch.arange(n, device=dev), plan.in_degree().long())
    col = plan.col.long()
    theirs = composed_backward(row, col, w, row_deg, G, S)
    scale = float(theirs.abs().max())
    rec["composed_max_abs_diff"] = float((ours - theirs).abs().max())
    rec["composed_max_abs"] = scale
    rec.update(measure({"composed_backward_ms": lambda: composed_backward(row, col, w, row_deg, G, S)}, rounds))
    del row, col, theirs

    x = torch.randn((n, 100), generator=gen, device=dev)
    rec.update(measure({"segment_sum_f100_ms": lambda: segment_reduce(plan, x, L.SUM, w_csr=w_out, self_coef=self_coef)}, rounds))

    # a 2-layer GCN training step; the weights arrive in the caller's order (that of ei)
    l1, l2 = tfg.layers.GCN(HIDDEN, activation=tfg.relu, seed=seed + 1), tfg.layers.GCN(CLASSES, seed=seed + 2)
    l1._maybe_build([x])
    l2._maybe_build([torch.empty(1, HIDDEN)])
    l1.trainable(True)
    l2.trainable(True)
    w_user = torch.rand(int(ei.shape[1]), generator=gen, device=dev) + 0.5

    def step(weight, cache):
        def run():
            h = l1([x, ei, weight], cache=cache, training=True)
            out = l2([h, ei, weight], cache=cache, training=True)
            out.sum().backward()
        return run
    tracked = w_user.clone().requires_grad_(True)
    cache_t, cache_u = {tfg.plan.CACHE_KEY_PLAN: plan}, {tfg.plan.CACHE_KEY_PLAN: plan}
    rec.update(measure({"gcn_step_untracked_ms": step(w_user, cache_u), "gcn_step_tracked_ms": step(tracked, cache_t)}, rounds))
    assert tracked.grad is not None and bool(torch.isfinite(tracked.grad).all())

    rec["algorithmic_bytes"] = algorithmic_bytes(n, E)
    for key in ("row_pass", "col_pass", "edge_pass"):
        rec["{}_gb_per_s".format(key)] = round(rec["algorithmic_bytes"][key] / (rec[key + "_ms"] * 1e-3) / 1e9, 1)
    return rec


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                                 "normgrad_bench.json"))
    p.add_argument("--rounds", type=int, default=9)
    p.add_argument("--graphs", nargs="*", default=["uniform", "rmat"])
    p.add_argument("--nodes", type=int, default=WORKLOADS["products"][0])
    p.add_argument("--edges", type=int, default=WORKLOADS["products"][1])
    p.add_argument("--seed", type=int, default=0)
    args = p.parse_args()
    L.require_gpu()
    dev = L.device()
    out = dict(box="{} (torch {})".format(torch.cuda.get_device_name(0), torch.__version__), rounds=args.rounds, graphs=[])
    for name in args.graphs:
        if name == "uniform":
            ei = torch.from_numpy(synthetic_edges(args.nodes, args.edges, args.seed)).to(dev)
        else:
            ei = rmat_edges(args.nodes, args.edges, args.seed, dev)
        rec = bench_graph(name, ei.contiguous(), args.nodes, args.rounds, args.seed)
        print(json.dumps(rec), flush=True)
        out["graphs"].append(rec)
        del ei
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
