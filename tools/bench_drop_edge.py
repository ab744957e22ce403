# coding=utf-8
"""DropEdge per-step cost: what a user writes without it against tfg.nn.drop_edge, sorted and derived plans.

    python tools/bench_drop_edge.py [--rounds 12] [--out profiles/drop_edge_products.jsonl] [--shapes products,sweep]

One process, variants interleaved round by round, host clock around work that ends in a device synchronise, medians with
the run-to-run spread (quartiles, min, max).  Per shape and rate, one JSON line with, in milliseconds:
  a_mask   torch.rand(E) >= rate and the three boolean-mask gathers (row, col, weight; nonzero syncs inside)
  a_sort   CsrPlan.build of that list + plan.transposed()                          (a) = a_mask + a_sort
  b_drop   drop_edge without a parent plan: the compaction alone (ids, list, weight gather)
  b_sort   CsrPlan.build of its output + plan.transposed()                         (b) = b_drop + b_sort
  c_drop   drop_edge with the parent's plan and transposed plan: both derived      (c) = c_drop
  step_a / step_b / step_c   a 2-layer GCN training step (forward + backward) on the plans each variant produced
Shapes: products (N = 2 449 029, E = 123 718 280; uniform and R-MAT endpoints), and a size sweep of uniform graphs for the
dispatch rule of nn/sampling/drop_edge.py (DERIVE_PLANS).  All three variants' plans are compared bit for bit once per shape
(with the keep mask of (b) fed to (a)) before anything is timed."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import tf_geometric_amd as tfg   # noqa: E402
from tf_geometric_amd.plan import CsrPlan   # noqa: E402
from tf_geometric_amd.nn.sampling.drop_edge import drop_edge_index   # noqa: E402

PRODUCTS = (2449029, 123718280)
SWEEP = [(2000, 20000), (20000, 500000), (200000, 8000000), (800000, 32000000)]


def edges(n, e, kind, dev, seed):
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    if kind == "uniform":
        return torch.randint(0, n, (2, e), device=dev, generator=g, dtype=torch.int32)
    bits = max(1, int(np.ceil(np.log2(n))))          # R-MAT, quadrant probabilities 0.57 / 0.19 / 0.19 / 0.05
    row = torch.zeros(e, dtype=torch.int64, device=dev)
    col = torch.zeros(e, dtype=torch.int64, device=dev)
    for _ in range(bits):
        u = torch.rand(e, device=dev, generator=g)
        q = (u >= 0.57).long() + (u >= 0.76).long() + (u >= 0.95).long()
        row, col = row * 2 + q // 2, col * 2 + q % 2
    return torch.stack([row % n, col % n]).to(torch.int32)


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def stats(v):
    v = np.asarray(v, np.float64)
    return dict(median=round(float(np.median(v)), 4), p25=round(float(np.percentile(v, 25)), 4),
                p75=round(float(np.percentile(v, 75)), 4), min=round(float(v.min()), 4), max=round(float(v.max()), 4))


def sorted_plans(ei, n):
    plan = CsrPlan.build(ei, n, n)
    plan.transposed()
    return plan


def run_shape(name, n, e, kind, rate, rounds, with_step, dev):
    ei = edges(n, e, kind, dev, seed=1)
    w = torch.rand(e, device=dev) + 0.5
    parent = sorted_plans(ei, n)
    ei_planned = ei.view(ei.shape)
    ei_planned._tfgx_plan = parent

    def a_mask(keep=None):
        if keep is None:
            keep = torch.rand(e, device=dev) >= rate
        return torch.stack([ei[0][keep], ei[1][keep]]), w[keep]

    def b_drop(seed):
        return tfg.nn.drop_edge([ei, w], rate=rate, training=True, seed=seed)

    def c_drop(seed):
        return tfg.nn.drop_edge([ei_planned, w], rate=rate, training=True, seed=seed, derive_plan=True)

    # same graph from all three (the mask of seed 1 handed to (a)), plans bit for bit
    (b_ei, b_w), (c_ei, c_w) = b_drop(1), c_drop(1)
    keep = torch.zeros(e, dtype=torch.bool, device=dev)
    keep[drop_edge_index(ei, rate, 1)[1].long()] = True
    a_ei, a_w = a_mask(keep)
    assert torch.equal(a_ei, b_ei) and torch.equal(b_ei, c_ei) and torch.equal(a_w, b_w) and torch.equal(b_w, c_w)
    ref, got = sorted_plans(b_ei, n), c_ei._tfgx_plan
    for p, q in ((ref, got), (ref._transposed, got._transposed)):
        assert torch.equal(p.row_ptr, q.row_ptr) and torch.equal(p.col, q.col) and torch.equal(p.perm, q.perm)
    del ref, got, keep, a_ei, a_w, b_ei, b_w, c_ei, c_w

    step = None
    if with_step:
        x = torch.randn(n, 100, device=dev)
        y = torch.randint(0, 47, (n,), device=dev)
        gcn0, gcn1 = tfg.layers.GCN(128, activation=tfg.relu), tfg.layers.GCN(47)
        gcn0._maybe_build([x])
        gcn1._maybe_build([torch.empty(1, 128, device=dev)])
        gcn0.trainable(True)
        gcn1.trainable(True)

        def step(d_ei, d_w):
            cache = {}
            for p in gcn0.parameters() + gcn1.parameters():
                p.grad = None
            h = gcn0([x, d_ei, d_w], cache=cache, training=True)
            out = gcn1([h, d_ei, d_w], cache=cache, training=True)
            torch.nn.functional.cross_entropy(out, y).backward()

    t = {k: [] for k in ("a_mask", "a_sort", "b_drop", "b_sort", "c_drop", "step_a", "step_b", "step_c")}
    for r in range(-2, rounds):              # two warm-up rounds
        rec = {}
        rec["a_mask"], (a_ei, a_w) = timed(a_mask)
        rec["a_sort"], a_plan = timed(lambda: sorted_plans(a_ei, n))
        a_ei._tfgx_plan = a_plan
        if step is not None:
            rec["step_a"], _ = timed(lambda: step(a_ei, a_w))
        del a_ei, a_w, a_plan
        rec["b_drop"], (b_ei, b_w) = timed(lambda: b_drop(100 + r))
        rec["b_sort"], b_plan = timed(lambda: sorted_plans(b_ei, n))
        b_ei._tfgx_plan = b_plan
        if step is not None:
            rec["step_b"], _ = timed(lambda: step(b_ei, b_w))
        del b_ei, b_w, b_plan
        rec["c_drop"], (c_ei, c_w) = timed(lambda: c_drop(100 + r))
        if step is not None:
            rec["step_c"], _ = timed(lambda: step(c_ei, c_w))
        del c_ei, c_w
        if r >= 0:
            for k, v in rec.items():
                t[k].append(v)
    row = dict(shape=name, kind=kind, n=n, E=e, rate=rate, rounds=rounds, unit="ms", device=torch.cuda.get_device_name(0))
    for k, v in t.items():
        if v:
            row[k] = stats(v)
    row["a_total"] = stats(np.add(t["a_mask"], t["a_sort"]))
    row["b_total"] = stats(np.add(t["b_drop"], t["b_sort"]))
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=12)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                                  "drop_edge_products.jsonl"))
    ap.add_argument("--shapes", default="products,sweep")
    ap.add_argument("--no-step", action="store_true", help="skip the GCN training step")
    args = ap.parse_args()
    if args.rounds < 12:
        print("note: fewer than 12 rounds — not a result to quote", file=sys.stderr)
    tfg._lib.require_gpu()
    dev = torch.device("cuda", 0)
    jobs = []
    if "sweep" in args.shapes:
        jobs += [("sweep", n, e, "uniform", 0.5, False) for n, e in SWEEP]
    if "products" in args.shapes:
        jobs += [("products", PRODUCTS[0], PRODUCTS[1], kind, rate, not args.no_step)
                 for kind in ("uniform", "rmat") for rate in (0.1, 0.5)]
    if "tiny" in args.shapes:       # rehearsal of the whole path
        jobs += [("tiny", 3000, 50000, kind, 0.5, not args.no_step) for kind in ("uniform", "rmat")]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        for name, n, e, kind, rate, with_step in jobs:
            row = run_shape(name, n, e, kind, rate, args.rounds, with_step, dev)
            f.write(json.dumps(row) + "\n")
            f.flush()
            print(json.dumps(row), flush=True)
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
