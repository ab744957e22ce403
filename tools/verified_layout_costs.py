# coding=utf-8
"""Costs of the verified static layout of plan.segment_reduce at products shape, one JSON line:
  plain_ms           the plain route (TFGX_STATIC_LAYOUT=explicit behaviour), HIP events over back-to-back launches
  verified_ms        the promoted table served through the verified route (check + gather + repair launch + 4-byte read-back)
  hidden_behind_counter_ms_per_call   a DIFFERENT table written into the same storage before every call, behind torch's
                     version counter (x.data.copy_): call 1 plain (first sighting), call 2 builds the layout, call 3 is the
                     first stale call (check fails, repair recomputes), later calls run demoted on the plain route
  hidden_torch_visible_ms_per_call    the same with x.copy_ (the version counter moves): never promoted
Each call of the two hidden-layer series is timed alone (events, synchronised).

    python tools/verified_layout_costs.py [--steps 20]"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    args = ap.parse_args()
    import tf_geometric_amd as tfg
    from tf_geometric_amd import plan as P, synthetic
    L = tfg._lib
    n, e, f = synthetic.WORKLOADS["products"]
    ei = L.as_i32(synthetic.synthetic_edges(n, e, seed=0))
    g = torch.Generator(device="cuda")
    g.manual_seed(1)
    x = torch.randn(n, f, generator=g, device="cuda")
    w = torch.rand(int(ei.shape[1]), generator=g, device="cuda") + 0.5
    sc = torch.rand(n, generator=g, device="cuda") + 0.5
    plan = P.CsrPlan.build(ei, n, n)
    w_csr = plan.edge_attr_to_csr(w)
    out = torch.empty_like(x)
    call = lambda t: P.segment_reduce(plan, t, L.SUM, w_csr=w_csr, self_coef=sc, out=out)   # noqa: E731

    def loop(t, steps):
        for _ in range(3):
            call(t)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(steps):
            call(t)
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / steps

    def one(t):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        call(t)
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1)

    P.AUTO_STATIC_LAYOUT = False
    plain_ms = loop(x, args.steps)
    P.AUTO_STATIC_LAYOUT = True
    verified_ms = loop(x, args.steps)
    res = {"plain_ms": plain_ms, "verified_ms": verified_ms,
           "verified_kernel": P.segment_reduce(plan, x, L.SUM, w_csr=w_csr, self_coef=sc, out=out, describe=True)}
    tables = [torch.randn(n, f, generator=g, device="cuda") for _ in range(2)]
    for name, write in (("hidden_behind_counter_ms_per_call", lambda h, s: h.data.copy_(s)),
                        ("hidden_torch_visible_ms_per_call", lambda h, s: h.copy_(s))):
        h = torch.empty_like(x)
        stats0 = dict(P.VERIFIED_STATS)
        ms = []
        for i in range(8):
            write(h, tables[i % 2])
            ms.append(one(h))
        res[name] = ms
        res[name.replace("ms_per_call", "stats")] = {k: P.VERIFIED_STATS[k] - stats0[k] for k in stats0}
        del h
    print(json.dumps(res))


if __name__ == "__main__":
    main()
