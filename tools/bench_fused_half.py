# coding=utf-8
"""Same-box A/B of the fused aggregate -> project launch over a 16-bit table (include/tfgx_fused_h16.h).

Shape: the products-shaped graph of bench.py (same generator, same seed) and the R-MAT graph of its `rmat` line; the GCN layer
F -> 256 (SUM, weighted, self_coef, bias, ReLU) and the mean GraphSAGE layer F -> 256 concat (two halves of 128 columns), F = 100
and 128; inference, and training forward + backward as layer 0 (the kernels and the bias take gradients, the input does not).
Variants, all in ONE process, interleaved round by round, one layer call per HIP-event pair, after warm-up calls of every
variant:

  f32_fused   (a) tfgx_aggregate_gemm_f32 on the widened float32 table (forced at F = 128, where plan.aggregate_gemm declines
                  large dense float32 tables at inference)
  h16_two     (b) what the 16-bit table got before this launch existed: tfgx_segment_reduce_h16 into a float32 [N, F] aggregate,
                  then the float32 GEMM
  h16_fused   (c) tfgx_aggregate_gemm_h16

The GraphSAGE variants over a 16-bit table (b, c) include widening the table for the self half, as the layer does on every call.
One JSON line per (graph, F, layer, mode) goes to --out (default profiles/fused_h16_products.jsonl): ms (min / median / max),
the run-to-run spread (max - min) / median of every variant, ratio c / b and c / a, and whether (c) is ahead of (b) by more than
the larger of their spreads — the yardstick plan._fused_h16_declines is decided from."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def stats(ms):
    s = sorted(ms)
    med = s[len(s) // 2] if len(s) % 2 else 0.5 * (s[len(s) // 2 - 1] + s[len(s) // 2])
    return {"ms_min": s[0], "ms_median": med, "ms_max": s[-1], "spread": (s[-1] - s[0]) / med, "launches": len(s)}


def time_variants(variants, rounds, warmup):
    ms = {k: [] for k in variants}
    for _ in range(warmup):
        for fn in variants.values():
            fn()
    torch.cuda.synchronize()
    for _ in range(rounds):                      # interleaved: every round times every variant once
        for k, fn in variants.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            ms[k].append(e0.elapsed_time(e1))
    return {k: stats(v) for k, v in ms.items()}


def layer_variants(tfg, plan, w_csr, self_coef, n, F, units, gen):
    """{(layer, mode): {variant: callable}} for one width."""
    from tf_geometric_amd import plan as P
    from tf_geometric_amd import autograd as AG
    L = tfg._lib
    h = tfg.prepare_half_features(torch.randn(n, F, generator=gen, device="cuda"), dtype=torch.bfloat16)
    xf = h.float()                     # the float32 route reads the SAME values: the widened table
    ku = units // 2
    K = (torch.randn(F, units, generator=gen, device="cuda") / F ** 0.5).requires_grad_(True)
    ks = (torch.randn(F, ku, generator=gen, device="cuda") / F ** 0.5).requires_grad_(True)
    kn = (torch.randn(F, ku, generator=gen, device="cuda") / F ** 0.5).requires_grad_(True)
    bias = torch.zeros(units, device="cuda", requires_grad=True)
    out = torch.empty((n, units), dtype=torch.float32, device="cuda")
    agg = torch.empty((n, F), dtype=torch.float32, device="cuda")
    g = torch.randn(n, units, generator=gen, device="cuda")
    Kd, ksd, knd, bd = K.detach(), ks.detach(), kn.detach(), bias.detach()
    R = L.ACT_RELU

    def gcn_inf(x):
        assert P.aggregate_gemm(plan, x, L.SUM, Kd, w_csr=w_csr, self_coef=self_coef, bias=bd, act=R, out=out) is not None

    def gcn_inf_two():
        P.segment_reduce(plan, h, L.SUM, w_csr=w_csr, self_coef=self_coef, out=agg)
        P.gemm_bias_act(agg, Kd, bias=bd, act=R, out=out)

    def sage_inf(x, self_rows):
        assert P.aggregate_gemm(plan, x, L.MEAN, knd, w_csr=w_csr, bias=bd[ku:].contiguous(), act=R, out=out[:, ku:]) is not None
        P.gemm_bias_act(self_rows(), ksd, bias=bd[:ku], act=R, out=out[:, :ku])

    def sage_inf_two():
        P.segment_reduce(plan, h, L.MEAN, w_csr=w_csr, out=agg)
        P.gemm_bias_act(h.float(), ksd, bias=bd[:ku], act=R, out=out[:, :ku])
        P.gemm_bias_act(agg, knd, bias=bd[ku:], act=R, out=out[:, ku:])

    def backward(o):
        for t in (K, ks, kn, bias):
            t.grad = None
        o.backward(g)

    def gcn_train(x):
        backward(AG.aggregate_project(plan, x, L.SUM, K, w_csr, self_coef, bias, R))

    def gcn_train_two():
        backward(AG.linear(AG.aggregate(plan, h, L.SUM, w_csr, self_coef), K, bias, R))

    def sage_train(x):
        backward(AG.sage_wide(plan, L.MEAN, x, ks, kn, w_csr, bias, R))

    def sage_train_two():
        backward(AG.dual_linear(h.float(), ks, AG.aggregate(plan, h, L.MEAN, w_csr), kn, bias, R))

    return {("gcn", "inference"): {"f32_fused": lambda: gcn_inf(xf), "h16_two": gcn_inf_two, "h16_fused": lambda: gcn_inf(h)},
            ("mean_sage", "inference"): {"f32_fused": lambda: sage_inf(xf, lambda: xf), "h16_two": sage_inf_two,
                                         "h16_fused": lambda: sage_inf(h, h.float)},
            ("gcn", "training"): {"f32_fused": lambda: gcn_train(xf), "h16_two": gcn_train_two, "h16_fused": lambda: gcn_train(h)},
            ("mean_sage", "training"): {"f32_fused": lambda: sage_train(xf), "h16_two": sage_train_two,
                                        "h16_fused": lambda: sage_train(h)}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--widths", default="100,128")
    ap.add_argument("--units", type=int, default=256)
    ap.add_argument("--graphs", default="uniform,rmat")
    ap.add_argument("--rounds", type=int, default=12)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--workload", default="products")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fused_h16_products.jsonl"))
    args = ap.parse_args()
    import tf_geometric_amd as tfg
    from tf_geometric_amd import plan as P
    from tf_geometric_amd import synthetic
    from tf_geometric_amd.nn.conv.gcn import gcn_norm_adj
    L = tfg._lib
    L.require_gpu()
    P.TFGX_FUSE_WIDE = True             # variant (a) is the float32 FUSED route at every width
    P.FUSED_H16_DECLINE_HUB_INFERENCE = False      # variant (c) is measured wherever the kernel takes the shape
    n, e_req, _ = synthetic.WORKLOADS[args.workload]
    gen = torch.Generator(device="cuda")
    gen.manual_seed(args.seed + 1)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:          # a fresh file every run: lines of two runs never mix
        for graph in args.graphs.split(","):
            if graph == "uniform":
                ei = L.as_i32(synthetic.synthetic_edge_stripe(n, e_req, seed=args.seed))
            else:
                ei = synthetic.rmat_edges(n, e_req, args.seed, torch.device("cuda"))
            normed = gcn_norm_adj(tfg.SparseMatrix(ei, None, [n, n]), sym=True)
            plan = normed.plan
            hub = plan.hub_info()
            for F in [int(v) for v in args.widths.split(",")]:
                with P.no_auto_promotion():
                    for (layer, mode), variants in layer_variants(tfg, plan, normed.w_csr, normed.self_coef, n, F, args.units, gen).items():
                        res = time_variants(variants, args.rounds, args.warmup)
                        a, b, c = (res[k]["ms_median"] for k in ("f32_fused", "h16_two", "h16_fused"))
                        spread = max(res["h16_two"]["spread"], res["h16_fused"]["spread"])
                        line = {"graph": graph, "workload": args.workload, "n": n, "edges": int(ei.shape[1]), "F": F, "units": args.units,
                                "layer": layer, "mode": mode, "hub_rows": 0 if hub is None else int(hub[0].shape[0]), "variants": res,
                                "c_over_b": c / b, "c_over_a": c / a, "spread": spread,
                                "c_ahead_of_b_by_more_than_spread": bool(c / b < 1.0 - spread),
                                "device": torch.cuda.get_device_name(0)}
                        fh.write(json.dumps(line) + "\n")
                        fh.flush()
                        print(json.dumps({k: line[k] for k in ("graph", "F", "layer", "mode", "c_over_b", "c_over_a", "spread",
                                                               "c_ahead_of_b_by_more_than_spread")},
                                         ), "a/b/c ms = {:.2f} / {:.2f} / {:.2f}".format(a, b, c), flush=True)
                torch.cuda.empty_cache()
            del normed, plan, ei
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
