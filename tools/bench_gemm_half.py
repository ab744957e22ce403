# coding=utf-8
"""Same-box A/B of the dense GEMM and its weight gradient reading a 16-bit table (include/tfgx_gemm_h16.h).

Shapes: the two GEMM shapes of bench.py's `configs` block (products 2.4 M x 100 -> 256, arxiv 170 k x 128 -> 256), plus the
wide raw-input projections the 16-bit tables are wanted for — 233 k x 602 -> 16 / 64 / 256 (Reddit-shaped), 173 k x 1433 -> 16
(Cora-wide), 2.4 M x 100 -> 47 / 256 and 2.4 M x 256 -> 128 (products-shaped) — for bf16 and fp16, at the table strides
roundup8(K) and plan.h16_friendly_ld(K).  Variants, all in ONE process, every shape, dtype and variant interleaved round by
round, one call per HIP-event pair, after warm-up calls of every variant; medians are reported:

  f32         (a) the float32 GEMM on an already widened table (which the caller then holds beside the 16-bit one)
  widen_f32   (b) tfgx_rows_h16_to_f32 into a float32 [M, K] buffer, then that GEMM — what "pass x.float()" costs per call
  h16         (c) tfgx_gemm_bias_act_cols_ws_h16

and the same three for the weight gradient (tfgx_gemm_tn_gated_f32 / widen + that / tfgx_gemm_tn_gated_h16, with bias).
One JSON line per (op, shape, dtype, stride) goes to --out (default profiles/gemm_h16.jsonl): ms (min / median / max), the
run-to-run spread (max - min) / median of every variant, c / a, c / b, and whether (c) is behind (b) by more than the spread."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = [(2449029, 100, 256), (170000, 128, 256),
          (233000, 602, 16), (233000, 602, 64), (233000, 602, 256), (173000, 1433, 16),
          (2449029, 100, 47), (2449029, 256, 128)]


def stats(ms):
    s = sorted(ms)
    med = s[len(s) // 2] if len(s) % 2 else 0.5 * (s[len(s) // 2 - 1] + s[len(s) // 2])
    return {"ms_min": s[0], "ms_median": med, "ms_max": s[-1], "spread": (s[-1] - s[0]) / med, "launches": len(s)}


def time_variants(groups, rounds, warmup):
    """groups: {key: {variant: callable}}; every round times every variant of every group once (interleaved)."""
    ms = {k: {v: [] for v in g} for k, g in groups.items()}
    for _ in range(warmup):
        for g in groups.values():
            for fn in g.values():
                fn()
    torch.cuda.synchronize()
    for _ in range(rounds):
        for k, g in groups.items():
            for v, fn in g.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fn()
                e1.record()
                e1.synchronize()
                ms[k][v].append(e0.elapsed_time(e1))
    return {k: {v: stats(t) for v, t in g.items()} for k, g in ms.items()}


def shape_groups(tfg, M, K, N, dtype, gen):
    """The forward and weight-gradient variants of one shape and dtype, for both table strides."""
    from tf_geometric_amd import plan as P
    L = tfg._lib
    lib = L.load_library()
    x = torch.randn((M, K), generator=gen, device="cuda")
    W = torch.randn((K, N), generator=gen, device="cuda") / K ** 0.5
    g = torch.randn((M, N), generator=gen, device="cuda")
    out = torch.empty((M, N), dtype=torch.float32, device="cuda")
    wide = torch.empty((M, K), dtype=torch.float32, device="cuda")          # (b)'s widened copy, rewritten every call
    groups = {}
    xf = None
    for ld in sorted({(K + 7) // 8 * 8, P.h16_friendly_ld(K)}):
        h = P.HalfRows.from_dense(x, dtype=dtype, ld=ld, gemm_operand=True)
        xf = h.float() if xf is None else xf           # the same values on either stride

        def widen(h=h):
            L.check(lib.tfgx_rows_h16_to_f32(L.ptr(h.table), h.ld, L.H16_DTYPES[h.dtype], M, K, L.ptr(wide), K, L.stream_ptr()),
                    "tfgx_rows_h16_to_f32")
            return wide

        groups[("gemm", ld)] = {"f32": lambda xf=xf: P.gemm_bias_act(xf, W, out=out),
                                "widen_f32": lambda: P.gemm_bias_act(widen(), W, out=out),
                                "h16": lambda h=h: P.gemm_bias_act(h, W, out=out)}
        groups[("gemm_tn", ld)] = {"f32": lambda xf=xf: P.gemm_tn(xf, g, want_bias=True),
                                   "widen_f32": lambda: P.gemm_tn(widen(), g, want_bias=True),
                                   "h16": lambda h=h: P.gemm_tn(h, g, want_bias=True)}
    return groups


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--dtypes", default="bf16,f16")
    ap.add_argument("--shapes", default="", help="M,K,N;M,K,N ... (default: the module's list)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gemm_h16.jsonl"))
    args = ap.parse_args()
    import tf_geometric_amd as tfg
    tfg._lib.require_gpu()
    shapes = [tuple(int(v) for v in s.split(",")) for s in args.shapes.split(";") if s] or SHAPES
    dtypes = {"bf16": torch.bfloat16, "f16": torch.float16}
    gen = torch.Generator(device="cuda")
    gen.manual_seed(args.seed + 1)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:          # a fresh file every run: lines of two runs never mix
        groups = {}                          # every shape, dtype, stride and op in ONE interleaved timing loop
        for M, K, N in shapes:
            for name in args.dtypes.split(","):
                for (op, ld), g in shape_groups(tfg, M, K, N, dtypes[name], gen).items():
                    groups[(op, M, K, N, name, ld)] = g
        res = time_variants(groups, args.rounds, args.warmup)
        for (op, M, K, N, name, ld), r in res.items():
            a, b, c = (r[k]["ms_median"] for k in ("f32", "widen_f32", "h16"))
            spread = max(v["spread"] for v in r.values())
            line = {"op": op, "M": M, "K": K, "N": N, "dtype": name, "ld": ld, "variants": r, "c_over_a": c / a, "c_over_b": c / b,
                    "spread": spread, "c_behind_b_by_more_than_spread": bool(c / b > 1.0 + spread),
                    "c_behind_a_by_more_than_spread": bool(c / a > 1.0 + spread), "device": torch.cuda.get_device_name(0)}
            fh.write(json.dumps(line) + "\n")
            print("{:8s} {:>8d} x {:4d} -> {:3d} {:4s} ld {:4d}  a/b/c ms = {:.3f} / {:.3f} / {:.3f}  c/a {:.2f} c/b {:.2f} spread {:.2f}"
                  .format(op, M, K, N, name, ld, a, b, c, c / a, c / b, spread), flush=True)


if __name__ == "__main__":
    main()
