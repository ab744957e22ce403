# coding=utf-8
"""Same-box A/B of the 16-bit feature tables (include/tfgx_h16.h) against the float32 segment-reduce routes.

Shape: the products-shaped graph of bench.py (same generator, same seed) and the R-MAT graph of its `rmat` line; widths
F = 100, 128, 256, 512; the GCN launch of the headline (SUM, weighted, self_coef).  Variants, all in ONE process, interleaved
round by round, one launch per HIP-event pair, after warm-up launches of every variant:

  f32_plain      tfgx_segment_reduce_f32 on the dense float32 table (promotion to the static layout switched off)
  f32_static     ... on the split-row static layout, where SplitRows.wanted says it applies (F = 100)
  bf16_f32       tfgx_segment_reduce_h16, bf16 table on the friendly stride, float32 output
  bf16_bf16      ... bf16 output
  bf16_f32_ld104 F = 100 only: the dense 16-byte aligned stride (104 elements, 2.5 lines per row) against 128 (2 lines)
  bf16_f32_blocks  F >= 256: column blocks of 128 elements on grid.y (wide_blocks = +1) against one burst per row

One JSON line per (graph, width) goes to --out (default profiles/h16_products.jsonl): ms (min / median / max of the timed
launches), the run-to-run spread (max - min) / median, algorithmic bytes, 128-byte lines per gathered row, the ratios to
f32_plain and the bar of the issue (ratio < 1 - spread and ratio <= lines ratio x 1.25).  --rocprof re-runs one width in a child
process under `rocprofv3 --kernel-trace --stats` and appends the kernel summary."""
import argparse
import csv
import glob
import json
import os
import subprocess
import sys
import tempfile

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def lines_per_row(row_bytes, stride_bytes):
    import math
    period = 128 // math.gcd(stride_bytes, 128)
    return sum(((i * stride_bytes) % 128 + row_bytes - 1) // 128 + 1 for i in range(period)) / period


def stats(ms):
    s = sorted(ms)
    med = s[len(s) // 2] if len(s) % 2 else 0.5 * (s[len(s) // 2 - 1] + s[len(s) // 2])
    return {"ms_min": s[0], "ms_median": med, "ms_max": s[-1], "spread": (s[-1] - s[0]) / med, "launches": len(s)}


def run_width(tfg, plan, w_csr, self_coef, n, e_agg, F, rounds, warmup, gen):
    from tf_geometric_amd import plan as P
    L = tfg._lib
    x = torch.randn(n, F, generator=gen, device="cuda")
    h = tfg.prepare_half_features(x, dtype=torch.bfloat16)
    x = h.float()                      # the float32 routes read the SAME values: the widened table
    out32 = torch.empty((n, F), dtype=torch.float32, device="cuda")
    out16 = P.HalfRows.empty(n, F, torch.bfloat16, "cuda")
    kw = dict(w_csr=w_csr, self_coef=self_coef)
    variants = {"f32_plain": lambda: P.segment_reduce(plan, x, L.SUM, out=out32, **kw),
                "bf16_f32": lambda: P.segment_reduce(plan, h, L.SUM, out=out32, **kw),
                "bf16_bf16": lambda: P.segment_reduce(plan, h, L.SUM, out=out16, out_dtype=torch.bfloat16, **kw)}
    names = {"f32_plain": P.segment_reduce(plan, x, L.SUM, describe=True, **kw), "bf16_f32": P.segment_reduce(plan, h, L.SUM, describe=True, **kw)}
    if P.SplitRows.wanted(n, F) and plan.hub_info() is None:
        rows = P.SplitRows.from_dense(x).with_edge_tail(plan)
        variants["f32_static"] = lambda: P.segment_reduce(plan, rows, L.SUM, out=out32, **kw)
    if (F + 7) // 8 * 8 != h.ld:
        h_dense = P.HalfRows.from_dense(x, dtype=torch.bfloat16, ld=(F + 7) // 8 * 8)
        variants["bf16_f32_ld%d" % h_dense.ld] = lambda: P.segment_reduce(plan, h_dense, L.SUM, out=out32, **kw)
    if F >= 256 and F % 64 == 0:
        variants["bf16_f32_blocks"] = lambda: P.segment_reduce(plan, h, L.SUM, out=out32, wide_blocks=1, **kw)
        variants["bf16_f32_burst"] = lambda: P.segment_reduce(plan, h, L.SUM, out=out32, wide_blocks=-1, **kw)
        names["bf16_f32_blocks"] = P.segment_reduce(plan, h, L.SUM, describe=True, wide_blocks=1, **kw)
    ms = {k: [] for k in variants}
    with P.no_auto_promotion():
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
        ref = P.segment_reduce(plan, x, L.SUM, **kw)
        same = bool(torch.equal(ref, P.segment_reduce(plan, h, L.SUM, **kw)))
    res = {k: stats(v) for k, v in ms.items()}
    ld32 = int(x.stride(0))
    lines32, lines16 = lines_per_row(4 * F, 4 * ld32), lines_per_row(2 * ((F + 7) // 8 * 8), 2 * h.ld)
    # algorithmic bytes: every edge gathers one row and reads (col, w); every destination reads its own row (self_coef) and
    # self_coef / row_ptr, and writes one output row
    def alg(elt_in, elt_out):
        return e_agg * (F * elt_in + 8) + n * (F * elt_in + F * elt_out + 12)
    base = res["f32_plain"]["ms_median"]
    for k, r in res.items():
        r["ratio_to_f32_plain"] = r["ms_median"] / base
    res["f32_plain"]["bytes_alg"], res["bf16_f32"]["bytes_alg"], res["bf16_bf16"]["bytes_alg"] = alg(4, 4), alg(2, 4), alg(2, 2)
    spread = max(res["f32_plain"]["spread"], res["bf16_f32"]["spread"])
    ratio = res["bf16_f32"]["ratio_to_f32_plain"]
    return {"F": F, "n": n, "edges": e_agg, "ld_f32": ld32, "ld_bf16": h.ld, "lines_per_row_f32": lines32, "lines_per_row_bf16": lines16,
            "kernels": names, "variants": res, "bit_identical_to_f32_route": same,
            "bar": {"ratio": ratio, "spread": spread, "lines_ratio": lines16 / lines32, "lines_ratio_x1.25": 1.25 * lines16 / lines32,
                    "below_one_by_more_than_spread": bool(ratio < 1.0 - spread), "within_lines_bar": bool(ratio <= 1.25 * lines16 / lines32)}}


def rocprof_summary(args):
    """One width in a child process under rocprofv3 --kernel-trace --stats (tracing only: no counters in the same run)."""
    tmp = tempfile.mkdtemp(prefix="h16_rocprof_")
    cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", tmp, "-o", "h16", "--", sys.executable, os.path.abspath(__file__),
           "--widths", "100", "--graphs", "uniform", "--rounds", "5", "--warmup", "1", "--out", os.path.join(tmp, "child.jsonl")]
    p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=900)
    rows = []
    for path in glob.glob(os.path.join(tmp, "**", "*kernel_stats.csv"), recursive=True):
        with open(path) as fh:
            for r in csv.DictReader(fh):
                if "seg_reduce" in r.get("Name", ""):
                    rows.append({k: r[k] for k in ("Name", "Calls", "TotalDurationNs", "AverageNs", "MinNs", "MaxNs", "Percentage") if k in r})
    return {"rocprofv3": "--kernel-trace --stats, F = 100, uniform graph, 1 warm-up + 5 timed rounds", "returncode": p.returncode,
            "kernel_stats": rows, "tail": p.stdout.decode(errors="replace")[-400:] if not rows else ""}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--widths", default="100,128,256,512")
    ap.add_argument("--graphs", default="uniform,rmat")
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--workload", default="products")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "h16_products.jsonl"))
    ap.add_argument("--rocprof", action="store_true")
    args = ap.parse_args()
    import tf_geometric_amd as tfg
    from tf_geometric_amd import synthetic
    from tf_geometric_amd.nn.conv.gcn import gcn_norm_adj
    L = tfg._lib
    L.require_gpu()
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
                line = run_width(tfg, plan, normed.w_csr, normed.self_coef, n, int(ei.shape[1]), F, args.rounds, args.warmup, gen)
                line.update(graph=graph, workload=args.workload, hub_rows=0 if hub is None else int(hub[0].shape[0]),
                            device=torch.cuda.get_device_name(0))
                fh.write(json.dumps(line) + "\n")
                fh.flush()
                print(json.dumps({k: line[k] for k in ("graph", "F", "bar")}), flush=True)
                torch.cuda.empty_cache()
            del normed, plan, ei
            torch.cuda.empty_cache()
        if args.rocprof:
            fh.write(json.dumps(rocprof_summary(args)) + "\n")


if __name__ == "__main__":
    main()
