# coding=utf-8
"""examples/c_abi_gat_demo.cpp — a host with nothing but include/tfgx.h and libtfgx.so — takes the same GAT attention
route as the Python package (source blocks with the policy's KB on a dense graph; walk order + hub lists on an R-MAT graph;
one pass on a small uniform graph) and writes BIT-IDENTICAL output to nn/conv/gat.py:gat_attention on the same tensors."""
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from conftest import ROOT

pytestmark = pytest.mark.gpu


def _demo():
    from tf_geometric_amd import _build
    if not os.path.exists(_build.GAT_DEMO_BIN) or os.path.getmtime(_build.GAT_DEMO_SRC) > os.path.getmtime(_build.GAT_DEMO_BIN):
        _build.build_c_abi_gat_demo(verbose=False)
    return _build.GAT_DEMO_BIN


def _edges(kind):
    from tf_geometric_amd import synthetic
    g = torch.Generator(device="cuda")
    g.manual_seed(21)
    if kind == "dense":       # 40 k nodes x 100 in-edges, K | V table 21.8 MB at A = 8, W = 128: the policy picks KB = 3
        n = 40000
        row = torch.arange(n, device="cuda").repeat_interleave(100)
        col = torch.randint(0, n, (n * 100,), device="cuda", generator=g)
        return torch.stack([row, col]).to(torch.int32), n, 8, 8, 128
    if kind == "rmat":
        n = 1 << 15
        return synthetic.rmat_edges(n, 600000, 5, torch.device("cuda")), n, 8, 8, 64
    n = 3000
    row = torch.randint(0, n, (40000,), device="cuda", generator=g)
    col = torch.randint(0, n, (40000,), device="cuda", generator=g)
    return torch.stack([row, col]).to(torch.int32), n, 4, 16, 64


@pytest.mark.parametrize("kind", ["dense", "rmat", "uniform"])
def test_c_host_gat_routes_bit_identical(tfg, tmp_path, kind):
    from tf_geometric_amd.plan import CsrPlan
    from tf_geometric_amd.nn.conv import gat as G
    demo = _demo()
    ei, n, H, A, W = _edges(kind)
    g = torch.Generator(device="cuda")
    g.manual_seed(22)
    Q = torch.randn(n, A, device="cuda", generator=g)
    K = torch.randn(n, A, device="cuda", generator=g)
    V = torch.randn(n, W, device="cuda", generator=g)

    assert G.SOURCE_BLOCKS is None
    plan = CsrPlan.build(ei, n, n)
    before = G.SOURCE_BLOCK_STATS["launches"]
    ref = G.gat_attention(plan, Q, K, V, H)
    torch.cuda.synchronize()
    launches = G.SOURCE_BLOCK_STATS["launches"] - before

    np.array([n, H, A, W], dtype="<i8").tofile(str(tmp_path / "meta.bin"))
    ei_h = ei.cpu().numpy().astype("<i4")
    ei_h[0].tofile(str(tmp_path / "row.bin"))
    ei_h[1].tofile(str(tmp_path / "col.bin"))
    for name, t in (("q", Q), ("k", K), ("v", V)):
        t.cpu().numpy().astype("<f4").tofile(str(tmp_path / (name + ".bin")))
    res = subprocess.run(["timeout", "-k", "10", "120", demo, str(tmp_path)], cwd=ROOT, stdout=subprocess.PIPE,
                         stderr=subprocess.STDOUT)
    text = res.stdout.decode(errors="replace")
    assert res.returncode == 0 and "C_ABI_GAT_DEMO_OK" in text, text
    kb = int(re.search(r"KB=(\d+)", text).group(1))
    print("\n" + text.strip())

    if kind == "dense":
        assert plan.row_order() is None and plan.hub_info() is None
        assert launches == kb and kb >= 2 and "route=source_blocks" in text, (launches, text)
        assert kb == G.source_block_count(plan, A, W)
    elif kind == "rmat":
        assert plan.row_order() is not None and plan.hub_info() is not None
        assert launches == 0 and "route=one_pass" in text and "row_order=1" in text
        assert "hub_rows={} ".format(int(plan.hub_info()[0].shape[0])) in text, text
    else:
        assert plan.row_order() is None and plan.hub_info() is None
        assert launches == 0 and "route=one_pass" in text and "row_order=0 hub_rows=0" in text

    got = np.fromfile(str(tmp_path / "out.bin"), dtype="<f4")
    want = ref.cpu().numpy().reshape(-1)
    assert got.shape == want.shape
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), "{}: {} elements differ".format(
        kind, int((got.view(np.uint32) != want.view(np.uint32)).sum()))
