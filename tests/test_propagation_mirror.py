# coding=utf-8
"""tests/propagation_mirror.py (the float64 reference of tests/test_gpu_propagation_backward.py) without a GPU: the float64
mirror reproduces each of the 13 tensor outputs the reference itself wrote for the `propagation_convs` case of
tests/golden/reference_cases.npz, at the band those goldens are held to (1e-5 + 1e-5 |ref|; 2e-4 for chebynet-None: key_tol in
reference_cases.py, explained in test_oracle_vs_reference.py).  The configurations the goldens do not hold (TAGCN / ChebyNet
with units >= F, k = 1, renorm=False, improved=True) are cross-checked against the oracle's restatement at the same band, on
the golden graph and on the directed graph of the GPU test (self-loops, duplicates, empty rows), where the self-loop rules
show."""
import os

import numpy as np
import pytest
import torch

from conftest import ROOT, assert_parity
import propagation_mirror as M
import reference_cases as RC

CASE = RC.by_name("propagation_convs")
GOLDEN = os.path.join(ROOT, "tests", "golden", "reference_cases.npz")


@pytest.fixture(scope="module")
def g():
    return CASE.inputs()


@pytest.fixture(scope="module")
def golden():
    blob = np.load(GOLDEN)
    pre = CASE.name + "::"
    return {k[len(pre):]: blob[k] for k in blob.files if k.startswith(pre)}


def _gin_mlp(w, dtype=torch.float64):
    wt = torch.as_tensor(np.asarray(w, np.float64)).to(dtype)
    return lambda h: torch.relu(h @ wt)


MIRROR = {
    "sgc-k1": lambda g: M.sgc(g["x"], g["ei"], g["w"], 1, g["k9"], g["b9"], "relu"),
    "sgc-k3": lambda g: M.sgc(g["x"], g["ei"], g["w"], 3, g["k9"], g["b9"], "relu"),
    "sgc-widening": lambda g: M.sgc(g["x"], g["ei"], g["w"], 2, g["kw30"], g["bw30"], "relu"),
    "tagcn": lambda g: M.tagcn(g["x"], g["ei"], g["w"], 3, g["tk"], g["tb"], "relu"),
    "appnp": lambda g: M.appnp(g["x"], g["ei"], g["w"], g["ks"], g["bs"], None, k=6, alpha=0.15),
    "ssgc": lambda g: M.ssgc(g["x"], g["ei"], g["w"], g["ks"], g["bs"], k=5, alpha=0.2),
    "ssgc-plain": lambda g: M.ssgc(g["x"], g["ei"], None, None, None, k=4),
    "chebynet-sym": lambda g: M.chebynet(g["x"], g["ei"], g["w"], 3, g["ck"], g["cb"], "relu", "sym"),
    "chebynet-rw": lambda g: M.chebynet(g["x"], g["ei"], g["w"], 3, g["ck"], g["cb"], "relu", "rw"),
    "chebynet-None": lambda g: M.chebynet(g["x"], g["ei"], g["w"], 3, g["ck"], g["cb"], "relu", None),
    "chebynet-sym-dynamic": lambda g: M.chebynet(g["x"], g["ei"], g["w"], 3, g["ck"], g["cb"], "relu", "sym",
                                                 use_dynamic_lambda_max=True),
    "gin": lambda g: M.gin(g["x"], g["ei"], _gin_mlp(g["gin_w"]), eps=0.3),
    "le_conv": lambda g: M.le_conv(g["x"], g["ei"], g["w"], g["lk"][0], g["lb"][0], g["lk"][1], g["lb"][1], g["lk"][2],
                                   g["lb"][2], "relu"),
}


def test_the_golden_file_holds_these_thirteen_tensors(golden):
    assert sorted(k for k in golden if not k.startswith("lambda_max")) == sorted(MIRROR)
    assert len(MIRROR) == 13


@pytest.mark.parametrize("name", sorted(MIRROR))
def test_float64_mirror_reproduces_the_reference(g, golden, name):
    got = MIRROR[name](g)
    assert got.dtype == torch.float64
    assert_parity(got.numpy(), golden[name], tol=CASE.tol_of(name), what=name)


@pytest.mark.parametrize("name", ["tagcn", "chebynet-sym", "chebynet-None", "sgc-widening"])
def test_rewritten_order_is_the_same_function(g, name):
    """The rewritten association (for the GPU test's tolerance only) is the literal one up to float64 rounding."""
    fn = {"tagcn": lambda o: M.tagcn(g["x"], g["ei"], g["w"], 3, g["tk"], g["tb"], "relu", order=o),
          "chebynet-sym": lambda o: M.chebynet(g["x"], g["ei"], g["w"], 3, g["ck"], g["cb"], "relu", "sym", order=o),
          "chebynet-None": lambda o: M.chebynet(g["x"], g["ei"], g["w"], 3, g["ck"], g["cb"], "relu", None, order=o),
          "sgc-widening": lambda o: M.sgc(g["x"], g["ei"], g["w"], 2, g["kw30"], g["bw30"], "relu", order=o)}[name]
    a, b = fn("literal"), fn("rewritten")
    assert float((a - b).abs().max()) <= 1e-12 * max(1.0, float(a.abs().max()))


def _graphs(g):
    s = M.structured_graph()
    rng = np.random.Generator(np.random.PCG64(5))
    s["x"] = rng.standard_normal((s["n"], s["f"]), dtype=np.float32)
    return {"golden": g, "structured": s}


@pytest.mark.parametrize("which", ["golden", "structured"])
def test_unreached_configurations_match_the_oracle(oracle, g, which):
    gg = _graphs(g)[which]
    x, ei, w, F = gg["x"], gg["ei"], gg["w"], gg["x"].shape[1]
    rng = np.random.Generator(np.random.PCG64(17))
    bias = lambda u: RC.small_bias(rng, u)      # noqa: E731

    def both(what, mirror, orc, tol=RC.TOL):
        assert_parity(mirror.numpy(), orc, tol=tol, what="{} ({})".format(what, which))

    for units in (7, 20):                        # units < F and units >= F (the concat form of the product)
        for k in (1, 3):
            tk, tb = RC.glorot(rng, F * (k + 1), units), bias(units)
            both("tagcn k={} units={}".format(k, units), M.tagcn(x, ei, w, k, tk, tb, "relu"),
                 oracle.tagcn(x, ei, w, k, tk, tb, "relu"))
    tk, tb = RC.glorot(rng, F * 3, 9), bias(9)
    for cfg in (dict(renorm=True), dict(improved=True), dict(renorm=True, improved=True)):
        both("tagcn {}".format(cfg), M.tagcn(x, ei, w, 2, tk, tb, None, **cfg), oracle.tagcn(x, ei, w, 2, tk, tb, None, **cfg))
    k9, b9 = RC.glorot(rng, F, 9), bias(9)
    for cfg in (dict(renorm=False), dict(improved=True), dict(renorm=False, improved=True)):
        both("sgc {}".format(cfg), M.sgc(x, ei, w, 2, k9, b9, "relu", **cfg), oracle.sgc(x, ei, w, 2, k9, b9, "relu", **cfg))
    for norm in ("sym", "rw", None):
        for units in (5, 16):
            for k in (1, 2, 4):
                if norm is None and k > 2 and which == "structured":
                    continue        # degree 60 cubed: the oracle rounds every hop to float32, far outside a 1e-5 band
                ck, cb = [RC.glorot(rng, F, units) for _ in range(k)], bias(units)
                both("chebynet {} k={} units={}".format(norm, k, units), M.chebynet(x, ei, w, k, ck, cb, "relu", norm),
                     oracle.chebynet(x, ei, w, k, ck, cb, "relu", norm), tol=RC.TOL if norm is not None else 2e-4)
    ck, cb = [RC.glorot(rng, F, 16) for _ in range(3)], bias(16)
    both("chebynet dynamic", M.chebynet(x, ei, w, 3, ck, cb, None, "sym", use_dynamic_lambda_max=True),
         oracle.chebynet(x, ei, w, 3, ck, cb, None, "sym", use_dynamic_lambda_max=True))
    both("chebynet unweighted", M.chebynet(x, ei, None, 2, ck[:2], cb, None, "rw"), oracle.chebynet(x, ei, None, 2, ck[:2], cb, None, "rw"))
    lk, lb = [RC.glorot(rng, F, 6) for _ in range(3)], [bias(6) for _ in range(3)]
    both("le_conv unweighted", M.le_conv(x, ei, None, lk[0], lb[0], lk[1], None, lk[2], lb[2]),
         oracle.le_conv(x, ei, None, lk[0], lb[0], lk[1], None, lk[2], lb[2]))
    ks, bs = [RC.glorot(rng, F, 16), RC.glorot(rng, 16, 6)], [bias(16), bias(6)]
    both("appnp k=0", M.appnp(x, ei, w, ks, bs, None, k=0), oracle.appnp(x, ei, w, ks, bs, "relu", None, k=0))
    both("appnp no mlp", M.appnp(x, ei, w, None, None, "relu", k=3, alpha=0.15),
         oracle.appnp(x, ei, w, None, None, "relu", "relu", k=3, alpha=0.15))


def test_structured_graph_has_the_structure_the_gpu_test_relies_on():
    s = M.structured_graph()
    row, col, n = s["ei"][0], s["ei"][1], s["n"]
    assert n == 130 and 850 <= row.size <= 950 and s["w"].min() >= 0.5 and s["w"].max() <= 1.5
    indeg, outdeg = np.bincount(row, minlength=n), np.bincount(col, minlength=n)
    assert (row == col).sum() >= 8
    pairs = row.astype(np.int64) * n + col
    assert row.size - np.unique(pairs).size >= 50                     # duplicated edges
    assert indeg[127] == indeg[128] == 0 and outdeg[127] > 0 and outdeg[128] > 0
    assert indeg[129] == 0 and outdeg[129] == 0                        # no edge at all
    assert indeg[s["hub"]] >= 40 and outdeg[s["hub"]] >= 40
    assert not np.all(np.diff(row) >= 0)                               # shuffled


def test_mirror_is_differentiable_through_the_normalisation():
    """d/d edge_weight exists and is finite for every normalised form, rows of degree 0 included."""
    s = M.structured_graph()
    x = torch.randn(s["n"], 4, dtype=torch.float64, generator=torch.Generator().manual_seed(0))
    k = torch.randn(4, 3, dtype=torch.float64, generator=torch.Generator().manual_seed(1))
    for fn in (lambda w: M.sgc(x, s["ei"], w, 2, k), lambda w: M.sgc(x, s["ei"], w, 2, k, renorm=False),
               lambda w: M.chebynet(x, s["ei"], w, 2, [k, k], normalization_type="sym"),
               lambda w: M.chebynet(x, s["ei"], w, 2, [k, k], normalization_type="rw"),
               lambda w: M.chebynet(x, s["ei"], w, 2, [k, k], normalization_type=None)):
        w = torch.as_tensor(s["w"]).double().requires_grad_(True)
        fn(w).square().sum().backward()
        assert w.grad is not None and bool(torch.isfinite(w.grad).all()) and float(w.grad.abs().max()) > 0
