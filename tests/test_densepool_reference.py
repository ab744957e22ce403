# coding=utf-8
"""tests/golden/densepool_cases.npz is what the reference's own diff_pool, diff_pool_coarsen, min_cut_pool,
min_cut_pool_coarsen and min_cut_pool_compute_losses produce on the inputs of tests/densepool_cases.py (no GPU needed); the
live comparison runs where the reference checkout exists.  The float64 mirror (tests/densepool_mirror.py), which the GPU
gradient tests take as their reference, is held to the same file here: index arrays exactly, values at 1e-6 (1 + |ref|) —
the mirror is float64 and the reference float32, whose sums here have at most a few dozen terms of order one."""
import os
import sys

import numpy as np
import pytest

from conftest import ROOT
import densepool_cases as dc
import densepool_mirror as dm

sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import make_densepool_golden as mk     # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden", "densepool_cases.npz")
MIRROR_TOL = 1e-6


@pytest.fixture(scope="module")
def golden():
    return dict(np.load(GOLDEN))


def _close(got, ref, what):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert got.shape == ref.shape, what
    err = np.abs(got - ref) / (1.0 + np.abs(ref))
    assert (err.max() if err.size else 0.0) <= MIRROR_TOL, "{}: max |d| / (1 + |ref|) = {:.3e}".format(what, float(err.max()))


def test_golden_file_is_small_and_names_its_backend(golden):
    assert os.path.getsize(GOLDEN) < 100 * 1024
    assert str(golden["__backend__"]) in ("tensorflow", "numpy-stub")


@pytest.mark.parametrize("case", dc.CASES, ids=lambda c: c.name)
def test_golden_inputs_are_the_case_table(case, golden):
    assert str(golden["{}::__inputs_sha256__".format(case.name)]) == mk.inputs_digest(case.inputs())
    for cfg in case.configs:
        assert "{}::{}/edge_index".format(case.name, cfg) in golden, cfg      # no configuration was left out
    for cfg in dc.LOSS_CONFIGS:
        assert "{}::{}/cut_loss".format(case.name, cfg) in golden and "{}::{}/orth_loss".format(case.name, cfg) in golden


def test_the_generators_conditions_hold():
    big, small = dc.checks(dc.batch())
    assert big <= dc.MAX_LOGIT and small >= dc.MIN_ENTRY


def test_golden_covers_the_corner_cases(golden):
    g = dc.batch()
    K = dc.K
    assert (g["w"] >= 0.5).all() and (g["w"] <= 1.5).all()
    assert (np.diff(g["gid"]) < 0).any()                                               # unsorted graph ids
    assert (g["gid"][g["ei"][0]] == g["gid"][g["ei"][1]]).all()                        # no edge between two graphs
    assert (g["ei"][0] != g["ei"][1]).all() and np.unique(g["ei"], axis=1).shape[1] == g["ei"].shape[1]
    counts = np.bincount(g["gid"])
    with_edges = np.unique(g["gid"][g["ei"][0]])
    assert (counts == 1).sum() == 1 and np.setdiff1d(np.flatnonzero(counts > 1), with_edges).size == 1
    assert np.setdiff1d(np.flatnonzero(np.isin(g["gid"], with_edges)), g["ei"].reshape(-1)).size >= 1      # an isolated node
    for cfg in dc.ALL_CONFIGS:
        ei = golden["densepool::{}/edge_index".format(cfg)]
        assert ei.dtype == np.int32 and golden["densepool::{}/edge_weight".format(cfg)].dtype == np.float32
        assert np.array_equal(np.unique(ei[0] // K), with_edges)                       # a graph without edges: no pooled edges
        assert (ei[0] // K == ei[1] // K).all()                                        # block-diagonal
        full = len(with_edges) * K * K
        if cfg.startswith("min_cut"):
            assert (ei[0] != ei[1]).all() and ei.shape[1] == full - len(with_edges) * K
        else:
            assert ei.shape[1] == full
        assert np.array_equal(golden["densepool::{}/node_graph_index".format(cfg)], np.repeat(np.arange(len(counts)), K))
        assert golden["densepool::{}/x".format(cfg)].shape[0] == len(counts) * K


@pytest.mark.parametrize("case", dc.CASES, ids=lambda c: c.name)
def test_golden_file_is_what_the_reference_produces(case, golden):
    from oracle.ref_harness import reference_available
    if not reference_available():
        pytest.skip("reference checkout not present")
    outs = case.ref(mk.reference(), case.inputs())
    keys = [k for k in golden if k.startswith(case.name + "::") and not k.endswith("__")]
    assert sorted(keys) == sorted(case.name + "::" + k for k in outs)
    for k, v in outs.items():
        ref = golden[case.name + "::" + k]
        v = np.asarray(v)
        assert v.dtype == ref.dtype and v.shape == ref.shape, k
        assert np.array_equal(v, ref), "{}: live reference run differs from the committed golden file".format(k)


def _gnns(g):
    return dc._f64((g["feature_kernel"], g["feature_bias"])), dc._f64((g["assign_kernel"], g["assign_bias"]))


def _hold(m, golden, pre):
    assert np.array_equal(m["edge_index"], golden[pre + "edge_index"]), pre
    assert np.array_equal(m["node_graph_index"], golden[pre + "node_graph_index"]), pre
    _close(m["x"].numpy(), golden[pre + "x"], pre + "x")
    _close(m["edge_weight"].numpy(), golden[pre + "edge_weight"], pre + "edge_weight")


@pytest.mark.parametrize("cfg", dc.DIFF_CONFIGS, ids=lambda c: c[0])
def test_mirror_reproduces_the_reference_diff_pool(cfg, golden):
    name, weighted, bias, act = cfg
    g = dc.batch()
    fg, ag = _gnns(g)
    m = dm.diff_pool_mirror(g["x"], g["ei"], g["w"] if weighted else None, g["gid"], fg, ag,
                            bias=dc._f64((g["bias"],))[0] if bias else None, activation=act)
    _hold(m, golden, "densepool::diff_pool/{}/".format(name))


@pytest.mark.parametrize("cfg", dc.MINCUT_CONFIGS, ids=lambda c: c[0])
def test_mirror_reproduces_the_reference_min_cut_pool(cfg, golden):
    name, weighted, bias, normed = cfg
    g = dc.batch()
    fg, ag = _gnns(g)
    m = dm.min_cut_pool_mirror(g["x"], g["ei"], g["w"] if weighted else None, g["gid"], fg, ag,
                               bias=dc._f64((g["bias"],))[0] if bias else None, gnn_use_normed_edge=normed)
    pre = "densepool::min_cut_pool/{}/".format(name)
    _hold(m, golden, pre)
    _close(m["cut_loss"].numpy(), golden[pre + "cut_loss"], pre + "cut_loss")
    _close(m["orth_loss"].numpy(), golden[pre + "orth_loss"], pre + "orth_loss")


@pytest.mark.parametrize("cfg", dc.COARSEN_CONFIGS, ids=lambda c: c[0])
def test_mirror_reproduces_the_reference_coarsening_and_losses(cfg, golden):
    name, weighted = cfg
    g = dc.batch()
    w = g["w"] if weighted else None
    _hold(dm.diff_pool_coarsen_mirror(g["x"], g["ei"], w, g["gid"], g["assign"]), golden,
          "densepool::diff_pool_coarsen/{}/".format(name))
    _hold(dm.min_cut_pool_coarsen_mirror(g["x"], g["ei"], w, g["gid"], g["assign"]), golden,
          "densepool::min_cut_pool_coarsen/{}/".format(name))
    cut, orth = dm.min_cut_losses_mirror(g["ei"], w, g["gid"], g["assign"])
    pre = "densepool::min_cut_pool_compute_losses/{}/".format(name)
    _close(cut.numpy(), golden[pre + "cut_loss"], pre + "cut_loss")
    _close(orth.numpy(), golden[pre + "orth_loss"], pre + "orth_loss")


def test_absolute_mode_keeps_the_values_and_bounds_the_gradient():
    """The bar of the GPU gradient tests: absolute=True leaves every forward value alone, and its gradients dominate the
    true ones entry by entry."""
    import torch
    g = dc.batch()
    fg, ag = _gnns(g)

    def run(absolute):
        x = torch.from_numpy(g["x"]).double().requires_grad_(True)
        m = dm.min_cut_pool_mirror(x, g["ei"], g["w"], g["gid"], fg, ag, absolute=absolute)
        (m["x"].sum() + m["edge_weight"].sum() + m["cut_loss"] + m["orth_loss"]).backward()
        return m, x.grad
    (m, gx), (ma, gabs) = run(False), run(True)
    assert torch.equal(m["x"], ma["x"]) and torch.equal(m["cut_loss"], ma["cut_loss"]) and torch.equal(m["orth_loss"], ma["orth_loss"])
    assert (gabs >= gx.abs() * (1 - 1e-12)).all() and (gabs > 0).all()
