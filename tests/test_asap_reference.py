# coding=utf-8
"""tests/golden/asap_cases.npz is what the reference's own asap() (with the two stated adapters) and cluster_pool() produce
on the inputs of tests/asap_cases.py (no GPU needed); the live comparison runs where the reference checkout exists.  The
float64 mirror (tests/asap_mirror.py), which the GPU fuzz and gradient tests take as their reference, is held to the same
file here."""
import os
import sys

import numpy as np
import pytest

from conftest import ROOT, assert_parity
import asap_cases as ac
import asap_mirror as am

sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import make_asap_golden as mk     # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden", "asap_cases.npz")


@pytest.fixture(scope="module")
def golden():
    return dict(np.load(GOLDEN))


def test_golden_file_is_small_and_names_its_backend(golden):
    assert os.path.getsize(GOLDEN) < 100 * 1024
    assert str(golden["__backend__"]) in ("tensorflow", "numpy-stub")


@pytest.mark.parametrize("case", ac.CASES, ids=lambda c: c.name)
def test_golden_inputs_are_the_case_table(case, golden):
    assert str(golden["{}::__inputs_sha256__".format(case.name)]) == mk.inputs_digest(case.inputs())
    for cfg in case.configs:
        assert "{}::{}/edge_index".format(case.name, cfg[0]) in golden, cfg[0]      # no configuration was left out


def test_scores_are_separated():
    """The generator's condition: no selection in the file hangs on the last float32 bit."""
    assert mk.min_score_gap(ac.asap_inputs()) >= ac.MIN_SCORE_GAP


def test_golden_covers_the_corner_cases(golden):
    g = ac.asap_inputs()
    assert (g["ei"][0] == g["ei"][1]).any()                                          # self-loops to remove
    assert np.unique(g["ei"], axis=1).shape[1] < g["ei"].shape[1]                    # duplicates
    assert (g["gid"][g["ei"][0]] != g["gid"][g["ei"][1]]).any()                      # edges across graphs
    assert (np.diff(g["gid"]) < 0).any() and np.setdiff1d(np.arange(g["gid"].max()), g["gid"]).size     # unsorted, gapped
    assert (g["w"] > 0).all()
    assert min(np.bincount(g["gid"])[np.unique(g["gid"])]) < 3                       # k = 3 is larger than a graph
    ei = golden["asap::ratio-sigmoid-w/edge_index"]
    K = golden["asap::ratio-sigmoid-w/x"].shape[0]
    assert ei.dtype == np.int32 and golden["asap::ratio-sigmoid-now/edge_weight"].dtype == np.float32
    assert np.array_equal(ei[:, -K:], np.stack([np.arange(K), np.arange(K)]))        # the appended diagonal
    assert (ei[0, :-K] != ei[1, :-K]).all()
    c = ac.cluster_inputs()
    assert (c["assign_zero_w"] == 0.0).sum() == 1
    full, zero = golden["cluster_pool::x-w/edge_index"], golden["cluster_pool::x-zero/edge_index"]
    assert (full == 5).any() and not (zero == 5).any()                               # the zero weight dropped entries
    assert "cluster_pool::nox-w/x" not in golden and (full[0] == full[1]).any()       # x = None; the diagonal stays


@pytest.mark.parametrize("case", ac.CASES, ids=lambda c: c.name)
def test_golden_file_is_what_the_reference_produces(case, golden):
    from oracle.ref_harness import reference_available
    if not reference_available():
        pytest.skip("reference checkout not present")
    import types
    from oracle.ref_harness import load_reference
    tfg, tf, tfs, _ = load_reference()
    outs = case.ref(types.SimpleNamespace(tfg=tfg, tf=tf, tfs=tfs), case.inputs())
    keys = [k for k in golden if k.startswith(case.name + "::") and not k.endswith("__")]
    assert sorted(keys) == sorted(case.name + "::" + k for k in outs)
    for k, v in outs.items():
        ref = golden[case.name + "::" + k]
        v = np.asarray(v)
        assert v.dtype == ref.dtype and v.shape == ref.shape, k
        assert np.array_equal(v, ref), "{}: live reference run differs from the committed golden file".format(k)


@pytest.mark.parametrize("cfg", ac.ASAP_CONFIGS, ids=lambda c: c[0])
def test_mirror_reproduces_the_reference_asap(cfg, golden):
    name, kr, act, weighted, _ = cfg
    g = ac.asap_inputs()
    w = dict(zip(am.WEIGHT_NAMES, ac.config_weights(g, name)))
    m = am.asap_mirror(g["x"], g["ei"], g["w"] if weighted else None, g["gid"], w, activation=act, **kr)
    pre = "asap::{}/".format(name)
    assert np.array_equal(m["node_graph_index"], golden[pre + "node_graph_index"])
    assert np.array_equal(m["edge_index"], golden[pre + "edge_index"])
    assert_parity(m["x"].detach().numpy(), golden[pre + "x"], what=name + " x")
    assert_parity(m["edge_weight"].numpy(), golden[pre + "edge_weight"], what=name + " edge_weight")


@pytest.mark.parametrize("cfg", ac.CLUSTER_CONFIGS, ids=lambda c: c[0])
def test_mirror_reproduces_the_reference_cluster_pool(cfg, golden):
    a, kw = ac._cluster_args(ac.cluster_inputs(), cfg)
    m = am.cluster_pool_mirror(*a, **kw)
    pre = "cluster_pool::{}/".format(cfg[0])
    assert np.array_equal(m["edge_index"], golden[pre + "edge_index"])
    assert_parity(m["edge_weight"].numpy(), golden[pre + "edge_weight"], what=cfg[0] + " edge_weight")
    if m["x"] is None:
        assert pre + "x" not in golden
    else:
        assert_parity(m["x"].numpy(), golden[pre + "x"], what=cfg[0] + " x")


def test_cluster_pool_without_x_needs_num_nodes():
    with pytest.raises(Exception, match="Please provide num_nodes if x is None"):
        am.cluster_pool_mirror(None, np.zeros((2, 0), np.int32), None, np.zeros((2, 0), np.int32), None, 3)
