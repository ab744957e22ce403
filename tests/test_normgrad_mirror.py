# coding=utf-8
"""tests/normgrad_mirror.py on the CPU: the closed form of the GCN normalisation's backward (the formulas of
include/tfgx_normgrad.h) against float64 autograd on the restatement with the masked power, for all 24 legal
configurations, on the n = 37 graph and on its variant with a zero-degree and a negative-degree node.  Both sides are
float64 and differ only in the order of a few hundred additions: 1e-12."""
import numpy as np
import pytest
import torch

import normgrad_mirror as nm
from asap_mirror import _Ops

CONFIGS = nm.configs()


def test_there_are_24_legal_configurations():
    assert len(CONFIGS) == len(set(CONFIGS)) == 24


def _cotangents(g, cfg, n_rows):
    """(G, S) of the loss sum c w_out + sum s self_coef: S is absent without a self-loop."""
    return g["c"], (g["s"] if cfg[2] else None)


@pytest.mark.parametrize("negate_row", [None, 2], ids=["positive", "zero-and-negative-degree"])
@pytest.mark.parametrize("cfg", CONFIGS, ids=nm.config_id)
def test_closed_form_equals_autograd(cfg, negate_row):
    g = nm.sweep_graph(negate_row=negate_row)
    n = g["n"]
    ref = nm.reference_gradient(g["row"], g["col"], g["w"], n, n, cfg, g["c"], g["s"])
    G, S = _cotangents(g, cfg, n)
    got = nm.closed_form(g["row"], g["col"], g["w"], n, n, cfg, G, S)
    assert np.isfinite(ref).all() and np.isfinite(got).all()
    err = np.abs(got - ref).max()
    print("{}: max |ref| {:.3e}, max err {:.3e}".format(nm.config_id(cfg), np.abs(ref).max(), err))
    assert err <= 1e-12 * (1.0 + np.abs(ref).max())
    assert np.abs(ref).max() > 1e-3


@pytest.mark.parametrize("shape, cfg", [((7, 11), ("both", False, False, True, False)), ((7, 11), ("left", False, False, True, False)),
                                        ((11, 7), ("right", False, False, True, False))], ids=["both", "left", "right"])
def test_closed_form_on_rectangular_operators(shape, cfg):
    g = nm.rect_graph(*shape)
    ref = nm.reference_gradient(g["row"], g["col"], g["w"], shape[0], shape[1], cfg, g["c"], g["s"])
    got = nm.closed_form(g["row"], g["col"], g["w"], shape[0], shape[1], cfg, g["c"], None)
    assert np.abs(got - ref).max() <= 1e-12 * (1.0 + np.abs(ref).max())


def test_the_masked_power_has_the_forward_value_and_a_zero_derivative_where_it_was_zeroed():
    d = torch.tensor([4.0, 0.0, -2.0, float("inf")], dtype=torch.float64, requires_grad=True)
    p = nm.masked_pow(_Ops(False), d, -0.5)
    assert p.tolist() == [0.5, 0.0, 0.0, 0.0]
    p.sum().backward()
    assert d.grad.tolist() == [-0.5 * 4.0 ** -1.5, 0.0, 0.0, 0.0]
    d2 = torch.tensor([4.0, 0.0, -2.0], dtype=torch.float64, requires_grad=True)
    q = nm.masked_pow(_Ops(False), d2, -1.0)
    assert q.tolist() == [0.25, 0.0, -0.5]              # 1 / d is finite for a negative degree: the forward keeps it
    q.sum().backward()
    assert d2.grad.tolist() == [-1.0 / 16.0, 0.0, -0.25]


def test_absolute_mode_keeps_values_and_bounds_the_gradient():
    g = nm.sweep_graph(negate_row=2)
    cfg = ("both", False, True, True, True)
    ref = nm.reference_gradient(g["row"], g["col"], g["w"], 37, 37, cfg, g["c"], g["s"])
    terms = nm.reference_gradient(g["row"], g["col"], g["w"], 37, 37, cfg, g["c"], g["s"], absolute=True)
    assert (terms >= np.abs(ref) * (1.0 - 1e-12)).all()
