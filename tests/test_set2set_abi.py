# coding=utf-8
"""include/tfgx_set2set.h (Set2Set: the attention readout and the sequence LSTM) without a GPU: the exact list of its names and
its own macros (the uniform header / table / version checks are tests/test_abi_registry.py's), the host argument checks
name the refused member before any device work, zero sizes succeed, the size queries return what the header documents, and
the float64 torch mirror (tests/set2set_mirror.py, the exact reference of tests/test_gpu_set2set.py) reproduces every case
the reference's own set2set wrote into tests/golden/set2set_cases.npz (tests/golden/make_set2set_golden.py) to 1e-12;
torch.nn.LSTM cross-checks the mirror's recurrence with a non-zero initial state."""
import os

import numpy as np
import pytest
import torch

from abi_header import declarations, macro, refused as _refused
import set2set_mirror as M
from set2set_mirror import GOLDEN, golden_cases, mirror_of_case
from tf_geometric_amd._lib import SET2SET_CHUNK_ROWS as CHUNK

HEADER = "tfgx_set2set.h"


def _lib():
    from tf_geometric_amd import _lib
    return _lib.load_library()


def test_set2set_symbols_and_versions():
    from tf_geometric_amd import _lib as L
    assert sorted(declarations(HEADER)) == sorted(L.SET2SET_SIGNATURES) == [
        "tfgx_lstm_sequence_backward_f32", "tfgx_lstm_sequence_f32", "tfgx_lstm_sequence_kernel_resident",
        "tfgx_lstm_sequence_saved_bytes", "tfgx_set2set_attend_backward_f32", "tfgx_set2set_attend_f32",
        "tfgx_set2set_attend_workspace_bytes", "tfgx_set2set_version"]
    assert macro(HEADER, "TFGX_SET2SET_CHUNK_ROWS") == L.SET2SET_CHUNK_ROWS
    assert macro(HEADER, "TFGX_SET2SET_MAX_FEATURES") == L.SET2SET_MAX_FEATURES


def test_size_queries():
    lib = _lib()
    ws = lib.tfgx_set2set_attend_workspace_bytes
    assert ws(CHUNK, 10, 64) == 0 and ws(0, 10, 64) == 0 and ws(4 * CHUNK, 0, 64) == 0 and ws(4 * CHUNK, 3, 0) == 0
    assert ws(CHUNK + 1, 10, 64) == 4 * (2 * 10 + 2 * (64 + 2))
    assert ws(4 * CHUNK - 7, 3, 5) == 4 * (2 * 3 + 4 * (5 + 2))
    sb = lib.tfgx_lstm_sequence_saved_bytes
    assert sb(2, 3, 16) == 4 * 2 * 16 * (5 * 3 + 1) and sb(1, 130, 256) == 4 * 256 * (5 * 130 + 1)
    assert sb(0, 3, 16) == 0 and sb(2, 0, 16) == 0 and sb(2, 3, 0) == 0
    res = [u for u in range(16, 257, 16) if lib.tfgx_lstm_sequence_kernel_resident(u)]
    assert res == list(range(16, 97, 16))                        # the limit the GPU sweep straddles
    assert lib.tfgx_lstm_sequence_kernel_resident(20) == 0 and lib.tfgx_lstm_sequence_kernel_resident(0) == 0


ATT_OK = dict(row_ptr=8, node=8, G=3, N=4, x=8, ldx=16, F=16, q=8, ldq=16, r=8, ldr=16, stats=None, ws=None, ws_bytes=0,
              flag=None, stream=None)
ATT_BWD_OK = dict(row_ptr=8, node=8, G=3, N=4, x=8, ldx=16, F=16, q=8, ldq=16, r=8, ldr=16, stats=8, d_r=8, ldg=16, d_x=8,
                  lddx=16, d_q=8, lddq=16, ws=None, ws_bytes=0, stream=None)
SEQ_OK = dict(P=8, ldp=64, B=2, T=3, R=8, U=16, h0=None, c0=None, h_seq=8, h_last=8, c_last=8, saved=None, saved_bytes=0,
              stream=None)
SEQ_BWD_OK = dict(B=2, T=3, U=16, R=8, h0=None, d_h_seq=None, d_h_last=None, d_c_last=None, saved=8,
                  saved_bytes=4 * 2 * 16 * 16, d_gates=8, h_prev=8, d_h0=8, d_c0=8, stream=None)
BIG_WS = 4 * (2 * 3 + 4 * (16 + 2))       # N = 4 * CHUNK, G = 3, F = 16


def _call(fn, args):
    return fn(*args.values())


ATT_COMMON = [
    (dict(G=-1), "negative"), (dict(N=-1), "negative"), (dict(F=-1), "negative"), (dict(G=1 << 31), "fit int32"),
    (dict(N=1 << 32), "fit int32"), (dict(F=1025, ldx=1025, ldq=1025, ldr=1025), "TFGX_SET2SET_MAX_FEATURES"),
    (dict(ldx=15), "ldx"), (dict(ldq=15), "ldq"), (dict(ldr=15), "ldr"),
    (dict(row_ptr=None), "row_ptr is null"), (dict(node=None), "node is null"), (dict(x=None), "x is null"),
    (dict(q=None), "q is null"), (dict(r=None), "r is null"),
    (dict(N=4 * CHUNK), "workspace is null"), (dict(N=4 * CHUNK, ws=8, ws_bytes=BIG_WS - 1), "workspace_bytes"),
]


@pytest.mark.parametrize("change, word", ATT_COMMON)
def test_attend_argument_checks_name_the_member(change, word):
    _refused("tfgx_set2set_attend_f32", ATT_OK, change, word)


@pytest.mark.parametrize("change, word", ATT_COMMON + [
    (dict(ldg=15), "ldg"), (dict(lddx=15), "lddx"), (dict(lddq=15), "lddq"), (dict(stats=None), "stats is null"),
    (dict(d_r=None), "d_r is null"), (dict(d_q=None), "d_q is null"),
])
def test_attend_backward_argument_checks_name_the_member(change, word):
    if "F" in change and change["F"] > 16:
        change = dict(change, ldg=1025, lddx=1025, lddq=1025)
    _refused("tfgx_set2set_attend_backward_f32", ATT_BWD_OK, change, word)


@pytest.mark.parametrize("change, word", [
    (dict(B=-1), "negative"), (dict(T=-2), "negative"), (dict(U=-16), "negative"), (dict(U=20, ldp=80), "U must be a multiple of 16"),
    (dict(U=272, ldp=4 * 272), "U must be a multiple of 16"), (dict(B=1 << 20, T=1 << 12), "B * T"), (dict(ldp=63), "ldp"),
    (dict(P=None), "P is null"), (dict(R=None), "R is null"), (dict(saved=8, saved_bytes=4 * 2 * 16 * 16 - 1), "saved_bytes"),
])
def test_sequence_argument_checks_name_the_member(change, word):
    _refused("tfgx_lstm_sequence_f32", SEQ_OK, change, word)


@pytest.mark.parametrize("change, word", [
    (dict(B=-1), "negative"), (dict(T=-2), "negative"), (dict(U=8), "U must be a multiple of 16"),
    (dict(B=1 << 20, T=1 << 12, saved_bytes=1 << 62), "B * T"),
    (dict(R=None), "R is null"), (dict(saved=None), "saved is null"), (dict(d_gates=None), "d_gates is null"),
    (dict(h_prev=None), "h_prev is null"), (dict(d_h0=None), "d_h0 is null"), (dict(d_c0=None), "d_c0 is null"),
    (dict(saved_bytes=7), "saved_bytes"),
])
def test_sequence_backward_argument_checks_name_the_member(change, word):
    _refused("tfgx_lstm_sequence_backward_f32", SEQ_BWD_OK, change, word)


def test_zero_sizes_succeed_without_device_work():
    lib = _lib()
    null = dict(row_ptr=None, node=None, x=None, q=None, r=None)
    for change in (dict(G=0), dict(F=0, ldx=0, ldq=0, ldr=0)):
        assert _call(lib.tfgx_set2set_attend_f32, dict(ATT_OK, **dict(null, **change))) == 0
        bchange = dict(change, ldg=0, lddx=0, lddq=0) if "F" in change else change
        assert _call(lib.tfgx_set2set_attend_backward_f32,
                     dict(ATT_BWD_OK, **dict(null, stats=None, d_r=None, d_x=None, d_q=None, **bchange))) == 0
    snull = dict(P=None, R=None, h_seq=None, h_last=None, c_last=None)
    bnull = dict(R=None, saved=None, saved_bytes=0, d_gates=None, h_prev=None, d_h0=None, d_c0=None)
    for change in (dict(B=0), dict(T=0), dict(U=0, ldp=0)):
        assert _call(lib.tfgx_lstm_sequence_f32, dict(SEQ_OK, **dict(snull, **change))) == 0
        assert _call(lib.tfgx_lstm_sequence_backward_f32,
                     dict(SEQ_BWD_OK, **dict(bnull, **{k: v for k, v in change.items() if k != "ldp"}))) == 0


# ---- the mirror -------------------------------------------------------------------------------------------------------------
def test_golden_file_is_small_and_covers_the_cases():
    assert os.path.getsize(GOLDEN) < 100 * 1024
    cs = golden_cases()
    ids = [c["node_graph_index"] for c in cs.values()]
    assert any(not np.all(np.diff(i) >= 0) for i in ids)                                    # shuffled ids
    counts = [np.bincount(i, minlength=int(i.max()) + 1) for i in ids]
    assert any(c.size > 2 and (c[1:-1] == 0).any() for c in counts)                          # an empty graph in the middle
    assert any((c == 1).any() for c in counts)                                               # a one-node graph
    assert any(c.size == 1 for c in counts)                                                  # G = 1
    assert {1} < {c["num_iterations"] for c in cs.values()} and max(c["num_iterations"] for c in cs.values()) >= 3
    assert {c["x"].shape[1] for c in cs.values()} == {1, 5}


@pytest.mark.parametrize("name", ["shuffled_f5_it3", "sorted_f1_it1", "shuffled_f1_it4", "one_graph_f5_it3", "sorted_f5_it1"])
def test_mirror_reproduces_the_reference(name):
    c = golden_cases()[name]
    got = mirror_of_case(c).numpy()
    assert got.shape == c["output"].shape
    assert np.abs(got - c["output"]).max() <= 1e-12, np.abs(got - c["output"]).max()


def test_reference_couples_the_graphs_of_a_batch():
    """The reference's literal call runs the LSTM over the graphs: two EMPTY graphs of one batch get different rows (their
    attention term is zero, their query is not), and a graph's row changes with what precedes it."""
    g = torch.Generator().manual_seed(2)
    F = 3
    x = torch.randn(5, F, generator=g, dtype=torch.float64)
    k, r, b = (torch.randn(*s, generator=g, dtype=torch.float64) for s in ((2 * F, 4 * F), (F, 4 * F), (4 * F,)))
    ids = torch.tensor([0, 0, 3, 3, 3])
    out = M.set2set_mirror(x, ids, k, r, b, 2)
    assert float((out[1] - out[2]).abs().max()) > 1e-3 and float(out[1, F:].abs().max()) == 0.0
    per_graph = M.set2set_mirror(x, ids, k, r, b, 2, batch_graphs=True)
    assert torch.equal(per_graph[1], per_graph[2])


def test_mirror_lstm_matches_torch_lstm_with_an_initial_state():
    g = torch.Generator().manual_seed(5)
    B, T, F, U = 3, 4, 6, 5
    r = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)      # noqa: E731
    seq, kernel, R, b, h0, c0 = r(B, T, F), r(F, 4 * U), r(U, 4 * U) * 0.5, r(4 * U), r(B, U), r(B, U)
    lstm = torch.nn.LSTM(F, U, batch_first=True).double()
    with torch.no_grad():
        lstm.weight_ih_l0.copy_(kernel.t())
        lstm.weight_hh_l0.copy_(R.t())
        lstm.bias_ih_l0.copy_(b)
        lstm.bias_hh_l0.zero_()
        ref_seq, (ref_h, ref_c) = lstm(seq, (h0.unsqueeze(0), c0.unsqueeze(0)))
    out, h, c = M.lstm_mirror(seq, kernel, R, b, h0, c0)
    assert float((out - ref_seq).abs().max()) <= 1e-12
    assert float((h - ref_h[0]).abs().max()) <= 1e-12 and float((c - ref_c[0]).abs().max()) <= 1e-12


def test_the_two_modes_agree_for_one_graph_and_differ_for_more():
    cs = golden_cases()
    one = cs["one_graph_f5_it3"]
    assert float((mirror_of_case(one) - mirror_of_case(one, batch_graphs=True)).abs().max()) <= 1e-15
    many = cs["shuffled_f5_it3"]
    assert float((mirror_of_case(many) - mirror_of_case(many, batch_graphs=True)).abs().max()) > 1e-3


def test_attention_weights_sum_to_one_minus_epsilon():
    g = torch.Generator().manual_seed(7)
    x, q = torch.randn(9, 4, generator=g, dtype=torch.float64), torch.randn(3, 4, generator=g, dtype=torch.float64)
    ids = torch.tensor([2, 0, 0, 2, 2, 0, 2, 2, 2])
    r, a = M.attend_mirror(x, ids, q, 3)
    sums = torch.zeros(3, dtype=torch.float64).index_add(0, ids, a)
    assert float(sums[1]) == 0.0 and float(r[1].abs().max()) == 0.0            # the empty graph
    assert float((sums[[0, 2]] - 1.0).abs().max()) < 1e-7


def test_public_names_and_constructors():
    import tf_geometric_amd as tfg
    assert callable(tfg.nn.set2set) and tfg.nn.pool.set2set is tfg.nn.set2set
    assert tfg.layers.Set2Set is tfg.layers.pool.Set2Set
    layer = tfg.layers.Set2Set()
    assert layer.num_iterations == 4 and layer.batch_graphs is False and layer.lstm is None
    assert tfg.layers.Set2Set(num_iterations=2, batch_graphs=True).batch_graphs is True
    lstm = tfg.layers.LSTM(7)
    assert lstm.return_sequences is False and lstm.return_state is False          # Keras's defaults
    lstm = tfg.layers.LSTM(7, return_sequences=True, return_state=True)
    assert lstm.return_sequences and lstm.return_state and lstm.units == 7
