# coding=utf-8
"""include/tfgx_lstm.h (the LSTM GraphSAGE aggregator) without a GPU: the exact list of its names (the uniform header /
table / version checks are tests/test_abi_registry.py's), the host argument checks name the refused member before any device work,
zero sizes succeed, and the float64 torch mirror of the layer (tests/lstm_mirror.py, the exact reference of
tests/test_gpu_lstm_sage.py) reproduces every case the reference's own lstm_graph_sage wrote into
tests/golden/lstm_sage_cases.npz (tests/golden/make_lstm_sage_golden.py) to 1e-12; torch.nn.LSTM cross-checks the recurrence."""
import os
import re

import numpy as np
import pytest
import torch

from abi_header import declarations, source
from conftest import ROOT
import lstm_mirror as M

HEADER = "tfgx_lstm.h"
GOLDEN = os.path.join(ROOT, "tests", "golden", "lstm_sage_cases.npz")


def _lib():
    from tf_geometric_amd import _lib
    return _lib.load_library()


def golden_cases():
    blob = np.load(GOLDEN)
    out = {}
    for name in blob["__cases__"].tolist():
        c = {k.split("::", 1)[1]: blob[k] for k in blob.files if k.startswith(name + "::")}
        c["activation"] = str(c["activation"]) if "activation" in c else None
        c["bias"] = c.get("bias")
        c["concat"], c["normalize"] = bool(c["concat"]), bool(c["normalize"])
        out[name] = c
    return out


def mirror_of_case(c, dtype=torch.float64):
    t = lambda k: None if c[k] is None else torch.as_tensor(np.asarray(c[k], dtype=np.float64)).to(dtype)      # noqa: E731
    return M.lstm_sage_mirror(t("x"), c["edge_index"], t("kernel"), t("recurrent_kernel"), t("lstm_bias"), t("self_kernel"),
                              t("neighbor_kernel"), t("bias"), c["activation"], c["concat"], c["normalize"])


def test_lstm_symbols_and_versions():
    from tf_geometric_amd import _lib as L
    assert sorted(declarations(HEADER)) == sorted(L.LSTM_SIGNATURES) == [
        "tfgx_lstm_aggregate_backward_f32", "tfgx_lstm_aggregate_f32", "tfgx_lstm_aggregate_saved_bytes",
        "tfgx_lstm_aggregate_tiles", "tfgx_lstm_recurrent_kernel_resident", "tfgx_lstm_version"]


def test_lstm_size_queries():
    lib = _lib()
    assert lib.tfgx_lstm_aggregate_saved_bytes(10, 7, 32) == 10 * 7 * 20 * 32
    assert lib.tfgx_lstm_aggregate_saved_bytes(0, 7, 32) == 0 and lib.tfgx_lstm_aggregate_saved_bytes(10, 0, 32) == 0
    assert [lib.tfgx_lstm_aggregate_tiles(n) for n in (0, 1, 32, 33, 130)] == [0, 1, 1, 2, 5]
    res_f = [u for u in range(16, 257, 16) if lib.tfgx_lstm_recurrent_kernel_resident(u, 0)]
    res_b = [u for u in range(16, 257, 16) if lib.tfgx_lstm_recurrent_kernel_resident(u, 1)]
    assert res_f == list(range(16, 97, 16)) and res_b == list(range(16, 81, 16))      # the limits the GPU sweep straddles
    assert lib.tfgx_lstm_recurrent_kernel_resident(20, 0) == 0 and lib.tfgx_lstm_recurrent_kernel_resident(0, 0) == 0


FWD_OK = dict(row_ptr=8, col=8, n_dst=4, n_src=4, T=2, P=8, ldp=64, p_pad=8, R=8, U=16, out=8, ldo=16, saved=None, saved_bytes=0,
              flag=None, stream=None)
BWD_OK = dict(row_ptr=8, n_dst=4, T=2, U=16, R=8, d_mean=8, ldd=16, saved=8, saved_bytes=4 * 2 * 20 * 16, d_gates=8, h_prev=8,
              d_pad=8, stream=None)


def _call(fn, args):
    return fn(*args.values())


@pytest.mark.parametrize("change, word", [
    (dict(n_dst=-1), "negative"), (dict(T=-2), "negative"), (dict(U=20), "U must be a multiple of 16"),
    (dict(U=272, ldp=4 * 272, ldo=272), "U must be a multiple of 16"), (dict(n_src=-1), "n_src"), (dict(n_src=1 << 31), "n_src"),
    (dict(ldp=63), "ldp"), (dict(ldo=15), "ldo"), (dict(out=None), "out_mean is null"), (dict(row_ptr=None), "row_ptr is null"),
    (dict(col=None), "col is null"), (dict(p_pad=None), "p_pad is null"), (dict(R=None), "R is null"), (dict(P=None), "P is null"),
    (dict(saved=8, saved_bytes=4 * 2 * 20 * 16 - 1), "saved_bytes"),
])
def test_forward_argument_checks_name_the_member(change, word):
    """Every refusal happens on the host, before any device work (the pointers here are never dereferenced)."""
    lib = _lib()
    rc = _call(lib.tfgx_lstm_aggregate_f32, dict(FWD_OK, **change))
    assert rc == 1, rc          # TFGX_ERR_INVALID_ARG
    assert word in lib.tfgx_last_error().decode(), lib.tfgx_last_error()


@pytest.mark.parametrize("change, word", [
    (dict(n_dst=-1), "negative"), (dict(U=8), "U must be a multiple of 16"), (dict(ldd=15), "ldd"),
    (dict(n_dst=1 << 20, T=1 << 12, saved_bytes=1 << 62), "n_dst * T"),
    (dict(row_ptr=None), "row_ptr is null"), (dict(R=None), "R is null"), (dict(d_mean=None), "d_mean is null"),
    (dict(saved=None), "saved is null"), (dict(d_gates=None), "d_gates is null"), (dict(h_prev=None), "h_prev is null"),
    (dict(d_pad=None), "d_pad_partial is null"), (dict(saved_bytes=7), "saved_bytes"),
])
def test_backward_argument_checks_name_the_member(change, word):
    lib = _lib()
    rc = _call(lib.tfgx_lstm_aggregate_backward_f32, dict(BWD_OK, **change))
    assert rc == 1, rc
    assert word in lib.tfgx_last_error().decode(), lib.tfgx_last_error()


def test_invalid_arg_code_is_one():
    assert re.search(r"TFGX_ERR_INVALID_ARG\s*=?\s*1\b", source("tfgx.h"))


@pytest.mark.parametrize("change", [dict(n_dst=0), dict(U=0, ldp=0, ldo=0)])
def test_zero_sizes_succeed_without_device_work(change):
    lib = _lib()
    null = dict(row_ptr=None, col=None, P=None, p_pad=None, R=None, out=None)
    assert _call(lib.tfgx_lstm_aggregate_f32, dict(FWD_OK, **dict(null, **change))) == 0
    bnull = dict(row_ptr=None, R=None, d_mean=None, saved=None, saved_bytes=0, d_gates=None, h_prev=None, d_pad=None)
    bchange = {k: v for k, v in change.items() if k in BWD_OK}
    if "U" in change:
        bchange["ldd"] = 0
    assert _call(lib.tfgx_lstm_aggregate_backward_f32, dict(BWD_OK, **dict(bnull, **bchange))) == 0
    assert _call(lib.tfgx_lstm_aggregate_backward_f32, dict(BWD_OK, **dict(bnull, T=0))) == 0


# ---- the mirror -------------------------------------------------------------------------------------------------------------
def test_golden_file_is_small_and_covers_the_cases():
    assert os.path.getsize(GOLDEN) < 100 * 1024
    cs = golden_cases()
    assert {(c["concat"], c["normalize"]) for c in cs.values()} == {(True, False), (False, False), (True, True), (False, True)}
    for c in cs.values():
        ei = c["edge_index"]
        deg = np.bincount(ei[0], minlength=c["x"].shape[0])
        assert deg.min() == 0 and deg.max() >= 3                       # a node of degree 0, a node of degree T
        assert not np.all(np.diff(ei[0]) >= 0)                         # shuffled order
        pairs = list(zip(*ei.tolist()))
        assert len(set(pairs)) < len(pairs)                            # repeated neighbours


@pytest.mark.parametrize("name", ["concat", "add", "concat_normalize", "add_normalize"])
def test_mirror_reproduces_the_reference(name):
    c = golden_cases()[name]
    got = mirror_of_case(c).numpy()
    assert got.shape == c["output"].shape
    assert np.abs(got - c["output"]).max() <= 1e-12, np.abs(got - c["output"]).max()


def test_mirror_recurrence_matches_torch_lstm():
    """torch.nn.LSTM has the same gate order (i, f, g, o): the mean of its outputs over a padded sequence is aggregate_mirror."""
    g = torch.Generator().manual_seed(5)
    n, T, F, U = 6, 4, 3, 5
    x = torch.randn(n, F, generator=g, dtype=torch.float64)
    kernel, R = torch.randn(F, 4 * U, generator=g, dtype=torch.float64), torch.randn(U, 4 * U, generator=g, dtype=torch.float64) * 0.5
    b = torch.randn(4 * U, generator=g, dtype=torch.float64)
    nbr = torch.randint(-1, n, (n, T), generator=g)
    nbr[0] = -1
    lstm = torch.nn.LSTM(F, U, batch_first=True).double()
    with torch.no_grad():
        lstm.weight_ih_l0.copy_(kernel.t())
        lstm.weight_hh_l0.copy_(R.t())
        lstm.bias_ih_l0.copy_(b)
        lstm.bias_hh_l0.zero_()
        seq = torch.cat([x, torch.zeros(1, F, dtype=torch.float64)])[torch.where(nbr >= 0, nbr, torch.full_like(nbr, n))]
        ref = lstm(seq)[0].mean(1)
    got = M.aggregate_mirror(x @ kernel + b, b, R, nbr)
    assert (got - ref).abs().max() <= 1e-12


def test_unit_padding_is_exact_in_the_mirror():
    """Zero-padding the units to a multiple of 16 (what the Python side does) adds exact zeros to every sum: the padded units
    stay at exactly 0 and the others move by no more than the BLAS's summation order over the longer rows (a few float64 ulp)."""
    from tf_geometric_amd.nn.conv.graph_sage import _pad_gate_blocks
    c = golden_cases()["add"]
    U, Up = 6, 16
    k, r, b = (torch.as_tensor(c[n]) for n in ("kernel", "recurrent_kernel", "lstm_bias"))
    x = torch.as_tensor(c["x"])
    nbr = M.neighbor_matrix(c["edge_index"], x.shape[0])
    base = M.aggregate_mirror(x @ k + b, b, r, nbr)
    kp, bp = _pad_gate_blocks(k, U, Up), _pad_gate_blocks(b, U, Up)
    rp = torch.nn.functional.pad(_pad_gate_blocks(r, U, Up), (0, 0, 0, Up - U))
    padded = M.aggregate_mirror(x @ kp + bp, bp, rp, nbr)
    assert float((padded[:, :U] - base).abs().max()) <= 1e-15 and float(padded[:, U:].abs().max()) == 0.0


def test_public_names_and_layer_constructor():
    import tf_geometric_amd as tfg
    assert callable(tfg.nn.lstm_graph_sage) and tfg.layers.LSTM and tfg.layers.LSTMGraphSage
    with pytest.raises(Exception, match="event number"):
        tfg.layers.LSTMGraphSage(7)
    tfg.layers.LSTMGraphSage(7, concat=False)
