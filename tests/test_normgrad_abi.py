# coding=utf-8
"""include/tfgx_normgrad.h (the backward of the GCN normalisation) without a GPU: the exact list of its names and its pass
macros (the uniform header / table / version checks are tests/test_abi_registry.py's), and the entry refuses null pointers, a bad
mode, negative sizes and an unweighted list on the host, before any device work."""
import pytest

from abi_header import declarations, macro, refused

HEADER = "tfgx_normgrad.h"
ENTRY = "tfgx_gcn_norm_backward_f32"


def _lib():
    from tf_geometric_amd import _lib
    return _lib.load_library()


def test_symbols_versions_and_signatures():
    from tf_geometric_amd import _lib as L
    assert sorted(declarations(HEADER)) == sorted(L.NORMGRAD_SIGNATURES) == [ENTRY, "tfgx_normgrad_version"]
    assert (L.NORMGRAD_ROW_PASS, L.NORMGRAD_COL_PASS, L.NORMGRAD_EDGE_PASS, L.NORMGRAD_ALL) == tuple(
        macro(HEADER, "TFGX_NORMGRAD_" + n) for n in ("ROW_PASS", "COL_PASS", "EDGE_PASS", "ALL")) == (1, 2, 4, 7)


# non-null pointers are never dereferenced: every refusal happens on the host
OK = dict(row_ptr=8, col=8, w=8, n_rows=5, n_cols=5, t_row_ptr=8, t2d=8, row_deg=8, col_deg=None, mode=0, fill=1.0,
          add_self_loop=1, renorm=1, G=8, S=8, A=8, B=8, t=8, dw=8, passes=7, stream=None)


@pytest.mark.parametrize("change, word", [
    (dict(n_rows=-1), "negative"), (dict(n_cols=-1), "negative"),
    (dict(mode=3), "bad norm mode"), (dict(mode=-1), "bad norm mode"),
    (dict(w=None), "w is null"), (dict(passes=0), "passes"), (dict(passes=8), "passes"), (dict(passes=-1), "passes"),
    (dict(row_ptr=None), "null pointer"), (dict(col=None), "null pointer"), (dict(row_deg=None), "null pointer"),
    (dict(G=None), "null pointer"), (dict(dw=None), "null pointer"), (dict(A=None), "null pointer (A)"),
    (dict(t_row_ptr=None), "t_row_ptr"), (dict(t2d=None), "t_row_ptr"), (dict(B=None), "t_row_ptr"), (dict(t=None), "t_row_ptr"),
    (dict(mode=1, A=None), "null pointer (A)"), (dict(mode=2, t=None), "t_row_ptr"),
    (dict(n_cols=7), "add_self_loop"), (dict(n_cols=7, add_self_loop=0), "symmetric"),
    (dict(mode=2, n_cols=7, add_self_loop=0), "n_cols <= n_rows"),
])
def test_argument_checks_happen_on_the_host(change, word):
    refused(ENTRY, OK, change, word)


def test_zero_rows_succeed_without_device_work_but_not_without_weights():
    lib = _lib()
    null = dict(row_ptr=None, col=None, t_row_ptr=None, t2d=None, row_deg=None, G=None, S=None, A=None, B=None, t=None, dw=None)
    assert getattr(lib, ENTRY)(*dict(OK, **dict(null, n_rows=0, n_cols=0)).values()) == 0
    refused(ENTRY, OK, dict(null, n_rows=0, n_cols=0, w=None), "w is null")


def test_gcn_norm_adj_fails_loudly_without_a_gpu():
    import numpy as np
    import torch
    import tf_geometric_amd as tfg
    from tf_geometric_amd import autograd
    from tf_geometric_amd._lib import TfgxError
    assert callable(autograd.gcn_norm) and callable(autograd.gcn_norm_backward)
    if torch.cuda.is_available():
        return
    w = torch.ones(2, requires_grad=True)
    with pytest.raises(TfgxError):
        tfg.nn.gcn_norm_edge(np.array([[0, 1], [1, 0]], np.int32), 2, w)
