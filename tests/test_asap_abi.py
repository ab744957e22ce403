# coding=utf-8
"""include/tfgx_asap.h (ASAP pooling: the fused attention and the sparse S^T A S) without a GPU: the exact list of its names and
its own macro (the uniform header / table / version checks are tests/test_abi_registry.py's), the host argument checks name the
refused member before any device work — the oversized expansion among them — and zero sizes succeed."""
import ctypes

import pytest

from abi_header import declarations, macro, refused as _refused

HEADER = "tfgx_asap.h"


def _lib():
    from tf_geometric_amd import _lib
    return _lib.load_library()


def test_symbols_versions_and_signatures():
    from tf_geometric_amd import _lib as L
    assert sorted(declarations(HEADER)) == sorted(L.ASAP_SIGNATURES) == [
        "tfgx_asap_attend_backward_f32", "tfgx_asap_attend_f32", "tfgx_asap_version", "tfgx_spasp_count",
        "tfgx_spasp_count_workspace_bytes", "tfgx_spasp_emit", "tfgx_spasp_reduce", "tfgx_spasp_workspace_bytes"]
    assert L.ASAP_MAX_FEATURES == macro(HEADER, "TFGX_ASAP_MAX_FEATURES") > 0
    # the host int64_t* of tfgx_spasp_count is an output to the host: bound with its type
    assert L.ASAP_SIGNATURES["tfgx_spasp_count"][1][9] is ctypes.POINTER(ctypes.c_int64)


ATT_OK = dict(row_ptr=8, col=8, N=4, E=6, x=8, ldx=16, F=16, sq=8, sh=8, bias=8, drop_rate=0.0, seed=0, c=8, ldc=16, p=8,
              p_self=8, p_drop=None, p_self_drop=None, flag=None, stream=None)
BWD_OK = dict(row_ptr=8, col=8, N=4, E=6, sq=8, sh=8, bias=8, p=8, p_self=8, p_drop=None, p_self_drop=None, dp=8, dp_self=8,
              ds=8, ds_self=8, dsq=8, stream=None)
EMIT_OK = dict(s_row_ptr=8, s_col=8, s_val=None, N=4, K=2, a_row=8, a_col=8, a_val=None, E=6, s_deg=8, offsets=8, total=10,
               ws=8, ws_bytes=1 << 30, stream=None)
REDUCE_OK = dict(total=10, K=2, drop_diagonal=0, out_row=8, out_col=8, out_val=8, out_row_ptr=8, out_count=8, ws=8,
                 ws_bytes=1 << 30, stream=None)


@pytest.mark.parametrize("change, word", [
    (dict(N=-1), "negative"), (dict(E=-1), "negative"), (dict(F=-1), "negative"), (dict(N=1 << 31), "fit int32"),
    (dict(F=257, ldx=257, ldc=257), "TFGX_ASAP_MAX_FEATURES"), (dict(ldx=15), "ldx"), (dict(ldc=15), "ldc"),
    (dict(drop_rate=1.0), "drop_rate"), (dict(drop_rate=-0.1), "drop_rate"),
    (dict(row_ptr=None), "row_ptr is null"), (dict(col=None), "col is null"), (dict(x=None), "x is null"),
    (dict(sq=None), "sq is null"), (dict(sh=None), "sh is null"), (dict(bias=None), "bias is null"), (dict(c=None), "c is null"),
    (dict(p=None), "p is null"), (dict(p_self=None), "p_self is null"), (dict(drop_rate=0.5), "p_drop is null"),
    (dict(drop_rate=0.5, p_drop=8), "p_self_drop is null"),
])
def test_attend_argument_checks_name_the_member(change, word):
    _refused("tfgx_asap_attend_f32", ATT_OK, change, word)


@pytest.mark.parametrize("change, word", [
    (dict(N=-1), "negative"), (dict(N=1 << 31), "fit int32"), (dict(row_ptr=None), "row_ptr is null"),
    (dict(p=None), "p is null"), (dict(p_drop=8), "both p_drop and p_self_drop"), (dict(dp=None), "dp is null"),
    (dict(dp_self=None), "dp_self is null"), (dict(ds=None), "ds is null"), (dict(ds_self=None), "ds_self is null"),
    (dict(dsq=None), "dsq is null"),
])
def test_attend_backward_argument_checks_name_the_member(change, word):
    _refused("tfgx_asap_attend_backward_f32", BWD_OK, change, word)


def test_an_oversized_expansion_is_refused_on_the_host():
    """2^31 products do not fit the int32 positions of the sort: refused by emit, by reduce and by the size query, with no
    launch (there is no device here to launch on)."""
    lib = _lib()
    big = 1 << 31
    _refused("tfgx_spasp_emit", EMIT_OK, dict(total=big), "2^31 - 1")
    _refused("tfgx_spasp_reduce", REDUCE_OK, dict(total=big), "2^31 - 1")
    assert lib.tfgx_spasp_workspace_bytes(big, 2) == 0
    assert lib.tfgx_spasp_workspace_bytes(big - 1, 2) > 8 * (big - 1)          # the largest size that is served


@pytest.mark.parametrize("fn, ok, change, word", [
    ("tfgx_spasp_emit", EMIT_OK, dict(total=-1), "negative"), ("tfgx_spasp_emit", EMIT_OK, dict(s_col=None), "s_col is null"),
    ("tfgx_spasp_emit", EMIT_OK, dict(offsets=None), "offsets is null"), ("tfgx_spasp_emit", EMIT_OK, dict(ws=None), "workspace is null"),
    ("tfgx_spasp_emit", EMIT_OK, dict(K=0), "empty S"),
    ("tfgx_spasp_reduce", REDUCE_OK, dict(K=-1), "negative"), ("tfgx_spasp_reduce", REDUCE_OK, dict(out_count=None), "out_count is null"),
    ("tfgx_spasp_reduce", REDUCE_OK, dict(out_val=None), "out_val is null"),
    ("tfgx_spasp_reduce", REDUCE_OK, dict(ws=None), "workspace is null"),
])
def test_spasp_argument_checks_name_the_member(fn, ok, change, word):
    _refused(fn, ok, change, word)


def test_spasp_workspace_too_small_is_its_own_code():
    _refused("tfgx_spasp_emit", EMIT_OK, dict(ws_bytes=16), "workspace_bytes", code=3)
    _refused("tfgx_spasp_reduce", REDUCE_OK, dict(ws_bytes=16), "workspace_bytes", code=3)


def test_count_refusals_and_size_queries():
    lib = _lib()
    total = ctypes.c_int64(-5)
    args = dict(s_row_ptr=8, s_col=8, N=4, K=2, a_row=8, a_col=8, E=6, s_deg=8, offsets=8, total=ctypes.byref(total), ws=8,
                ws_bytes=1 << 20, stream=None)
    for change, word in ((dict(N=-1), "negative"), (dict(E=1 << 31), "fit int32"), (dict(offsets=None), "offsets is null"),
                         (dict(total=None), "total is null")):
        assert lib.tfgx_spasp_count(*dict(args, **change).values()) == 1
        assert word in lib.tfgx_last_error().decode()
    assert lib.tfgx_spasp_count_workspace_bytes(-1, 3) == 0 and lib.tfgx_spasp_count_workspace_bytes(4, 1 << 31) == 0
    assert lib.tfgx_spasp_count_workspace_bytes(4, 6) >= 8 * 7
    assert lib.tfgx_spasp_workspace_bytes(0, 2) == 0 and lib.tfgx_spasp_workspace_bytes(10, 0) == 0
    assert lib.tfgx_spasp_workspace_bytes(10, 2) >= 10 * (8 + 8 + 4 + 4 + 4 + 4)


def test_zero_sizes_succeed_without_device_work():
    lib = _lib()
    null = {k: None for k in ("row_ptr", "col", "x", "sq", "sh", "bias", "c", "p", "p_self")}
    assert lib.tfgx_asap_attend_f32(*dict(ATT_OK, **dict(null, N=0, E=0)).values()) == 0
    bnull = {k: None for k in ("row_ptr", "col", "sq", "sh", "bias", "p", "p_self", "dp", "dp_self", "ds", "ds_self", "dsq")}
    assert lib.tfgx_asap_attend_backward_f32(*dict(BWD_OK, **dict(bnull, N=0, E=0)).values()) == 0
    enull = {k: None for k in ("s_row_ptr", "s_col", "a_row", "a_col", "s_deg", "offsets", "ws")}
    assert lib.tfgx_spasp_emit(*dict(EMIT_OK, **dict(enull, total=0, ws_bytes=0)).values()) == 0


def test_public_names_and_constructor():
    import torch
    import tf_geometric_amd as tfg
    assert callable(tfg.nn.asap) and tfg.nn.pool.asap is tfg.nn.asap and tfg.nn.pool.cluster_pool is tfg.nn.cluster_pool
    assert tfg.layers.ASAP is tfg.layers.pool.ASAP
    layer = tfg.layers.ASAP(ratio=0.5)
    assert layer.k is None and layer.ratio == 0.5 and layer.drop_rate == 0.0 and layer.attention_units is None
    assert layer.le_conv_activation is torch.sigmoid and layer.le_conv_use_bias is True
    assert callable(tfg.utils.convert_dense_adj_to_edge) and callable(tfg.utils.convert_dense_assign_to_edge)
