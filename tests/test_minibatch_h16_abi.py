# coding=utf-8
"""include/tfgx_minibatch_h16.h (the minibatch route over a 16-bit feature table) without a GPU: the exact list of its names,
every refusal on the host with the argument named, the zero-size calls, and the Python refusals that need no device — an
undeclared HalfRows, a 16-bit tensor, a declared table whose source requires grad — with minibatch=True reaching HalfRows
through prepare_half_features.  The uniform header / table / version checks are tests/test_abi_registry.py's, through the
registry entry."""
import inspect

import numpy as np
import pytest
import torch

from abi_header import declarations, macro, refused as _refused

HEADER = "tfgx_minibatch_h16.h"
NAMES = ["tfgx_gather_rows_h16_f32", "tfgx_minibatch_h16_version", "tfgx_nbr_static_input_hop_h16", "tfgx_sample_reduce_h16"]


def test_symbols_and_macros():
    from tf_geometric_amd import _lib as L
    assert sorted(declarations(HEADER)) == sorted(L.MINIBATCH_H16_SIGNATURES) == NAMES
    assert macro(HEADER, "TFGX_MINIBATCH_H16_ABI_VERSION") == L.MINIBATCH_H16_ABI_VERSION == 1
    assert L.load_library().tfgx_minibatch_h16_version() == 1
    assert [a.constants for a in L.ABIS if a.header == HEADER] == [()]
    # one new header: the float32 entry points keep their signatures and versions
    assert macro("tfgx_samplereduce.h", "TFGX_SAMPLEREDUCE_ABI_VERSION") == 1 and macro("tfgx_nbrstatic.h", "TFGX_NBRSTATIC_ABI_VERSION") == 1
    assert macro("tfgx_h16.h", "TFGX_H16_ABI_VERSION") == 1
    assert len(L.SAMPLEREDUCE_SIGNATURES["tfgx_samplereduce_f32"][1]) + 1 == len(L.MINIBATCH_H16_SIGNATURES["tfgx_sample_reduce_h16"][1])
    assert len(L.NBRSTATIC_SIGNATURES["tfgx_nbrstatic_input_hop_f32"][1]) + 1 == \
        len(L.MINIBATCH_H16_SIGNATURES["tfgx_nbr_static_input_hop_h16"][1])


P = [(i + 1) << 30 for i in range(12)]        # fake device pointers, 16-byte aligned: never dereferenced on the host
BF16, F16 = 1, 2
REDUCE_OK = dict(row_ptr=P[0], col=P[1], w=P[2], n_nodes=100, rows=P[3], n_rows=10, k=5, replace=0, seed=7, x=P[4], ldx=16, F=12,
                 x_dtype=BF16, op=1, out=P[5], ldo=12, out_count=P[6], bad_flag=P[7], stream=None)
STATIC_OK = dict(row_ptr=P[0], col=P[1], w=P[2], n_nodes=100, node=P[3], n_rows=10, k=5, replace=0, seed=P[8], hop=1, x=P[4],
                 ldx=16, F=12, x_dtype=F16, op=1, out=P[5], ldo=12, out_count=P[6], bad_flag=P[7], stream=None)
GATHER_OK = dict(x=P[0], ldx=16, x_dtype=BF16, idx=P[1], M=10, F=12, out=P[2], ldo=12, stream=None)
BIG = 1 << 31
FNS = {"tfgx_sample_reduce_h16": REDUCE_OK, "tfgx_nbr_static_input_hop_h16": STATIC_OK, "tfgx_gather_rows_h16_f32": GATHER_OK}

TABLE = [        # what a 16-bit table adds, refused by all three
    (dict(x_dtype=0), "x_dtype must be TFGX_DT_BF16 or TFGX_DT_F16"),
    (dict(x_dtype=3), "x_dtype must be TFGX_DT_BF16 or TFGX_DT_F16"),
    (dict(x_dtype=-1), "x_dtype must be TFGX_DT_BF16 or TFGX_DT_F16"),
    (dict(ldx=20), "ldx must be a multiple of 8"),
    (dict(ldx=12), "ldx must be a multiple of 8"),
    (dict(x=P[4] + 2), "x must be 16-byte aligned"),
    (dict(x=P[4] + 8), "x must be 16-byte aligned"),
    (dict(ldx=8), "ldx must be at least F"),
    (dict(F=0), "F must be at least 1"),
    (dict(F=-3), "F must be at least 1"),
    (dict(ldo=11), "ldo must be at least F"),
    (dict(x=None), "x is null"),
    (dict(out=None), "out is null"),
]
LAUNCH = [       # the float32 launch's own, through both 16-bit forms of it
    (dict(n_nodes=-1), "negative size (n_nodes"),
    (dict(n_rows=-1), "negative size (n_rows"),
    (dict(n_nodes=BIG), "n_nodes = 2147483648 does not fit int32"),
    (dict(n_rows=BIG), "n_rows = 2147483648 does not fit int32"),
    (dict(k=-1), "k must not be negative"),
    (dict(k="above"), "k is above TFGX_SAMPLEREDUCE_MAX_DRAWS"),
    (dict(op=2), "op must be TFGX_SUM or TFGX_MEAN"),
    (dict(op=-1), "op must be TFGX_SUM or TFGX_MEAN"),
    (dict(row_ptr=None), "row_ptr is null"),
    (dict(col=None), "col is null"),
    (dict(bad_flag=None), "bad_flag is null"),
]
CASES = [(fn, c, w) for fn in FNS for c, w in TABLE] + \
        [(fn, c, w) for fn in ("tfgx_sample_reduce_h16", "tfgx_nbr_static_input_hop_h16") for c, w in LAUNCH] + [
    ("tfgx_sample_reduce_h16", dict(rows=None), "rows is null"),
    ("tfgx_nbr_static_input_hop_h16", dict(node=None), "node is null"),
    ("tfgx_nbr_static_input_hop_h16", dict(seed=None), "seed is null"),
    ("tfgx_nbr_static_input_hop_h16", dict(hop=-1), "hop must not be negative"),
    ("tfgx_gather_rows_h16_f32", dict(M=-1), "negative size (M"),
    ("tfgx_gather_rows_h16_f32", dict(M=BIG), "M = 2147483648 does not fit int32"),
    ("tfgx_gather_rows_h16_f32", dict(idx=None), "idx is null"),
]


@pytest.mark.parametrize("fn, change, word", CASES,
                         ids=["{}-{}".format(fn[5:], "-".join("{}={}".format(*i) for i in c.items())) for fn, c, _ in CASES])
def test_host_side_refusals_name_the_argument(fn, change, word):
    """TFGX_ERR_INVALID_ARG (1) on the host, before any device work: the pointers here are not memory."""
    if change.get("k") == "above":
        change = dict(k=macro("tfgx_samplereduce.h", "TFGX_SAMPLEREDUCE_MAX_DRAWS") + 1)
    _refused(fn, FNS[fn], change, word)


def test_the_zero_size_calls_launch_nothing():
    from tf_geometric_amd import _lib as L
    lib = L.load_library()
    limit = macro("tfgx_samplereduce.h", "TFGX_SAMPLEREDUCE_MAX_DRAWS")
    for fn, ok, ptrs in (("tfgx_sample_reduce_h16", REDUCE_OK, ("row_ptr", "col", "w", "rows", "x", "out", "out_count", "bad_flag")),
                         ("tfgx_nbr_static_input_hop_h16", STATIC_OK,
                          ("row_ptr", "col", "w", "node", "seed", "x", "out", "out_count", "bad_flag"))):
        nothing = {k: None for k in ptrs}
        for dt in (BF16, F16):
            assert getattr(lib, fn)(*dict(ok, n_rows=0, x_dtype=dt).values()) == 0, lib.tfgx_last_error()
            assert getattr(lib, fn)(*dict(ok, n_rows=0, n_nodes=0, k=limit, x_dtype=dt, **nothing).values()) == 0
        # the sizes and the table are still checked when there is nothing to do
        _refused(fn, dict(ok, n_rows=0), dict(k=limit + 1), "k is above")
        _refused(fn, dict(ok, n_rows=0), dict(x_dtype=0), "x_dtype must be")
        _refused(fn, dict(ok, n_rows=0), dict(ldx=20), "ldx must be a multiple of 8")
    for dt in (BF16, F16):
        assert lib.tfgx_gather_rows_h16_f32(*dict(GATHER_OK, M=0, x_dtype=dt).values()) == 0
        assert lib.tfgx_gather_rows_h16_f32(*dict(GATHER_OK, M=0, x_dtype=dt, x=None, idx=None, out=None).values()) == 0
    _refused("tfgx_gather_rows_h16_f32", dict(GATHER_OK, M=0), dict(F=0), "F must be at least 1")
    _refused("tfgx_gather_rows_h16_f32", dict(GATHER_OK, M=0), dict(x_dtype=0), "x_dtype must be")


# ---- Python, before any device work -------------------------------------------------------------------------------------
def _bare(cls):
    """An object without its graph or device state: every check below must come before anything touches the device."""
    return object.__new__(cls)


def _host_table(dtype, minibatch, source=None):
    from tf_geometric_amd.plan import HalfRows
    t = torch.zeros((4, 8), dtype=dtype) if source is None else source.detach()
    return HalfRows(t, 3 if source is None else int(source.shape[1]), source=source, minibatch=minibatch)


def _bare_static(tfg, input_hop=None):
    mb = _bare(tfg.utils.StaticMinibatch)
    mb.node_index, mb._n_nodes, mb.input_hop = None, 0, input_hop
    return mb


def _static_with_input_hop(tfg):
    return _bare_static(tfg, (5, False, 0))


def test_the_flag_reaches_halfrows():
    import tf_geometric_amd as tfg
    from tf_geometric_amd.plan import HalfRows
    for fn in (tfg.prepare_half_features, HalfRows.__init__, HalfRows.from_dense, HalfRows.from_tensor):
        assert inspect.signature(fn).parameters["minibatch"].default is False, fn
    assert _host_table(torch.bfloat16, True).minibatch is True and _host_table(torch.float16, False).minibatch is False
    assert _host_table(torch.bfloat16, True).gemm_operand is False
    seen = []
    real = HalfRows.from_dense
    try:
        HalfRows.from_dense = staticmethod(lambda x, **kw: seen.append(kw) or "table")
        x = np.zeros((4, 3), dtype=np.float32)
        assert tfg.prepare_half_features(x, torch.float16, minibatch=True) == "table"
        assert tfg.prepare_half_features(x) == "table"
    finally:
        HalfRows.from_dense = staticmethod(real)
    assert [kw["minibatch"] for kw in seen] == [True, False] and seen[0]["dtype"] == torch.float16
    assert [kw["gemm_operand"] for kw in seen] == [False, False]


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
def test_an_undeclared_table_and_a_16_bit_tensor_are_refused_as_before(dtype):
    import tf_geometric_amd as tfg
    s = _bare(tfg.utils.RandomNeighborSampler)
    dyn = tfg.utils.SampledMinibatch([], None, 0, [], input_hop=(5, False, 1), sampler=s)
    h = _host_table(dtype, False)
    for call in (lambda: s.sample_reduce([0, 1], h, k=3), lambda: dyn.gather(h), lambda: dyn.input_aggregate(h),
                 lambda: _bare_static(tfg).gather(h), lambda: _static_with_input_hop(tfg).input_aggregate(h)):
        with pytest.raises(TypeError, match=r"float32 table, got a HalfRows.*minibatch=True"):
            call()
    t = torch.zeros((4, 3), dtype=dtype)
    for call in (lambda: s.sample_reduce([0, 1], t, k=3), lambda: dyn.gather(t), lambda: dyn.input_aggregate(t),
                 lambda: _bare_static(tfg).gather(t)):
        with pytest.raises(TypeError, match="takes a float32 table, got torch"):
            call()
    with pytest.raises(ValueError, match="takes a float32 table, got torch"):
        _static_with_input_hop(tfg).input_aggregate(t)


def test_a_declared_table_takes_the_routes_of_a_float32_one():
    import tf_geometric_amd as tfg
    from tf_geometric_amd import _lib as L
    from tf_geometric_amd.utils import minibatch as M
    h = _host_table(torch.bfloat16, True)
    assert M.sample_reduce_route(0, h) == M.sample_reduce_route(L.SAMPLEREDUCE_MAX_DRAWS, h) == "fused"
    assert M.sample_reduce_route(L.SAMPLEREDUCE_MAX_DRAWS + 1, h) == "composed"
    src = torch.zeros((4, 8), dtype=torch.bfloat16, requires_grad=True)
    trained = _host_table(torch.bfloat16, True, source=src)
    assert trained.requires_grad and M.sample_reduce_route(5, trained) == "composed"
    with torch.no_grad():
        assert M.sample_reduce_route(5, trained) == "fused"
    # a trained table is refused by name where the float32 one is refused or goes through torch's indexing
    for mb in (tfg.utils.SampledMinibatch([], None, 0, []), _bare_static(tfg)):
        with pytest.raises(NotImplementedError, match="source requires grad"):
            mb.gather(trained)
    with pytest.raises(ValueError, match="carries no gradient to a table that requires grad"):
        _static_with_input_hop(tfg).input_aggregate(trained)
    # the checks of the arguments beside the table come first, as for a float32 one
    s = _bare(tfg.utils.RandomNeighborSampler)
    with pytest.raises(ValueError, match="no fused form for k=None"):
        s.sample_reduce([0, 1], h)
    with pytest.raises(ValueError, match="op must be"):
        s.sample_reduce([0, 1], h, k=3, op="max")
    with pytest.raises(ValueError, match="fuse_input_hop=True"):
        tfg.utils.SampledMinibatch([], None, 0, []).input_aggregate(h)
