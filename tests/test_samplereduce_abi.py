# coding=utf-8
"""include/tfgx_samplereduce.h (the fused input hop of minibatch GraphSAGE) without a GPU: the exact list of its names, its
macros, every refusal on the host with the argument named, the zero-size call, the Python mirror of the draw limit, and the
refusals of RandomNeighborSampler.sample_reduce that need no device.  The uniform header / table / version checks are
tests/test_abi_registry.py's, through the registry entry."""
import os

import numpy as np
import pytest

from abi_header import INCLUDE, declarations, macro, refused as _refused

HEADER = "tfgx_samplereduce.h"
NAMES = ["tfgx_samplereduce_f32", "tfgx_samplereduce_version"]


def test_samplereduce_symbols_and_macros():
    from tf_geometric_amd import _lib as L
    assert sorted(declarations(HEADER)) == sorted(L.SAMPLEREDUCE_SIGNATURES) == NAMES
    assert macro(HEADER, "TFGX_SAMPLEREDUCE_ABI_VERSION") == L.SAMPLEREDUCE_ABI_VERSION == 1
    assert macro(HEADER, "TFGX_SAMPLEREDUCE_MAX_DRAWS") == L.SAMPLEREDUCE_MAX_DRAWS >= 128
    assert macro(HEADER, "TFGX_SAMPLEREDUCE_BAD_RANGE") == macro("tfgx_nbrblock.h", "TFGX_NBRBLOCK_BAD_RANGE") \
        == L.SAMPLEREDUCE_BAD_RANGE == L.NBRBLOCK_BAD_RANGE
    for abi in L.ABIS:
        assert abi.signatures is L.SAMPLEREDUCE_SIGNATURES or not any("samplereduce" in n for n in abi.signatures), abi.header
    # a header of its own: nothing was added to tfgx.h or tfgx_nbrblock.h, and no constant was registered for it
    for other in ("tfgx.h", "tfgx_nbrblock.h"):
        assert "samplereduce" not in open(os.path.join(INCLUDE, other)).read()
    assert [a.constants for a in L.ABIS if a.header == HEADER] == [()]


P = [(i + 1) << 30 for i in range(12)]        # fake device pointers: never dereferenced on the host
OK = dict(row_ptr=P[0], col=P[1], w=P[2], n_nodes=100, rows=P[3], n_rows=10, k=5, replace=0, seed=7, x=P[4], ldx=16, F=12, op=1,
          out=P[5], ldo=12, out_count=P[6], bad_flag=P[7], stream=None)
BIG = 1 << 31


def _max_draws():
    return macro(HEADER, "TFGX_SAMPLEREDUCE_MAX_DRAWS")


@pytest.mark.parametrize("change, word", [
    (dict(n_nodes=-1), "negative size (n_nodes"),
    (dict(n_rows=-1), "negative size (n_rows"),
    (dict(n_nodes=BIG), "n_nodes = 2147483648 does not fit int32"),
    (dict(n_rows=BIG), "n_rows = 2147483648 does not fit int32"),
    (dict(k=-1), "k must not be negative"),
    (dict(k="above"), "k is above TFGX_SAMPLEREDUCE_MAX_DRAWS"),
    (dict(F=0), "F must be at least 1"),
    (dict(F=-3), "F must be at least 1"),
    (dict(ldx=11), "ldx must be at least F"),
    (dict(ldo=11), "ldo must be at least F"),
    (dict(op=2), "op must be TFGX_SUM or TFGX_MEAN"),
    (dict(op=-1), "op must be TFGX_SUM or TFGX_MEAN"),
    (dict(row_ptr=None), "row_ptr is null"),
    (dict(col=None), "col is null"),
    (dict(rows=None), "rows is null"),
    (dict(x=None), "x is null"),
    (dict(out=None), "out is null"),
    (dict(bad_flag=None), "bad_flag is null"),
], ids=lambda v: "-".join("{}={}".format(*i) for i in v.items()) if isinstance(v, dict) else None)
def test_host_side_refusals_name_the_argument(change, word):
    """TFGX_ERR_INVALID_ARG (1) on the host, before any device work: the pointers here are not memory."""
    if change.get("k") == "above":
        change = dict(k=_max_draws() + 1)
    _refused("tfgx_samplereduce_f32", OK, change, word)


def test_optional_pointers_and_the_zero_size_call():
    from tf_geometric_amd import _lib as L
    lib = L.load_library()
    nothing = {k: None for k in ("row_ptr", "col", "w", "rows", "x", "out", "out_count", "bad_flag")}
    assert lib.tfgx_samplereduce_f32(*dict(OK, n_rows=0).values()) == 0, lib.tfgx_last_error()
    assert lib.tfgx_samplereduce_f32(*dict(OK, n_rows=0, n_nodes=0, **nothing).values()) == 0
    assert lib.tfgx_samplereduce_f32(*dict(OK, n_rows=0, k=_max_draws(), **nothing).values()) == 0
    # the sizes are still checked when there is nothing to do
    _refused("tfgx_samplereduce_f32", dict(OK, n_rows=0), dict(k=_max_draws() + 1), "k is above")
    _refused("tfgx_samplereduce_f32", dict(OK, n_rows=0), dict(F=0), "F must be at least 1")


def test_the_python_mirror_of_the_draw_limit():
    from tf_geometric_amd import _lib as L
    from tf_geometric_amd.utils import minibatch as M
    assert L.SAMPLEREDUCE_MAX_DRAWS == _max_draws()
    assert M.sample_reduce_route(0, None) == M.sample_reduce_route(L.SAMPLEREDUCE_MAX_DRAWS, None) == "fused"
    assert M.sample_reduce_route(L.SAMPLEREDUCE_MAX_DRAWS + 1, None) == "composed"
    assert M.sample_reduce_route(np.int64(5), np.zeros((3, 2), np.float32)) == "fused"


def _bare_sampler():
    """A sampler object without its graph: the checks below must all come before anything touches the device."""
    import tf_geometric_amd as tfg
    return object.__new__(tfg.utils.RandomNeighborSampler)


def test_python_refusals_before_any_device_work():
    from tf_geometric_amd.utils import minibatch as M
    s = _bare_sampler()
    x = np.zeros((4, 3), dtype=np.float32)
    with pytest.raises(ValueError, match="no fused form for k=None"):
        s.sample_reduce([0, 1], x, k=None)
    with pytest.raises(ValueError, match="no fused form for k=None"):
        s.sample_reduce([0, 1], x)
    with pytest.raises(ValueError, match="no fused form for ratio="):
        s.sample_reduce([0, 1], x, ratio=0.5)
    with pytest.raises(ValueError, match="no fused form for ratio="):
        s.sample_reduce([0, 1], x, k=3, ratio=0.5)
    with pytest.raises(ValueError, match="negative"):
        s.sample_reduce([0, 1], x, k=-1)
    with pytest.raises(ValueError, match="integer"):
        s.sample_reduce([0, 1], x, k=2.5)
    with pytest.raises(ValueError, match="integer"):
        s.sample_reduce([0, 1], x, k=True)
    with pytest.raises(ValueError, match="op must be"):
        s.sample_reduce([0, 1], x, k=3, op="max")
    with pytest.raises(ValueError, match="rows must be integers"):
        s.sample_reduce(np.asarray([0.5]), x, k=3)
    with pytest.raises(ValueError, match="one-dimensional"):
        s.sample_reduce(np.zeros((2, 2), dtype=np.int64), x, k=3)
    for check in (M.check_sample_reduce_args, M.sample_reduce_route):
        with pytest.raises(ValueError, match="k=None"):
            check(None, None)
    # a minibatch that was not sampled with fuse_input_hop has no input hop to aggregate
    import tf_geometric_amd as tfg
    with pytest.raises(ValueError, match="fuse_input_hop=True"):
        tfg.utils.SampledMinibatch([], None, 0, []).input_aggregate(x)


def test_the_layers_expose_combine():
    import tf_geometric_amd as tfg
    assert callable(tfg.nn.graph_sage_combine)
    assert callable(tfg.layers.MeanGraphSage.combine) and callable(tfg.layers.SumGraphSage.combine)
    for other in (tfg.layers.GCNGraphSage, tfg.layers.MeanPoolGraphSage, tfg.layers.MaxPoolGraphSage, tfg.layers.LSTMGraphSage):
        assert not hasattr(other, "combine"), other
