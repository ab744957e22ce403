# coding=utf-8
"""include/tfgx_dropedge.h (DropEdge) without a GPU: the exact list of its names, of which tfgx.h knows none (the uniform header /
table / version / struct checks are tests/test_abi_registry.py's), the host argument checks name the refused member before
any device work, E = 0 succeeds, the numpy mirror of the whole operator (both forms, attributes included; used as the exact
reference by tests/test_gpu_drop_edge.py) keeps its promises, the keep rule's kept fraction sits inside the binomial's
5 sigma, and the Python entry points return their inputs when not training."""
import ctypes

import numpy as np
import pytest
import torch

from abi_header import declarations, source

HEADER = "tfgx_dropedge.h"


def _lib():
    from tf_geometric_amd import _lib
    return _lib.load_library()


# ---- the mirror: test infrastructure shared with the GPU tests ------------------------------------------------------------
def keep_mask(seed, E, rate):
    """tfgx_dropout_keep (host-callable) for edge ids 0 .. E-1."""
    lib = _lib()
    return np.fromiter((lib.tfgx_dropout_keep(seed, i, rate) for i in range(E)), dtype=bool, count=E)


def mirror_drop_edge(ei, attrs, rate, seed, force_undirected=False):
    """numpy restatement of tf_geometric/nn/sampling/drop_edge.py:31-47 with the library's keep rule as the mask:
    (dropped edge_index, index of original ids, dropped attributes)."""
    ei = np.asarray(ei).reshape(2, -1)
    row, col = ei[0], ei[1]
    keep = keep_mask(seed, ei.shape[1], rate)
    if force_undirected:
        index = np.nonzero(row < col)[0]                                   # :33
        index = index[keep[index]]                                         # :34  (each candidate keyed on its own id)
        out = ei[:, index]                                                 # :35
        out = np.concatenate([out, out[[1, 0]]], axis=-1)                  # :36
        index = np.concatenate([index, index], axis=-1)                    # :37
    else:
        index = np.nonzero(keep)[0]                                        # :39-40
        out = ei[:, index]                                                 # :41
    return out.astype(np.int32), index.astype(np.int32), [np.take(a, index, axis=-1) for a in attrs]   # :43-47


def mirror_plan(ei, n_dst):
    """tfgx_build_csr_by_dst as numpy: a stable sort by destination -> (row_ptr, col, perm)."""
    ei = np.asarray(ei).reshape(2, -1)
    perm = np.argsort(ei[0], kind="stable").astype(np.int32)
    row_ptr = np.concatenate([[0], np.cumsum(np.bincount(ei[0], minlength=n_dst))]).astype(np.int32)
    return row_ptr, ei[1][perm].astype(np.int32), perm


def _random_edges(rng, n_dst, n_src, e):
    return np.stack([rng.integers(0, n_dst, e), rng.integers(0, n_src, e)]).astype(np.int32)


# ---- ABI -------------------------------------------------------------------------------------------------------------------
def test_dropedge_symbols_and_versions():
    from tf_geometric_amd import _lib as L
    assert sorted(declarations(HEADER)) == sorted(L.DROPEDGE_SIGNATURES) == [
        "tfgx_drop_edge_count", "tfgx_drop_edge_emit", "tfgx_drop_edge_workspace_bytes", "tfgx_dropedge_version"]
    assert not any("drop_edge" in n or "dropedge" in n for n in L.SIGNATURES)
    assert "drop_edge" not in source("tfgx.h") and "dropedge" not in source("tfgx.h")
    # struct tfgx_drop_edge_plan: six pointers
    assert [t for _, t in L.DropEdgePlan._fields_] == [ctypes.c_void_p] * 6


def _count(lib, row=1 << 30, col=2 << 30, E=10, n_dst=5, n_src=5, rate=0.5, seed=1, und=0, n_out=True, ws=3 << 30, ws_bytes=1 << 20):
    out = ctypes.c_int64(-7)
    rc = lib.tfgx_drop_edge_count(row, col, E, n_dst, n_src, rate, seed, und, ctypes.byref(out) if n_out else None, ws, ws_bytes, None)
    return rc, out.value


def _emit(lib, row=1 << 30, col=2 << 30, E=10, n_dst=5, n_src=5, rate=0.5, seed=1, und=0, n_out=4, o_row=4 << 30, o_col=5 << 30,
          o_id=6 << 30, plan=None, plan_t=None, ws=3 << 30, ws_bytes=1 << 20):
    return lib.tfgx_drop_edge_emit(row, col, E, n_dst, n_src, rate, seed, und, n_out, o_row, o_col, o_id,
                                   None if plan is None else ctypes.byref(plan), None if plan_t is None else ctypes.byref(plan_t),
                                   ws, ws_bytes, None)


def test_dropedge_argument_validation_without_gpu():
    """Every refusal returns TFGX_ERR_INVALID_ARG (1) on the host, before any device work, with the member named."""
    from tf_geometric_amd import _lib as L
    lib = L.load_library()

    def refused(rc, word):
        assert rc == 1, rc
        assert word in lib.tfgx_last_error(), (word, lib.tfgx_last_error())

    for fn in (lambda **kw: _count(lib, **kw)[0], lambda **kw: _emit(lib, **kw)):
        refused(fn(rate=-0.1), b"rate")
        refused(fn(rate=1.5), b"rate")
        refused(fn(rate=float("nan")), b"rate")
        refused(fn(E=-1), b"negative size")
        refused(fn(n_dst=-1), b"negative size")
        refused(fn(n_src=-2), b"negative size")
        refused(fn(E=1 << 31), b"int32")
        refused(fn(row=None), b"row is null")
        refused(fn(col=None), b"col is null")
        refused(fn(und=2), b"force_undirected")
        refused(fn(und=1, n_src=6), b"n_dst == n_src")
        refused(fn(ws=None), b"workspace is null")
        refused(fn(ws=(3 << 30) + 4), b"16-byte aligned")
    refused(_count(lib, n_out=False)[0], b"n_out")
    assert _count(lib, ws_bytes=8)[0] == 3 and b"workspace too small" in lib.tfgx_last_error()        # TFGX_ERR_WORKSPACE
    assert _emit(lib, ws_bytes=8) == 3 and b"workspace too small" in lib.tfgx_last_error()
    refused(_emit(lib, n_out=-1), b"n_out")
    refused(_emit(lib, n_out=11), b"n_out")
    refused(_emit(lib, und=1, n_out=3), b"n_out")
    refused(_emit(lib, und=1, n_out=22), b"n_out")                 # the mirrored form emits at most 2 E edges
    assert _emit(lib, und=1, n_out=12, ws_bytes=8) == 3              # ... and 12 > E = 10 is a legal count there
    refused(_emit(lib, o_row=None), b"out_row is null")
    refused(_emit(lib, o_col=None), b"out_col is null")
    refused(_emit(lib, o_id=None), b"out_edge_id is null")
    full = dict(parent_row_ptr=7 << 30, parent_col=8 << 30, parent_perm=9 << 30, out_row_ptr=10 << 30, out_col=11 << 30,
                out_perm=12 << 30)
    for member in full:
        p = L.DropEdgePlan(**dict(full, **{member: None}))
        refused(_emit(lib, plan=p), b"plan->" + member.encode())
        refused(_emit(lib, plan_t=p), b"plan_t->" + member.encode())
    refused(_emit(lib, und=1, plan=L.DropEdgePlan(**full)), b"force_undirected")
    # sizes: 0 for negative input, grows with E, and the plans cost workspace
    assert lib.tfgx_drop_edge_workspace_bytes(-1, 4, 4, 0, 0) == 0 and lib.tfgx_drop_edge_workspace_bytes(4, -1, 4, 0, 0) == 0
    small, big = lib.tfgx_drop_edge_workspace_bytes(10, 4, 4, 0, 0), lib.tfgx_drop_edge_workspace_bytes(1 << 20, 4, 4, 0, 0)
    assert 0 < small < big < lib.tfgx_drop_edge_workspace_bytes(1 << 20, 4, 4, 1, 0)
    assert lib.tfgx_drop_edge_workspace_bytes(1 << 20, 4, 4, 1, 0) == lib.tfgx_drop_edge_workspace_bytes(1 << 20, 4, 4, 1, 1)


def test_dropedge_empty_edge_list_succeeds_without_gpu():
    lib = _lib()
    for und in (0, 1):
        rc, n_out = _count(lib, row=None, col=None, E=0, und=und, ws=None, ws_bytes=0)
        assert rc == 0 and n_out == 0, lib.tfgx_last_error()
        assert _emit(lib, row=None, col=None, E=0, und=und, n_out=0, o_row=None, o_col=None, o_id=None, ws=None, ws_bytes=0) == 0
    assert _count(lib, row=None, col=None, E=0, n_dst=0, n_src=0, rate=1.0, ws=None, ws_bytes=0) == (0, 0)


# ---- the keep rule -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rate", [0.3, 0.5])
@pytest.mark.parametrize("seed", [1, 0x9E3779B97F4A7C15, (0xDEADBEEF << 32) | 42])
def test_kept_fraction_within_five_sigma(rate, seed):
    """E = 200 000 ids: 5 sigma of the binomial, 5 sqrt(p (1 - p) / E), is 0.0052 at rate 0.3 and 0.0056 at rate 0.5.  The
    hash alone is checked, on the host."""
    E = 200000
    frac = float(keep_mask(seed, E, rate).mean())
    print("rate {} seed {:#x}: kept fraction {:.5f}".format(rate, seed, frac))
    assert abs(frac - (1.0 - rate)) <= {0.3: 0.0052, 0.5: 0.0056}[rate], (rate, seed, frac)


def test_keep_rule_end_points_and_seed_dependence():
    assert keep_mask(5, 3000, 0.0).all() and not keep_mask(5, 3000, 1.0).any()
    a, b = keep_mask(5, 3000, 0.5), keep_mask(6, 3000, 0.5)
    assert np.array_equal(a, keep_mask(5, 3000, 0.5)) and not np.array_equal(a, b)
    assert abs(float((a == b).mean()) - 0.5) < 0.05           # different seeds: independent-looking masks
    # a higher rate only ever drops more (one threshold on one hash)
    assert not (keep_mask(5, 3000, 0.6) & ~keep_mask(5, 3000, 0.3)).any()


# ---- the mirror ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("E", [0, 1, 2049, 5000])
@pytest.mark.parametrize("rate", [0.0, 0.37, 1.0])
def test_mirror_plain_form(E, rate):
    rng = np.random.Generator(np.random.PCG64(100 + E))
    ei = _random_edges(rng, 40, 23, E)
    w, a2 = rng.standard_normal(E).astype(np.float32), rng.standard_normal((3, E)).astype(np.float32)
    out, index, (dw, da2) = mirror_drop_edge(ei, [w, a2], rate, seed=77)
    keep = keep_mask(77, E, rate)
    assert out.shape == (2, int(keep.sum())) and index.shape == (int(keep.sum()),) and dw.shape == index.shape
    assert da2.shape == (3, index.shape[0])
    assert (np.diff(index) > 0).all()                              # original order, no id twice
    assert np.array_equal(out, ei[:, keep]) and np.array_equal(dw, w[keep]) and np.array_equal(da2, a2[:, keep])
    if rate == 0.0:
        assert np.array_equal(out, ei) and np.array_equal(index, np.arange(E))
    if rate == 1.0:
        assert out.shape == (2, 0) and dw.shape == (0,) and da2.shape == (3, 0)


@pytest.mark.parametrize("rate", [0.0, 0.37, 1.0])
def test_mirror_undirected_form(rate):
    rng = np.random.Generator(np.random.PCG64(7))
    half = _random_edges(rng, 50, 50, 1500)
    ei = np.concatenate([half, half[[1, 0]]], axis=1)               # symmetric, with self-loops and duplicates
    E = ei.shape[1]
    w = rng.standard_normal(E).astype(np.float32)
    out, index, (dw,) = mirror_drop_edge(ei, [w], rate, seed=9, force_undirected=True)
    K = out.shape[1] // 2
    assert out.shape[1] == 2 * K == index.shape[0] == dw.shape[0]
    assert (out[0, :K] < out[1, :K]).all() and np.array_equal(out[:, K:], out[[1, 0], :K])
    assert np.array_equal(index[:K], index[K:]) and (np.diff(index[:K]) > 0).all()
    assert np.array_equal(out[:, :K], ei[:, index[:K]]) and np.array_equal(dw, w[index])
    upper = ei[0] < ei[1]
    assert K == int((upper & keep_mask(9, E, rate)).sum())
    if rate == 0.0:
        assert K == int(upper.sum())
    # a list without any row < col edge gives an empty result
    lower = np.stack([np.maximum(half[0], half[1]), np.minimum(half[0], half[1])])
    out, index, (dw,) = mirror_drop_edge(lower, [w[:1500]], rate, seed=9, force_undirected=True)
    assert out.shape == (2, 0) and index.shape == (0,) and dw.shape == (0,)


def test_mirror_plan_is_a_stable_sort():
    rng = np.random.Generator(np.random.PCG64(3))
    ei = _random_edges(rng, 17, 9, 400)
    row_ptr, col, perm = mirror_plan(ei, 17)
    assert row_ptr[0] == 0 and row_ptr[-1] == 400 and row_ptr.shape == (18,)
    for r in range(17):
        p = perm[row_ptr[r]:row_ptr[r + 1]]
        assert (ei[0][p] == r).all() and (np.diff(p) > 0).all()
    assert np.array_equal(col, ei[1][perm])


# ---- Python surface --------------------------------------------------------------------------------------------------------------
def test_not_training_returns_the_input_objects():
    import tf_geometric_amd as tfg
    ei, w = np.zeros((2, 5), np.int32), torch.ones(5)
    for inputs in ([ei, w], (ei,), [torch.zeros(2, 5, dtype=torch.int32), w, w]):
        for training in (None, False, 0):
            assert tfg.nn.drop_edge(inputs, rate=0.5, training=training) is inputs
            assert tfg.layers.DropEdge(0.3)(inputs, training=training) is inputs
            assert tfg.layers.DropEdge(0.3, force_undirected=True).call(inputs, training=training) is inputs
    assert tfg.nn.drop_edge([ei, w]) is not None and tfg.nn.drop_edge([ei, w])[1] is w          # training defaults to None
    assert tfg.nn.drop_edge([ei], rate=7.0, training=False)[0] is ei                             # reference: rate unchecked here


def test_rate_outside_unit_interval_raises_value_error():
    import tf_geometric_amd as tfg
    ei = np.zeros((2, 5), np.int32)
    for rate in (-0.1, 1.5):
        with pytest.raises(ValueError, match="Dropout probability has to be between 0 and 1"):
            tfg.nn.drop_edge([ei], rate=rate, training=True)
        with pytest.raises(ValueError, match="Dropout probability has to be between 0 and 1"):
            tfg.layers.DropEdge(rate)
    layer = tfg.layers.DropEdge()
    assert layer.rate == 0.5 and layer.force_undirected is False and layer.parameters() == []


def test_training_needs_a_gpu():
    import tf_geometric_amd as tfg
    if torch.cuda.is_available():
        pytest.skip("a GPU is present: the refusal cannot be observed")
    with pytest.raises(tfg._lib.TfgxError):
        tfg.nn.drop_edge([np.zeros((2, 5), np.int32)], rate=0.5, training=True)
