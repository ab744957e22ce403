# coding=utf-8
"""include/tfgx_linkpred.h (link prediction) without a GPU: the exact list of its names, of which tfgx.h knows none (the uniform
header / table / version checks are tests/test_abi_registry.py's), the host argument checks name the refused member before any device work, zero
sizes succeed, and the numpy mirror of both samplers — built ONLY on tfgx_negative_draw called from the host, used as the
exact reference by tests/test_gpu_linkpred.py — is uniform over the non-edges within the binomial's 5 sigma.  The torch-op
utilities (extract_unique_edge, the hash converters) are compared with the reference's own outputs
(tests/golden/link_cases.npz, written by tests/golden/make_link_golden.py through oracle/ref_harness); the train / test
split is compared with the reference's convert_edge_to_upper on the GPU (it runs on the merge kernel)."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from abi_header import declarations, source
from conftest import ROOT

HEADER = "tfgx_linkpred.h"
GOLDEN = os.path.join(ROOT, "tests", "golden", "link_cases.npz")

# the fixed graph of the uniformity checks: 8 nodes, 10 undirected edges -> 28 - 10 = 18 non-edges; no node is full
GRAPH8 = np.array([[0, 0, 0, 1, 1, 2, 3, 4, 5, 6],
                   [1, 2, 3, 2, 4, 5, 6, 7, 6, 7]], dtype=np.int32)
N8 = 8


def _lib():
    from tf_geometric_amd import _lib
    return _lib.load_library()


# ---- the mirror: test infrastructure shared with the GPU tests ------------------------------------------------------------
def draw(seed, slot, attempt, n):
    """tfgx_negative_draw (host-callable): the candidate (u, v) of (seed, slot, attempt)."""
    u, v = ctypes.c_int32(-9), ctypes.c_int32(-9)
    _lib().tfgx_negative_draw(seed, slot, attempt, n, ctypes.byref(u), ctypes.byref(v))
    return u.value, v.value


def upper_edge_set(ei):
    ei = np.asarray(ei).reshape(2, -1)
    return {(min(a, b), max(a, b)) for a, b in ei.T.tolist() if a != b}


def directed_edge_set(ei):
    return {(a, b) for a, b in np.asarray(ei).reshape(2, -1).T.tolist()}


def mirror_pairs(num_samples, n, edges, seed, slot_base=0, max_attempts=64, undirected=True, attempts_used=None):
    """tfgx_negative_sample_pairs: `edges` = None (no filter) or a set of pairs ((min, max) when undirected).
    Returns int32 [2, num_samples]; a slot that exhausts max_attempts holds (-1, -1)."""
    out = np.full((2, num_samples), -1, dtype=np.int32)
    for s in range(num_samples):
        if edges is None:
            out[:, s] = draw(seed, slot_base + s, 0, n)
            continue
        for t in range(max_attempts):
            u, v = draw(seed, slot_base + s, t, n)
            if u == v:
                continue
            if undirected and u > v:
                u, v = v, u
            if (u, v) in edges:
                continue
            out[:, s] = (u, v)
            if attempts_used is not None:
                attempts_used.append(t + 1)
            break
    return out


def mirror_from(start, n, edges, seed, slot_base=0, max_attempts=64, attempts_used=None):
    """tfgx_negative_sample_from: `edges` = None or the DIRECTED edge set.  int32 [len(start)], -1 = exhausted."""
    start = np.asarray(start).reshape(-1)
    out = np.full(start.shape[0], -1, dtype=np.int32)
    for s, a in enumerate(start.tolist()):
        if edges is None:
            out[s] = draw(seed, slot_base + s, 0, n)[1]
            continue
        for t in range(max_attempts):
            v = draw(seed, slot_base + s, t, n)[1]
            if v == a or (a, v) in edges:
                continue
            out[s] = v
            if attempts_used is not None:
                attempts_used.append(t + 1)
            break
    return out


def mirror_without_replacement(num_samples, n, edges, seed, slot_base=0, max_attempts=64):
    """negative_sampling(replace=False): the first num_samples DISTINCT accepted pairs of slots slot_base, slot_base + 1, ..."""
    non_edges = n * (n - 1) // 2 - len(edges)
    if num_samples > non_edges:
        raise ValueError("{} samples without replacement requested, the graph has {} non-edges".format(num_samples, non_edges))
    seen, out, slot = set(), [], slot_base
    while len(out) < num_samples:
        pair = tuple(mirror_pairs(1, n, edges, seed, slot, max_attempts)[:, 0].tolist())
        slot += 1
        assert pair[0] >= 0, "a slot exhausted its attempts"
        if pair not in seen:
            seen.add(pair)
            out.append(pair)
    return np.asarray(out, dtype=np.int32).reshape(-1, 2).T


def within_five_sigma(counts, trials, p):
    sigma = np.sqrt(trials * p * (1.0 - p))
    return np.abs(np.asarray(counts, dtype=np.float64) - trials * p).max() <= 5.0 * sigma


# ---- ABI -------------------------------------------------------------------------------------------------------------------
def test_linkpred_symbols_and_versions():
    from tf_geometric_amd import _lib as L
    assert sorted(declarations(HEADER)) == sorted(L.LINKPRED_SIGNATURES) == [
        "tfgx_edge_dot_f32", "tfgx_linkpred_version", "tfgx_negative_draw", "tfgx_negative_sample_from",
        "tfgx_negative_sample_pairs"]
    tfgx_h = source("tfgx.h")
    assert "edge_dot" not in tfgx_h and "negative_" not in tfgx_h and "linkpred" not in tfgx_h
    assert L.NEGATIVE_BAD_START == -(1 << 31)
    assert re.search(r"#define\s+TFGX_NEGATIVE_BAD_START\s+\(\(int32_t\)0x80000000\)", source(HEADER))


P = [k << 30 for k in range(1, 9)]      # distinct non-null stand-ins: a refused call never touches them


def _dot(lib, row=P[0], col=P[1], E=10, a=P[2], lda=8, n_a=5, b=P[3], ldb=8, n_b=5, F=8, out=P[4], flag=None):
    return lib.tfgx_edge_dot_f32(row, col, E, a, lda, n_a, b, ldb, n_b, F, out, flag, None)


def _pairs(lib, S=10, n=5, adj_ptr=None, adj_col=None, und=1, seed=1, base=0, att=8, o_row=P[0], o_col=P[1], n_failed=P[2]):
    return lib.tfgx_negative_sample_pairs(S, n, adj_ptr, adj_col, und, seed, base, att, o_row, o_col, n_failed, None)


def _from(lib, start=P[0], S=10, n=5, adj_ptr=None, adj_col=None, seed=1, base=0, att=8, o_col=P[1], n_failed=P[2]):
    return lib.tfgx_negative_sample_from(start, S, n, adj_ptr, adj_col, seed, base, att, o_col, n_failed, None)


def test_linkpred_argument_validation_without_gpu():
    """Every refusal returns TFGX_ERR_INVALID_ARG (1) on the host, before any device work, with the member named."""
    lib = _lib()

    def refused(rc, word):
        assert rc == 1, rc
        assert word in lib.tfgx_last_error(), (word, lib.tfgx_last_error())

    refused(_dot(lib, E=-1), b"negative size")
    refused(_dot(lib, n_a=-1), b"negative size")
    refused(_dot(lib, n_b=-2), b"negative size")
    refused(_dot(lib, F=-1), b"negative size")
    refused(_dot(lib, n_a=1 << 31), b"fit int32")
    refused(_dot(lib, lda=7), b"lda")
    refused(_dot(lib, ldb=4), b"ldb")
    refused(_dot(lib, row=None), b"row is null")
    refused(_dot(lib, col=None), b"col is null")
    refused(_dot(lib, out=None), b"out is null")
    refused(_dot(lib, a=None), b"a is null")
    refused(_dot(lib, b=None), b"b is null")
    for fn in (lambda **kw: _pairs(lib, **kw), lambda **kw: _from(lib, **kw)):
        refused(fn(S=-1), b"num_samples")
        refused(fn(n=0), b"num_nodes")
        refused(fn(n=-3), b"num_nodes")
        refused(fn(n=1 << 31), b"num_nodes")
        refused(fn(att=0), b"max_attempts")
        refused(fn(att=-5), b"max_attempts")
        refused(fn(n_failed=None), b"n_failed is null")
        refused(fn(o_col=None), b"out_col is null")
        refused(fn(adj_ptr=P[5]), b"adj_col is null")
        refused(fn(adj_col=P[5]), b"adj_ptr is null")
    refused(_pairs(lib, o_row=None), b"out_row is null")
    refused(_pairs(lib, und=2), b"undirected")
    refused(_from(lib, start=None), b"start is null")


def test_linkpred_zero_sizes_succeed_without_gpu():
    lib = _lib()
    assert _dot(lib, E=0, row=None, col=None, a=None, b=None, out=None) == 0
    assert _dot(lib, E=0, F=0, lda=0, ldb=0, n_a=0, n_b=0) == 0
    assert _pairs(lib, S=0, o_row=None, o_col=None) == 0
    assert _from(lib, S=0, start=None, o_col=None) == 0


def test_negative_draw_is_a_pure_function_in_range():
    assert draw(7, 11, 3, 1000) == draw(7, 11, 3, 1000)
    seen = {draw(7, s, t, 1 << 20) for s in range(50) for t in range(4)}
    assert len(seen) == 200                                        # slots and attempts give different candidates
    assert draw(7, 11 + (1 << 32), 3, 1 << 20) != draw(7, 11, 3, 1 << 20)      # the high half of the slot counts
    assert draw(8, 11, 3, 1 << 20) != draw(7, 11, 3, 1 << 20)
    assert draw(7 + (1 << 32), 11, 3, 1 << 20) != draw(7, 11, 3, 1 << 20)
    for n in (1, 2, 3, 1000, (1 << 31) - 1):
        pairs = np.array([draw(3, s, 0, n) for s in range(300)])
        assert pairs.min() >= 0 and pairs.max() < n
    big = np.array([draw(3, s, 0, (1 << 31) - 1) for s in range(300)])
    assert big.max() > (1 << 30)                                   # the whole range is reached
    assert draw(3, 0, 0, 0) == (-1, -1) and draw(3, 0, 0, 1 << 31) == (-1, -1) and draw(3, 0, 1 << 31, 5) == (-1, -1)


# ---- uniformity of the mirror (the GPU tests show the kernels equal it bit for bit) -----------------------------------------
def test_pairs_mirror_is_uniform_over_the_non_edges():
    edges = upper_edge_set(GRAPH8)
    assert len(edges) == 10
    non_edges = sorted({(a, b) for a in range(N8) for b in range(a + 1, N8)} - edges)
    assert len(non_edges) == 18
    trials, used = 36000, []
    out = mirror_pairs(trials, N8, edges, seed=2024, attempts_used=used)
    # P(reject) = 18/64 + 1/8 (an edge in either orientation, or a self-pair): 64 attempts fail with probability < 1e-22
    assert len(used) == trials and max(used) <= 64
    assert (out[0] < out[1]).all() and out.min() >= 0 and out.max() < N8
    got = set(map(tuple, out.T.tolist()))
    assert not got & edges
    counts = [int(((out[0] == a) & (out[1] == b)).sum()) for a, b in non_edges]
    assert sum(counts) == trials
    assert within_five_sigma(counts, trials, 1.0 / 18.0), counts


def test_start_node_mirror_is_uniform_over_each_nodes_non_neighbours():
    both = np.concatenate([GRAPH8, GRAPH8[::-1]], axis=1)
    edges = directed_edge_set(both)
    start = np.arange(36000, dtype=np.int32) % N8
    used = []
    out = mirror_from(start, N8, edges, seed=99, attempts_used=used)
    assert len(used) == start.shape[0] and max(used) <= 64
    for a in range(N8):
        allowed = [v for v in range(N8) if v != a and (a, v) not in edges]
        mine = out[start == a]
        assert set(mine.tolist()) <= set(allowed)
        counts = [int((mine == v).sum()) for v in allowed]
        assert within_five_sigma(counts, mine.shape[0], 1.0 / len(allowed)), (a, counts)


def test_unfiltered_mirror_returns_attempt_zero():
    out = mirror_pairs(500, N8, None, seed=5, slot_base=1000)
    assert out.tolist() == np.array([draw(5, 1000 + s, 0, N8) for s in range(500)]).T.tolist()
    assert (out[0] == out[1]).any()                                # self-pairs are not filtered (np.random.randint)
    ends = mirror_from(np.zeros(500, np.int32), N8, None, seed=5, slot_base=1000)
    assert ends.tolist() == out[1].tolist()


def test_without_replacement_mirror():
    edges = upper_edge_set(GRAPH8)
    non_edges = {(a, b) for a in range(N8) for b in range(a + 1, N8)} - edges
    some = mirror_without_replacement(10, N8, edges, seed=4)
    assert some.shape == (2, 10) and len(set(map(tuple, some.T.tolist()))) == 10
    every = mirror_without_replacement(18, N8, edges, seed=4)
    assert set(map(tuple, every.T.tolist())) == non_edges and every.shape == (2, 18)
    assert every[:, :10].tolist() == some.tolist()                 # a prefix: the slot stream is the same
    with pytest.raises(ValueError):
        mirror_without_replacement(19, N8, edges, seed=4)


# ---- the torch-op utilities against the reference's outputs --------------------------------------------------------------
@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


@pytest.mark.parametrize("case", ["mixed", "empty"])
@pytest.mark.parametrize("kind", ["numpy", "torch"])
def test_unique_and_hash_utilities_match_the_reference(golden, case, kind):
    import tf_geometric_amd as tfg
    g = lambda k: golden["{}::{}".format(case, k)]                 # noqa: E731
    wrap = (lambda v: v) if kind == "numpy" else torch.from_numpy
    back = (lambda v: v) if kind == "numpy" else (lambda v: v.numpy())
    ei, w, n = g("edge_index"), g("edge_weight"), int(g("num_nodes"))
    for mode in ("undirected", "directed"):
        u_ei, u_w = tfg.utils.extract_unique_edge(wrap(ei), wrap(w), mode=mode)
        assert isinstance(u_ei, np.ndarray if kind == "numpy" else torch.Tensor)
        assert back(u_ei).dtype == np.int32
        assert back(u_ei).tolist() == g("unique_{}_index".format(mode)).tolist()
        assert back(u_w).tolist() == g("unique_{}_weight".format(mode)).tolist()
    assert tfg.utils.extract_unique_edge(wrap(ei))[1] is None
    edge_hash, n_out = tfg.utils.convert_edge_index_to_edge_hash(wrap(ei), n)
    assert back(edge_hash).dtype == np.int64 and back(edge_hash).tolist() == g("hash").tolist()
    assert int(n_out) == int(g("hash_num_nodes"))
    index = tfg.utils.convert_edge_hash_to_edge_index(edge_hash, n)
    assert back(index).dtype == np.int32 and back(index).tolist() == g("hash_to_index").tolist()
    if case == "mixed":
        edge_hash, n_out = tfg.utils.convert_edge_index_to_edge_hash(wrap(ei))
        assert back(edge_hash).tolist() == g("hash_inferred").tolist() and int(n_out) == int(g("hash_inferred_num_nodes"))


def test_split_sizes_follow_sklearn():
    from tf_geometric_amd.utils.link import _split_sizes
    assert _split_sizes(0.25, 35) == (26, 9)                       # ceil(8.75) = 9
    assert _split_sizes(0.2, 10) == (8, 2)
    assert _split_sizes(3, 35) == (32, 3)
    for bad in (0.0, 1.0, 1.5, -0.1, 0, 35, 40, "half", None, True):
        with pytest.raises(ValueError):
            _split_sizes(bad, 35)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["numpy", "torch"])
def test_edge_train_test_split_against_the_reference_upper_edges(tfg, golden, kind):
    ei, w = golden["mixed::edge_index"], golden["mixed::edge_weight"]
    ref = {(int(a), int(b)): float(x) for (a, b), x in zip(golden["mixed::upper_index"].T, golden["mixed::upper_weight"])}
    U = len(ref)
    wrap = (lambda v: v) if kind == "numpy" else (lambda v: torch.from_numpy(v).cuda())
    back = (lambda v: v) if kind == "numpy" else (lambda v: v.cpu().numpy())
    for test_size, n_test in ((0.25, int(np.ceil(0.25 * U))), (4, 4)):
        tr, te, tr_w, te_w = tfg.utils.edge_train_test_split(wrap(ei), test_size, wrap(w), seed=7)
        assert isinstance(tr, np.ndarray if kind == "numpy" else torch.Tensor) and type(tr_w) is type(tr)
        tr, te, tr_w, te_w = back(tr), back(te), back(tr_w), back(te_w)
        assert te.shape == (2, n_test) and tr.shape == (2, U - n_test) and tr.dtype == np.int32
        train, test = set(map(tuple, tr.T.tolist())), set(map(tuple, te.T.tolist()))
        assert len(train) == tr.shape[1] and len(test) == te.shape[1] and not train & test
        assert train | test == set(ref)
        for idx, wt in ((tr, tr_w), (te, te_w)):                   # weights travel with their edges ("max" of the duplicates)
            assert [ref[tuple(e)] for e in idx.T.tolist()] == wt.tolist()
        again = tfg.utils.edge_train_test_split(wrap(ei), test_size, wrap(w), seed=7)
        assert back(again[1]).tolist() == te.tolist()              # a seed reproduces the call
        other = tfg.utils.edge_train_test_split(wrap(ei), test_size, wrap(w), seed=8)
        assert back(other[0]).tolist() != tr.tolist()
    tr, te, tr_w, te_w = tfg.utils.edge_train_test_split(wrap(ei), 0.5, seed=1)
    assert tr_w is None and te_w is None
    with pytest.warns(UserWarning, match="num_nodes"):
        tfg.utils.edge_train_test_split(wrap(ei), 0.5, seed=1, num_nodes=12)
    with pytest.raises(NotImplementedError):
        tfg.utils.edge_train_test_split(wrap(ei), 0.5, mode="directed")


# ---- no GPU: the package's usual error -------------------------------------------------------------------------------------
@pytest.mark.skipif(torch.cuda.is_available(), reason="checks the error raised on a machine without a GPU")
def test_link_entry_points_raise_the_no_device_error_without_gpu():
    import tf_geometric_amd as tfg
    from tf_geometric_amd._lib import TfgxError
    z = np.zeros((4, 8), np.float32)
    ei = np.array([[0, 1], [1, 2]], np.int32)
    for call in (lambda: tfg.nn.edge_dot(z, ei),
                 lambda: tfg.nn.edge_dot(torch.zeros(4, 8, requires_grad=True), torch.from_numpy(ei)),
                 lambda: tfg.utils.negative_sampling(4, 4, ei),
                 lambda: tfg.utils.negative_sampling(4, 4),
                 lambda: tfg.utils.negative_sampling_with_start_node(ei[0], 4, ei),
                 lambda: tfg.utils.edge_train_test_split(ei, 0.5)):
        with pytest.raises(TfgxError, match="needs an AMD GPU"):
            call()
