# coding=utf-8
"""include/tfgx_nbrblock.h (minibatch neighbour sampling) without a GPU: the exact list of its names, which no other header's
table and not tfgx.h know (the uniform header / table / version checks are tests/test_abi_registry.py's), every refusal happens on the host with the
argument named, the zero-size calls succeed; the numpy mirror of the relabel and block assembly (the exact reference of
tests/test_gpu_nbrblock.py) is held to np.unique(..., return_index=True) on hand-written cases; and the Python-side refusals of
RandomNeighborSampler.sample_rows / sample_blocks that need no device."""
import os

import numpy as np
import pytest

from abi_header import INCLUDE, declarations, macro, refused as _refused

HEADER = "tfgx_nbrblock.h"
NAMES = ["tfgx_nbrblock_relabel", "tfgx_nbrblock_relabel_workspace_bytes", "tfgx_nbrblock_reset", "tfgx_nbrblock_sample_rows",
         "tfgx_nbrblock_stamp", "tfgx_nbrblock_version"]


# ---- the mirror: test infrastructure shared with the GPU tests ----------------------------------------------------------
def mirror_blocks(seeds, hop_lists):
    """numpy restatement of sample_blocks' relabel and block assembly.  hop_lists[h] maps a GLOBAL node id to the
    (neighbour ids, weights) sampled for it in hop h (h = 0 next to the seeds; a node that is missing has none).  Returns
    node_index int32 and blocks (input side first), each a dict of edge_index [2, E] = [row position; virtual id], edge_weight,
    num_dst, num_src and the CSR (row_ptr, col) of that list."""
    node_index = [int(s) for s in seeds]
    virtual = {g: i for i, g in enumerate(node_index)}
    assert len(virtual) == len(node_index), "seeds repeat"
    blocks = []
    for lists in hop_lists:
        n_dst = len(node_index)
        rows, vcol, ws, row_ptr = [], [], [], [0]
        for i in range(n_dst):
            cols, w = lists.get(node_index[i], ((), ()))
            for c, wc in zip(cols, w):
                c = int(c)
                if c not in virtual:                      # first occurrence: the next virtual id
                    virtual[c] = len(node_index)
                    node_index.append(c)
                rows.append(i)
                vcol.append(virtual[c])
                ws.append(wc)
            row_ptr.append(len(vcol))
        blocks.append({"edge_index": np.asarray([rows, vcol], dtype=np.int32).reshape(2, -1),
                       "edge_weight": np.asarray(ws, dtype=np.float32), "num_dst": n_dst, "num_src": len(node_index),
                       "row_ptr": np.asarray(row_ptr, dtype=np.int32), "col": np.asarray(vcol, dtype=np.int32)})
    return {"node_index": np.asarray(node_index, dtype=np.int32), "blocks": blocks[::-1]}


def lists_of(edge_index, edge_weight):
    """{node: (neighbour ids, weights)} of a sampled list whose edge_index[0] holds GLOBAL row ids (what sample() returns)."""
    out = {}
    if edge_index is None:
        return out
    ei, ew = np.asarray(edge_index), np.asarray(edge_weight)
    for r in np.unique(ei[0]):
        sel = ei[0] == r
        out[int(r)] = (ei[1][sel], ew[sel])
    return out


# ---- ABI ----------------------------------------------------------------------------------------------------------------
def test_nbrblock_symbols_and_versions():
    from tf_geometric_amd import _lib as L
    assert sorted(declarations(HEADER)) == sorted(L.NBRBLOCK_SIGNATURES) == NAMES
    assert all(n.startswith("tfgx_nbrblock_") for n in NAMES)
    assert macro(HEADER, "TFGX_NBRBLOCK_EMPTY") == L.NBRBLOCK_EMPTY == 2 ** 31 - 1
    assert macro(HEADER, "TFGX_NBRBLOCK_BAD_RANGE") == L.NBRBLOCK_BAD_RANGE
    assert macro(HEADER, "TFGX_NBRBLOCK_BAD_REPEAT") == L.NBRBLOCK_BAD_REPEAT
    for abi in L.ABIS:
        assert abi.signatures is L.NBRBLOCK_SIGNATURES or not any("nbrblock" in n for n in abi.signatures), abi.header
    assert "nbrblock" not in open(os.path.join(INCLUDE, "tfgx.h")).read()          # not even in a comment


P = [(i + 1) << 30 for i in range(12)]        # fake device pointers: never dereferenced on the host
SAMPLE_OK = dict(row_ptr=P[0], col=P[1], w=P[2], n_nodes=100, rows=P[3], n_rows=10, out_ptr=P[4], replace=0, seed=7,
                 out_col=P[5], out_w=P[6], bad_flag=P[7], stream=None)
STAMP_OK = dict(table=P[0], n_nodes=100, ids=P[1], n=10, base=0, flag=P[2], stream=None)
RELABEL_OK = dict(table=P[0], n_nodes=100, n_known=10, cols=P[1], E=50, out_vcol=P[2], node_list=P[3], n_new=P[4],
                  workspace=P[5], workspace_bytes=1 << 30, stream=None)
RESET_OK = dict(table=P[0], n_nodes=100, node_list=P[1], n=10, stream=None)
BIG = 1 << 31


@pytest.mark.parametrize("fn, ok, change, word", [
    ("tfgx_nbrblock_sample_rows", SAMPLE_OK, dict(n_nodes=-1), "negative size (n_nodes"),
    ("tfgx_nbrblock_sample_rows", SAMPLE_OK, dict(n_rows=-1), "negative size (n_rows"),
    ("tfgx_nbrblock_sample_rows", SAMPLE_OK, dict(n_nodes=BIG), "n_nodes = 2147483648 does not fit int32"),
    ("tfgx_nbrblock_sample_rows", SAMPLE_OK, dict(n_rows=BIG), "n_rows = 2147483648 does not fit int32"),
    ("tfgx_nbrblock_sample_rows", SAMPLE_OK, dict(row_ptr=None), "row_ptr is null"),
    ("tfgx_nbrblock_sample_rows", SAMPLE_OK, dict(col=None), "col is null"),
    ("tfgx_nbrblock_sample_rows", SAMPLE_OK, dict(rows=None), "rows is null"),
    ("tfgx_nbrblock_sample_rows", SAMPLE_OK, dict(out_ptr=None), "out_ptr is null"),
    ("tfgx_nbrblock_sample_rows", SAMPLE_OK, dict(out_col=None), "out_col is null"),
    ("tfgx_nbrblock_sample_rows", SAMPLE_OK, dict(bad_flag=None), "bad_flag is null"),
    ("tfgx_nbrblock_stamp", STAMP_OK, dict(n_nodes=-1), "negative size (n_nodes"),
    ("tfgx_nbrblock_stamp", STAMP_OK, dict(n=-1), "negative size (n "),
    ("tfgx_nbrblock_stamp", STAMP_OK, dict(base=-1), "negative size (base"),
    ("tfgx_nbrblock_stamp", STAMP_OK, dict(n=BIG), "n = 2147483648 does not fit int32"),
    ("tfgx_nbrblock_stamp", STAMP_OK, dict(base=BIG - 5, n=10), "base + n = 2147483653 does not fit int32"),
    ("tfgx_nbrblock_stamp", STAMP_OK, dict(table=None), "table is null"),
    ("tfgx_nbrblock_stamp", STAMP_OK, dict(ids=None), "ids is null"),
    ("tfgx_nbrblock_stamp", STAMP_OK, dict(flag=None), "flag is null"),
    ("tfgx_nbrblock_relabel", RELABEL_OK, dict(n_nodes=-1), "negative size (n_nodes"),
    ("tfgx_nbrblock_relabel", RELABEL_OK, dict(n_known=-1), "negative size (n_known"),
    ("tfgx_nbrblock_relabel", RELABEL_OK, dict(E=-1), "negative size (E "),
    ("tfgx_nbrblock_relabel", RELABEL_OK, dict(E=BIG), "E = 2147483648 does not fit int32"),
    ("tfgx_nbrblock_relabel", RELABEL_OK, dict(n_known=BIG - 40), "n_known + E = 2147483658 does not fit int32"),
    ("tfgx_nbrblock_relabel", RELABEL_OK, dict(table=None), "table is null"),
    ("tfgx_nbrblock_relabel", RELABEL_OK, dict(cols=None), "cols is null"),
    ("tfgx_nbrblock_relabel", RELABEL_OK, dict(out_vcol=None), "out_vcol is null"),
    ("tfgx_nbrblock_relabel", RELABEL_OK, dict(node_list=None), "node_list is null"),
    ("tfgx_nbrblock_relabel", RELABEL_OK, dict(n_new=None), "n_new is null"),
    ("tfgx_nbrblock_relabel", RELABEL_OK, dict(workspace=None), "workspace is null"),
    ("tfgx_nbrblock_reset", RESET_OK, dict(n_nodes=-1), "negative size (n_nodes"),
    ("tfgx_nbrblock_reset", RESET_OK, dict(n=-1), "negative size (n "),
    ("tfgx_nbrblock_reset", RESET_OK, dict(n=BIG), "n = 2147483648 does not fit int32"),
    ("tfgx_nbrblock_reset", RESET_OK, dict(table=None), "table is null"),
    ("tfgx_nbrblock_reset", RESET_OK, dict(node_list=None), "node_list is null"),
])
def test_host_side_refusals_name_the_argument(fn, ok, change, word):
    """TFGX_ERR_INVALID_ARG (1) on the host, before any device work: the pointers here are not memory."""
    _refused(fn, ok, change, word)


def test_a_small_workspace_is_refused_with_its_own_code():
    from tf_geometric_amd import _lib as L
    lib = L.load_library()
    need = lib.tfgx_nbrblock_relabel_workspace_bytes(50)
    assert need >= 2 * 50 * 4
    _refused("tfgx_nbrblock_relabel", RELABEL_OK, dict(workspace_bytes=need - 1), "workspace_bytes", code=3)   # TFGX_ERR_WORKSPACE
    assert lib.tfgx_nbrblock_relabel_workspace_bytes(0) == 0
    # the scratch grows with the batch alone: two int32 arrays and a scan's block partials
    assert lib.tfgx_nbrblock_relabel_workspace_bytes(1 << 20) < 3 * 4 * (1 << 20)


def test_zero_size_calls_succeed_and_launch_nothing():
    from tf_geometric_amd import _lib as L
    lib = L.load_library()
    nothing = {k: None for k in ("row_ptr", "col", "w", "rows", "out_ptr", "out_col", "out_w", "bad_flag")}
    assert lib.tfgx_nbrblock_sample_rows(*dict(SAMPLE_OK, n_rows=0).values()) == 0, lib.tfgx_last_error()
    assert lib.tfgx_nbrblock_sample_rows(*dict(SAMPLE_OK, n_rows=0, n_nodes=0, **nothing).values()) == 0
    assert lib.tfgx_nbrblock_stamp(*dict(STAMP_OK, n=0).values()) == 0
    assert lib.tfgx_nbrblock_stamp(*dict(STAMP_OK, n=0, table=None, ids=None, flag=None).values()) == 0
    assert lib.tfgx_nbrblock_relabel(*dict(RELABEL_OK, E=0).values()) == 0
    assert lib.tfgx_nbrblock_relabel(*dict(RELABEL_OK, E=0, table=None, cols=None, out_vcol=None, node_list=None, n_new=None,
                                           workspace=None, workspace_bytes=0).values()) == 0
    assert lib.tfgx_nbrblock_reset(*dict(RESET_OK, n=0).values()) == 0
    assert lib.tfgx_nbrblock_reset(*dict(RESET_OK, n=0, table=None, node_list=None).values()) == 0


# ---- the mirror against np.unique ---------------------------------------------------------------------------------------
def _w(cols):
    return np.asarray(cols, dtype=np.float32) * 0.5 + 1.0


def _check_against_unique(seeds, hop_lists):
    """node_index is the seeds followed, hop by hop, by the ids not seen before in order of their first occurrence — np.unique's
    return_index gives that order without any dictionary — and every virtual id points back at its global id."""
    m = mirror_blocks(seeds, hop_lists)
    known = list(seeds)
    blocks = m["blocks"][::-1]
    assert len(blocks) == len(hop_lists)
    for lists, b in zip(hop_lists, blocks):
        flat = np.concatenate([np.asarray(lists.get(g, ((), ()))[0], dtype=np.int64) for g in known] + [np.zeros(0, np.int64)])
        ws = np.concatenate([np.asarray(lists.get(g, ((), ()))[1], dtype=np.float32) for g in known] + [np.zeros(0, np.float32)])
        cnt = [len(lists.get(g, ((), ()))[0]) for g in known]
        fresh = flat[~np.isin(flat, known)]
        u, first = np.unique(fresh, return_index=True)
        appended = list(u[np.argsort(first)])
        assert b["num_dst"] == len(known)
        known = known + [int(a) for a in appended]
        assert b["num_src"] == len(known)
        assert np.array_equal(np.asarray(known)[b["edge_index"][1]], flat)
        assert np.array_equal(b["edge_index"][0], np.repeat(np.arange(b["num_dst"]), cnt))
        assert np.array_equal(b["row_ptr"], np.concatenate([[0], np.cumsum(cnt)])) and np.array_equal(b["col"], b["edge_index"][1])
        assert np.array_equal(b["edge_weight"], ws) and b["edge_weight"].dtype == np.float32
        assert b["edge_index"].dtype == np.int32 and b["edge_index"].shape == (2, len(flat))
    assert np.array_equal(m["node_index"], known) and m["node_index"].dtype == np.int32
    assert len(set(known)) == len(known)
    return m


def test_mirror_blocks_on_hand_written_cases():
    # a neighbour that is a seed (7 -> 3), a new neighbour seen twice (9), first-occurrence order 9, 4 (not sorted)
    m = _check_against_unique([3, 7], [{3: ([9, 4], _w([9, 4])), 7: ([3, 9], _w([3, 9]))}])
    assert list(m["node_index"]) == [3, 7, 9, 4]
    assert m["blocks"][0]["edge_index"].tolist() == [[0, 0, 1, 1], [2, 3, 0, 2]]
    # two hops: in hop 2 node 9 samples 4 (seen in hop 1), 3 (a seed) and 11 (new); rows of hop 2 are all four known nodes
    hop1 = {3: ([9, 4], _w([9, 4])), 7: ([3, 9], _w([3, 9]))}
    hop2 = {3: ([7], _w([7])), 9: ([4, 3, 11], _w([4, 3, 11])), 4: ([11, 20], _w([11, 20]))}
    m = _check_against_unique([3, 7], [hop1, hop2])
    assert list(m["node_index"]) == [3, 7, 9, 4, 11, 20]
    assert m["blocks"][0]["num_dst"] == 4 and m["blocks"][0]["num_src"] == 6        # blocks[0]: the outer hop, input side
    assert m["blocks"][1]["num_dst"] == 2 and m["blocks"][1]["num_src"] == 4
    assert m["blocks"][0]["edge_index"].tolist() == [[0, 2, 2, 2, 3, 3], [1, 3, 0, 4, 4, 5]]
    # a repeated neighbour inside one row (padding draws with replacement): one virtual id, every occurrence kept
    m = _check_against_unique([5], [{5: ([8, 8, 2, 8], _w([8, 8, 2, 8]))}])
    assert list(m["node_index"]) == [5, 8, 2] and m["blocks"][0]["edge_index"][1].tolist() == [1, 1, 2, 1]
    # an empty hop in the middle and at the end; a self-loop
    m = _check_against_unique([1, 2], [{}, {1: ([1, 6], _w([1, 6]))}, {}])
    assert list(m["node_index"]) == [1, 2, 6]
    assert [b["edge_index"].shape[1] for b in m["blocks"]] == [0, 2, 0]
    assert [(b["num_dst"], b["num_src"]) for b in m["blocks"]] == [(3, 3), (2, 3), (2, 2)]
    # no seeds at all
    m = _check_against_unique([], [{4: ([1], _w([1]))}])
    assert m["node_index"].shape == (0,) and m["blocks"][0]["row_ptr"].tolist() == [0]


def test_lists_of_splits_a_sampled_list_by_row():
    ei = np.asarray([[0, 0, 2, 5, 5, 5], [4, 1, 2, 9, 9, 0]], dtype=np.int32)
    ew = np.arange(6, dtype=np.float32)
    got = lists_of(ei, ew)
    assert sorted(got) == [0, 2, 5]
    assert got[5][0].tolist() == [9, 9, 0] and got[5][1].tolist() == [3.0, 4.0, 5.0] and got[0][0].tolist() == [4, 1]
    assert lists_of(None, None) == {}


# ---- Python-side refusals that need no device ---------------------------------------------------------------------------
def _bare_sampler():
    """A sampler object without its graph: the checks below must all come before anything touches the device."""
    import tf_geometric_amd as tfg
    return object.__new__(tfg.utils.RandomNeighborSampler)


def test_python_refusals_before_any_device_work():
    s = _bare_sampler()
    with pytest.raises(Exception, match="k and ratio cannot be provided simultaneously"):
        s.sample_rows([0, 1], k=3, ratio=0.5)
    with pytest.raises(ValueError, match="non-empty"):
        s.sample_blocks([0, 1], [])
    with pytest.raises(ValueError, match="non-empty"):
        s.sample_blocks([0, 1], None)
    with pytest.raises(ValueError, match="negative"):
        s.sample_blocks([0, 1], [5, -1])
    with pytest.raises(ValueError, match="integers"):
        s.sample_blocks([0, 1], [5, 2.5])
    with pytest.raises(ValueError, match="seeds must be integers"):
        s.sample_blocks([0.0, 1.5], [5])
    with pytest.raises(ValueError, match="seeds must be integers"):
        s.sample_blocks(np.asarray([0.0, 1.0]), [5])
    with pytest.raises(ValueError, match="rows must be integers"):
        s.sample_rows(np.asarray([0.5]), k=2)
    with pytest.raises(ValueError, match="one-dimensional"):
        s.sample_blocks(np.zeros((2, 2), dtype=np.int64), [5])


def test_hop_seeds_formula():
    import tf_geometric_amd as tfg
    seed = 123456789
    for h in range(4):
        v = tfg.utils.hop_seed(seed, h)
        assert v == (seed + (h + 1) * 0x9E3779B97F4A7C15) % (1 << 63) and 0 <= v < 1 << 63
    assert len({tfg.utils.hop_seed(seed, h) for h in range(8)}) == 8


def test_sampling_needs_a_gpu():
    import torch
    import tf_geometric_amd as tfg
    if torch.cuda.is_available():
        pytest.skip("a GPU is present: the refusal cannot be observed")
    s = _bare_sampler()
    with pytest.raises(tfg._lib.TfgxError):
        s.sample_rows([0, 1], k=2)
    with pytest.raises(tfg._lib.TfgxError):
        s.sample_blocks([0, 1], [5, 3])
    mb = tfg.utils.SampledMinibatch([], None, 0, [])
    with pytest.raises(tfg._lib.TfgxError):
        mb.gather(np.zeros((4, 3), dtype=np.float32))
