# coding=utf-8
"""include/tfgx_nbrstatic.h (fixed-shape minibatch sampling) without a GPU: the exact list of its names and its macros, every
refusal on the host with the argument named, the zero-size calls, static_capacities against hand-computed values, the numpy
mirror of the fixed-shape layout (the exact reference of tests/test_gpu_nbrstatic.py) against one hand-written answer, and the
Python-side refusals of RandomNeighborSampler.sample_blocks_static that need no device.  The uniform header / table / version
checks are tests/test_abi_registry.py's, through the registry entry."""
import os

import numpy as np
import pytest

from abi_header import INCLUDE, declarations, macro, refused as _refused
from test_nbrblock_abi import mirror_blocks

HEADER = "tfgx_nbrstatic.h"
NAMES = ["tfgx_nbrstatic_gather_rows_f32", "tfgx_nbrstatic_hop", "tfgx_nbrstatic_hop_workspace_bytes",
         "tfgx_nbrstatic_input_hop_f32", "tfgx_nbrstatic_seeds", "tfgx_nbrstatic_transpose",
         "tfgx_nbrstatic_transpose_workspace_bytes", "tfgx_nbrstatic_version"]


# ---- the mirror: test infrastructure shared with the GPU tests ----------------------------------------------------------
def mirror_static_blocks(m, seeds, fanouts):
    """The fixed-shape layout restated in numpy.  `m` = mirror_blocks(live seeds, hop lists): the DYNAMIC minibatch of the live
    seeds; `seeds` = the fixed-length list with -1 for a dead slot; `fanouts` = the fan-outs of m's blocks, input side first.
    Hop h over R rows at fan-out k: E = R * k edge slots and new-node slots, S = R sinks (0 when k == 0), R' = R + E + S nodes in
    the order [rows | new-node slots | sinks].  A dynamic virtual id maps to a static one in order: the live seeds to their
    positions in `seeds`, the j-th new node of a hop to R + j.  A block keeps the dynamic block's edges (mapped, same order,
    same weights) and fills its E - total tail slots with unit self-loops on the sinks, in order, at most k per sink.  Returns
    node_index int32 [R_L] (-1 = dead), counts [hops, 2] = (edges, new nodes) per hop outward, and blocks (input side first),
    each a dict of edge_index [2, E], edge_weight, num_dst, num_src and row_ptr [R' + 1]."""
    seeds = [int(s) for s in seeds]
    live_pos = [i for i, s in enumerate(seeds) if s >= 0]
    dyn = m["blocks"][::-1]                                   # hop order
    ks = [int(k) for k in fanouts][::-1]
    assert len(dyn) == len(ks) and [seeds[i] for i in live_pos] == list(m["node_index"][:len(live_pos)])
    s_of_d = list(live_pos)                                   # dynamic virtual id -> static virtual id
    R = len(seeds)
    node = [-1] * R
    for i in live_pos:
        node[i] = seeds[i]
    blocks, counts = [], []
    for b, k in zip(dyn, ks):
        E, S = R * k, (R if k > 0 else 0)
        Rn = R + E + S
        n_new = b["num_src"] - b["num_dst"]
        assert b["num_dst"] == len(s_of_d) and n_new <= E
        s_of_d = s_of_d + [R + j for j in range(n_new)]
        node = node + [-1] * (E + S)
        for d in range(b["num_dst"], b["num_src"]):
            node[s_of_d[d]] = int(m["node_index"][d])
        total = b["edge_index"].shape[1]
        assert total <= E
        row = [s_of_d[r] for r in b["edge_index"][0]]
        col = [s_of_d[c] for c in b["edge_index"][1]]
        w = [float(v) for v in b["edge_weight"]]
        for t in range(E - total):                            # the tail: self-loops on the sinks, k per sink
            v = R + E + t // k
            row.append(v)
            col.append(v)
            w.append(1.0)
        assert row == sorted(row) and len(row) == E
        row_ptr = np.concatenate([[0], np.cumsum(np.bincount(np.asarray(row, dtype=np.int64), minlength=Rn))]) if Rn else [0]
        assert k == 0 or max(np.diff(row_ptr), default=0) <= k
        blocks.append({"edge_index": np.asarray([row, col], dtype=np.int32).reshape(2, -1),
                       "edge_weight": np.asarray(w, dtype=np.float32), "num_dst": R, "num_src": Rn,
                       "row_ptr": np.asarray(row_ptr, dtype=np.int32)})
        counts.append((total, n_new))
        R = Rn
    return {"node_index": np.asarray(node, dtype=np.int32), "blocks": blocks[::-1],
            "counts": np.asarray(counts, dtype=np.int32).reshape(-1, 2)}


# ---- ABI ----------------------------------------------------------------------------------------------------------------
def test_nbrstatic_symbols_and_macros():
    from tf_geometric_amd import _lib as L
    assert sorted(declarations(HEADER)) == sorted(L.NBRSTATIC_SIGNATURES) == NAMES
    assert all(n.startswith("tfgx_nbrstatic_") for n in NAMES)
    assert macro(HEADER, "TFGX_NBRSTATIC_ABI_VERSION") == L.NBRSTATIC_ABI_VERSION == 1
    assert macro(HEADER, "TFGX_NBRSTATIC_DEAD") == L.NBRSTATIC_DEAD == -1
    assert macro(HEADER, "TFGX_NBRSTATIC_BAD_RANGE") == macro("tfgx_nbrblock.h", "TFGX_NBRBLOCK_BAD_RANGE") == L.NBRSTATIC_BAD_RANGE
    assert macro(HEADER, "TFGX_NBRSTATIC_BAD_REPEAT") == macro("tfgx_nbrblock.h", "TFGX_NBRBLOCK_BAD_REPEAT") == L.NBRSTATIC_BAD_REPEAT
    for abi in L.ABIS:
        assert abi.signatures is L.NBRSTATIC_SIGNATURES or not any("nbrstatic" in n for n in abi.signatures), abi.header
    # a header of its own: nothing was added to the headers it builds on, and no constant was registered for it
    for other in ("tfgx.h", "tfgx_nbrblock.h", "tfgx_samplereduce.h"):
        assert "nbrstatic" not in open(os.path.join(INCLUDE, other)).read()
    assert [a.constants for a in L.ABIS if a.header == HEADER] == [()]


P = [(i + 1) << 30 for i in range(16)]        # fake device pointers: never dereferenced on the host
BIG = 1 << 31
SEEDS_OK = dict(table=P[0], n_nodes=100, seeds=P[1], B=8, node=P[2], flag=P[3], stream=None)
HOP_OK = dict(row_ptr=P[0], col=P[1], w=P[2], n_nodes=100, table=P[3], node=P[4], R=8, k=5, replace=0, seed=P[5], hop=0,
              block_row_ptr=P[6], block_row=P[7], block_col=P[8], block_w=P[9], counts=P[10], workspace=P[11],
              workspace_bytes=1 << 30, stream=None)
TRANSPOSE_OK = dict(block_row=P[0], block_col=P[1], E=40, n=56, t_row_ptr=P[2], t_col=P[3], t_perm=P[4], workspace=P[5],
                    workspace_bytes=1 << 30, stream=None)
GATHER_OK = dict(x=P[0], ldx=16, idx=P[1], M=10, F=12, out=P[2], ldo=12, stream=None)
INPUT_OK = dict(row_ptr=P[0], col=P[1], w=P[2], n_nodes=100, node=P[3], n_rows=10, k=5, replace=0, seed=P[4], hop=1, x=P[5],
                ldx=16, F=12, op=1, out=P[6], ldo=12, out_count=P[7], bad_flag=P[8], stream=None)


@pytest.mark.parametrize("fn, ok, change, word", [
    ("tfgx_nbrstatic_seeds", SEEDS_OK, dict(n_nodes=-1), "negative size (n_nodes"),
    ("tfgx_nbrstatic_seeds", SEEDS_OK, dict(B=-1), "negative size (B "),
    ("tfgx_nbrstatic_seeds", SEEDS_OK, dict(B=BIG), "B = 2147483648 does not fit int32"),
    ("tfgx_nbrstatic_seeds", SEEDS_OK, dict(table=None), "table is null"),
    ("tfgx_nbrstatic_seeds", SEEDS_OK, dict(seeds=None), "seeds is null"),
    ("tfgx_nbrstatic_seeds", SEEDS_OK, dict(node=None), "node is null"),
    ("tfgx_nbrstatic_seeds", SEEDS_OK, dict(flag=None), "flag is null"),
    ("tfgx_nbrstatic_hop", HOP_OK, dict(n_nodes=-1), "negative size (n_nodes"),
    ("tfgx_nbrstatic_hop", HOP_OK, dict(R=-1), "negative size (R "),
    ("tfgx_nbrstatic_hop", HOP_OK, dict(R=BIG), "R = 2147483648 does not fit int32"),
    ("tfgx_nbrstatic_hop", HOP_OK, dict(k=-1), "k must not be negative"),
    ("tfgx_nbrstatic_hop", HOP_OK, dict(hop=-1), "hop must not be negative"),
    ("tfgx_nbrstatic_hop", HOP_OK, dict(R=1 << 28, k=7), "2415919104 nodes do not fit int32"),
    ("tfgx_nbrstatic_hop", HOP_OK, dict(row_ptr=None), "row_ptr is null"),
    ("tfgx_nbrstatic_hop", HOP_OK, dict(col=None), "col is null"),
    ("tfgx_nbrstatic_hop", HOP_OK, dict(table=None), "table is null"),
    ("tfgx_nbrstatic_hop", HOP_OK, dict(node=None), "node is null"),
    ("tfgx_nbrstatic_hop", HOP_OK, dict(seed=None), "seed is null"),
    ("tfgx_nbrstatic_hop", HOP_OK, dict(block_row_ptr=None), "block_row_ptr is null"),
    ("tfgx_nbrstatic_hop", HOP_OK, dict(block_row=None), "block_row is null"),
    ("tfgx_nbrstatic_hop", HOP_OK, dict(block_col=None), "block_col is null"),
    ("tfgx_nbrstatic_hop", HOP_OK, dict(block_w=None), "block_w is null"),
    ("tfgx_nbrstatic_hop", HOP_OK, dict(counts=None), "counts is null"),
    ("tfgx_nbrstatic_hop", HOP_OK, dict(workspace=None), "workspace is null"),
    ("tfgx_nbrstatic_transpose", TRANSPOSE_OK, dict(E=-1), "negative size (E "),
    ("tfgx_nbrstatic_transpose", TRANSPOSE_OK, dict(n=-1), "negative size (n "),
    ("tfgx_nbrstatic_transpose", TRANSPOSE_OK, dict(E=BIG), "E = 2147483648 does not fit int32"),
    ("tfgx_nbrstatic_transpose", TRANSPOSE_OK, dict(n=BIG), "n = 2147483648 does not fit int32"),
    ("tfgx_nbrstatic_transpose", TRANSPOSE_OK, dict(n=0), "edges over n = 0 nodes"),
    ("tfgx_nbrstatic_transpose", TRANSPOSE_OK, dict(block_row=None), "block_row is null"),
    ("tfgx_nbrstatic_transpose", TRANSPOSE_OK, dict(block_col=None), "block_col is null"),
    ("tfgx_nbrstatic_transpose", TRANSPOSE_OK, dict(t_row_ptr=None), "t_row_ptr is null"),
    ("tfgx_nbrstatic_transpose", TRANSPOSE_OK, dict(t_col=None), "t_col is null"),
    ("tfgx_nbrstatic_transpose", TRANSPOSE_OK, dict(t_perm=None), "t_perm is null"),
    ("tfgx_nbrstatic_transpose", TRANSPOSE_OK, dict(workspace=None), "workspace is null"),
    ("tfgx_nbrstatic_gather_rows_f32", GATHER_OK, dict(M=-1), "negative size (M "),
    ("tfgx_nbrstatic_gather_rows_f32", GATHER_OK, dict(M=BIG), "M = 2147483648 does not fit int32"),
    ("tfgx_nbrstatic_gather_rows_f32", GATHER_OK, dict(F=0), "F must be at least 1"),
    ("tfgx_nbrstatic_gather_rows_f32", GATHER_OK, dict(ldx=11), "ldx must be at least F"),
    ("tfgx_nbrstatic_gather_rows_f32", GATHER_OK, dict(ldo=11), "ldo must be at least F"),
    ("tfgx_nbrstatic_gather_rows_f32", GATHER_OK, dict(x=None), "x is null"),
    ("tfgx_nbrstatic_gather_rows_f32", GATHER_OK, dict(idx=None), "idx is null"),
    ("tfgx_nbrstatic_gather_rows_f32", GATHER_OK, dict(out=None), "out is null"),
    ("tfgx_nbrstatic_input_hop_f32", INPUT_OK, dict(n_nodes=-1), "negative size (n_nodes"),
    ("tfgx_nbrstatic_input_hop_f32", INPUT_OK, dict(n_rows=-1), "negative size (n_rows"),
    ("tfgx_nbrstatic_input_hop_f32", INPUT_OK, dict(n_rows=BIG), "n_rows = 2147483648 does not fit int32"),
    ("tfgx_nbrstatic_input_hop_f32", INPUT_OK, dict(k=-1), "k must not be negative"),
    ("tfgx_nbrstatic_input_hop_f32", INPUT_OK, dict(k="above"), "k is above TFGX_SAMPLEREDUCE_MAX_DRAWS"),
    ("tfgx_nbrstatic_input_hop_f32", INPUT_OK, dict(hop=-1), "hop must not be negative"),
    ("tfgx_nbrstatic_input_hop_f32", INPUT_OK, dict(F=0), "F must be at least 1"),
    ("tfgx_nbrstatic_input_hop_f32", INPUT_OK, dict(ldx=11), "ldx must be at least F"),
    ("tfgx_nbrstatic_input_hop_f32", INPUT_OK, dict(ldo=11), "ldo must be at least F"),
    ("tfgx_nbrstatic_input_hop_f32", INPUT_OK, dict(op=2), "op must be TFGX_SUM or TFGX_MEAN"),
    ("tfgx_nbrstatic_input_hop_f32", INPUT_OK, dict(row_ptr=None), "row_ptr is null"),
    ("tfgx_nbrstatic_input_hop_f32", INPUT_OK, dict(col=None), "col is null"),
    ("tfgx_nbrstatic_input_hop_f32", INPUT_OK, dict(node=None), "node is null"),
    ("tfgx_nbrstatic_input_hop_f32", INPUT_OK, dict(seed=None), "seed is null"),
    ("tfgx_nbrstatic_input_hop_f32", INPUT_OK, dict(x=None), "x is null"),
    ("tfgx_nbrstatic_input_hop_f32", INPUT_OK, dict(out=None), "out is null"),
    ("tfgx_nbrstatic_input_hop_f32", INPUT_OK, dict(bad_flag=None), "bad_flag is null"),
])
def test_host_side_refusals_name_the_argument(fn, ok, change, word):
    """TFGX_ERR_INVALID_ARG (1) on the host, before any device work: the pointers here are not memory."""
    if change.get("k") == "above":
        change = dict(k=macro("tfgx_samplereduce.h", "TFGX_SAMPLEREDUCE_MAX_DRAWS") + 1)
    _refused(fn, ok, change, word)


def test_small_workspaces_are_refused_with_their_own_code():
    from tf_geometric_amd import _lib as L
    lib = L.load_library()
    need = lib.tfgx_nbrstatic_hop_workspace_bytes(8, 5)
    assert need >= (9 + 40) * 4 + lib.tfgx_nbrblock_relabel_workspace_bytes(40)
    _refused("tfgx_nbrstatic_hop", HOP_OK, dict(workspace_bytes=need - 1), "workspace_bytes", code=3)       # TFGX_ERR_WORKSPACE
    assert lib.tfgx_nbrstatic_hop_workspace_bytes(0, 5) == lib.tfgx_nbrstatic_hop_workspace_bytes(8, 0) == 0
    assert lib.tfgx_nbrstatic_hop_workspace_bytes(1 << 28, 7) == 0          # a hop that is refused needs nothing
    need = lib.tfgx_nbrstatic_transpose_workspace_bytes(40, 56)
    assert need >= 2 * 40 * 4
    _refused("tfgx_nbrstatic_transpose", TRANSPOSE_OK, dict(workspace_bytes=need - 1), "workspace_bytes", code=3)
    assert lib.tfgx_nbrstatic_transpose_workspace_bytes(0, 56) == 0
    # the scratch grows with the batch alone
    assert lib.tfgx_nbrstatic_hop_workspace_bytes(12288, 25) < 6 * 4 * 12288 * 25
    assert lib.tfgx_nbrstatic_transpose_workspace_bytes(307200, 331776) < 8 * 4 * 331776


def test_zero_size_calls_succeed_and_launch_nothing():
    from tf_geometric_amd import _lib as L
    lib = L.load_library()
    assert lib.tfgx_nbrstatic_seeds(*dict(SEEDS_OK, B=0).values()) == 0, lib.tfgx_last_error()
    assert lib.tfgx_nbrstatic_seeds(*dict(SEEDS_OK, B=0, table=None, seeds=None, node=None, flag=None).values()) == 0
    nothing = {k: None for k in ("row_ptr", "col", "w", "table", "node", "seed", "block_row_ptr", "block_row", "block_col",
                                 "block_w", "counts", "workspace")}
    assert lib.tfgx_nbrstatic_hop(*dict(HOP_OK, R=0).values()) == 0
    assert lib.tfgx_nbrstatic_hop(*dict(HOP_OK, R=0, workspace_bytes=0, **nothing).values()) == 0
    _refused("tfgx_nbrstatic_hop", dict(HOP_OK, R=0), dict(k=-1), "k must not be negative")      # sizes are still checked
    assert lib.tfgx_nbrstatic_transpose(*dict(TRANSPOSE_OK, E=0, n=0).values()) == 0
    assert lib.tfgx_nbrstatic_transpose(*dict(TRANSPOSE_OK, E=0, n=0, block_row=None, block_col=None, t_row_ptr=None, t_col=None,
                                              t_perm=None, workspace=None, workspace_bytes=0).values()) == 0
    assert lib.tfgx_nbrstatic_gather_rows_f32(*dict(GATHER_OK, M=0).values()) == 0
    assert lib.tfgx_nbrstatic_gather_rows_f32(*dict(GATHER_OK, M=0, x=None, idx=None, out=None).values()) == 0
    _refused("tfgx_nbrstatic_gather_rows_f32", dict(GATHER_OK, M=0), dict(F=0), "F must be at least 1")
    nothing = {k: None for k in ("row_ptr", "col", "w", "node", "seed", "x", "out", "out_count", "bad_flag")}
    assert lib.tfgx_nbrstatic_input_hop_f32(*dict(INPUT_OK, n_rows=0).values()) == 0
    assert lib.tfgx_nbrstatic_input_hop_f32(*dict(INPUT_OK, n_rows=0, n_nodes=0, **nothing).values()) == 0


# ---- static_capacities --------------------------------------------------------------------------------------------------
def test_static_capacities_against_hand_computed_values():
    import tf_geometric_amd as tfg
    cap = tfg.utils.static_capacities(1024, [25, 10])
    # hop 1: 1024 rows * 10 = 10 240 edges and slots, 1024 sinks; hop 2: 12 288 rows * 25 = 307 200, 12 288 sinks
    assert cap.rows == [1024, 12288, 331776] and cap.edges == [10240, 307200] and cap.sinks == [1024, 12288]
    assert cap.fanouts == [10, 25]
    # a zero fan-out: no edges, no slots and NO sinks in that hop — next to the seeds, and on the input side
    cap = tfg.utils.static_capacities(8, [3, 0])
    assert cap.rows == [8, 8, 8 + 24 + 8] and cap.edges == [0, 24] and cap.sinks == [0, 8]
    cap = tfg.utils.static_capacities(8, [0, 3])
    assert cap.rows == [8, 40, 40] and cap.edges == [24, 0] and cap.sinks == [8, 0]
    assert tfg.utils.static_capacities(0, [5, 3]).rows == [0, 0, 0]
    assert tfg.utils.static_capacities(np.int64(6), [np.int64(40), 5, 2]).rows == [6, 24, 168, 7056]
    # 2^20 seeds * 52 * 52 > 2^31 - 1: the total is refused, not wrapped; the largest total below the limit is taken
    with pytest.raises(ValueError, match="more than int32 indexes"):
        tfg.utils.static_capacities(1 << 20, [50, 50])
    with pytest.raises(ValueError, match="more than int32 indexes"):
        tfg.utils.static_capacities((1 << 31) - 1, [0])
    assert tfg.utils.static_capacities((1 << 31) - 2, [0]).rows[-1] == (1 << 31) - 2
    for bad, word in (([], "non-empty"), (None, "non-empty"), ([5, -1], "negative"), ([5, 2.5], "integers"), ([5, True], "integers"),
                      ([5, None], "fan-out of None")):
        with pytest.raises(ValueError, match=word):
            tfg.utils.static_capacities(8, bad)
    with pytest.raises(ValueError, match="non-negative integer"):
        tfg.utils.static_capacities(-1, [5])


# ---- the mirror against a hand-written answer ---------------------------------------------------------------------------
def _w(cols):
    return np.asarray(cols, dtype=np.float32) * 0.5 + 1.0


def test_mirror_static_blocks_on_a_hand_written_case():
    # seeds [3, dead, 7] at fan-out 2: node 3 draws 9 and 4 (both new, in that order), node 7 draws the seed 3.
    # R = 3, E = 6, S = 3, R' = 12: rows 0..2, new-node slots 3..8 (two used), sinks 9..11.
    m = mirror_blocks([3, 7], [{3: ([9, 4], _w([9, 4])), 7: ([3], _w([3]))}])
    s = mirror_static_blocks(m, [3, -1, 7], [2])
    assert s["node_index"].tolist() == [3, -1, 7, 9, 4, -1, -1, -1, -1, -1, -1, -1]
    assert s["counts"].tolist() == [[3, 2]]
    b, = s["blocks"]
    assert (b["num_dst"], b["num_src"]) == (3, 12)
    # the three sampled edges (row 2 is the dynamic row 1; its neighbour 3 is virtual node 0), then the tail: 3 self-loops, two
    # on sink 9 and one on sink 10
    assert b["edge_index"].tolist() == [[0, 0, 2, 9, 9, 10], [3, 4, 0, 9, 9, 10]]
    assert b["edge_weight"].tolist() == [5.5, 3.0, 2.5, 1.0, 1.0, 1.0]
    assert b["row_ptr"].tolist() == [0, 2, 2, 3, 3, 3, 3, 3, 3, 3, 5, 6, 6]
    # two hops, a dead slot in front, a zero fan-out on the input side: the second block is empty and adds no nodes
    m = mirror_blocks([3, 7], [{3: ([9, 4], _w([9, 4])), 7: ([3], _w([3]))}, {}])
    s = mirror_static_blocks(m, [-1, 3, 7], [0, 2])
    assert s["node_index"].tolist() == [-1, 3, 7, 9, 4] + [-1] * 7 and s["counts"].tolist() == [[3, 2], [0, 0]]
    assert s["blocks"][0]["edge_index"].shape == (2, 0) and (s["blocks"][0]["num_dst"], s["blocks"][0]["num_src"]) == (12, 12)
    assert s["blocks"][0]["row_ptr"].tolist() == [0] * 13
    assert s["blocks"][1]["edge_index"].tolist() == [[1, 1, 2, 9, 9, 10], [3, 4, 1, 9, 9, 10]]
    # every seed dead: every edge slot is a sink self-loop
    s = mirror_static_blocks(mirror_blocks([], [{}]), [-1, -1], [2])
    assert s["node_index"].tolist() == [-1] * 8 and s["blocks"][0]["edge_index"].tolist() == [[6, 6, 7, 7], [6, 6, 7, 7]]


# ---- Python-side refusals that need no device ---------------------------------------------------------------------------
def _bare_sampler():
    """A sampler object without its graph: the checks below must all come before anything touches the device."""
    import tf_geometric_amd as tfg
    return object.__new__(tfg.utils.RandomNeighborSampler)


def test_python_refusals_before_any_device_work():
    from tf_geometric_amd import _lib as L
    s = _bare_sampler()
    with pytest.raises(ValueError, match="no form for ratio="):
        s.sample_blocks_static([0, 1], [5], ratio=0.5)
    with pytest.raises(ValueError, match="fan-out of None"):
        s.sample_blocks_static([0, 1], [5, None])
    with pytest.raises(ValueError, match="non-empty"):
        s.sample_blocks_static([0, 1], [])
    with pytest.raises(ValueError, match="negative"):
        s.sample_blocks_static([0, 1], [5, -1])
    with pytest.raises(ValueError, match="integers"):
        s.sample_blocks_static([0, 1], [5, 2.5])
    with pytest.raises(ValueError, match="seeds must be integers"):
        s.sample_blocks_static([0.0, 1.5], [5])
    with pytest.raises(ValueError, match="one-dimensional"):
        s.sample_blocks_static(np.zeros((2, 2), dtype=np.int64), [5])
    with pytest.raises(ValueError, match="composed dynamic route"):
        s.sample_blocks_static([0, 1], [L.SAMPLEREDUCE_MAX_DRAWS + 1, 5], fuse_input_hop=True)
