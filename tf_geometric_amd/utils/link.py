# coding=utf-8
"""Link-prediction utilities — tf_geometric/utils/graph_utils.py:14-64 (edge hashes), :369-412 (negative_sampling),
:415-452 (negative_sampling_with_start_node), :455-485 (extract_unique_edge), :488-535 (edge_train_test_split).

The samplers are rejection samplers on the device (include/tfgx_linkpred.h): slot s tries attempts 0, 1, ... of
tfgx_negative_draw(seed, slot, attempt, num_nodes) and keeps the first candidate that is neither a self-pair nor in a
sorted adjacency, which the host builds once per edge_index (torch sort + unique) and memoises on the tensor.  The
reference builds a dense [N, N] float64 matrix (undirected form) or loops in Python per sample (start-node form).
A call is reproduced by its seed; the random stream is this library's, not numpy's."""
import math
import warnings

import numpy as np
import torch

from .. import _lib as L

MAX_ATTEMPTS = 64               # per slot; a slot that exhausts them sends the call to the dense construction (or raises)
DENSE_FALLBACK_MAX_NODES = 4096     # the reference's [N, N] construction is only run up to this size (16 M bools)
BATCH_SLOT_STRIDE = 1 << 40     # batch b draws from slots [b << 40, (b + 1) << 40): disjoint windows
STATS = {"rounds": 0, "dense_fallback": 0, "launches": 0}      # diagnostics (tests assert the route taken)


def _seed_from_torch():
    hi, lo = torch.randint(0, 1 << 32, (2,), dtype=torch.int64).tolist()
    return (hi << 32) | lo


def _u64(v):
    return int(v) & 0xFFFFFFFFFFFFFFFF


def _to_long_tensor(x):
    """numpy / list / torch -> int64 tensor on the device the input lives on (CPU for host data): plain torch plumbing."""
    if isinstance(x, torch.Tensor):
        return x.detach().to(torch.int64)
    return torch.from_numpy(np.ascontiguousarray(np.asarray(x)).astype(np.int64))


# ---- edge hashes and first-occurrence unique (torch ops, on whichever device the input is) --------------------------------

def convert_edge_index_to_edge_hash(edge_index, num_nodes=None):
    """(num_nodes * row + col as int64, num_nodes); num_nodes=None -> max(edge_index) + 1 (reference :14-43)."""
    as_np = not isinstance(edge_index, torch.Tensor)
    ei = _to_long_tensor(edge_index).reshape(2, -1)
    if num_nodes is None:
        n = ei.max() + 1                 # (an empty edge_index has no maximum: an error, as in the reference)
    else:
        n = num_nodes.to(device=ei.device, dtype=torch.int64) if isinstance(num_nodes, torch.Tensor) else int(num_nodes)
    edge_hash = n * ei[0] + ei[1]
    if as_np:
        edge_hash = edge_hash.cpu().numpy()
    if num_nodes is None:
        n = np.int64(n.item()) if as_np else n
    elif not isinstance(num_nodes, torch.Tensor):
        n = np.int64(n)
    else:
        n = num_nodes
    return edge_hash, n


def convert_edge_hash_to_edge_index(edge_hash, num_nodes):
    """int32 [2, E]: (hash // num_nodes, hash % num_nodes) (reference :46-64)."""
    as_np = not isinstance(edge_hash, torch.Tensor)
    h = _to_long_tensor(edge_hash).reshape(-1)
    n = num_nodes.to(device=h.device, dtype=torch.int64) if isinstance(num_nodes, torch.Tensor) else int(num_nodes)
    ei = torch.stack([torch.div(h, n, rounding_mode="floor"), torch.remainder(h, n)]).to(torch.int32)
    return ei.cpu().numpy() if as_np else ei


def extract_unique_edge(edge_index, edge_weight=None, mode="undirected"):
    """Edges at their FIRST occurrence, in input order; mode="undirected" treats (u, v) and (v, u) as one edge and keeps
    the orientation that came first (reference :455-485).  Weights travel with the kept edges."""
    as_np = not isinstance(edge_index, torch.Tensor)
    ei = _to_long_tensor(edge_index).reshape(2, -1)
    E = int(ei.shape[1])
    if E == 0:
        first = torch.zeros(0, dtype=torch.int64, device=ei.device)
    else:
        a, b = (torch.minimum(ei[0], ei[1]), torch.maximum(ei[0], ei[1])) if mode == "undirected" else (ei[0], ei[1])
        lo = torch.minimum(a.min(), b.min())
        key = (a - lo) * (b.max() - lo + 1) + (b - lo)
        uniq, inverse = torch.unique(key, return_inverse=True)
        first = torch.full((int(uniq.shape[0]),), E, dtype=torch.int64, device=ei.device)
        first.scatter_reduce_(0, inverse, torch.arange(E, dtype=torch.int64, device=ei.device), reduce="amin")
        first = torch.sort(first).values
    out = ei[:, first].to(torch.int32)
    w = edge_weight
    if edge_weight is not None:
        if isinstance(edge_weight, torch.Tensor):
            w = edge_weight[first.to(edge_weight.device)]
        else:
            w = np.asarray(edge_weight, dtype=np.float32)[first.cpu().numpy()]
    return (out.cpu().numpy() if as_np else out), w


# ---- the membership structure ------------------------------------------------------------------------------------------

def sorted_adjacency(edge_index, num_nodes, undirected=True):
    """(adj_ptr int32 [n + 1], adj_col int32 [U], U) of include/tfgx_linkpred.h: rows in order, columns strictly ascending,
    no self-pairs; undirected=True stores every edge once as (min, max).  One torch sort + unique per edge_index, memoised
    on the tensor (keyed on its version counter, so an in-place edit rebuilds it)."""
    L.require_gpu()
    n = int(num_nodes)
    memo_key = (n, bool(undirected))
    if isinstance(edge_index, torch.Tensor):
        memo = getattr(edge_index, "_tfgx_adjacency", None)
        if memo is not None and memo[0] == edge_index._version and memo_key in memo[1]:
            return memo[1][memo_key]
    ei = L.as_i32(edge_index)
    if ei.numel() == 0:
        ei = ei.reshape(2, 0)
    if ei.dim() != 2 or ei.shape[0] != 2:
        raise ValueError("edge_index must have shape [2, num_edges]")
    dev = ei.device
    r, c = ei[0].long(), ei[1].long()
    if undirected:
        r, c = torch.minimum(r, c), torch.maximum(r, c)
    if int(ei.shape[1]) > 0:
        lo, hi = int(ei.min().item()), int(ei.max().item())
        if lo < 0 or hi >= n:
            raise L.TfgxError("sorted_adjacency failed with code 2: edge endpoint outside [0, {})".format(n))
    keep = r != c
    key = torch.unique(r[keep] * n + c[keep])                      # sorted: by row, then by column
    rows = torch.div(key, n, rounding_mode="floor")
    adj_col = (key - rows * n).to(torch.int32).contiguous()
    adj_ptr = torch.zeros(n + 1, dtype=torch.int32, device=dev)
    adj_ptr[1:] = torch.cumsum(torch.bincount(rows, minlength=n), 0).to(torch.int32)
    if adj_col.numel() == 0:
        adj_col = torch.zeros(1, dtype=torch.int32, device=dev)    # a non-null pointer for "an adjacency without entries"
    res = (adj_ptr, adj_col, int(key.shape[0]))
    if isinstance(edge_index, torch.Tensor):
        memo = getattr(edge_index, "_tfgx_adjacency", None)
        if memo is None or memo[0] != edge_index._version:
            memo = (edge_index._version, {})
            edge_index._tfgx_adjacency = memo
        memo[1][memo_key] = res
    return res


# ---- negative sampling ---------------------------------------------------------------------------------------------------

def _launch_pairs(num_slots, n, adj, undirected, seed, slot_base, n_failed, dev):
    lib = L.require_gpu()
    out = torch.empty((2, num_slots), dtype=torch.int32, device=dev)
    L.check(lib.tfgx_negative_sample_pairs(num_slots, n, None if adj is None else L.ptr(adj[0]),
                                           None if adj is None else L.ptr(adj[1]), int(bool(undirected)), _u64(seed),
                                           _u64(slot_base), MAX_ATTEMPTS, L.ptr(out[0]), L.ptr(out[1]), L.ptr(n_failed),
                                           L.stream_ptr()), "tfgx_negative_sample_pairs")
    STATS["launches"] += 1
    return out


def _dense_negative_sampling(num_samples, n, adj, replace, seed, batches, dev):
    """The reference's own construction (:391-401) in torch on the device: triu mask -> nonzero -> seeded index draw."""
    STATS["dense_fallback"] += 1
    adj_ptr, adj_col, U = adj
    free = torch.ones((n, n), dtype=torch.bool, device=dev).triu(1)
    if U > 0:
        rows = torch.repeat_interleave(torch.arange(n, device=dev), (adj_ptr[1:] - adj_ptr[:-1]).long())
        free[rows, adj_col[:U].long()] = False
    neg = torch.nonzero(free).t().to(torch.int32)                  # [2, K], row-major order as np.nonzero
    K = int(neg.shape[1])
    gen = torch.Generator(device=dev)
    gen.manual_seed(_u64(seed) & 0x7FFFFFFFFFFFFFFF)
    outs = []
    for _ in range(batches):
        if replace:
            idx = torch.randint(0, K, (num_samples,), generator=gen, device=dev)
        else:
            idx = torch.randperm(K, generator=gen, device=dev)[:num_samples]
        outs.append(neg[:, idx].contiguous())
    return outs


def _density_error(n, U, pairs):
    return RuntimeError("negative_sampling: the graph is too dense for rejection sampling ({} of {} node pairs are edges) "
                        "and num_nodes = {} exceeds the {} nodes up to which the dense construction is run".format(
                            U, pairs, n, DENSE_FALLBACK_MAX_NODES))


def _sample_without_replacement(num_samples, n, adj, non_edges, seed, slot_base, dev):
    """The first num_samples DISTINCT accepted pairs of slots slot_base, slot_base + 1, ... — uniform sampling without
    replacement whatever the round sizes are.  Rounds: draw a window, keep a pair only at its first occurrence (stable
    sort by key, the smallest position per key), one host read of {distinct so far, failed slots} per round.
    Returns None when a slot failed (the caller decides between the dense construction and an error)."""
    n_failed = torch.zeros(1, dtype=torch.int32, device=dev)
    kept = torch.zeros(0, dtype=torch.int64, device=dev)           # keys n * row + col, distinct, in slot order
    have, base = 0, int(slot_base)
    while have < num_samples:
        q = num_samples - have
        if have == 0:
            m = q + q // 8 + 32                                    # sparse graphs: hardly any repeats, one round
        else:      # later rounds: the coupon collector's expectation for q new ones among non_edges - have, plus a margin
            left = non_edges - have
            m = int(1.25 * non_edges * math.log((left + 1.0) / (left - q + 1.0))) + 32
        pairs = _launch_pairs(m, n, adj, True, seed, base, n_failed, dev)
        base += m
        STATS["rounds"] += 1
        cand = torch.cat([kept, pairs[0].long() * n + pairs[1].long()])
        order = torch.sort(cand, stable=True).indices
        sorted_keys = cand[order]
        first = torch.ones_like(sorted_keys, dtype=torch.bool)
        first[1:] = sorted_keys[1:] != sorted_keys[:-1]
        is_first = torch.zeros_like(first)
        is_first[order] = first                                    # position i holds the first occurrence of its key
        front = torch.sort((~is_first).to(torch.int8), stable=True).indices      # first occurrences, in slot order, then the rest
        have, failed = torch.stack([is_first.sum().to(torch.int32), n_failed[0]]).tolist()
        if failed:
            return None
        kept = cand[front[:have]]
    kept = kept[:num_samples]
    rows = torch.div(kept, n, rounding_mode="floor")
    return torch.stack([rows, kept - rows * n]).to(torch.int32)


def negative_sampling(num_samples, num_nodes, edge_index=None, replace=True, mode="undirected", batch_size=None, seed=None):
    """
    Reference: tf_geometric/utils/graph_utils.py:369-412 (same names and order; `seed` is the one extra keyword).

    :param num_samples: pairs per returned edge_index
    :param num_nodes: ids are drawn from [0, num_nodes)
    :param edge_index: if provided, self-pairs and (undirected) edges of it are never returned and every pair has row < col;
        without it the pairs are plain uniform draws (self-pairs possible), as np.random.randint gives
    :param replace: only with edge_index: False returns distinct pairs (uniform sampling without replacement)
    :param batch_size: None: one edge_index [2, num_samples]; k: a list of k of them, drawn from disjoint slot windows
    :param seed: None draws a fresh seed from torch's generator; an int reproduces the call
    :return: a tensor when edge_index is a tensor, numpy otherwise
    """
    L.require_gpu()
    num_samples, n = int(num_samples), int(num_nodes)
    if num_samples < 0:
        raise ValueError("num_samples must not be negative")
    seed = _seed_from_torch() if seed is None else seed
    batches = 1 if batch_size is None else int(batch_size)
    as_np = not isinstance(edge_index, torch.Tensor)
    dev = L.device()
    if edge_index is None:
        n_failed = torch.zeros(1, dtype=torch.int32, device=dev)   # never written without a filter
        outs = [_launch_pairs(num_samples, n, None, False, seed, b * BATCH_SLOT_STRIDE, n_failed, dev) for b in range(batches)]
    else:
        if mode != "undirected":
            raise NotImplementedError()                            # :402-403
        adj = sorted_adjacency(edge_index, n, undirected=True)
        pairs = n * (n - 1) // 2
        non_edges = pairs - adj[2]
        if num_samples > 0 and (non_edges == 0 or (not replace and num_samples > non_edges)):
            raise ValueError("negative_sampling: {} samples{} requested, the graph has {} non-edges".format(
                num_samples, "" if replace else " without replacement", non_edges))
        outs = None
        if 2 * non_edges >= pairs:         # sparse enough: a draw is accepted with probability of about 1/2 or more
            if replace:
                n_failed = torch.zeros(1, dtype=torch.int32, device=dev)
                outs = [_launch_pairs(num_samples, n, adj, True, seed, b * BATCH_SLOT_STRIDE, n_failed, dev)
                        for b in range(batches)]
                if int(n_failed.item()) != 0:                      # the call's one host read
                    outs = None
            else:
                outs = []
                for b in range(batches):
                    one = _sample_without_replacement(num_samples, n, adj, non_edges, seed, b * BATCH_SLOT_STRIDE, dev)
                    if one is None:
                        outs = None
                        break
                    outs.append(one)
        if outs is None:
            if n > DENSE_FALLBACK_MAX_NODES:
                raise _density_error(n, adj[2], pairs)
            outs = _dense_negative_sampling(num_samples, n, adj, replace, seed, batches, dev)
    if as_np:
        outs = [o.cpu().numpy() for o in outs]
    return outs[0] if batch_size is None else outs


def negative_sampling_with_start_node(start_node_index, num_nodes, edge_index=None, seed=None):
    """
    Reference: tf_geometric/utils/graph_utils.py:415-452.  For every start node a one end node b != a with (a, b) not in
    edge_index (the DIRECTED edge set, as the reference's edge_set); without edge_index b is a plain uniform draw.

    :return: [2, len(start_node_index)] = [start_node_index, end nodes]; a tensor when start_node_index is a tensor
    """
    lib = L.require_gpu()
    as_np = not isinstance(start_node_index, torch.Tensor)
    start = L.as_i32(start_node_index).reshape(-1)
    n, S, dev = int(num_nodes), int(start.shape[0]), start.device
    seed = _seed_from_torch() if seed is None else seed
    adj = None if edge_index is None else sorted_adjacency(edge_index, n, undirected=False)
    end = torch.empty(S, dtype=torch.int32, device=dev)
    n_failed = torch.zeros(1, dtype=torch.int32, device=dev)
    L.check(lib.tfgx_negative_sample_from(L.ptr(start), S, n, None if adj is None else L.ptr(adj[0]),
                                          None if adj is None else L.ptr(adj[1]), _u64(seed), 0, MAX_ATTEMPTS, L.ptr(end),
                                          L.ptr(n_failed), L.stream_ptr()), "tfgx_negative_sample_from")
    STATS["launches"] += 1
    word = int(n_failed.item())                                    # the call's one host read
    if word < 0:
        raise L.TfgxError("tfgx_negative_sample_from failed with code 2: start node outside [0, {})".format(n))
    if word > 0:
        raise RuntimeError("negative_sampling_with_start_node: {} start nodes found no non-neighbour in {} draws "
                           "(rows of the graph that are full or nearly full)".format(word, MAX_ATTEMPTS))
    out = torch.stack([start, end])
    return out.cpu().numpy() if as_np else out


# ---- train / test split ----------------------------------------------------------------------------------------------------

def _split_sizes(test_size, num_edges):
    """sklearn's rules (model_selection._split._validate_shuffle_split): a float is a fraction, n_test = ceil(f * U); an
    int is taken literally; n_train is the rest and must not be empty."""
    if isinstance(test_size, (bool, np.bool_)) or not isinstance(test_size, (int, float, np.integer, np.floating)):
        raise ValueError("Invalid value for test_size: {!r}".format(test_size))
    if isinstance(test_size, (float, np.floating)):
        if not 0.0 < float(test_size) < 1.0:
            raise ValueError("test_size={} should be a float in the (0, 1) range".format(test_size))
        n_test = int(math.ceil(float(test_size) * num_edges))
    else:
        if not 0 < int(test_size) < num_edges:
            raise ValueError("test_size={} should be a positive integer smaller than the number of unique edges {}".format(
                test_size, num_edges))
        n_test = int(test_size)
    n_train = num_edges - n_test
    if n_train <= 0:
        raise ValueError("With {} unique edges and test_size={} the train set would be empty".format(num_edges, test_size))
    return n_train, n_test


def edge_train_test_split(edge_index, test_size, edge_weight=None, mode="undirected", seed=None, **kwargs):
    """
    Reference: tf_geometric/utils/graph_utils.py:488-535.  The edges are made upper-triangular and unique
    (convert_edge_to_upper, duplicate weights merged with "max"), shuffled by a seeded permutation on the device and cut:
    the first n_test go to the test set.

    :return: (train_edge_index, test_edge_index, train_edge_weight, test_edge_weight); the weights are None without edge_weight
    """
    if "num_nodes" in kwargs:
        warnings.warn("argument \"num_nodes\" is deprecated for the method \"edge_train_test_split\", you can remove it")
    if mode != "undirected":
        raise NotImplementedError()
    from . import convert_edge_to_upper
    L.require_gpu()
    as_np = not isinstance(edge_index, torch.Tensor)
    w_np = not isinstance(edge_weight, torch.Tensor)
    ei = L.as_i32(edge_index)
    if ei.numel() == 0:
        raise ValueError("edge_train_test_split: edge_index holds no edges")
    w = None if edge_weight is None else L.as_f32(edge_weight, ei.device)
    upper, (upper_w,) = convert_edge_to_upper(ei, [w], merge_modes=["max"])
    U = int(upper.shape[1])
    n_train, n_test = _split_sizes(test_size, U)
    gen = torch.Generator(device=ei.device)
    gen.manual_seed(_u64(_seed_from_torch() if seed is None else seed) & 0x7FFFFFFFFFFFFFFF)
    perm = torch.randperm(U, generator=gen, device=ei.device)
    test_idx, train_idx = perm[:n_test], perm[n_test:n_test + n_train]
    out = [upper[:, train_idx].contiguous(), upper[:, test_idx].contiguous(), None, None]
    if upper_w is not None:
        out[2], out[3] = upper_w[train_idx], upper_w[test_idx]
    if as_np:
        out[0], out[1] = out[0].cpu().numpy(), out[1].cpu().numpy()
    if upper_w is not None and w_np:
        out[2], out[3] = out[2].cpu().numpy(), out[3].cpu().numpy()
    return tuple(out)
