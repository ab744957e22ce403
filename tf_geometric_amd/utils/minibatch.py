# coding=utf-8
"""Minibatch neighbour sampling on the device (include/tfgx_nbrblock.h): RandomNeighborSampler.sample_rows and
RandomNeighborSampler.sample_blocks, and what they return.

The reference trains GraphSAGE on sampled neighbourhoods (demo/demo_graph_sage.py: num_sampled_neighbors_list = [25, 10]) with
a Python loop over nodes; here every hop is a handful of launches whose size is the batch: counts from row_ptr[rows], the
row-list sampler (bit for bit the rows of RandomNeighborSampler.sample), and an order-stable relabel over a table the sampler
keeps.  Nothing per call is proportional to the graph's nodes or edges.

The outermost hop's ids are consumed once, by layer 0's neighbour reduction: RandomNeighborSampler.sample_reduce
(include/tfgx_samplereduce.h) draws and reduces in one launch, and sample_blocks(fuse_input_hop=True) leaves that hop to it.

sample_blocks reads its sizes back (L + 1 host reads) and cannot be captured.  RandomNeighborSampler.sample_blocks_static
(include/tfgx_nbrstatic.h) is the same sample padded to capacities the host knows from (len(seeds), fanouts): no read, a fixed
launch sequence, replayable from a hipGraph.

Every entry point here that reads the feature table takes a float32 table or a 16-bit one declared for this route
(prepare_half_features(..., minibatch=True); include/tfgx_minibatch_h16.h) and returns float32: for the 16-bit table, bit for bit
what it returns for the table widened to float32."""
import collections

import numpy as np
import torch

from .. import _lib as L
from .subgraph import refuse_capture

_SEED_MASK = (1 << 63) - 1
_GOLDEN = 0x9E3779B97F4A7C15


def hop_seed(seed, hop):
    """The sampling seed of hop `hop` (0 = the hop next to the seeds): (seed + (hop + 1) * 0x9E3779B97F4A7C15) mod 2^63.
    Distinct per hop, so a node that is a row in two hops does not draw the same neighbours twice; each value is a valid
    `seed=` of RandomNeighborSampler.sample, which then reproduces the hop's rows."""
    return (int(seed) + (int(hop) + 1) * _GOLDEN) & _SEED_MASK


class SampledBlock(object):
    """One hop as a layer sees it: edge_index int32 [2, E] = [position of the destination in the block; virtual id of the
    sampled neighbour], edge_weight float32 [E], over num_src nodes of which the first num_dst are the destinations.
    edge_index carries its CSR plan (plan.attach_plan): a layer called on x[:num_src] sorts nothing."""

    def __init__(self, edge_index, edge_weight, num_dst, num_src):
        self.edge_index = edge_index
        self.edge_weight = edge_weight
        self.num_dst = int(num_dst)
        self.num_src = int(num_src)

    @property
    def num_edges(self):
        return int(self.edge_index.shape[1])


class SampledMinibatch(object):
    """blocks[l] belongs to layer l (input side first); node_index int32 [n] are the global ids of the virtual nodes, the
    seeds first and in the given order; hop_seeds are the per-hop sampling seeds (hop_seed); num_host_syncs counts the
    device-to-host reads the call made.

        h = mb.gather(x)
        for layer, b in zip(layers, mb.blocks):
            h = layer([h[:b.num_src], b.edge_index, b.edge_weight], training=True)[:b.num_dst]
    """

    def __init__(self, blocks, node_index, num_seeds, hop_seeds, num_host_syncs=0, input_hop=None, sampler=None):
        self.blocks = blocks
        self.node_index = node_index
        self.num_seeds = int(num_seeds)
        self.hop_seeds = list(hop_seeds)
        self.num_host_syncs = int(num_host_syncs)
        # sample_blocks(fuse_input_hop=True): (k, padding, seed) of the outermost hop, which was NOT sampled — blocks then belong
        # to layers 1 .. L-1, node_index holds the nodes known after the inner hops, and layer 0 is
        #     h = layers[0].combine([mb.gather(x), mb.input_aggregate(x, "mean")], training=True)
        self.input_hop = input_hop
        self._sampler = sampler

    def input_aggregate(self, x, op="mean"):
        """The outermost hop, drawn and reduced in one launch: float32 [len(node_index), F], row i the `op` ("mean" / "sum")
        over the neighbours node node_index[i] draws with the recorded (k, padding, seed) — what the unfused call's blocks[0]
        reduces from gather(x).  No host read: the ids are the sampler's own.  x: a float32 table, or a HalfRows declared
        minibatch=True (the bits of the call on x.float())."""
        if self.input_hop is None:
            raise ValueError("input_aggregate needs a minibatch of sample_blocks(..., fuse_input_hop=True)")
        k, padding, seed = self.input_hop
        return sample_reduce(self._sampler, self.node_index, x, k, op=op, padding=padding, seed=seed, _own_ids=True)

    def gather(self, x):
        """x[node_index] for a float32 feature table [N, F] (tfgx_gather_rows_f32; a table that is being trained goes through
        torch's indexing, which carries the gradient), or for a HalfRows declared minibatch=True: its rows widened to float32
        (tfgx_gather_rows_h16_f32), the bits of gather(x.float())."""
        half = _half_table(x, "SampledMinibatch.gather")
        if half is not None:
            n_nodes = _state(self._sampler).n_nodes if self._sampler is not None else 0
            return _gather_half(half, self.node_index, n_nodes, "SampledMinibatch.gather")
        if isinstance(x, torch.Tensor):
            if x.dtype != torch.float32:
                raise TypeError("SampledMinibatch.gather takes a float32 table, got {}".format(x.dtype))
            if x.requires_grad and torch.is_grad_enabled():
                return x[self.node_index.long()]
        from ..plan import gather_rows
        return gather_rows(L.as_f32(x), self.node_index)


def _is_integral(ids):
    if isinstance(ids, torch.Tensor):
        return ids.dtype in (torch.int8, torch.int16, torch.int32, torch.int64, torch.uint8)
    return np.asarray(ids).dtype.kind in "iu" or np.asarray(ids).size == 0


def _check_ids(ids, what):
    if not _is_integral(ids):
        raise ValueError("{} must be integers (node ids), got dtype {}".format(
            what, ids.dtype if isinstance(ids, torch.Tensor) else np.asarray(ids).dtype))
    shape = tuple(ids.shape) if isinstance(ids, torch.Tensor) else np.asarray(ids).shape
    if len(shape) != 1:
        raise ValueError("{} must be one-dimensional, got shape {}".format(what, shape))


def _check_fanouts(fanouts):
    if not isinstance(fanouts, (list, tuple)) or len(fanouts) == 0:
        raise ValueError("fanouts must be a non-empty list of neighbour counts, one per layer (input side first)")
    for f in fanouts:
        if isinstance(f, bool) or not isinstance(f, (int, np.integer)):
            raise ValueError("fanouts must be integers, got {!r}".format(f))
        if f < 0:
            raise ValueError("fanouts must not be negative, got {}".format(f))


def check_sample_blocks_args(seeds, fanouts):
    """The refusals of sample_blocks that need no device."""
    _check_fanouts(fanouts)
    _check_ids(seeds, "seeds")


def _fresh_seed():
    """seed=None: one from torch's host generator (reproducible under torch.manual_seed, different on every call)."""
    return int(torch.randint(0, 2 ** 62, (1,), dtype=torch.int64).item())


def _table(x, n_nodes, who):
    """The refusals of a float32 feature table, in the caller's name: (the table with dense rows, its leading dimension, F)."""
    if x.dim() != 2 or int(x.shape[1]) < 1:
        raise ValueError("{}: x must be a [num_nodes, F] table with F >= 1, got shape {}".format(who, tuple(x.shape)))
    if int(x.shape[0]) < n_nodes:
        raise ValueError("{}: x has {} rows but the sampler's graph has {} nodes".format(who, int(x.shape[0]), n_nodes))
    x2, ldx = L.row_major_2d(x)
    return x2, ldx, int(x.shape[1])


def _half_table(x, who):
    """x as a 16-bit table of the minibatch route (include/tfgx_minibatch_h16.h): the HalfRows when it was declared
    minibatch=True, None for anything that is no HalfRows (the float32 path judges it), TypeError for an undeclared one."""
    from ..plan import HalfRows
    if not isinstance(x, HalfRows):
        return None
    if not x.minibatch:
        raise TypeError("{} takes a float32 table, got a HalfRows that was not declared for the minibatch route: make it with "
                        "prepare_half_features(..., minibatch=True) / HalfRows(..., minibatch=True), or pass x.float()".format(who))
    return x


def _half_args(h, n_nodes, who):
    """(the table, its leading dimension in elements, F, TFGX_DT_*) of a declared HalfRows, with the float32 route's refusal of a
    table shorter than the graph."""
    if int(h.shape[0]) < n_nodes:
        raise ValueError("{}: x has {} rows but the sampler's graph has {} nodes".format(who, int(h.shape[0]), n_nodes))
    return h.table, h.ld, h.F, L.H16_DTYPES[h.dtype]


def _gather_half(h, idx, n_nodes, who):
    """float32 [len(idx), F] = widen(h[idx]), zeros where idx < 0 (tfgx_gather_rows_h16_f32): no host read."""
    if h.requires_grad and torch.is_grad_enabled():
        raise NotImplementedError("{}: a HalfRows whose source requires grad has no gather that carries the gradient (a trained "
                                  "16-bit table is out of scope): gather from a float32 tensor that requires grad".format(who))
    lib = L.require_gpu()
    table, ld, F, dt = _half_args(h, n_nodes, who)
    M = int(idx.shape[0])
    out = torch.empty((M, F), dtype=torch.float32, device=table.device)
    L.check(lib.tfgx_gather_rows_h16_f32(L.ptr(table), ld, dt, L.ptr(idx), M, F, L.ptr(out), F, L.stream_ptr()),
            "tfgx_gather_rows_h16_f32")
    return out


class _State(object):
    """What a sampler keeps for the row-list calls: row_ptr padded to every node id (nodes that only appear as neighbours have
    degree 0) and the relabel table, both made once.  begin() / end() bracket a call that writes to the table."""

    def __init__(self, sampler):
        plan = sampler.plan
        dev = plan.col.device
        self.n_nodes = max(sampler.num_row_nodes, sampler.num_col_nodes)
        tail = plan.row_ptr[-1:].expand(self.n_nodes - sampler.num_row_nodes)
        self.row_ptr = torch.cat([plan.row_ptr, tail]).contiguous()
        self.table = torch.full((self.n_nodes,), L.NBRBLOCK_EMPTY, dtype=torch.int32, device=dev)
        self.dirty = False

    def begin(self):
        if self.dirty:           # a call that raised midway left entries behind: refill once (the only O(n_nodes) step)
            self.table.fill_(L.NBRBLOCK_EMPTY)
        self.dirty = True        # until end() has reset what the call wrote

    def end(self, lib, node_list, n, stream):
        """Empties the entries of the n ids the call wrote."""
        L.check(lib.tfgx_nbrblock_reset(L.ptr(self.table), self.n_nodes, L.ptr(node_list), n, stream), "tfgx_nbrblock_reset")
        self.dirty = False


def _state(sampler):
    st = getattr(sampler, "_nbrblock", None)
    if st is None:
        st = sampler._nbrblock = _State(sampler)
    return st


def _flat_ids(ids, dev):
    t = ids if isinstance(ids, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(np.asarray(ids)))
    return t.detach().to(dev).reshape(-1)


def _ids_on_device(ids, n_nodes, dev):
    """(int32 ids, a device flag that is non-zero when an id wider than int32 was out of range before the cast)."""
    t = _flat_ids(ids, dev)
    if t.dtype == torch.int32:
        return t.contiguous(), None
    wide_bad = ((t < 0) | (t >= n_nodes)).any().to(torch.int32) if t.numel() else None
    return t.to(torch.int32).contiguous(), wide_bad


def _counts(deg, k, ratio, padding):
    """Draws per row from its degree: the rules of RandomNeighborSampler.sample."""
    if k is None and ratio is None:
        return deg
    if ratio is not None:
        return torch.ceil(deg.to(torch.float64) * float(ratio)).to(torch.int32)
    if padding:
        return torch.where(deg > 0, torch.full_like(deg, int(k)), torch.zeros_like(deg))
    return torch.clamp(deg, max=int(k))


def _degrees(st, rows):
    """deg[i] of node rows[i] from row_ptr[rows] alone; 0 for an id outside the graph (the kernels refuse those)."""
    valid = (rows >= 0) & (rows < st.n_nodes)
    r = torch.where(valid, rows, torch.zeros_like(rows)).long()
    return torch.where(valid, st.row_ptr[r + 1] - st.row_ptr[r], torch.zeros_like(rows))


def _out_ptr(cnt):
    """(out_ptr int32 [n + 1], the total as a 0-d int64 device tensor)."""
    n = int(cnt.shape[0])
    out_ptr = torch.zeros(n + 1, dtype=torch.int32, device=cnt.device)
    if n == 0:
        return out_ptr, torch.zeros((), dtype=torch.int64, device=cnt.device)
    csum = torch.cumsum(cnt, 0, dtype=torch.int64)
    out_ptr[1:] = csum
    return out_ptr, csum[-1]


def _launch_sample(sampler, st, rows, n_rows, out_ptr, total, padding, seed, flag):
    dev = rows.device
    out_col = torch.empty(max(total, 1), dtype=torch.int32, device=dev)
    out_w = torch.empty(max(total, 1), dtype=torch.float32, device=dev)
    L.check(L.load_library().tfgx_nbrblock_sample_rows(
        L.ptr(st.row_ptr), L.ptr(sampler.plan.col), L.ptr(sampler.w_csr), st.n_nodes, L.ptr(rows), n_rows, L.ptr(out_ptr),
        1 if padding else 0, int(seed), L.ptr(out_col), L.ptr(out_w), L.ptr(flag), L.stream_ptr()),
        "tfgx_nbrblock_sample_rows")
    return out_col[:total], out_w[:total]


def _row_positions(cnt, n_rows, total):
    ar = torch.arange(n_rows, dtype=torch.int32, device=cnt.device)
    return torch.repeat_interleave(ar, cnt.long(), output_size=total)


def _check_total(total):
    if total >= (1 << 31) - 1:
        raise ValueError("the sample holds {} edges: more than int32 indexes".format(total))


def _sample_rows_device(sampler, rows, k, ratio, padding, seed, who):
    """sample_rows on the device: (edge_index [2, E], edge_weight [E], out_ptr [n_rows + 1])."""
    st = _state(sampler)
    dev = st.table.device
    rows_t, wide_bad = _ids_on_device(rows, st.n_nodes, dev)
    n_rows = int(rows_t.shape[0])
    if n_rows == 0:
        return (torch.zeros((2, 0), dtype=torch.int32, device=dev), torch.zeros(0, dtype=torch.float32, device=dev),
                torch.zeros(1, dtype=torch.int32, device=dev))
    cnt = _counts(_degrees(st, rows_t), k, ratio, padding)
    out_ptr, total_dev = _out_ptr(cnt)
    flag = torch.zeros(1, dtype=torch.int32, device=dev)
    if wide_bad is not None:
        flag |= wide_bad
    total = int(total_dev.item())
    _check_total(total)
    out_col, out_w = _launch_sample(sampler, st, rows_t, n_rows, out_ptr, total, padding, seed, flag)
    if int(flag.item()) != 0:
        raise ValueError("{}: a row id is outside [0, {})".format(who, st.n_nodes))
    return torch.stack([_row_positions(cnt, n_rows, total), out_col]), out_w.contiguous(), out_ptr


def sample_rows(sampler, rows, k=None, ratio=None, padding=False, seed=None):
    if k is not None and ratio is not None:
        raise Exception("k and ratio cannot be provided simultaneously")
    _check_ids(rows, "rows")
    L.require_gpu()
    refuse_capture("RandomNeighborSampler.sample_rows")
    if seed is None:
        seed = _fresh_seed()
    ei, ew, _ = _sample_rows_device(sampler, rows, k, ratio, padding, seed, "sample_rows")
    return (ei.cpu().numpy(), ew.cpu().numpy()) if sampler._numpy else (ei, ew)


# ---- the fused input hop (include/tfgx_samplereduce.h) ------------------------------------------------------------------
_OPS = {"mean": L.MEAN, "sum": L.SUM}


def check_sample_reduce_args(k, ratio=None):
    """The refusals of sample_reduce that need no device."""
    if ratio is not None:
        raise ValueError("sample_reduce has no fused form for ratio= sampling (the kernel keeps at most {} draws per row on chip): "
                         "pass k, or reduce the list of sample_rows(ratio=...)".format(L.SAMPLEREDUCE_MAX_DRAWS))
    if k is None:
        raise ValueError("sample_reduce has no fused form for k=None (every neighbour: a row may be as long as the graph): "
                         "pass k, or reduce the whole graph with segment_reduce")
    if isinstance(k, bool) or not isinstance(k, (int, np.integer)):
        raise ValueError("k must be an integer, got {!r}".format(k))
    if k < 0:
        raise ValueError("k must not be negative, got {}".format(k))


def sample_reduce_route(k, x):
    """"fused" (one launch of tfgx_samplereduce_f32, or of tfgx_sample_reduce_h16 for a HalfRows) or "composed" (sample_rows,
    then the reduction over the list, which carries d/dx): what sample_reduce itself dispatches on."""
    check_sample_reduce_args(k)
    # a torch.Tensor, or a HalfRows (whose source tensor receives d/dx)
    trained = bool(getattr(x, "requires_grad", False)) and torch.is_grad_enabled()
    return "fused" if int(k) <= L.SAMPLEREDUCE_MAX_DRAWS and not trained else "composed"


def _check_out(out, n_rows, F, dev):
    if not (isinstance(out, torch.Tensor) and out.dtype == torch.float32 and out.device == dev and out.dim() == 2
            and tuple(out.shape) == (n_rows, F) and (n_rows == 0 or out.stride(1) == 1) and (n_rows <= 1 or out.stride(0) >= F)):
        raise ValueError("sample_reduce: out must be a float32 [{}, {}] tensor on {} with dense rows".format(n_rows, F, dev))


def sample_reduce(sampler, rows, x, k, op="mean", padding=False, seed=None, ratio=None, out=None, return_count=False,
                  _own_ids=False):
    from ..plan import CsrPlan, segment_reduce
    check_sample_reduce_args(k, ratio)
    if op not in _OPS:
        raise ValueError("sample_reduce: op must be 'mean' or 'sum', got {!r}".format(op))
    half = _half_table(x, "sample_reduce")
    if isinstance(x, torch.Tensor) and x.dtype != torch.float32:
        raise TypeError("sample_reduce takes a float32 table, got {}".format(x.dtype))
    _check_ids(rows, "rows")
    lib = L.require_gpu()
    refuse_capture("RandomNeighborSampler.sample_reduce")
    route = sample_reduce_route(k, x)
    st = _state(sampler)
    if half is not None:        # a declared 16-bit table, read in place (include/tfgx_minibatch_h16.h)
        x2, ldx, F, x_dt = _half_args(half, st.n_nodes, "sample_reduce")
    else:
        x = L.as_f32(x)
        x2, ldx, F = _table(x, st.n_nodes, "sample_reduce")
    if seed is None:
        seed = _fresh_seed()
    dev = st.table.device
    if route == "composed":
        ei, ew, out_ptr = _sample_rows_device(sampler, rows, int(k), None, padding, seed, "sample_reduce")
        n_rows = int(out_ptr.shape[0]) - 1
        count = out_ptr[1:] - out_ptr[:-1]
        if out is not None:
            _check_out(out, n_rows, F, dev)
        if n_rows == 0:
            res = torch.empty((0, F), dtype=torch.float32, device=dev) if out is None else out
        else:
            plan = CsrPlan.from_sorted(out_ptr, ei[1], int(x.shape[0]), edge_index=ei)      # global column ids: x is the table
            if x.requires_grad and torch.is_grad_enabled():
                if out is not None:
                    raise ValueError("sample_reduce: out= cannot be given for an x that requires grad")
                from .. import autograd as AG
                res = AG.aggregate(plan, x, _OPS[op], ew)
            else:
                res = segment_reduce(plan, x, _OPS[op], w_csr=ew, out=out)
        return (res, count) if return_count else res
    rows_t, wide_bad = _ids_on_device(rows, st.n_nodes, dev)
    n_rows = int(rows_t.shape[0])
    if out is None:
        out = torch.empty((n_rows, F), dtype=torch.float32, device=dev)
    else:
        _check_out(out, n_rows, F, dev)
    count = torch.zeros(n_rows, dtype=torch.int32, device=dev) if return_count else None
    if n_rows == 0:
        return (out, count) if return_count else out
    ldo = int(out.stride(0)) if n_rows > 1 else F
    flag = torch.zeros(1, dtype=torch.int32, device=dev)
    if wide_bad is not None:
        flag |= wide_bad
    if half is not None:
        L.check(lib.tfgx_sample_reduce_h16(
            L.ptr(st.row_ptr), L.ptr(sampler.plan.col), L.ptr(sampler.w_csr), st.n_nodes, L.ptr(rows_t), n_rows, int(k),
            1 if padding else 0, int(seed), L.ptr(x2), ldx, F, x_dt, _OPS[op], L.ptr(out), ldo, L.ptr(count), L.ptr(flag),
            L.stream_ptr()), "tfgx_sample_reduce_h16")
    else:
        L.check(lib.tfgx_samplereduce_f32(
            L.ptr(st.row_ptr), L.ptr(sampler.plan.col), L.ptr(sampler.w_csr), st.n_nodes, L.ptr(rows_t), n_rows, int(k),
            1 if padding else 0, int(seed), L.ptr(x2), ldx, F, _OPS[op], L.ptr(out), ldo, L.ptr(count), L.ptr(flag),
            L.stream_ptr()), "tfgx_samplereduce_f32")
    # the one host read: the verdict on `rows` (not taken for ids the sampler produced itself)
    if not _own_ids and int(flag.item()) != 0:
        raise ValueError("sample_reduce: a row id is outside [0, {})".format(st.n_nodes))
    return (out, count) if return_count else out


def sample_blocks(sampler, seeds, fanouts, padding=False, seed=None, fuse_input_hop=False):
    from ..plan import CsrPlan, attach_plan
    check_sample_blocks_args(seeds, fanouts)
    lib = L.require_gpu()
    refuse_capture("RandomNeighborSampler.sample_blocks")
    if seed is None:
        seed = _fresh_seed()
    hop_seeds = [hop_seed(seed, h) for h in range(len(fanouts))]
    # fuse_input_hop: the outermost hop (fanouts[0], the last seed) is left to sample_reduce; the hops before it run as ever
    n_hops = len(fanouts) - (1 if fuse_input_hop else 0)
    input_hop = (int(fanouts[0]), bool(padding), hop_seeds[-1]) if fuse_input_hop else None
    st = _state(sampler)
    dev = st.table.device
    st.begin()
    stream = L.stream_ptr()
    syncs = 0

    node_list, wide_bad = _ids_on_device(seeds, st.n_nodes, dev)
    num_seeds = n_known = int(node_list.shape[0])
    flag = torch.zeros(1, dtype=torch.int32, device=dev)
    if wide_bad is not None:
        flag |= wide_bad
    L.check(lib.tfgx_nbrblock_stamp(L.ptr(st.table), st.n_nodes, L.ptr(node_list), n_known, 0, L.ptr(flag), stream),
            "tfgx_nbrblock_stamp")
    cnt = _counts(_degrees(st, node_list), int(fanouts[-1]), None, padding)
    out_ptr, total_dev = _out_ptr(cnt)
    bad, total = torch.stack([flag[0].long(), total_dev]).tolist()      # host read: the seeds' verdict and hop 1's edges
    syncs += 1
    if bad & L.NBRBLOCK_BAD_RANGE:
        raise ValueError("sample_blocks: a seed is outside [0, {})".format(st.n_nodes))
    if bad & L.NBRBLOCK_BAD_REPEAT:
        raise ValueError("sample_blocks: seeds must not repeat")

    blocks = []
    for h in range(n_hops):
        _check_total(total + n_known)
        out_col, out_w = _launch_sample(sampler, st, node_list, n_known, out_ptr, total, padding, hop_seeds[h], flag)
        grown = torch.zeros(n_known + total, dtype=torch.int32, device=dev)      # room for every sampled id to be new
        grown[:n_known] = node_list[:n_known]
        vcol = torch.empty(total, dtype=torch.int32, device=dev)
        n_new_dev = torch.zeros(1, dtype=torch.int32, device=dev)
        if total > 0:
            ws_bytes = lib.tfgx_nbrblock_relabel_workspace_bytes(total)
            ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
            L.check(lib.tfgx_nbrblock_relabel(L.ptr(st.table), st.n_nodes, n_known, L.ptr(out_col), total, L.ptr(vcol),
                                              L.ptr(grown), L.ptr(n_new_dev), L.ptr(ws), ws_bytes, stream),
                    "tfgx_nbrblock_relabel")
        if h + 1 < n_hops:
            # the next hop's counts over the whole buffer (entries past the new total are masked out), so that ONE host read
            # brings both the new-node total and the next hop's edge total
            live = torch.arange(n_known + total, device=dev) < (n_known + n_new_dev[0])
            deg = torch.where(live, _degrees(st, grown), torch.zeros_like(grown))
            next_cnt = _counts(deg, int(fanouts[len(fanouts) - 2 - h]), None, padding)
            next_ptr, next_total_dev = _out_ptr(next_cnt)
            n_new, next_total = torch.stack([n_new_dev[0].long(), next_total_dev]).tolist()
        else:
            n_new, bad = torch.stack([n_new_dev[0].long(), flag[0].long()]).tolist()
            if bad:
                raise L.TfgxError("sample_blocks: the sampler refused a row id it produced itself")
        syncs += 1
        n_src = n_known + n_new
        ei = torch.stack([_row_positions(cnt, n_known, total), vcol])
        # the kernels have written the list: hand its plan on with it (out_ptr IS the row_ptr; no sort)
        attach_plan(ei, CsrPlan.from_sorted(out_ptr, vcol, n_src, edge_index=ei))
        blocks.append(SampledBlock(ei, out_w.contiguous(), n_known, n_src))
        node_list, n_known = grown, n_src
        if h + 1 < n_hops:
            cnt, out_ptr, total = next_cnt[:n_src].contiguous(), next_ptr[:n_src + 1].contiguous(), next_total

    st.end(lib, node_list, n_known, stream)
    return SampledMinibatch(blocks[::-1], node_list[:n_known].contiguous(), num_seeds, hop_seeds, syncs, input_hop, sampler)


# ---- fixed-shape sampling (include/tfgx_nbrstatic.h): no host read, hipGraph-capturable ---------------------------------
StaticCapacities = collections.namedtuple("StaticCapacities", "rows edges sinks fanouts")
StaticCapacities.__doc__ = """The sizes of sample_blocks_static, hop by hop outward from the seeds (hop h = 1 .. L uses
fanouts[L - h]): rows[0] = B and rows[h] = R_h virtual nodes after hop h; edges[h - 1] = E_h = R_{h-1} * k_h, also the number
of new-node slots; sinks[h - 1] = S_h = R_{h-1} (0 when k_h == 0); fanouts[h - 1] = k_h.  R_h = R_{h-1} + E_h + S_h."""


def _capacities(B, ks):
    """StaticCapacities for the hop-ordered fan-outs `ks`; refuses a total that int32 does not index."""
    rows, edges, sinks = [int(B)], [], []
    for k in ks:
        R = rows[-1]
        E, S = R * int(k), (R if int(k) > 0 else 0)
        if R + E + S >= (1 << 31) - 1:
            raise ValueError("static_capacities: {} seeds with fan-outs {} need {} virtual nodes after hop {}: more than int32 "
                             "indexes".format(B, [int(v) for v in ks][::-1], R + E + S, len(edges) + 1))
        rows.append(R + E + S)
        edges.append(E)
        sinks.append(S)
    return StaticCapacities(rows, edges, sinks, [int(k) for k in ks])


def check_static_args(fanouts, ratio=None):
    """The refusals of sample_blocks_static that need neither the seeds nor a device."""
    if ratio is not None:
        raise ValueError("sample_blocks_static has no form for ratio= sampling (a row's list has no bound the host knows): pass "
                         "fan-outs, or use sample_rows(ratio=...)")
    if isinstance(fanouts, (list, tuple)) and any(f is None for f in fanouts):
        raise ValueError("sample_blocks_static has no form for a fan-out of None (k=None keeps every neighbour: a row may be as "
                         "long as the graph, so there is no capacity): pass integer fan-outs, or use sample_blocks")
    _check_fanouts(fanouts)


def static_capacities(B, fanouts):
    """The shapes of sample_blocks_static(seeds of length B, fanouts), from the two arguments alone (StaticCapacities).
    static_capacities(1024, [25, 10]).rows == [1024, 12288, 331776].  ValueError beyond int32."""
    check_static_args(fanouts)
    if isinstance(B, bool) or not isinstance(B, (int, np.integer)) or B < 0:
        raise ValueError("static_capacities: B must be a non-negative integer, got {!r}".format(B))
    return _capacities(int(B), [int(k) for k in fanouts][::-1])


def _device_seed(seed, dev, who):
    """The seed as one int64 on the device.  A tensor is used where it is (the kernels read it when they run); an int is
    placed with a fill; None draws from torch's host generator, which a capture would freeze into the graph."""
    if isinstance(seed, torch.Tensor):
        if seed.dtype != torch.int64 or seed.numel() != 1 or seed.device != dev:
            raise ValueError("{}: a tensor seed must be one int64 on {}, got {} {} on {}".format(
                who, dev, tuple(seed.shape), seed.dtype, seed.device))
        return seed.detach().reshape(1)
    if seed is None:
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError("{}: seed=None inside a hipGraph capture would freeze one by-value seed into the graph and every "
                               "replay would draw the same sample: pass an int64 one-element device tensor and advance it inside "
                               "the captured function (state.add_(1))".format(who))
        seed = _fresh_seed()
    if isinstance(seed, bool) or not isinstance(seed, (int, np.integer)):
        raise ValueError("{}: seed must be an int, an int64 one-element device tensor or None, got {!r}".format(who, seed))
    s = int(seed) & ((1 << 64) - 1)
    return torch.full((1,), s - (1 << 64) if s >= (1 << 63) else s, dtype=torch.int64, device=dev)


def _no_fused_static(why):
    return ValueError("sample_blocks_static: the fused input hop {}; use the composed dynamic route, sample_blocks(..., "
                      "fuse_input_hop=True), whose input_aggregate falls back to sample_rows and a differentiable "
                      "reduction".format(why))


class StaticMinibatch(object):
    """What sample_blocks_static returns.  blocks[l] belongs to layer l (input side first), each a square graph on its
    num_src nodes with both CSR plans attached; node_index int32 [R_L] = the global id of a live virtual node, -1 for a dead
    one (a dead seed slot, an unused new-node slot, a sink row); live = node_index >= 0; seed_mask = live[:num_seeds];
    counts int32 [hops, 2] on the device = (sampled edges, new nodes) per hop outward; flag: the device word check() reads;
    seed: the device seed the kernels read.  num_host_syncs == 0: nothing was read back.

        h = mb.gather(x)                                   # zeros for dead rows
        for layer, b in zip(layers, mb.blocks):
            h = layer([h[:b.num_src], b.edge_index, b.edge_weight], training=True)[:b.num_dst]
        loss = (per_seed_loss(h) * mb.seed_mask).sum() / mb.seed_mask.sum().clamp(min=1)
    """

    num_host_syncs = 0

    def __init__(self, blocks, node_index, num_seeds, counts, flag, seed, capacities, n_nodes, input_hop=None, sampler=None):
        self.blocks = blocks
        self.node_index = node_index
        self.num_seeds = int(num_seeds)
        self.live = node_index >= 0
        self.seed_mask = self.live[:self.num_seeds]
        self.counts = counts
        self.flag = flag
        self.seed = seed
        self.capacities = capacities
        # fuse_input_hop=True: (k, padding, hop index) of the outermost hop, which was NOT sampled (blocks belong to layers 1 .. L-1)
        self.input_hop = input_hop
        self._n_nodes = int(n_nodes)
        self._sampler = sampler

    def check(self):
        """The ONE host read of a static minibatch, when the caller wants it: the ValueErrors of sample_blocks — a seed outside
        the graph (other than -1), seeds that repeat.  The offending slots are dead in this minibatch either way."""
        bad = int(self.flag.item())
        if bad & L.NBRSTATIC_BAD_RANGE:
            raise ValueError("sample_blocks_static: a seed is outside [0, {})".format(self._n_nodes))
        if bad & L.NBRSTATIC_BAD_REPEAT:
            raise ValueError("sample_blocks_static: seeds must not repeat")
        return self

    def gather(self, x):
        """float32 [R_L, F]: x[node_index] for the live rows, zeros for the dead ones (tfgx_nbrstatic_gather_rows_f32; a table
        that is being trained goes through torch's indexing with a clamp and a mask, which carries the gradient).  A HalfRows
        declared minibatch=True is widened as it is gathered (tfgx_gather_rows_h16_f32): the bits of gather(x.float())."""
        half = _half_table(x, "StaticMinibatch.gather")
        if half is not None:
            return _gather_half(half, self.node_index, self._n_nodes, "StaticMinibatch.gather")
        if isinstance(x, torch.Tensor):
            if x.dtype != torch.float32:
                raise TypeError("StaticMinibatch.gather takes a float32 table, got {}".format(x.dtype))
            if x.requires_grad and torch.is_grad_enabled():
                rows = x[self.node_index.clamp(min=0).long()]
                return torch.where(self.live[:, None], rows, torch.zeros((), dtype=x.dtype, device=x.device))
        lib = L.require_gpu()
        x = L.as_f32(x)
        x2, ldx, F = _table(x, self._n_nodes, "StaticMinibatch.gather")
        M = int(self.node_index.shape[0])
        out = torch.empty((M, F), dtype=torch.float32, device=x2.device)
        L.check(lib.tfgx_nbrstatic_gather_rows_f32(L.ptr(x2), ldx, L.ptr(self.node_index), M, F, L.ptr(out), F, L.stream_ptr()),
                "tfgx_nbrstatic_gather_rows_f32")
        return out

    def input_aggregate(self, x, op="mean"):
        """The outermost hop, drawn and reduced in one launch with the seed read from the device: float32 [len(node_index), F],
        row i the `op` ("mean" / "sum") over the neighbours node_index[i] draws — bit for bit what the dynamic minibatch's
        input_aggregate gives that node — and zeros for a dead row.  No host read.  x: a float32 table, or a HalfRows declared
        minibatch=True (tfgx_nbr_static_input_hop_h16: the bits of the call on x.float())."""
        if self.input_hop is None:
            raise ValueError("input_aggregate needs a minibatch of sample_blocks_static(..., fuse_input_hop=True)")
        if op not in _OPS:
            raise ValueError("input_aggregate: op must be 'mean' or 'sum', got {!r}".format(op))
        half = _half_table(x, "StaticMinibatch.input_aggregate")
        if isinstance(x, torch.Tensor) and x.dtype != torch.float32:
            raise _no_fused_static("takes a float32 table, got {}".format(x.dtype))
        if bool(getattr(x, "requires_grad", False)) and torch.is_grad_enabled():      # a tensor, or a HalfRows over a trained one
            raise _no_fused_static("carries no gradient to a table that requires grad")
        lib = L.require_gpu()
        k, padding, hop = self.input_hop
        st = _state(self._sampler)
        M = int(self.node_index.shape[0])
        if half is not None:        # a declared 16-bit table, read in place (include/tfgx_minibatch_h16.h)
            x2, ldx, F, x_dt = _half_args(half, st.n_nodes, "input_aggregate")
            out = torch.empty((M, F), dtype=torch.float32, device=x2.device)
            L.check(lib.tfgx_nbr_static_input_hop_h16(
                L.ptr(st.row_ptr), L.ptr(self._sampler.plan.col), L.ptr(self._sampler.w_csr), st.n_nodes, L.ptr(self.node_index), M,
                int(k), 1 if padding else 0, L.ptr(self.seed), int(hop), L.ptr(x2), ldx, F, x_dt, _OPS[op], L.ptr(out), F, None,
                L.ptr(self.flag), L.stream_ptr()), "tfgx_nbr_static_input_hop_h16")
            return out
        x = L.as_f32(x)
        x2, ldx, F = _table(x, st.n_nodes, "input_aggregate")
        out = torch.empty((M, F), dtype=torch.float32, device=x2.device)
        L.check(lib.tfgx_nbrstatic_input_hop_f32(
            L.ptr(st.row_ptr), L.ptr(self._sampler.plan.col), L.ptr(self._sampler.w_csr), st.n_nodes, L.ptr(self.node_index), M,
            int(k), 1 if padding else 0, L.ptr(self.seed), int(hop), L.ptr(x2), ldx, F, _OPS[op], L.ptr(out), F, None,
            L.ptr(self.flag), L.stream_ptr()), "tfgx_nbrstatic_input_hop_f32")
        return out


def _static_seeds_on_device(seeds, n_nodes, dev):
    """int32 seeds on the device without a read: an id wider than int32 is clamped to an out-of-range int32 first (the kernel
    then flags it as it flags any other)."""
    t = _flat_ids(seeds, dev)
    if t.dtype != torch.int32:
        t = t.long().clamp(min=-2, max=n_nodes).to(torch.int32)
    return t.contiguous()


def sample_blocks_static(sampler, seeds, fanouts, padding=False, seed=None, fuse_input_hop=False, ratio=None):
    from ..plan import CsrPlan, attach_plan, hub_policy
    check_static_args(fanouts, ratio)
    _check_ids(seeds, "seeds")
    who = "RandomNeighborSampler.sample_blocks_static"
    n_layers = len(fanouts)
    k_input = int(fanouts[0])
    if fuse_input_hop and k_input > L.SAMPLEREDUCE_MAX_DRAWS:
        raise _no_fused_static("keeps at most {} draws per row on chip, got fanouts[0] = {}".format(L.SAMPLEREDUCE_MAX_DRAWS, k_input))
    lib = L.require_gpu()
    st = getattr(sampler, "_nbrblock", None)
    if st is None:
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError("{}: the sampler's row_ptr and relabel table are made on its first call, which cannot be a captured "
                               "one: call it once eagerly before the capture (the warm-up of CapturedTrainStep does)".format(who))
        st = _state(sampler)
    dev = st.table.device
    seed_t = _device_seed(seed, dev, who)
    seeds_t = _static_seeds_on_device(seeds, st.n_nodes, dev)
    B = int(seeds_t.shape[0])
    # fuse_input_hop: the outermost hop (fanouts[0], hop index L - 1) is left to input_aggregate
    ks = [int(k) for k in (fanouts[1:] if fuse_input_hop else fanouts)][::-1]
    cap = _capacities(B, ks)
    input_hop = (k_input, bool(padding), n_layers - 1) if fuse_input_hop else None
    st.begin()
    stream = L.stream_ptr()
    n_total = cap.rows[-1]
    node = torch.empty(n_total, dtype=torch.int32, device=dev)
    flag = torch.zeros(1, dtype=torch.int32, device=dev)
    counts = torch.zeros((len(ks), 2), dtype=torch.int32, device=dev)
    L.check(lib.tfgx_nbrstatic_seeds(L.ptr(st.table), st.n_nodes, L.ptr(seeds_t), B, L.ptr(node), L.ptr(flag), stream),
            "tfgx_nbrstatic_seeds")
    blocks = []
    for h, k in enumerate(ks):
        R, E, Rn = cap.rows[h], cap.edges[h], cap.rows[h + 1]
        if R == 0:
            brp = torch.zeros(1, dtype=torch.int32, device=dev)
        else:
            brp = torch.empty(Rn + 1, dtype=torch.int32, device=dev)
        ei = torch.empty((2, E), dtype=torch.int32, device=dev)
        ew = torch.empty(E, dtype=torch.float32, device=dev)
        ws_bytes = lib.tfgx_nbrstatic_hop_workspace_bytes(R, k)
        ws = torch.empty(max(ws_bytes, 1), dtype=torch.uint8, device=dev)
        L.check(lib.tfgx_nbrstatic_hop(
            L.ptr(st.row_ptr), L.ptr(sampler.plan.col), L.ptr(sampler.w_csr), st.n_nodes, L.ptr(st.table), L.ptr(node), R, k,
            1 if padding else 0, L.ptr(seed_t), h, L.ptr(brp), L.ptr(ei[0]), L.ptr(ei[1]), L.ptr(ew), L.ptr(counts[h]), L.ptr(ws),
            ws_bytes, stream), "tfgx_nbrstatic_hop")
        # both plans, no sort of the list by destination (brp IS the row_ptr, sink and empty rows included) and no host read
        plan = CsrPlan.from_sorted(brp, ei[1], Rn, edge_index=ei)
        t_row_ptr = torch.empty(Rn + 1, dtype=torch.int32, device=dev)
        t_col = torch.empty(E, dtype=torch.int32, device=dev)
        t_perm = torch.empty(E, dtype=torch.int32, device=dev)
        tws_bytes = lib.tfgx_nbrstatic_transpose_workspace_bytes(E, Rn)
        tws = torch.empty(max(tws_bytes, 1), dtype=torch.uint8, device=dev)
        L.check(lib.tfgx_nbrstatic_transpose(L.ptr(ei[0]), L.ptr(ei[1]), E, Rn, L.ptr(t_row_ptr), L.ptr(t_col), L.ptr(t_perm),
                                             L.ptr(tws), tws_bytes, stream), "tfgx_nbrstatic_transpose")
        if Rn == 0:
            t_row_ptr.zero_()
        pt = CsrPlan(t_row_ptr, t_col, t_perm, Rn, Rn, E)
        plan._transposed, pt._transposed = pt, plan
        # no destination row is longer than k: where that is within the hub threshold the plan has no hub rows, and the walk
        # order (a speed-up of skewed plans; results do not depend on it) is left out — neither is computed, neither reads back.
        # The transposed plan (a popular source may be long) keeps its lazy metadata.
        thr, _ = hub_policy(E, Rn)
        if k <= thr:
            plan.hub_threshold, plan._hub, plan._row_order = thr, False, False
        attach_plan(ei, plan)
        blocks.append(SampledBlock(ei, ew, R, Rn))
    st.end(lib, node, n_total, stream)
    return StaticMinibatch(blocks[::-1], node, B, counts, flag, seed_t, cap, st.n_nodes, input_hop, sampler)
