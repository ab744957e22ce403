# coding=utf-8
"""GraphStore: a dataset of whole graphs held on the device, and minibatches assembled from it in one kernel launch
(include/tfgx_collate.h) — features, index arrays and all three CSR plans, with no sort and no host synchronisation.

A batch of whole graphs is block-diagonal, so its plans are the concatenation of its graphs' pieces of the dataset's plans
with the offsets exchanged.  The dataset's two plans (by destination, by source) are built once, when the store goes to the
device: the only sorts the dataset ever pays for."""
import collections
import ctypes

import numpy as np
import torch

from .. import _lib as L
from ..plan import CsrPlan, CACHE_KEY_PLAN, attach_plan
from .graph import Graph, BatchGraph, StaticBatchGraph

COLLATE_TILE = L.COLLATE_TILE        # output elements per workgroup of the collate kernel (TFGX_COLLATE_TILE)
_INT32_LIMIT = (1 << 31) - 1         # sizes the C ABI takes are below this


StaticBatchCapacities = collections.namedtuple("StaticBatchCapacities", "batch_size max_nodes max_edges sink_degree sinks n_cap e_cap")
StaticBatchCapacities.__doc__ = """The sizes of GraphStore.collate_static for B = batch_size slots: the live nodes / edges of a batch
stay within max_nodes / max_edges; sinks = P = max(1, ceil(max_edges / sink_degree)) dead rows take the padded edges, at most
sink_degree each; the batch has n_cap = max_nodes + P rows and e_cap = max_edges edges."""


def _host(a):
    return a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)


class GraphStore(object):
    """``GraphStore(graphs)`` packs a list of ``Graph`` once: x [N_total, F] float32, the edge list in dataset-global node
    ids int32 [2, E_total], edge_weight [E_total], y with one leading row per graph (any dtype, or None) and the per-graph
    ``node_ptr`` / ``edge_ptr`` [G + 1], which stay on the host as numpy: all batch sizes are host arithmetic.

    Refused, with the graph named: an endpoint outside its own graph, graphs of different feature widths, totals beyond int32.

    Packing and every refusal are host work.  The packed arrays go to the device (and the two dataset plans are built) in the
    constructor when a GPU is present, else at the first ``collate``, which then raises: there is no CPU path."""

    def __init__(self, graphs):
        graphs = list(graphs)
        xs, eis, ws, ys = [], [], [], []
        F = None
        for i, g in enumerate(graphs):
            x = _host(g.x)
            if x.ndim != 2:
                raise ValueError("graph {}: x must be [num_nodes, num_features], got shape {}".format(i, x.shape))
            if F is None:
                F = int(x.shape[1])
            elif int(x.shape[1]) != F:
                raise ValueError("graph {} has {} features, graph 0 has {}".format(i, x.shape[1], F))
            n, e = int(x.shape[0]), int(g.num_edges)
            ei = _host(g.edge_index).astype(np.int64).reshape(2, e)
            if e and (ei.min() < 0 or ei.max() >= n):
                k = int(np.nonzero((ei < 0).any(0) | (ei >= n).any(0))[0][0])
                raise ValueError("graph {}: edge {} ({}, {}) has an endpoint outside its {} nodes".format(
                    i, k, ei[0, k], ei[1, k], n))
            w = np.ones(e, np.float32) if g.edge_weight is None else _host(g.edge_weight).astype(np.float32).reshape(-1)
            if w.shape[0] != e:
                raise ValueError("graph {}: {} edge weights for {} edges".format(i, w.shape[0], e))
            if (g.y is None) != (graphs[0].y is None):
                raise ValueError("graph {}: y is {} but graph 0's is {}".format(
                    i, "absent" if g.y is None else "given", "absent" if graphs[0].y is None else "given"))
            if g.y is not None:
                y = _host(g.y)
                if y.ndim < 1 or y.shape[0] != 1:
                    raise ValueError("graph {}: y must have one leading row ([1, ...]), got shape {}".format(i, y.shape))
                ys.append(y)
            xs.append(x.astype(np.float32))
            eis.append(ei)
            ws.append(w)
        F = 0 if F is None else F
        node_ptr = np.concatenate([[0], np.cumsum([x.shape[0] for x in xs], dtype=np.int64)]).astype(np.int64)
        edge_ptr = np.concatenate([[0], np.cumsum([ei.shape[1] for ei in eis], dtype=np.int64)]).astype(np.int64)
        x = np.concatenate(xs, axis=0) if xs else np.zeros((0, F), np.float32)
        ei = np.concatenate([ei + off for ei, off in zip(eis, node_ptr[:-1])], axis=1) if eis else np.zeros((2, 0), np.int64)
        w = np.concatenate(ws) if ws else np.zeros(0, np.float32)
        y = np.concatenate(ys, axis=0) if ys else None
        self._init_packed(x, ei, node_ptr, edge_ptr, w, y)

    @classmethod
    def from_arrays(cls, x, edge_index, node_ptr, edge_ptr, edge_weight=None, y=None):
        """A store over ALREADY PACKED numpy arrays: x [N_total, F], edge_index [2, E_total] in dataset-global node ids with
        the edges of graph g at [edge_ptr[g], edge_ptr[g + 1]) and its nodes at [node_ptr[g], node_ptr[g + 1]), edge_weight
        [E_total] (ones when absent), y [G, ...] or None.  The same refusals as the constructor."""
        store = cls.__new__(cls)
        x = np.asarray(x)
        if x.ndim != 2:
            raise ValueError("x must be [N_total, F], got shape {}".format(x.shape))
        ei = np.asarray(edge_index).astype(np.int64).reshape(2, -1)
        w = np.ones(ei.shape[1], np.float32) if edge_weight is None else np.asarray(edge_weight, dtype=np.float32).reshape(-1)
        store._init_packed(x.astype(np.float32), ei, np.asarray(node_ptr, dtype=np.int64).reshape(-1),
                           np.asarray(edge_ptr, dtype=np.int64).reshape(-1), w, None if y is None else np.asarray(y))
        return store

    def _init_packed(self, x, ei, node_ptr, edge_ptr, w, y):
        G = int(node_ptr.shape[0]) - 1
        if G < 0 or edge_ptr.shape[0] != G + 1 or node_ptr[0] != 0 or edge_ptr[0] != 0:
            raise ValueError("node_ptr and edge_ptr must both be [G + 1] and start at 0")
        if (np.diff(node_ptr) < 0).any() or (np.diff(edge_ptr) < 0).any():
            raise ValueError("node_ptr and edge_ptr must not decrease")
        for name, ptr in (("nodes", node_ptr), ("edges", edge_ptr)):
            if ptr[-1] >= _INT32_LIMIT:
                g = int(np.nonzero(ptr >= _INT32_LIMIT)[0][0]) - 1
                raise ValueError("graph {}: the dataset's {} up to and including it ({}) do not fit int32".format(
                    g, name, int(ptr[g + 1])))
        if node_ptr[-1] != x.shape[0] or edge_ptr[-1] != ei.shape[1] or w.shape[0] != ei.shape[1]:
            raise ValueError("packed sizes disagree: node_ptr ends at {} for {} rows of x, edge_ptr at {} for {} edges and {} "
                             "weights".format(node_ptr[-1], x.shape[0], edge_ptr[-1], ei.shape[1], w.shape[0]))
        if y is not None and y.shape[0] != G:
            raise ValueError("y has {} rows for {} graphs".format(y.shape[0], G))
        if ei.shape[1]:
            graph_of_edge = np.repeat(np.arange(G), np.diff(edge_ptr))
            bad = ((ei < node_ptr[graph_of_edge]) | (ei >= node_ptr[graph_of_edge + 1])).any(0)
            if bad.any():
                k = int(np.nonzero(bad)[0][0])
                g = int(graph_of_edge[k])
                raise ValueError("graph {}: edge {} ({}, {}) has an endpoint outside its {} nodes".format(
                    g, k - int(edge_ptr[g]), int(ei[0, k] - node_ptr[g]), int(ei[1, k] - node_ptr[g]),
                    int(node_ptr[g + 1] - node_ptr[g])))
        self.node_ptr, self.edge_ptr = node_ptr, edge_ptr
        self._x, self._edge_index, self._edge_weight, self._y = x, ei.astype(np.int32), w, y
        self._dev = None
        if torch.cuda.is_available():
            self._resident()

    def __len__(self):
        return int(self.node_ptr.shape[0]) - 1

    @property
    def num_features(self):
        return int(self._x.shape[1])

    def graph(self, i):
        """The Graph of entry i, in its own (local) node ids, as numpy."""
        i = int(self._check_ids(np.asarray([i]))[0])
        n0, n1, e0, e1 = self.node_ptr[i], self.node_ptr[i + 1], self.edge_ptr[i], self.edge_ptr[i + 1]
        return Graph(self._x[n0:n1], self._edge_index[:, e0:e1] - np.int32(n0), y=None if self._y is None else self._y[i:i + 1],
                     edge_weight=self._edge_weight[e0:e1])

    # ---- host side --------------------------------------------------------------------------------------------------
    def _check_ids(self, ids):
        ids = np.asarray(ids).reshape(-1)
        if ids.size and not np.issubdtype(ids.dtype, np.integer):
            raise IndexError("graph ids must be integers, got {}".format(ids.dtype))
        ids = ids.astype(np.int64)
        bad = (ids < 0) | (ids >= len(self))
        if bad.any():
            raise IndexError("graph id {} (position {} of the batch) is outside [0, {})".format(
                int(ids[bad][0]), int(np.nonzero(bad)[0][0]), len(self)))
        return ids

    def batch_table(self, graph_ids):
        """(table int32 [4, B + 1], n_out, e_out) of a batch: the columns src_node_begin, out_node_ptr, src_edge_begin,
        out_edge_ptr of include/tfgx_collate.h (entry B of the two begin columns is 0).  numpy on the ptr arrays only;
        IndexError for an id outside the store, ValueError for a batch whose sizes leave int32."""
        ids = self._check_ids(graph_ids)
        B = int(ids.shape[0])
        table = np.zeros((4, B + 1), dtype=np.int64)
        table[0, :B] = self.node_ptr[ids]
        table[1, 1:] = np.cumsum(self.node_ptr[ids + 1] - self.node_ptr[ids])
        table[2, :B] = self.edge_ptr[ids]
        table[3, 1:] = np.cumsum(self.edge_ptr[ids + 1] - self.edge_ptr[ids])
        n_out, e_out = int(table[1, B]), int(table[3, B])
        if n_out >= _INT32_LIMIT or e_out >= _INT32_LIMIT or B >= _INT32_LIMIT:
            raise ValueError("a batch of {} graphs, {} nodes and {} edges does not fit int32".format(B, n_out, e_out))
        return table.astype(np.int32), n_out, e_out

    # ---- device side ------------------------------------------------------------------------------------------------
    def _resident(self):
        """The packed arrays and the dataset's two plans on the device (made once)."""
        if self._dev is None:
            dev = L.device()
            up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)      # noqa: E731
            d = {"x": up(self._x), "ei": up(self._edge_index), "w": up(self._edge_weight),
                 "y": None if self._y is None else up(self._y), "device": dev}
            n = int(self.node_ptr[-1])
            d["plan"] = CsrPlan.build(d["ei"], n, n)
            d["plan_t"] = CsrPlan.build(torch.stack([d["ei"][1], d["ei"][0]]), n, n)
            d["arange"] = torch.arange(n + 1, dtype=torch.int32, device=dev)      # identity index arrays are views of it
            d["node_ptr"], d["edge_ptr"] = up(self.node_ptr.astype(np.int32)), up(self.edge_ptr.astype(np.int32))   # collate_static
            self._dev = d
        return self._dev

    def collate(self, graph_ids):
        """The BatchGraph (device tensors) of the graphs `graph_ids`, in that order; repeats are allowed, and so are graphs
        without nodes or without edges.  `graph_ids` is a host sequence or numpy array; a DEVICE tensor is brought to the host
        first, which synchronises once — the only form of this call that does.

        The batch carries its plans: the by-destination plan is attached to ``edge_index`` (with the by-source plan as its
        transposed plan, both ways) and kept in ``batch.cache``, where the graph plan over ``node_graph_index`` sits too, so
        CsrPlan.from_cache, plan.transposed() and the readouts' graph plan find what they look for and nothing sorts."""
        if isinstance(graph_ids, torch.Tensor):
            graph_ids = graph_ids.cpu().numpy()          # the documented synchronisation
        table, n_out, e_out = self.batch_table(graph_ids)                 # IndexError before any device work
        ids = np.asarray(graph_ids).reshape(-1)
        B = int(ids.shape[0])
        lib = L.require_gpu()
        d = self._resident()
        dev = d["device"]
        # one transfer: the four table columns and, behind them, the graph ids (for y); pinned, so the copy is asynchronous
        staged = torch.empty((5, B + 1), dtype=torch.int32, pin_memory=True)
        host = staged.numpy()
        host[:4] = table
        host[4, :B] = ids
        host[4, B] = 0
        tab = staged.to(dev, non_blocking=True)

        F = self.num_features
        i32 = dict(dtype=torch.int32, device=dev)
        x = torch.empty((n_out, F), dtype=torch.float32, device=dev)
        ei = torch.empty((2, e_out), **i32)
        ngi, egi = torch.empty(n_out, **i32), torch.empty(e_out, **i32)
        w = torch.empty(e_out, dtype=torch.float32, device=dev)
        plans, ios = [], []
        for parent in (d["plan"], d["plan_t"]):
            row_ptr, col, perm = torch.empty(n_out + 1, **i32), torch.empty(e_out, **i32), torch.empty(e_out, **i32)
            io = L.CollatePlan()
            io.ds_row_ptr, io.ds_col, io.ds_perm = parent.row_ptr.data_ptr(), parent.col.data_ptr(), parent.perm.data_ptr()
            io.out_row_ptr, io.out_col, io.out_perm = row_ptr.data_ptr(), col.data_ptr(), perm.data_ptr()
            ios.append(io)
            plans.append(CsrPlan(row_ptr, col, perm, n_out, n_out, e_out))
        a = L.CollateArgs()
        a.ds_x, a.ds_ldx, a.F = d["x"].data_ptr(), max(F, 1), F
        a.ds_row, a.ds_col, a.ds_w = d["ei"].data_ptr(), d["ei"].data_ptr() + 4 * int(d["ei"].shape[1]), d["w"].data_ptr()
        a.ds_n, a.ds_e = int(self.node_ptr[-1]), int(self.edge_ptr[-1])
        a.table, a.B, a.n_out, a.e_out = tab.data_ptr(), B, n_out, e_out
        a.out_x, a.out_ldx, a.out_node_graph_index = x.data_ptr(), max(F, 1), ngi.data_ptr()
        a.out_row, a.out_col, a.out_edge_graph_index, a.out_w = ei.data_ptr(), ei.data_ptr() + 4 * e_out, egi.data_ptr(), w.data_ptr()
        a.plan, a.plan_t = ctypes.pointer(ios[0]), ctypes.pointer(ios[1])
        L.check(lib.tfgx_collate(ctypes.byref(a), L.stream_ptr()), "tfgx_collate")

        y = None if d["y"] is None else d["y"].index_select(0, tab[4, :B])
        batch = BatchGraph(x, ei, ngi, egi, y=y, edge_weight=w)
        batch._num_graphs = B
        plan, plan_t = plans
        plan._edge_index = ei
        plan._transposed, plan_t._transposed = plan_t, plan
        attach_plan(ei, plan)
        batch.cache[CACHE_KEY_PLAN] = plan
        # the graph plan (rows = graphs, col = node ids) of a batch in graph order: out_node_ptr and the identity
        if d["arange"].shape[0] < n_out + 1:
            d["arange"] = torch.arange(2 * (n_out + 1), **i32)
        nodes = d["arange"][:n_out]
        from ..nn.pool.common_pool import CACHE_KEY_GRAPH_PLAN
        graph_plan = CsrPlan(tab[1], nodes, nodes, B, max(n_out, 1), n_out)
        graph_plan._longest_row = int(np.diff(np.asarray(table[1])).max(initial=0))      # host arithmetic: nn.sort_pool_3d's route
        if n_out > 0:       # its flip has one edge per row, in row order: identity row_ptr and perm, col = the graph ids
            graph_plan._transposed = CsrPlan(d["arange"][:n_out + 1], ngi, nodes, n_out, B, n_out)
            graph_plan._transposed._transposed = graph_plan
        else:
            graph_plan._edge_index = torch.stack([ngi, nodes])
        batch.cache[CACHE_KEY_GRAPH_PLAN] = (ngi, ngi._version, graph_plan)
        return batch

    def batches(self, batch_size, shuffle=False, seed=None, drop_last=False):
        """One epoch of collated batches of `batch_size` graphs; shuffle=True draws the order from numpy's PCG64(seed)."""
        batch_size = int(batch_size)
        if batch_size < 1:
            raise ValueError("batch_size must be at least 1")
        order = np.arange(len(self))
        if shuffle:
            order = np.random.Generator(np.random.PCG64(seed)).permutation(len(self))
        for i in range(0, len(self), batch_size):
            ids = order[i:i + batch_size]
            if drop_last and ids.shape[0] < batch_size:
                return
            yield self.collate(ids)

    # ---- fixed-shape batches (include/tfgx_collate_static.h): no host read, hipGraph-capturable ------------------------------
    def static_capacities(self, batch_size, max_nodes=None, max_edges=None, sink_degree=32):
        """StaticBatchCapacities of collate_static for `batch_size` slots: host arithmetic on node_ptr / edge_ptr, no device.
        The defaults are the worst case — max_nodes = the sum of the batch_size largest node counts of the store, max_edges
        likewise for edges —, so no batch of distinct graphs overflows; smaller values pad less and drop the slots that do not
        fit (flagged; StaticBatchGraph.check).  ValueError for a negative or non-integer argument, sink_degree < 1, and sizes
        that leave int32."""
        for name, v, low in (("batch_size", batch_size, 0), ("sink_degree", sink_degree, 1)) + tuple(
                (n, v, 0) for n, v in (("max_nodes", max_nodes), ("max_edges", max_edges)) if v is not None):
            if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or v < low:
                raise ValueError("static_capacities: {} must be an integer of at least {}, got {!r}".format(name, low, v))
        B = int(batch_size)

        def largest(ptr):
            sizes = np.sort(np.diff(ptr))[::-1]
            return int(sizes[:B].sum())

        max_nodes = largest(self.node_ptr) if max_nodes is None else int(max_nodes)
        max_edges = largest(self.edge_ptr) if max_edges is None else int(max_edges)
        sinks = max(1, -(-max_edges // int(sink_degree)))
        if max_nodes + sinks >= _INT32_LIMIT or max_edges >= _INT32_LIMIT or B > L.COLLATE_STATIC_MAX_SLOTS:
            raise ValueError("static_capacities: {} slots, {} nodes + {} sinks and {} edges: more than collate_static indexes "
                             "(int32 sizes, at most {} slots)".format(B, max_nodes, sinks, max_edges, L.COLLATE_STATIC_MAX_SLOTS))
        return StaticBatchCapacities(B, max_nodes, max_edges, int(sink_degree), sinks, max_nodes + sinks, max_edges)

    def _max_degrees(self):
        """(largest in-degree, largest out-degree) over the whole dataset: host work, once."""
        if getattr(self, "_degrees", None) is None:
            n = int(self.node_ptr[-1])
            ei = self._edge_index
            self._degrees = tuple(int(np.bincount(ei[k], minlength=1).max()) if ei.shape[1] and n else 0 for k in (0, 1))
        return self._degrees

    def _max_graph_nodes(self):
        """The node count of the store's largest graph: host work, once (nn.sag_pool_static holds it to the selection's cap)."""
        if getattr(self, "_largest_graph", None) is None:
            self._largest_graph = int(np.diff(self.node_ptr).max(initial=0))
        return self._largest_graph

    def _static_ids(self, ids, dev):
        """int32 ids on the device without a read: an id wider than int32 is clamped to an out-of-range int32 first (the
        kernel then flags it as it flags any other)."""
        if not isinstance(ids, torch.Tensor):
            if torch.cuda.is_current_stream_capturing():
                raise RuntimeError("GraphStore.collate_static: host graph ids inside a hipGraph capture would be frozen into the "
                                   "graph: pass a device tensor that the captured function fills (StaticLoader.next_ids)")
            ids = np.asarray(ids).reshape(-1)
            if ids.size and not np.issubdtype(ids.dtype, np.integer):
                raise IndexError("graph ids must be integers, got {}".format(ids.dtype))
            ids = torch.from_numpy(np.ascontiguousarray(ids.astype(np.int64))).to(dev)
        if ids.dtype not in (torch.int32, torch.int64):
            raise IndexError("graph ids must be int32 or int64, got {}".format(ids.dtype))
        if ids.device != dev:
            raise ValueError("GraphStore.collate_static: ids live on {}, the store on {}".format(ids.device, dev))
        ids = ids.detach().reshape(-1)
        if ids.dtype != torch.int32:
            ids = ids.clamp(min=-2, max=len(self)).to(torch.int32)
        return ids.contiguous()

    def _static_outputs(self, d, n_cap, e_cap):
        """The output tensors of a batch of n_cap rows and e_cap edges, its two (still unlinked) plans and the CollatePlan
        records that point the kernel at the dataset's plans and at theirs: (x, ei, ngi, egi, w, plans, ios)."""
        dev, F = d["device"], self.num_features
        i32 = dict(dtype=torch.int32, device=dev)
        x = torch.empty((n_cap, F), dtype=torch.float32, device=dev)
        ei = torch.empty((2, e_cap), **i32)
        ngi, egi = torch.empty(n_cap, **i32), torch.empty(e_cap, **i32)
        w = torch.empty(e_cap, dtype=torch.float32, device=dev)
        plans, ios = [], []
        for parent in (d["plan"], d["plan_t"]):
            row_ptr, col, perm = torch.empty(n_cap + 1, **i32), torch.empty(e_cap, **i32), torch.empty(e_cap, **i32)
            io = L.CollatePlan()
            io.ds_row_ptr, io.ds_col, io.ds_perm = parent.row_ptr.data_ptr(), parent.col.data_ptr(), parent.perm.data_ptr()
            io.out_row_ptr, io.out_col, io.out_perm = row_ptr.data_ptr(), col.data_ptr(), perm.data_ptr()
            ios.append(io)
            plans.append(CsrPlan(row_ptr, col, perm, n_cap, n_cap, e_cap))
        return x, ei, ngi, egi, w, plans, ios

    @staticmethod
    def _identity(d, n):
        """The first n entries of the store's identity index array, grown when it is too short — never inside a hipGraph
        capture: the new array would live in the graph's private pool while the store goes on using it eagerly."""
        if d["arange"].shape[0] < n:
            if torch.cuda.is_current_stream_capturing():
                raise RuntimeError("GraphStore.collate_static: these capacities need a longer identity array than the store "
                                   "holds, and it cannot be made inside a hipGraph capture: call collate_static once eagerly "
                                   "with the same capacities first (the warm-up of CapturedTrainStep does)")
            d["arange"] = torch.arange(2 * n, dtype=torch.int32, device=d["device"])
        return d["arange"][:n]

    def collate_static(self, ids, capacities=None):
        """The StaticBatchGraph of the B = len(ids) slots `ids`: a device int32 / int64 tensor of graph ids, -1 for a dead slot
        (a host sequence is uploaded when eager and refused inside a capture).  Every output has the size `capacities` says
        (default: static_capacities(B)), whatever the ids are, so the call makes no host read, uses no pinned staging, and can
        be captured in a hipGraph; two launches (include/tfgx_collate_static.h, where the layout is written down).

        The live rows and edges are bit for bit what collate(live ids in slot order) gives, with the slot number as the graph
        index; padded rows are zero and belong to the dead graph B (num_graphs == B + 1); padded edges are unit self-loops on
        the dead sink rows.  An id outside [-1, G) and a slot that does not fit the capacities become dead slots and raise a
        flag that StaticBatchGraph.check() reads.  y has one row per slot (a dead slot holds graph 0's label: mask it).

        All three plans are attached and cached as collate does.  Where the dataset's largest in- / out-degree and the sink
        degree are within plan.hub_policy's threshold for these capacities, both edge plans are marked as having no hub rows
        and no walk order, so neither is computed or read back; otherwise both stay lazy and the first eager layer call on
        the batch reads a count back.  The graph plan is always marked so (the dead graph is its one long row; it is walked
        inline, same sums)."""
        from ..plan import hub_policy
        from ..nn.pool.common_pool import CACHE_KEY_GRAPH_PLAN
        lib = L.require_gpu()
        d = self._resident()
        dev = d["device"]
        given = ids if isinstance(ids, torch.Tensor) else None
        ids = self._static_ids(ids, dev)
        B = int(ids.shape[0])
        cap = self.static_capacities(B) if capacities is None else capacities
        if cap.batch_size != B:
            raise ValueError("collate_static: capacities for {} slots, {} ids".format(cap.batch_size, B))
        G, F = len(self), self.num_features
        n_cap, e_cap = cap.n_cap, cap.e_cap
        i32 = dict(dtype=torch.int32, device=dev)
        stream = L.stream_ptr()
        table = torch.empty((4, B + 1), **i32)
        mask = torch.empty(B, dtype=torch.bool, device=dev)
        counts = torch.empty(4, **i32)
        L.check(lib.tfgx_static_batch_table(L.ptr(ids), B, L.ptr(d["node_ptr"]), L.ptr(d["edge_ptr"]), G, cap.max_nodes,
                                              cap.max_edges, L.ptr(table), L.ptr(mask), L.ptr(counts), stream),
                "tfgx_static_batch_table")

        x, ei, ngi, egi, w, plans, ios = self._static_outputs(d, n_cap, e_cap)
        graph_row_ptr = torch.empty(B + 2, **i32)
        a = L.CollateStaticArgs()
        a.ds_x, a.ds_ldx, a.F = d["x"].data_ptr(), max(F, 1), F
        a.ds_row, a.ds_col, a.ds_w = d["ei"].data_ptr(), d["ei"].data_ptr() + 4 * int(d["ei"].shape[1]), d["w"].data_ptr()
        a.ds_n, a.ds_e = int(self.node_ptr[-1]), int(self.edge_ptr[-1])
        a.table, a.B = table.data_ptr(), B
        a.n_cap, a.e_cap, a.sinks, a.sink_degree = n_cap, e_cap, cap.sinks, cap.sink_degree
        a.out_x, a.out_ldx, a.out_node_graph_index = x.data_ptr(), max(F, 1), ngi.data_ptr()
        a.out_row, a.out_col, a.out_edge_graph_index, a.out_w = ei.data_ptr(), ei.data_ptr() + 4 * e_cap, egi.data_ptr(), w.data_ptr()
        a.plan, a.plan_t = ctypes.pointer(ios[0]), ctypes.pointer(ios[1])
        a.graph_row_ptr = graph_row_ptr.data_ptr()
        L.check(lib.tfgx_static_batch(ctypes.byref(a), stream), "tfgx_static_batch")

        y = None
        if d["y"] is not None:
            if G > 0:
                y = d["y"].index_select(0, ids.clamp(min=0, max=G - 1))     # an id is never an index before it is held in range
            else:
                y = d["y"].new_zeros((B,) + tuple(d["y"].shape[1:]))
        batch = StaticBatchGraph(x, ei, ngi, egi, y, w, ids, mask, counts, cap, G, given_ids=given)
        batch._store, batch.graph_row_ptr = self, graph_row_ptr
        plan, plan_t = plans
        plan._edge_index = ei
        plan._transposed, plan_t._transposed = plan_t, plan
        thr, _ = hub_policy(e_cap, n_cap)
        if max(max(self._max_degrees()), cap.sink_degree) <= thr:
            for pl in plans:
                pl.hub_threshold, pl._hub, pl._row_order = thr, False, False
        attach_plan(ei, plan)
        batch.cache[CACHE_KEY_PLAN] = plan
        # the graph plan over B + 1 graphs: the slots' output offsets closed with n_cap, identity columns
        arange = self._identity(d, n_cap + 1)
        nodes = arange[:n_cap]
        graph_plan = CsrPlan(graph_row_ptr, nodes, nodes, B + 1, n_cap, n_cap)
        graph_plan._transposed = CsrPlan(arange, ngi, nodes, n_cap, B + 1, n_cap)
        graph_plan._transposed._transposed = graph_plan
        for pl, rows in ((graph_plan, B + 1), (graph_plan._transposed, n_cap)):
            pl.hub_threshold, pl._hub, pl._row_order = hub_policy(n_cap, rows)[0], False, False
        batch.cache[CACHE_KEY_GRAPH_PLAN] = (ngi, ngi._version, graph_plan)
        return batch

    def static_loader(self, batch_size, shuffle=False, seed=None, drop_last=False):
        """A StaticLoader over this store: the epoch order of `batches` (same arguments), held on the device."""
        return StaticLoader(self, batch_size, shuffle=shuffle, seed=seed, drop_last=drop_last)


class StaticLoader(object):
    """Graph ids for collate_static, drawn on the device.  `order` int32 holds one epoch — what GraphStore.batches walks
    (arange, or PCG64(seed).permutation) — padded with -1 to a multiple of batch_size (drop_last=True: cut to one);
    `cursor` is an int64 device word.

        ids = loader.next_ids()      # order[(cursor + arange(B)) % len(order)], then cursor += B

    is torch device ops only: it can be captured in a hipGraph, and every replay hands on the next batch (the epoch wraps).
    reshuffle(seed) writes a new order in place (eager: it uploads), so a captured step follows it."""

    def __init__(self, store, batch_size, shuffle=False, seed=None, drop_last=False):
        batch_size = int(batch_size)
        if batch_size < 1:
            raise ValueError("batch_size must be at least 1")
        self.store, self.batch_size, self.shuffle, self.drop_last = store, batch_size, bool(shuffle), bool(drop_last)
        G = len(store)
        self.steps_per_epoch = G // batch_size if drop_last else -(-G // batch_size)
        if self.steps_per_epoch < 1:
            raise ValueError("static_loader: {} graphs give no batch of {}{}".format(G, batch_size,
                                                                                     " with drop_last" if drop_last else ""))
        dev = store._resident()["device"]
        self.order = torch.empty(self.steps_per_epoch * batch_size, dtype=torch.int32, device=dev)
        self.cursor = torch.zeros(1, dtype=torch.int64, device=dev)
        self._lane = torch.arange(batch_size, dtype=torch.int64, device=dev)
        self.reshuffle(seed)

    def _host_order(self, seed):
        G, n = len(self.store), self.steps_per_epoch * self.batch_size
        order = np.arange(G)
        if self.shuffle:
            order = np.random.Generator(np.random.PCG64(seed)).permutation(G)
        out = np.full(n, -1, dtype=np.int32)
        out[:min(G, n)] = order[:n]
        return out

    def reshuffle(self, seed=None):
        """A new epoch order (shuffle=False: the same one), written IN PLACE; the cursor is left where it is."""
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError("StaticLoader.reshuffle uploads a host permutation: call it between replays, not inside a capture")
        self.order.copy_(torch.from_numpy(self._host_order(seed)))
        return self

    def next_ids(self):
        """int32 [batch_size] on the device: the next batch's graph ids (-1 pads a short last batch); advances the cursor."""
        ids = self.order[(self.cursor + self._lane) % int(self.order.shape[0])]
        self.cursor.add_(self.batch_size)
        return ids
