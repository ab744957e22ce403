# coding=utf-8
"""GraphStore: a dataset of whole graphs held on the device, and minibatches assembled from it in one kernel launch
(include/tfgx_collate.h) — features, index arrays and all three CSR plans, with no sort and no host synchronisation.

A batch of whole graphs is block-diagonal, so its plans are the concatenation of its graphs' pieces of the dataset's plans
with the offsets exchanged.  The dataset's two plans (by destination, by source) are built once, when the store goes to the
device: the only sorts the dataset ever pays for."""
import ctypes

import numpy as np
import torch

from .. import _lib as L
from ..plan import CsrPlan, CACHE_KEY_PLAN, attach_plan
from .graph import Graph, BatchGraph

COLLATE_TILE = L.COLLATE_TILE        # output elements per workgroup of the collate kernel (TFGX_COLLATE_TILE)
_INT32_LIMIT = (1 << 31) - 1         # sizes the C ABI takes are below this


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
