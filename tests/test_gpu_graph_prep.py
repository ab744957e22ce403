# coding=utf-8
"""The once-per-graph kernels against float64, on the GPU: the forward GCN normalisation (tfgx_segment_weight_sum_f32 and
tfgx_gcn_norm_edges_f32, csrc/tfgx_norm.hip) on its short-row, long-row, second-grid-trip, rectangular and degenerate paths, and
the duplicate-edge merge (tfgx_merge_duplicated_edges, csrc/tfgx_plan.hip) with the utilities built on it.  Draws, references,
comparators and the derivation of every bar: tests/graph_prep_cases.py; tests/test_graph_prep_cases.py shows on the CPU that the
draws reach every path and that the comparators reject planted errors.

Normalised weights are held RELATIVELY (16 * 2^-24 |ref| on exact degrees, the degree bars on top for uniform weights): a hub's
weights are about 1 / degree, where the absolute 1e-5 of assert_parity would be a bar of several per cent."""
import numpy as np
import pytest
import torch

import graph_prep_cases as gp
import normgrad_mirror as nm

pytestmark = pytest.mark.gpu


def _dev(a):
    return torch.from_numpy(np.array(a)).cuda()          # (a copy: the module's weight arrays are read-only)


def _nan_filled(n):
    return torch.full((n,), gp.NAN_BITS, dtype=torch.int32, device="cuda").view(torch.float32)


def _host(t):
    return None if t is None else t.cpu().numpy()


# ---- A. normalisation ------------------------------------------------------------------------------------------------------------
_GRAPHS = {}


class _OnDevice(object):
    """A draw's edge list, its plan (built once) and an unweighted SparseMatrix that lends the plan to the public route."""

    def __init__(self, d):
        from tf_geometric_amd.sparse import SparseMatrix
        self.d = d
        self.ei = _dev(np.stack([d["row"], d["col"]]))
        self.adj = SparseMatrix(self.ei, None, [d["n_rows"], d["n_cols"]])
        self.plan = self.adj.plan
        self.perm = self.plan.perm.cpu().numpy().astype(np.int64)
        E = d["row"].size
        assert self.plan.num_edges == E and self.perm.shape == (E,)
        if E:
            assert np.array_equal(np.sort(self.perm), np.arange(E))

    def to_caller_order(self, csr_values, total):
        out = np.empty(total, np.float32)
        E = self.perm.size
        out[self.perm] = csr_values[:E]
        out[E:] = csr_values[E:]
        return out


def _graph(d):
    if d["name"] not in _GRAPHS:
        _GRAPHS[d["name"]] = _OnDevice(d)
    return _GRAPHS[d["name"]]


def _raw(g, w, cfg):
    """The two C entry points called as autograd.gcn_norm_forward calls them, into NaN-filled buffers with a guard behind."""
    from tf_geometric_amd import _lib as L
    lib = L.require_gpu()
    norm, sym, asl, renorm, improved = cfg
    fill, diag = gp.fill_diag(cfg)
    plan = g.plan
    n, E = plan.n_dst, plan.num_edges
    wt = None if w is None else _dev(w)
    w_csr = None if wt is None else plan.edge_attr_to_csr(wt)
    row_deg = _nan_filled(n)
    L.check(lib.tfgx_segment_weight_sum_f32(L.ptr(plan.row_ptr), L.ptr(w_csr), n, diag, L.ptr(row_deg), L.stream_ptr()),
            "tfgx_segment_weight_sum_f32")
    col_deg = None
    if norm == "both" and not sym:
        tplan = plan.transposed()
        tw = None if wt is None else tplan.edge_attr_to_csr(wt)
        col_deg = _nan_filled(tplan.n_dst)
        L.check(lib.tfgx_segment_weight_sum_f32(L.ptr(tplan.row_ptr), L.ptr(tw), tplan.n_dst, diag, L.ptr(col_deg),
                                                L.stream_ptr()), "tfgx_segment_weight_sum_f32")
    w_out, self_coef = _nan_filled(E + gp.GUARD), _nan_filled(n + gp.GUARD)
    L.check(lib.tfgx_gcn_norm_edges_f32(L.ptr(plan.row_ptr), L.ptr(plan.col), L.ptr(w_csr), n, L.ptr(row_deg), L.ptr(col_deg),
                                        L.NORM_MODES[norm], fill, int(asl), int(renorm), L.ptr(w_out), L.ptr(self_coef),
                                        L.stream_ptr()), "tfgx_gcn_norm_edges_f32")
    return dict(row_deg=_host(row_deg), col_deg=_host(col_deg), w_out=g.to_caller_order(_host(w_out), E + gp.GUARD),
                self_coef=_host(self_coef))


def _public(g, w, cfg):
    from tf_geometric_amd.nn.conv.gcn import gcn_norm_adj
    norm, sym, asl, renorm, improved = cfg
    adj = g.adj.with_value(None if w is None else _dev(w))
    normed = gcn_norm_adj(adj, norm=norm, add_self_loop=asl, sym=sym, renorm=renorm, improved=improved)
    assert normed.plan is g.plan and list(normed.shape) == [g.d["n_rows"], g.d["n_cols"]]
    E = g.perm.size
    assert tuple(normed.w_csr.shape) == (E,) and normed.w_csr.dtype == torch.float32
    return normed, dict(w_out=g.to_caller_order(_host(normed.w_csr), E), self_coef=_host(normed.self_coef))


def _same_bits(a, b, what):
    for k in ("row_deg", "col_deg", "w_out", "self_coef"):
        if a.get(k) is None and b.get(k) is None:
            continue
        assert np.array_equal(gp._bits(a[k]), gp._bits(b[k])), "{}: {} differs in bits".format(what, k)


def _dense(d, normed):
    sm = normed.to_sparse_matrix()
    index, value = sm.index.cpu().numpy(), sm.value.cpu().numpy().astype(np.float64)
    out = np.zeros((d["n_rows"], d["n_cols"]))
    np.add.at(out, (index[0], index[1]), value)
    return out


@pytest.mark.parametrize("mode", gp.WEIGHT_MODES)
@pytest.mark.parametrize("name", gp.NORM_DRAWS)
def test_normalisation_forward_against_float64(tfg, name, mode):
    """Every legal configuration, raw C entry points and gcn_norm_adj, on one draw with one kind of weights."""
    d = gp.norm_draw(name)
    g = _graph(d)
    w = gp.weights(d, mode)
    exact = gp.exact_mode(mode)
    E, n = d["row"].size, d["n_rows"]
    worst, differ, elements = {}, 0, 0
    for cfg in gp.configs_for(d):
        what = "{} {} {}".format(name, mode, nm.config_id(cfg))
        ref = gp.reference(d, w, cfg)
        raw = _raw(g, w, cfg)
        stats = gp.compare(raw, ref, exact, what=what + " raw")
        for k, v in stats.items():
            worst[k] = max(worst.get(k, 0.0), v)
        differ += gp.bit_differences(raw, gp.f32_eval(d, w, cfg))
        elements += E + n + n + (0 if raw["col_deg"] is None else d["n_cols"])
        _same_bits(raw, _raw(g, w, cfg), what + " run to run")

        normed, public = _public(g, w, cfg)
        gp.compare(public, ref, exact, what=what + " public", guard=False)
        assert np.array_equal(gp._bits(public["w_out"]), gp._bits(raw["w_out"][:E])), what + ": public w_csr != raw"
        if cfg[2]:
            assert np.array_equal(gp._bits(public["self_coef"]), gp._bits(raw["self_coef"][:n])), what + ": public self_coef != raw"
        if name in gp.SMALL_DRAWS:
            A, B = gp.dense_reference(d, ref, exact)
            got = _dense(d, normed)
            assert got.shape == A.shape and np.isfinite(got).all() and (np.abs(got - A) <= B).all(), what + " dense"
    print("{} {}: worst error / bar {}; {} of {} elements differ in bits from the float32 numpy evaluation".format(
        name, mode, {k: round(v, 3) for k, v in sorted(worst.items())}, differ, elements))


@pytest.mark.parametrize("name", gp.IDENTITY_DRAWS)
def test_exact_degrees_make_every_value_a_function_of_its_operands(tfg, name):
    """Quantised weights: an edge's value depends on (deg_r, w, deg_c) alone, so neither the order of the caller's edge list nor
    the names of the nodes (which move long rows between tiles and next to other rows) may change a bit."""
    d = gp.norm_draw(name)
    w = gp.weights(d, "quantised")
    E, n = d["row"].size, d["n_rows"]
    de, q = gp.permuted_edges(d)
    dn, p = gp.relabelled(d)
    g, ge, gn = _graph(d), _OnDevice(de), _OnDevice(dn)
    wq = np.ascontiguousarray(w[q])
    for cfg in gp.configs_for(d):
        what = "{} {}".format(name, nm.config_id(cfg))
        base, moved, named = _raw(g, w, cfg), _raw(ge, wq, cfg), _raw(gn, w, cfg)
        assert np.array_equal(gp._bits(moved["w_out"][:E]), gp._bits(base["w_out"][:E][q])), what + ": edge order"
        assert np.array_equal(gp._bits(moved["self_coef"]), gp._bits(base["self_coef"])), what + ": edge order, self_coef"
        assert np.array_equal(gp._bits(named["w_out"]), gp._bits(base["w_out"])), what + ": node names"
        assert np.array_equal(gp._bits(named["self_coef"][:n][p]), gp._bits(base["self_coef"][:n])), what + ": node names, self_coef"
        assert np.array_equal(gp._bits(named["row_deg"][p]), gp._bits(base["row_deg"])), what + ": node names, degrees"


# ---- B. duplicate-edge merge -------------------------------------------------------------------------------------------------------
def _merge_case(tfg, what, ei, props, inputs=("tensor", "numpy"), derived=True):
    for kind in inputs:
        as_np = kind == "numpy"
        ei_in = ei if as_np else _dev(ei)
        u, none = tfg.utils.merge_duplicated_edge(ei_in)
        assert none is None and isinstance(u, np.ndarray if as_np else torch.Tensor)
        for prop in props:
            ref_u, ref_props, tol = gp.merge_reference(ei, prop, gp.MODES)
            gp.check_merged("{} {} (no props)".format(what, kind), u if as_np else _host(u), ref_u)
            p_in = prop if as_np else _dev(prop)
            u2, merged = tfg.utils.merge_duplicated_edge(ei_in, [p_in] * 4, list(gp.MODES))
            assert all(isinstance(m, np.ndarray if as_np else torch.Tensor) for m in merged)
            gp.check_merged("{} {}".format(what, kind), u2 if as_np else _host(u2), ref_u)
            gp.check_props("{} {} {}".format(what, kind, prop.shape), [m if as_np else _host(m) for m in merged], ref_props, tol)
        if not derived:
            continue
        from conftest import assert_parity
        w = props[0]
        assert w.ndim == 1
        w_in = w if as_np else _dev(w)
        up_ref, uw_ref, de_ref, dw_ref, tol = gp.upper_reference(ei, w)
        up, (uw,) = tfg.utils.convert_edge_to_upper(ei_in, [w_in])
        gp.check_merged("{} {} upper".format(what, kind), up if as_np else _host(up), up_ref)
        assert_parity(uw if as_np else _host(uw), uw_ref, tol=tol, what=what + " upper weights")
        props_in = [w_in]
        de, dprops = tfg.utils.convert_edge_to_directed(ei_in, props_in)
        if de_ref is None:
            assert de is ei_in and dprops is props_in, what + ": an all-self-loop list comes back as it went in"
        else:
            gp.check_merged("{} {} directed".format(what, kind), de if as_np else _host(de), de_ref)
            assert_parity(dprops[0] if as_np else _host(dprops[0]), dw_ref, tol=tol, what=what + " directed weights")


@pytest.mark.parametrize("n", gp.HASH_N)
def test_merge_hash_widths(tfg, n):
    """n * n below, between, at and above 2^31 and 2^32, and at 62 bits; the edge (n - 1, n - 1) present and duplicated."""
    ei = gp.hash_draw(n)
    _merge_case(tfg, "n={}".format(n), ei, [gp.props_for(ei), gp.props_for(ei, 3, seed=1)])


@pytest.mark.parametrize("mix", gp.MIXES)
@pytest.mark.parametrize("E", gp.EDGE_COUNTS)
def test_merge_edge_counts(tfg, E, mix):
    ei = gp.edge_draw(E, mix)
    small = E <= 70001
    props = [gp.props_for(ei)] + ([gp.props_for(ei, 3, seed=1)] if small else [])
    _merge_case(tfg, "E={} {}".format(E, mix), ei, props, inputs=("tensor", "numpy") if small else ("tensor",))


def test_merge_of_a_hub_group_takes_the_hub_route(tfg):
    """3000 copies of one edge under a forced hub policy: the property merge's segment_reduce walks that group chunk by chunk."""
    import tf_geometric_amd.plan as P
    ei = gp.hub_draw()
    key = ei[0].astype(np.int64) * (int(ei.max()) + 1) + ei[1]
    _, first, inv = np.unique(key, return_index=True, return_inverse=True)
    rank = np.empty(first.size, np.int64)
    rank[np.argsort(first, kind="stable")] = np.arange(first.size)
    uidx = rank[inv.reshape(-1)].astype(np.int32)
    old = P.HUB_THRESHOLD, P.HUB_CHUNK
    try:
        P.HUB_THRESHOLD, P.HUB_CHUNK = 64, 48
        plan = P.CsrPlan.build(_dev(np.stack([uidx, np.arange(uidx.size, dtype=np.int32)])), first.size, uidx.size)
        hub = plan.hub_info()
        assert hub is not None and int(plan.in_degree().max().item()) >= gp.HUB_COPIES > 64
        _merge_case(tfg, "hub group", ei, [gp.props_for(ei), gp.props_for(ei, 3, seed=1)], derived=False)
    finally:
        P.HUB_THRESHOLD, P.HUB_CHUNK = old


def test_directed_of_self_loops_alone_returns_its_input(tfg):
    ei = np.array([[4, 4, 2, 0], [4, 4, 2, 0]], np.int32)
    w = np.array([1.0, 2.0, 3.0, 4.0], np.float32)
    for ei_in, props in ((ei, [w]), (_dev(ei), [_dev(w)])):
        out, out_props = tfg.utils.convert_edge_to_directed(ei_in, props)
        assert out is ei_in and out_props is props
        out, out_props = tfg.utils.convert_edge_to_directed(ei_in)
        assert out is ei_in and out_props is None
