# coding=utf-8
"""The GAT attention backward through the C ABI (include/tfgx.h, tfgx_gat_backward_args) on every layout the header
documents for a C caller — not only the head-block route the package itself takes (autograd.py:_GatAttention.backward):

  dense        q / stats_ml / dsum / grad_out separate arrays, ld_stats_ml = ld_dsum = 0
  interleaved  one row per destination [dO | Q | (m, l) | D] (tfgx_gat_pack_dst_f32), every pointer into it, stride P
  head-pack    tfgx_gat_pack_dst_heads_f32's table and tfgx_gat_backward_args.head_pack (source pass only)

through tfgx_gat_backward_{dst,src}_f32 and the *_hub_f32 forms (NULL lists and real ones), on the tuned kernels and on the
one-lane-per-(row, head) kernels.  Every route's dQ / dK / dV is held to torch autograd over a float64 restatement of the
attention (tests/f64_layers.py), and routes that read the same numbers must give the same bits."""
import ctypes
import math

import numpy as np
import pytest
import torch

from conftest import assert_parity

pytestmark = pytest.mark.gpu

FAST = [(1, 1, 8), (8, 1, 8), (4, 8, 16), (2, 16, 8), (2, 32, 64), (1, 4, 44)]     # (H, d, dv)
ONE_LANE = [(2, 3, 10), (3, 9, 9), (1, 2, 7), (2, 64, 8)]
NAN = float("nan")


def _roundup(v, m):
    return -(-v // m) * m


def fast_route(H, d, dv, ldv, ldgo, v_addr, go_addr, ldgv, gv_addr):
    """Python mirror of gat_bwd_fast_ok (tf_geometric_amd/csrc/tfgx_backward.hip): True = the tuned lane-group kernels."""
    lh = dv // 4
    d_ok = d in (1, 2, 4, 8, 16, 32)
    v_ok = dv % 4 == 0 and lh <= 64 and ((lh & (lh - 1)) == 0 or H == 1)
    al = ldv % 4 == 0 and ldgo % 4 == 0 and v_addr % 16 == 0 and go_addr % 16 == 0 and ldgv % 4 == 0 and gv_addr % 16 == 0
    return d_ok and v_ok and al


def _geom_route(H, d, dv):
    """Route of a geometry with dense, aligned tables."""
    return "fast" if fast_route(H, d, dv, H * dv, H * dv, 0, 0, H * dv, 0) else "onelane"


def _gid(g):
    return "{}-H{}d{}dv{}".format(_geom_route(*g), *g)


def _nan(*shape):
    return torch.full(shape, NAN, dtype=torch.float32, device="cuda")


class _Case(object):
    """A graph, the package's forward on it, dO, and the two packed destination tables."""

    def __init__(self, geom, variant, hubs=False, seed=0):
        from tf_geometric_amd import _lib as L
        import tf_geometric_amd.plan as P
        from tf_geometric_amd.autograd import _transposed
        from tf_geometric_amd.nn.conv.gat import gat_attention
        from test_gpu_backward import _keep_mask_host
        self.L, self.lib = L, L.require_gpu()
        H, d, dv = self.geom = geom
        self.variant = variant
        A, W = self.A, self.W = H * d, H * dv
        rng = np.random.Generator(np.random.PCG64(seed + 1000 * H + 10 * d + dv))
        n = self.n_dst = 200
        ns = self.n_src = 260 if variant == "rect" else n          # rect: sources [200, 260) are no destinations
        # plus a destination with 80 more in-edges and a source with 80 more out-edges: rows of several lane-group batches
        dst = [rng.integers(0, n, 3000), np.full(80, 7), rng.integers(0, n, 80)]
        src = [rng.integers(0, ns, 3000), rng.integers(0, ns, 80), np.full(80, 5)]
        if hubs:    # a 3000-in-edge destination and a 2500-out-edge source under a low threshold: both passes chunk-wise
            dst += [np.full(3000, 9), rng.integers(0, n, 2500)]
            src += [rng.integers(0, ns, 3000), np.full(2500, 4)]
        ei = np.stack([np.concatenate(dst), np.concatenate(src)]).astype(np.int32)
        old_policy = (P.HUB_THRESHOLD, P.HUB_CHUNK)
        if hubs:
            P.HUB_THRESHOLD, P.HUB_CHUNK = 64, 48
        try:
            self.plan = P.CsrPlan.build(L.as_i32(ei), n, ns)
            self.pt, self.t2d = _transposed(self.plan)
            hub_d, hub_s = self.plan.hub_info(), self.pt.hub_info()       # (memoised on the plans under this policy)
        finally:
            P.HUB_THRESHOLD, P.HUB_CHUNK = old_policy
        assert (hub_d is not None, hub_s is not None) == (hubs, hubs)
        self.E = E = self.plan.num_edges
        self.rate = 0.4 if variant == "dropout" else 0.0
        self.seed = (0x5EED1234 << 32) | (H * 100 + d)
        self.keep = None
        if self.rate > 0.0:
            self.keep = _keep_mask_host(self.seed, (E + n) * H, self.rate).reshape(E + n, H)

        def table(rows, cols):
            """[rows, cols] float32 on the GPU: dense, or a column slice of a wider table (strided variants)"""
            if variant == "strided":          # 16-byte aligned slice, ld % 4 == 0: the tuned kernels stay eligible
                off, ld = 4, _roundup(cols, 4) + 8
            elif variant == "strided_odd":    # ld % 4 != 0, 4-byte offset: the one-lane kernels
                off, ld = 1, _roundup(cols, 4) + 5
            else:
                off, ld = 0, cols
            t = torch.from_numpy(rng.standard_normal((rows, ld)).astype(np.float32)).cuda()
            return t[:, off:off + cols]

        self.Q, self.K, self.V, self.dO = table(n, A), table(ns, A), table(ns, W), table(n, W)
        self.ldq, self.ldk, self.ldv, self.ldgo = (int(t.stride(0)) for t in (self.Q, self.K, self.V, self.dO))
        self.stats = _nan(n, 2 * H)
        self.out = gat_attention(self.plan, self.Q, self.K, self.V, H, True, stats_ml=self.stats, drop_rate=self.rate,
                                 drop_seed=self.seed)
        assert not torch.isnan(self.stats).any()
        st = L.stream_ptr()
        # head-block table (the package's route): [dO | pad | per head: Q, m, 1 / (l + 1e-8), D, pad], one spare row
        self.HB, self.W4 = _roundup(d + 3, 4), _roundup(W, 4)
        self.Ph = _roundup(self.W4 + H * self.HB, 32)
        self.hpack_buf = _nan(n + 1, self.Ph)
        self.hpack = self.hpack_buf[:n]
        self.dsum = _nan(n, H)
        L.check(self.lib.tfgx_gat_pack_dst_heads_f32(L.ptr(self.dO), self.ldgo, L.ptr(self.out), W, L.ptr(self.Q), self.ldq,
                                                     L.ptr(self.stats), n, H, d, dv, L.ptr(self.hpack), self.Ph,
                                                     L.ptr(self.dsum), st), "tfgx_gat_pack_dst_heads_f32")
        # interleaved table [dO | Q | (m, l) | D], P = roundup32(W + A + 3H); its D column is replaced by the head-block
        # route's dsum, so that every route reads the same numbers (the 16-byte pack kernel sums D in another order)
        self.P = _roundup(W + A + 3 * H, 32)
        self.pack = _nan(n, self.P)
        dsum_i = _nan(n, H)
        L.check(self.lib.tfgx_gat_pack_dst_f32(L.ptr(self.dO), self.ldgo, L.ptr(self.out), W, L.ptr(self.Q), self.ldq,
                                               L.ptr(self.stats), n, H, d, dv, L.ptr(self.pack), self.P, L.ptr(dsum_i), st),
                "tfgx_gat_pack_dst_f32")
        assert_parity(dsum_i.cpu().numpy(), self.dsum.cpu().numpy(), tol=1e-5, what="pack D vs head-block D")
        self.pack[:, W + A + 2 * H:W + A + 3 * H] = self.dsum
        self.hub_d, self.nc_d = L.hub_lists(self.plan) if hubs else (None, 0)
        self.hub_s, self.nc_s = L.hub_lists(self.pt) if hubs else (None, 0)
        self._ref = None

    def args(self, layout):
        """tfgx_gat_backward_args as autograd.py fills it, with the inputs of `layout`"""
        L = self.L
        H, d, dv = self.geom
        a = L.GatBackwardArgs()
        a.row_ptr, a.col, a.n_dst = self.plan.row_ptr.data_ptr(), self.plan.col.data_ptr(), self.n_dst
        a.row_ptr_t, a.dst_t, a.n_src = self.pt.row_ptr.data_ptr(), self.pt.col.data_ptr(), self.pt.n_dst
        a.k, a.ldk, a.v, a.ldv = self.K.data_ptr(), self.ldk, self.V.data_ptr(), self.ldv
        a.H, a.d, a.dv, a.add_self_loop = H, d, dv, 1
        a.scale = math.sqrt(float(d))
        if self.rate > 0.0:
            from tf_geometric_amd.nn.conv.gat import _set_drop
            _set_drop(a, self.rate, self.seed, self.E)
            a.edge_pos_t = self.t2d.data_ptr()
        if layout == "interleaved":
            f = 4      # bytes per float
            base = self.pack.data_ptr()
            a.grad_out, a.ld_grad_out = base, self.P
            a.q, a.ldq = base + f * self.W, self.P
            a.stats_ml, a.ld_stats_ml = base + f * (self.W + self.A), self.P
            a.dsum, a.ld_dsum = base + f * (self.W + self.A + 2 * H), self.P
        else:
            a.q, a.ldq = self.Q.data_ptr(), self.ldq
            a.stats_ml, a.dsum = self.stats.data_ptr(), self.dsum.data_ptr()
            if layout == "head_pack":       # as autograd.py: dO out of the packed rows, q / stats_ml / dsum stay dense
                a.grad_out, a.ld_grad_out = self.hpack.data_ptr(), self.Ph
                a.head_pack, a.ld_head_pack = self.hpack.data_ptr() + 4 * self.W4, self.Ph
            else:
                assert layout == "dense"
                a.grad_out, a.ld_grad_out = self.dO.data_ptr(), self.ldgo
        return a

    def run(self, pass_, layout, entry):
        """(dQ,) of the destination pass or (dK, dV) of the source pass; entry: plain | hub_null | hub"""
        L, lib = self.L, self.lib
        a = self.args(layout)
        st = L.stream_ptr()
        if pass_ == "dst":
            gq = _nan(self.n_dst, self.A)
            a.grad_q, a.ld_grad_q = gq.data_ptr(), self.A
            route = fast_route(a.H, a.d, a.dv, a.ldv, a.ld_grad_out, a.v, a.grad_out, 0, 0)
            if entry == "plain":
                rc = lib.tfgx_gat_backward_dst_f32(ctypes.byref(a), st)
            else:
                hub = self.hub_d if entry == "hub" else None
                scratch = _nan(max(self.nc_d * self.A, 1)) if hub is not None else None
                rc = lib.tfgx_gat_backward_dst_hub_f32(ctypes.byref(a), None if hub is None else ctypes.byref(hub),
                                                       L.ptr(scratch), st)
            L.check(rc, "dst pass ({}, {})".format(layout, entry))
            grads = (gq,)
        else:
            gk, gv = _nan(self.n_src, self.A), _nan(self.n_src, self.W)
            a.grad_k, a.ld_grad_k, a.grad_v, a.ld_grad_v = gk.data_ptr(), self.A, gv.data_ptr(), self.W
            route = fast_route(a.H, a.d, a.dv, a.ldv, a.ld_grad_out, a.v, a.grad_out, self.W, gv.data_ptr())
            if entry == "plain":
                rc = lib.tfgx_gat_backward_src_f32(ctypes.byref(a), st)
            else:
                hub = self.hub_s if entry == "hub" else None
                scratch = _nan(max(self.nc_s * (self.A + self.W), 1)) if hub is not None else None
                rc = lib.tfgx_gat_backward_src_hub_f32(ctypes.byref(a), None if hub is None else ctypes.byref(hub),
                                                       L.ptr(scratch), st)
            L.check(rc, "src pass ({}, {})".format(layout, entry))
            grads = (gk, gv)
        torch.cuda.synchronize()
        return route, tuple(g.cpu().numpy() for g in grads)

    def reference(self):
        """float64 (dQ, dK, dV) of sum(out * dO) by torch autograd"""
        if self._ref is None:
            from f64_layers import gat_attention_f64
            r = [torch.tensor(t.cpu().numpy(), dtype=torch.float64, requires_grad=True) for t in (self.Q, self.K, self.V)]
            out = gat_attention_f64(r[0], r[1], r[2], self.plan.row_ptr.cpu().numpy(), self.plan.col.cpu().numpy(),
                                    self.geom[0], keep=self.keep, rate=self.rate)
            assert_parity(self.out.cpu().numpy(), out.detach().numpy(), tol=2e-5, what="forward")
            out.backward(torch.tensor(self.dO.cpu().numpy(), dtype=torch.float64))
            self._ref = tuple(t.grad.numpy() for t in r)
        return self._ref

    def autograd_grads(self, monkeypatch):
        """(out, dQ, dK, dV) of the package's own route, AG.gat_attention(...).backward, on the same inputs (dQ from the
        destination pass: the d == 1 forward sums are switched off, so that the forward is the one the case ran)"""
        import tf_geometric_amd.autograd as AG
        from tf_geometric_amd.nn.conv import gat as G_
        monkeypatch.setattr(G_, "QUERY_GRAD_SUMS", False)
        t = [x.detach().requires_grad_(True) for x in (self.Q, self.K, self.V)]
        out = AG.gat_attention(self.plan, t[0], t[1], t[2], self.geom[0], drop_rate=self.rate, drop_seed=self.seed)
        out.backward(self.dO)
        torch.cuda.synchronize()
        return (out.detach().cpu().numpy(),) + tuple(x.grad.cpu().numpy() for x in t)


def _same(a, b, what):
    assert a.shape == b.shape, what
    diff = int((a.view(np.uint32) != b.view(np.uint32)).sum())
    assert diff == 0, "{}: {} of {} elements differ in their bits (max |d| = {:.3e})".format(
        what, diff, a.size, float(np.nanmax(np.abs(a.astype(np.float64) - b))))


def _check_routes(c, entries, monkeypatch, expect_route):
    dQr, dKr, dVr = c.reference()
    dst = {(lay, ent): c.run("dst", lay, ent) for lay in ("dense", "interleaved") for ent in entries}
    src = {(lay, ent): c.run("src", lay, ent) for lay in ("dense", "interleaved", "head_pack") for ent in entries}
    for key, (route, (gq,)) in dst.items():
        assert ("fast" if route else "onelane") == expect_route, ("dst",) + key
        assert_parity(gq, dQr, tol=5e-5, what="dQ {}".format(key))
    for key, (route, (gk, gv)) in src.items():
        assert ("fast" if route else "onelane") == expect_route, ("src",) + key
        assert_parity(gk, dKr, tol=5e-5, what="dK {}".format(key))
        assert_parity(gv, dVr, tol=5e-5, what="dV {}".format(key))
    # same inputs (one dsum for every route), same bits: layouts and entry points are only different ways to read them
    k0 = ("dense", entries[0])
    for key, (_, (gq,)) in dst.items():
        _same(gq, dst[k0][1][0], "dQ {} vs {}".format(key, k0))
    for key, (_, (gk, gv)) in src.items():
        _same(gk, src[k0][1][0], "dK {} vs {}".format(key, k0))
        _same(gv, src[k0][1][1], "dV {} vs {}".format(key, k0))
    # the package's route (head blocks, hub lists of the plans when they have any) on the same forward
    out, gq, gk, gv = c.autograd_grads(monkeypatch)
    _same(out, c.out.cpu().numpy(), "autograd forward")
    ent = entries[-1]
    _same(gq, dst[("dense", ent)][1][0], "autograd dQ vs dst pass ({})".format(ent))
    _same(gk, src[("head_pack", ent)][1][0], "autograd dK vs head-pack src pass ({})".format(ent))
    _same(gv, src[("head_pack", ent)][1][1], "autograd dV vs head-pack src pass ({})".format(ent))


LAYOUT_CASES = [(g, v) for g in FAST + ONE_LANE for v in ("plain", "dropout", "rect", "strided")] + [((4, 8, 16), "strided_odd")]


@pytest.mark.parametrize("geom,variant", LAYOUT_CASES,
                         ids=["{}-{}".format("onelane-H{}d{}dv{}".format(*g) if v == "strided_odd" else _gid(g), v)
                              for g, v in LAYOUT_CASES])
def test_gat_backward_layouts_vs_float64(tfg, monkeypatch, geom, variant):
    """Dense / interleaved / head-pack inputs through tfgx_gat_backward_{dst,src}_f32 and *_hub_f32(NULL): float64 parity
    of dQ, dK, dV on every route, bit identity between routes, and bit identity with autograd.py's route.  Variants:
    attention dropout 0.4 (edge_pos_t), n_src > n_dst (source-only rows take no self-loop), column slices of wider tables
    (ld % 4 == 0 keeps the tuned kernels, ld % 4 != 0 drops to the one-lane kernels)."""
    c = _Case(geom, variant)
    assert c.plan.hub_info() is None and c.pt.hub_info() is None
    expect = "onelane" if variant == "strided_odd" else _geom_route(*geom)
    _check_routes(c, ("plain", "hub_null"), monkeypatch, expect)


HUB_CASES = [(g, v) for g in [(8, 1, 8), (4, 8, 16), (2, 32, 64), (1, 4, 44)] for v in ("plain", "dropout")]


@pytest.mark.parametrize("geom,variant", HUB_CASES, ids=["{}-{}".format(_gid(g), v) for g, v in HUB_CASES])
def test_gat_backward_hub_lists_vs_float64(tfg, monkeypatch, geom, variant):
    """Real hub lists (a 3000-in-edge destination, a 2500-out-edge source, threshold 64 / chunk 48): every layout through
    *_hub_f32 with the plans' lists — chunk partials added in order — against float64, the layouts bit-identical, the
    head-pack route bit-identical with autograd.py's (which takes the same lists)."""
    c = _Case(geom, variant, hubs=True)
    _check_routes(c, ("hub",), monkeypatch, "fast")


def _pack_vec4(H, d, dv, ld_pack):
    """Python mirror of the 16-byte condition of tfgx_gat_pack_dst_f32 (dense, 16-byte aligned dO / O / pack)"""
    lh = dv // 4
    per_row4 = H * dv // 4 + (H * d + 2 * H + 3) // 4
    return (dv % 4 == 0 and lh >= 1 and (lh & (lh - 1)) == 0 and lh <= 64 and per_row4 % lh == 0 and (H * dv) % 4 == 0
            and ld_pack % 4 == 0)


PACK_CASES = [(g, 0) for g in FAST + ONE_LANE] + [((2, 6, 16), 0), ((8, 1, 8), 1), ((2, 6, 16), 3)]


@pytest.mark.parametrize("geom,extra", PACK_CASES,
                         ids=["{}-H{}d{}dv{}{}".format("vec4" if _pack_vec4(*g, _roundup(g[0] * (g[1] + g[2] + 3), 32) + e)
                                                       else "scalar", *g, "-ld+{}".format(e) if e else "")
                              for g, e in PACK_CASES])
def test_gat_pack_dst_tables(tfg, geom, extra):
    """tfgx_gat_pack_dst_f32 on its 16-byte and its scalar kernel and tfgx_gat_pack_dst_heads_f32, into tables prefilled
    with NaN: the copies of dO, Q, m, l bit-exact, D against float64 <dO, O> per head (scalar kernel: the head-block
    form's bits, same sequential fma order), nothing written past the row, the head blocks' 1 / (l + 1e-8) and zero pad."""
    from tf_geometric_amd import _lib as L
    lib = L.require_gpu()
    H, d, dv = geom
    A, W = H * d, H * dv
    n = 300
    rng = np.random.Generator(np.random.PCG64(7 * H + d + dv))
    dO = rng.standard_normal((n, W)).astype(np.float32)
    O = rng.standard_normal((n, W)).astype(np.float32)
    Q = rng.standard_normal((n, A)).astype(np.float32)
    ml = np.stack([rng.standard_normal((n, H)), rng.uniform(1.0, 30.0, (n, H))], -1).reshape(n, 2 * H).astype(np.float32)
    t = {k: torch.from_numpy(v).cuda() for k, v in dict(dO=dO, O=O, Q=Q, ml=ml).items()}
    st = L.stream_ptr()
    P = _roundup(W + A + 3 * H, 32) + extra
    vec4 = _pack_vec4(H, d, dv, P)
    pack, dsum = _nan(n, P), _nan(n, H)
    L.check(lib.tfgx_gat_pack_dst_f32(L.ptr(t["dO"]), W, L.ptr(t["O"]), W, L.ptr(t["Q"]), A, L.ptr(t["ml"]), n, H, d, dv,
                                      L.ptr(pack), P, L.ptr(dsum), st), "tfgx_gat_pack_dst_f32")
    HB, W4 = _roundup(d + 3, 4), _roundup(W, 4)
    Ph = _roundup(W4 + H * HB, 32)
    hpack, hdsum = _nan(n, Ph), _nan(n, H)
    L.check(lib.tfgx_gat_pack_dst_heads_f32(L.ptr(t["dO"]), W, L.ptr(t["O"]), W, L.ptr(t["Q"]), A, L.ptr(t["ml"]), n, H, d,
                                            dv, L.ptr(hpack), Ph, L.ptr(hdsum), st), "tfgx_gat_pack_dst_heads_f32")
    pack, dsum, hpack, hdsum = (x.cpu().numpy() for x in (pack, dsum, hpack, hdsum))
    D64 = (dO.astype(np.float64) * O).reshape(n, H, dv).sum(-1)
    # interleaved table
    _same(pack[:, :W], dO, "pack dO")
    _same(pack[:, W:W + A], Q, "pack Q")
    _same(pack[:, W + A:W + A + 2 * H], ml, "pack (m, l)")
    _same(pack[:, W + A + 2 * H:W + A + 3 * H], dsum, "pack D == dsum")
    assert_parity(dsum, D64, tol=1e-5, what="pack D")
    assert np.isnan(pack[:, W + A + 3 * H:]).all(), "tfgx_gat_pack_dst_f32 wrote past W + A + 3H"
    if not vec4:
        _same(dsum, hdsum, "scalar pack D vs head-block D")
    # head-block table
    _same(hpack[:, :W], dO, "head-pack dO")
    hb = hpack[:, W4:W4 + H * HB].reshape(n, H, HB)
    _same(hb[:, :, :d], Q.reshape(n, H, d), "head-pack Q")
    _same(hb[:, :, d], ml[:, 0::2], "head-pack m")
    linv = np.float32(1.0) / (ml[:, 1::2] + np.float32(1e-8))
    _same(hb[:, :, d + 1], linv, "head-pack 1 / (l + 1e-8)")
    _same(hb[:, :, d + 2], hdsum, "head-pack D == dsum")
    assert (hb[:, :, d + 3:].view(np.uint32) == 0).all(), "head-block pad is not +0.0"
    assert np.isnan(hpack[:, W4 + H * HB:]).all(), "tfgx_gat_pack_dst_heads_f32 wrote past its head blocks"
    assert_parity(hdsum, D64, tol=1e-5, what="head-pack D")


def test_pack_routes_are_covered():
    """PACK_CASES reach both kernels of tfgx_gat_pack_dst_f32; the layout cases reach both backward kernel families."""
    routes = {_pack_vec4(*g, _roundup(g[0] * (g[1] + g[2] + 3), 32) + e) for g, e in PACK_CASES}
    assert routes == {True, False}
    assert {_geom_route(*g) for g in FAST} == {"fast"} and {_geom_route(*g) for g in ONE_LANE} == {"onelane"}


def test_gat_backward_argument_errors_on_real_buffers(tfg):
    """Invalid strides / head_pack / dropout without edge_pos_t: TFGX_ERR_INVALID_ARG with its message, nothing written.
    Every buffer is large enough that a call which wrongly passed the checks would still stay inside it."""
    c = _Case((4, 8, 16), "plain")
    L, lib = c.L, c.lib
    H = 4
    gq, gk, gv = _nan(c.n_dst, c.A), _nan(c.n_src, c.A), _nan(c.n_src, c.W)
    st = L.stream_ptr()

    def call(pass_, a, msg):
        a.grad_q, a.ld_grad_q = gq.data_ptr(), c.A
        a.grad_k, a.ld_grad_k, a.grad_v, a.ld_grad_v = gk.data_ptr(), c.A, gv.data_ptr(), c.W
        fn = lib.tfgx_gat_backward_dst_f32 if pass_ == "dst" else lib.tfgx_gat_backward_src_f32
        assert fn(ctypes.byref(a), st) == 1, (pass_, msg)
        assert msg in lib.tfgx_last_error(), lib.tfgx_last_error()

    for pass_ in ("dst", "src"):
        a = c.args("interleaved")
        a.ld_stats_ml = 2 * H - 1
        call(pass_, a, b"ld_stats_ml / ld_dsum too small")
        a = c.args("interleaved")
        a.ld_dsum = H - 1
        call(pass_, a, b"ld_stats_ml / ld_dsum too small")
    a = c.args("head_pack")
    a.head_pack += 4                                       # 4-byte aligned only (the spare row keeps reads inside)
    call("src", a, b"head_pack")
    a = c.args("head_pack")
    a.ld_head_pack = H * c.HB - 4
    call("src", a, b"head_pack")
    a = c.args("dense")
    from tf_geometric_amd.nn.conv.gat import _set_drop
    _set_drop(a, 0.4, c.seed, c.E)
    call("src", a, b"edge_pos_t")
    torch.cuda.synchronize()
    assert all(torch.isnan(x).all() for x in (gq, gk, gv)), "a rejected call wrote gradients"


@pytest.mark.parametrize("H", [1, 3, 8])
@pytest.mark.parametrize("hubs", [False, True], ids=["plain", "hub"])
def test_edge_softmax_null_perm(tfg, H, hubs):
    """tfgx_edge_softmax_f32 / _hub_f32 with perm = NULL (scores already in CSR order) give, bit for bit, the CSR-ordered
    result of the run over the original order with plan.perm; both against a float64 segment softmax."""
    from tf_geometric_amd import _lib as L
    import tf_geometric_amd.plan as P
    lib = L.require_gpu()
    rng = np.random.Generator(np.random.PCG64(31 + H))
    n = 400
    dst = [rng.integers(0, n, 5000), np.full(150, 11)]
    if hubs:
        dst.append(np.full(2000, 3))
    dst = np.concatenate(dst)
    ei = np.stack([dst, rng.integers(0, n, dst.shape[0])]).astype(np.int32)
    old_policy = (P.HUB_THRESHOLD, P.HUB_CHUNK)
    if hubs:
        P.HUB_THRESHOLD, P.HUB_CHUNK = 64, 48
    try:
        plan = P.CsrPlan.build(L.as_i32(ei), n, n)
        hub, nc = L.hub_lists(plan) if hubs else (None, 0)
    finally:
        P.HUB_THRESHOLD, P.HUB_CHUNK = old_policy
    assert (hub is not None) == hubs
    E = plan.num_edges
    score = torch.from_numpy((3.0 * rng.standard_normal((E, H))).astype(np.float32)).cuda()   # original edge order
    perm = plan.perm.long()
    score_csr = score[perm].contiguous()
    out_perm, out_null = _nan(E, H), _nan(E, H)
    st = L.stream_ptr()
    if hubs:
        hp = 1
        while hp < H:
            hp <<= 1
        for s, pm, o in ((score, plan.perm, out_perm), (score_csr, None, out_null)):
            scratch = _nan(max(nc * 2 * hp, 1))
            L.check(lib.tfgx_edge_softmax_hub_f32(L.ptr(plan.row_ptr), L.ptr(pm), L.ptr(s), H, n, L.ptr(o), ctypes.byref(hub),
                                                  L.ptr(scratch), st), "tfgx_edge_softmax_hub_f32")
    else:
        for s, pm, o in ((score, plan.perm, out_perm), (score_csr, None, out_null)):
            L.check(lib.tfgx_edge_softmax_f32(L.ptr(plan.row_ptr), L.ptr(pm), L.ptr(s), H, n, L.ptr(o), st),
                    "tfgx_edge_softmax_f32")
    torch.cuda.synchronize()
    _same(out_null.cpu().numpy(), out_perm[perm].cpu().numpy(), "NULL perm vs plan.perm")
    # float64: exp(s - segmax) / (segsum + 1e-8) per destination (nn/kernel/segment.py:26-33), CSR order
    rp = plan.row_ptr.cpu().numpy()
    row = torch.repeat_interleave(torch.arange(n), torch.from_numpy(np.diff(rp)).long())
    s64 = score_csr.cpu().double()
    m = torch.full((n, H), -1e300, dtype=torch.float64).scatter_reduce(0, row[:, None].expand(-1, H), s64, "amax")
    p = torch.exp(s64 - m[row])
    den = torch.zeros((n, H), dtype=torch.float64).index_add(0, row, p) + 1e-8
    assert_parity(out_null.cpu().numpy(), (p / den[row]).numpy(), tol=1e-5, what="edge softmax")
