# coding=utf-8
"""tfgx_segment_gram_f32 / tfgx_segment_gram_backward_f32 (include/tfgx_seggram.h) on the GPU, through the raw entry points.

Reference: float64 sums of outer products (index_add), forward; the same restatement differentiated by hand in float64,
backward.  Bar per element, as tests/test_gpu_fuzz_backward.py: max(1e-5 (1 + |ref|), 8 * 2^-24 * sqrt(n) * sum|terms|) with n the
number of terms of the element's own chain (the segment's length forward; W for dS, K for dY) and sum|terms| from the same
product on |S|, |Y|, |dOut| in float64.  Everything the header promises beyond values is asserted bit for bit."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

KS = [1, 5, 20, 64]
WS = [1, 20, 65, 300]
EPS = 8.0 * 2.0 ** -24


def _lib():
    from tf_geometric_amd import _lib as L
    return L, L.require_gpu()


def _lengths(B):
    """An empty first and last segment, 0 / 1 / B - 1 / B / B + 1 / 3B + 7 nodes, and a run of 2B one-node segments."""
    return [0, 1, B - 1, 0, B, B + 1, 3 * B + 7] + [1] * (2 * B) + [5, 0]


def _ptr(lengths):
    return np.concatenate([[0], np.cumsum(lengths)]).astype(np.int32)


def _padded(a, extra, dev):
    """A [rows, cols + extra] device buffer holding `a` with NaN in the extra columns; -> (buffer, leading dimension)."""
    rows, cols = a.shape
    buf = torch.full((rows, cols + extra), float("nan"), dtype=torch.float32, device=dev)
    buf[:, :cols] = a
    return buf, cols + extra


def _forward(seg_ptr, seg_node, N, S, Y, pad=(3, 2, 5), flag=None):
    """One raw forward call on padded buffers; -> out [G K, W] (the columns past W are asserted to have kept their NaN)."""
    L, lib = _lib()
    dev = S.device
    G, K, W = int(seg_ptr.shape[0]) - 1, int(S.shape[1]), int(Y.shape[1])
    Sb, lds = _padded(S, pad[0], dev)
    Yb, ldy = _padded(Y, pad[1], dev)
    out = torch.full((G * K, W + pad[2]), float("nan"), dtype=torch.float32, device=dev)
    nbytes = lib.tfgx_segment_gram_workspace_bytes(N, G, K, W)
    ws = torch.full((max(nbytes // 4, 1),), float("nan"), dtype=torch.float32, device=dev)
    L.check(lib.tfgx_segment_gram_f32(L.ptr(seg_ptr), L.ptr(seg_node), G, N, L.ptr(Sb), lds, K, L.ptr(Yb), ldy, W, L.ptr(out),
                                      W + pad[2], L.ptr(flag), L.ptr(ws), nbytes, L.stream_ptr()), "tfgx_segment_gram_f32")
    assert torch.isnan(out[:, W:]).all(), "columns past W were written"
    return out[:, :W].contiguous()


def _reference(ptr, node, S, Y):
    """float64 on the host: (out [G K, W], sum|terms| [G K, W], terms per row [G K])."""
    G, K, W = len(ptr) - 1, S.shape[1], Y.shape[1]
    seg = np.repeat(np.arange(G), np.diff(ptr))
    node = np.arange(len(seg)) if node is None else np.asarray(node)
    ok = (node >= 0) & (node < S.shape[0])
    seg_t, node_t = torch.from_numpy(seg[ok]), torch.from_numpy(node[ok].astype(np.int64))
    S64, Y64 = torch.from_numpy(S).double(), torch.from_numpy(Y).double()

    def product(a, b):
        outer = a[node_t].unsqueeze(2) * b[node_t].unsqueeze(1)
        return torch.zeros((G, K, W), dtype=torch.float64).index_add(0, seg_t, outer).reshape(G * K, W).numpy()
    return product(S64, Y64), product(S64.abs(), Y64.abs()), np.repeat(np.diff(ptr), K)


def _check(got, ref, absref, terms, what):
    got = got.double().cpu().numpy()
    assert np.isfinite(got).all(), what + ": a row was not written"
    bound = np.maximum(1e-5 * (1.0 + np.abs(ref)), EPS * np.sqrt(np.maximum(terms, 1))[:, None] * absref)
    err = np.abs(got - ref)
    print("{}: max |ref| {:.3e}, max err {:.3e}, max err / bound {:.3f}".format(
        what, float(np.abs(ref).max()), float(err.max()), float((err / bound).max())))
    assert (err <= bound).all(), "{}: max err / bound = {:.3f}".format(what, float((err / bound).max()))


def _data(N, K, W, seed):
    rng = np.random.Generator(np.random.PCG64(seed))
    return rng.standard_normal((N, K)).astype(np.float32), rng.standard_normal((N, W)).astype(np.float32)


@pytest.mark.parametrize("W", WS)
@pytest.mark.parametrize("K", KS)
def test_forward_against_float64(tfg, K, W):
    L, lib = _lib()
    dev = L.device()
    B = lib.tfgx_seggram_block()
    lengths = _lengths(B)
    ptr = _ptr(lengths)
    N = int(ptr[-1])
    S, Y = _data(N, K, W, 100 * K + W)
    St, Yt, ptr_t = torch.from_numpy(S).to(dev), torch.from_numpy(Y).to(dev), torch.from_numpy(ptr).to(dev)
    flag = torch.zeros(1, dtype=torch.int32, device=dev)
    # seg_node = NULL
    out = _forward(ptr_t, None, N, St, Yt, flag=flag)
    _check(out, *_reference(ptr, None, S, Y), what="identity K={} W={}".format(K, W))
    assert torch.equal(out, _forward(ptr_t, None, N, St, Yt)), "not bit-identical from run to run"
    empty = np.flatnonzero(np.repeat(np.diff(ptr), K) == 0)
    assert empty.size >= 3 * K and (out[torch.from_numpy(empty).to(dev)] == 0).all()            # zero rows, not NaN
    # a random permutation, as the graph plan of an unsorted node_graph_index gives it
    node = np.random.Generator(np.random.PCG64(7)).permutation(N).astype(np.int32)
    out_p = _forward(ptr_t, torch.from_numpy(node).to(dev), N, St, Yt, flag=flag)
    _check(out_p, *_reference(ptr, node, S, Y), what="permuted K={} W={}".format(K, W))
    assert int(flag.item()) == 0
    # the same rows through an explicit identity list: the bits of seg_node = NULL
    ident = torch.arange(N, dtype=torch.int32, device=dev)
    assert torch.equal(out, _forward(ptr_t, ident, N, St, Yt, pad=(0, 0, 0)))


@pytest.mark.parametrize("K, W", [(5, 20), (64, 65)])
def test_a_segment_keeps_its_bits_when_others_change_length(tfg, K, W):
    """Segments behind a segment that grows by exactly one block keep their position modulo B, hence every bit."""
    L, lib = _lib()
    dev = L.device()
    B = lib.tfgx_seggram_block()
    lengths = _lengths(B)
    ptr = _ptr(lengths)
    N = int(ptr[-1])
    S, Y = _data(N, K, W, 5)
    grown = 2                                   # the segment of B - 1 nodes takes B more
    lengths2 = list(lengths)
    lengths2[grown] += B
    ptr2 = _ptr(lengths2)
    cut = int(ptr[grown + 1])
    S_new, Y_new = _data(B, K, W, 6)
    S2 = np.concatenate([S[:cut], S_new, S[cut:]])
    Y2 = np.concatenate([Y[:cut], Y_new, Y[cut:]])
    t = lambda a: torch.from_numpy(a).to(dev)       # noqa: E731
    out = _forward(t(ptr), None, N, t(S), t(Y))
    out2 = _forward(t(ptr2), None, N + B, t(S2), t(Y2))
    rows = np.arange(len(lengths) * K).reshape(len(lengths), K)
    same = np.concatenate([rows[g] for g in range(len(lengths)) if g != grown])
    assert torch.equal(out[t(same)], out2[t(same)])
    assert not torch.equal(out[t(rows[grown])], out2[t(rows[grown])])
    _check(out2, *_reference(ptr2, None, S2, Y2), what="grown")


def _reference_by_segment(ptr, S, Y):
    """_reference for long segments: one float64 product per segment instead of N outer products."""
    S64, Y64 = S.astype(np.float64), Y.astype(np.float64)
    out = [S64[a:b].T @ Y64[a:b] for a, b in zip(ptr[:-1], ptr[1:])]
    absout = [np.abs(S64[a:b]).T @ np.abs(Y64[a:b]) for a, b in zip(ptr[:-1], ptr[1:])]
    return np.concatenate(out), np.concatenate(absout), np.repeat(np.diff(ptr), S.shape[1])


@pytest.mark.parametrize("K, W", [(5, 20), (64, 65)])
def test_long_segments_fold_in_groups(tfg, K, W):
    """Segments that leave partials in 64, 65 and 201 blocks: the fold takes the partials behind the first 64 at a time (none,
    exactly one group and nothing left over, three groups and eight left over).  The groups are counted from the segment's
    own first block, so a shift of the whole batch by one block changes no bit."""
    L, lib = _lib()
    dev = L.device()
    B = lib.tfgx_seggram_block()
    lengths = [3, 63 * B + 10, 64 * B, 200 * B + 17, 5, 0]
    ptr = _ptr(lengths)
    N = int(ptr[-1])
    S, Y = _data(N, K, W, 31)
    t = lambda a: torch.from_numpy(a).to(dev)       # noqa: E731
    out = _forward(t(ptr), None, N, t(S), t(Y))
    _check(out, *_reference_by_segment(ptr, S, Y), what="long segments K={} W={}".format(K, W))
    assert torch.equal(out, _forward(t(ptr), None, N, t(S), t(Y))), "not bit-identical from run to run"
    S_new, Y_new = _data(B, K, W, 32)
    ptr2 = _ptr([3 + B] + lengths[1:])
    S2, Y2 = np.concatenate([S[:3], S_new, S[3:]]), np.concatenate([Y[:3], Y_new, Y[3:]])
    out2 = _forward(t(ptr2), None, N + B, t(S2), t(Y2))
    assert torch.equal(out[K:], out2[K:])
    _check(out2, *_reference_by_segment(ptr2, S2, Y2), what="long segments, shifted")


def test_bad_spans_and_bad_nodes_set_the_flag_and_touch_nothing_else(tfg):
    L, lib = _lib()
    dev = L.device()
    B = lib.tfgx_seggram_block()
    K, W = 5, 20
    lengths = _lengths(B)
    ptr = _ptr(lengths)
    G, N = len(lengths), int(ptr[-1])
    S, Y = _data(N, K, W, 9)
    t = lambda a: torch.from_numpy(a).to(dev)       # noqa: E731
    ref, absref, terms = _reference(ptr, None, S, Y)
    # (a) a span that runs backwards, in the middle of the one-node segments
    j = 7 + B
    bad_ptr = ptr.copy()
    bad_ptr[j] = ptr[j - 1] - 3                      # segment j - 1 runs backwards; segment j now overlaps its predecessors
    flag = torch.zeros(1, dtype=torch.int32, device=dev)
    out = _forward(t(bad_ptr), None, N, t(S), t(Y), flag=flag)
    assert int(flag.item()) == 1
    assert (out[(j - 1) * K:j * K] == 0).all(), "a backwards span is an empty segment"
    far = np.setdiff1d(np.arange(G), [j - 1, j])          # every segment but the damaged span and the one that grew over it
    rows = (far[:, None] * K + np.arange(K)).reshape(-1)
    _check(out[t(rows)], ref[rows], absref[rows], terms[rows], what="beside a backwards span")
    assert torch.equal(out[t(rows)], _forward(t(ptr), None, N, t(S), t(Y))[t(rows)])
    # (b) a span outside [0, N]
    bad_ptr = ptr.copy()
    bad_ptr[-1] = N + 9
    flag.zero_()
    out = _forward(t(bad_ptr), None, N, t(S), t(Y), flag=flag)
    assert int(flag.item()) == 1 and (out[-K:] == 0).all()
    _check(out[:-K], ref[:-K], absref[:-K], terms[:-K], what="beside a span past N")
    # (c) node ids outside [0, N): skipped
    node = np.random.Generator(np.random.PCG64(3)).permutation(N).astype(np.int32)
    node[[5, B + 1, N - 2]] = [N, -1, 2 ** 31 - 1]
    flag.zero_()
    out = _forward(t(ptr), t(node), N, t(S), t(Y), flag=flag)
    assert int(flag.item()) == 1
    _check(out, *_reference(ptr, node, S, Y), what="bad nodes skipped")


def _backward(node_seg, G, S, Y, dOut, want_s, want_y, flag=None, pad=(3, 2, 5, 1, 4)):
    L, lib = _lib()
    dev = S.device
    N, K, W = int(S.shape[0]), int(S.shape[1]), int(Y.shape[1])
    Sb, lds = _padded(S, pad[0], dev)
    Yb, ldy = _padded(Y, pad[1], dev)
    Ob, ldo = _padded(dOut, pad[2], dev)
    dS = torch.full((N, K + pad[3]), float("nan"), dtype=torch.float32, device=dev) if want_s else None
    dY = torch.full((N, W + pad[4]), float("nan"), dtype=torch.float32, device=dev) if want_y else None
    L.check(lib.tfgx_segment_gram_backward_f32(L.ptr(node_seg), N, G, L.ptr(Sb), lds, K, L.ptr(Yb), ldy, W, L.ptr(Ob), ldo,
                                               L.ptr(dS), K + pad[3], L.ptr(dY), W + pad[4], L.ptr(flag), L.stream_ptr()),
            "tfgx_segment_gram_backward_f32")
    if want_s:
        assert torch.isnan(dS[:, K:]).all()
        dS = dS[:, :K].contiguous()
    if want_y:
        assert torch.isnan(dY[:, W:]).all()
        dY = dY[:, :W].contiguous()
    return dS, dY


def _backward_reference(seg, G, S, Y, dOut):
    """d/dS and d/dY of sum(out * dOut) for the forward's restatement, float64, with sum|terms|."""
    K, W = S.shape[1], Y.shape[1]
    ok = (seg >= 0) & (seg < G)
    blocks = torch.from_numpy(dOut).double().reshape(G, K, W)
    per_node = torch.zeros((len(seg), K, W), dtype=torch.float64)
    per_node[torch.from_numpy(ok)] = blocks[torch.from_numpy(seg[ok].astype(np.int64))]
    S64, Y64 = torch.from_numpy(S).double(), torch.from_numpy(Y).double()
    dS = torch.einsum("nkw,nw->nk", per_node, Y64)
    dY = torch.einsum("nkw,nk->nw", per_node, S64)
    dS_abs = torch.einsum("nkw,nw->nk", per_node.abs(), Y64.abs())
    dY_abs = torch.einsum("nkw,nk->nw", per_node.abs(), S64.abs())
    return dS.numpy(), dS_abs.numpy(), dY.numpy(), dY_abs.numpy()


@pytest.mark.parametrize("order", ["sorted", "shuffled"])
@pytest.mark.parametrize("K, W", [(1, 1), (5, 20), (20, 65), (64, 300), (64, 1), (1, 300)])
def test_backward_against_float64(tfg, K, W, order):
    """Segments cross the kernel's node runs (sorted ids: long segments span several runs, the one-node segments give a run
    one segment per node; shuffled ids: a new segment at almost every node)."""
    L, lib = _lib()
    dev = L.device()
    lengths = _lengths(lib.tfgx_seggram_block())
    G = len(lengths)
    seg = np.repeat(np.arange(G), lengths).astype(np.int32)
    if order == "shuffled":
        seg = np.random.Generator(np.random.PCG64(11)).permutation(seg)
    N = len(seg)
    S, Y = _data(N, K, W, 1000 + 10 * K + W)
    dOut = np.random.Generator(np.random.PCG64(K * W)).standard_normal((G * K, W)).astype(np.float32)
    t = lambda a: torch.from_numpy(a).to(dev)       # noqa: E731
    flag = torch.zeros(1, dtype=torch.int32, device=dev)
    dS_ref, dS_abs, dY_ref, dY_abs = _backward_reference(seg, G, S, Y, dOut)
    dS, dY = _backward(t(seg), G, t(S), t(Y), t(dOut), True, True, flag=flag)
    _check(dS, dS_ref, dS_abs, np.full(N, W), what="dS K={} W={} {}".format(K, W, order))
    _check(dY, dY_ref, dY_abs, np.full(N, K), what="dY K={} W={} {}".format(K, W, order))
    dS_only, none = _backward(t(seg), G, t(S), t(Y), t(dOut), True, False, flag=flag)
    assert none is None and torch.equal(dS_only, dS)
    none, dY_only = _backward(t(seg), G, t(S), t(Y), t(dOut), False, True, flag=flag)
    assert none is None and torch.equal(dY_only, dY)
    assert int(flag.item()) == 0


def test_backward_out_of_range_segment_ids_give_zero_rows(tfg):
    L, lib = _lib()
    dev = L.device()
    lengths = _lengths(lib.tfgx_seggram_block())
    G, K, W = len(lengths), 5, 70
    seg = np.repeat(np.arange(G), lengths).astype(np.int32)
    N = len(seg)
    bad = np.array([0, 31, 32, 100, N - 1])
    seg[bad] = [-1, G, G + 7, -5, 2 ** 31 - 1]
    S, Y = _data(N, K, W, 77)
    dOut = np.random.Generator(np.random.PCG64(78)).standard_normal((G * K, W)).astype(np.float32)
    t = lambda a: torch.from_numpy(a).to(dev)       # noqa: E731
    flag = torch.zeros(1, dtype=torch.int32, device=dev)
    dS, dY = _backward(t(seg), G, t(S), t(Y), t(dOut), True, True, flag=flag)
    assert int(flag.item()) == 1
    assert (dS[t(bad)] == 0).all() and (dY[t(bad)] == 0).all()
    dS_ref, dS_abs, dY_ref, dY_abs = _backward_reference(seg, G, S, Y, dOut)
    _check(dS, dS_ref, dS_abs, np.full(N, W), what="dS beside bad ids")
    _check(dY, dY_ref, dY_abs, np.full(N, K), what="dY beside bad ids")


def test_zero_width_and_no_segments(tfg):
    """W == 0: dS is written as zeros.  G == 0 backward: every id is out of range.  N == 0 forward: zero rows."""
    L, lib = _lib()
    dev = L.device()
    N, K = 70, 5
    S = torch.randn(N, K, device=dev)
    seg = torch.zeros(N, dtype=torch.int32, device=dev)
    dS, _ = _backward(seg, 1, S, torch.zeros(N, 0, device=dev), torch.zeros(K, 0, device=dev), True, False)
    assert (dS == 0).all()
    flag = torch.zeros(1, dtype=torch.int32, device=dev)
    dS, dY = _backward(seg, 0, S, torch.randn(N, 3, device=dev), torch.zeros(0, 3, device=dev), True, True, flag=flag)
    assert (dS == 0).all() and (dY == 0).all() and int(flag.item()) == 1
    ptr = torch.zeros(4, dtype=torch.int32, device=dev)
    out = _forward(ptr, None, 0, torch.zeros(0, K, device=dev), torch.zeros(0, 3, device=dev))
    assert out.shape == (3 * K, 3) and (out == 0).all()


def test_autograd_function_against_float64_autograd(tfg):
    """autograd.segment_gram on a graph plan of unsorted ids: values and both gradients, S and Y the same tensor included
    (the two gradients of one tensor add up), and the backward skips what is not asked for.  Same bar; sum|terms| of a
    gradient is the float64 gradient of the product on absolute values under |coefficients|."""
    from tf_geometric_amd import autograd as AG
    from tf_geometric_amd.nn.pool.common_pool import _graph_plan
    L, lib = _lib()
    dev = L.device()
    rng = np.random.Generator(np.random.PCG64(21))
    G, K, W = 9, 5, 7
    counts = rng.integers(0, 90, G)
    ids_np = rng.permutation(np.repeat(np.arange(G), counts)).astype(np.int32)
    N = len(ids_np)
    ids = torch.from_numpy(ids_np).to(dev)
    plan = _graph_plan(ids, G, N, None)
    S_np, Y_np = _data(N, K, W, 22)
    ids64 = torch.from_numpy(ids_np.astype(np.int64))

    def f64(S, Y):
        outer = S.unsqueeze(2) * Y.unsqueeze(1)
        return torch.zeros((G, S.shape[1], Y.shape[1]), dtype=torch.float64).index_add(0, ids64, outer).reshape(
            G * S.shape[1], Y.shape[1])

    def grads64(coef, same, absolute):
        conv = (lambda a: torch.from_numpy(a).double().abs()) if absolute else (lambda a: torch.from_numpy(a).double())
        S64 = conv(S_np).requires_grad_(True)
        Y64 = S64 if same else conv(Y_np).requires_grad_(True)
        out = f64(S64, Y64)
        (out * (coef.abs() if absolute else coef)).sum().backward()
        return out.detach().numpy(), S64.grad.numpy(), (None if same else Y64.grad.numpy())

    for same in (False, True):
        coef = torch.from_numpy(rng.standard_normal((G * K, K if same else W)))
        S = torch.from_numpy(S_np).to(dev).requires_grad_(True)
        Y = S if same else torch.from_numpy(Y_np).to(dev).requires_grad_(True)
        out = AG.segment_gram(plan, ids, S, Y)
        (out.double() * coef.to(dev)).sum().backward()
        ref, dS_ref, dY_ref = grads64(coef, same, False)
        absref, dS_abs, dY_abs = grads64(coef, same, True)
        _check(out.detach(), ref, absref, np.repeat(counts, K), what="autograd out (S is Y: {})".format(same))
        _check(S.grad, dS_ref, dS_abs, np.full(N, 2 * K if same else W), what="autograd dS (S is Y: {})".format(same))
        if not same:
            _check(Y.grad, dY_ref, dY_abs, np.full(N, K), what="autograd dY")
    # only Y tracked: no dS is computed; nothing tracked: no graph
    Y3 = torch.from_numpy(Y_np).to(dev).requires_grad_(True)
    S3 = torch.from_numpy(S_np).to(dev)
    AG.segment_gram(plan, ids, S3, Y3).sum().backward()
    assert Y3.grad is not None and S3.grad is None and not AG.segment_gram(plan, ids, S3, Y3.detach()).requires_grad
    with pytest.raises(ValueError, match="TFGX_SEGGRAM_MAX_K"):
        AG.segment_gram(plan, ids, torch.zeros(N, 65, device=dev), Y3.detach())
