# coding=utf-8
"""The plan-level entry (plan.segment_reduce on a dense table) promotes a table it meets twice unchanged to the split +
edge-resident-tail layout and serves it through the VERIFIED route (tfgx_reduce_args.verify): every launch
compares every row of the table with the layout on the device and a repair launch recomputes the output from the table when
anything differed.  Outputs are bit-identical to the plain route, also right after a write that torch's version counter
never saw; calls queue without a host synchronisation; nothing is memoised inside a hipGraph capture."""
import pytest
import torch

pytestmark = pytest.mark.gpu


def _plain(P, *args, **kw):
    auto = P.AUTO_STATIC_LAYOUT
    P.AUTO_STATIC_LAYOUT = False
    try:
        return P.segment_reduce(*args, **kw)
    finally:
        P.AUTO_STATIC_LAYOUT = auto


def _entry(P, plan, x):
    memo = plan.__dict__.get("_verified") or {}
    return memo.get(x.data_ptr())


@pytest.fixture(scope="module")
def products(tfg):
    from tf_geometric_amd import synthetic
    from tf_geometric_amd.plan import CsrPlan
    n, e, f = synthetic.WORKLOADS["products"]
    ei = tfg._lib.as_i32(synthetic.synthetic_edges(n, e, seed=0))
    g = torch.Generator(device="cuda")
    g.manual_seed(3)
    x = torch.randn(n, f, generator=g, device="cuda")
    w = torch.rand(int(ei.shape[1]), generator=g, device="cuda") + 0.5
    sc = torch.rand(n, generator=g, device="cuda") + 0.5
    plan = CsrPlan.build(ei, n, n)
    return dict(n=n, f=f, x=x, plan=plan, w_csr=plan.edge_attr_to_csr(w), sc=sc)


def _small(tfg, n, e, f, seed, n_src=None):
    from tf_geometric_amd.plan import CsrPlan
    g = torch.Generator(device="cuda")
    g.manual_seed(seed)
    n_src = n if n_src is None else n_src
    ei = torch.stack([torch.randint(0, n, (e,), generator=g, device="cuda"),
                      torch.randint(0, n_src, (e,), generator=g, device="cuda")]).to(torch.int32)
    plan = CsrPlan.build(ei, n, n_src)
    x = torch.randn(n_src, f, generator=g, device="cuda")
    w = torch.rand(e, generator=g, device="cuda") + 0.5
    sc = torch.rand(n, generator=g, device="cuda") + 0.5
    return plan, x, plan.edge_attr_to_csr(w), sc


@pytest.fixture
def small_tables_wanted(monkeypatch):
    """Small tables take the layout too (SplitRows.wanted asks for tables beyond the caches otherwise)."""
    from tf_geometric_amd import plan as P
    monkeypatch.setattr(P.SplitRows, "wanted", staticmethod(lambda n, F: F % 4 == 0 and 32 < F <= 128 and F % 32 != 0))
    monkeypatch.setenv("TFGX_STATIC_LAYOUT_BUDGET", "1e12")
    return P


@pytest.mark.parametrize("f", [36, 100, 124])
@pytest.mark.parametrize("kind", ["gcn", "sum", "mean", "max"])
def test_small_promoted_route_is_bit_identical(tfg, small_tables_wanted, f, kind):
    P, L = small_tables_wanted, tfg._lib
    plan, x, w, sc = _small(tfg, 3000, 40000, f, seed=f)
    op = {"gcn": L.SUM, "sum": L.SUM, "mean": L.MEAN, "max": L.MAX}[kind]
    kw = dict(w_csr=w, self_coef=sc) if kind == "gcn" else dict(w_csr=w if kind != "max" else None)
    ref = _plain(P, plan, x, op, **kw)
    promos = P.VERIFIED_STATS["promotions"]
    outs = [P.segment_reduce(plan, x, op, **kw) for _ in range(4)]        # call 2 promotes, calls 3-4 are served
    assert P.VERIFIED_STATS["promotions"] == promos + 1
    assert _entry(P, plan, x).rows is not None
    for o in outs:
        assert torch.equal(o, ref)
    name = P.segment_reduce(plan, x, op, describe=True, **kw)
    assert "seg_reduce_verify_kernel" in name and ("split_rows_compare_kernel" in name) == (kind != "gcn")


def test_small_rectangular_plan_checks_every_table_row(tfg, small_tables_wanted):
    """More table rows than destinations: the fused check would not see rows >= n_dst, the compare pass in front does."""
    P, L = small_tables_wanted, tfg._lib
    plan, x, w, sc = _small(tfg, 2000, 30000, 100, seed=5, n_src=2600)
    for _ in range(3):
        P.segment_reduce(plan, x, L.SUM, w_csr=w, self_coef=sc)
    assert "split_rows_compare_kernel" in P.segment_reduce(plan, x, L.SUM, w_csr=w, self_coef=sc, describe=True)
    x.data[2500, 7] += 1.0                                                   # a row no destination's self-loop reads
    got = P.segment_reduce(plan, x, L.SUM, w_csr=w, self_coef=sc)
    assert torch.equal(got, _plain(P, plan, x, L.SUM, w_csr=w, self_coef=sc))
    torch.cuda.synchronize()
    P.segment_reduce(plan, x, L.SUM, w_csr=w, self_coef=sc)
    assert _entry(P, plan, x).demoted


def _poke_through_out(P, x, row, col, delta):
    """Change ONE element of x through this library's out= (tfgx_gather_rows_f32 into a view of x.data): the version counter
    that moves is x.data's, not x's."""
    src = x[row:row + 1].clone()
    src[0, col] += delta
    idx = torch.zeros(1, dtype=torch.int32, device=x.device)
    v = x._version
    P.gather_rows(src, idx, out=x.data[row:row + 1])
    assert x._version == v


def _write_behind_the_counter(tfg, P, plan, x, w, sc, row):
    L = tfg._lib
    kw = dict(w_csr=w, self_coef=sc)
    for _ in range(3):
        P.segment_reduce(plan, x, L.SUM, **kw)
    ent = _entry(P, plan, x)
    assert ent is not None and ent.rows is not None
    demos = P.VERIFIED_STATS["demotions"]
    _poke_through_out(P, x, row, 3, 1.0)
    got = P.segment_reduce(plan, x, L.SUM, **kw)                             # the check fails, the repair recomputes
    assert torch.equal(got, _plain(P, plan, x, L.SUM, **kw))
    torch.cuda.synchronize()                                                 # (the host learns of it on a later call)
    again = P.segment_reduce(plan, x, L.SUM, **kw)
    assert torch.equal(again, got) and ent.demoted and ent.rows is None
    assert P.VERIFIED_STATS["demotions"] == demos + 1
    for _ in range(2):                                                       # demotion is permanent for this storage
        assert torch.equal(P.segment_reduce(plan, x, L.SUM, **kw), got)
    assert _entry(P, plan, x) is ent and ent.demoted
    assert "seg_reduce_verify_kernel" not in P.segment_reduce(plan, x, L.SUM, describe=True, **kw)


def test_small_write_behind_the_version_counter(tfg, small_tables_wanted):
    plan, x, w, sc = _small(tfg, 3000, 40000, 100, seed=11)
    _write_behind_the_counter(tfg, small_tables_wanted, plan, x, w, sc, row=1234)


def test_products_write_behind_the_version_counter(tfg, products):
    from tf_geometric_amd import plan as P
    p = products
    x = p["x"].clone()
    _write_behind_the_counter(tfg, P, p["plan"], x, p["w_csr"], p["sc"], row=1234567)


def test_products_promoted_route_is_bit_identical_and_queues_without_a_sync(tfg, products):
    from tf_geometric_amd import plan as P
    L = tfg._lib
    p = products
    x = p["x"].clone()
    kw = dict(w_csr=p["w_csr"], self_coef=p["sc"])
    ref = _plain(P, p["plan"], x, L.SUM, **kw)
    out = torch.empty_like(ref)
    for _ in range(3):
        P.segment_reduce(p["plan"], x, L.SUM, out=out, **kw)
        assert torch.equal(out, ref)
    assert _entry(P, p["plan"], x).rows is not None
    assert P.segment_reduce(p["plan"], x, L.SUM, describe=True, **kw).startswith("seg_reduce_verify_kernel<4, 32, 1, false, true")
    torch.cuda.synchronize()
    stream = torch.cuda.current_stream()
    served = P.VERIFIED_STATS["served"]
    for _ in range(10):                                                      # ~80 ms of device work
        P.segment_reduce(p["plan"], x, L.SUM, out=out, **kw)
    assert not stream.query(), "the host waited for the device"
    assert P.VERIFIED_STATS["served"] == served + 10
    torch.cuda.synchronize()
    assert torch.equal(out, ref)


def test_products_fresh_content_under_a_reused_pointer(tfg, products):
    """A table freed and another one allocated at the same address (version counter 0 again, same shape): it is a new
    sighting, read as it is — and a layout never outlives the storage it was built from."""
    from tf_geometric_amd import plan as P
    L = tfg._lib
    p = products
    kw = dict(w_csr=p["w_csr"], self_coef=p["sc"])
    t1 = p["x"].clone()
    for _ in range(3):
        P.segment_reduce(p["plan"], t1, L.SUM, **kw)
    ent = _entry(P, p["plan"], t1)
    assert ent is not None and ent.rows is not None
    ptr = t1.data_ptr()
    del t1
    assert ent.rows is None                                                  # freed with the storage (weakref.finalize)
    t2 = torch.empty_like(p["x"])
    t2.copy_(p["x"] * 3.0)
    got = P.segment_reduce(p["plan"], t2, L.SUM, **kw)
    assert torch.equal(got, _plain(P, p["plan"], t2, L.SUM, **kw))
    if t2.data_ptr() == ptr:
        assert _entry(P, p["plan"], t2) is not ent
    got2 = P.segment_reduce(p["plan"], t2, L.SUM, **kw)                      # second sighting of t2: promoted, same bits
    assert torch.equal(got2, got)


def test_nothing_is_memoised_under_capture(tfg, small_tables_wanted):
    P, L = small_tables_wanted, tfg._lib
    plan, x, w, sc = _small(tfg, 3000, 40000, 100, seed=21)
    kw = dict(w_csr=w, self_coef=sc)
    ref = _plain(P, plan, x, L.SUM, **kw)
    out = torch.empty_like(ref)
    cap = tfg.CapturedForward(lambda: P.segment_reduce(plan, x, L.SUM, out=out, **kw))
    assert _entry(P, plan, x) is None                                        # warm-up and capture recorded nothing
    for _ in range(3):
        assert torch.equal(cap(), ref)
    assert _entry(P, plan, x) is None
    # a table promoted by eager calls is read as it is inside a capture (a replay cannot be demoted by the host)
    for _ in range(3):
        P.segment_reduce(plan, x, L.SUM, **kw)
    ent = _entry(P, plan, x)
    assert ent is not None and ent.rows is not None
    served = P.VERIFIED_STATS["served"]
    cap2 = tfg.CapturedForward(lambda: P.segment_reduce(plan, x, L.SUM, out=out, **kw))
    assert P.VERIFIED_STATS["served"] == served
    x.copy_(x * 2.0)
    assert torch.equal(cap2(), ref * 2.0)
