# coding=utf-8
"""The drawn bits of the neighbour sampler, pinned by an expectation that does not come from any kernel: sampler_mirror.py
restates csrc/tfgx_sample_rows.h in Python integers.  The whole-graph sampler must equal it exactly; test_gpu_nbrblock.py,
test_gpu_nbrstatic.py and test_gpu_samplereduce.py then pin sample_rows, sample_blocks and the static and fused forms to the
whole-graph sampler."""
import numpy as np
import pytest

import sampler_mirror as SM
from test_gpu_nbrblock import world, HUB       # noqa: F401  (the 401-node graph: every branch of the per-row sampler)

SEEDS = [3, 2 ** 61 + 12345]
# (d, m): six long rows (the wave's strata), three for Floyd, two for the lane's Algorithm S (d <= 64 < 2 * m)
SHAPES = [(5000, 40), (5000, 2500), (100, 40), (100, 50), (100, 70), (65, 33), (33, 32), (20, 5), (6, 5), (64, 33), (40, 35)]


@pytest.mark.parametrize("seed", SEEDS)
def test_the_mirror_draws_m_distinct_positions(seed):
    for row in (0, 8, 399):
        for d, m in SHAPES:
            p = SM.sample_row(seed, row, d, m)
            assert len(p) == m and len(set(p)) == m and min(p) >= 0 and max(p) < d, (row, d, m)
            if m > SM.FLOYD_MAX:                                   # both selection branches keep the neighbour order
                assert p == sorted(p), (row, d, m)
            q = SM.sample_row(seed, row, d, d + 3, padding=True)   # with replacement: every draw in range
            assert len(q) == d + 3 and min(q) >= 0 and max(q) < d
            assert SM.sample_row(seed, row, d, d) == list(range(d))
    assert [SM.row_is_long(d, m) for d, m in SHAPES] == [True] * 6 + [False] * 5
    assert [SM.draws(7, k=5), SM.draws(3, k=5), SM.draws(3, k=5, padding=True), SM.draws(0, k=5, padding=True),
            SM.draws(5, ratio=0.5), SM.draws(5000, ratio=0.5), SM.draws(9)] == [5, 3, 5, 0, 3, 2500, 9]
    assert SM.draw_u32(seed, 8, 0) != SM.draw_u32(seed, 8, 1) and 0 <= SM.draw_u32(seed, 2 ** 40, 0xFFFFFFFF) < 2 ** 32


@pytest.mark.gpu
@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("kw", [dict(k=5), dict(k=32), dict(k=33), dict(k=40), dict(ratio=0.5), dict(k=8, padding=True)],
                         ids=lambda kw: "-".join("{}={}".format(*i) for i in kw.items()))
def test_the_whole_graph_sampler_equals_the_mirror(world, kw, seed):     # noqa: F811
    s = world["sampler"]
    row_ptr, col, w = s.plan.row_ptr.cpu().numpy(), s.plan.col.cpu().numpy(), s.w_csr.cpu().numpy()
    rows, pos = SM.sample_graph(row_ptr, seed, **kw)
    if kw.get("k") == 40 or "ratio" in kw:
        assert SM.row_is_long(5000, rows.count(HUB))               # the wave path is among what is compared
    ei, ew = s.sample(seed=seed, **kw)
    want_ei = np.stack([np.asarray(rows, np.int32), col[pos].astype(np.int32)])
    assert np.array_equal(ei.cpu().numpy(), want_ei)
    assert np.array_equal(ew.cpu().numpy().view(np.uint32), w[pos].astype(np.float32).view(np.uint32))
