# coding=utf-8
"""Census and comparator check of tests/graph_prep_cases.py, without a device: every path that tests/test_gpu_graph_prep.py is
meant to reach is reached by a default draw (recomputed from the draw), the conditions behind the bars hold, the float32 numpy
evaluation of the normalisation passes every comparator on every draw (none is skipped), and the comparators reject each planted
error — so the GPU tests would fail on a subtly wrong kernel without one ever being built."""
import numpy as np
import pytest

import graph_prep_cases as gp


# ---- census ----------------------------------------------------------------------------------------------------------------------
def test_every_named_path_is_reached_by_a_default_draw():
    reached = set()
    for name in gp.NORM_DRAWS:
        d = gp.norm_draw(name)
        found = gp.norm_paths(d)
        assert set(d["paths"]) <= found, "{} misses {}".format(name, sorted(set(d["paths"]) - found))
        reached |= set(d["paths"])
    assert reached >= set(gp.REQUIRED_NORM_PATHS), sorted(set(gp.REQUIRED_NORM_PATHS) - reached)


def test_draw_shapes():
    lens = gp.row_lengths(gp.norm_draw("long"))
    assert lens[0] > gp.K_LONG and lens[-1] > gp.K_LONG and lens[5] == gp.K_LONG
    assert gp.long_rows(gp.norm_draw("long")).size == 7 and 200 <= gp.norm_draw("long")["n_rows"] <= 999
    tile = gp.norm_draw("tile")
    assert list(gp.long_rows(tile)) == list(range(gp.TILE)) and tile["n_rows"] == 40
    g2 = gp.norm_draw("grid2")
    assert g2["n_rows"] == 8191 * 32 + 40 and list(gp.long_rows(g2)) == [g2["n_rows"] - 5]
    assert 3.5 < g2["row"].size / g2["n_rows"] < 4.5
    assert int(np.bincount(gp.norm_draw("long")["col"]).max()) >= 2049
    for name, shape in (("rect7x11", (7, 11)), ("rect300x40", (300, 40)), ("rect40x30", (40, 30)), ("empty", (1, 1))):
        d = gp.norm_draw(name)
        assert (d["n_rows"], d["n_cols"]) == shape
    assert gp.norm_draw("empty")["row"].size == 0
    assert len(gp.configs_for(gp.norm_draw("long"))) == 24
    assert [c[0] for c in gp.configs_for(gp.norm_draw("rect7x11"))] == ["both"] * 4 + ["left"]
    assert ("right", False, False, True, False) in gp.configs_for(gp.norm_draw("rect40x30"))


def test_weights_are_what_the_bars_assume():
    for name in gp.NORM_DRAWS:
        d = gp.norm_draw(name)
        q, u = gp.weights(d, "quantised"), gp.weights(d, "uniform")
        assert gp.weights(d, "unweighted") is None and q.dtype == u.dtype == np.float32
        assert (np.abs(q) * 4 == np.round(np.abs(q) * 4)).all() and (np.abs(q) >= 0.25).all() and (np.abs(q) <= 1.75).all()
        assert (np.abs(u) >= 0.5).all() and (np.abs(u) <= 1.5).all()
        if d["sign"] is None:
            assert (q > 0).all() and (u > 0).all()
        else:
            assert (q < 0).any() and (u < 0).any()
        for mode in ("quantised", "uniform"):
            w64 = gp.weights(d, mode).astype(np.float64)
            for idx, n in ((d["row"], d["n_rows"]), (d["col"], d["n_cols"])):
                _, s, a = gp._sums(idx, w64, n)
                for diag in sorted({gp.fill_diag(cfg)[1] for cfg in gp.configs_for(d)}):
                    deg, total = s + diag, a + diag
                    nz = deg != 0.0
                    assert (np.abs(deg[nz]) >= 0.25 * total[nz]).all(), (name, mode, diag)
                    if mode == "quantised":
                        assert (deg.astype(np.float32).astype(np.float64) == deg).all() and (total < 2.0 ** 22).all()


def test_degenerate_draw_holds_its_three_nodes():
    d = gp.norm_draw("degenerate")
    for mode in ("quantised", "uniform"):
        w = gp.weights(d, mode).astype(np.float64)
        deg = np.bincount(d["row"], weights=w, minlength=24)
        cdeg = np.bincount(d["col"], weights=w, minlength=24)
        assert deg[21] == 0.0 and (d["row"] == 21).sum() == 2 and deg[23] < 0.0 and (w[d["row"] == 23] < 0).all()
        assert not (d["row"] == 20).any() and (d["col"] == 20).any() and cdeg[22] == 0.0 and cdeg[19] < 0.0
        # a negative degree: 0 under "both", a finite negative factor under "left" / "right"
        both = gp.reference(d, gp.weights(d, mode), ("both", True, False, True, False))
        left = gp.reference(d, gp.weights(d, mode), ("left", True, False, True, False))
        assert (both["w_out"][d["row"] == 23] == 0.0).all() and (left["w_out"][d["row"] == 23] > 0.0).all()
        assert (left["w_out"][d["row"] == 21] == 0.0).all()


def test_merge_draws_cross_every_width_and_block_boundary():
    assert {gp.hash_class(n) for n in gp.HASH_N} == {"below-2^31", "2^31-to-2^32", "exactly-2^32", "above-2^32", "62-bits"}
    assert gp.hash_class(46340) == "below-2^31" and gp.hash_class(46341) == "2^31-to-2^32"
    assert gp.hash_class(65535) == "2^31-to-2^32" and gp.hash_class(65537) == "above-2^32" and gp.hash_class(2 ** 31 - 1) == "62-bits"
    for n in gp.HASH_N:
        ei = gp.hash_draw(n)
        assert ei.dtype == np.int32 and int(ei.max()) + 1 == n and ei.min() >= 0 and 200 <= ei.shape[1] <= 999
        assert ((ei[0] == n - 1) & (ei[1] == n - 1)).sum() >= 2
    assert {gp.edge_count_class(E) for E in gp.EDGE_COUNTS} == {"below-block", "one-block", "block+1", "many-blocks"}
    for E in gp.EDGE_COUNTS:
        for mix in gp.MIXES:
            ei = gp.edge_draw(E, mix)
            assert ei.shape == (2, E)
            if E > 70001:
                continue
            U = np.unique(ei[0].astype(np.int64) * (int(ei.max()) + 1) + ei[1]).size
            if mix == "no-duplicates":
                assert U == E
            elif mix == "all-same":
                assert U == 1
            elif mix == "half-duplicated":
                assert U <= max(1, E // 2) and (E < 4 or U > E // 4)
            elif E >= 255:
                assert (ei[0] == ei[1]).sum() > E // 3 and U < E
    hub = gp.hub_draw()
    assert ((hub[0] == 2) & (hub[1] == 7)).sum() >= gp.HUB_COPIES


# ---- the float32 evaluation passes every comparator ---------------------------------------------------------------------------------
@pytest.mark.parametrize("name", gp.NORM_DRAWS)
def test_float32_evaluation_passes_every_comparator(name):
    d = gp.norm_draw(name)
    compared = 0
    for mode in gp.WEIGHT_MODES:
        w = gp.weights(d, mode)
        worst = {}
        for cfg in gp.configs_for(d):
            ref = gp.reference(d, w, cfg)
            res = gp.f32_eval(d, w, cfg)
            stats = gp.compare(res, ref, gp.exact_mode(mode), what="{} {} {}".format(name, mode, gp.nm.config_id(cfg)))
            public = dict(w_out=res["w_out"][:-gp.GUARD], self_coef=res["self_coef"][:-gp.GUARD] if ref["has_self_coef"] else None)
            gp.compare(public, ref, gp.exact_mode(mode), what="public", guard=False)
            for k, v in stats.items():
                worst[k] = max(worst.get(k, 0.0), v)
            compared += 1
        print("{} {}: worst error / bar {}".format(name, mode, {k: round(v, 3) for k, v in sorted(worst.items())}))
        if gp.exact_mode(mode) and d["row"].size:
            assert worst["w_out"] <= 6.0 / 16.0       # six correctly rounded operations: at most 6 * 2^-24 (measured: 3.9)
    assert compared == len(gp.WEIGHT_MODES) * len(gp.configs_for(d))           # the share of skipped draws is zero


def test_edge_permutation_and_relabelling_keep_float32_bits():
    """The identities the GPU test asserts hold for exact-degree float32 arithmetic."""
    for name in gp.IDENTITY_DRAWS:
        d = gp.norm_draw(name)
        w = gp.weights(d, "quantised")
        E, n = d["row"].size, d["n_rows"]
        for cfg in (("both", False, True, True, False), ("right", True, True, True, True)):
            base = gp.f32_eval(d, w, cfg)
            de, q = gp.permuted_edges(d)
            moved = gp.f32_eval(de, np.ascontiguousarray(w[q]), cfg)
            assert np.array_equal(gp._bits(moved["w_out"][:E]), gp._bits(base["w_out"][:E][q]))
            dn, p = gp.relabelled(d)
            named = gp.f32_eval(dn, w, cfg)
            assert np.array_equal(gp._bits(named["w_out"][:E]), gp._bits(base["w_out"][:E]))
            assert np.array_equal(gp._bits(named["self_coef"][:n][p]), gp._bits(base["self_coef"][:n]))


# ---- planted errors ----------------------------------------------------------------------------------------------------------------
def _rejects(d, mode, cfg, kind, match):
    w = gp.weights(d, mode)
    ref = gp.reference(d, w, cfg)
    gp.compare(gp.f32_eval(d, w, cfg), ref, gp.exact_mode(mode))
    with pytest.raises(AssertionError, match=match):
        gp.compare(gp.planted(d, w, cfg, kind), ref, gp.exact_mode(mode), what=kind)


@pytest.mark.parametrize("mode", gp.WEIGHT_MODES)
@pytest.mark.parametrize("name", ["long", "tile", "grid2", "rect300x40"])
def test_a_long_row_degree_without_its_last_edge_is_rejected(name, mode):
    d = gp.norm_draw(name)
    for cfg in gp.configs_for(d)[:1] + gp.configs_for(d)[-1:]:
        _rejects(d, mode, cfg, "degree-drops-last-edge", "row_deg")


def test_the_value_comparator_alone_rejects_a_wrong_hub_degree():
    """The public route shows no degrees: the 1 / 2049 of a dropped edge must fail on the normalised weights (the absolute 1e-5
    would let it through: a hub's weights are about 1 / degree)."""
    d = gp.norm_draw("long")
    for mode in gp.WEIGHT_MODES:
        w = gp.weights(d, mode)
        for cfg in (("both", True, True, True, False), ("left", True, True, True, False), ("right", True, False, True, False)):
            ref = gp.reference(d, w, cfg)
            bad = gp.planted(d, w, cfg, "degree-drops-last-edge")
            wrong = dict(w_out=bad["w_out"][:-gp.GUARD], self_coef=bad["self_coef"][:-gp.GUARD] if ref["has_self_coef"] else None)
            err = np.abs(wrong["w_out"] - ref["w_out"])
            assert (err <= 1e-5 + 1e-5 * np.abs(ref["w_out"])).all()          # inside assert_parity's bar, which is NOT used here
            with pytest.raises(AssertionError, match="w_out"):
                gp.compare(wrong, ref, gp.exact_mode(mode), what="public", guard=False)


@pytest.mark.parametrize("mode", gp.WEIGHT_MODES)
def test_an_unwritten_remainder_edge_is_rejected(mode):
    for name in ("long", "grid2", "rect40x30"):
        d = gp.norm_draw(name)
        _rejects(d, mode, gp.configs_for(d)[0], "remainder-edge-unwritten", "NaN or inf")


@pytest.mark.parametrize("mode", gp.WEIGHT_MODES)
def test_the_row_degree_in_place_of_the_column_degree_is_rejected(mode):
    for name in ("short", "long", "tile", "degenerate"):
        d = gp.norm_draw(name)
        for cfg in (("both", False, True, True, False), ("both", False, False, False, True)):
            _rejects(d, mode, cfg, "row-degree-for-column", "w_out")


def test_a_written_guard_is_rejected():
    for name in gp.NORM_DRAWS:
        d = gp.norm_draw(name)
        _rejects(d, "quantised", gp.configs_for(d)[0], "guard-written", "guard")


def test_a_zeroed_factor_returned_as_inf_is_rejected():
    d = gp.norm_draw("degenerate")
    for mode in gp.WEIGHT_MODES:
        for cfg in (("both", True, False, True, False), ("both", False, False, True, False), ("right", True, False, True, False)):
            if mode == "unweighted" and not cfg[1]:
                continue          # without signs every row and column that has an edge has a positive degree
            _rejects(d, mode, cfg, "zero-factor-inf", "NaN or inf")


def test_the_merge_comparator_rejects_a_wrong_modulus():
    for n in gp.HASH_N:
        ei = gp.hash_draw(n)
        ref_u, _, _ = gp.merge_reference(ei, gp.props_for(ei), gp.MODES)
        gp.check_merged("n={}".format(n), ref_u, ref_u)
        if n == 1:
            continue          # one node: every key is 0 under any modulus
        with pytest.raises(AssertionError, match="unique edges differ"):
            gp.check_merged("n={}".format(n), gp.wrong_merge(ei), ref_u)


def test_merge_reference_on_a_hand_example():
    ei = np.array([[3, 1, 3, 1, 0], [2, 1, 2, 1, 3]], np.int32)
    p = np.array([1.0, 2.0, 4.0, -8.0, 16.0], np.float32)
    u, (s, m, hi, lo), tol = gp.merge_reference(ei, p, gp.MODES)
    assert u.tolist() == [[3, 1, 0], [2, 1, 3]]
    assert s.tolist() == [5.0, -6.0, 16.0] and m.tolist() == [2.5, -3.0, 16.0]
    assert hi.tolist() == [4.0, 2.0, 16.0] and lo.tolist() == [1.0, -8.0, 16.0]
    assert tol[0] == pytest.approx(1e-5 * 4.0) and tol[2] is None and tol[3] is None
    u3, out3, _ = gp.merge_reference(ei, np.stack([p, -p, 2 * p], axis=1), gp.MODES)
    assert out3[0].shape == (3, 3) and out3[0][:, 2].tolist() == [10.0, -12.0, 32.0] and out3[2][:, 1].tolist() == [-1.0, 8.0, -16.0]
    up, uw, de, dw, _ = gp.upper_reference(np.array([[1, 3, 5], [2, 1, 4]], np.int32), np.ones(3, np.float32))
    assert de.tolist() == [[1, 1, 4, 2, 3, 5], [2, 3, 5, 1, 1, 4]] and dw.tolist() == [1.0] * 6
    assert gp.upper_reference(np.array([[4, 4, 2], [4, 4, 2]], np.int32), np.ones(3, np.float32))[2] is None
