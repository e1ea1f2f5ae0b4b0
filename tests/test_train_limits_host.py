"""The crafted inputs of tests/test_train_limits.py are what they claim -- proved here on the restatement tests/train_ref.py
alone, without a GPU, for every seed listed below.  The GPU tests import these case lists and builders, so what is proved
here is proved about the cases they run.  No builder drops or redraws anything until its property holds: a set is made once
from its seed (train_ref.make_few_valued / make_extreme / make_samples) and the property is asserted on it as it came out.
Dialect CPP is parity-unpinned: the yardstick is this repo's restatement of the reference's source, not the reference."""
import functools

import numpy as np
import pytest

import train_ref

# (seed, pos_n, neg_n, L, multi_scale, F): the few-valued set at the counts of the collision item -- one full batch of
# k_train_hist, one batch and one entry, two batches and one entry, four batches and 44 entries
FEW_CASES = [(61, 64, 65, 5, True, 24), (62, 65, 129, 5, False, 24), (63, 129, 64, 27, True, 24), (64, 300, 300, 5, True, 24)]
FEW_SPREAD = 8.0                    # the score spread the order control below needed: make_samples' own, nothing was widened
EXTREME_CASES = [(71, 129, 65, 5, True, 24), (72, 64, 257, 27, False, 24)]
# regression: (maker, seed, pos_n, L, multi_scale, F); every case runs under the three u of U_KINDS
REG_CASES = [("random", 81, 257, 5, True, 24), ("few", 82, 129, 5, True, 24), ("random", 83, 65, 27, False, 24)]
U_KINDS = ("pool", "zero", "top")
MAKERS = dict(random=train_ref.make_samples, few=train_ref.make_few_valued, extreme=train_ref.make_extreme)


def u_of(kind, u):
    """The pool's own draws, all 0.0 (kidx 0) or all nextafter(1, 0) (kidx pos_n - 1 through the min of cart.cpp:320)."""
    return list(u) if kind == "pool" else [0.0 if kind == "zero" else float(np.nextafter(1., 0.))] * len(u)


@functools.lru_cache(maxsize=None)
def node(maker, seed, pos_n, neg_n, L, multi, F, sizes=(48, 36, 24)):
    """One node's inputs and the restatement's values on the full lists -> (pd, nd, rows, u, pos, neg, pf, nf)."""
    pd, nd = MAKERS[maker](seed, pos_n, L, sizes), MAKERS[maker](seed + 100, neg_n, L, sizes)
    rows, u = train_ref.gen_feature_pool(F, L, train_ref.RADIUS, multi, seed, 1)
    pos, neg, pool = train_ref.ref_set(pd), train_ref.ref_set(nd), train_ref.pool_of(rows)
    pf = train_ref.calc_feature_values(pos, pool, list(range(pos_n)))
    nf = train_ref.calc_feature_values(neg, pool, list(range(neg_n)))
    return pd, nd, rows, u, pos, neg, pf, nf


def classification(pos, neg, pf, nf, reverse=False):
    detail = {}
    out = train_ref.split_classification(pos, list(range(pos.n)), neg, list(range(neg.n)), pf, nf, reverse=reverse, detail=detail)
    return out, detail


def bits(rows):
    return np.array(rows, np.float64).view(np.uint64)


@pytest.mark.parametrize("case", FEW_CASES)
def test_few_valued_set_collides_deeply_opens_gates_and_shows_the_order(case):
    seed, pos_n, neg_n, L, multi, F = case
    pd, nd, rows, u, pos, neg, pf, nf = node("few", *case)
    assert all(len(set(r)) <= 5 for r in pf + nf) and max(len(set(r)) for r in pf) >= 3
    # in every full 64-entry batch the most-hit bin gets at least 16 entries: ranks 0 .. 15 and deeper in every batch
    (plo, phi), (nlo, nhi) = train_ref.deepest_rank(pf, pos_n), train_ref.deepest_rank(nf, neg_n)
    print("case %r: most-hit bin of a batch, positives %d .. %d entries, negatives %d .. %d: deepest rank %d"
          % (case, plo, phi, nlo, nhi, max(phi, nhi) - 1))
    assert plo >= 16 and nlo >= 16
    (fi, th, es, ths), d = classification(pos, neg, pf, nf)
    # the histograms reach the criterion: bins that hold 10-90 % of both classes, and gates that opened
    wide = [sum(0.1 * pos_n <= d["p_n"][i][b] <= 0.9 * pos_n and 0.1 * neg_n <= d["n_n"][i][b] <= 0.9 * neg_n for b in range(511))
            for i in range(F)]
    opened = sum(t != -256 for t in ths)
    print("features with three such bins: %d of %d; gates opened for %d" % (sum(w >= 3 for w in wide), F, opened))
    assert max(wide) >= 3 and opened > F // 2 and th != -256
    # the second opinion on the ordered histogram
    for i in range(F):
        assert train_ref.ordered_histogram(pf[i], list(range(pos_n)), pos.weights) == d["wp"][i]
        assert train_ref.ordered_histogram(nf[i], list(range(neg_n)), neg.weights) == d["wn"][i]
    # the order is visible in the bits of the weighted histograms (score spread FEW_SPREAD)
    _, r = classification(pos, neg, pf, nf, reverse=True)
    differ = sum(not np.array_equal(bits(d["wp"][i]), bits(r["wp"][i])) or not np.array_equal(bits(d["wn"][i]), bits(r["wn"][i]))
                 for i in range(F))
    print("reversed order changes the weighted histograms of %d of %d features" % (differ, F))
    assert differ > F // 2 and r["p_n"] == d["p_n"] and r["n_n"] == d["n_n"]


def test_flat_set_is_one_bin_with_ranks_to_63_and_its_order_is_visible():
    """The existing one_value corner (tests/test_train.py): every value 0, every batch one bin, 64 rounds."""
    pd, nd, rows, _ = (train_ref.make_samples(31, 260, 5, flat=True), train_ref.make_samples(131, 230, 5, flat=True),
                       *train_ref.gen_feature_pool(24, 5, train_ref.RADIUS, True, 31, 1))
    pos, neg, pool = train_ref.ref_set(pd), train_ref.ref_set(nd), train_ref.pool_of(rows)
    pf = train_ref.calc_feature_values(pos, pool, list(range(260)))
    nf = train_ref.calc_feature_values(neg, pool, list(range(230)))
    assert all(set(r) == {0} for r in pf + nf) and train_ref.deepest_rank(pf, 260) == (64, 64)
    (_, th, _, ths), d = classification(pos, neg, pf, nf)
    assert th == -256 and set(ths) == {-256}                # no gate opens: the criterion does not read the histogram
    _, r = classification(pos, neg, pf, nf, reverse=True)
    assert not np.array_equal(bits(d["wp"]), bits(r["wp"])) and not np.array_equal(bits(d["wn"]), bits(r["wn"]))


@pytest.mark.parametrize("case", EXTREME_CASES)
def test_extreme_set_fills_the_end_bins_and_the_order_statistic_lands_on_them(case):
    seed, pos_n, neg_n, L, multi, F = case
    pd, nd, rows, u, pos, neg, pf, nf = node("extreme", *case)
    assert all(set(r) <= {-255, 0, 255} for r in pf + nf)
    _, d = classification(pos, neg, pf, nf)
    both = sum(d["p_n"][i][0] > 0 and d["p_n"][i][510] > 0 and d["n_n"][i][0] > 0 and d["n_n"][i][510] > 0 for i in range(F))
    assert both > F // 2
    outside = sum(not (0. <= v <= 1.) for s in pos.shapes for v in s)
    assert 0 < outside < pos_n * 2 * L                     # shapes inside and pushed outside the patch
    reg = {}
    train_ref.split_regression(pos, list(range(pos_n)), pf, u, detail=reg)
    assert -255 in reg["th"] and 255 in reg["th"]


@pytest.mark.parametrize("case", REG_CASES)
def test_regression_sets_reach_both_ends_ties_and_an_empty_side(case):
    maker, seed, pos_n, L, multi, F = case
    pd, nd, rows, u, pos, neg, pf, nf = node(maker, seed, pos_n, 8, L, multi, F)
    det = {}
    for kind in U_KINDS:
        det[kind] = {}
        train_ref.split_regression(pos, list(range(pos_n)), pf, u_of(kind, u), detail=det[kind])
    assert set(det["zero"]["kidx"]) == {0} and set(det["top"]["kidx"]) == {pos_n - 1}
    assert all(0 < k < pos_n - 1 for k in det["pool"]["kidx"])
    # ties at the threshold (claimed for the few-valued set, reported for the others): several samples equal it, so `<=` and
    # `<` part the samples differently
    ties = [sum(v == det["pool"]["th"][i] for v in pf[i]) for i in range(F)]
    print("case %r: samples equal to the threshold per feature: %d .. %d" % (case, min(ties), max(ties)))
    assert maker != "few" or min(ties) >= 3
    # one side empty: the largest value as threshold sends everybody left
    assert set(det["top"]["n_right"]) == {0} and min(det["top"]["n_left"]) == pos_n
    assert all(det["top"]["th"][i] == max(pf[i]) and det["zero"]["th"][i] == min(pf[i]) for i in range(F))
    # the search ends on the last bin for the extreme set's features (value 255 present): see the extreme test; here the
    # count histogram is the values' own
    assert all(sum(c) == pos_n for c in det["pool"]["counts"])


def test_has_gt_all_zero_empties_both_sides():
    maker, seed, pos_n, L, multi, F = REG_CASES[0]
    pd, nd, rows, u, pos, neg, pf, nf = node(maker, seed, pos_n, 8, L, multi, F)
    none = train_ref.SampleSet([], [], [])
    none.patches, none.shapes, none.weights, none.residual, none.has_gt, none.n = pos.patches, pos.shapes, pos.weights, pos.residual, [0] * pos_n, pos_n
    d = {}
    _, _, vs, _ = train_ref.split_regression(none, list(range(pos_n)), pf, u, detail=d)
    assert set(d["n_left"]) == {0} and set(d["n_right"]) == {0} and set(vs) == {0.}


def test_pairwise_cover_covers():
    """The cover the shape sweeps run: every pair of values of two factors occurs, every value at least twice."""
    import test_train_limits as gpu_tests
    for rows, factors, allowed in ((gpu_tests.CLS_ROWS, gpu_tests.CLS_FACTORS, gpu_tests.cls_allowed),
                                   (gpu_tests.REG_ROWS, gpu_tests.REG_FACTORS, gpu_tests.reg_allowed)):
        for i in range(len(factors)):
            for a in factors[i]:
                assert sum(r[i] == a for r in rows) >= 2, (i, a)
            for j in range(i + 1, len(factors)):
                for a in factors[i]:
                    for b in factors[j]:
                        assert not allowed({i: a, j: b}) or any(r[i] == a and r[j] == b for r in rows), (i, a, j, b)
        assert all(allowed(dict(enumerate(r))) for r in rows)
    assert any(r[0] == 0 and r[1] > 0 for r in gpu_tests.CLS_ROWS) and any(r[1] == 0 and r[0] > 0 for r in gpu_tests.CLS_ROWS)
    print("mode 1: %d cases, mode 0: %d cases" % (len(gpu_tests.CLS_ROWS), len(gpu_tests.REG_ROWS)))
