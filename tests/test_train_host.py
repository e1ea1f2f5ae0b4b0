"""CPU-side checks of the CART-training entries (include/jda.h, "Dialect CPP: training one CART"): the host-only pool
generator against a Python restatement of its documented draw order, the restatement tests/train_ref.py on hand-worked
tiny nodes, the refusals that need no device, and the CONTROL of the yardstick -- on the weight sets of the GPU tests,
summing in reversed sample order changes bits of the criteria, so "bit-exact in sample order" tests something."""
import math

import numpy as np
import pytest

from conftest import same
import train_ref


@pytest.mark.parametrize("L,multi", [(5, False), (27, True), (1, True)])
def test_gen_feature_pool_equals_the_documented_draw_order(built, L, multi):
    from jda_amd import api
    F, radius = 300, 0.37
    feats, u = api.gen_feature_pool_cpp(F, L, radius, multi, seed=0xDEADBEEFCAFE, key=17)
    want, want_u = train_ref.gen_feature_pool(F, L, radius, multi, 0xDEADBEEFCAFE, 17)
    for k, name in enumerate(("scale", "landmark_id1", "landmark_id2")):
        assert np.array_equal(feats[name], np.array([w[k] for w in want], np.int32)), name
    for k, name in enumerate(("offset1_x", "offset1_y", "offset2_x", "offset2_y")):
        assert same(np.ascontiguousarray(feats[name]), np.array([w[3 + k] for w in want])), name
    assert same(u, np.array(want_u))
    # Cart::GenFeaturePool's properties (cart.cpp:364-388)
    for a, b in (("offset1_x", "offset1_y"), ("offset2_x", "offset2_y")):
        assert ((feats[a] / radius) ** 2 + (feats[b] / radius) ** 2 <= 1. + 1e-12).all()
    assert ((feats["landmark_id1"] >= 0) & (feats["landmark_id1"] < L) & (feats["landmark_id2"] >= 0) & (feats["landmark_id2"] < L)).all()
    assert ((u >= 0.1) & (u < 0.9)).all()
    if multi:
        assert set(feats["scale"].tolist()) == {0, 1, 2}
    else:
        assert (feats["scale"] == 0).all()
    # another key, other draws; the same key, the same draws
    again, _ = api.gen_feature_pool_cpp(F, L, radius, multi, seed=0xDEADBEEFCAFE, key=17)
    other, _ = api.gen_feature_pool_cpp(F, L, radius, multi, seed=0xDEADBEEFCAFE, key=18)
    assert again.tobytes() == feats.tobytes() and other.tobytes() != feats.tobytes()


def test_gen_feature_pool_refuses_bad_arguments(built):
    from jda_amd import api
    for args in ((-1, 5, 0.3), (4, 0, 0.3), (4, 5, float("nan"))):
        with pytest.raises(api.JdaError):
            api.gen_feature_pool_cpp(*args)
    assert len(api.gen_feature_pool_cpp(0, 5, 0.3)[0]) == 0


class _W:
    def __init__(self, weights, residual=None, has_gt=None):
        self.weights, self.residual, self.has_gt = weights, residual, has_gt


def _h(p):                      # calcEntropy's expression (cart.cpp:171-172), by hand
    e = -(p) * math.log(p) - (1. - p) * math.log(1. - p)
    return e / math.log(2.)


def test_restatement_on_a_hand_worked_three_sample_node():
    # classification, 2 positives + 1 negative: n_ratio is 0 or 1 at every threshold, no gate ever opens, so the node keeps
    # threshold -256 and the entropy of p = (0.5 + 0.25) / 1.0 = 0.75 -- for either feature
    pos, neg = _W([0.5, 0.25]), _W([0.25])
    fi, th, es, ths = train_ref.split_classification(pos, [0, 1], neg, [0], [[10, -5], [3, 3]], [[0], [7]])
    assert (fi, th) == (0, -256) and ths == [-256, -256]
    assert es[0] == es[1] == _h(0.75)
    assert abs(es[0] - 0.8112781244591328) < 1e-15
    # regression, 3 positives, values (10, -5, 3), u = 0.5: sorted (-5, 3, 10)[int(3 * 0.5) = 1] = 3; left = samples 1, 2,
    # right = sample 0
    res = [(0.5, -1.0), (0.25, 0.5), (-0.75, 1.5)]
    fi, th, vs, ths = train_ref.split_regression(_W(None, res), [0, 1, 2], [[10, -5, 3]], [0.5])
    lx, ly = [0.25, -0.75], [0.5, 1.5]
    var = lambda v: sum(a * a for a in v) * (1. / len(v)) - (sum(v) * (1. / len(v))) ** 2
    by_hand = (var(lx) + var(ly)) * 2. + (0. + 0.) * 1.            # one sample on the right: variance 0
    assert (fi, th, ths) == (0, 3, [3]) and vs[0] == by_hand == (0.25 + 0.25) * 2.
    # ... with has_gt = 0 for sample 1 the left side is sample 2 alone: everything 0; the threshold is still taken over
    # ALL positives (cart.cpp:314-325)
    fi, th, vs, _ = train_ref.split_regression(_W(None, res, [1, 0, 1]), [0, 1, 2], [[10, -5, 3]], [0.5])
    assert (th, vs[0]) == (3, 0.)
    assert train_ref.split_regression(_W(None, res), [], [[], []], [0.5, 0.5]) == (0, -256, [0., 0.], [-256, -256])


def test_restatement_on_a_hand_worked_split():
    # 2 + 2 samples; feature 1 separates the classes at th = -10 (left: 0.4 pos + 0.1 neg, right: 0.1 + 0.4), feature 0
    # does not separate anything (one value: the gates stay shut)
    pos, neg = _W([0.4, 0.1]), _W([0.1, 0.4])
    fi, th, es, ths = train_ref.split_classification(pos, [0, 1], neg, [0, 1], [[5, 5], [-10, 20]], [[5, 5], [-10, 20]])
    assert es[0] == _h(0.5) and abs(es[0] - 1.) < 1e-15 and ths[0] == -256
    wp_r, wn_r = 0.5 - 0.4, 0.5 - 0.1                   # the sweep's running right sides (cart.cpp:220-221)
    e = (0.5 / 1.0) * _h(0.4 / 0.5) + ((wp_r + wn_r) / 1.0) * _h(wp_r / (wp_r + wn_r))
    assert (fi, th, ths[1]) == (1, -10, -10) and es[1] == e
    assert abs(e - 0.7219280948873623) < 1e-12          # H(0.8)


def _cascador(model_file, L=5, D=4):
    from jda_amd import api
    p, _ = model_file((1, 2, L, D))
    return api.Cascador(p, "double")


def test_refusals_that_need_no_device(built, model_file):
    from jda_amd import api
    c = _cascador(model_file)
    pos = train_ref.make_samples(1, 6, 5)
    neg = train_ref.make_samples(2, 5, 5)
    pool, u = api.gen_feature_pool_cpp(8, 5, 0.3, True, 1, 1)
    with pytest.raises(api.JdaError, match=r"\[1, 128\]"):
        c.calc_feature_values_cpp(dict(pos, patches=np.zeros((6, 129 * 129 + 2), np.uint8)), pool, 129, 1, 1)
    bad = pool.copy(); bad["scale"][3] = 3
    with pytest.raises(api.JdaError, match="scale"):
        c.split_node_cpp(pos, neg, bad, 1)
    bad = pool.copy(); bad["landmark_id2"][7] = 5
    with pytest.raises(api.JdaError, match="landmark"):
        c.calc_feature_values_cpp(pos, bad)
    with pytest.raises(api.JdaError, match="modes"):
        c.train_cart_cpp(pos, neg, np.tile(pool, 7), [1, 1, 2, 1, 1, 1, 1])
    with pytest.raises(api.JdaError, match="us"):
        c.train_cart_cpp(pos, neg, np.tile(pool, 7), [1, 1, 0, 1, 1, 1, 1])
    c.set_similarity_transform(True)
    for call in (lambda: c.calc_feature_values_cpp(pos, pool), lambda: c.split_node_cpp(pos, neg, pool, 1),
                 lambda: c.train_cart_cpp(pos, neg, np.tile(pool, 7), [1] * 7)):
        with pytest.raises(api.JdaError, match="data.cpp:168"):
            call()
    c.close()


@pytest.mark.parametrize("case", train_ref.CLS_CASES)
def test_control_reversed_summation_order_changes_the_criteria(case):
    """The yardstick's control: on the very weight sets tests/test_train.py uses, adding the weights of every bin and of
    both totals in reversed sample order changes bits of the criteria -- of the CHOSEN feature's too."""
    seed, pos_n, neg_n, L, multi, F = case
    pd, nd = train_ref.make_samples(seed, pos_n, L), train_ref.make_samples(seed + 100, neg_n, L)
    pos, neg = train_ref.ref_set(pd), train_ref.ref_set(nd)
    rows, _ = train_ref.gen_feature_pool(F, L, train_ref.RADIUS, multi, seed, 1)
    pool = train_ref.pool_of(rows)
    pi, ni = list(range(pos_n)), list(range(neg_n))
    pf, nf = train_ref.calc_feature_values(pos, pool, pi), train_ref.calc_feature_values(neg, pool, ni)
    fi, th, es, ths = train_ref.split_classification(pos, pi, neg, ni, pf, nf)
    fr, tr, er, thr = train_ref.split_classification(pos, pi, neg, ni, pf, nf, reverse=True)
    assert th != -256                                   # a real split: some gate opened
    differing = sum(1 for a, b in zip(es, er) if not same(np.float64(a), np.float64(b)))
    print("criteria whose bits change under reversed order: %d of %d; chosen: %r vs %r" % (differing, F, es[fi], er[fi]))
    assert differing >= F // 4
    assert not same(np.float64(es[fi]), np.float64(er[fi]))
    assert max(abs(a - b) for a, b in zip(es, er)) < 1e-9    # ... and nothing but the order changed
