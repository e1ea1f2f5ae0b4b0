"""The host entries of one step of the boosting loop (jdaBoostScoresCpp, jdaSampleOrderCpp, jdaScoreThresholdCpp,
jdaScoreCutCpp, jdaUpdateWeightsCpp, jdaGatherRowsCpp) against the sequential restatement tests/boost_ref.py, bit for bit:
every comparison is exact (`same`), there is no tolerance anywhere.  No GPU and no cascador.  Dialect CPP is
parity-unpinned: bit-exact against this repo's restatement of the reference's source, not against the reference."""
import math

import numpy as np
import pytest

from conftest import same
import boost_ref


@pytest.fixture(scope="module")
def api(built):
    from jda_amd import api
    return api


def f64(v):
    return np.array(v, np.float64)


def _refused(api, fn, *a, **kw):
    """The call raises and leaves a message in jdaGetLastError()."""
    with pytest.raises(api.JdaError) as e:
        fn(*a, **kw)
    assert api.last_error() and str(e.value) == api.last_error()
    return api.last_error()


# ---- order -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("scores,want", [boost_ref.TIES_4, boost_ref.TIES_8])
def test_tie_vectors(api, scores, want):
    assert boost_ref.qsort(scores)[0] == want                                 # the restatement itself
    order, srt = api.sample_order_cpp(scores)
    assert same(order, np.array(want, np.int32)) and same(srt, f64(scores)[want])


@pytest.mark.parametrize("halves", [False, True])
@pytest.mark.parametrize("n", [1, 2, 3, 64, 67, 1000])
def test_order_equals_the_restatement(api, n, halves):
    s = boost_ref.sort_input(1000 * halves + n, n, halves)
    want_order, want_sorted = boost_ref.qsort(s.tolist())
    order, srt = api.sample_order_cpp(s)
    assert same(order, np.array(want_order, np.int32)) and same(srt, f64(want_sorted))
    assert sorted(order.tolist()) == list(range(n)) and same(srt, s[order])
    assert (np.diff(srt) <= 0).all()
    stable = np.argsort(-s, kind="stable")
    if not halves:
        assert len(set(s.tolist())) == n and same(order, stable.astype(np.int32))       # without ties: a descending stable sort
    elif n >= 3:
        assert not np.array_equal(order, stable)                              # the control: the test sees the quicksort


def test_sorted_inputs(api):
    s = np.sort(boost_ref.sort_input(5, 200, True))
    for v in (s[::-1].copy(), s):                                             # descending, ascending
        want_order, want_sorted = boost_ref.qsort(v.tolist())
        order, srt = api.sample_order_cpp(v)
        assert same(order, np.array(want_order, np.int32)) and same(srt, f64(want_sorted))
    # a sorted set with ties is NOT a fixed point of the quicksort: what DataSet::is_sorted saves is visible
    assert boost_ref.qsort(s[::-1].tolist())[0] != list(range(200))


def test_order_nan_inf_empty(api):
    msg = _refused(api, api.sample_order_cpp, [1., math.nan, 0.])
    assert "NaN" in msg
    _refused(api, api.sample_order_cpp, [math.nan])
    s = [0., math.inf, -math.inf, 3., math.inf, -math.inf, -2.]
    order, srt = api.sample_order_cpp(s)
    assert order.tolist() == boost_ref.qsort(s)[0] and same(srt, f64(boost_ref.qsort(s)[1]))
    assert srt[0] == math.inf and srt[-1] == -math.inf
    order, srt = api.sample_order_cpp([])
    assert order.size == 0 and srt.size == 0
    assert api.lib.jdaSampleOrderCpp(None, 0, None, None) == 0                # n == 0 reads nothing
    assert api.lib.jdaSampleOrderCpp(None, 3, None, None) == -1 and api.last_error()
    assert api.lib.jdaSampleOrderCpp(None, -1, None, None) == -1 and api.last_error()


# ---- threshold and cut -------------------------------------------------------------------------------------------------

def test_cut_edges(api):
    srt = [5., 4., 4., 3., 2., 2., 2., 1., 0.5, 0.5]
    n = len(srt)
    for drop_n in (0, 1, n - 1, n, n + 5):
        th = api.score_threshold_cpp(srt, drop_n)
        assert th == boost_ref.threshold_by_number(srt, drop_n) == srt[max(0, n - 1 - drop_n)]
        keep, gone = api.score_cut_cpp(srt, th)
        assert keep == boost_ref.remove(srt, th) and gone == boost_ref.pre_remove(srt, th) == n - keep
    # ties straddling the cut all stay: drop_n = 4 lands on the middle one of the three 2.s
    th = api.score_threshold_cpp(srt, 4)
    assert th == 2. and api.score_cut_cpp(srt, th) == (7, 3)
    assert api.score_cut_cpp(srt, 6.) == (0, n)                               # th above every score
    assert api.score_cut_cpp(srt, -1.) == (n, 0)                              # ... and below
    assert api.score_cut_cpp(srt, math.inf) == (0, n) and api.score_cut_cpp(srt, -math.inf) == (n, 0)
    assert api.score_cut_cpp([], 0.) == (0, 0)
    _refused(api, api.score_threshold_cpp, [], 0)
    _refused(api, api.score_threshold_cpp, srt, -1)
    _refused(api, api.score_cut_cpp, srt, math.nan)


# ---- scores ------------------------------------------------------------------------------------------------------------

def _score_case(seed, pos_n, neg_n, leaf_n):
    rng = np.random.default_rng(seed)
    return (rng.normal(0, 1, leaf_n), rng.integers(0, leaf_n, pos_n), rng.integers(0, leaf_n, neg_n),
            rng.uniform(-8, 8, pos_n), rng.uniform(-8, 8, neg_n))


@pytest.mark.parametrize("normalize", [False, True])
def test_scores_after_a_cart(api, normalize):
    cs, pl, nl, ps, ns = _score_case(4, 67, 131, 4)
    keep = ps.copy()
    got = api.boost_scores_cpp(cs, pl, nl, ps, ns, normalize)
    assert same(ps, keep)                                                     # the wrapper works on copies
    wp, lp = boost_ref.update_scores(ps.tolist(), pl.tolist(), cs.tolist())
    wn, ln = boost_ref.update_scores(ns.tolist(), nl.tolist(), cs.tolist())
    mean, std = 0., 1.
    if normalize:
        mean, std = boost_ref.calc_mean_and_std(wp, wn)
        wp, wn = boost_ref.apply_mean_and_std(wp, mean, std), boost_ref.apply_mean_and_std(wn, mean, std)
        assert mean != 0. and std != 1.
    assert same(got["pos_scores"], f64(wp)) and same(got["neg_scores"], f64(wn))
    assert same(got["pos_last"], ps) and same(got["neg_last"], ns)
    assert same(f64([got["mean"], got["std"]]), f64([mean, std]))


def test_scores_degenerate_and_refused(api):
    # std == 0: every score equal after the cart -> 0 / 0 = NaN scores like the reference, and the call succeeds
    got = api.boost_scores_cpp([0.25], [0, 0], [0], [1., 1.], [1.], True)
    assert got["std"] == 0. and got["mean"] == 1.25
    assert np.isnan(got["pos_scores"]).all() and np.isnan(got["neg_scores"]).all()
    assert same(got["pos_last"], f64([1., 1.]))
    # an empty side, and both
    got = api.boost_scores_cpp([0.5, -0.5], [1, 0], [], [0., 0.], [], True)
    m, s = boost_ref.calc_mean_and_std([-0.5, 0.5], [])
    assert same(f64([got["mean"], got["std"]]), f64([m, s])) and got["neg_scores"].size == 0
    got = api.boost_scores_cpp([0.5], [], [], [], [], True)
    assert math.isnan(got["mean"]) and math.isnan(got["std"])
    # leaf indices out of range: refused before anything is written
    for pl, nl in (([0, 4], [0]), ([0, -1], [0]), ([0, 1], [4])):
        msg = _refused(api, api.boost_scores_cpp, [0.] * 4, pl, nl, [1., 2.], [3.])
        assert "leaf" in msg


# ---- weights -----------------------------------------------------------------------------------------------------------

def test_weights(api):
    rng = np.random.default_rng(9)
    ps, ns = rng.uniform(-8, 8, 500), rng.uniform(-8, 8, 400)                 # the range tests/test_train_host.py uses
    pw, nw = api.update_weights_cpp(ps, ns)
    wp, wn, r = boost_ref.update_weights(ps.tolist(), ns.tolist())
    assert same(pw, f64(wp)) and same(nw, f64(wn))
    # the control, on the restatement alone: reversed summation order changes the bits of r on this very input
    _, _, r_rev = boost_ref.update_weights(ps.tolist(), ns.tolist(), reverse=True)
    assert r != r_rev
    # one side empty, both empty
    pw, nw = api.update_weights_cpp(ps[:3], [])
    assert same(pw, f64(boost_ref.update_weights(ps[:3].tolist(), [])[0])) and nw.size == 0
    pw, nw = api.update_weights_cpp([], [])
    assert pw.size == 0 and nw.size == 0
    assert api.lib.jdaUpdateWeightsCpp(None, 2, None, 0, None, None) == -1 and api.last_error()


# ---- rows along --------------------------------------------------------------------------------------------------------

def test_gather_rows(api):
    rng = np.random.default_rng(2)
    a, b = rng.normal(size=(5, 10)), rng.normal(size=(3, 10))
    both = np.concatenate([a, b])
    idx = [4, 5, 0, 7, 4, 3]                                                  # both sides of the segment edge, a repeat
    assert same(api.gather_rows_cpp([a, b], idx), both[idx])
    assert same(api.gather_rows_cpp([a, b], idx, keep=2), both[idx[:2]])
    assert api.gather_rows_cpp([a, b], idx, keep=0).shape == (0, 10)
    assert same(api.gather_rows_cpp([a, np.zeros((0, 10)), b], idx), both[idx])          # an empty segment in between
    flags = rng.integers(0, 2, 8).astype(np.uint8)                            # one-byte rows
    assert same(api.gather_rows_cpp(flags, [7, 0, 3]), flags[[7, 0, 3]])
    for bad in (8, -1):
        msg = _refused(api, api.gather_rows_cpp, [a, b], [0, bad])
        assert "index[1]" in msg
    _refused(api, api.gather_rows_cpp, [a] * 9, [0])
    # dst inside a source: refused
    import ctypes as C
    ptrs = (C.c_void_p * 1)(a.ctypes.data)
    ns = (C.c_int * 1)(5)
    ix = np.array([1], np.int32)
    assert api.lib.jdaGatherRowsCpp(ptrs, ns, 1, 80, ix.ctypes.data_as(C.POINTER(C.c_int)), 1, a.ctypes.data + 160) == -1
    assert "overlaps" in api.last_error()
