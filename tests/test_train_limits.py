"""The trainer kernels of jda_amd/csrc/k_train.hip (k_train_transpose, k_train_values<ST>, k_train_hist, k_train_var) at their
limits, on their RAW outputs: jdaSplitNodeSumsCpp returns what the device wrote for one node -- the 16-bit values per list
position, the weighted and the count histograms, TrainVar's eight sums, counts and order statistic -- and every one of them is
compared with tests/train_ref.py's intermediates bit for bit (`same` / np.array_equal; there is no tolerance anywhere), next
to the criteria, thresholds and choice that jdaSplitNodeCpp returns.  The one relaxation: where the restatement's criterion is
a NaN (a node without any sample: 0 / 0) the device's must be a NaN too, of whatever sign and payload.
tests/test_train_limits_host.py proves on the restatement alone that the crafted inputs have the properties claimed for
them.  Each case stays below about 60,000 feature evaluations on the restatement.  Dialect CPP is parity-unpinned: bit-exact
against this repo's restatement of the reference's source, not against the reference (src/jda needs OpenCV)."""
import numpy as np
import pytest

from conftest import same
import st_ref
import train_ref
import test_train_limits_host as host

pytestmark = pytest.mark.gpu

SIZES, SMALL = (48, 36, 24), (31, 17, 9)
COUNTS = [0, 1, 7, 8, 9, 63, 64, 65, 128, 129, 255, 256, 257]
EVAL_CAP = 60000

# mode 1: pos_n, neg_n, F, L, multi_scale, patch sizes
CLS_FACTORS = [COUNTS, COUNTS, [1, 3, 4, 5, 63, 64, 65, 129], [1, 5, 27], [False, True], [SIZES, SMALL]]
# mode 0: pos_n, F, has_gt (null / partly set / all zero), u (the pool's, all 0.0, all nextafter(1, 0))
REG_FACTORS = [COUNTS, [1, 63, 64, 65, 128, 129], ["null", "partly", "zero"], list(host.U_KINDS)]


def cls_allowed(row):
    return (row.get(0, 0) + row.get(1, 0)) * row.get(2, 1) <= EVAL_CAP


def reg_allowed(row):
    return row.get(0, 0) * row.get(1, 1) <= EVAL_CAP


CLS_ROWS = train_ref.pairwise_cover(CLS_FACTORS, cls_allowed)
REG_ROWS = train_ref.pairwise_cover(REG_FACTORS, reg_allowed)


@pytest.fixture(scope="module")
def gpu():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def cascadors(built, gpu, tmp_path_factory):
    """One cascador per landmark count (the patch sizes are call arguments, the scales the pool's)."""
    from jda_amd import api, synth
    made = {}

    def get(L, D=4):
        if (L, D) not in made:
            p = str(tmp_path_factory.mktemp("limits") / ("m_%d_%d.model" % (L, D)))
            synth.make_model(1, 2, L, D).save(p, 8)
            made[(L, D)] = api.Cascador(p, "double", device=0)
        return made[(L, D)]
    yield get
    for c in made.values():
        c.close()


def _pool(rows):
    from jda_amd import api
    a = np.zeros(len(rows), api.FEATURE_DTYPE)
    for i, r in enumerate(rows):
        a[i] = (r[0], r[1], r[2], 0, r[3], r[4], r[5], r[6])
    return a


def _same_criteria(got, want):
    want = np.array(want, np.float64)
    nan = np.isnan(want)
    return got.shape == want.shape and np.array_equal(np.isnan(got), nan) and same(got[~nan], want[~nan])


def _reference(pd, nd, rows, mode, u, pl=None, nl=None, values=None):
    """The restatement on the lists pl / nl (None: everybody) -> (choice, criteria, thresholds, pf, nf, intermediates);
    values: (pos, neg) value functions of (set, pool, list) other than train_ref.calc_feature_values'."""
    pos, neg, pool = train_ref.ref_set(pd), train_ref.ref_set(nd), train_ref.pool_of(rows)
    pidx = list(range(pos.n)) if pl is None else [int(v) for v in pl]
    nidx = list(range(neg.n)) if nl is None else [int(v) for v in nl]
    pf = (values[0] if values else train_ref.calc_feature_values)(pos, pool, pidx)
    nf = (values[1] if values else train_ref.calc_feature_values)(neg, pool, nidx)
    det = {}
    if mode == 1:
        fi, th, es, ths = train_ref.split_classification(pos, pidx, neg, nidx, pf, nf, detail=det)
    else:
        fi, th, es, ths = train_ref.split_regression(pos, pidx, pf, u, detail=det)
    return (fi, th), es, ths, pf, nf, det


def _compare(got, ref, F, mode):
    """Every raw output of the device and what jdaSplitNodeCpp returns against the restatement."""
    (fi, th), es, ths, pf, nf, det = ref
    P, N = len(pf[0]), len(nf[0])
    assert same(got["pos_values"], np.array(pf, np.int16).reshape(F, P))
    if mode == 1:
        assert same(got["neg_values"], np.array(nf, np.int16).reshape(F, N))
        assert same(got["pos_hist_c"], np.array(det["p_n"], np.int32)) and same(got["neg_hist_c"], np.array(det["n_n"], np.int32))
        assert same(got["pos_hist_w"], np.array(det["wp"], np.float64)), "positives' weighted histogram"
        assert same(got["neg_hist_w"], np.array(det["wn"], np.float64)), "negatives' weighted histogram"
    elif P == 0:                                               # cart.cpp:299-301: nothing is launched, nothing written
        for k in ("pos_hist_c", "var_sums", "var_n_left", "var_n_right", "var_th"):
            assert not got[k].any(), k
        assert got["chunks"] == 0
    else:
        assert same(got["pos_hist_c"], np.array(det["counts"], np.int32))
        assert same(got["var_th"], np.array(det["th"], np.int32))
        assert same(got["var_n_left"], np.array(det["n_left"], np.int32)) and same(got["var_n_right"], np.array(det["n_right"], np.int32))
        assert same(got["var_sums"], np.array(det["sums"], np.float64)), "TrainVar's eight sums"
    assert _same_criteria(got["criterion"], es)
    assert same(got["thresholds"], np.array(ths, np.int32))
    assert (got["feature_idx"], got["threshold"]) == (fi, th)


def _same_outputs(a, b):
    for k in a:
        if k != "chunks":
            x, y = np.asarray(a[k]), np.asarray(b[k])
            assert (_same_criteria(x, y) if k == "criterion" else same(x, y)), k


def _run(c, pd, nd, rows, mode, u=None, pl=None, nl=None, sizes=SIZES, values=None):
    ref = _reference(pd, nd, rows, mode, u, pl, nl, values)
    got = c.split_node_sums_cpp(pd, nd, _pool(rows), mode, u, pl, nl, *sizes)
    _compare(got, ref, len(rows), mode)
    return got, ref


# ---- 1, 2: the shape sweeps ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("i", range(len(CLS_ROWS)), ids=lambda i: "-".join(str(v).replace(" ", "") for v in CLS_ROWS[i]))
def test_classification_shape_sweep(cascadors, i):
    """The counts around a batch of 64 list entries, 256 lanes of the values kernel and the rows' padding to 8; F around the
    4 waves of k_train_hist's workgroup and the 64-feature tiles; an empty side follows from the same IEEE expressions."""
    pos_n, neg_n, F, L, multi, sizes = CLS_ROWS[i]
    pd, nd = train_ref.make_samples(1000 + i, pos_n, L, sizes), train_ref.make_samples(2000 + i, neg_n, L, sizes)
    rows, _ = train_ref.gen_feature_pool(F, L, train_ref.RADIUS, multi, 1000 + i, 1)
    _run(cascadors(L), pd, nd, rows, 1, sizes=sizes)


@pytest.mark.parametrize("i", range(len(REG_ROWS)), ids=lambda i: "-".join(str(v) for v in REG_ROWS[i]))
def test_regression_shape_sweep(cascadors, i):
    """k_train_var's 64 x 64 tiles with rows = min(64, F - f0) and cols = min(64, count - j0) at and around 64; kidx 0 and
    pos_n - 1; has_gt null, partly set and all zero (n_left = n_right = 0: variance_of's empty side)."""
    pos_n, F, gt, kind = REG_ROWS[i]
    L = 5
    pd, nd = train_ref.make_samples(3000 + i, pos_n, L, gt_drop=0.35), train_ref.make_samples(4000 + i, 9, L)
    pd["has_gt"] = None if gt == "null" else (pd["has_gt"] if gt == "partly" else np.zeros(pos_n, np.uint8))
    rows, u = train_ref.gen_feature_pool(F, L, train_ref.RADIUS, True, 3000 + i, 1)
    got, _ = _run(cascadors(L), pd, nd, rows, 0, host.u_of(kind, u))
    if gt == "zero":
        assert not got["var_n_left"].any() and not got["var_n_right"].any() and not got["criterion"].any()
    if pos_n and kind == "top":
        assert not got["var_n_right"].any()


# ---- 3: collisions ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", host.FEW_CASES, ids=lambda c: "%d-%d" % (c[1], c[2]))
def test_few_valued_set_deep_ranks(cascadors, case):
    """Ranks of 16 and more in every batch, gates that open, an order that is visible (all proved in the host file): the
    weighted histograms are the ordered sums.  Mode 0 on the same positives: ties at the threshold."""
    seed, pos_n, neg_n, L, multi, F = case
    pd, nd, rows, u, pos, neg, pf, nf = host.node("few", *case)
    (plo, phi), (nlo, nhi) = train_ref.deepest_rank(pf, pos_n), train_ref.deepest_rank(nf, neg_n)
    assert min(plo, nlo) >= 16
    print("deepest rank reached (from the restatement's values): %d" % (max(phi, nhi) - 1))
    c = cascadors(L)
    got, _ = _run(c, pd, nd, rows, 1)
    assert (got["thresholds"] != -256).sum() > F // 2
    _run(c, pd, nd, rows, 0, u)


def test_flat_set_one_bin_ranks_to_63(cascadors):
    """The one_value corner: every batch falls into bin 255, one add per round for 64 rounds in lane order.  No gate opens,
    so only the histogram itself can show a wrong order -- the host file shows that the reversed order changes its bits."""
    pd, nd = train_ref.make_samples(31, 260, 5, flat=True), train_ref.make_samples(131, 230, 5, flat=True)
    rows, _ = train_ref.gen_feature_pool(24, 5, train_ref.RADIUS, True, 31, 1)
    got, _ = _run(cascadors(5), pd, nd, rows, 1)
    assert (got["pos_hist_c"][:, 255] == 260).all() and (got["neg_hist_c"][:, 255] == 230).all() and got["threshold"] == -256


# ---- 4: extremes -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", host.EXTREME_CASES, ids=lambda c: "%d-%d" % (c[1], c[2]))
def test_extreme_values_reach_bins_0_and_510(cascadors, case):
    seed, pos_n, neg_n, L, multi, F = case
    pd, nd, rows, u, *_ = host.node("extreme", *case)
    c = cascadors(L)
    got, _ = _run(c, pd, nd, rows, 1)
    assert got["pos_hist_c"][:, 0].any() and got["pos_hist_c"][:, 510].any()
    got, _ = _run(c, pd, nd, rows, 0, u)
    assert -255 in got["var_th"] and 255 in got["var_th"]     # the threshold search ends on the first and on the last bin


# ---- 5: sublists -----------------------------------------------------------------------------------------------------------

def _cut(d, idx):
    idx = np.asarray(idx, np.int64)
    return {k: (v if k == "sizes" or v is None else v[idx]) for k, v in d.items()}


@pytest.fixture(scope="module")
def pair():
    pd, nd = train_ref.make_samples(91, 300, 5, gt_drop=0.3), train_ref.make_samples(191, 280, 5)
    return (pd, nd) + train_ref.gen_feature_pool(40, 5, train_ref.RADIUS, True, 91, 1)


@pytest.mark.parametrize("which", ["every_second", "first_65", "last_63", "single"])
@pytest.mark.parametrize("mode", [1, 0])
def test_sublists(cascadors, pair, which, mode):
    """The values kernel indexes list[j], writes by position, and the weights, residuals and has_gt are read at list[j]: the
    result on a list equals the restatement's on that list AND the device's own on a set physically cut down to it."""
    pd, nd, rows, u = pair
    cut = dict(every_second=lambda n: list(range(0, n, 2)), first_65=lambda n: list(range(65)),
               last_63=lambda n: list(range(n - 63, n)), single=lambda n: [n - 7])[which]
    pl, nl = cut(300), cut(280)
    c = cascadors(5)
    got, _ = _run(c, pd, nd, rows, mode, u if mode == 0 else None, pl, nl)
    small = c.split_node_sums_cpp(_cut(pd, pl), _cut(nd, nl), _pool(rows), mode, u if mode == 0 else None)
    _same_outputs(got, small)


def test_bad_lists_are_refused(cascadors, pair):
    from jda_amd import api
    pd, nd, rows, u = pair
    c = cascadors(5)
    for pl, nl in (([0, 2, 2], None), ([3, 1], None), ([0, 300], None), ([-1], None), (None, [5, 4]), (None, [280])):
        with pytest.raises(api.JdaError, match="strictly ascending"):
            c.split_node_sums_cpp(pd, nd, _pool(rows[:3]), 1, None, pl, nl)


# ---- 6: chunks -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("mode", [1, 0])
def test_feature_chunks(built, gpu, model_file, mode):
    """workspace_mb = 1 with F = 129 on 230 + 200 samples: chunks of 35 features (neither a multiple of the 4 waves of a
    k_train_hist workgroup nor of k_train_var's 64-feature tile), so chunk boundaries fall inside both; mode 0 reads
    d_kidx + f0.  Identical to the one-chunk call in every raw output."""
    from jda_amd import api
    p, _ = model_file((1, 2, 5, 4))
    c = api.Cascador(p, "double", device=0)
    pd, nd = train_ref.make_samples(95, 230, 5, gt_drop=0.2), train_ref.make_samples(195, 200, 5)
    rows, u = train_ref.gen_feature_pool(129, 5, train_ref.RADIUS, True, 95, 1)
    u = u if mode == 0 else None
    one, _ = _run(c, pd, nd, rows, mode, u)
    assert one["chunks"] == 1
    c.set_option("workspace_mb", 1)
    many = c.split_node_sums_cpp(pd, nd, _pool(rows), mode, u)
    assert many["chunks"] >= 3
    _same_outputs(one, many)
    c.close()


# ---- 7: the per-sample transform -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("pos_n,neg_n,F", [(1, 257, 65), (64, 1, 1), (65, 64, 65), (257, 65, 1)])
def test_values_under_the_similarity_transform(built, gpu, pos_n, neg_n, F):
    """k_train_values<true> as tests/test_train_st.py sets it up (the sample's own stp_mc, odd patch sizes) at the counts
    around a wave and a workgroup and one and two feature tiles."""
    from jda_amd import api, synth
    L = 5
    mean = synth.make_mean_shape(L, np.random.default_rng(L))
    c = api.Cascador.create_training_cpp(1, 2, L, 4, mean, device=0)
    c.set_similarity_transform(True)
    c.set_option("train_similarity", 1)
    pd, nd = st_ref.make_samples(300 + pos_n, pos_n, mean), st_ref.make_samples(400 + neg_n, neg_n, mean)
    rows, _ = train_ref.gen_feature_pool(F, L, train_ref.RADIUS, True, 7, 1)
    pmc, nmc = st_ref.st_parameters(pd["shapes"], mean)[0], st_ref.st_parameters(nd["shapes"], mean)[0]
    values = (lambda s, pool, idx: st_ref.calc_feature_values(s, pool, idx, pmc),
              lambda s, pool, idx: st_ref.calc_feature_values(s, pool, idx, nmc))
    _, ref = _run(c, pd, nd, rows, 1, sizes=st_ref.ODD, values=values)
    plain = train_ref.calc_feature_values(train_ref.ref_set(nd if neg_n > pos_n else pd), train_ref.pool_of(rows),
                                          list(range(max(pos_n, neg_n))))
    assert F * max(pos_n, neg_n) < 100 or plain != (ref[4] if neg_n > pos_n else ref[3])      # the transform is visible
    c.close()


# ---- 8: resident patches ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("mode", [1, 0])
def test_patches_resident_on_the_device(cascadors, gpu, mode):
    import torch
    pd, nd = train_ref.make_samples(97, 129, 27, gt_drop=0.2), train_ref.make_samples(197, 65, 27)
    rows, u = train_ref.gen_feature_pool(65, 27, train_ref.RADIUS, True, 97, 1)
    _run(cascadors(27), dict(pd, patches=torch.from_numpy(pd["patches"]).cuda()),
         dict(nd, patches=torch.from_numpy(nd["patches"]).cuda()), rows, mode, u if mode == 0 else None)


# ---- 9: the whole cart on small lists --------------------------------------------------------------------------------------

def test_cart_on_small_lists(cascadors):
    """D = 5 on 40 + 36 samples: the deep nodes get lists of 0 to 5 samples, feature_row (F = 1, its own stride) runs with
    counts below 8.  Compared as tests/test_train.py's _check_cart compares, field for field."""
    D, L, F = 5, 5, 16
    inner = (1 << (D - 1)) - 1
    pd, nd = train_ref.make_samples(55, 40, L, gt_drop=0.2), train_ref.make_samples(155, 36, L)
    pools, us = zip(*[train_ref.gen_feature_pool(F, L, train_ref.RADIUS, True, 55, node) for node in range(1, inner + 1)])
    modes = [1] + [int(v) for v in (np.random.default_rng(55).random(inner - 1) < 0.6)]
    pos, neg = train_ref.ref_set(pd), train_ref.ref_set(nd)
    want = train_ref.train_cart(D, pos, neg, [train_ref.pool_of(p) for p in pools], modes, us)
    sizes = sorted(n[0] + n[1] for n in want["nodes"][inner // 2:])
    assert sizes[0] <= 5 and any(0 < n[0] < 8 or 0 < n[1] < 8 for n in want["nodes"])       # (on the restatement)
    got = cascadors(L, D).train_cart_cpp(pd, nd, _pool([r for p in pools for r in p]), modes, np.array(us))
    assert np.array_equal(got["nodes"]["feature_idx"], np.array(want["features"], np.int32))
    assert np.array_equal(got["thresholds"], np.array(want["thresholds"], np.int32))
    assert same(got["scores"], np.array(want["scores"]))
    assert np.array_equal(got["pos_leaf"], np.array(want["pos_leaf"], np.int32))
    assert np.array_equal(got["neg_leaf"], np.array(want["neg_leaf"], np.int32))
    for i in range(inner):
        n = got["nodes"][i]
        assert (int(n["pos_n"]), int(n["neg_n"]), int(n["feature_idx"])) == want["nodes"][i][:3], i
        assert _same_criteria(np.array([n["criterion"]]), [want["nodes"][i][3]]), i
        assert int(n["mode"]) == modes[i] and int(n["threshold"]) == want["thresholds"][i]
