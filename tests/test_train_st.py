"""The trainer pieces under the similarity transform (jdaSetSimilarityTransform(1) with the option "train_similarity",
include/jda.h): jdaCalcSTParametersCpp, the three cart-training entries, the two stage-close entries and jdaValidateSamplesCpp
against tests/st_ref.py, bit for bit -- every comparison is exact (`same`), there is no tolerance anywhere -- and one stage
pair trained end to end with the pieces, whose carried scores and shapes the model then reproduces.  Shapes are the mean
shape under each sample's own rotation and scale, so the transform matters: the share of feature values it changes is asserted
on the restatement (here and in tests/test_train_st_host.py).  Dialect CPP is parity-unpinned."""
import numpy as np
import pytest

from conftest import same
import model_ref
import st_ref
import stage_ref
import train_ref

pytestmark = pytest.mark.gpu

ODD = st_ref.ODD


@pytest.fixture(scope="module")
def gpu():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    return torch.device("cuda", 0)


def _mean(L, seed=None):
    from jda_amd import synth
    return synth.make_mean_shape(L, np.random.default_rng(L if seed is None else seed))


def _trainer(T, K, L, D, mean):
    """A cascador on an empty model in training with the transform on and the trainer opted in."""
    from jda_amd import api
    c = api.Cascador.create_training_cpp(T, K, L, D, mean, device=0)
    c.set_similarity_transform(True)
    c.set_option("train_similarity", 1)
    return c


def _split(row, sizes=ODD):
    o, h, q = sizes
    return row[:o * o].reshape(o, o), row[o * o:o * o + h * h].reshape(h, h), row[o * o + h * h:].reshape(q, q)


# ---- jdaCalcSTParametersCpp ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("L", [2, 5, 6, 33])
@pytest.mark.parametrize("n", [1, 70])
def test_st_parameters_equal_calc_run_twice(built, gpu, L, n):
    """2L mod 4 is 0 (L = 2, 6) and 2 (L = 5, 33): cv::norm's four-at-a-time loop with and without its tail; L = 33 has more
    coordinates than a wave has lanes.  One sample equals the mean shape: the sines are +0. in both directions."""
    mean = _mean(L)
    shapes = st_ref.make_shapes(L + n, n, mean)
    if n > 1:
        shapes[5] = mean
    c = _trainer(1, 1, L, 2, mean)
    c.set_option("train_similarity", 0)                   # (the entry needs no opt-in: it trains nothing)
    mc, cm = c.calc_st_parameters_cpp(shapes)
    want_mc, want_cm = st_ref.st_parameters(shapes, mean)
    assert same(mc, np.array(want_mc, np.float64).reshape(n, 5)) and same(cm, np.array(want_cm, np.float64).reshape(n, 5))
    assert n == 1 or np.abs(mc[:, 3]).max() > 0.2         # (rotations of up to 30 degrees: sines up to 0.5)
    c.set_similarity_transform(False)                     # the transform off: STParameter's default
    mc, cm = c.calc_st_parameters_cpp(shapes)
    assert same(mc, np.tile(np.array([1., 1., 0., 0., 1.]), (n, 1))) and same(cm, mc)
    c.close()


# ---- values, one node, one cart -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [3, 70])
def test_feature_values_under_each_samples_own_parameter(built, gpu, n):
    """F = 70 is two feature tiles of the values kernel, and for n = 3 more features than samples: the reading stp_mc[i] of
    data.cpp:168 would leave the array there; the reading built is stp_mc[idx[j]]."""
    L = 5
    mean = _mean(L)
    d = st_ref.make_samples(40 + L, n, mean)
    rows, _ = train_ref.gen_feature_pool(70, L, 0.45, True, 5, 9)
    assert {r[0] for r in rows} == {0, 1, 2}
    s, pool = train_ref.ref_set(d), train_ref.pool_of(rows)
    mc, _ = st_ref.st_parameters(d["shapes"], mean)
    want = np.array(st_ref.calc_feature_values(s, pool, list(range(n)), mc), np.int32)
    plain = np.array(train_ref.calc_feature_values(s, pool, list(range(n))), np.int32)
    assert (want != plain).mean() > 0.5                    # on the restatement alone: the test cannot pass vacuously
    c = _trainer(1, 2, L, 4, mean)
    assert same(c.calc_feature_values_cpp(d, stage_ref.pool_array(rows), *ODD), want)
    c.set_option("workspace_mb", 1)
    assert same(c.calc_feature_values_cpp(d, stage_ref.pool_array(rows), *ODD), want)
    c.set_similarity_transform(False)                     # with the transform off the option has no effect
    assert same(c.calc_feature_values_cpp(d, stage_ref.pool_array(rows), *ODD), plain)
    c.close()


def _sets(L, mean, pos_n=40, neg_n=30, seed=7):
    pd, nd = st_ref.make_samples(seed, pos_n, mean), st_ref.make_samples(seed + 100, neg_n, mean)
    pos, neg = train_ref.ref_set(pd), train_ref.ref_set(nd)
    return pd, nd, pos, neg, st_ref.st_parameters(pd["shapes"], mean)[0], st_ref.st_parameters(nd["shapes"], mean)[0]


@pytest.mark.parametrize("mode", [1, 0])
def test_split_node_in_both_modes(built, gpu, mode):
    L = 5
    mean = _mean(L)
    pd, nd, pos, neg, pmc, nmc = _sets(L, mean)
    rows, u = train_ref.gen_feature_pool(24, L, train_ref.RADIUS, True, 3, 1)
    fi, th, es, ths, _, _ = st_ref.split_node(pos, list(range(pos.n)), neg, list(range(neg.n)), train_ref.pool_of(rows), mode, u, pmc, nmc)
    plain = train_ref.split_node(pos, list(range(pos.n)), neg, list(range(neg.n)), train_ref.pool_of(rows), mode, u)
    assert es != plain[2]                                  # the transform is visible in the criteria
    c = _trainer(1, 2, L, 4, mean)
    got = c.split_node_cpp(pd, nd, stage_ref.pool_array(rows), mode, u, *ODD)
    assert same(got["criterion"], np.array(es, np.float64)) and same(got["thresholds"], np.array(ths, np.int32))
    assert (got["feature_idx"], got["threshold"]) == (fi, th)
    c.close()


def test_train_cart_and_its_leaves_are_forward(built, gpu):
    """D = 3 on 40 + 30 samples, a classification root and mixed children: the cart equals the restatement's, and
    pos_leaf / neg_leaf are what Cart::Forward returns for each sample under its own parameter -- the contract that
    training under stp_mc[idx[j]] exists for."""
    L, D, F = 5, 3, 16
    mean = _mean(L)
    pd, nd, pos, neg, pmc, nmc = _sets(L, mean)
    modes = [1, 0, 1]
    pools, us = [], []
    for i in range(3):
        r, u = train_ref.gen_feature_pool(F, L, train_ref.RADIUS, True, 9, i)
        pools.append(r); us.append(u)
    want = st_ref.train_cart(D, pos, neg, [train_ref.pool_of(p) for p in pools], modes, us, pmc, nmc)
    c = _trainer(1, 2, L, D, mean)
    got = c.train_cart_cpp(pd, nd, stage_ref.pool_array([f for p in pools for f in p]), modes, us, *ODD)
    assert [int(t) for t in got["thresholds"]] == want["thresholds"]
    rows = [pools[i][want["features"][i]] for i in range(3)]
    assert got["features"].tobytes() == stage_ref.pool_array(rows).tobytes() and same(got["scores"], np.array(want["scores"], np.float64))
    assert got["pos_leaf"].tolist() == want["pos_leaf"] and got["neg_leaf"].tolist() == want["neg_leaf"]
    fwd = [st_ref.forward(D, rows, want["thresholds"], pos.patches[i], pos.shapes[i], pmc[i]) for i in range(pos.n)]
    assert got["pos_leaf"].tolist() == fwd and len(set(fwd)) > 1
    fwd = [st_ref.forward(D, rows, want["thresholds"], neg.patches[i], neg.shapes[i], nmc[i]) for i in range(neg.n)]
    assert got["neg_leaf"].tolist() == fwd
    c.close()


# ---- closing a stage ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("L", [5, 33])
@pytest.mark.parametrize("K", [1, 64, 65, 130])
def test_stage_close(built, gpu, K, L):
    """Carts at and around the 64 lanes of a wave; 2L = 10 and 66 coordinates (one round and two of lane = coordinate, the
    partner of every coordinate in its own round); nine samples are three workgroups of four waves, the last one partly
    empty.  Walked and with lbf_in, from LDS (lbf_lds_kb 160) and from global memory (0)."""
    D, n = 3, 9
    mean = _mean(L)
    d = st_ref.make_samples(K + L, n, mean)
    rows, th = stage_ref.make_carts(K + 1, K, D, L, True, th_span=40)
    w = stage_ref.make_w(K, K, D, L)
    s = train_ref.ref_set(d)
    want_sh, want_lbf = st_ref.stage_update(D, stage_ref.carts_of(D, rows, th), s, w.tolist(), mean)
    plain_sh, plain_lbf = stage_ref.stage_update(D, stage_ref.carts_of(D, rows, th), s, w.tolist())
    want_sh, want_lbf = np.array(want_sh, np.float64), np.array(want_lbf, np.int32)
    assert not same(want_sh, np.array(plain_sh, np.float64)) and (K < 64 or not same(want_lbf, np.array(plain_lbf, np.int32)))
    c = _trainer(1, K, L, D, mean)
    feats = stage_ref.pool_array(rows)
    for kb in (160, 0):
        c.set_option("lbf_lds_kb", kb)
        assert same(c.gen_lbf_cpp(d, feats, th, *ODD), want_lbf), kb
        sh, lbf, st = c.stage_update_shapes_cpp(d, feats, th, w, None, *ODD, want_lbf=True, stats=True)
        assert same(sh, want_sh) and same(lbf, want_lbf) and st["lds_path"] == (1 if kb else 0), kb
        sh, st = c.stage_update_shapes_cpp(d, None, None, w, want_lbf, *ODD, stats=True)      # nothing is walked
        assert same(sh, want_sh) and st["lds_path"] == (1 if kb else 0), kb
    c.close()


# ---- re-validation --------------------------------------------------------------------------------------------------------------

def _reval_model(K, L, D, seed):
    from jda_amd import synth
    m = synth.make_model(2, K, L, D, seed=seed, cart_th=0.0, norm_every=7, multi_scale=True, w_sigma=2e-2, f32_exact=False)
    m.cth[:] = -np.inf
    return m


def _reference(blob, patches, starts):
    m2 = model_ref.model2_of(blob)
    res = [st_ref.validate_record(m2, *_split(patches[i]), starts[i]) for i in range(len(patches))]
    return dict(is_face=np.array([r[0] for r in res], np.uint8), score=np.array([r[1] for r in res], np.float64),
                shape=np.array([r[2] for r in res], np.float64).reshape(len(res), -1), carts_n=np.array([r[3] for r in res], np.int32))


@pytest.fixture(scope="module")
def reval_case():
    """K = 65, T = 2: thresholds that reject at cart 0, at carts 63 and 64 (the last lane of a round of 64 and the first of
    the next) and at cart 2 of stage 1 (inside the partial stage of the snapshot (1, 3)); each the score of a sample still
    alive there, so about an eighth of the survivors lie below it and `score == th` occurs and passes."""
    K, L, D, n = 65, 5, 3, 40
    m = _reval_model(K, L, D, seed=11)
    rng = np.random.default_rng(5)
    patches = rng.integers(0, 256, (n, sum(v * v for v in ODD)), dtype=np.uint8)
    starts = st_ref.make_shapes(17, n, m.mean_shape)
    cuts = [(0, 0), (0, 63), (0, 64), (1, 2)]
    for (t, k) in cuts:
        r = _reference(m.tobytes(8, t, k), patches, starts)
        alive = np.sort(r["score"][r["is_face"] == 1])
        below = np.searchsorted(alive, alive, side="left")
        m.cth[t, k] = alive[np.argmax(below >= max(1, len(alive) // 8))]
    return m, patches, starts, cuts


@pytest.mark.parametrize("hdr", [None, (0, 1), (1, -1), (1, 3)])
def test_revalidation_on_a_complete_model_and_on_snapshots(built, gpu, tmp_path, reval_case, hdr):
    from jda_amd import api
    m, patches, starts, cuts = reval_case
    K = m.K
    p = str(tmp_path / "m.model")
    with open(p, "wb") as f:
        f.write(m.tobytes(8) if hdr is None else m.tobytes(8, *hdr))
    blob = open(p, "rb").read()
    want = _reference(blob, patches, starts)
    plain = [model_ref.validate_record(model_ref.model2_of(blob), *_split(patches[i]), starts[i]) for i in range(len(patches))]
    # the transform is visible -- except at (0, 1), where only the partial stage 0 runs, with STParameter's default
    assert same(want["score"], np.array([r[1] for r in plain], np.float64)) == (hdr == (0, 1))
    rejected = want["is_face"] == 0
    ends = {t * K + k + 1 for (t, k) in cuts if hdr is None or (t, k) <= tuple(hdr)}
    assert set(want["carts_n"][rejected].tolist()) == ends and (~rejected).any()         # every position rejected somebody
    c = api.Cascador(p, "double", device=0)
    c.set_similarity_transform(True)
    c.set_option("train_similarity", 1)
    s = dict(patches=patches, shapes=starts)
    for form, kb in ((0, 160), (0, 0), (1, 160)):
        c.set_option("reval_form", form); c.set_option("reval_lds_kb", kb)
        got = c.validate_samples_cpp(s, *ODD)
        for k in ("is_face", "carts_n", "score", "shape"):
            assert same(got[k], want[k]), (form, kb, k)
        assert form == 1 or got["stats"]["lds_path"] == (1 if kb else 0)
    c.close()


def test_revalidation_with_two_rounds_of_coordinates(built, gpu, tmp_path):
    """L = 33: 66 coordinates, the regression's Apply pairs lanes in two rounds; K = 5, nothing rejects."""
    from jda_amd import api
    m = _reval_model(5, 33, 3, seed=4)
    patches = np.random.default_rng(6).integers(0, 256, (9, sum(v * v for v in ODD)), dtype=np.uint8)
    starts = st_ref.make_shapes(23, 9, m.mean_shape)
    p = str(tmp_path / "m.model")
    m.save(p, 8)
    want = _reference(open(p, "rb").read(), patches, starts)
    c = api.Cascador(p, "double", device=0)
    c.set_similarity_transform(True)
    c.set_option("train_similarity", 1)
    for form, kb in ((0, 160), (0, 0), (1, 160)):
        c.set_option("reval_form", form); c.set_option("reval_lds_kb", kb)
        got = c.validate_samples_cpp(dict(patches=patches, shapes=starts), *ODD)
        for k in ("is_face", "carts_n", "score", "shape"):
            assert same(got[k], want[k]), (form, kb, k)
    c.close()


# ---- end to end -------------------------------------------------------------------------------------------------------------------

def test_two_stages_trained_with_the_pieces_are_the_model_validate_runs(built, gpu):
    """T = 2, K = 2, D = 3: each stage is trained with the pieces under the transform -- carts (scores carried from cart to
    cart), put, indicators, the residual through jdaShapeResidualStCpp, the fit, the shape update, close.  Every sample starts
    from the mean shape, so stage 0's parameters are the identity's and stage 1's are not (asserted).  jdaValidateSamplesCpp
    on the start shapes must then return the carried scores and shapes, and jdaValidateCpp on the same patches (each o patch
    an image of its own, the crop the whole image, shift_size 0, resize_mode 1) must agree with it."""
    from jda_amd import api
    T, K, L, D, F = 2, 2, 5, 3, 12
    mean = _mean(L)
    c = _trainer(T, K, L, D, mean)
    rng = np.random.default_rng(31)
    n_pos, n_neg = 40, 30
    n = n_pos + n_neg
    o = rng.integers(0, 256, (n, ODD[0], ODD[0]), dtype=np.uint8)
    patches = np.stack([np.concatenate([o[i].reshape(-1), c.resize_cv(o[i], ODD[1], ODD[1]).reshape(-1),
                                        c.resize_cv(o[i], ODD[2], ODD[2]).reshape(-1)]) for i in range(n)])
    start = api.random_shapes_cpp(mean, n)                 # mean_shape + 0.: Validate's own start
    gt = st_ref.make_shapes(3, n_pos, mean)
    shapes, scores = start.copy(), np.zeros(n)
    for t in range(T):
        mc, cm = c.calc_st_parameters_cpp(shapes)
        assert (np.abs(mc[:, 3]).max() > 0.) == (t == 1)
        weights = np.exp(-scores * np.r_[np.ones(n_pos), -np.ones(n_neg)])
        feats, ths = [], []
        for k in range(K):
            pos = dict(patches=patches[:n_pos], shapes=shapes[:n_pos], weights=weights[:n_pos],
                       residual=api.shape_residual_cpp(gt, shapes[:n_pos], landmark_id=k, stp_cm=cm[:n_pos]))
            neg = dict(patches=patches[n_pos:], shapes=shapes[n_pos:], weights=weights[n_pos:])
            pools, us = zip(*[api.gen_feature_pool_cpp(F, L, 0.3, True, 10 * t + k, i) for i in range(3)])
            cart = c.train_cart_cpp(pos, neg, np.concatenate(pools), [1, 0, 1], np.concatenate(us), *ODD)
            c.put_cart_cpp(k, cart["features"], cart["thresholds"], cart["scores"], -1e300)
            scores = scores + cart["scores"][np.r_[cart["pos_leaf"], cart["neg_leaf"]]]       # DataSet::UpdateScores; (score - 0.) / 1. changes nothing
            feats.append(cart["features"]); ths.append(cart["thresholds"])
        every = dict(patches=patches, shapes=shapes)
        feats, ths = np.concatenate(feats), np.concatenate(ths)
        lbf = c.gen_lbf_cpp(every, feats, ths, *ODD)
        residual = api.shape_residual_cpp(gt, shapes[:n_pos], stp_cm=cm[:n_pos])
        w = c.global_regression_cpp(lbf[:n_pos], residual, max_iter=30)[0]
        assert np.abs(w).max() > 0
        shapes = c.stage_update_shapes_cpp(every, None, None, w, lbf, *ODD)
        c.close_stage_cpp(w)
    assert c.model_status_cpp() == (T, -1)
    got = c.validate_samples_cpp(dict(patches=patches, shapes=start), *ODD)
    assert got["is_face"].all() and (got["carts_n"] == T * K).all()
    assert same(got["score"], scores) and same(got["shape"], shapes)
    crops = [(i, 0, 0, ODD[0], ODD[0]) for i in range(n)]
    val = c.validate_cpp([o[i] for i in range(n)], crops, 1, *ODD, shift_size=0.0)
    for k in ("is_face", "carts_n", "score", "shape"):
        assert same(val[k], got[k]), k
    c.close()
