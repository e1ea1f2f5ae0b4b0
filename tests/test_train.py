"""Training one CART on the device (jdaCalcFeatureValuesCpp, jdaSplitNodeCpp, jdaTrainCartCpp) against the sequential
restatement tests/train_ref.py, bit for bit: every comparison is exact (`same`), there is no tolerance anywhere.
tests/test_train_host.py holds the control that the summation order these tests pin is visible in the bits.  Dialect CPP
is parity-unpinned: bit-exact against this repo's restatement of the reference's source, not against the reference."""
import numpy as np
import pytest

from conftest import same
import train_ref

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    return torch.device("cuda", 0)


def _cascador(model_file, L, D=4):
    from jda_amd import api
    p, _ = model_file((1, 2, L, D))
    return api.Cascador(p, "double", device=0)


def _pool(rows):
    from jda_amd import api
    a = np.zeros(len(rows), api.FEATURE_DTYPE)
    for i, r in enumerate(rows):
        a[i] = (r[0], r[1], r[2], 0, r[3], r[4], r[5], r[6])
    return a


def _rows(feats):
    return [(int(f["scale"]), int(f["landmark_id1"]), int(f["landmark_id2"]), float(f["offset1_x"]), float(f["offset1_y"]),
             float(f["offset2_x"]), float(f["offset2_y"])) for f in feats]


# ---- feature values ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("L,multi,sizes", [(5, False, (48, 36, 24)), (27, True, (48, 36, 24)), (5, True, (31, 17, 9))])
def test_feature_values_equal_the_restatement(built, gpu, model_file, L, multi, sizes):
    import torch
    c = _cascador(model_file, L)
    d = train_ref.make_samples(21 + L, 300, L, sizes, outside=0.3)
    rows, _ = train_ref.gen_feature_pool(70, L, 0.45, multi, 5, 9)
    want = np.array(train_ref.calc_feature_values(train_ref.ref_set(d), train_ref.pool_of(rows), list(range(300))), np.int32)
    got = c.calc_feature_values_cpp(d, _pool(rows), *sizes)
    assert same(got, want)
    assert (want == 0).mean() < 0.5 and np.abs(want).max() > 200          # (a real test: values spread over the range)
    # shapes pushed outside the patch were clamped, not skipped: some sample reads the patch's border
    dev = c.calc_feature_values_cpp(dict(d, patches=torch.from_numpy(d["patches"]).cuda()), _pool(rows), *sizes)
    assert same(dev, got)
    # chunking over features: a workspace so small that the pool is cut into several chunks
    c.set_option("workspace_mb", 1)
    assert same(c.calc_feature_values_cpp(d, _pool(rows), *sizes), want)
    c.close()


# ---- one node ----------------------------------------------------------------------------------------------------------

def _node_case(seed, pos_n, neg_n, L, multi, F, **kw):
    pd, nd = train_ref.make_samples(seed, pos_n, L, **kw), train_ref.make_samples(seed + 100, neg_n, L, **kw)
    rows, u = train_ref.gen_feature_pool(F, L, train_ref.RADIUS, multi, seed, 1)
    return pd, nd, rows, u


def _check_node(c, pd, nd, rows, mode, u):
    pos, neg = train_ref.ref_set(pd), train_ref.ref_set(nd)
    fi, th, es, ths, _, _ = train_ref.split_node(pos, list(range(pos.n)), neg, list(range(neg.n)), train_ref.pool_of(rows), mode, u)
    got = c.split_node_cpp(pd, nd, _pool(rows), mode, u)
    print("mode %d: chosen %d / %d, threshold %d / %d, criterion %r / %r" % (mode, got["feature_idx"], fi, got["threshold"], th,
                                                                            got["criterion"][got["feature_idx"]], es[fi]))
    assert same(got["criterion"], np.array(es, np.float64))
    assert same(got["thresholds"], np.array(ths, np.int32))
    assert (got["feature_idx"], got["threshold"]) == (fi, th)
    return got


@pytest.mark.parametrize("case", train_ref.CLS_CASES)
def test_classification_split_equals_the_restatement(built, gpu, model_file, case):
    seed, pos_n, neg_n, L, multi, F = case
    c = _cascador(model_file, L)
    pd, nd, rows, _ = _node_case(*case)
    got = _check_node(c, pd, nd, rows, 1, None)
    assert got["threshold"] != -256 and (got["thresholds"] != -256).sum() > F // 2
    # several feature chunks give the same node
    c.set_option("workspace_mb", 1)
    again = c.split_node_cpp(pd, nd, _pool(rows), 1)
    for k in got:
        assert same(np.asarray(got[k]), np.asarray(again[k])), k
    c.close()


@pytest.mark.parametrize("what", ["no_negatives", "no_positives", "equal_weights", "one_value"])
def test_classification_split_corner_cases(built, gpu, model_file, what):
    c = _cascador(model_file, 5)
    kw = dict(equal_weights=True) if what == "equal_weights" else (dict(flat=True) if what == "one_value" else {})
    pd, nd, rows, _ = _node_case(31, 0 if what == "no_positives" else 260, 0 if what == "no_negatives" else 230, 5, True, 24, **kw)
    got = _check_node(c, pd, nd, rows, 1, None)
    if what in ("no_negatives", "no_positives", "one_value"):
        assert got["threshold"] == -256 and (got["thresholds"] == -256).all()      # no gate ever opens
    if what == "one_value":
        # no gate opens, so the criterion never reads the histograms: compare them themselves (jdaSplitNodeSumsCpp) -- one bin,
        # 64 rounds of k_train_hist's rank loop per batch, whose order tests/test_train_limits_host.py shows in the bits
        pos, neg, det = train_ref.ref_set(pd), train_ref.ref_set(nd), {}
        train_ref.split_node(pos, list(range(pos.n)), neg, list(range(neg.n)), train_ref.pool_of(rows), 1, None, detail=det)
        sums = c.split_node_sums_cpp(pd, nd, _pool(rows), 1)
        assert same(sums["pos_hist_w"], np.array(det["wp"], np.float64)) and same(sums["neg_hist_w"], np.array(det["wn"], np.float64))
        assert same(sums["pos_hist_c"], np.array(det["p_n"], np.int32)) and same(sums["neg_hist_c"], np.array(det["n_n"], np.int32))
        assert sums["pos_hist_c"][:, 255].tolist() == [260] * 24 and same(sums["criterion"], got["criterion"])
    c.close()


@pytest.mark.parametrize("what", ["plain", "gt_partly", "no_positives", "u_low", "u_high"])
def test_regression_split_equals_the_restatement(built, gpu, model_file, what):
    c = _cascador(model_file, 27)
    pd, nd, rows, u = _node_case(41, 0 if what == "no_positives" else 520, 300, 27, True, 80,
                                 gt_drop=0.35 if what == "gt_partly" else 0.0)
    if what == "u_low":
        u = [0.1] * len(u)
    if what == "u_high":
        u = [float(np.nextafter(0.9, 0.))] * len(u)
    if what != "gt_partly":
        pd["has_gt"] = None
    got = _check_node(c, pd, nd, rows, 0, u)
    if what == "no_positives":
        assert (got["feature_idx"], got["threshold"]) == (0, -256)
    else:
        assert len(set(got["thresholds"].tolist())) > 10
    c.set_option("workspace_mb", 1)
    again = c.split_node_cpp(pd, nd, _pool(rows), 0, u)
    for k in got:
        assert same(np.asarray(got[k]), np.asarray(again[k])), k
    c.close()


# ---- the whole cart ----------------------------------------------------------------------------------------------------

def _cart_case(seed, D, L, multi, F, pos_n, neg_n, modes=None):
    inner = (1 << (D - 1)) - 1
    pd = train_ref.make_samples(seed, pos_n, L, gt_drop=0.2)
    nd = train_ref.make_samples(seed + 100, neg_n, L)
    pools, us = [], []
    for node in range(1, inner + 1):
        rows, u = train_ref.gen_feature_pool(F, L, train_ref.RADIUS, multi, seed, node)
        pools.append(rows); us.append(u)
    rng = np.random.default_rng(seed)
    if modes is None:
        modes = [int(v) for v in (rng.random(inner) < 0.6)]
        modes[0] = 1
    return pd, nd, pools, us, modes


def _check_cart(c, D, pd, nd, pools, us, modes):
    pos, neg = train_ref.ref_set(pd), train_ref.ref_set(nd)
    want = train_ref.train_cart(D, pos, neg, [train_ref.pool_of(p) for p in pools], modes, us)
    flat = _pool([r for p in pools for r in p])
    got = c.train_cart_cpp(pd, nd, flat, modes, np.array(us))
    inner = len(pools)
    assert np.array_equal(got["nodes"]["feature_idx"], np.array(want["features"], np.int32))
    assert np.array_equal(got["thresholds"], np.array(want["thresholds"], np.int32))
    assert _rows(got["features"]) == [pools[i][want["features"][i]] for i in range(inner)]
    assert same(got["scores"], np.array(want["scores"]))
    assert np.array_equal(got["pos_leaf"], np.array(want["pos_leaf"], np.int32))
    assert np.array_equal(got["neg_leaf"], np.array(want["neg_leaf"], np.int32))
    for i in range(inner):
        n = got["nodes"][i]
        assert (int(n["pos_n"]), int(n["neg_n"]), int(n["feature_idx"])) == want["nodes"][i][:3], i
        assert same(np.float64(n["criterion"]), np.float64(want["nodes"][i][3])), i
        assert int(n["mode"]) == modes[i] and int(n["threshold"]) == want["thresholds"][i]
    assert got["stats"]["call_ms"] > 0 and got["stats"]["feature_evals"] > 0
    return got, want, neg


@pytest.mark.parametrize("D,L,multi,F,pos_n,neg_n", [(3, 5, False, 40, 420, 380), (4, 27, True, 40, 520, 480),
                                                    (6, 5, True, 40, 700, 640)])
def test_cart_equals_the_restatement(built, gpu, model_file, D, L, multi, F, pos_n, neg_n):
    c = _cascador(model_file, L, D)
    pd, nd, pools, us, modes = _cart_case(50 + D, D, L, multi, F, pos_n, neg_n)
    got, want, neg = _check_cart(c, D, pd, nd, pools, us, modes)
    assert len(set(got["neg_leaf"].tolist())) > 2 and len(set(got["pos_leaf"].tolist())) > 2      # a real tree
    # the leaf of every negative is the leaf the existing dialect-CPP walk (oracle.cpp_reading2.forward, what Validate
    # runs) reaches when the TRAINED cart is evaluated on the same patches: UpdateScores for free
    rows = _rows(got["features"])
    for s in range(neg.n):
        assert train_ref.forward(D, rows, got["thresholds"], neg.patches[s], neg.shapes[s]) == got["neg_leaf"][s], s
    # several feature chunks, and the patches resident on the device: the same cart
    import torch
    c.set_option("workspace_mb", 1)
    flat = _pool([r for p in pools for r in p])
    again = c.train_cart_cpp(dict(pd, patches=torch.from_numpy(pd["patches"]).cuda()),
                             dict(nd, patches=torch.from_numpy(nd["patches"]).cuda()), flat, modes, np.array(us))
    assert again["stats"]["feature_chunks"] > got["stats"]["feature_chunks"]
    for k in ("features", "thresholds", "scores", "pos_leaf", "neg_leaf", "nodes"):
        assert got[k].tobytes() == again[k].tobytes(), k
    c.close()


def test_cart_larger_case(built, gpu, model_file):
    """The large pool: F = 512 over 4,000 samples, two levels (the restatement takes 17 s for it on the CPU; at 20 k samples
    it would take minutes, so the pool keeps its size and the sample count gives)."""
    D, L, F = 3, 5, 512
    c = _cascador(model_file, L, D)
    pd, nd, pools, us, modes = _cart_case(77, D, L, True, F, 2200, 1800, modes=[1, 1, 1])
    _check_cart(c, D, pd, nd, pools, us, modes)
    c.close()


def test_cart_on_mined_negatives(built, gpu, tmp_path):
    """End to end: negatives come from mine_negatives_cpp(device=True) and go into train_cart_cpp as they are."""
    from jda_amd import api, synth
    mdl = synth.make_model(3, 20, 5, 4, seed=3, cart_th=-2.0, norm_every=5, multi_scale=True)
    p = str(tmp_path / "mine.model")
    mdl.save(p, 8)
    c = api.Cascador(p, "double", device=0)
    imgs = [synth.make_frames(1, w, h, seed=9, first=i)[0] for i, (w, h) in enumerate([(160, 120), (131, 97)])]
    mined = c.mine_negatives_cpp(imgs, [3, 4], [1.2, 1.25], [0, 3], 300, device=True)
    n = len(mined["score"])
    assert n == 300, "the synthetic model calls 310 of these 3,425 windows faces"
    w = np.exp(-mined["score"]); w /= w.sum()
    nd = dict(patches=mined["patches"], shapes=mined["shape"], weights=w, residual=None, has_gt=None, sizes=(48, 36, 24))
    pd = train_ref.make_samples(5, 350, 5, gt_drop=0.1)
    D, F = 4, 32
    pools, us = zip(*[train_ref.gen_feature_pool(F, 5, train_ref.RADIUS, True, 8, node) for node in range(1, 8)])
    modes = [1, 1, 0, 1, 1, 0, 1]
    nd_ref = dict(nd, residual=np.zeros((n, 2)), has_gt=np.ones(n, np.uint8))
    pos, neg = train_ref.ref_set(pd), train_ref.ref_set(nd_ref)
    want = train_ref.train_cart(D, pos, neg, [train_ref.pool_of(q) for q in pools], modes, us)
    got = c.train_cart_cpp(pd, nd, _pool([r for q in pools for r in q]), modes, np.array(us))
    assert np.array_equal(got["nodes"]["feature_idx"], np.array(want["features"], np.int32))
    assert np.array_equal(got["thresholds"], np.array(want["thresholds"], np.int32))
    assert same(got["scores"], np.array(want["scores"]))
    assert np.array_equal(got["neg_leaf"], np.array(want["neg_leaf"], np.int32))
    assert np.array_equal(got["pos_leaf"], np.array(want["pos_leaf"], np.int32))
    c.close()


def test_similarity_transform_is_refused(built, gpu, model_file):
    from jda_amd import api
    c = _cascador(model_file, 5)
    pd, nd, rows, u = _node_case(3, 40, 30, 5, False, 8)
    c.set_similarity_transform(True)
    with pytest.raises(api.JdaError, match="data.cpp:168"):
        c.split_node_cpp(pd, nd, _pool(rows), 1)
    c.set_similarity_transform(False)
    assert c.split_node_cpp(pd, nd, _pool(rows), 1)["criterion"].shape == (8,)
    c.close()
