"""The invariant of the model in training (include/jda.h, "Dialect CPP: the model in training") on the device: after every
put and every close, the grown cascador answers validate, mining and detect -- results and work counters -- bit for bit
like a cascador created from the file of that moment.  The mining tables are patched in place and the detect tables
rebuilt; a stale table of either kind shows here."""
import numpy as np
import pytest

from conftest import same
import model_ref

pytestmark = pytest.mark.gpu

T, K, L, D = 2, 5, 5, 3
OS, HS, QS = 24, 18, 12


@pytest.fixture(scope="module")
def gpu():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    return torch.device("cuda", 0)


def _source(seed=4):
    from jda_amd import synth
    return synth.make_model(T, K, L, D, seed=seed, cart_th=-1.0, norm_every=2, multi_scale=True)


def _images():
    from jda_amd import synth
    return [synth.make_frames(1, 64, 48, seed=8, first=i)[0] for i in range(3)]


def _crops(imgs):
    rng = np.random.default_rng(3)
    out = []
    for j in range(20):
        i = j % len(imgs)
        H, W = imgs[i].shape
        w = int(rng.integers(OS, H + 1))
        out.append((i, int(rng.integers(0, W - w + 1)), int(rng.integers(0, H - w + 1)), w, w))
    return np.array(out, np.int32)


COUNTERS = lambda st: {k: v for k, v in st.items() if not k.endswith("_ms")}


def _mine(c, imgs):
    return c.mine_negatives_cpp(imgs, [4] * 3, [1.3] * 3, [0, 3, 6], size=40, origin_size=OS, half_size=HS, quarter_size=QS,
                                shift_size=0.05, seed=11)


def _same_mine(a, b):
    for k in ("hits", "score", "shape", "patches"):
        assert same(a[k], b[k]), k
    assert COUNTERS(a["stats"]) == COUNTERS(b["stats"])


def _same_dets(a, b, keys):
    (ra, sa), (rb, sb) = a, b
    assert len(ra) == len(rb)
    for x, y in zip(ra, rb):
        for k in keys:
            assert same(x[k], y[k]), k
    assert COUNTERS(sa) == COUNTERS(sb)


def _compare(a, b, imgs, crops, frames):
    """Every entry on the grown cascador a and on b, created from the file of the moment."""
    va = a.validate_cpp(imgs, crops, origin_size=OS, half_size=HS, quarter_size=QS, shift_size=0.04, seed=5, stats=True)
    vb = b.validate_cpp(imgs, crops, origin_size=OS, half_size=HS, quarter_size=QS, shift_size=0.04, seed=5, stats=True)
    for k in ("is_face", "score", "carts_n", "shape"):
        assert same(va[0][k], vb[0][k]), k
    assert COUNTERS(va[1]) == COUNTERS(vb[1])
    ma, mb = _mine(a, imgs), _mine(b, imgs)
    _same_mine(ma, mb)
    _same_dets(a.detect_batch_cpp(frames, minimum_size=20, step=3, factor=1.2, stats=True),
               b.detect_batch_cpp(frames, minimum_size=20, step=3, factor=1.2, stats=True), ("rects", "scores", "shapes"))
    _same_dets(a.detect_batch(frames[:1], min_size=24, th=-0.5, stats=True),
               b.detect_batch(frames[:1], min_size=24, th=-0.5, stats=True), ("bboxes", "scores", "shapes"))
    assert a.multi_scale == b.multi_scale and a.model_status_cpp() == b.model_status_cpp()
    return va[0], ma


def test_the_invariant_step_by_step(built, gpu, tmp_path):
    """Every status of a T = 2, K = 5 growth.  Detect runs at every status, the snapshots included (the closed-stage and
    complete ones are the issue's; the others are the same comparison on padded tables)."""
    from jda_amd import api
    src = _source()
    a = api.Cascador.create_training_cpp(T, K, L, D, src.mean_shape)
    ref = model_ref.GrowModel(T, K, L, D, src.mean_shape)
    imgs = _images()
    crops = _crops(imgs)
    frames = np.stack(imgs[:2])
    seen_faces, seen_rejects, seen_hits = 0, 0, 0

    def check(tag):
        nonlocal seen_faces, seen_rejects, seen_hits
        p = str(tmp_path / ("at_%s.model" % tag))
        if a.model_status_cpp()[1] == K - 1:
            ref.save(p)                                   # header (s, K - 1): nothing is written there, the loader accepts it
        else:
            a.serialize_to_cpp(p)
            assert open(p, "rb").read() == ref.tobytes()
        with api.Cascador(p) as b:
            v, m = _compare(a, b, imgs, crops, frames)
        seen_faces += int(v["is_face"].sum()); seen_rejects += int((v["is_face"] == 0).sum()); seen_hits += len(m["hits"])

    check("0_start")
    for t in range(T):
        for k in range(K):
            cart = model_ref.cart_of(src, t, k)
            a.put_cart_cpp(k, *cart); ref.put(k, *cart)
            check("%d_%d" % (t, k))
        a.close_stage_cpp(src.w[t]); ref.close(src.w[t])
        check("%d_closed" % t)
    assert a.model_status_cpp() == (T, -1)
    assert seen_faces > 0 and seen_rejects > 0 and seen_hits > 0      # the comparison saw both outcomes
    a.close()


def test_mining_after_a_put_and_after_a_close_reads_the_new_model(built, gpu, tmp_path):
    """mine, put, mine on ONE cascador: the second call's tables were built by the first and must have been patched; the
    same around close, where `full` / `part` and the stage's w change.  The models differ enough for the results to differ."""
    from jda_amd import api
    src = _source(seed=6)
    imgs = _images()
    a = api.Cascador.create_training_cpp(T, K, L, D, src.mean_shape)
    ref = model_ref.GrowModel(T, K, L, D, src.mean_shape)

    def fresh():
        p = ref.save(str(tmp_path / "fresh.model"))
        with api.Cascador(p) as b:
            return _mine(b, imgs)

    for k in range(K - 1):
        cart = model_ref.cart_of(src, 0, k)
        a.put_cart_cpp(k, *cart); ref.put(k, *cart)
    before = _mine(a, imgs)                               # builds the tables at (0, K - 2)
    _same_mine(before, fresh())
    cart = model_ref.cart_of(src, 0, K - 1)
    a.put_cart_cpp(K - 1, *cart); ref.put(K - 1, *cart)
    after_put = _mine(a, imgs)
    _same_mine(after_put, fresh())
    assert not same(after_put["score"], before["score"])
    a.close_stage_cpp(src.w[0]); ref.close(src.w[0])
    cart = model_ref.cart_of(src, 1, 0)
    a.put_cart_cpp(0, *cart); ref.put(0, *cart)           # a cart of stage 1 walks on the shape stage 0's w moved
    after_close = _mine(a, imgs)
    _same_mine(after_close, fresh())
    assert not same(after_close["shape"], after_put["shape"])
    # replacing the last cart: the restart path
    other = _source(seed=7)
    cart = model_ref.cart_of(other, 1, 0)
    a.put_cart_cpp(0, *cart); ref.put(0, *cart)
    _same_mine(_mine(a, imgs), fresh())
    a.close()


def test_fifty_rounds_of_mine_grow_detect(built, gpu):
    """One cascador that mines, has its last cart replaced and detects in both dialects, 50 times over: nothing fails, equal
    models give equal answers, and from the end of the first round on nothing changes -- ws_regrows of both detect calls
    (jdaMineStats has no such counter: mining sizes no queue from earlier passes), the bytes the cascador holds on the device
    (model tables of both dialects, mining tables, every lane's buffers: all grow-only, so a leak shows as growth) and the
    number of plan buffers in the plan map and the pool.  Rounds alternate between two models of the same dimensions; every
    put resets the queue hints, so a round sizes its queues like a fresh cascador whichever model it holds."""
    from jda_amd import api
    src, other = _source(seed=4), _source(seed=9)
    imgs = _images()
    frames = np.stack(imgs[:2])
    a = api.Cascador.create_training_cpp(T, K, L, D, src.mean_shape)
    for k in range(K):
        a.put_cart_cpp(k, *model_ref.cart_of(src, 0, k))
    a.close_stage_cpp(src.w[0])
    a.put_cart_cpp(0, *model_ref.cart_of(src, 1, 0))
    first = {}
    flat = []
    for r in range(50):
        which = r & 1
        a.put_cart_cpp(0, *model_ref.cart_of(other if which else src, 1, 0))
        m = _mine(a, imgs)
        dc, sc = a.detect_batch_cpp(frames, minimum_size=20, step=3, factor=1.2, stats=True)
        df, sf = a.detect_batch(frames, min_size=24, th=-0.5, stats=True)
        flat.append((sc["ws_regrows"], sf["ws_regrows"], a.get_option("mem_device_bytes"), a.get_option("mem_plan_buffers")))
        if which not in first:
            first[which] = (m, dc, df)
            continue
        m0, dc0, df0 = first[which]
        _same_mine(m, m0)
        for x, y in zip(dc, dc0):
            assert same(x["scores"], y["scores"]) and same(x["shapes"], y["shapes"]) and same(x["rects"], y["rects"])
        for x, y in zip(df, df0):
            assert same(x["scores"], y["scores"]) and same(x["shapes"], y["shapes"]) and same(x["bboxes"], y["bboxes"])
    assert a.model_status_cpp() == (1, 0)
    print("round 0:", flat[0])
    assert flat[0][2] > 0 and flat[0][3] == 2                      # something is held, and one plan per dialect
    assert all(v == flat[0] for v in flat[1:]), flat
    assert not same(first[0][0]["score"], first[1][0]["score"])    # the two models do differ
    a.close()


def test_the_model_written_is_the_model_trained(built, gpu, tmp_path):
    """One stage of real pieces at the sizes of tests/test_fit.py's whole-stage case (60 + 60 samples, L = 5, D = 3, F = 24,
    K = 6, patches 48 / 36 / 24): build_positives_cpp, random_shapes_cpp, K x (update_weights_cpp, train_cart_cpp,
    boost_scores_cpp, put_cart_cpp), gen_lbf_cpp, global_regression_cpp, close_stage_cpp, stage_update_shapes_cpp -- every cart
    the model gets is jdaTrainCartCpp's output as it is.  Then Validate under the file the grown cascador writes, on every
    positive's three stored patches from the shape it started from, must return the score the trainer carried and the shape
    the stage update left, bit for bit, with every sample a face after K carts; and after a further put in stage 1 the scores
    boost_scores_cpp carries.  Every cart's threshold is the smallest carried positive score, so no positive is cut and
    `score == th` is exercised.  Validate is validate_samples_cpp on the device, in both forms, and tests/model_ref.py's
    sequential restatement; all three must agree with what the trainer carried."""
    from jda_amd import api, synth
    import stage_ref
    import train_ref
    Le, De, F, Ke, n = 5, 3, 24, 6, 60
    rng = np.random.default_rng(17)
    mean = synth.make_mean_shape(Le, rng)
    a = api.Cascador.create_training_cpp(2, Ke, Le, De, mean)
    imgs = [synth.make_frames(1, 96, 80, seed=21, first=i)[0] for i in range(6)]
    faces = []
    for i in range(n):
        w = int(rng.integers(30, 61))
        faces.append((i % 6, int(rng.integers(-5, 96 - w + 5)), int(rng.integers(-5, 80 - w + 5)), w, w))     # some leave the image
    pos_patches = a.build_positives_cpp(imgs, faces)
    start = api.random_shapes_cpp(mean, n, shift_size=0.05, seed=3)
    gt = start + rng.normal(0, 0.04, start.shape) + 0.03
    nd = train_ref.make_samples(131, n, Le)
    nd["shapes"] = api.random_shapes_cpp(mean, n, shift_size=0.05, seed=3, first_key=n)
    pos_scores, neg_scores = np.zeros(n), np.zeros(n)
    shapes = start

    def one_cart(k, stage):
        nonlocal pos_scores, neg_scores
        pw, nw = api.update_weights_cpp(pos_scores, neg_scores)
        pd = dict(patches=pos_patches, shapes=shapes, weights=pw, residual=api.shape_residual_cpp(gt, shapes, landmark_id=k % Le))
        ng = dict(nd, weights=nw)
        pools = [train_ref.gen_feature_pool(F, Le, train_ref.RADIUS, True, 100 * stage + 31 + k, node) for node in range(1, 4)]
        flat = stage_ref.pool_array([r for p, _ in pools for r in p])
        got = a.train_cart_cpp(pd, ng, flat, [1, 0, 1], np.array([u for _, u in pools]))
        b = api.boost_scores_cpp(got["scores"], got["pos_leaf"], got["neg_leaf"], pos_scores, neg_scores, normalize=(k + 1) % 2 == 0)
        pos_scores, neg_scores = b["pos_scores"], b["neg_scores"]
        a.put_cart_cpp(k, got["features"], got["thresholds"], got["scores"], float(pos_scores.min()), b["mean"], b["std"])
        return got

    def validate_all(tag):
        p = str(tmp_path / (tag + ".model"))
        a.serialize_to_cpp(p)
        from oracle import cpp_reading2 as r2
        m2 = r2.Model2(p)
        out = []
        for i in range(n):
            row = pos_patches[i]
            o, h, q = row[:2304].reshape(48, 48), row[2304:2304 + 1296].reshape(36, 36), row[2304 + 1296:].reshape(24, 24)
            out.append(model_ref.validate_record(m2, o, h, q, start[i]))
        ref = ([r[0] for r in out], np.array([r[1] for r in out]), np.array([r[2] for r in out]), [r[3] for r in out])
        for form in (0, 1):                               # ... and the device entry, both forms, on the resident positives
            a.set_option("reval_form", form)
            got = a.validate_samples_cpp(dict(patches=pos_patches, shapes=start))
            assert got["is_face"].tolist() == [int(f) for f in ref[0]] and got["carts_n"].tolist() == ref[3]
            assert same(got["score"], ref[1]) and same(got["shape"], ref[2])
        return ref

    carts = [one_cart(k, 0) for k in range(Ke - 1)]
    face, score, shape, cn = validate_all("mid")                   # (0, K - 2): the partial stage, no regression
    assert all(face) and cn == [Ke - 1] * n and same(score, pos_scores) and same(shape, start)
    carts.append(one_cart(Ke - 1, 0))
    feats, ths = np.concatenate([c["features"] for c in carts]), np.concatenate([c["thresholds"] for c in carts])
    pos = dict(patches=pos_patches, shapes=shapes)
    lbf = a.gen_lbf_cpp(pos, feats, ths)
    w = a.global_regression_cpp(lbf, api.shape_residual_cpp(gt, shapes), C=10.0, max_iter=40, seed=9)[0]
    a.close_stage_cpp(w)
    shapes = a.stage_update_shapes_cpp(pos, None, None, w, lbf)
    assert a.model_status_cpp() == (1, -1) and not same(shapes, start)
    face, score, shape, cn = validate_all("closed")
    assert all(face) and cn == [Ke] * n
    assert same(score, pos_scores) and same(shape, shapes)
    assert len(set(pos_scores.tolist())) > n // 2                   # the carried scores are not a constant
    one_cart(0, 1)                                                  # stage 1 trains on the updated shapes
    face, score, shape, cn = validate_all("next")
    assert all(face) and cn == [Ke + 1] * n
    assert same(score, pos_scores) and same(shape, shapes)
    a.close()
