"""The similarity transform in training (option "train_similarity", include/jda.h), the part that needs no device: the
restatement tests/st_ref.py against oracle/cpp_reading2.py's Validate, jdaShapeResidualStCpp, the option's default with the
refusals it leaves standing, and the shortcut for stp_cm the device does NOT take.  Every comparison is exact."""
import ctypes as C

import numpy as np
import pytest

from conftest import same
from oracle import cpp_reading2 as r2
import model_ref
import st_ref
import train_ref


def _split(row, sizes):
    o, h, q = sizes
    return row[:o * o].reshape(o, o), row[o * o:o * o + h * h].reshape(h, h), row[o * o + h * h:].reshape(q, q)


@pytest.mark.parametrize("hdr", [None, (1, 1), (0, 0)])
def test_restatement_equals_the_second_reading_of_validate(hdr):
    """st_ref.validate_record from the mean shape against cpp_reading2.validate(similarity=True): a one-cart-a-stage model
    (two stages, so that stage 1 computes its parameter from a regressed shape), a snapshot inside stage 1 (the partial stage
    keeps stage 0's parameter) and one inside stage 0 (the default parameter)."""
    from jda_amd import synth
    m = synth.make_model(2, 2 if hdr else 1, 5, 4, seed=7, cart_th=-0.2, norm_every=1, multi_scale=True, w_sigma=3e-2, f32_exact=False)
    blob = m.tobytes(8) if hdr is None else m.tobytes(8, *hdr)
    m2 = model_ref.model2_of(blob)
    rng = np.random.default_rng(3)
    faces = 0
    for i in range(24):
        o, h, q = _split(rng.integers(0, 256, sum(v * v for v in st_ref.ODD), dtype=np.uint8), st_ref.ODD)
        patches = tuple((p.tolist(), 0, 0, p.shape[1], p.shape[0]) for p in (o, h, q))
        want = r2.validate(m2, None, patches=patches, similarity=True)
        got = st_ref.validate_record(m2, o, h, q, m2.mean_shape)
        assert got[0] == want[0] and got[3] == want[3]
        assert same(np.array([got[1]] + got[2]), np.array([want[1]] + want[2]))
        faces += int(got[0])
    assert 0 < faces < 24


def test_inputs_make_the_transform_matter():
    """More than half of the (feature, sample) values differ from the identity reading, on the restatement alone, for the
    shapes and pools the GPU tests use (all three scales, odd patch sizes)."""
    from jda_amd import synth
    for L in (5, 33):
        mean = synth.make_mean_shape(L, np.random.default_rng(L))
        d = st_ref.make_samples(40 + L, 70, mean)
        rows, _ = train_ref.gen_feature_pool(70, L, 0.45, True, 5, 9)
        assert {r[0] for r in rows} == {0, 1, 2}
        mc, _ = st_ref.st_parameters(d["shapes"], mean)
        share = st_ref.differing_share(train_ref.ref_set(d), train_ref.pool_of(rows), mc)
        print("L = %d: %.3f of the values differ from the identity reading" % (L, share))
        assert share > 0.5


def test_stp_cm_derived_from_stp_mc_is_not_calc_run_twice():
    """stp_cm = Calc(mean_shape, shape) against the shortcut (scale2 / scale1, the same cosine, the sine negated): the same
    bits for every rotated, scaled, noisy shape -- each term of `num` negates exactly -- but NOT for a shape that equals the
    mean shape (every negative sample's start with shift_size 0): there every term of `num` is +0. in both orders, the sine
    is +0. in both and the shortcut's rot entries are -0. where Calc gives +0.  So k_stp runs a second pair of add chains."""
    from jda_amd import synth
    for L in (2, 5, 6, 33):
        mean = synth.make_mean_shape(L, np.random.default_rng(L))
        shapes = st_ref.make_shapes(L, 50, mean)
        mc, cm = st_ref.st_parameters(shapes, mean)
        for a, b in zip(mc, cm):
            assert same(np.array(st_ref.derive_cm(a, b[0])), np.array(b))
    mean = synth.make_mean_shape(5, np.random.default_rng(5))
    mc, cm = st_ref.st_parameters([mean], mean)
    assert cm[0][2] == 0. and cm[0][3] == 0.
    assert not same(np.array(st_ref.derive_cm(mc[0], cm[0][0])), np.array(cm[0]))


def test_shape_residual_st(built):
    from jda_amd import api, synth
    L, size = 5, 12
    mean = synth.make_mean_shape(L, np.random.default_rng(1))
    cur = st_ref.make_shapes(2, size, mean)
    gt = cur + np.random.default_rng(3).normal(0, 0.03, cur.shape)
    _, cm = st_ref.st_parameters(cur, mean)
    cm_a = np.array(cm, np.float64)
    idx = [7, 0, 0, 11, 3]
    mask = (np.arange(size) % 3 != 0).astype(np.int32)
    got_all, hg = api.shape_residual_cpp(gt, cur, idx, shape_mask=mask, stp_cm=cm_a)
    assert same(got_all, np.array(st_ref.shape_residual(gt, cur, idx, cm), np.float64)) and same(hg, mask[idx].astype(np.uint8))
    got_one = api.shape_residual_cpp(gt, cur, idx, landmark_id=3, stp_cm=cm_a)
    assert same(got_one, np.array(st_ref.shape_residual(gt, cur, idx, cm, 3), np.float64))
    assert not same(got_all, api.shape_residual_cpp(gt, cur, idx))               # the transform is visible
    # NULL stp_cm: jdaShapeResidualCpp's bits, through the new entry itself
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int)
    ix = np.array(idx, np.int32)

    def raw(stp, out, lid=-1, idx_p=ix.ctypes.data_as(ip), n=len(idx), size_=size):
        return api.lib.jdaShapeResidualStCpp(gt.ctypes.data_as(dp), cur.ctypes.data_as(dp), None, size_, L, idx_p, n, lid, stp,
                                             out.ctypes.data_as(dp), None)
    out = np.zeros((len(idx), 2 * L))
    assert raw(None, out) == 0 and same(out, api.shape_residual_cpp(gt, cur, idx))
    # the identity rows give x + 0. * y: equal values (a -0. may become +0.)
    ident = np.tile(np.array(r2.IDENTITY), (size, 1))
    assert np.array_equal(api.shape_residual_cpp(gt, cur, idx, stp_cm=ident), api.shape_residual_cpp(gt, cur, idx))
    # refusals, outputs untouched
    out[:] = 7.5
    assert raw(cm_a.ctypes.data_as(dp), out, lid=L) == -1 and "landmark_id" in api.last_error()
    assert raw(cm_a.ctypes.data_as(dp), out, lid=-2) == -1
    bad = np.array([0, size, 1, 2, 3], np.int32)
    assert raw(cm_a.ctypes.data_as(dp), out, idx_p=bad.ctypes.data_as(ip)) == -1 and "outside" in api.last_error()
    assert raw(cm_a.ctypes.data_as(dp), out, idx_p=None) == -1 and raw(cm_a.ctypes.data_as(dp), out, n=-1) == -1
    assert api.lib.jdaShapeResidualStCpp(None, cur.ctypes.data_as(dp), None, size, L, ix.ctypes.data_as(ip), 5, -1, None, out.ctypes.data_as(dp), None) == -1
    hgo = np.zeros(5, np.uint8)
    assert api.lib.jdaShapeResidualStCpp(gt.ctypes.data_as(dp), cur.ctypes.data_as(dp), None, size, L, ix.ctypes.data_as(ip), 5, -1, None,
                                         out.ctypes.data_as(dp), hgo.ctypes.data_as(C.POINTER(C.c_ubyte))) == -1
    assert (out == 7.5).all()
    assert raw(cm_a.ctypes.data_as(dp), out, n=0) == 0 and (out == 7.5).all()


def test_option_defaults_to_off_and_the_refusals_stand(built, model_file):
    from jda_amd import api
    p, m = model_file((1, 2, 5, 4))
    c = api.Cascador(p, "double")
    assert c.get_option("train_similarity") == 0
    pos, neg = train_ref.make_samples(1, 6, 5), train_ref.make_samples(2, 5, 5)
    pool, _ = api.gen_feature_pool_cpp(8, 5, 0.3, True, 1, 1)
    w = np.zeros((2 * 8, 10))
    lbf = np.tile(np.arange(2, dtype=np.int32) * 8, (6, 1))
    calls = (lambda: c.calc_feature_values_cpp(pos, pool), lambda: c.split_node_cpp(pos, neg, pool, 1),
             lambda: c.train_cart_cpp(pos, neg, np.tile(pool, 7), [1] * 7), lambda: c.gen_lbf_cpp(pos, np.tile(pool, 2)[:14], np.zeros(14, np.int32)),
             lambda: c.stage_update_shapes_cpp(pos, None, None, w, lbf), lambda: c.validate_samples_cpp(pos))
    c.set_option("train_similarity", 1)                   # the option alone changes nothing ...
    c.set_similarity_transform(True)
    c.set_option("train_similarity", 0)                   # ... and without it the transform is refused, as before
    for call in calls:
        with pytest.raises(api.JdaError, match="jdaSetSimilarityTransform"):
            call()
    with pytest.raises(api.JdaError):
        c.set_option("train_similarity", -1)
    # jdaCalcSTParametersCpp needs no opt-in; what it refuses, and what it does without a device
    dp = C.POINTER(C.c_double)
    out = np.full((3, 5), 7.5)
    sh = np.zeros((3, 10))
    assert api.lib.jdaCalcSTParametersCpp(c.h, None, 3, out.ctypes.data_as(dp), None) == -1
    assert api.lib.jdaCalcSTParametersCpp(c.h, sh.ctypes.data_as(dp), -1, out.ctypes.data_as(dp), None) == -1
    assert api.lib.jdaCalcSTParametersCpp(None, sh.ctypes.data_as(dp), 3, out.ctypes.data_as(dp), None) == -1
    assert (out == 7.5).all()
    assert api.lib.jdaCalcSTParametersCpp(c.h, None, 0, out.ctypes.data_as(dp), None) == 0 and (out == 7.5).all()
    c.set_similarity_transform(False)                     # the transform off: STParameter's default, no device
    mc, cm = c.calc_st_parameters_cpp(sh)
    assert same(mc, np.tile(np.array(r2.IDENTITY), (3, 1))) and same(cm, mc)
    c.close()
