"""CPU-side checks of the stage-close entries (include/jda.h, "Dialect CPP: closing a stage"): the symbols, the host-only
mean error against tests/stage_ref.py, n == 0, every refusal that must come before the device is touched (on a machine
without a GPU a call that reached the device would fail with a HIP error instead of the reason matched here), and the
CONTROL of the yardstick of tests/test_stage_close.py -- on that test's own weight rows, summing in reversed cart order
changes bits, so "bit-exact in cart order" tests something."""
import numpy as np
import pytest

from conftest import same
import stage_ref
import train_ref


def _cascador(model_file, L=5, D=4):
    from jda_amd import api
    p, _ = model_file((1, 2, L, D))
    return api.Cascador(p, "double")


def test_the_three_symbols_are_exported(built):
    from jda_amd import api
    for name in ("jdaGenLbfCpp", "jdaStageUpdateShapesCpp", "jdaMeanErrorCpp"):
        assert hasattr(api.lib, name), name


@pytest.mark.parametrize("L,left,right", [(5, [0], [1]), (27, [3, 7, 11], [20, 2]), (68, [36, 37, 38, 39, 40, 41], [42, 43, 44, 45, 46, 47])])
def test_mean_error_equals_the_restatement(built, L, left, right):
    from jda_amd import api
    rng = np.random.default_rng(L)
    n = 37
    gt = rng.uniform(0.1, 0.9, (n, 2 * L))
    cur = gt + rng.normal(0, 0.03, (n, 2 * L)) * np.exp2(rng.integers(-20, 1, (n, 1)))
    want = stage_ref.mean_error(gt.tolist(), cur.tolist(), L, left, right)
    got = api.mean_error_cpp(gt, cur, left, right)
    print("mean error %r / %r" % (got, want))
    assert same(np.float64(got), np.float64(want)) and 0 < got < 1
    assert api.mean_error_cpp(gt, gt, left, right) == 0.
    assert np.isnan(api.mean_error_cpp(gt[:0], cur[:0], left, right))       # n == 0: returns 0; 0. / 0. like the reference


def test_mean_error_refuses_bad_arguments(built):
    from jda_amd import api
    gt = np.full((3, 10), 0.5)
    for left, right in (([5], [1]), ([0], [-1]), ([], [1]), ([0], [])):
        with pytest.raises(api.JdaError):
            api.mean_error_cpp(gt, gt, left, right)
    assert api.lib.jdaMeanErrorCpp(None, None, 3, 5, None, 1, None, 1, None) == -1 and api.last_error()


def test_empty_set_returns_at_once(built, model_file):
    c = _cascador(model_file)
    rows, th = stage_ref.make_carts(1, 3, 4, 5, True)
    d = train_ref.make_samples(1, 0, 5)
    assert c.gen_lbf_cpp(d, stage_ref.pool_array(rows), th).shape == (0, 3)
    out, lbf = c.stage_update_shapes_cpp(d, stage_ref.pool_array(rows), th, stage_ref.make_w(1, 3, 4, 5), want_lbf=True)
    assert out.shape == (0, 10) and lbf.shape == (0, 3)
    c.close()


def test_refusals_that_need_no_device(built, model_file):
    from jda_amd import api
    import ctypes as C
    L, D, K = 5, 4, 3
    c = _cascador(model_file, L, D)
    d = train_ref.make_samples(1, 6, L)
    rows, th = stage_ref.make_carts(1, K, D, L, True)
    pool, w = stage_ref.pool_array(rows), stage_ref.make_w(1, K, D, L)
    good_lbf = np.arange(K, dtype=np.int32)[None, :] * 8 + np.zeros((6, 1), np.int32)
    both = (lambda **kw: c.gen_lbf_cpp(kw.get("d", d), kw.get("pool", pool), th, *kw.get("sizes", ())),
            lambda **kw: c.stage_update_shapes_cpp(kw.get("d", d), kw.get("pool", pool), th, w, None, *kw.get("sizes", ())))
    for call in both:
        with pytest.raises(api.JdaError, match=r"\[1, 128\]"):
            call(d=dict(d, patches=np.zeros((6, 129 * 129 + 2), np.uint8)), sizes=(129, 1, 1))
        with pytest.raises(api.JdaError, match=r"\[1, 128\]"):
            call(d=dict(d, patches=np.zeros((6, 48 * 48 + 36 * 36), np.uint8)), sizes=(48, 36, 0))
        bad = pool.copy(); bad["scale"][4] = 3
        with pytest.raises(api.JdaError, match="scale"):
            call(pool=bad)
        bad = pool.copy(); bad["scale"][0] = -1
        with pytest.raises(api.JdaError, match="scale"):
            call(pool=bad)
        bad = pool.copy(); bad["landmark_id1"][len(bad) - 1] = L
        with pytest.raises(api.JdaError, match="landmark"):
            call(pool=bad)
        bad = pool.copy(); bad["landmark_id2"][2] = -1
        with pytest.raises(api.JdaError, match="landmark"):
            call(pool=bad)
    # K <= 0, NULL pointers: through the C ABI itself
    s, keep = api._samples(d, 2 * L, 48 * 48 + 36 * 36 + 24 * 24)
    carts, kc = api._stage_carts(pool, th, 7)
    out = np.zeros((6, 2 * L)); lbf = np.zeros((6, K), np.int32)
    ip, dp = C.POINTER(C.c_int), C.POINTER(C.c_double)
    sizes = (48, 36, 24)

    def refused(rc, what):
        assert rc == -1 and what in api.last_error(), (rc, api.last_error())
    for k in (0, -4):
        carts.K = k
        refused(api.lib.jdaGenLbfCpp(c.h, C.byref(s), *sizes, C.byref(carts), lbf.ctypes.data_as(ip)), "K must be positive")
        refused(api.lib.jdaStageUpdateShapesCpp(c.h, C.byref(s), *sizes, C.byref(carts), w.ctypes.data_as(dp), None,
                                                out.ctypes.data_as(dp), None, None), "K must be positive")
    carts.K = K
    refused(api.lib.jdaGenLbfCpp(None, C.byref(s), *sizes, C.byref(carts), lbf.ctypes.data_as(ip)), "bad arguments")
    refused(api.lib.jdaGenLbfCpp(c.h, None, *sizes, C.byref(carts), lbf.ctypes.data_as(ip)), "null sample set")
    refused(api.lib.jdaGenLbfCpp(c.h, C.byref(s), *sizes, None, lbf.ctypes.data_as(ip)), "bad arguments")
    refused(api.lib.jdaGenLbfCpp(c.h, C.byref(s), *sizes, C.byref(carts), None), "no output")
    refused(api.lib.jdaStageUpdateShapesCpp(c.h, C.byref(s), *sizes, C.byref(carts), None, None, out.ctypes.data_as(dp), None, None),
            "w must be given")
    refused(api.lib.jdaStageUpdateShapesCpp(c.h, C.byref(s), *sizes, C.byref(carts), w.ctypes.data_as(dp), None, None, None, None),
            "out_shapes")
    refused(api.lib.jdaStageUpdateShapesCpp(c.h, C.byref(s), *sizes, None, w.ctypes.data_as(dp), None, out.ctypes.data_as(dp), None, None),
            "carts must be given")
    no_arrays = api.jdaStageCartsCpp(); no_arrays.K = K
    refused(api.lib.jdaGenLbfCpp(c.h, C.byref(s), *sizes, C.byref(no_arrays), lbf.ctypes.data_as(ip)), "features and thresholds")
    empty = api.jdaSamplesCpp(); empty.n = 6
    refused(api.lib.jdaGenLbfCpp(c.h, C.byref(empty), *sizes, C.byref(carts), lbf.ctypes.data_as(ip)), "patches, shapes")
    # indices that are not a leaf of their cart
    for i, k, v in ((0, 0, -1), (5, 2, 2 * 8 - 1), (3, 1, 2 * 8)):
        bad = good_lbf.copy(); bad[i, k] = v
        with pytest.raises(api.JdaError, match=r"lbf_in\[%d\] is not a leaf of cart %d" % (i * K + k, k)):
            c.stage_update_shapes_cpp(d, None, None, w, bad)
    # the similarity transform: refused, for the reason the header gives
    c.set_similarity_transform(True)
    for call in both + (lambda: c.stage_update_shapes_cpp(d, None, None, w, good_lbf),):
        with pytest.raises(api.JdaError, match="jdaSetSimilarityTransform"):
            call()
    c.close()
    del keep, kc


# the order-control case of tests/test_stage_close.py: (seed, n, K, D, L)
def test_control_reversed_cart_order_changes_the_shapes():
    seed, n, K, D, L = stage_ref.ORDER_CASE
    d = train_ref.make_samples(seed, n, L)
    rows, th = stage_ref.make_carts(seed, K, D, L, True)
    carts = stage_ref.carts_of(D, rows, th)
    w = stage_ref.make_w(seed, K, D, L).tolist()
    s = train_ref.ref_set(d)
    fwd, lbf = stage_ref.stage_update(D, carts, s, w)
    rev, _ = stage_ref.stage_update(D, carts, s, w, lbf=lbf, reverse=True)
    differing = sum(1 for a, b in zip(sum(fwd, []), sum(rev, [])) if not same(np.float64(a), np.float64(b)))
    print("coordinates whose bits change under reversed cart order: %d of %d" % (differing, n * 2 * L))
    assert differing >= 1
    assert max(abs(a - b) for a, b in zip(sum(fwd, []), sum(rev, []))) < 1e-12     # ... and nothing but the order changed
