"""The model in training on the host (no GPU): jdaCascadorCreateTrainingCpp, jdaModelStatusCpp, jdaModelPutCartCpp,
jdaModelCloseStageCpp and jdaCascadorSerializeToCpp against the plain-Python model of tests/model_ref.py, whose file goes
through jda_amd.synth.Model.tobytes.  Dialect CPP is parity-unpinned: the writer is checked against the layout restated in
Python, not against a file the reference wrote."""
import ctypes as C
import struct

import numpy as np
import pytest

import model_ref

T, K, L, D = 2, 3, 4, 3


def _source(multi=False, seed=5):
    from jda_amd import synth
    return synth.make_model(T, K, L, D, seed=seed, cart_th=-0.75, norm_every=2, multi_scale=multi, f32_exact=False)


def _pair(src):
    from jda_amd import api
    return api.Cascador.create_training_cpp(T, K, L, D, src.mean_shape), model_ref.GrowModel(T, K, L, D, src.mean_shape)


def _blob(c, tmp_path, name="out.model"):
    p = str(tmp_path / name)
    c.serialize_to_cpp(p)
    return open(p, "rb").read()


def _grow_to(c, ref, src, stage, cart):
    """Both models to status (stage, cart) with src's content."""
    for t in range(T):
        if (t, -1) == (stage, cart):
            return
        for k in range(K):
            a = model_ref.cart_of(src, t, k)
            c.put_cart_cpp(k, *a); ref.put(k, *a)
            if (t, k) == (stage, cart):
                return
        c.close_stage_cpp(src.w[t]); ref.close(src.w[t])
    assert (stage, cart) == (T, -1)


@pytest.mark.parametrize("status", [(0, -1), (0, 1), (1, -1), (T, -1)])
def test_file_equals_the_python_writer_and_reloads_to_itself(built, tmp_path, status):
    """(0, 1) stands for the issue's (0, 2) at K = 3, where (0, 2) = (s, K - 1) is the status nothing is written at."""
    from jda_amd import api
    src = _source()
    c, ref = _pair(src)
    _grow_to(c, ref, src, *status)
    assert c.model_status_cpp() == status == ref.status()
    blob = _blob(c, tmp_path)
    assert blob == ref.tobytes()
    assert struct.unpack_from("<7i", blob) == (0, T, K, L, D) + status
    with api.Cascador(str(tmp_path / "out.model")) as again:
        assert again.model_status_cpp() == status and again.source_real_bytes == 8
        assert _blob(again, tmp_path, "again.model") == blob
    c.close()


def test_status_two_of_a_four_cart_stage(built, tmp_path):
    """The issue's status (0, 2), at a K where it is not the last cart."""
    from jda_amd import api, synth
    src = synth.make_model(1, 4, L, D, seed=2, norm_every=2, f32_exact=False)
    c = api.Cascador.create_training_cpp(1, 4, L, D, src.mean_shape)
    ref = model_ref.GrowModel(1, 4, L, D, src.mean_shape)
    for k in range(3):
        a = model_ref.cart_of(src, 0, k)
        c.put_cart_cpp(k, *a); ref.put(k, *a)
    assert c.model_status_cpp() == (0, 2)
    assert _blob(c, tmp_path) == ref.tobytes()
    c.close()


def test_every_step_of_a_growth_agrees_with_the_python_model(built, tmp_path):
    src = _source()
    c, ref = _pair(src)
    steps = 0
    assert _blob(c, tmp_path) == ref.tobytes()
    for t in range(T):
        for k in range(K):
            a = model_ref.cart_of(src, t, k)
            c.put_cart_cpp(k, *a); ref.put(k, *a)
            assert c.model_status_cpp() == ref.status() == (t, k)
            if k < K - 1:
                assert _blob(c, tmp_path) == ref.tobytes()
            steps += 1
        c.close_stage_cpp(src.w[t]); ref.close(src.w[t])
        assert c.model_status_cpp() == ref.status() == (t + 1, -1)
        assert _blob(c, tmp_path) == ref.tobytes()
        steps += 1
    assert steps == T * (K + 1) and _blob(c, tmp_path) == src.tobytes(8)       # the complete model IS the source, header (T, -1)
    c.close()


def test_node_order_is_cart_serialize_to(built, tmp_path):
    """Cart::SerializeTo (cart.cpp:429-450): for node i = 1 .. nodes_n/2 - 1 {scale, id1, id2, four offsets, threshold}, then
    scores[0 .. nodes_n/2), then th, mean, std.  One cart of depth 4 with a distinct value everywhere, read back from the
    file by hand."""
    from jda_amd import api
    D4, L4 = 4, 9
    c = api.Cascador.create_training_cpp(1, 2, L4, D4, np.arange(2 * L4) / 32.0)
    nodes, leaves = 7, 8
    f = np.zeros(nodes, api.FEATURE_DTYPE)
    f["scale"] = [0, 1, 2, 0, 1, 2, 0]
    f["landmark_id1"] = np.arange(nodes) + 1
    f["landmark_id2"] = 8 - np.arange(nodes)
    for j, name in enumerate(("offset1_x", "offset1_y", "offset2_x", "offset2_y")):
        f[name] = 0.001 * (np.arange(nodes) + 1) + 0.1 * (j + 1)
    ths = np.arange(nodes, dtype=np.int32) * 3 - 7
    sc = 10.0 + np.arange(leaves)
    c.put_cart_cpp(0, f, ths, sc, -1.5, 0.25, 2.0)
    blob = _blob(c, tmp_path)
    at = 28 + 2 * L4 * 8
    for i in range(1, nodes + 1):                       # node i of Cart::features is slot i - 1
        scale, id1, id2 = struct.unpack_from("<3i", blob, at); at += 12
        offs = struct.unpack_from("<4d", blob, at); at += 32
        (nth,) = struct.unpack_from("<i", blob, at); at += 4
        assert (scale, id1, id2, nth) == (f["scale"][i - 1], i, 9 - i, 3 * (i - 1) - 7)
        assert offs == tuple(0.001 * i + 0.1 * (j + 1) for j in range(4))
    assert struct.unpack_from("<8d", blob, at) == tuple(sc); at += 64
    assert struct.unpack_from("<3d", blob, at) == (-1.5, 0.25, 2.0); at += 24
    # the next cart is the constructor's: Feature() nodes, zero scores, th 0 (uninitialised in the reference), mean 0, std 1
    assert blob[at:at + nodes * 48 + leaves * 8] == bytes(nodes * 48 + leaves * 8)
    assert struct.unpack_from("<3d", blob, at + nodes * 48 + leaves * 8) == (0.0, 0.0, 1.0)
    c.close()


def test_a_new_training_model_is_the_constructors(built, tmp_path):
    from jda_amd import api, synth
    ms = np.linspace(0.2, 0.8, 2 * L)
    c = api.Cascador.create_training_cpp(T, K, L, D, ms)
    empty = synth.Model(T, K, L, D)
    empty.mean_shape = ms
    assert c.model_status_cpp() == (0, -1) and (c.T, c.K, c.L, c.D) == (T, K, L, D) and not c.multi_scale
    assert _blob(c, tmp_path) == empty.tobytes(8, 0, -1)
    c.close()
    for bad in [(0, K, L, D), (17, K, L, D), (T, 0, L, D), (T, K, 0, D), (T, K, 4097, D), (T, K, L, 1), (T, K, L, 13)]:
        assert not api.lib.jdaCascadorCreateTrainingCpp(*bad, ms.ctypes.data_as(C.POINTER(C.c_double)))
        assert "dimensions" in api.last_error()
    assert not api.lib.jdaCascadorCreateTrainingCpp(T, K, L, D, None) and "mean_shape" in api.last_error()


def _refused(c, tmp_path, before, call, match):
    from jda_amd import api
    status = c.model_status_cpp()
    with pytest.raises(api.JdaError, match=match):
        call()
    assert c.model_status_cpp() == status
    if before is not None:
        assert _blob(c, tmp_path, "after.model") == before


def test_every_refusal_leaves_model_and_status_untouched(built, tmp_path):
    from jda_amd import api
    src = _source()
    c, ref = _pair(src)
    a = model_ref.cart_of(src, 0, 0)
    before = _blob(c, tmp_path)
    # at (0, -1): nothing to replace, nothing to close, k too far ahead or behind
    _refused(c, tmp_path, before, lambda: c.put_cart_cpp(-1, *a), "neither appended nor replaced")
    _refused(c, tmp_path, before, lambda: c.put_cart_cpp(1, *a), "neither appended nor replaced")
    _refused(c, tmp_path, before, lambda: c.put_cart_cpp(-2, *a), "neither appended nor replaced")
    _refused(c, tmp_path, before, lambda: c.close_stage_cpp(src.w[0]), "0 of its 3 carts")
    # bad content
    for field, v in (("scale", 3), ("scale", -1), ("landmark_id1", L), ("landmark_id2", -1)):
        f = a[0].copy(); f[field][1] = v
        _refused(c, tmp_path, before, lambda: c.put_cart_cpp(0, f, *a[1:]), "scale outside 0..2 or a landmark id")
    for std in (0.0, float("nan"), float("inf")):
        _refused(c, tmp_path, before, lambda: c.put_cart_cpp(0, *a[:5], std), "std must be finite and not 0")
    fp = a[0].ctypes.data_as(C.POINTER(api.jdaFeatureCpp)); ip = a[1].ctypes.data_as(C.POINTER(C.c_int)); dp = a[2].ctypes.data_as(C.POINTER(C.c_double))
    for args in ((None, ip, dp), (fp, None, dp), (fp, ip, None)):
        assert api.lib.jdaModelPutCartCpp(c.h, 0, *args, a[3], a[4], a[5]) == -1 and "null" in api.last_error()
    assert api.lib.jdaModelPutCartCpp(None, 0, fp, ip, dp, a[3], a[4], a[5]) == -1
    assert api.lib.jdaModelCloseStageCpp(None, None) == -1 and api.lib.jdaCascadorSerializeToCpp(None, b"x") == -1
    assert api.lib.jdaCascadorSerializeToCpp(c.h, None) == -1 and api.lib.jdaModelStatusCpp(None, None, None) == -1
    assert _blob(c, tmp_path, "after.model") == before and c.model_status_cpp() == (0, -1)
    # at (0, 1): behind, ahead, close before K - 1, NULL w
    _grow_to(c, ref, src, 0, 1)
    before = _blob(c, tmp_path)
    _refused(c, tmp_path, before, lambda: c.put_cart_cpp(0, *a), "neither appended nor replaced")
    _refused(c, tmp_path, before, lambda: c.put_cart_cpp(3, *a), "neither appended nor replaced")
    _refused(c, tmp_path, before, lambda: c.close_stage_cpp(src.w[0]), "2 of its 3 carts")
    # at (0, K - 1): no file, no further cart; a NULL w closes nothing
    c.put_cart_cpp(2, *model_ref.cart_of(src, 0, 2)); ref.put(2, *model_ref.cart_of(src, 0, 2))
    _refused(c, tmp_path, None, lambda: c.serialize_to_cpp(str(tmp_path / "no.model")), "not closed")
    assert not (tmp_path / "no.model").exists()
    _refused(c, tmp_path, None, lambda: c.put_cart_cpp(3, *a), "neither appended nor replaced")
    assert api.lib.jdaModelCloseStageCpp(c.h, None) == -1 and "null w" in api.last_error() and c.model_status_cpp() == (0, 2)
    c.close_stage_cpp(src.w[0]); ref.close(src.w[0])
    assert _blob(c, tmp_path) == ref.tobytes()              # ... and none of the refusals at (0, 2) touched anything
    # complete
    _grow_to_complete = [(1, k) for k in range(K)]
    for t, k in _grow_to_complete:
        c.put_cart_cpp(k, *model_ref.cart_of(src, t, k))
    c.close_stage_cpp(src.w[1])
    before = _blob(c, tmp_path)
    assert before == src.tobytes(8)
    _refused(c, tmp_path, before, lambda: c.put_cart_cpp(0, *a), "complete")
    _refused(c, tmp_path, before, lambda: c.close_stage_cpp(src.w[0]), "complete")
    c.close()


def test_an_f32_cascador_does_not_grow(built, tmp_path, model_file):
    from jda_amd import api
    p, m = model_file((T, K, L, D), 4, seed=3)
    c = api.Cascador(p)
    a = model_ref.cart_of(m, 0, 0)
    for call in (lambda: c.put_cart_cpp(0, *a), lambda: c.close_stage_cpp(m.w[0]), lambda: c.serialize_to_cpp(str(tmp_path / "x.model"))):
        with pytest.raises(api.JdaError, match="f32 file"):
            call()
    assert c.model_status_cpp() == (T + 1, -1)              # the float file's own convention, as found
    q = str(tmp_path / "same.model")
    c.serialize(q)
    assert open(q, "rb").read() == open(p, "rb").read()     # jdaCascadorSerializeTo is what it was
    c.close()


def test_a_loaded_snapshot_resumes(built, tmp_path):
    from jda_amd import api
    src = _source(seed=9)
    ref = model_ref.GrowModel(T, K, L, D, src.mean_shape)
    for k in range(2):
        ref.put(k, *model_ref.cart_of(src, 0, k))
    c = api.Cascador(ref.save(str(tmp_path / "snap.model")))
    assert c.model_status_cpp() == (0, 1)
    _grow_to_rest = [(0, 2)]
    for t, k in _grow_to_rest:
        a = model_ref.cart_of(src, t, k)
        c.put_cart_cpp(k, *a); ref.put(k, *a)
    c.close_stage_cpp(src.w[0]); ref.close(src.w[0])
    assert _blob(c, tmp_path) == ref.tobytes()
    c.close()
    # a snapshot at (s, K - 1) -- the loader accepts the header -- closes but does not serialize
    ref2 = model_ref.GrowModel(T, K, L, D, src.mean_shape)
    for k in range(K):
        ref2.put(k, *model_ref.cart_of(src, 0, k))
    c2 = api.Cascador(ref2.save(str(tmp_path / "snap2.model")))
    assert c2.model_status_cpp() == (0, K - 1)
    with pytest.raises(api.JdaError, match="not closed"):
        c2.serialize_to_cpp(str(tmp_path / "no.model"))
    c2.close_stage_cpp(src.w[0]); ref2.close(src.w[0])
    assert _blob(c2, tmp_path) == ref2.tobytes()
    c2.close()


def test_replacing_the_last_cart_changes_only_its_bytes(built, tmp_path):
    src, other = _source(seed=5), _source(seed=6)
    c, ref = _pair(src)
    _grow_to(c, ref, src, 1, 1)
    before = _blob(c, tmp_path)
    c.put_cart_cpp(1, *model_ref.cart_of(other, 1, 1))
    assert c.model_status_cpp() == (1, 1)
    after = _blob(c, tmp_path)
    node_n, leaf_n = (1 << (D - 1)) - 1, 1 << (D - 1)
    cart_bytes = node_n * 48 + leaf_n * 8 + 24
    stage_bytes = K * cart_bytes + K * leaf_n * 2 * L * 8
    lo = 28 + 2 * L * 8 + stage_bytes + cart_bytes
    assert len(after) == len(before) and after[:lo] == before[:lo] and after[lo + cart_bytes:] == before[lo + cart_bytes:]
    assert after[lo:lo + cart_bytes] != before[lo:lo + cart_bytes]
    ref.put(1, *model_ref.cart_of(other, 1, 1))
    assert after == ref.tobytes()
    c.close()


def test_multi_scale_follows_the_model(built):
    """jdaCascadorInfo's multi_scale is cached in the host model: a put of a cart with a scale != 0 node sets it, the replace
    that takes the node away clears it."""
    from jda_amd import api
    src = _source()
    c, _ = _pair(src)
    info = api.jdaModelInfo()

    def multi():
        assert api.lib.jdaCascadorInfo(c.h, C.byref(info)) == 0
        return info.multi_scale

    assert multi() == 0
    a = model_ref.cart_of(src, 0, 0)
    c.put_cart_cpp(0, *a)
    assert multi() == 0
    f = a[0].copy(); f["scale"][2] = 2
    c.put_cart_cpp(1, f, *a[1:])
    assert multi() == 1 and c.multi_scale
    c.put_cart_cpp(1, *a)
    assert multi() == 0 and not c.multi_scale
    c.close()
