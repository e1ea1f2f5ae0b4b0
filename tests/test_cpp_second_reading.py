"""Dialect CPP (the reference's fp64 src/jda path) cannot be pinned in this image: src/jda needs OpenCV, jsmnpp and liblinear.
What CAN be done: a second restatement written independently from the reference's C++ (oracle/cpp_reading2.py, plain Python
on IEEE doubles) must agree BIT FOR BIT with oracle/jda_oracle.c's dialect CPP -- per window (reject length, score, leaf-path
hash, shape) and per image (rects, scores, relocated shapes after the multimap NMS).  Agreement narrows the room for a
misreading of cascador.cpp:166-211 / cart.cpp:392-404 / data.cpp:18-58 / btcart.cpp:407-424 / cascador.cpp:310-477; it
does not pin the dialect (module docstring of cpp_reading2.py).  CPU only."""
import numpy as np
import pytest

from oracle import cpp_reading2 as r2
from oracle.pyoracle import Oracle


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def _image(w, h, seed):
    from jda_amd import synth
    return synth.make_frames(1, w, h, seed=seed)[0]


CASES = [((3, 20, 5, 4), dict(seed=3, cart_th=-1.0, norm_every=5), (64, 52)),
         ((2, 8, 5, 3), dict(seed=1, cart_th=-0.5), (47, 61)),
         ((2, 6, 4, 6), dict(seed=2, cart_th=-2.0, norm_every=2), (40, 40)),
         ((1, 4, 3, 2), dict(seed=5, cart_th=-0.2), (33, 25))]


@pytest.mark.parametrize("dims,kw,size", CASES)
def test_two_independent_readings_of_validate_agree_window_by_window(model_file, dims, kw, size):
    p, _ = model_file(dims, 8, **kw)
    img = _image(size[0], size[1], seed=7 + dims[1])
    orc = Oracle(p)
    tr = orc.trace_cpp(img, minimum_size=20, step=5, factor=1.2)
    m = r2.Model2(p)
    assert (m.T, m.K, m.L, m.D) == tuple(dims) and m.stage_idx == m.T and m.cart_idx == -1
    rows = img.tolist()
    wins = r2.windows_method1(size[0], size[1], 20, 5, 1.2)
    assert len(wins) == len(tr["carts_n"]) > 0
    faces = 0
    for i, (x, y, win) in enumerate(wins):
        ok, score, shape, n, h = r2.validate(m, rows, x, y, win, win)
        faces += ok
        assert n == tr["carts_n"][i], (i, x, y, win)
        assert h == tr["path_hash"][i], (i, "leaf path")
        assert _bits([score])[0] == _bits(tr["score"][i:i + 1])[0], (i, score, tr["score"][i])
        assert np.array_equal(_bits(shape), _bits(tr["shapes"][i])), (i, "shape")
    assert 0 < faces < len(wins) or dims[1] <= 4            # (the cases reject some windows and keep some)
    orc.close()


@pytest.mark.parametrize("nms", [True, False])
def test_two_independent_readings_of_detect_agree(model_file, nms):
    dims, kw = (3, 20, 5, 4), dict(seed=3, cart_th=-1.0, norm_every=5)
    p, _ = model_file(dims, 8, **kw)
    img = _image(70, 58, seed=11)
    orc = Oracle(p)
    want = orc.detect_cpp(img, minimum_size=20, step=5, factor=1.2, overlap=0.3, nms=nms)
    m = r2.Model2(p)
    rects, scores, shapes = r2.detect(m, img.tolist(), 20, 5, 1.2, 0.3, nms)
    assert len(rects) == len(want["rects"]) > 0
    assert np.array_equal(np.array(rects, np.int32), want["rects"])
    assert np.array_equal(_bits(scores), _bits(want["scores"]))
    assert np.array_equal(_bits(shapes), _bits(want["shapes"]))
    orc.close()


def test_nms_ties_resolve_the_same_way_in_both_readings(model_file):
    """A constant image: every window of a level sees the same pixels, so whole levels share one score -- the multimap's
    order among equal keys (insertion order, the LAST inserted is picked first) decides which window survives."""
    dims = (2, 8, 5, 3)
    p, _ = model_file(dims, 8, seed=1, cart_th=-1e30)
    img = np.full((50, 58), 117, np.uint8)
    orc = Oracle(p)
    want = orc.detect_cpp(img, minimum_size=20, step=5, factor=1.2, overlap=0.3, nms=True)
    m = r2.Model2(p)
    rects, scores, shapes = r2.detect(m, img.tolist(), 20, 5, 1.2, 0.3, True)
    assert len(set(scores)) == 1 and len(rects) > 1
    assert np.array_equal(np.array(rects, np.int32), want["rects"])
    assert np.array_equal(_bits(scores), _bits(want["scores"]))
    assert np.array_equal(_bits(shapes), _bits(want["shapes"]))
    orc.close()


def test_a_model_still_in_training_runs_its_last_stage_without_regression(model_file, tmp_path):
    """cascador.cpp:198-209: stages [0, current_stage_idx) in full, then carts [0, current_cart_idx] of the stage in
    training with NO shape update -- the header fields decide, in both readings."""
    from jda_amd import synth
    dims = (3, 20, 5, 4)
    mdl = synth.make_model(*dims, seed=3, cart_th=-1.0, norm_every=5)
    p = str(tmp_path / "partial.model")
    mdl.save(p, 8, header_stage=1, header_cart=6)
    img = _image(56, 48, seed=4)
    m = r2.Model2(p)
    assert (m.stage_idx, m.cart_idx) == (1, 6)
    try:
        orc = Oracle(p)
    except Exception:
        pytest.skip("jda_oracle.c takes complete models only")
    tr = orc.trace_cpp(img, minimum_size=20, step=5, factor=1.2)
    rows = img.tolist()
    for i, (x, y, win) in enumerate(r2.windows_method1(56, 48, 20, 5, 1.2)):
        ok, score, shape, n, h = r2.validate(m, rows, x, y, win, win)
        assert n == tr["carts_n"][i] and h == tr["path_hash"][i], i
        assert _bits([score])[0] == _bits(tr["score"][i:i + 1])[0], i
        assert np.array_equal(_bits(shape), _bits(tr["shapes"][i])), i
    orc.close()


def _resize_with(orc):
    """jda_oracle.c's restatement of cv::resize as the second reading's resize(img, dw, dh) (rows of ints in and out): the
    second reading covers everything around the resize, not the resize."""
    def f(img, dw, dh):
        return orc.resize_cv(np.asarray(img, np.uint8), dw, dh).tolist()
    return f


@pytest.mark.parametrize("dims,kw,size", [((3, 20, 5, 4), dict(seed=3, cart_th=-1.0, norm_every=5, multi_scale=True), (64, 52)),
                                           ((2, 8, 5, 3), dict(seed=4, cart_th=-0.5, multi_scale=True), (47, 61))])
def test_multi_scale_models_method_1_which_patch_which_size(model_file, dims, kw, size):
    """detectMultiScale1 hands Validate three ROIs of three images (cascador.cpp:323-353): the half image is
    int(cols / sqrt 2) wide, the quarter image cols / 2; a window's half ROI starts at int(x / sqrt 2) and is int(win / sqrt 2)
    wide -- and a HALF feature scales its offsets by THAT width (data.cpp:37-43).  Both readings must agree on all of it."""
    p, mdl = model_file(dims, 8, **kw)
    assert (mdl.scale != 0).any()
    img = _image(size[0], size[1], seed=21)
    orc = Oracle(p)
    tr = orc.trace_cpp(img, minimum_size=20, step=5, factor=1.2)
    m = r2.Model2(p)
    mine = []
    # (the half / quarter images through the SECOND recollection of cv::resize: nothing of jda_oracle.c on this side)
    rects, scores, shapes = r2.detect(m, img.tolist(), 20, 5, 1.2, 0.3, True, resize=r2.resize_cv2, trace=mine)
    assert len(mine) == len(tr["carts_n"])
    for i, (ok, score, shape, n, h) in enumerate(mine):
        assert n == tr["carts_n"][i] and h == tr["path_hash"][i], i
        assert _bits([score])[0] == _bits(tr["score"][i:i + 1])[0], i
        assert np.array_equal(_bits(shape), _bits(tr["shapes"][i])), i
    want = orc.detect_cpp(img, 20, 5, 1.2, 0.3, True)
    assert len(rects) == len(want["rects"]) > 0
    assert np.array_equal(np.array(rects, np.int32), want["rects"])
    assert np.array_equal(_bits(scores), _bits(want["scores"])) and np.array_equal(_bits(shapes), _bits(want["shapes"]))
    orc.close()


def test_method_0_multi_scale_end_to_end_on_the_second_reading_alone(model_file):
    """Levels AND per-window patches through cpp_reading2.resize_cv2: no line of jda_oracle.c on this side."""
    p, _ = model_file((2, 8, 5, 3), 8, seed=4, cart_th=-0.5, multi_scale=True)
    img = _image(70, 62, seed=13)
    orc = Oracle(p)
    want = orc.detect_cpp_pyramid(img, 48, 5, 1.2, 0.3, True, half_size=36, quarter_size=24)
    rects, scores, shapes = r2.detect_pyramid(r2.Model2(p), img.tolist(), r2.resize_cv2, 48, 36, 24, 5, 1.2, 0.3, True)
    assert len(rects) == len(want["rects"]) > 0
    assert np.array_equal(np.array(rects, np.int32), want["rects"])
    assert np.array_equal(_bits(scores), _bits(want["scores"])) and np.array_equal(_bits(shapes), _bits(want["shapes"]))
    orc.close()


@pytest.mark.parametrize("multi", [False, True])
def test_method_0_the_image_pyramid_around_the_resize(model_file, multi):
    """detectMultiScale / detectSingleScale (cascador.cpp:215-308): fixed 48-pixel windows on an image that is resized level
    after level FROM THE PREVIOUS LEVEL, rects scaled back with `int *= double` truncation, the scale a running product."""
    dims = (3, 20, 5, 4)
    p, _ = model_file(dims, 8, seed=3, cart_th=-1.0, norm_every=5, multi_scale=multi)
    img = _image(150, 121, seed=9)
    orc = Oracle(p)
    m = r2.Model2(p)
    for nms in (True, False):
        want = orc.detect_cpp_pyramid(img, 48, 5, 1.2, 0.3, nms, half_size=36 if multi else 0, quarter_size=24 if multi else 0)
        # (single-scale: every resize through the second recollection -- the levels; multi-scale: 1,900 patch resizes in
        # pure Python would take a minute, so the first recollection serves them and a smaller image below goes all the way)
        rects, scores, shapes = r2.detect_pyramid(m, img.tolist(), _resize_with(orc) if multi else r2.resize_cv2, 48, 36, 24, 5, 1.2, 0.3, nms)
        assert len(rects) == len(want["rects"]) > 0
        assert np.array_equal(np.array(rects, np.int32), want["rects"])
        assert np.array_equal(_bits(scores), _bits(want["scores"])) and np.array_equal(_bits(shapes), _bits(want["shapes"]))
    orc.close()


@pytest.mark.parametrize("src,dst", [((64, 48), (45, 33)), ((64, 48), (32, 24)), ((47, 61), (33, 43)), ((150, 121), (125, 100)),
                                     ((48, 48), (36, 36)), ((48, 48), (24, 24)), ((48, 48), (48, 48)), ((31, 20), (40, 29)),
                                     ((125, 100), (104, 83)), ((20, 20), (14, 14)), ((33, 25), (16, 12)), ((101, 77), (50, 38))])
def test_two_recollections_of_cv_resize_agree(model_file, src, dst):
    """cv::resize (8-bit, INTER_LINEAR) twice from memory of OpenCV's imgwarp.cpp -- jda_oracle.c's orc_resize_cv and
    cpp_reading2.resize_cv2: float coordinates, border rules, 11-bit coefficients rounded half to even, the fixed-point vertical
    pass, the exact-2x switch to the area average.  Equal on down- and up-scaling, the sizes method 1 and method 0 use, and the
    identity.  Two memories of a library that is not here: still not a pin."""
    p, _ = model_file((1, 4, 3, 2), 8, seed=5)
    orc = Oracle(p)
    img = _image(src[0], src[1], seed=src[0] * 7 + dst[0])
    a = orc.resize_cv(img, dst[0], dst[1])
    b = np.array(r2.resize_cv2(img.tolist(), dst[0], dst[1]), np.uint8)
    assert a.shape == b.shape == (dst[1], dst[0])
    assert np.array_equal(a, b), (np.argwhere(a != b)[:5], a[a != b][:5], b[a != b][:5])
    orc.close()


@pytest.mark.parametrize("hdr", [None, (2, 7)])
def test_similarity_transform_on_both_readings(model_file, tmp_path, hdr):
    """face.similarity_transform: STParameter::Calc per stage from the window's current shape (data.cpp:64-114,
    cascador.cpp:180), applied to every feature offset (data.cpp:33-34) and to the stage's delta shape (btcart.cpp:422).  A
    snapshot's stage in training walks with the PREVIOUS stage's parameter (cascador.cpp:198-200: stp_mc is not recomputed)."""
    from jda_amd import synth
    dims = (3, 20, 5, 4)
    mdl = synth.make_model(*dims, seed=3, cart_th=-1.0, norm_every=5, w_sigma=2e-2)
    p = str(tmp_path / "st.model")
    if hdr:
        mdl.save(p, 8, header_stage=hdr[0], header_cart=hdr[1])
    else:
        mdl.save(p, 8)
    img = _image(64, 52, seed=17)
    orc = Oracle(p)
    orc.set_similarity_transform(True)
    try:
        tr = orc.trace_cpp(img, minimum_size=20, step=5, factor=1.2)
        want = orc.detect_cpp(img, 20, 5, 1.2, 0.3, True)
    finally:
        orc.set_similarity_transform(False)
    m = r2.Model2(p)
    mine = []
    rects, scores, shapes = r2.detect(m, img.tolist(), 20, 5, 1.2, 0.3, True, trace=mine, similarity=True)
    later = 0
    for i, (ok, score, shape, n, h) in enumerate(mine):
        assert n == tr["carts_n"][i] and h == tr["path_hash"][i], i
        assert _bits([score])[0] == _bits(tr["score"][i:i + 1])[0], i
        assert np.array_equal(_bits(shape), _bits(tr["shapes"][i])), i
        later += n > dims[1]
    assert later > 0                                        # (windows that reached a stage whose parameter is not the stage-0 one)
    assert len(rects) == len(want["rects"]) > 0
    assert np.array_equal(np.array(rects, np.int32), want["rects"])
    assert np.array_equal(_bits(scores), _bits(want["scores"])) and np.array_equal(_bits(shapes), _bits(want["shapes"]))
    orc.close()


def test_randomised_cases_agree():
    """tools/fuzz_second_reading.py for a few seconds with a fixed seed (r06: 17,150 cases / 2.97 M windows over six seeds)."""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, os.path.join(root, "tools", "fuzz_second_reading.py"), "11", "6"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "the two readings agree" in r.stdout, (r.stdout[-2000:], r.stderr[-4000:])


# cart thresholds of the three regimes: every window rejected by its first cart, a mix, every window a face
REGIMES = {"reject_all": 1e30, "mix": -1.0, "pass_all": -3.0e38}


def _counter_model(tmp_path, kind, regime):
    """(path, (stage_idx, cart_idx)) of a small model: single-scale, multi-scale or a trainer snapshot."""
    from jda_amd import synth
    dims = (3, 20, 5, 4) if kind != "multi" else (2, 8, 5, 3)
    mdl = synth.make_model(*dims, seed=3, cart_th=REGIMES[regime], norm_every=5, multi_scale=kind == "multi")
    p = str(tmp_path / ("%s_%s.model" % (kind, regime)))
    hdr = {"snap_1_6": (1, 6), "snap_0_-1": (0, -1)}.get(kind)
    if hdr:
        mdl.save(p, 8, header_stage=hdr[0], header_cart=hdr[1])
    else:
        mdl.save(p, 8)
    return p, hdr or (dims[0], -1)


def _check_regime(st, regime, windows):
    assert st["patch_n"] == windows > 0
    assert st["face_patch_n"] + st["nonface_patch_n"] == st["patch_n"]
    if regime == "reject_all":
        assert st["face_patch_n"] == 0 and st["cart_gothrough_n"] == st["cart_total_n"] == windows
        assert not any(st["stage_done_n"])
    elif regime == "pass_all":
        assert st["nonface_patch_n"] == 0 and st["cart_gothrough_n"] == 0
    else:
        assert 0 < st["face_patch_n"] < st["patch_n"]


@pytest.mark.parametrize("regime", sorted(REGIMES))
@pytest.mark.parametrize("kind", ["single", "multi", "snap_1_6", "snap_0_-1"])
def test_both_readings_count_the_same_work(tmp_path, kind, regime):
    """DetectionStatisic (include/jda/cascador.hpp:14-25) plus cart_total_n and stage_done_n, counted by jda_oracle.c's walks
    (orc_detect_cpp, orc_detect_cpp_pyramid_ms) and by the second reading: equal on method 1 and method 0, single- and
    multi-scale models and trainer snapshots, in all three threshold regimes.  These are the numbers the GPU tests hold the
    product's jdaStats to (tests/test_cpp_stats.py)."""
    p, (s_idx, c_idx) = _counter_model(tmp_path, kind, regime)
    orc = Oracle(p)
    m = r2.Model2(p)
    T, K = m.T, m.K
    multi = kind == "multi"
    resize = _resize_with(orc) if multi else None
    regime = "pass_all" if kind == "snap_0_-1" else regime      # (Validate runs no cart of (0, -1): every window is a face)
    keys = ("patch_n", "face_patch_n", "nonface_patch_n", "cart_gothrough_n", "cart_total_n")
    # method 1
    img = _image(64, 52, seed=17)
    want = orc.detect_cpp(img, 20, 5, 1.2, 0.3, True, stats=True)["stats"]
    mine = r2.new_stats(T)
    r2.detect(m, img.tolist(), 20, 5, 1.2, 0.3, True, resize=resize, stats=mine)
    for k in keys:
        assert mine[k] == want[k], ("method 1", k, mine[k], want[k])
    assert mine["stage_done_n"] == want["stage_done_n"][:T] and not any(want["stage_done_n"][T:])
    _check_regime(want, regime, len(r2.windows_method1(64, 52, 20, 5, 1.2)))
    # the walk stops where Validate stops: a face ran every cart of the stages it runs, no regression in the stage in training
    ran = (s_idx * K + c_idx + 1) if s_idx < T else T * K
    assert want["cart_total_n"] == want["cart_gothrough_n"] + want["face_patch_n"] * ran
    assert not any(want["stage_done_n"][min(s_idx, T):])
    # method 0
    img0 = _image(70, 62, seed=13)
    want0 = orc.detect_cpp_pyramid(img0, 48, 5, 1.2, 0.3, True, half_size=36 if multi else 0, quarter_size=24 if multi else 0,
                                   stats=True)
    mine0 = r2.new_stats(T)
    r2.detect_pyramid(m, img0.tolist(), _resize_with(orc) if multi else r2.resize_cv2, 48, 36, 24, 5, 1.2, 0.3, True, stats=mine0)
    for k in keys:
        assert mine0[k] == want0["stats"][k], ("method 0", k, mine0[k], want0["stats"][k])
    assert mine0["stage_done_n"] == want0["stats"]["stage_done_n"][:T]
    _check_regime(want0["stats"], regime, want0["windows"])
    orc.close()
