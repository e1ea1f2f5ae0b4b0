"""Frames larger than the faces need (include/jda.h), without a GPU: jdaReduceSize, jdaPackGrayReduced against the restatement of
tests/reduce_ref.py -- every factor, format and orientation, every block sum --, and jdaReduceBack -- boxes, landmarks, pair
exchange, refusals.  Every comparison is exact."""
import ctypes as C

import numpy as np
import pytest

import pack_ref as pr
import reduce_ref as rr
import turn_ref as tr
from conftest import same
from mining_ref import transform


def sizes_of(f):
    """Rectangle widths and heights: one block, one and a dropped column, two less one, a lane's four pixels, four and three
    dropped, 16, 16 and one dropped, more than a tile."""
    return [f, f + 1, 2 * f - 1, 4 * f, 4 * f + 3, 16 * f, 16 * f + 1, 65 * f + 2]


@pytest.fixture(scope="module")
def api(built):
    from jda_amd import api
    return api


def _eq(got, want):
    assert got.shape == want.shape and got.dtype == np.uint8 and np.array_equal(got, want)


def test_reduce_size(api):
    for f in rr.FACTORS:
        for t in tr.ORIENTS:
            for w, h in ((1920, 1080), (641, 479), (f, 8 * f + 7), (0, 5)):
                want = (h // f, w // f) if t in tr.SWAP else (w // f, h // f)
                assert api.reduce_size(w, h, f, t) == want == rr.size(w, h, f, t)
    assert api.reduce_size(640, 480, 1, 3) == api.orient_size(640, 480, 3)
    rw, rh = C.c_int(7), C.c_int(7)
    for args, word in (((4, 3, 0, 0), "factor 0"), ((4, 3, 9, 0), "factor 9"), ((4, 3, -1, 0), "factor -1"), ((4, 3, 2, 8), "orientation 8"),
                       ((4, 3, 2, -1), "orientation -1"), ((-4, 3, 2, 0), "-4 x 3"), ((4, -3, 2, 0), "4 x -3")):
        assert api.lib.jdaReduceSize(*args, C.byref(rw), C.byref(rh)) == -1 and word in api.last_error(), args
        assert "jdaReduceSize" in api.last_error()
    assert api.lib.jdaReduceSize(4, 3, 2, 1, None, C.byref(rh)) == -1 and api.lib.jdaReduceSize(4, 3, 2, 1, C.byref(rw), None) == -1
    assert (rw.value, rh.value) == (7, 7)


# ---- jdaPackGrayReduced -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("fmt", pr.FORMATS)
@pytest.mark.parametrize("f", rr.FACTORS)
def test_shapes(api, f, fmt):
    """Every orientation in one call; width k meets height (k + t) % 8, so over the eight orientations every width meets every
    height."""
    rng = np.random.default_rng(8 * fmt + f)
    z = sizes_of(f)
    views, ts = [], []
    for t in tr.ORIENTS:
        for k, w in enumerate(z):
            h = z[(k + t) % 8]
            views.append(pr.pitched(rng, h, w, fmt, (w + h) % 4, (3 * w + h) % 16)[1]); ts.append(t)
    got = api.pack_gray_reduced(views, fmt, f, ts)
    for g, v, t in zip(got, views, ts):
        _eq(g, rr.reduce(v, fmt, f, t))
        assert g.shape[::-1] == api.reduce_size(v.shape[1], v.shape[0], f, t)
    for g, v in zip(api.pack_gray_reduced(views[:8], fmt, f), views[:8]):       # orients None: upright
        _eq(g, rr.reduce(v, fmt, f))


@pytest.mark.parametrize("name", sorted(pr.RECTS))
def test_rectangles(api, name):
    """pack_ref.RECTS on a 37 x 21 image: where the rectangle holds a block it is reduced, where not it is refused."""
    rng = np.random.default_rng(7)
    rect = pr.RECTS[name](37, 21)
    for fmt in pr.FORMATS:
        for f in rr.FACTORS:
            for t in (0, 1, 4, 5):
                v = pr.pitched(rng, 21, 37, fmt, 5, 1)[1]
                if rect[2] >= f and rect[3] >= f:
                    _eq(api.pack_gray_reduced([v], fmt, f, t, [rect])[0], rr.reduce(v, fmt, f, t, rect))
                else:
                    with pytest.raises(api.JdaError, match="image 0.*%d x %d.*factor %d" % (rect[2], rect[3], f)):
                        api.pack_gray_reduced([v], fmt, f, t, [rect])


def test_factor_1_is_pack_gray_oriented(api):
    rng = np.random.default_rng(2)
    views = [pr.pitched(rng, 1 + 7 * i, 3 + 11 * i, pr.FORMATS[i % 5], i, i)[1] for i in range(16)]
    fmts = [pr.FORMATS[i % 5] for i in range(16)]
    rects = [None if i % 2 else (1, 0, 2 + 5 * i, 1 + 3 * i) for i in range(16)]
    ts = [i % 8 for i in range(16)]
    for a, b in zip(api.pack_gray_reduced(views, fmts, 1, ts, rects), api.pack_gray_oriented(views, fmts, ts, rects)):
        _eq(a, b)
    for a, b in zip(api.pack_gray_reduced(views, fmts, 1, None, rects), api.pack_gray(views, fmts, rects)):
        _eq(a, b)
    assert api.lib.jdaPackGrayReduced(None, None, None, 0, None, None) == 0    # touches nothing


def test_factor_2_is_resize_cv_to_half(api, model_file):
    """(S + 2) >> 2 is the area path cv::resize takes at exactly 2x, as the project's restatement of cv::resize has it."""
    from oracle.pyoracle import Oracle
    p, _ = model_file((2, 8, 5, 3), 8)
    o = Oracle(p)
    rng = np.random.default_rng(4)
    for w, h in ((2, 2), (64, 48), (130, 98), (6, 200)):
        img = rng.integers(0, 256, (h, w), dtype=np.uint8)
        _eq(api.pack_gray_reduced([img], "gray8", 2)[0], o.resize_cv(img, w // 2, h // 2))


@pytest.mark.parametrize("f", rr.FACTORS)
def test_colour_reduces_like_its_gray_image(api, f):
    """Rounding happens per pixel first: reducing a colour image is reducing its jdaPackGray image."""
    rng = np.random.default_rng(f)
    for fmt in pr.FORMATS[1:]:
        v = pr.pitched(rng, 9 * f + 2, 11 * f + 1, fmt, 3, 2)[1]
        gray = api.pack_gray([v], fmt)[0]
        for t in (0, 3, 6):
            _eq(api.pack_gray_reduced([v], fmt, f, t)[0], api.pack_gray_reduced([gray], "gray8", f, t)[0])


@pytest.mark.parametrize("f", rr.FACTORS)
def test_reduce_then_turn_is_turn_then_reduce(api, f):
    """Where w and h are multiples of f no column or row is dropped, and the block means of the turned image are the turned
    block means."""
    rng = np.random.default_rng(10 + f)
    img = rng.integers(0, 256, (6 * f, 9 * f), dtype=np.uint8)
    for t in tr.ORIENTS:
        _eq(api.pack_gray_reduced([img], "gray8", f, t)[0], rr.block_means(np.ascontiguousarray(transform(img, t)), f))


@pytest.mark.parametrize("f", rr.FACTORS)
def test_every_block_sum(api, f):
    """One gray image whose blocks take every sum 0 .. 255 f^2: the division is exact for each."""
    img, sums = rr.block_sum_image(f)
    assert set(range(255 * f * f + 1)) <= set(sums.ravel().tolist())
    if f == 8:
        assert img.shape == (1024, 1024)
    want = ((sums + f * f // 2) // (f * f)).astype(np.uint8)
    _eq(api.pack_gray_reduced([img], "gray8", f)[0], want)
    _eq(rr.reduce(img, pr.GRAY8, f), want)


def test_pack_refusals_name_the_image_and_leave_dst_alone(api):
    from test_pack_host import _px, refusals
    rng = np.random.default_rng(3)
    a = rng.integers(0, 256, (6, 8, 3), dtype=np.uint8)
    b = rng.integers(0, 256, (6, 8, 3), dtype=np.uint8)
    # jdaPackGray's own, at factor 1 (the destinations are the 48 bytes they are there)
    cases = [(what, px, offs, n, words, (1, 1), (1, 4)) for what, px, offs, n, words in refusals(api, a, b)]
    ok = [_px(api, a, pr.BGR24), _px(api, b, pr.BGR24)]
    cases += [("orientation 8", ok, [64, 112], 2, ["image 1", "orientation 8"], (2, 2), (0, 8)),
              ("factor 0", ok, [64, 112], 2, ["image 1", "factor 0"], (2, 0), (0, 1)), ("factor 9", ok, [64, 112], 2, ["image 0", "factor 9"], (9, 2), (0, 1)),
              ("factor -3", ok, [64, 112], 2, ["image 1", "factor -3"], (2, -3), (0, 1)),
              ("h below f", ok, [64, 112], 2, ["image 1", "8 x 6", "factor 7"], (2, 7), (0, 1)),
              ("w below f", [ok[0], _px(api, b, pr.BGR24, (1, 0, 4, 6))], [64, 112], 2, ["image 1", "4 x 6", "factor 5"], (2, 5), (0, 1)),
              # 8 x 6 by 2 is 4 x 3 = 12 bytes: one byte less than needed still overlaps
              ("reduced destinations overlap", ok, [64, 75], 2, ["image 0", "image 1", "12 bytes", "overlap"], (2, 2), (1, 3))]
    for what, px, offs, n, words, fs, ts in cases:
        dst = np.full(256, 0xA5, np.uint8)
        arr = (api.jdaPixels * len(px))(*px)
        rc = api.lib.jdaPackGrayReduced(arr, (C.c_int * 2)(*fs), (C.c_int * 2)(*ts), n, dst.ctypes.data, (C.c_size_t * len(offs))(*offs))
        assert rc == -1, what
        for w in words:
            assert w in api.last_error(), (what, api.last_error())
        assert "jdaPackGrayReduced" in api.last_error() and (dst == 0xA5).all(), what
    arr = (api.jdaPixels * 2)(*ok)
    o, fs, ts = (C.c_size_t * 2)(64, 76), (C.c_int * 2)(2, 2), (C.c_int * 2)(1, 4)
    dst = np.full(256, 0xA5, np.uint8)
    for args in ((None, fs, ts, 2, dst.ctypes.data, o), (arr, None, ts, 2, dst.ctypes.data, o), (arr, fs, ts, 2, None, o), (arr, fs, ts, 2, dst.ctypes.data, None)):
        assert api.lib.jdaPackGrayReduced(*args) == -1 and "null" in api.last_error()
    assert (dst == 0xA5).all()
    # ... and right behind each other they are taken; NULL orients is every image upright
    assert api.lib.jdaPackGrayReduced(arr, fs, ts, 2, dst.ctypes.data, o) == 0
    assert np.array_equal(dst[64:76].reshape(4, 3), rr.reduce(a, pr.BGR24, 2, 1)) and np.array_equal(dst[76:88].reshape(3, 4), rr.reduce(b, pr.BGR24, 2, 4))
    assert (dst[:64] == 0xA5).all() and (dst[88:] == 0xA5).all()
    assert api.lib.jdaPackGrayReduced(arr, fs, None, 2, dst.ctypes.data, o) == 0
    assert np.array_equal(dst[64:76].reshape(3, 4), rr.reduce(a, pr.BGR24, 2)) and np.array_equal(dst[76:88].reshape(3, 4), rr.reduce(b, pr.BGR24, 2))


# ---- jdaReduceBack ----------------------------------------------------------------------------------------------------------

W, H = 61, 47


def rect_of(f):
    """A rectangle inside the larger image with a dropped column and a dropped row (none at factor 1): 5 x 4 blocks."""
    return (4, 3, 5 * f + min(f - 1, 2), 4 * f + min(f - 1, 1))


@pytest.fixture(scope="module")
def image():
    return np.random.default_rng(1).integers(0, 256, (H, W), dtype=np.uint8)


def _boxes(tw, th):
    """(x, y, w, h) in a tw x th turned rectangle: sizes 1, 2, 7 (clipped to the image: non-square then) and the whole image."""
    out = [(0, 0, 1, 1), (tw - 1, th - 1, 1, 1), (1, 2, 2, 2), (tw - 2, 0, 2, 2), (0, 0, min(7, tw), min(7, th)), (0, 0, tw, th)]
    out += [(1, 0, 3, 4), (tw - 4, th - 2, 4, 2), (0, 3, tw, 1), (2, 0, 1, th), (0, 0, 4, 4)]
    return out


@pytest.mark.parametrize("t", tr.ORIENTS)
@pytest.mark.parametrize("f", rr.FACTORS)
def test_boxes_land_on_the_same_pixels(api, image, f, t):
    """The source pixels under a mapped box, reduced and turned, are the reduced image's pixels under the box."""
    for rect in (rect_of(f), None):
        r = tr.rect_of(image, rect)
        reduced = rr.reduce(image, pr.GRAY8, f, t, rect)
        th, tw = reduced.shape
        for box_ints in (3, 4):
            boxes = [b for b in _boxes(tw, th) if box_ints == 4 or b[2] == b[3]]
            assert len(boxes) >= 5
            arr = np.array([b[:box_ints] for b in boxes], np.int32)
            got, none = api.reduce_back([image], "gray8", f, t, [0] * len(boxes), boxes=arr, rects=[rect])
            assert none is None and got.dtype == np.int32 and got.shape == arr.shape
            for b, g in zip(boxes, got):
                assert tuple(g) == rr.back_box(b[:box_ints], f, t, r), (b, g)
                x, y, bw = int(g[0]), int(g[1]), int(g[2])
                bh = int(g[3]) if box_ints == 4 else bw
                assert r[0] <= x and x + bw <= r[0] + r[2] and r[1] <= y and y + bh <= r[1] + r[3]
                under = transform(rr.block_means(image[y:y + bh, x:x + bw], f), t)
                assert np.array_equal(under, reduced[b[1]:b[1] + b[3], b[0]:b[0] + b[2]]), (f, t, b, g)


@pytest.mark.parametrize("real", [np.float32, np.float64])
@pytest.mark.parametrize("f", rr.FACTORS)
def test_landmarks_land_on_the_centre_of_the_right_block(api, f, real):
    """A landmark on an integer reduced pixel lands on i f + (f - 1) / 2 of the block that pixel is the mean of: the block is
    found through an image whose every block has its own value."""
    rect = rect_of(f)
    rx, ry, w, h = rect
    img = np.zeros((H, W), np.uint8)
    ids = np.arange(1, 21, dtype=np.uint8).reshape(4, 5)
    img[ry:ry + 4 * f, rx:rx + 5 * f] = np.kron(ids, np.ones((f, f), np.uint8))
    for t in tr.ORIENTS:
        reduced = api.pack_gray_reduced([img], "gray8", f, t, [rect])[0]
        th, tw = reduced.shape
        pts = [(u, v) for v in range(th) for u in range(tw)]
        lm = np.array(pts, real).reshape(1, -1)
        _, got = api.reduce_back([img], "gray8", f, t, [0], landmarks=lm, rects=[rect])
        assert got.dtype == real and got.shape == lm.shape
        for (u, v), (x, y) in zip(pts, got.reshape(-1, 2)):
            j, i = np.argwhere(ids == reduced[v, u])[0]
            assert x == rx + i * f + (f - 1) / 2 and y == ry + j * f + (f - 1) / 2, (f, t, u, v, x, y)
        # ... and between pixel centres, to the bit, against the restatement
        rng = np.random.default_rng(t)
        frac = rng.uniform(-3, 20, (4, 10)).astype(real)
        _, got = api.reduce_back([img] * 2, "gray8", [f, 1], [t, 0], [0, 1, 0, 1], landmarks=frac, rects=[rect, rect])
        for k in range(4):
            want = rr.back_landmarks(frac[k], f if k % 2 == 0 else 1, t if k % 2 == 0 else 0, rect)
            assert same(got[k], want), (f, t, k)


def test_pairs_are_exchanged_for_mirrors_only_and_sequentially(api, image):
    L = 5
    lm = np.arange(2 * L, dtype=np.float64).reshape(1, -1) / 4
    left, right = [0, 1, 0], [3, 4, 1]                   # landmark 0 and 1 are named twice
    rect = rect_of(3)
    for t in tr.ORIENTS:
        _, plain = api.reduce_back([image], "gray8", 3, t, [0], landmarks=lm, rects=[rect])
        _, got = api.reduce_back([image], "gray8", 3, t, [0], landmarks=lm, rects=[rect], left=left, right=right)
        want = plain.reshape(L, 2).copy()
        if t in tr.MIRROR:
            for a, b in zip(left, right):
                want[[a, b]] = want[[b, a]]
            assert not np.array_equal(want, plain.reshape(L, 2))
        assert np.array_equal(got.reshape(L, 2), want), t
        assert same(got[0], rr.back_landmarks(lm[0], 3, t, rect, left, right))


def test_factor_1_is_orient_back(api, image):
    rng = np.random.default_rng(9)
    rect = (4, 3, 11, 9)
    boxes = np.array([(1, 2, 3, 2), (0, 0, 9, 9), (4, 5, 1, 1), (2, 2, 5, 6)], np.int32)
    for real in (np.float32, np.float64):
        lm = rng.uniform(-3, 20, (4, 10)).astype(real)
        lm[0, :4] = (0.0, -0.0, 10.0, 8.0)
        for t in tr.ORIENTS:
            for rects in ([rect, None], [None, rect]):
                a = api.reduce_back([image] * 2, "gray8", 1, [t, 7 - t], [0, 1, 1, 0], boxes, lm, rects, [0, 2], [1, 4])
                b = api.orient_back([image] * 2, "gray8", [t, 7 - t], [0, 1, 1, 0], boxes, lm, rects, [0, 2], [1, 4])
                assert same(a[0], b[0]) and same(a[1], b[1]), (real, t)
    # the detect-results form
    c = [dict(bboxes=np.array([[1, 2, 3]], np.int32), scores=np.array([0.5], np.float32), shapes=np.array([[1, 2, 3, 4]], np.float32)), None]
    a, b = api.reduce_back([image] * 2, "gray8", 1, [1, 2], c, rects=[rect, None]), api.orient_back([image] * 2, "gray8", [1, 2], c, rects=[rect, None])
    assert a[1] is None and b[1] is None and all(same(a[0][k], b[0][k]) for k in ("bboxes", "scores", "shapes"))


def test_detect_results_form(api, image):
    """One detect result per image (None: no face), either dialect's."""
    rect = rect_of(3)
    c = [dict(bboxes=np.array([[1, 2, 2]], np.int32), scores=np.array([0.5], np.float32), shapes=np.array([[1, 2, 3, 4]], np.float32)), None]
    got = api.reduce_back([image] * 2, "gray8", [3, 2], [1, 2], c, rects=[rect, None])
    assert got[1] is None and np.array_equal(got[0]["scores"], c[0]["scores"]) and got[0]["shapes"].dtype == np.float32
    assert tuple(got[0]["bboxes"][0]) == rr.back_box((1, 2, 2), 3, 1, rect)
    assert same(got[0]["shapes"][0], rr.back_landmarks(c[0]["shapes"][0], 3, 1, rect))
    assert np.array_equal(c[0]["bboxes"], [[1, 2, 2]])                       # the caller's results are not touched
    d = [dict(rects=np.zeros((0, 4), np.int32), scores=np.zeros(0), shapes=np.zeros((0, 4))),
         dict(rects=np.array([[0, 1, 2, 3], [1, 1, 1, 1]], np.int32), scores=np.array([1., 2.]), shapes=np.array([[0, 0, 1, 1], [2, 2, 3, 3]], np.float64))]
    got = api.reduce_back([image] * 2, "gray8", [4, 5], [4, 7], d)
    assert len(got[0]["scores"]) == 0 and got[1]["shapes"].dtype == np.float64
    for k in range(2):
        assert tuple(got[1]["rects"][k]) == rr.back_box(tuple(d[1]["rects"][k]), 5, 7, (0, 0, W, H))
        assert same(got[1]["shapes"][k], rr.back_landmarks(d[1]["shapes"][k], 5, 7, (0, 0, W, H)))
    up = api.reduce_back([image] * 2, "gray8", [4, 5], None, d)              # orients None: upright
    assert tuple(up[1]["rects"][0]) == rr.back_box((0, 1, 2, 3), 5, 0, (0, 0, W, H))


def test_back_refusals_name_the_index_and_write_nothing(api, image):
    from test_pack_host import _px
    ip = C.POINTER(C.c_int)
    rect = (5, 3, 11, 9)
    good = dict(px=[_px(api, image, pr.GRAY8, rect), _px(api, image, pr.GRAY8)], factors=[3, 2], orients=[1, 4], n_images=2, face_image=[0, 1, 1],
                n_faces=3, boxes=True, box_ints=4, landmarks=True, real_bytes=8, landmark_n=3, left=[0], right=[2], sym_n=1)

    def call(**kw):
        a = dict(good, **kw)
        boxes = np.full(3 * 4, 0x5A5A, np.int32)
        lm = np.full(3 * 6, 1.5, np.float64)
        px = (api.jdaPixels * len(a["px"]))(*a["px"]) if a["px"] is not None else None
        vec = lambda v: None if v is None else (C.c_int * max(len(v), 1))(*v)
        rc = api.lib.jdaReduceBack(px, vec(a["factors"]), vec(a["orients"]), a["n_images"], vec(a["face_image"]), a["n_faces"],
                                   boxes.ctypes.data_as(ip) if a["boxes"] else None, a["box_ints"], lm.ctypes.data if a["landmarks"] else None,
                                   a["real_bytes"], a["landmark_n"], vec(a["left"]), vec(a["right"]), a["sym_n"])
        return rc, (boxes == 0x5A5A).all() and (lm == 1.5).all()
    rc, untouched = call()
    assert rc == 0 and not untouched
    bad = lambda **kw: [_px(api, image, pr.GRAY8, rect), _px(api, image, pr.GRAY8, **kw)]
    cases = [("null images", dict(px=None), ["null"]), ("null orients", dict(orients=None), ["null"]), ("null face_image", dict(face_image=None), ["null"]),
             ("null factors", dict(factors=None), ["null factors"]),
             ("factor 0", dict(factors=[0, 2]), ["image 0", "factor 0"]), ("factor 9", dict(factors=[3, 9]), ["image 1", "factor 9"]),
             ("w below f", dict(factors=[3, 2], px=bad(rect=(0, 0, 1, 5))), ["image 1", "1 x 5", "factor 2"]),
             ("h below f", dict(factors=[8, 8], px=[_px(api, image, pr.GRAY8, (5, 3, 11, 7)), good["px"][1]]), ["image 0", "11 x 7", "factor 8"]),
             ("negative n_faces", dict(n_faces=-2), ["-2"]), ("box_ints 2", dict(box_ints=2), ["box_ints", "2"]), ("box_ints 5", dict(box_ints=5), ["box_ints", "5"]),
             ("real_bytes 2", dict(real_bytes=2), ["real_bytes", "2"]), ("real_bytes 16", dict(real_bytes=16), ["real_bytes", "16"]),
             ("face_image high", dict(face_image=[0, 1, 2]), ["face 2", "face_image 2"]), ("face_image negative", dict(face_image=[0, -1, 1]), ["face 1", "face_image -1"]),
             ("pair id high", dict(left=[3]), ["pair 0", "(3, 2)"]), ("pair id negative", dict(left=[0, 1], right=[2, -1], sym_n=2), ["pair 1", "(1, -1)"]),
             ("null pairs", dict(left=None), ["null"]), ("negative sym_n", dict(sym_n=-1), ["-1"]),
             ("orientation 8", dict(orients=[1, 8]), ["image 1", "orientation 8"]), ("orientation -1", dict(orients=[-1, 4]), ["image 0", "orientation -1"]),
             ("null data", dict(px=bad(data=False)), ["image 1", "null"]), ("unknown format", dict(px=[good["px"][0], _px(api, image, 5)]), ["image 1", "format 5"]),
             ("no width", dict(px=bad(width=0)), ["image 1", "0 x 47"]), ("rectangle leaves", dict(px=bad(rect=(60, 0, 4, 2))), ["image 1", "(60, 0, 4, 2)"]),
             ("w below 1", dict(px=bad(rect=(0, 0, 0, 3))), ["image 1", "(0, 0, 0, 3)"]), ("pitch below a row", dict(px=bad(pitch=60)), ["image 1", "pitch 60"])]
    for what, kw, words in cases:
        rc, untouched = call(**kw)
        assert rc == -1 and untouched, what
        for w in words:
            assert w in api.last_error(), (what, api.last_error())
        assert "jdaReduceBack" in api.last_error(), what
    # what may be NULL: boxes, landmarks (then real_bytes, landmark_n and the pairs are not looked at); no faces touches nothing
    assert call(boxes=False, box_ints=0)[0] == 0 and call(landmarks=False, real_bytes=0, landmark_n=0, left=None, right=None)[0] == 0
    assert call(sym_n=0, left=None, right=None)[0] == 0 and call(box_ints=3)[0] == 0
    assert api.lib.jdaReduceBack(None, None, None, 0, None, 0, None, 0, None, 0, 0, None, None, 0) == 0
