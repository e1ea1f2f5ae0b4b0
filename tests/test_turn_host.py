"""Frames in any orientation (include/jda.h), without a GPU: the orientation table against numpy, jdaOrientSize,
jdaPackGrayOriented against the restatement of tests/turn_ref.py, and jdaOrientBack -- boxes, landmarks, pair exchange,
refusals.  Every comparison is exact."""
import ctypes as C

import numpy as np
import pytest

import pack_ref as pr
import turn_ref as tr
from mining_ref import transform

WIDTHS = [1, 2, 3, 15, 16, 17, 63, 64, 65, 100]
HEIGHTS = [1, 2, 3, 63, 64, 65]


@pytest.fixture(scope="module")
def api(built):
    from jda_amd import api
    return api


def _eq(got, want):
    assert got.shape == want.shape and got.dtype == np.uint8 and np.array_equal(got, want)


# ---- the orientation, defined once ------------------------------------------------------------------------------------------

def test_exif_table_against_numpy(api):
    """EXIF Orientation: what has to be done to the STORED image to display it (tag 6: the 0th row is the visual right-hand
    side, the 0th column the visual top -- a quarter turn clockwise; tag 8: counter-clockwise; 5 / 7: the two diagonals)."""
    a = np.arange(5 * 7, dtype=np.uint8).reshape(5, 7)
    display = {1: a, 2: np.fliplr(a), 3: np.rot90(a, 2), 4: np.flipud(a), 5: a.T, 6: np.rot90(a, -1), 7: np.rot90(a, 2).T, 8: np.rot90(a, 1)}
    for tag in range(1, 9):
        t = api.orient_from_exif(tag)
        assert t == tr.EXIF[tag] and np.array_equal(transform(a, t), display[tag]), tag
        _eq(api.pack_gray_oriented([a], "gray8", t)[0], np.ascontiguousarray(display[tag]))
    assert sorted(api.orient_from_exif(k) for k in range(1, 9)) == list(range(8))
    for bad in (0, 9, -1):
        with pytest.raises(ValueError):
            api.orient_from_exif(bad)


def test_the_formula_is_the_transform(api):
    """include/jda.h's (swap, flipX, flipY) formula, pixel by pixel, against mining_ref.transform."""
    a = np.arange(3 * 4, dtype=np.uint8).reshape(3, 4)
    for t in tr.ORIENTS:
        T = transform(a, t)
        for v in range(T.shape[0]):
            for u in range(T.shape[1]):
                x, y = (v, u) if t in tr.SWAP else (u, v)
                x = 4 - 1 - x if t in tr.FLIP_X else x
                y = 3 - 1 - y if t in tr.FLIP_Y else y
                assert T[v, u] == a[y, x], (t, u, v)


def test_orient_size(api):
    for t in tr.ORIENTS:
        assert api.orient_size(640, 480, t) == ((480, 640) if t in (1, 3, 5, 7) else (640, 480)) == tr.size(640, 480, t)
    tw, th = C.c_int(7), C.c_int(7)
    for t in (-1, 8):
        assert api.lib.jdaOrientSize(4, 3, t, C.byref(tw), C.byref(th)) == -1 and str(t) in api.last_error()
    assert api.lib.jdaOrientSize(4, 3, 1, None, C.byref(th)) == -1 and api.lib.jdaOrientSize(4, 3, 1, C.byref(tw), None) == -1
    assert (tw.value, th.value) == (7, 7)


# ---- jdaPackGrayOriented ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("t", tr.ORIENTS)
@pytest.mark.parametrize("fmt", pr.FORMATS)
def test_shapes(api, fmt, t):
    rng = np.random.default_rng(8 * fmt + t)
    views = [pr.pitched(rng, h, w, fmt, (w + h) % 4, (3 * w + h) % 16)[1] for w in WIDTHS for h in HEIGHTS]
    got = api.pack_gray_oriented(views, fmt, t)
    for g, v in zip(got, views):
        _eq(g, tr.turn(v, fmt, t))


@pytest.mark.parametrize("name", sorted(pr.RECTS))
def test_rectangles(api, name):
    rng = np.random.default_rng(7)
    views, fmts, rects, ts = [], [], [], []
    for fmt in pr.FORMATS:
        for t in tr.ORIENTS:
            views.append(pr.pitched(rng, 21, 37, fmt, 5, 1)[1]); fmts.append(fmt); rects.append(pr.RECTS[name](37, 21)); ts.append(t)
    for g, v, f, r, t in zip(api.pack_gray_oriented(views, fmts, ts, rects), views, fmts, rects, ts):
        _eq(g, tr.turn(v, f, t, r))


def test_orientation_0_is_pack_gray(api):
    rng = np.random.default_rng(2)
    views = [pr.pitched(rng, 1 + 7 * i, 3 + 11 * i, pr.FORMATS[i % 5], i, i)[1] for i in range(10)]
    fmts = [pr.FORMATS[i % 5] for i in range(10)]
    rects = [None if i % 2 else (1, 0, 2 + 5 * i, 1 + 3 * i) for i in range(10)]
    for a, b in zip(api.pack_gray_oriented(views, fmts, 0, rects), api.pack_gray(views, fmts, rects)):
        _eq(a, b)
    assert api.lib.jdaPackGrayOriented(None, None, 0, None, None) == 0        # touches nothing


def test_pack_refusals_name_the_image_and_leave_dst_alone(api):
    from test_pack_host import _px, refusals
    rng = np.random.default_rng(3)
    a = rng.integers(0, 256, (6, 8, 3), dtype=np.uint8)
    b = rng.integers(0, 256, (6, 8, 3), dtype=np.uint8)
    cases = [(what, px, offs, n, words, (1, 4)) for what, px, offs, n, words in refusals(api, a, b)]
    ok = [_px(api, a, pr.BGR24), _px(api, b, pr.BGR24)]
    cases += [("orientation 8", ok, [64, 112], 2, ["image 1", "orientation 8"], (0, 8)), ("orientation -1", ok, [64, 112], 2, ["image 0", "orientation -1"], (-1, 3)),
              # a 6 x 8 turned image takes the 48 bytes the upright one takes: one byte less than needed still overlaps
              ("turned destinations overlap", ok, [64, 111], 2, ["image 0", "image 1", "overlap"], (1, 3))]
    for what, px, offs, n, words, ts in cases:
        dst = np.full(256, 0xA5, np.uint8)
        arr = (api.jdaPixels * len(px))(*px)
        rc = api.lib.jdaPackGrayOriented(arr, (C.c_int * 2)(*ts), n, dst.ctypes.data, (C.c_size_t * len(offs))(*offs))
        assert rc == -1, what
        for w in words:
            assert w in api.last_error(), (what, api.last_error())
        assert "jdaPackGrayOriented" in api.last_error() and (dst == 0xA5).all(), what
    arr = (api.jdaPixels * 2)(*ok)
    o, ts = (C.c_size_t * 2)(64, 112), (C.c_int * 2)(1, 4)
    dst = np.full(256, 0xA5, np.uint8)
    for args in ((None, ts, 2, dst.ctypes.data, o), (arr, None, 2, dst.ctypes.data, o), (arr, ts, 2, None, o), (arr, ts, 2, dst.ctypes.data, None)):
        assert api.lib.jdaPackGrayOriented(*args) == -1 and "null" in api.last_error()
    assert (dst == 0xA5).all()
    assert api.lib.jdaPackGrayOriented(arr, ts, 2, dst.ctypes.data, o) == 0
    assert np.array_equal(dst[64:112].reshape(8, 6), tr.turn(a, pr.BGR24, 1)) and np.array_equal(dst[112:160].reshape(6, 8), tr.turn(b, pr.BGR24, 4))


# ---- jdaOrientBack ----------------------------------------------------------------------------------------------------------

W, H, RECT = 23, 17, (5, 3, 11, 9)                       # a rectangle inside a larger image


@pytest.fixture(scope="module")
def image():
    # every pixel its own value: "the pixel holding the same byte" is one pixel
    return (np.arange(W * H, dtype=np.int64) % 251).astype(np.uint8).reshape(H, W)


def _boxes(tw, th):
    """(x, y, w, h) in a tw x th turned rectangle: sizes 1, 2, 7 and the whole image, square and not."""
    out = [(0, 0, 1, 1), (tw - 1, th - 1, 1, 1), (1, 2, 2, 2), (tw - 2, 0, 2, 2), (2, 1, 7, 7), (0, 0, tw, th)]
    out += [(1, 0, 3, 5), (tw - 4, th - 2, 4, 2), (0, 3, tw, 1), (2, 0, 1, th)]
    return out


@pytest.mark.parametrize("t", tr.ORIENTS)
@pytest.mark.parametrize("rect", [RECT, None])
def test_boxes_land_on_the_same_pixels(api, image, t, rect):
    turned = tr.turn(image, pr.GRAY8, t, rect)
    th, tw = turned.shape
    r = tr.rect_of(image, rect)
    for box_ints in (3, 4):
        boxes = [b for b in _boxes(tw, th) if box_ints == 4 or b[2] == b[3]]
        arr = np.array([b[:box_ints] for b in boxes], np.int32)
        got, none = api.orient_back([image], "gray8", t, [0] * len(boxes), boxes=arr, rects=[rect])
        assert none is None and got.dtype == np.int32 and got.shape == arr.shape
        for b, g in zip(boxes, got):
            assert tuple(g) == tr.back_box(b[:box_ints], t, r), (b, g)
            x, y, bw = int(g[0]), int(g[1]), int(g[2])
            bh = int(g[3]) if box_ints == 4 else bw
            assert 0 <= x and x + bw <= W and 0 <= y and y + bh <= H
            under = transform(image[y:y + bh, x:x + bw], t)
            assert np.array_equal(under, turned[b[1]:b[1] + b[3], b[0]:b[0] + b[2]]), (t, b, g)


@pytest.mark.parametrize("real", [np.float32, np.float64])
@pytest.mark.parametrize("t", tr.ORIENTS)
def test_landmarks_land_on_the_same_pixel(api, image, t, real):
    turned = tr.turn(image, pr.GRAY8, t, RECT)
    th, tw = turned.shape
    pts = [(u, v) for v in range(th) for u in range(tw)]
    lm = np.array(pts, real).reshape(1, -1)
    _, got = api.orient_back([image], "gray8", t, [0], landmarks=lm, rects=[RECT])
    assert got.dtype == real and got.shape == lm.shape
    for (u, v), (x, y) in zip(pts, got.reshape(-1, 2)):
        assert x == int(x) and y == int(y) and image[int(y), int(x)] == turned[v, u], (t, u, v, x, y)
    # ... and between pixel centres, to the bit, against the restatement
    rng = np.random.default_rng(t)
    frac = rng.uniform(-3, 20, (4, 10)).astype(real)
    _, got = api.orient_back([image] * 2, "gray8", [t, 0], [0, 1, 0, 1], landmarks=frac, rects=[RECT, RECT])
    for f in range(4):
        want = tr.back_landmarks(frac[f], t if f % 2 == 0 else 0, RECT)
        assert np.array_equal(got[f].view(np.uint8), want.view(np.uint8)), (t, f)


def test_pairs_are_exchanged_for_mirrors_only_and_sequentially(api, image):
    L = 5
    lm = np.arange(2 * L, dtype=np.float64).reshape(1, -1) / 4
    left, right = [0, 1, 0], [3, 4, 1]                   # landmark 0 and 1 are named twice
    for t in tr.ORIENTS:
        _, plain = api.orient_back([image], "gray8", t, [0], landmarks=lm, rects=[RECT])
        _, got = api.orient_back([image], "gray8", t, [0], landmarks=lm, rects=[RECT], left=left, right=right)
        want = plain.reshape(L, 2).copy()
        if t in (4, 5, 6, 7):
            for a, b in zip(left, right):
                want[[a, b]] = want[[b, a]]
            assert not np.array_equal(want, plain.reshape(L, 2))
        assert np.array_equal(got.reshape(L, 2), want), t
        assert np.array_equal(got[0], tr.back_landmarks(lm[0], t, RECT, left, right))


def test_back_and_forth_is_the_identity(api, image):
    """Turn by t, then turn the turned image by the inverse orientation: boxes and landmarks mapped back twice are where they were."""
    boxes = np.array([(1, 2, 3, 2), (0, 0, 11, 9), (4, 5, 1, 1)], np.int32)
    lm = np.array([[0.5, 1.25, 3, 4], [10, 8, 0, 0], [2.75, 6.5, 1, 1]], np.float64)
    for t in tr.ORIENTS:
        inv = [s for s in tr.ORIENTS if np.array_equal(transform(transform(image, t), s), image)]
        assert len(inv) == 1
        turned = transform(image, t)
        # coordinates in `image` -> found on transform(turned, inv) == image; back to `turned`, then back to `image`
        b1, l1 = api.orient_back([turned], "gray8", inv[0], [0, 0, 0], boxes=boxes, landmarks=lm, left=[0], right=[1])
        b2, l2 = api.orient_back([image], "gray8", t, [0, 0, 0], boxes=b1, landmarks=l1, left=[0], right=[1])
        assert np.array_equal(b2, boxes) and np.array_equal(l2, lm), t


def test_detect_results_form(api, image):
    """One detect result per image (None: no face), either dialect's."""
    c = [dict(bboxes=np.array([[1, 2, 3]], np.int32), scores=np.array([0.5], np.float32), shapes=np.array([[1, 2, 3, 4]], np.float32)), None]
    got = api.orient_back([image] * 2, "gray8", [1, 2], c, rects=[RECT, None])
    assert got[1] is None and np.array_equal(got[0]["scores"], c[0]["scores"]) and got[0]["shapes"].dtype == np.float32
    assert tuple(got[0]["bboxes"][0]) == tr.back_box((1, 2, 3), 1, RECT)
    assert np.array_equal(got[0]["shapes"][0], tr.back_landmarks(c[0]["shapes"][0], 1, RECT))
    assert np.array_equal(c[0]["bboxes"], [[1, 2, 3]])                       # the caller's results are not touched
    d = [dict(rects=np.zeros((0, 4), np.int32), scores=np.zeros(0), shapes=np.zeros((0, 4))),
         dict(rects=np.array([[0, 1, 2, 3], [1, 1, 1, 1]], np.int32), scores=np.array([1., 2.]), shapes=np.array([[0, 0, 1, 1], [2, 2, 3, 3]], np.float64))]
    got = api.orient_back([image] * 2, "gray8", [4, 7], d)
    assert len(got[0]["scores"]) == 0 and got[1]["shapes"].dtype == np.float64
    for k in range(2):
        assert tuple(got[1]["rects"][k]) == tr.back_box(tuple(d[1]["rects"][k]), 7, (0, 0, W, H))
        assert np.array_equal(got[1]["shapes"][k], tr.back_landmarks(d[1]["shapes"][k], 7, (0, 0, W, H)))


def test_back_refusals_name_the_index_and_write_nothing(api, image):
    from test_pack_host import _px
    ip = C.POINTER(C.c_int)
    good = dict(px=[_px(api, image, pr.GRAY8, RECT), _px(api, image, pr.GRAY8)], orients=[1, 4], n_images=2, face_image=[0, 1, 1], n_faces=3,
                boxes=True, box_ints=4, landmarks=True, real_bytes=8, landmark_n=3, left=[0], right=[2], sym_n=1)

    def call(**kw):
        a = dict(good, **kw)
        boxes = np.full(3 * 4, 0x5A5A, np.int32)
        lm = np.full(3 * 6, 1.5, np.float64)
        px = (api.jdaPixels * len(a["px"]))(*a["px"]) if a["px"] is not None else None
        vec = lambda v: None if v is None else (C.c_int * max(len(v), 1))(*v)
        rc = api.lib.jdaOrientBack(px, vec(a["orients"]), a["n_images"], vec(a["face_image"]), a["n_faces"],
                                   boxes.ctypes.data_as(ip) if a["boxes"] else None, a["box_ints"], lm.ctypes.data if a["landmarks"] else None,
                                   a["real_bytes"], a["landmark_n"], vec(a["left"]), vec(a["right"]), a["sym_n"])
        return rc, (boxes == 0x5A5A).all() and (lm == 1.5).all()
    rc, untouched = call()
    assert rc == 0 and not untouched
    bad = lambda **kw: [_px(api, image, pr.GRAY8, RECT), _px(api, image, pr.GRAY8, **kw)]
    cases = [("null images", dict(px=None), ["null"]), ("null orients", dict(orients=None), ["null"]), ("null face_image", dict(face_image=None), ["null"]),
             ("negative n_faces", dict(n_faces=-2), ["-2"]), ("box_ints 2", dict(box_ints=2), ["box_ints", "2"]), ("box_ints 5", dict(box_ints=5), ["box_ints", "5"]),
             ("real_bytes 2", dict(real_bytes=2), ["real_bytes", "2"]), ("real_bytes 16", dict(real_bytes=16), ["real_bytes", "16"]),
             ("face_image high", dict(face_image=[0, 1, 2]), ["face 2", "face_image 2"]), ("face_image negative", dict(face_image=[0, -1, 1]), ["face 1", "face_image -1"]),
             ("pair id high", dict(left=[3]), ["pair 0", "(3, 2)"]), ("pair id negative", dict(left=[0, 1], right=[2, -1], sym_n=2), ["pair 1", "(1, -1)"]),
             ("null pairs", dict(left=None), ["null"]), ("negative sym_n", dict(sym_n=-1), ["-1"]),
             ("orientation 8", dict(orients=[1, 8]), ["image 1", "orientation 8"]), ("orientation -1", dict(orients=[-1, 4]), ["image 0", "orientation -1"]),
             ("null data", dict(px=bad(data=False)), ["image 1", "null"]), ("unknown format", dict(px=[good["px"][0], _px(api, image, 5)]), ["image 1", "format 5"]),
             ("no width", dict(px=bad(width=0)), ["image 1", "0 x 17"]), ("rectangle leaves", dict(px=bad(rect=(20, 0, 4, 2))), ["image 1", "(20, 0, 4, 2)"]),
             ("w below 1", dict(px=bad(rect=(0, 0, 0, 3))), ["image 1", "(0, 0, 0, 3)"]), ("pitch below a row", dict(px=bad(pitch=22)), ["image 1", "pitch 22"])]
    for what, kw, words in cases:
        rc, untouched = call(**kw)
        assert rc == -1 and untouched, what
        for w in words:
            assert w in api.last_error(), (what, api.last_error())
        assert "jdaOrientBack" in api.last_error(), what
    # what may be NULL: boxes, landmarks (then real_bytes, landmark_n and the pairs are not looked at); no faces touches nothing
    assert call(boxes=False, box_ints=0)[0] == 0 and call(landmarks=False, real_bytes=0, landmark_n=0, left=None, right=None)[0] == 0
    assert call(sym_n=0, left=None, right=None)[0] == 0 and call(box_ints=3)[0] == 0
    assert api.lib.jdaOrientBack(None, None, 0, None, 0, None, 0, None, 0, 0, None, None, 0) == 0
