"""jdaRotationPlan, jdaPackGrayRotated and jdaRotateBack (include/jda.h, "frames whose faces are rolled"; rotate.cpp) against
tests/rotate_ref.py, the numpy restatement that takes c, s, tw, th from the plan and is integer arithmetic from X, Y on.  No
GPU.  Every image comparison is exact."""
import ctypes as C

import numpy as np
import pytest

import pack_ref as pr
import rotate_ref as ro

SIDES = (1, 2, 7, 63, 64, 65, 130)
QUARTERS = {0: 0, 90: 1, 180: 2, 270: 3}


@pytest.fixture(scope="module")
def api(built):
    from jda_amd import api
    return api


def _eq(got, want):
    assert got.shape == want.shape and got.dtype == np.uint8 and np.array_equal(got, want)


def check(api, views, fmts, degs, rects=None):
    """One call; every image against the restatement on the plan of its rectangle."""
    got = api.pack_gray_rotated(views, fmts, degs, rects)
    fmts = [fmts] * len(views) if isinstance(fmts, int) else fmts
    for i, (g, v, fm, d) in enumerate(zip(got, views, fmts, degs)):
        r = None if rects is None else rects[i]
        w, h = (v.shape[1], v.shape[0]) if r is None else r[2:]
        _eq(g, ro.rotate(v, fm, api.rotation_plan(w, h, d), r))
    return got


# ---- jdaRotationPlan ----------------------------------------------------------------------------------------------------------

def test_plan_is_exact_at_quarter_turns(api):
    for d, cs in ((-360, (1, 0)), (-90, (0, -1)), (0, (1, 0)), (90, (0, 1)), (180, (-1, 0)), (270, (0, -1)), (450, (0, 1)), (36000, (1, 0)), (-35910, (0, 1))):
        p = api.rotation_plan(37, 21, d)
        assert (p["c"], p["s"]) == cs, d
        assert (p["tw"], p["th"]) == ((37, 21) if cs[1] == 0 else (21, 37)) and (p["w"], p["h"]) == (37, 21)
        assert (api.rotation_plan(1, 1, d)["tw"], api.rotation_plan(1, 1, d)["th"]) == (1, 1)    # 1 x 1 stays 1 x 1 at every quarter turn


def test_plan_elsewhere(api):
    """c and s within 1e-15 of numpy's; tw and th by the header's formula from the plan's own c and s."""
    rng = np.random.default_rng(1)
    for d in list(ro.ANGLES) + list(rng.uniform(-36000, 36000, 200)) + [89.99999, 90.00001, 1e-9, -36000 + 1e-7]:
        for w, h in ((640, 480), (1, 1), (7, 130), (32768, 3)):
            p = api.rotation_plan(w, h, d)
            if d % 90:
                assert abs(p["c"] - np.cos(d * (np.pi / 180))) <= 1e-15 and abs(p["s"] - np.sin(d * (np.pi / 180))) <= 1e-15, d
            assert (p["tw"], p["th"]) == ro.plan_size(w, h, p["c"], p["s"]), (d, w, h)
            assert p["tw"] >= 1 and p["th"] >= 1
    # (the formula, not 1 x 1: at 45 degrees the pixel's square is 1.414 wide)
    assert (api.rotation_plan(1, 1, 45)["tw"], api.rotation_plan(1, 1, 45)["th"]) == (2, 2)
    assert (api.rotation_plan(640, 480, 30)["tw"], api.rotation_plan(640, 480, 30)["th"]) == (795, 736)


def test_plan_refusals(api):
    rot = api.jdaRotation(tw=7, th=7)
    for args, word in (((4, 3, float("nan")), "nan"), ((4, 3, float("inf")), "inf"), ((4, 3, -float("inf")), "inf"), ((4, 3, 36001.0), "36001"),
                       ((4, 3, -36000.5), "-36000.5"), ((0, 3, 10.0), "0 x 3"), ((4, -1, 10.0), "4 x -1")):
        assert api.lib.jdaRotationPlan(*args, C.byref(rot)) == -1 and word in api.last_error(), (args, api.last_error())
        assert "jdaRotationPlan" in api.last_error()
    assert api.lib.jdaRotationPlan(4, 3, 10.0, None) == -1 and "null" in api.last_error()
    assert (rot.tw, rot.th) == (7, 7)
    assert api.lib.jdaRotationPlan(4, 3, 36000.0, C.byref(rot)) == 0 and (rot.tw, rot.th) == (4, 3)


# ---- jdaPackGrayRotated -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("k", range(len(SIDES)))
def test_gray_every_width_meets_every_height(api, k):
    """GRAY8: width SIDES[i] with height SIDES[(i + k) % 7], every angle of the list on every pair, pitch slack and source
    misalignment 0..3."""
    rng = np.random.default_rng(k)
    views, degs = [], []
    for i, w in enumerate(SIDES):
        h = SIDES[(i + k) % len(SIDES)]
        for j, d in enumerate(ro.ANGLES):
            views.append(pr.pitched(rng, h, w, pr.GRAY8, (w + j) % 4, (i + j) % 4)[1]); degs.append(d)
    check(api, views, pr.GRAY8, degs)


@pytest.mark.parametrize("fmt", pr.FORMATS[1:])
def test_colour_shapes(api, fmt):
    rng = np.random.default_rng(10 + fmt)
    views, degs = [], []
    for j, (w, h) in enumerate(((1, 1), (2, 7), (7, 2), (63, 65), (64, 64), (65, 63), (130, 7), (7, 130), (130, 67))):
        for i, d in enumerate(ro.ANGLES):
            if (i + j) % 3 == fmt % 3:
                views.append(pr.pitched(rng, h, w, fmt, (w + i) % 4, (j + i) % 4)[1]); degs.append(d)
    assert len(set(degs)) == len(ro.ANGLES)
    check(api, views, fmt, degs)


@pytest.mark.parametrize("name", sorted(pr.RECTS))
def test_rectangles(api, name):
    rng = np.random.default_rng(7)
    views, fmts, degs, rects = [], [], [], []
    for fmt in pr.FORMATS:
        for d in (30, -33.3, 90, 135):
            views.append(pr.pitched(rng, 21, 37, fmt, 5, 1)[1]); fmts.append(fmt); degs.append(d); rects.append(pr.RECTS[name](37, 21))
    check(api, views, fmts, degs, rects)


def test_quarter_turns_are_the_orientations(api):
    """90 / 180 / 270 = jdaPackGrayOriented at 1 / 2 / 3 and 0 = jdaPackGray, on non-square sizes: in a call of quarter turns
    only (which may forward) and in a call that also holds another angle (the loops over the definition)."""
    rng = np.random.default_rng(2)
    for fmt in pr.FORMATS:
        for w, h in ((37, 21), (1, 9), (64, 3), (2, 131)):
            v = pr.pitched(rng, h, w, fmt, 3, 1)[1]
            other = pr.pitched(rng, 5, 4, fmt)[1]
            for d, t in QUARTERS.items():
                want = api.pack_gray_oriented([v], fmt, t)[0]
                for dd in (d, d - 360, d + 720):
                    _eq(api.pack_gray_rotated([v], fmt, dd)[0], want)
                    _eq(api.pack_gray_rotated([v, other], fmt, [dd, 15])[0], want)
            _eq(api.pack_gray_rotated([v, other], fmt, [0, 15])[0], api.pack_gray([v], fmt)[0])


def test_colour_rotates_like_its_gray_image(api):
    rng = np.random.default_rng(3)
    for fmt in pr.FORMATS[1:]:
        v = pr.pitched(rng, 33, 41, fmt, 2, 3)[1]
        g = api.pack_gray([v], fmt)[0]
        for a, b in zip(api.pack_gray_rotated([v] * len(ro.ANGLES), fmt, ro.ANGLES), api.pack_gray_rotated([g] * len(ro.ANGLES), pr.GRAY8, ro.ANGLES)):
            _eq(a, b)


def test_nothing_outside_the_rectangle_leaks_in(api):
    """A black rectangle with one gray pixel inside an image of 255s: the rotated image holds nothing brighter than that
    pixel, and its corners are black."""
    img = np.full((40, 50), 255, np.uint8)
    rect = (9, 7, 30, 20)
    img[7:27, 9:39] = 0
    img[15, 20] = 100
    for d in ro.ANGLES:
        g = api.pack_gray_rotated([img], pr.GRAY8, d, [rect])[0]
        assert g.max() <= 100 and g.max() > 0, d
        if d % 90:
            assert g[0, 0] == g[0, -1] == g[-1, 0] == g[-1, -1] == 0, d
    full = np.full((20, 30), 255, np.uint8)
    g = api.pack_gray_rotated([np.pad(full, 5)], pr.GRAY8, 30, [(5, 5, 30, 20)])[0]
    _eq(g, api.pack_gray_rotated([full], pr.GRAY8, 30)[0])
    assert g[0, 0] == 0 and g[-1, -1] == 0 and g[g.shape[0] // 2, g.shape[1] // 2] == 255


def test_pack_refusals_name_the_image_and_leave_dst_alone(api):
    from test_pack_host import _px, refusals
    rng = np.random.default_rng(3)
    a = rng.integers(0, 256, (6, 8, 3), dtype=np.uint8)
    b = rng.integers(0, 256, (6, 8, 3), dtype=np.uint8)
    # jdaPackGray's own, at angle 0 (the destinations are the 48 bytes they are there)
    cases = [(what, px, offs, n, words, (0.0, 0.0)) for what, px, offs, n, words in refusals(api, a, b)]
    ok = [_px(api, a, pr.BGR24), _px(api, b, pr.BGR24)]
    big = api.jdaPixels(a.ctypes.data, 3 * 50000, 50000, 1, pr.BGR24, 0, 0, 0, 0)              # (refused before a byte of it is read)
    cases += [("nan", ok, [64, 112], 2, ["image 1", "nan"], (0.0, float("nan"))), ("inf", ok, [64, 112], 2, ["image 0", "inf"], (float("inf"), 0.0)),
              ("36001", ok, [64, 112], 2, ["image 1", "36001"], (0.0, 36001.0)),
              ("too wide", [ok[0], big], [64, 112], 2, ["image 1", "50000 x 1", "32768"], (0.0, 45.0)),
              # 8 x 6 at 30 degrees is 10 x 10 = 100 bytes: one byte less than needed still overlaps
              ("rotated destinations overlap", ok, [0, 99], 2, ["image 0", "image 1", "100 bytes", "overlap"], (30.0, 30.0))]
    for what, px, offs, n, words, degs in cases:
        dst = np.full(256, 0xA5, np.uint8)
        arr = (api.jdaPixels * len(px))(*px)
        rc = api.lib.jdaPackGrayRotated(arr, (C.c_double * 2)(*degs), n, dst.ctypes.data, (C.c_size_t * len(offs))(*offs))
        assert rc == -1, what
        for w in words:
            assert w in api.last_error(), (what, api.last_error())
        assert "jdaPackGrayRotated" in api.last_error() and (dst == 0xA5).all(), what
    arr = (api.jdaPixels * 2)(*ok)
    o, degs = (C.c_size_t * 2)(0, 100), (C.c_double * 2)(30.0, 30.0)
    dst = np.full(256, 0xA5, np.uint8)
    for args in ((None, degs, 2, dst.ctypes.data, o), (arr, None, 2, dst.ctypes.data, o), (arr, degs, 2, None, o), (arr, degs, 2, dst.ctypes.data, None)):
        assert api.lib.jdaPackGrayRotated(*args) == -1 and "null" in api.last_error()
    assert (dst == 0xA5).all()
    # ... and right behind each other they are taken; an empty call touches nothing
    assert api.lib.jdaPackGrayRotated(arr, degs, 2, dst.ctypes.data, o) == 0
    p = api.rotation_plan(8, 6, 30)
    assert np.array_equal(dst[:100].reshape(10, 10), ro.rotate(a, pr.BGR24, p)) and np.array_equal(dst[100:200].reshape(10, 10), ro.rotate(b, pr.BGR24, p))
    assert (dst[200:] == 0xA5).all()
    assert api.lib.jdaPackGrayRotated(None, None, 0, None, None) == 0


# ---- jdaRotateBack ------------------------------------------------------------------------------------------------------------

W, H, RECT, BLOB = 90, 70, (11, 6, 61, 47), (40, 30)          # the blob's centre, in the whole image: inside the rectangle


@pytest.fixture(scope="module")
def blob():
    img = np.full((H, W), 255, np.uint8)                          # (255s outside the rectangle: a leak would move the centroid)
    img[RECT[1]:RECT[1] + RECT[3], RECT[0]:RECT[0] + RECT[2]] = 0
    img[BLOB[1] - 1:BLOB[1] + 2, BLOB[0] - 1:BLOB[0] + 2] = 240
    return img


@pytest.mark.parametrize("d", ro.ANGLES)
def test_a_blob_comes_back_to_where_it_is(api, blob, d):
    """The rotated image's intensity centroid, as a landmark in float and in double, lands within 0.51 pixel of the blob's
    centre; boxes of box_ints 3 and 4 around it come back centred within 1 pixel, sizes unchanged; all equal the restatement."""
    g = api.pack_gray_rotated([blob], pr.GRAY8, d, [RECT])[0].astype(np.float64)
    ys, xs = np.mgrid[0:g.shape[0], 0:g.shape[1]]
    cx, cy = (g * xs).sum() / g.sum(), (g * ys).sum() / g.sum()
    plan = api.rotation_plan(RECT[2], RECT[3], d)
    for real in (np.float32, np.float64):
        lm = np.array([[cx, cy, cx + 3.25, cy - 2.5]], real)
        _, back = api.rotate_back([blob], pr.GRAY8, d, [0], None, lm, [RECT])
        assert back.dtype == real and abs(back[0, 0] - BLOB[0]) <= 0.51 and abs(back[0, 1] - BLOB[1]) <= 0.51, (d, back)
        assert np.array_equal(back[0], ro.back_landmarks(lm[0], plan, RECT))
    for box in ((int(round(cx)) - 4, int(round(cy)) - 4, 9), (int(round(cx)) - 5, int(round(cy)) - 3, 11, 7), (int(round(cx)) - 3, int(round(cy)) - 3, 8)):
        b, _ = api.rotate_back([blob], pr.GRAY8, d, [0], [box], None, [RECT])
        bw, bh = box[2], box[-1]
        assert tuple(b[0][2:]) == tuple(box[2:])
        # centred within 1 pixel on where its centre -- a point within half a pixel of the centroid -- lies in the source image
        _, c = api.rotate_back([blob], pr.GRAY8, d, [0], None, np.array([[box[0] + (bw - 1) / 2, box[1] + (bh - 1) / 2]]), [RECT])
        assert abs(b[0][0] + (bw - 1) / 2 - c[0, 0]) <= 1 and abs(b[0][1] + (bh - 1) / 2 - c[0, 1]) <= 1, (d, box, b, c)
        assert abs(c[0, 0] - BLOB[0]) <= 0.51 + 0.5 * 2 ** 0.5 and abs(c[0, 1] - BLOB[1]) <= 0.51 + 0.5 * 2 ** 0.5, (d, box, c)
        assert tuple(b[0]) == ro.back_box(box, plan, RECT)


def test_quarter_turns_are_orient_back(api, blob):
    """Square boxes, bit for bit; landmarks bit for bit where jdaOrientBack's own float steps are exact -- values on a 1/64
    grid, which both types hold exactly through every step here -- and within double's rounding of the exact value for
    arbitrary doubles."""
    rng = np.random.default_rng(5)
    n = 40
    boxes = np.column_stack([rng.integers(-20, 80, n), rng.integers(-20, 80, n), rng.integers(1, 40, n)]).astype(np.int32)
    grid = rng.integers(-64 * 30, 64 * 90, (n, 10)) / 64.0
    free = rng.uniform(-30, 90, (n, 10))
    for d, t in QUARTERS.items():
        for dd in (d, d - 360):
            for real in (np.float32, np.float64):
                b1, l1 = api.rotate_back([blob], pr.GRAY8, dd, [0] * n, boxes, grid.astype(real), [RECT])
                b2, l2 = api.orient_back([blob], pr.GRAY8, t, [0] * n, boxes, grid.astype(real), [RECT])
                assert np.array_equal(b1, b2) and l1.dtype == real and np.array_equal(l1, l2), (dd, real)
            b4 = np.column_stack([boxes, boxes[:, 2]])
            assert np.array_equal(api.rotate_back([blob], pr.GRAY8, dd, [0] * n, b4)[0], api.orient_back([blob], pr.GRAY8, t, [0] * n, b4)[0])
            _, l1 = api.rotate_back([blob], pr.GRAY8, dd, [0] * n, None, free, [RECT])
            _, l2 = api.orient_back([blob], pr.GRAY8, t, [0] * n, None, free, [RECT])
            assert np.abs(l1 - l2).max() <= 2.0 ** -44                # (three roundings of values below 2^7: 3 * 2^-46)


def test_detect_results_form(api, blob):
    res = [{"bboxes": np.array([[3, 4, 9], [10, 2, 5]], np.int32), "scores": np.array([1.5, 0.5], np.float32), "shapes": np.array([[1.5, 2.5], [7, 8]], np.float32)},
           None]
    out = api.rotate_back([blob, blob], pr.GRAY8, [30, -30], res, rects=[RECT, None])
    plan = api.rotation_plan(RECT[2], RECT[3], 30)
    assert out[1] is None and np.array_equal(out[0]["scores"], res[0]["scores"])
    for k in range(2):
        assert tuple(out[0]["bboxes"][k]) == ro.back_box(tuple(res[0]["bboxes"][k]), plan, RECT)
        assert np.array_equal(out[0]["shapes"][k], ro.back_landmarks(res[0]["shapes"][k], plan, RECT))


def test_back_refusals_name_the_index_and_write_nothing(api, blob):
    from test_pack_host import _px
    ip, dp = C.POINTER(C.c_int), C.POINTER(C.c_double)
    ok = (api.jdaPixels * 2)(_px(api, blob, pr.GRAY8, RECT), _px(api, blob, pr.GRAY8))
    bad = (api.jdaPixels * 2)(_px(api, blob, pr.GRAY8, RECT), _px(api, blob, pr.GRAY8, (80, 0, 20, 5)))
    degs, fi = (C.c_double * 2)(30.0, 90.0), (C.c_int * 3)(0, 1, 1)
    boxes0 = np.arange(12, dtype=np.int32)
    lms0 = np.arange(12, dtype=np.float32)

    def call(px=ok, dg=degs, n_img=2, face=fi, n=3, bx=True, bi=3, lm=True, rb=4, ln=2):
        b, l = boxes0.copy(), lms0.copy()
        rc = api.lib.jdaRotateBack(px, dg, n_img, face, n, b.ctypes.data_as(ip) if bx else None, bi, l.ctypes.data if lm else None, rb, ln)
        return rc, np.array_equal(b, boxes0) and np.array_equal(l, lms0)
    for kw, words in ((dict(px=None), ["null images"]), (dict(dg=None), ["null degrees"]), (dict(face=None), ["null face_image"]), (dict(n=-1), ["-1"]),
                      (dict(n_img=-2), ["-2"]), (dict(bi=5), ["box_ints = 5"]), (dict(rb=2), ["real_bytes = 2"]), (dict(ln=0), ["landmark_n = 0"]),
                      (dict(face=(C.c_int * 3)(0, 2, 1)), ["face 1", "face_image 2"]), (dict(px=bad), ["image 1", "(80, 0, 20, 5)"]),
                      (dict(dg=(C.c_double * 2)(30.0, float("nan"))), ["image 1", "nan"]), (dict(dg=(C.c_double * 2)(36000.5, 0.0)), ["image 0", "36000.5"])):
        rc, untouched = call(**kw)
        assert rc == -1 and untouched, kw
        for w in words:
            assert w in api.last_error(), (kw, api.last_error())
        assert "jdaRotateBack" in api.last_error()
    rc, untouched = call()
    assert rc == 0 and not untouched
    assert api.lib.jdaRotateBack(None, None, 0, None, 0, None, 0, None, 0, 0) == 0
    assert isinstance(dp, type)
