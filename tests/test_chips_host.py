"""jdaFaceChips and jdaCascadorMeanShape (include/jda.h, "faces as they leave"): upright face chips cut from host images,
without a GPU.  Every comparison is exact -- chips byte for byte, matrices bit for bit -- against the definition restated in
tests/chips_ref.py."""
import ctypes as C
import math

import numpy as np
import pytest

import chips_ref as cr
import pack_ref as pr
from conftest import same


@pytest.fixture(scope="module")
def api(built):
    from jda_amd import api
    return api


def _eq(got, want):
    assert got.shape == want.shape and got.dtype == np.uint8
    bad = np.argwhere(got != want)
    assert bad.size == 0, ("first wrong byte at", bad[0].tolist(), int(got[tuple(bad[0])]), int(want[tuple(bad[0])]))


SQUARE = np.array([2.0, 1.0, 6.0, 1.0, 2.0, 5.0, 6.0, 5.0])          # four template points whose mean is exact


def test_identity_is_the_crop(api):
    rng = np.random.default_rng(1)
    for fmt, chip_fmt in ((pr.GRAY8, "gray8"), (pr.BGR24, "bgr24"), (pr.RGB24, "rgb24")):
        img = rng.integers(0, 256, pr.shape_of(23, 31, fmt), dtype=np.uint8)
        ox, oy = 7, 5
        lm = SQUARE + np.tile([ox, oy], 4)
        got, M = api.face_chips([img], fmt, [0], [lm], SQUARE, 9, 8, chip_fmt, matrices=True)
        _eq(got[0], img[oy:oy + 8, ox:ox + 9])
        assert same(np.abs(M[0]), np.array([1.0, 0.0, ox, 0.0, 1.0, oy])) and same(M[0, [0, 2, 3, 4, 5]], np.array([1.0, ox, 0.0, 1.0, oy]))


@pytest.mark.parametrize("k", [1, 2, 3])
@pytest.mark.parametrize("size", [(8, 8), (5, 3)])
def test_quarter_turns_are_rot90_of_the_crop(api, k, size):
    cw, ch = size
    rng = np.random.default_rng(k)
    img = rng.integers(0, 256, (40, 40, 3), dtype=np.uint8)
    a, b = [(1, 0), (0, 1), (-1, 0), (0, -1)][k]
    tx, ty = 20, 19
    q = SQUARE.reshape(-1, 2)
    lm = np.stack([a * q[:, 0] - b * q[:, 1] + tx, b * q[:, 0] + a * q[:, 1] + ty], 1).reshape(-1)
    got, M = api.face_chips([img], "bgr24", [0], [lm], SQUARE, cw, ch, "bgr24", matrices=True)
    assert np.array_equal(M[0] + 0.0, np.array([a, -b, tx, b, a, ty], np.float64))
    xs = [a * u - b * v + tx for u in (0, cw - 1) for v in (0, ch - 1)]
    ys = [b * u + a * v + ty for u in (0, cw - 1) for v in (0, ch - 1)]
    crop = img[min(ys):max(ys) + 1, min(xs):max(xs) + 1]
    _eq(got[0], np.rot90(crop, k))


def _case(rng, src_fmt, cw, ch):
    """Two images (pitch slack, buffers that end with the last pixel; the second with a rectangle of non-zero origin) and six
    faces: inside, rotated and reduced, half outside, wholly outside, at the rectangle's edge, enlarged."""
    a = pr.pitched(rng, 30, 41, src_fmt, 5, 3)[1]
    b = pr.pitched(rng, 26, 33, src_fmt, 0, 0)[1]
    rects = [None, (6, 4, 20, 17)]
    L = 5
    tmpl = cr.template(L, cw, ch, rng)
    s = max(cw, ch)
    faces = [(0, 9.0 / s, 17.0, (20.0, 14.0)), (0, 25.0 / s, -38.0, (19.5, 15.2)), (0, 14.0 / s, 205.0, (39.0, 2.0)),
             (0, 6.0 / s, 10.0, (-40.0, -35.0)), (1, 11.0 / s, 80.0, (1.0, 15.5)), (1, 0.4, -120.0, (9.0, 8.0))]
    fi = [f[0] for f in faces]
    lm = np.stack([cr.place(tmpl, sc, ang, c, rng, 0.3) for _, sc, ang, c in faces])
    return [a, b], rects, fi, lm, tmpl


@pytest.mark.parametrize("chip_fmt", cr.CHIP_FORMATS)
@pytest.mark.parametrize("src_fmt", pr.FORMATS)
def test_against_the_reference(api, src_fmt, chip_fmt):
    rng = np.random.default_rng(10 * src_fmt + chip_fmt)
    for k, (cw, ch) in enumerate([(1, 1), (5, 3), (16, 16), (17, 9)]):
        imgs, rects, fi, lm, tmpl = _case(rng, src_fmt, cw, ch)
        use = None if k % 2 == 0 else np.array([1, 0, 1, 1, 1], np.uint8)
        lm = lm.astype(np.float32) if k >= 2 else lm                    # real_bytes 4 and 8
        want, wm = cr.chips(imgs, [src_fmt] * 2, rects, fi, lm, tmpl, cw, ch, chip_fmt, use)
        got, gm = api.face_chips(imgs, src_fmt, fi, lm, tmpl, cw, ch, chip_fmt, rects=rects, use=use, matrices=True)
        assert same(gm, wm), (cw, ch)
        _eq(got, want)
        assert not want[3].any() and (cw * ch == 1 or want[0].any())     # wholly outside: zero
        if use is not None:                                              # the mask matters
            assert not same(gm, cr.chips(imgs, [src_fmt] * 2, rects, fi, lm, tmpl, cw, ch, chip_fmt)[1])


def test_supersampling_thresholds(api):
    """a * a + b * b exactly 1, 4, 9 and the next double above each: landmarks = a * template on points that keep every
    operation of the fit exact."""
    rng = np.random.default_rng(2)
    img = rng.integers(0, 256, (40, 48), dtype=np.uint8)
    q = np.array([0.0, 0.0, 4.0, 0.0])                                   # (two points: 4a + 4a is the only sum)
    for base, n_at, n_above in ((1.0, 1, 2), (2.0, 2, 3), (3.0, 3, 4)):
        for a, n in ((base, n_at), (math.nextafter(base, 9.0), n_above)):
            lm = q * a + 5.0 if a == base else q * a
            got, M = api.face_chips([img], "gray8", [0], [lm], q, 7, 6, "gray8", matrices=True)
            assert M[0, 0] == a and M[0, 3] == 0.0 and cr.auto_n(list(M[0])) == n
            _eq(got[0], cr.chip(img, pr.GRAY8, list(M[0]), 7, 6, cr.GRAY8, n))
            # (the n of the threshold's other side gives another chip: the test can tell them apart)
            others = [cr.chip(img, pr.GRAY8, list(M[0]), 7, 6, cr.GRAY8, m) for m in (n - 1, n + 1) if 1 <= m <= 4]
            assert all(not np.array_equal(o, got[0]) for o in others)


@pytest.mark.parametrize("n", [1, 2, 3, 4])
def test_forced_supersampling(api, n):
    rng = np.random.default_rng(3)
    img = rng.integers(0, 256, (37, 45, 3), dtype=np.uint8)
    tmpl = cr.template(4, 11, 7, rng)
    lm = np.stack([cr.place(tmpl, 2.6, 33.0, (22.0, 18.0)), cr.place(tmpl, 0.7, -71.0, (12.0, 20.0))])
    want, wm = cr.chips([img], [pr.RGB24], None, [0, 0], lm, tmpl, 11, 7, cr.BGR24, supersample=n)
    got, gm = api.face_chips([img], "rgb24", [0, 0], lm, tmpl, 11, 7, "bgr24", supersample=n, matrices=True)
    assert same(gm, wm)
    _eq(got, want)


@pytest.mark.parametrize("fmt", pr.FORMATS[1:])
def test_gray_chip_of_a_colour_image_is_the_gray_chip_of_its_packed_image(api, fmt):
    rng = np.random.default_rng(fmt)
    img = pr.pitched(rng, 33, 29, fmt, 3)[1]
    tmpl = cr.template(5, 12, 12, rng)
    lm = np.stack([cr.place(tmpl, s, ang, (14.0, 17.0)) for s, ang in ((0.8, 12.0), (1.7, -50.0), (3.4, 140.0))])
    packed = api.pack_gray([img], fmt)[0]
    _eq(api.face_chips([img], fmt, [0, 0, 0], lm, tmpl, 12, 12, "gray8"), api.face_chips([packed], "gray8", [0, 0, 0], lm, tmpl, 12, 12, "gray8"))


def test_a_detect_result_per_image(api):
    rng = np.random.default_rng(4)
    imgs = [rng.integers(0, 256, (30, 30), dtype=np.uint8) for _ in range(3)]
    tmpl = cr.template(3, 8, 8, rng)
    lm = np.stack([cr.place(tmpl, 1.2, 20.0 * i, (15.0, 15.0)) for i in range(3)]).astype(np.float32)
    results = [dict(shapes=lm[:2]), None, dict(shapes=lm[2:])]
    _eq(api.face_chips(imgs, "gray8", results, None, tmpl, 8, 8), api.face_chips(imgs, "gray8", [0, 0, 2], lm, tmpl, 8, 8))
    assert api.face_chips(imgs, "gray8", [], np.zeros((0, 6)), tmpl, 8, 8).shape == (0, 8, 8)
    assert api.lib.jdaFaceChips(None, 0, None, None, 0, 0, 0, None, None, 0, 0, 9, 9, None, None) == 0   # n_faces == 0 touches nothing


def refusals(api, a, b):
    """(what, keyword changes, words the message must hold) on a good call: two 8 x 6 BGR24 images a and b, three faces of
    three landmarks, 4 x 4 GRAY8 chips."""
    px = lambda im, **kw: api.jdaPixels(**{**dict(data=im.ctypes.data, pitch=24, width=8, height=6, format=pr.BGR24, x=0, y=0, w=0, h=0), **kw})
    lm = np.tile(np.array([1.0, 1.0, 5.0, 1.5, 3.0, 4.0]), (3, 1))
    nan, inf = lm.copy(), lm.copy()
    nan[1, 3] = np.nan; inf[2, 0] = np.inf
    tmpl = np.array([0.5, 0.5, 3.0, 1.0, 2.0, 3.0])
    bad_t = tmpl.copy(); bad_t[4] = np.inf
    same_t = np.tile([1.0, 2.0], 3)
    good = dict(images=[px(a), px(b)], n_images=2, face_image=[0, 1, 1], landmarks=lm, real_bytes=8, n_faces=3, landmark_n=3, tmpl=tmpl,
                use=None, chip_w=4, chip_h=4, chip_format=pr.GRAY8, supersample=0)
    cases = [("null images", dict(images=None), ["null images"]), ("null face_image", dict(face_image=None), ["null face_image"]),
             ("null landmarks", dict(landmarks=None), ["null landmarks"]), ("null dst", dict(dst=None), ["null destination"]),
             ("negative faces", dict(n_faces=-2), ["-2"]), ("negative images", dict(n_images=-1), ["-1"]),
             ("no landmarks", dict(landmark_n=0), ["landmark_n = 0"]),
             ("real_bytes", dict(real_bytes=2), ["real_bytes = 2"]), ("chip format", dict(chip_format=pr.BGRA32), ["chip format 3"]),
             ("chip format", dict(chip_format=-1), ["chip format -1"]), ("chip_w", dict(chip_w=0), ["0 x 4"]), ("chip_w", dict(chip_w=4097), ["4097 x 4"]),
             ("chip_h", dict(chip_h=-1), ["4 x -1"]), ("chip_h", dict(chip_h=4097), ["4 x 4097"]),
             ("supersample", dict(supersample=5), ["supersample = 5"]), ("supersample", dict(supersample=-1), ["supersample = -1"]),
             ("face_image high", dict(face_image=[0, 1, 2]), ["face 2", "face_image = 2"]), ("face_image low", dict(face_image=[0, -1, 1]), ["face 1", "face_image = -1"]),
             ("no images", dict(n_images=0), ["face 0", "face_image = 0"]),
             ("one landmark used", dict(use=[0, 1, 0]), ["face 0", "at least 2"]), ("den == 0", dict(tmpl=same_t), ["face 0", "den == 0"]),
             ("nan landmark", dict(landmarks=nan), ["face 1", "landmark 1", "not finite"]), ("inf landmark", dict(landmarks=inf), ["face 2", "landmark 0"]),
             ("inf template", dict(tmpl=bad_t), ["face 0", "template point 2"]),
             # everything check_pack refuses about an image
             ("null data", dict(images=[px(a), px(b, data=None)]), ["image 1", "null data"]),
             ("unknown format", dict(images=[px(a), px(b, format=5)]), ["image 1", "format 5"]),
             ("no width", dict(images=[px(a), px(b, width=0)]), ["image 1", "0 x 6"]),
             ("no height", dict(images=[px(a, height=-2), px(b)]), ["image 0", "8 x -2"]),
             ("w below 1", dict(images=[px(a), px(b, w=0, h=3)]), ["image 1", "(0, 0, 0, 3)"]),
             ("whole image from elsewhere", dict(images=[px(a), px(b, x=1)]), ["image 1", "(1, 0, 0, 0)"]),
             ("leaves on the right", dict(images=[px(a), px(b, x=5, w=4, h=2)]), ["image 1", "(5, 0, 4, 2)", "8 x 6"]),
             ("negative origin", dict(images=[px(a), px(b, x=-1, w=2, h=2)]), ["image 1", "(-1, 0, 2, 2)"]),
             ("pitch below a row", dict(images=[px(a), px(b, pitch=23)]), ["image 1", "pitch 23"])]
    return good, cases


def call(api, dst, mats, fn=None, head=(), tail=(), **kw):
    """The raw entry on keyword arguments of refusals(); dst / mats: addresses (or None)."""
    images = kw["images"]
    arr = None if images is None else (api.jdaPixels * len(images))(*images)
    fi = kw["face_image"]
    fi = None if fi is None else (C.c_int * len(fi))(*fi)
    lm = kw["landmarks"]
    lm = None if lm is None else np.ascontiguousarray(lm)
    t = None if kw["tmpl"] is None else np.ascontiguousarray(kw["tmpl"], np.float64)
    u = None if kw["use"] is None else np.ascontiguousarray(kw["use"], np.uint8)
    args = [arr, kw["n_images"], fi, None if lm is None else lm.ctypes.data, kw["real_bytes"], kw["n_faces"], kw["landmark_n"],
            None if t is None else t.ctypes.data_as(C.POINTER(C.c_double)), None if u is None else u.ctypes.data, kw["chip_w"], kw["chip_h"],
            kw["chip_format"], kw["supersample"], dst, None if mats is None else C.cast(mats, C.POINTER(C.c_double))]
    return (fn or api.lib.jdaFaceChips)(*head, *args, *tail)


def test_refusals_name_the_index_and_leave_dst_alone(api):
    rng = np.random.default_rng(5)
    a = rng.integers(0, 256, (6, 8, 3), dtype=np.uint8)
    b = rng.integers(0, 256, (6, 8, 3), dtype=np.uint8)
    good, cases = refusals(api, a, b)
    dst = np.full(256, 0xA5, np.uint8)
    mats = np.full(18, 7.0)
    for what, change, words in cases + [("null template", dict(tmpl=None), ["null template"])]:
        kw = {**good, **change}
        d = kw.pop("dst", dst.ctypes.data)
        assert call(api, d, mats.ctypes.data, **kw) == -1, what
        for w in words:
            assert w in api.last_error(), (what, api.last_error())
        assert (dst == 0xA5).all() and (mats == 7.0).all(), what
    # a destination on the bytes of a source image (any of them; its last byte still counts, the byte behind it does not)
    pool = np.full(1024, 0xA5, np.uint8)
    pool[:144] = a.ravel()
    for off, refused in ((0, True), (143, True), (144, False)):
        kw = {**good, "images": [api.jdaPixels(pool.ctypes.data, 24, 8, 6, pr.BGR24, 0, 0, 0, 0), good["images"][1]]}
        rc = call(api, pool.ctypes.data + off, None, **kw)
        assert rc == (-1 if refused else 0), off
        if refused:
            assert "image 0" in api.last_error() and "overlaps" in api.last_error() and (pool[144:] == 0xA5).all() and np.array_equal(pool[:144], a.ravel())
    # ... and the good call is taken
    assert call(api, dst.ctypes.data + 3, mats.ctypes.data, **good) == 0
    assert (dst[:3] == 0xA5).all() and (dst[3 + 48:] == 0xA5).all() and not (mats == 7.0).any()


def test_mean_shape(api, model_file):
    p, m = model_file((2, 8, 5, 3), 8)
    c = api.Cascador(p)
    assert same(c.mean_shape(), np.asarray(m.mean_shape, np.float64))
    assert api.lib.jdaCascadorMeanShape(c.h, None) == -1 and api.lib.jdaCascadorMeanShape(None, None) == -1
    c.close()
    p4, m4 = model_file((1, 4, 3, 2), 4)
    c = api.Cascador(p4)
    assert same(c.mean_shape(), np.asarray(m4.mean_shape, np.float32).astype(np.float64))
    c.close()
