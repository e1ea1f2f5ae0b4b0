"""jdaPackGray (include/jda.h, "frames as they arrive"): colour, pitched and cropped host images -> dense 8-bit gray, without
a GPU.  Every comparison is exact, against the definition restated in tests/pack_ref.py."""
import ctypes as C

import numpy as np
import pytest

import pack_ref as pr


@pytest.fixture(scope="module")
def api(built):
    from jda_amd import api
    return api


def _eq(got, want):
    assert got.shape == want.shape and got.dtype == np.uint8 and np.array_equal(got, want)


def test_all_colours(api):
    img = pr.all_colours()
    want = pr.gray(img, pr.BGR24)
    _eq(api.pack_gray([img], "bgr24")[0], want)
    _eq(api.pack_gray([img], "rgb24")[0], pr.gray(img, pr.RGB24))
    # the extremes of the definition, by hand
    assert want[0, 0] == 0 and want[-1, -1] == 255 and want[0, 255] == (255 * 1868 + 8192) >> 14


def test_agrees_with_the_fddb_harness_conversion(api):
    from jda_amd import fddb
    rgb = np.random.default_rng(1).integers(0, 256, (61, 47, 3), dtype=np.uint8)
    _eq(fddb.bgr2gray(rgb), pr.gray(rgb, pr.RGB24))
    _eq(api.pack_gray([rgb], api.JDA_PIX_RGB24)[0], fddb.bgr2gray(rgb))


@pytest.mark.parametrize("fmt", pr.FORMATS)
def test_formats_and_alpha(api, fmt):
    rng = np.random.default_rng(fmt)
    img = rng.integers(0, 256, pr.shape_of(37, 53, fmt), dtype=np.uint8)
    _eq(api.pack_gray([img], fmt)[0], pr.gray(img, fmt))
    if pr.BPP[fmt] == 4:                                 # alpha does not matter
        other = img.copy()
        other[..., 3] = rng.integers(0, 256, other.shape[:2], dtype=np.uint8)
        _eq(api.pack_gray([other], fmt)[0], pr.gray(img, fmt))
        three = pr.BGR24 if fmt == pr.BGRA32 else pr.RGB24
        _eq(api.pack_gray([img], fmt)[0], pr.gray(img[..., :3], three))


@pytest.mark.parametrize("slack", [0, 1, 3, 64])
def test_pitch(api, slack):
    rng = np.random.default_rng(slack)
    for fmt in pr.FORMATS:
        for base in (0, 1):
            _, view, _ = pr.pitched(rng, 9, 31, fmt, slack, base)
            _eq(api.pack_gray([view], fmt)[0], pr.gray(view, fmt))


@pytest.mark.parametrize("name", sorted(pr.RECTS))
def test_rectangles(api, name):
    rng = np.random.default_rng(7)
    for fmt in pr.FORMATS:
        _, view, _ = pr.pitched(rng, 21, 37, fmt, 5)
        rect = pr.RECTS[name](37, 21)
        _eq(api.pack_gray([view], fmt, [rect])[0], pr.pack(view, fmt, rect))


def _mixed(rng, n):
    imgs, fmts, rects = [], [], []
    for i in range(n):
        fmt = pr.FORMATS[i % 5]
        h, w = int(rng.integers(1, 40)), int(rng.integers(1, 70))
        imgs.append(pr.pitched(rng, h, w, fmt, int(rng.integers(0, 9)))[1])
        fmts.append(fmt)
        rects.append(None if i % 3 else (w // 2, h // 3, w - w // 2, h - h // 3))
    return imgs, fmts, rects


@pytest.mark.parametrize("n", [0, 1, 7])
def test_sets_of_mixed_formats_and_sizes(api, n):
    imgs, fmts, rects = _mixed(np.random.default_rng(n), n)
    got = api.pack_gray(imgs, fmts, rects)
    assert len(got) == n
    for g, im, f, r in zip(got, imgs, fmts, rects):
        _eq(g, pr.pack(im, f, r))
    if n == 0:                                           # touches nothing: not even a NULL destination
        assert api.lib.jdaPackGray(None, 0, None, None) == 0


def _px(api, a, fmt, rect=(0, 0, 0, 0), pitch=None, width=None, height=None, data=True):
    bpp = pr.BPP[fmt] if fmt in pr.BPP else 1
    return api.jdaPixels(a.ctypes.data if data else None, a.shape[1] * bpp if pitch is None else pitch,
                         a.shape[1] if width is None else width, a.shape[0] if height is None else height, fmt, *rect)


def refusals(api, a, b):
    """(what, jdaPixels list, dst offsets, words the message must hold) for two 8 x 6 BGR24 images a and b; the destination is
    bytes [64, 64 + 2 * 48) of the caller's buffer unless the case says otherwise."""
    ok = lambda: [_px(api, a, pr.BGR24), _px(api, b, pr.BGR24)]
    cases = []

    def case(what, second, words, offs=(64, 112), n=2):
        px = ok()
        if second is not None:
            px[1] = second
        cases.append((what, px, list(offs), n, words))
    case("null data", _px(api, b, pr.BGR24, data=False), ["image 1", "null"])
    case("negative n", None, ["-3"], n=-3)
    case("unknown format", _px(api, b, 5), ["image 1", "format 5"])
    case("negative format", _px(api, b, -1), ["image 1", "format -1"])
    case("no width", _px(api, b, pr.BGR24, width=0), ["image 1", "0 x 6"])
    case("no height", _px(api, b, pr.BGR24, height=-2), ["image 1", "8 x -2"])
    case("w below 1", _px(api, b, pr.BGR24, (0, 0, 0, 3)), ["image 1", "(0, 0, 0, 3)"])
    case("h below 1", _px(api, b, pr.BGR24, (1, 1, 2, -1)), ["image 1", "(1, 1, 2, -1)"])
    case("leaves on the right", _px(api, b, pr.BGR24, (5, 0, 4, 2)), ["image 1", "(5, 0, 4, 2)", "8 x 6"])
    case("leaves below", _px(api, b, pr.BGR24, (0, 5, 1, 2)), ["image 1", "(0, 5, 1, 2)"])
    case("negative origin", _px(api, b, pr.BGR24, (-1, 0, 2, 2)), ["image 1", "(-1, 0, 2, 2)"])
    case("pitch below a row", _px(api, b, pr.BGR24, pitch=23), ["image 1", "pitch 23"])
    case("destinations overlap", None, ["image 0", "image 1", "overlap"], offs=(64, 111))
    return cases


def test_refusals_name_the_image_and_leave_dst_alone(api):
    rng = np.random.default_rng(3)
    a = rng.integers(0, 256, (6, 8, 3), dtype=np.uint8)
    b = rng.integers(0, 256, (6, 8, 3), dtype=np.uint8)
    for what, px, offs, n, words in refusals(api, a, b):
        dst = np.full(256, 0xA5, np.uint8)
        arr = (api.jdaPixels * len(px))(*px)
        o = (C.c_size_t * len(offs))(*offs)
        assert api.lib.jdaPackGray(arr, n, dst.ctypes.data, o) == -1, what
        for w in words:
            assert w in api.last_error(), (what, api.last_error())
        assert (dst == 0xA5).all(), what
    arr = (api.jdaPixels * 2)(_px(api, a, pr.BGR24), _px(api, b, pr.BGR24))
    o = (C.c_size_t * 2)(64, 112)
    dst = np.full(256, 0xA5, np.uint8)
    for args in ((None, 2, dst.ctypes.data, o), (arr, 2, None, o), (arr, 2, dst.ctypes.data, None)):
        assert api.lib.jdaPackGray(*args) == -1 and "null" in api.last_error()
    assert (dst == 0xA5).all()
    # a destination inside the source rows of ANOTHER image (in place is refused as well)
    src = rng.integers(0, 256, 6 * 24 + 48, dtype=np.uint8)
    keep = src.copy()
    arr = (api.jdaPixels * 2)(_px(api, a, pr.BGR24), api.jdaPixels(src.ctypes.data, 24, 8, 6, pr.BGR24, 0, 0, 0, 0))
    o = (C.c_size_t * 2)(6 * 24 + 0, 40)                # image 1's own destination lies in its source rows, image 0's behind them
    assert api.lib.jdaPackGray(arr, 2, src.ctypes.data, o) == -1
    assert "image 1" in api.last_error() and "source rows" in api.last_error() and np.array_equal(src, keep)
    # ... while the slack between the rows of a pitched source is free: 4 x 1 pixels into the 8 spare bytes of row 0
    wide = rng.integers(0, 256, 6 * 32, dtype=np.uint8)
    arr = (api.jdaPixels * 1)(api.jdaPixels(wide.ctypes.data, 32, 8, 6, pr.BGR24, 0, 0, 4, 1))
    want = pr.pack(np.lib.stride_tricks.as_strided(wide, (6, 8, 3), (32, 3, 1)), pr.BGR24, (0, 0, 4, 1))
    assert api.lib.jdaPackGray(arr, 1, wide.ctypes.data, (C.c_size_t * 1)(24)) == 0 and np.array_equal(wide[24:28], want[0])
