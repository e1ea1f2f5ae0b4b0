"""jdaFaceChipsDevice (include/jda.h, "faces as they leave"; k_chips.hip): upright face chips cut from device images by one
kernel launch.  The destination sits inside a patterned buffer at an odd address, and the WHOLE buffer is compared with what
it must hold afterwards: the chips of tests/chips_ref.py (which the host form must give as well) where they belong, the
pattern in the guard bytes before and after.  Every comparison is exact.  On the bounds-check build
(JDA_LIB_PATH=jda_amd/libjda_bounds.so) conftest.py's autouse fixture fails any test whose launch reported a site."""
import ctypes as C
import threading

import numpy as np
import pytest

import chips_ref as cr
import pack_ref as pr
from conftest import same

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    return torch.device("cuda", 0)


@pytest.fixture()
def casc(built, gpu, model_file):
    from jda_amd import api
    p, _ = model_file((2, 8, 5, 3), 8)
    c = api.Cascador(p)
    yield c
    c.close()


def pattern(n):
    return ((np.arange(n, dtype=np.int64) * 7 + 13) % 251).astype(np.uint8)


def source(rng, h, w, fmt, slack, base):
    """A source whose buffer -- on the device its ALLOCATION -- ends with its last pixel: (host view, flat buffer, strides, base)."""
    flat, view, strides = pr.pitched(rng, h, w, fmt, slack, base)
    return view, flat, strides, base


def on_device(srcs):
    """-> (host view, device view of the same strides) per source (an allocation is 256-byte aligned: `base` is the misalignment)."""
    import torch
    return [(view, torch.as_strided(torch.from_numpy(flat).cuda(), view.shape, strides, base)) for view, flat, strides, base in srcs]


# scale = source pixels per chip pixel: 0.97 | 1.04 (n 1 | 2), 1.96 | 2.05 (2 | 3), 2.95 | 3.06 (3 | 4), and an enlargement
# at the corner of the smallest image
FACES = [(1, 0.97, 14.0, (30.0, 22.0)), (1, 1.04, -33.0, (36.0, 25.0)), (2, 1.96, 47.0, (25.0, 19.0)), (2, 2.05, 171.0, (24.0, 21.0)),
         (1, 2.95, -101.0, (35.0, 24.0)), (1, 3.06, 62.0, (33.0, 26.0)), (0, 0.55, 29.0, (32.0, 0.5))]


def ragged_host(cw, ch):
    """3 images of different sizes and formats (33 x 21 up to 97 x 64; the second with a rectangle) and 7 faces: rotations
    that are no multiple of 90 degrees, scales on both sides of every threshold of n (the landmarks' noise, 0.1 % of the
    face's size, keeps the fitted scale on its side), one face half outside its image."""
    rng = np.random.default_rng(31)
    srcs = [source(rng, 21, 33, pr.GRAY8, 3, 1), source(rng, 64, 97, pr.BGRA32, 0, 0), source(rng, 40, 51, pr.RGB24, 7, 5)]
    fmts, rects = [pr.GRAY8, pr.BGRA32, pr.RGB24], [None, (10, 6, 70, 50), None]
    tmpl = cr.template(5, cw, ch, rng)
    lm = np.stack([cr.place(tmpl, sc, ang, c, rng, 0.001 * sc * max(cw, ch)) for _, sc, ang, c in FACES])
    return srcs, fmts, rects, [f[0] for f in FACES], lm, tmpl


def ragged_set(cw, ch):
    s = ragged_host(cw, ch)
    return (on_device(s[0]),) + s[1:]


def run(casc, srcs, fmts, rects, fi, lm, tmpl, cw, ch, chip_fmt, mis=1, hip_stream=None, want=None, **kw):
    """Chips into a patterned buffer, 64 guard bytes in front and behind, the destination `mis` bytes behind a 256-byte
    boundary; compares the whole buffer, the matrices, the host form and the statistics; returns the reference."""
    import torch
    from jda_amd import api
    views, tensors = [s[0] for s in srcs], [s[1] for s in srcs]
    if want is None:
        want = cr.chips(views, fmts, rects, fi, lm, tmpl, cw, ch, chip_fmt, kw.get("use"), kw.get("supersample", 0))
    chips, mats = want
    host, hm = api.face_chips(views, fmts, fi, lm, tmpl, cw, ch, chip_fmt, rects=rects, matrices=True, **kw)
    assert np.array_equal(host, chips) and same(hm, mats)
    nbytes = chips.size
    expect = pattern(256 + mis + nbytes + 64)
    buf = torch.from_numpy(expect.copy()).cuda()
    assert buf.data_ptr() % 256 == 0
    expect[256 + mis:256 + mis + nbytes] = chips.ravel()
    out = buf[256 + mis:256 + mis + nbytes]
    got, gm, st = casc.face_chips_device(tensors, fmts, fi, lm, tmpl, cw, ch, chip_fmt, rects=rects, matrices=True, stats=True,
                                         hip_stream=hip_stream, out=out, **kw)
    if hip_stream is None:
        torch.cuda.synchronize()
    res = buf.cpu().numpy()
    bad = np.flatnonzero(res != expect)
    assert bad.size == 0, ("first wrong byte", int(bad[0]) - 256 - mis, "of", nbytes, "chip bytes", chips[0].size)
    assert same(gm, mats) and got.shape == chips.shape and got.data_ptr() == out.data_ptr()
    ns = [kw.get("supersample") or cr.auto_n(list(m)) for m in mats]
    assert st["launches"] == (1 if len(fi) else 0) and st["faces"] == len(fi) and st["chip_bytes"] == nbytes
    assert st["taps"] == sum(cw * ch * n * n * 4 for n in ns)
    if len(fi):
        assert st["device_ms"] > 0 and st["call_ms"] >= st["device_ms"]
    return want, ns


@pytest.fixture(scope="module")
def small():
    """The ragged set with 5 x 3 BGR24 chips (45 bytes: every chip starts unaligned) and its reference, computed once."""
    s = ragged_set(5, 3)
    views = [x[0] for x in s[0]]
    return s, cr.chips(views, s[1], s[2], s[3], s[4], s[5], 5, 3, cr.BGR24)


def test_ragged_set_of_45_byte_chips_at_an_odd_address(casc, small):
    s, want = small
    _, ns = run(casc, *s, 5, 3, cr.BGR24, mis=1, want=want)
    assert ns[:6] == [1, 2, 2, 3, 3, 4]


@pytest.mark.parametrize("mis", [0, 3, 15, 16 + 9])
def test_every_head_and_tail(casc, small, mis):
    s, want = small
    run(casc, *s, 5, 3, cr.BGR24, mis=mis, want=want)


@pytest.mark.parametrize("chip_fmt", cr.CHIP_FORMATS)
def test_chip_formats_and_sizes(casc, chip_fmt):
    """16 x 16 (units inside a row, more than one workgroup for colour chips), 17 x 9 (units that straddle rows and chips), 1 x 1."""
    for cw, ch in ((16, 16), (17, 9), (1, 1)):
        run(casc, *ragged_set(cw, ch), cw, ch, chip_fmt, mis=7)


def test_masks_float_landmarks_and_forced_n(casc):
    s = ragged_set(8, 8)
    srcs, fmts, rects, fi, lm, tmpl = s
    run(casc, srcs, fmts, rects, fi, lm.astype(np.float32), tmpl, 8, 8, cr.GRAY8, use=np.array([1, 1, 0, 1, 0], np.uint8))
    run(casc, srcs, fmts, rects, fi, lm, tmpl, 8, 8, cr.RGB24, supersample=3)


def test_one_large_chip_at_a_fourfold_reduction(casc):
    """64 x 64 at 4x and 30 degrees out of 300 x 280 BGR24: 256 source pixels across, n = 4, 3 workgroups."""
    rng = np.random.default_rng(32)
    srcs = on_device([source(rng, 280, 300, pr.BGR24, 4, 2)])
    tmpl = cr.template(5, 64, 64, rng)
    lm = cr.place(tmpl, 4.0, 30.0, (150.0, 140.0), rng, 0.5)[None]
    _, ns = run(casc, srcs, [pr.BGR24], None, [0], lm, tmpl, 64, 64, cr.RGB24, mis=5)
    assert ns == [4]


def test_empty_set_touches_nothing(casc):
    import torch
    buf = torch.from_numpy(pattern(64)).cuda()
    got, mats, st = casc.face_chips_device([], [], [], np.zeros((0, 10)), None, 5, 3, "bgr24", matrices=True, stats=True, out=buf[:0])
    assert got.shape == (0, 3, 5, 3) and mats.shape == (0, 6) and st["launches"] == 0 and np.array_equal(buf.cpu().numpy(), pattern(64))


def test_a_user_stream(casc, small):
    import torch
    s, want = small
    srcs = s[0]
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):                                              # the pixels are produced on st, just before the call
        srcs = [(v, t.clone() if t.is_contiguous() else t) for v, t in srcs]
        run(casc, srcs, *s[1:], 5, 3, cr.BGR24, hip_stream=st.cuda_stream, want=want)
    st.synchronize()


def test_two_threads_on_one_cascador(casc, small):
    s, want = small
    s2 = ragged_set(17, 9)
    want2 = cr.chips([x[0] for x in s2[0]], s2[1], s2[2], s2[3], s2[4], s2[5], 17, 9, cr.GRAY8)
    jobs = [(s, 5, 3, cr.BGR24, want), (s2, 17, 9, cr.GRAY8, want2)]
    errors = []

    def work(k):
        try:
            st, cw, ch, f, w = jobs[k]
            for _ in range(6):
                run(casc, *st, cw, ch, f, mis=1 + k, want=w)
        except BaseException as e:                                           # noqa: B036 (an assertion is what we are after)
            errors.append((k, repr(e)))
    threads = [threading.Thread(target=work, args=(k,)) for k in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors


def test_default_template_is_the_mean_shape_at_the_chip_size(casc):
    rng = np.random.default_rng(33)
    ms = casc.mean_shape()
    cw, ch = 12, 10
    tmpl = ms * np.tile([float(cw), float(ch)], len(ms) // 2)
    srcs = on_device([source(rng, 50, 60, pr.BGR24, 0, 0)])
    lm = np.stack([cr.place(tmpl, 1.5, 21.0, (30.0, 26.0), rng, 0.4), cr.place(tmpl, 0.8, -15.0, (28.0, 22.0), rng, 0.4)])
    want = cr.chips([srcs[0][0]], [pr.BGR24], None, [0, 0], lm, tmpl, cw, ch, cr.BGR24)
    got, mats = casc.face_chips_device([srcs[0][1]], "bgr24", [0, 0], lm, None, cw, ch, "bgr24", matrices=True)
    assert np.array_equal(got.cpu().numpy(), want[0]) and same(mats, want[1])
    # ... and a detect() result per image goes in as it is
    got2 = casc.face_chips_device([srcs[0][1]], "bgr24", [dict(shapes=lm.astype(np.float32))], None, None, cw, ch, "bgr24")
    want2 = cr.chips([srcs[0][0]], [pr.BGR24], None, [0, 0], lm.astype(np.float32), tmpl, cw, ch, cr.BGR24)
    assert np.array_equal(got2.cpu().numpy(), want2[0])
    from jda_amd import api
    with pytest.raises(api.JdaError, match="the model has 5 landmarks"):
        casc.face_chips_device([srcs[0][1]], "bgr24", [0], lm[:1, :8], None, cw, ch, "bgr24")


def test_refusals_launch_nothing(casc):
    """Sources and destination live in ONE patterned allocation (a at byte 0, b at 1024, the destination at 4096), which must
    come back as it was."""
    import torch
    from jda_amd import api
    from test_chips_host import call, refusals
    pool = torch.from_numpy(pattern(8192)).cuda()
    base = pool.data_ptr()

    class Dev:                                                               # what refusals() reads of an image: its address
        def __init__(self, address):
            self.ctypes = type("P", (), {"data": address})
    good, cases = refusals(api, Dev(base), Dev(base + 1024))
    mats = np.full(18, 7.0)
    fn = api.lib.jdaFaceChipsDevice
    for what, change, words in cases:
        kw = {**good, **change}
        d = kw.pop("dst", base + 4096)
        st = api.jdaChipStats(launches=7)
        assert call(api, d, mats.ctypes.data, fn, (casc.h,), (None, C.byref(st)), **kw) == -1 and st.launches == 7, what
        for w in words:
            assert w in api.last_error(), (what, api.last_error())
        assert (mats == 7.0).all(), what
    assert call(api, base + 4096, None, fn, (None,), (None, None), **good) == -1 and "null cascador" in api.last_error()
    assert call(api, base + 4096, None, fn, (casc.h,), (None, None), **{**good, "tmpl": None}) == -1 and "the model has 5" in api.last_error()
    for off, image in ((100, 0), (143, 0), (1024 - 47, 1), (1024 + 143, 1)):      # the destination on an image's bytes
        assert call(api, base + off, None, fn, (casc.h,), (None, None), **good) == -1
        assert "image %d" % image in api.last_error() and "overlaps" in api.last_error()
    torch.cuda.synchronize()
    assert np.array_equal(pool.cpu().numpy(), pattern(8192))
    # ... and right behind an image it is taken
    assert call(api, base + 144, mats.ctypes.data, fn, (casc.h,), (None, None), **good) == 0
    torch.cuda.synchronize()
    want = pattern(8192)
    imgs = [want[k:k + 144].reshape(6, 8, 3).copy() for k in (0, 1024)]
    chips, wm = cr.chips(imgs, [pr.BGR24] * 2, None, good["face_image"], good["landmarks"], good["tmpl"], 4, 4, cr.GRAY8)
    want[144:144 + 48] = chips.ravel()
    assert np.array_equal(pool.cpu().numpy(), want) and same(mats.reshape(3, 6), wm)
