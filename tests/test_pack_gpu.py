"""jdaPackGrayDevice (include/jda.h, "frames as they arrive"; k_pack.hip): colour, pitched and cropped device images ->
dense 8-bit gray by one kernel launch.  Every destination sits inside a patterned buffer, and the WHOLE buffer is compared
with what it must hold afterwards: the gray images of tests/pack_ref.py where they belong, the pattern everywhere else.
Every comparison is exact.  On the bounds-check build (JDA_LIB_PATH=jda_amd/libjda_bounds.so) conftest.py's autouse fixture
fails any test whose launch reported a site."""
import threading

import numpy as np
import pytest

import pack_ref as pr
from conftest import same

pytestmark = pytest.mark.gpu

WIDTHS = [1, 2, 3, 15, 16, 17, 31, 33, 47, 63, 64, 65, 100]
HEIGHTS = [1, 2, 3]


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


def on_device(flat, base, shape, strides):
    """The flat host buffer on the device and the strided view of pr.pitched into it (an allocation is 256-byte aligned, so
    `base` is the source's misalignment)."""
    import torch
    t = torch.from_numpy(flat).cuda()
    return torch.as_strided(t, shape, strides, base)


def source(rng, h, w, fmt, slack=0, base=0):
    flat, view, strides = pr.pitched(rng, h, w, fmt, slack, base)
    return view, on_device(flat, base, view.shape, strides)


def pattern(n):
    return ((np.arange(n, dtype=np.int64) * 7 + 13) % 251).astype(np.uint8)


def run(casc, views, tensors, fmts, rects=None, ts=None, dst_mis=None, hip_stream=None):
    """Packs -- with orientations ts (test_turn_gpu.py) turned -- into a patterned buffer -- image i at the first 16-byte boundary
    at least 32 bytes behind image i - 1, plus dst_mis[i] -- and compares the whole buffer, and the host form's images; returns
    the statistics."""
    import torch
    from jda_amd import api
    n = len(views)
    rects = rects or [None] * n
    if ts is None:
        want = [pr.pack(v, f, r) for v, f, r in zip(views, fmts, rects)]
    else:
        import turn_ref as tr
        want = [tr.turn(v, f, t, r) for v, f, t, r in zip(views, fmts, ts, rects)]
    offs, end = [], 0
    for i, g in enumerate(want):
        o = (end + 32 + 15) // 16 * 16 + (dst_mis[i] if dst_mis else (i * 5) % 16)
        offs.append(o)
        end = o + g.size
    expect = pattern(end + 64)
    buf = torch.from_numpy(expect.copy()).cuda()
    for o, g in zip(offs, want):
        expect[o:o + g.size] = g.ravel()
    if ts is None:
        (b, o2, ws, hs), st = casc.pack_gray_device(tensors, fmts, rects, stats=True, hip_stream=hip_stream, out=(buf, offs))
    else:
        (b, o2, ws, hs), st = casc.pack_gray_oriented_device(tensors, fmts, ts, rects, stats=True, hip_stream=hip_stream, out=(buf, offs))
    if hip_stream is None:
        torch.cuda.synchronize()
    got = buf.cpu().numpy()
    bad = np.flatnonzero(got != expect)
    assert bad.size == 0, ("first wrong byte", int(bad[0]), "of", got.size, "image offsets", offs[:8])
    assert ws == [g.shape[1] for g in want] and hs == [g.shape[0] for g in want] and list(o2) == offs
    assert st["launches"] == (1 if n else 0) and st["pixels"] == sum(g.size for g in want) == st["bytes_out"]
    assert st["bytes_in"] == sum(g.size * pr.BPP[f] for g, f in zip(want, fmts))
    host = api.pack_gray(views, fmts, rects) if ts is None else api.pack_gray_oriented(views, fmts, ts, rects)
    for h, g in zip(host, want):                                                 # device form == host form
        assert h.shape == g.shape and np.array_equal(h, g)
    return st


@pytest.mark.parametrize("fmt", pr.FORMATS)
def test_smallest_shapes(casc, fmt):
    """Narrower than a 16-byte unit, exactly one, one more, rows that units straddle; one to three rows."""
    rng = np.random.default_rng(fmt)
    srcs = [source(rng, h, w, fmt, slack=(w + h) % 4, base=(3 * w + h) % 16) for w in WIDTHS for h in HEIGHTS]
    run(casc, [s[0] for s in srcs], [s[1] for s in srcs], [fmt] * len(srcs))


@pytest.mark.parametrize("slack", [0, 1, 2, 3, 5, 64])
@pytest.mark.parametrize("fmt", [pr.BGR24, pr.GRAY8])
def test_misalignments(casc, fmt, slack):
    """Source base 0..15 x destination offset 0..15 at 47 x 3: every source shift against every head / tail length."""
    rng = np.random.default_rng(slack)
    srcs = [source(rng, 3, 47, fmt, slack, sb) for sb in range(16) for _ in range(16)]
    run(casc, [s[0] for s in srcs], [s[1] for s in srcs], [fmt] * 256, dst_mis=[i % 16 for i in range(256)])


def test_rectangles(casc):
    rng = np.random.default_rng(5)
    views, tensors, fmts, rects = [], [], [], []
    for fmt in pr.FORMATS:
        for name in sorted(pr.RECTS):
            v, t = source(rng, 21, 37, fmt, 5, 1)
            views.append(v); tensors.append(t); fmts.append(fmt); rects.append(pr.RECTS[name](37, 21))
    v, t = source(rng, 480, 640, pr.BGRA32)             # a face crop out of a frame
    views.append(v); tensors.append(t); fmts.append(pr.BGRA32); rects.append((301, 207, 48, 48))
    run(casc, views, tensors, fmts, rects)


def mixed(rng, n):
    views, tensors, fmts, rects = [], [], [], []
    for i in range(n):
        fmt = pr.FORMATS[(i * 3 + 1) % 5]
        h, w = int(rng.integers(1, 60)), int(rng.integers(1, 150))
        v, t = source(rng, h, w, fmt, int(rng.integers(0, 9)), int(rng.integers(0, 16)))
        views.append(v); tensors.append(t); fmts.append(fmt)
        rects.append(None if i % 3 else (w // 2, h // 3, w - w // 2, h - h // 3))
    return views, tensors, fmts, rects


@pytest.mark.parametrize("n", [1, 2, 5, 130])
def test_ragged_sets_are_one_launch(casc, n):
    run(casc, *mixed(np.random.default_rng(n), n))


def test_empty_set_touches_nothing(casc):
    import torch
    buf = torch.from_numpy(pattern(64)).cuda()
    (b, offs, ws, hs), st = casc.pack_gray_device([], [], stats=True, out=(buf, []))
    assert len(offs) == 0 and ws == [] and hs == [] and st["launches"] == 0 and np.array_equal(buf.cpu().numpy(), pattern(64))


def test_all_colours(casc):
    import torch
    img = pr.all_colours()
    (buf, offs, ws, hs) = casc.pack_gray_device([torch.from_numpy(img).cuda()], "bgr24")
    assert ws == [4096] and hs == [4096] and int(offs[0]) == 0
    assert np.array_equal(buf[:1 << 24].cpu().numpy().reshape(4096, 4096), pr.gray(img, pr.BGR24))


def test_source_offsets_beyond_32_bits(casc):
    """A rectangle more than 4 GB into a pitched plane: the row offset y * pitch does not fit 32 bits."""
    import torch
    pitch, rows = 1 << 20, 4100
    plane = torch.empty(rows * pitch, dtype=torch.uint8, device="cuda")
    rng = np.random.default_rng(9)
    tail = rng.integers(0, 256, (3, pitch), dtype=np.uint8)
    plane[(rows - 3) * pitch:] = torch.from_numpy(tail.reshape(-1)).cuda()
    view = torch.as_strided(plane, (rows, pitch), (pitch, 1))
    rect = (pitch - 1000 - 47, rows - 3, 47, 3)
    (buf, offs, ws, hs) = casc.pack_gray_device([view], "gray8", [rect])
    assert np.array_equal(buf[:47 * 3].cpu().numpy().reshape(3, 47), tail[:, rect[0]:rect[0] + 47])
    del view, plane
    torch.cuda.empty_cache()


def test_both_stream_forms(casc):
    import torch
    rng = np.random.default_rng(11)
    views, tensors, fmts, rects = mixed(rng, 9)
    run(casc, views, tensors, fmts, rects)                                   # hip_stream NULL: the lane's own stream
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):                                               # the pixels are produced on s, just before the call
        tensors = [t.clone() if t.is_contiguous() else t for t in tensors]
        run(casc, views, tensors, fmts, rects, hip_stream=s.cuda_stream)
    s.synchronize()


def test_two_threads_on_one_cascador(casc):
    rng = np.random.default_rng(12)
    sets = [mixed(rng, 17), mixed(rng, 23)]
    errors = []

    def work(k):
        try:
            for _ in range(6):
                run(casc, *sets[k])
        except BaseException as e:                                           # noqa: B036 (an assertion is what we are after)
            errors.append((k, repr(e)))
    threads = [threading.Thread(target=work, args=(k,)) for k in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors


def test_refusals_launch_nothing(casc):
    """Sources and destination live in ONE patterned allocation (a at byte 0, b at 1024, the destination of the host file's
    cases at 4096), which must come back as it was."""
    import ctypes as C
    import torch
    from jda_amd import api
    from test_pack_host import refusals
    pool = torch.from_numpy(pattern(8192)).cuda()
    base = pool.data_ptr()

    class Dev:                                                               # what refusals() reads of an image: address and shape
        def __init__(self, address):
            self.shape = (6, 8, 3)
            self.ctypes = type("P", (), {"data": address})
    for what, px, offs, n, words in refusals(api, Dev(base), Dev(base + 1024)):
        arr = (api.jdaPixels * len(px))(*px)
        st = api.jdaPackStats(launches=7)
        rc = api.lib.jdaPackGrayDevice(casc.h, arr, n, C.c_void_p(base + 4096), (C.c_size_t * len(offs))(*offs), None, C.byref(st))
        assert rc == -1 and st.launches == 7, what                           # (the statistics are not touched either)
        for w in words:
            assert w in api.last_error(), (what, api.last_error())
    two = (api.jdaPixels * 2)(api.jdaPixels(base, 24, 8, 6, pr.BGR24, 0, 0, 0, 0), api.jdaPixels(base + 1024, 24, 8, 6, pr.BGR24, 0, 0, 0, 0))
    good = (C.c_size_t * 2)(4096, 5000)
    for args in ((None, two, 2, C.c_void_p(base), good), (casc.h, None, 2, C.c_void_p(base), good), (casc.h, two, 2, None, good),
                 (casc.h, two, 2, C.c_void_p(base), None)):
        assert api.lib.jdaPackGrayDevice(*args, None, None) == -1 and "null" in api.last_error()
    # the destination inside the source rows: of the image itself (first and last byte of them), and of another image
    for offs, words in (((40, 5000), ["image 0", "source rows of image 0"]), ((5000, 1024 + 143), ["image 1", "source rows of image 1"]),
                        ((5000, 100), ["image 1", "source rows of image 0"]), ((1024 - 47, 5000), ["image 0", "source rows of image 1"])):
        assert api.lib.jdaPackGrayDevice(casc.h, two, 2, C.c_void_p(base), (C.c_size_t * 2)(*offs), None, None) == -1
        for w in words:
            assert w in api.last_error(), (offs, api.last_error())
    # ... and right behind them it is taken
    assert api.lib.jdaPackGrayDevice(casc.h, two, 2, C.c_void_p(base), (C.c_size_t * 2)(144, 1024 + 144), None, None) == 0
    torch.cuda.synchronize()
    want = pattern(8192)
    for k in (0, 1024):
        src = want[k:k + 144].reshape(6, 8, 3).copy()
        want[k + 144:k + 192] = pr.gray(src, pr.BGR24).ravel()
    assert np.array_equal(pool.cpu().numpy(), want)


# ---- end to end on a synthetic model ------------------------------------------------------------------------------------

def colour_of(gray, rng, fmt):
    """A colour image around a synthetic gray frame: every channel the frame plus a little noise of its own."""
    ch = [np.clip(gray.astype(np.int16) + rng.integers(-6, 7, gray.shape), 0, 255).astype(np.uint8) for _ in range(pr.BPP[fmt])]
    return np.ascontiguousarray(np.stack(ch, -1))


def _eq_c(a, b):
    for k in ("bboxes", "scores", "shapes"):
        assert same(a[k], b[k]), k


def _eq_cpp(a, b):
    for k in ("rects", "scores", "shapes"):
        assert same(a[k], b[k]), k


def test_colour_frames_into_the_batch_entry(built, gpu, model_file):
    import torch
    from jda_amd import api, synth
    p, _ = model_file((3, 20, 5, 4), 4, seed=3, cart_th=-1.0)
    c = api.Cascador(p)
    rng = np.random.default_rng(21)
    frames = synth.make_frames(4, 160, 120, seed=5)
    colour = [colour_of(f, rng, pr.BGRA32) for f in frames]
    want = c.detect_batch(np.stack([pr.gray(x, pr.BGRA32) for x in colour]), min_size=24)
    assert sum(len(w["scores"]) for w in want) > 0
    buf, offs, ws, hs = c.pack_gray_device([torch.from_numpy(x).cuda() for x in colour], "bgra32", frame_stride=160 * 120)
    assert list(offs) == [i * 160 * 120 for i in range(4)]
    got = c.detect_batch_device(buf.view(4, 120, 160), min_size=24)
    for a, b in zip(got, want):
        _eq_c(a, b)
    c.close()


def test_packed_set_into_the_ragged_entries(built, gpu, model_file):
    import torch
    from jda_amd import api, synth
    p, _ = model_file((3, 20, 5, 4), 8, seed=3, cart_th=-1.0, norm_every=5)
    c = api.Cascador(p)
    rng = np.random.default_rng(22)
    sizes = [(200, 150), (131, 97), (64, 48), (47, 200), (161, 159)]
    fmts = [pr.RGB24, pr.BGRA32, pr.BGR24, pr.RGBA32, pr.RGB24]
    colour = [colour_of(synth.make_frames(1, w, h, seed=11, first=i)[0], rng, f) for i, ((w, h), f) in enumerate(zip(sizes, fmts))]
    grays = [pr.gray(x, f) for x, f in zip(colour, fmts)]
    packed = c.pack_gray_device([torch.from_numpy(x).cuda() for x in colour], fmts)
    want_c, want_cpp = c.detect_ragged(grays, min_size=24), c.detect_ragged_cpp(grays)
    assert sum(len(w["scores"]) for w in want_c) > 0 and sum(len(w["scores"]) for w in want_cpp) > 0
    for a, b in zip(c.detect_ragged_packed(*packed, min_size=24), want_c):
        _eq_c(a, b)
    for a, b in zip(c.detect_ragged_cpp_packed(*packed), want_cpp):
        _eq_cpp(a, b)
    c.close()


def test_fddb_fold_from_pixels(built, gpu, model_file):
    from jda_amd import api, fddb, synth
    p, _ = model_file((3, 20, 5, 4), 8, seed=3, cart_th=-1.0, norm_every=5)
    c = api.Cascador(p)
    rng = np.random.default_rng(23)
    rgbs = [colour_of(synth.make_frames(1, w, h, seed=13, first=i)[0], rng, pr.RGB24) for i, (w, h) in enumerate([(180, 140), (97, 131), (210, 90)])]
    for dialect in ("cpp", "c"):
        grays = [fddb.bgr2gray(x) for x in rgbs]
        want, st_w = fddb.detect_fold_ragged_cpp(c, grays) if dialect == "cpp" else fddb.detect_fold_ragged(c, grays)
        got, st_g = fddb.detect_fold_ragged_pixels(c, rgbs, dialect)
        assert sum(len(w[1]) for w in want) > 0 and st_g["patch_n"] == st_w["patch_n"]
        for a, b in zip(got, want):
            assert all(same(x, y) for x, y in zip(a, b))
    c.close()


def test_positives_from_a_packed_set(built, gpu, model_file):
    import torch
    from jda_amd import api, synth
    p, _ = model_file((1, 2, 5, 3))
    c = api.Cascador(p, "double", device=0)
    rng = np.random.default_rng(24)
    colour = [colour_of(synth.make_frames(1, w, h, seed=17, first=i)[0], rng, pr.BGR24) for i, (w, h) in enumerate([(150, 120), (90, 140)])]
    faces = [(0, 20, 10, 80, 80), (1, -5, 30, 70, 70)]                        # (image, x, y, w, h); the second leaves its image
    want = c.build_positives_cpp([pr.gray(x, pr.BGR24) for x in colour], faces)
    got = c.build_positives_cpp(c.pack_gray_device([torch.from_numpy(x).cuda() for x in colour], "bgr24"), faces)
    assert want.any() and np.array_equal(got, want)
    c.close()
