"""jdaPackGrayReducedDevice (include/jda.h, "frames larger than the faces need"; k_reduce.hip): colour, pitched and cropped
device images -> dense 8-bit gray, reduced by an integer factor and turned, by one kernel launch.  As in test_turn_gpu.py every
destination sits inside a patterned buffer and the WHOLE buffer is compared with what it must hold afterwards -- the images of
tests/reduce_ref.py where they belong, the pattern everywhere else -- and the host form must give the same bytes.  Every
comparison is exact.  On the bounds-check build (JDA_LIB_PATH=jda_amd/libjda_bounds.so) conftest.py's autouse fixture fails
any test whose launch reported a site."""
import threading

import numpy as np
import pytest

import pack_ref as pr
import reduce_ref as rr
import turn_ref as tr
from conftest import same
from mining_ref import transform
from test_pack_gpu import pattern, source

pytestmark = pytest.mark.gpu

# reduced sizes: narrower than a unit, than a tile, exactly a tile, and one more
SIZES = [(w, h) for w in (1, 2, 3, 15, 16, 17, 63, 64, 65) for h in (1, 2, 63, 64, 65)]


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


def run(casc, views, tensors, fmts, fs, ts=None, rects=None, dst_mis=None, hip_stream=None):
    """Packs reduced by fs and turned by ts (None: upright, orients NULL) into a patterned buffer -- image i at the first 16-byte
    boundary at least 32 bytes behind image i - 1, plus dst_mis[i] -- and compares the whole buffer, and the host form's
    images; returns the statistics."""
    import torch
    from jda_amd import api
    n = len(views)
    rects = rects or [None] * n
    want = [rr.reduce(v, fm, f, t, r) for v, fm, f, t, r in zip(views, fmts, fs, ts or [0] * n, rects)]
    offs, end = [], 0
    for i, g in enumerate(want):
        o = (end + 32 + 15) // 16 * 16 + (dst_mis[i] if dst_mis else (i * 5) % 16)
        offs.append(o)
        end = o + g.size
    expect = pattern(end + 64)
    buf = torch.from_numpy(expect.copy()).cuda()
    for o, g in zip(offs, want):
        expect[o:o + g.size] = g.ravel()
    (b, o2, ws, hs), st = casc.pack_gray_reduced_device(tensors, fmts, fs, ts, rects, stats=True, hip_stream=hip_stream, out=(buf, offs))
    if hip_stream is None:
        torch.cuda.synchronize()
    got = buf.cpu().numpy()
    bad = np.flatnonzero(got != expect)
    assert bad.size == 0, ("first wrong byte", int(bad[0]), "of", got.size, "image offsets", offs[:8])
    assert ws == [g.shape[1] for g in want] and hs == [g.shape[0] for g in want] and list(o2) == offs
    assert st["launches"] == (1 if n else 0) and st["pixels"] == sum(g.size for g in want) == st["bytes_out"]
    assert st["bytes_in"] == sum(g.size * f * f * pr.BPP[fm] for g, f, fm in zip(want, fs, fmts))
    host = api.pack_gray_reduced(views, fmts, fs, ts, rects)
    for h, g in zip(host, want):                                                 # device form == host form
        assert h.shape == g.shape and np.array_equal(h, g)
    return st


@pytest.mark.parametrize("shift", range(5))
def test_every_factor_orientation_and_format_in_one_call(casc, shift):
    """Every factor x orientation x format in ONE ragged call, the reduced sizes dealt round from SIZES (every size seven
    times a call, with other partners in every case); the sources are those times f plus 0 .. f - 1 dropped columns and rows."""
    rng = np.random.default_rng(shift)
    srcs, fmts, fs, ts = [], [], [], []
    for f in rr.FACTORS:
        for t in tr.ORIENTS:
            for fmt in pr.FORMATS:
                k = len(srcs)
                rw, rh = SIZES[(7 * k + 11 * shift) % len(SIZES)]
                w, h = rw * f + (k + shift) % f, rh * f + (k // 3 + shift) % f
                srcs.append(source(rng, h, w, fmt, slack=(w + h) % 4, base=(3 * w + h + t) % 16)); fmts.append(fmt); fs.append(f); ts.append(t)
    st = run(casc, [s[0] for s in srcs], [s[1] for s in srcs], fmts, fs, ts)
    assert st["launches"] == 1


@pytest.mark.parametrize("fmt", [pr.BGR24, pr.GRAY8])
@pytest.mark.parametrize("t", [0, 1, 4])
@pytest.mark.parametrize("f", [3, 8])
@pytest.mark.parametrize("wh", [(47, 3), (3, 47)])
def test_misalignments(casc, wh, f, t, fmt):
    """Source base 0..15 x destination offset 0..15: every source shift against every head / tail length of every turned row."""
    rng = np.random.default_rng(t)
    srcs = [source(rng, wh[1] * f + sb % f, wh[0] * f + (sb // 2) % f, fmt, sb % 3, sb) for sb in range(16) for _ in range(16)]
    run(casc, [s[0] for s in srcs], [s[1] for s in srcs], [fmt] * 256, [f] * 256, [t] * 256, dst_mis=[i % 16 for i in range(256)])


def test_rectangles(casc):
    rng = np.random.default_rng(5)
    views, tensors, fmts, rects, fs, ts = [], [], [], [], [], []
    for fmt in pr.FORMATS:
        for f in (2, 3, 5):
            for t in (0, 1, 6):
                v, d = source(rng, 21 * f, 37 * f, fmt, 5, 1)
                r = pr.RECTS["interior"](37 * f, 21 * f)
                views.append(v); tensors.append(d); fmts.append(fmt); rects.append((r[0], r[1], r[2] + t % 4, r[3] + 1)); fs.append(f); ts.append(t)
    v, d = source(rng, 300, 400, pr.BGRA32)             # a crop of more than one tile out of a frame
    views.append(v); tensors.append(d); fmts.append(pr.BGRA32); rects.append((101, 7, 297, 290)); fs.append(2); ts.append(3)
    run(casc, views, tensors, fmts, fs, ts, rects)


def test_source_ends_with_its_allocation(casc):
    """The last pixel that takes part is the allocation's last byte -- no dropped row, the dropped columns are the pitch's
    slack --, every start alignment, every factor and format (under the bounds-check build every dword read must hold a byte
    of a pixel that takes part)."""
    rng = np.random.default_rng(6)
    srcs, fmts, fs, ts = [], [], [], []
    for fmt in pr.FORMATS:
        for f in rr.FACTORS:
            for rw, rh in ((67, 2), (5, 9), (2, 3)):
                t = (f + rw) % 8
                srcs.append(source(rng, rh * f, rw * f, fmt, (f + rw) % 3 * pr.BPP[fmt], (t + rw) % 4)); fmts.append(fmt); fs.append(f); ts.append(t)
    run(casc, [s[0] for s in srcs], [s[1] for s in srcs], fmts, fs, ts)


def test_every_block_sum(casc):
    """The block-sum images of the host test, every factor in one call, as gray and as colour with equal channels (whose gray
    is the channel): the device's division is exact for every sum."""
    import torch
    for fmt in (pr.GRAY8, pr.BGR24):
        views, want = [], []
        for f in rr.FACTORS:
            img, sums = rr.block_sum_image(f)
            views.append(img if fmt == pr.GRAY8 else np.ascontiguousarray(np.repeat(img[..., None], 3, 2)))
            want.append(((sums + f * f // 2) // (f * f)).astype(np.uint8))
        (buf, offs, ws, hs), st = casc.pack_gray_reduced_device([torch.from_numpy(v).cuda() for v in views], fmt, list(rr.FACTORS), stats=True)
        assert st["launches"] == 1
        got = buf.cpu().numpy()
        for o, w, h, g in zip(offs, ws, hs, want):
            assert (h, w) == g.shape and np.array_equal(got[int(o):int(o) + w * h].reshape(h, w), g)


def mixed(rng, n):
    views, tensors, fmts, rects, fs, ts = [], [], [], [], [], []
    for i in range(n):
        fmt = pr.FORMATS[(i * 3 + 1) % 5]
        f = int(rng.integers(1, 9))
        h, w = int(rng.integers(f, 40 * f)), int(rng.integers(f, 40 * f))
        v, d = source(rng, h, w, fmt, int(rng.integers(0, 9)), int(rng.integers(0, 16)))
        views.append(v); tensors.append(d); fmts.append(fmt); fs.append(f); ts.append(int(rng.integers(0, 8)))
        rects.append(None if i % 3 or w < 2 * f or h < 3 * f else (w // 2 - f // 2, h // 3, w - w // 2, h - h // 3))
    return views, tensors, fmts, fs, ts, rects


@pytest.mark.parametrize("n", [1, 2, 40])
def test_ragged_sets_are_one_launch(casc, n):
    run(casc, *mixed(np.random.default_rng(n), n))


def test_factor_1_is_pack_gray_oriented_device(casc):
    """Every factor 1: jdaPackGrayOrientedDevice's bytes -- and with orients NULL or all 0 jdaPackGrayDevice's -- in one launch;
    an empty set touches nothing."""
    import torch
    views, tensors, fmts, fs, ts, rects = mixed(np.random.default_rng(3), 7)
    run(casc, views, tensors, fmts, [1] * 7, ts, rects)
    run(casc, views, tensors, fmts, [1] * 7, None, rects)
    a = casc.pack_gray_reduced_device(tensors, fmts, 1, ts, rects)
    b = casc.pack_gray_oriented_device(tensors, fmts, ts, rects)
    assert a[2:] == b[2:] and list(a[1]) == list(b[1])
    for o, w, h in zip(a[1], a[2], a[3]):
        assert torch.equal(a[0][int(o):int(o) + w * h], b[0][int(o):int(o) + w * h])
    buf = torch.from_numpy(pattern(64)).cuda()
    (b, offs, ws, hs), st = casc.pack_gray_reduced_device([], [], [], [], stats=True, out=(buf, []))
    assert len(offs) == 0 and ws == [] and hs == [] and st["launches"] == 0 and np.array_equal(buf.cpu().numpy(), pattern(64))


def test_both_stream_forms(casc):
    import torch
    views, tensors, fmts, fs, ts, rects = mixed(np.random.default_rng(11), 9)
    run(casc, views, tensors, fmts, fs, ts, rects)                           # hip_stream NULL: the lane's own stream
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):                                               # the pixels are produced on s, just before the call
        tensors = [d.clone() if d.is_contiguous() else d for d in tensors]
        run(casc, views, tensors, fmts, fs, ts, rects, hip_stream=s.cuda_stream)
    s.synchronize()


def test_two_threads_on_one_cascador(casc):
    rng = np.random.default_rng(12)
    sets = [mixed(rng, 11), mixed(rng, 13)]
    errors = []

    def work(k):
        try:
            for _ in range(3):
                run(casc, *sets[k])
        except BaseException as e:                                           # noqa: B036 (an assertion is what we are after)
            errors.append((k, repr(e)))
    threads = [threading.Thread(target=work, args=(k,)) for k in range(2)]
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    assert not errors, errors


def test_refusals_launch_nothing(casc):
    """Sources and destination live in ONE patterned allocation (a at byte 0, b at 1024, the destination at 4096), which
    must come back as it was."""
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
    cases = [(what, px, offs, n, words, (1, 1), (1, 4)) for what, px, offs, n, words in refusals(api, Dev(base), Dev(base + 1024))]
    ok = [api.jdaPixels(base, 24, 8, 6, pr.BGR24, 0, 0, 0, 0), api.jdaPixels(base + 1024, 24, 8, 6, pr.BGR24, 0, 0, 0, 0)]
    cases += [("orientation 8", ok, [64, 112], 2, ["image 1", "orientation 8"], (2, 2), (0, 8)), ("factor 0", ok, [64, 112], 2, ["image 0", "factor 0"], (0, 2), (1, 4)),
              ("factor 9", ok, [64, 112], 2, ["image 1", "factor 9"], (2, 9), (1, 4)), ("h below f", ok, [64, 112], 2, ["image 0", "8 x 6", "factor 7"], (7, 2), (1, 4)),
              ("reduced destinations overlap", ok, [64, 75], 2, ["image 0", "image 1", "overlap"], (2, 2), (1, 4))]
    for what, px, offs, n, words, fs, ts in cases:
        arr = (api.jdaPixels * len(px))(*px)
        st = api.jdaPackStats(launches=7)
        rc = api.lib.jdaPackGrayReducedDevice(casc.h, arr, (C.c_int * 2)(*fs), (C.c_int * 2)(*ts), n, C.c_void_p(base + 4096), (C.c_size_t * len(offs))(*offs), None,
                                              C.byref(st))
        assert rc == -1 and st.launches == 7, what                           # (the statistics are not touched either)
        for w in words:
            assert w in api.last_error(), (what, api.last_error())
        assert "jdaPackGrayReducedDevice" in api.last_error(), what
    two, fs, ts, good = (api.jdaPixels * 2)(*ok), (C.c_int * 2)(2, 2), (C.c_int * 2)(1, 4), (C.c_size_t * 2)(4096, 5000)
    for args in ((None, two, fs, ts, 2, C.c_void_p(base), good), (casc.h, None, fs, ts, 2, C.c_void_p(base), good), (casc.h, two, None, ts, 2, C.c_void_p(base), good),
                 (casc.h, two, fs, ts, 2, None, good), (casc.h, two, fs, ts, 2, C.c_void_p(base), None)):
        assert api.lib.jdaPackGrayReducedDevice(*args, None, None) == -1 and "null" in api.last_error()
    # the destination inside the source rows of the image itself and of another image
    for offs, words in (((40, 5000), ["image 0", "source rows of image 0"]), ((5000, 100), ["image 1", "source rows of image 0"])):
        assert api.lib.jdaPackGrayReducedDevice(casc.h, two, fs, ts, 2, C.c_void_p(base), (C.c_size_t * 2)(*offs), None, None) == -1
        for w in words:
            assert w in api.last_error(), (offs, api.last_error())
    torch.cuda.synchronize()
    assert np.array_equal(pool.cpu().numpy(), pattern(8192))
    # ... and right behind them it is taken
    assert api.lib.jdaPackGrayReducedDevice(casc.h, two, fs, ts, 2, C.c_void_p(base), (C.c_size_t * 2)(144, 1024 + 144), None, None) == 0
    torch.cuda.synchronize()
    want = pattern(8192)
    for k, t in ((0, 1), (1024, 4)):
        src = want[k:k + 144].reshape(6, 8, 3).copy()
        want[k + 144:k + 156] = rr.reduce(src, pr.BGR24, 2, t).ravel()
    assert np.array_equal(pool.cpu().numpy(), want)


def test_factor_2_is_resize_cv_to_half_on_the_device(casc):
    import torch
    rng = np.random.default_rng(4)
    img = rng.integers(0, 256, (98, 130), dtype=np.uint8)
    buf, offs, ws, hs = casc.pack_gray_reduced_device([torch.from_numpy(img).cuda()], "gray8", 2)
    assert np.array_equal(buf[:65 * 49].cpu().numpy().reshape(49, 65), casc.resize_cv(img, 65, 49))


# ---- into the entries that take the packed images, and back, on a synthetic model -------------------------------------------

@pytest.mark.parametrize("f,t", [(2, 0), (3, 1), (4, 6), (5, 7), (8, 5)])
def test_end_to_end_back_to_the_source_frame(built, gpu, model_file, f, t):
    """S is the frame F enlarged by pixel replication and turned back, in BGR with equal channels, so S reduced by f and
    turned by t IS F; detecting on the device-reduced S gives F's results -- the batch entry and a ragged dialect-CPP entry --,
    and reduce_back puts every box on the S pixels that, reduced and turned, are the F pixels under the box."""
    import torch
    from jda_amd import api, synth
    p, _ = model_file((3, 20, 5, 4), 4, seed=3, cart_th=-1.0)
    c = api.Cascador(p)
    F = synth.make_frames(2, 96, 80, seed=5)
    inv = [s for s in tr.ORIENTS if np.array_equal(transform(transform(F[0], s), t), F[0])][0]
    Sg = [np.kron(np.ascontiguousarray(transform(x, inv)), np.ones((f, f), np.uint8)) for x in F]
    S = [np.ascontiguousarray(np.repeat(x[..., None], 3, 2)) for x in Sg]
    dev = [torch.from_numpy(x).cuda() for x in S]
    buf, offs, ws, hs = c.pack_gray_reduced_device(dev, "bgr24", f, t, frame_stride=96 * 80)
    assert (ws, hs) == ([96] * 2, [80] * 2) and np.array_equal(buf.cpu().numpy().reshape(2, 80, 96), F)
    want = c.detect_batch(F, min_size=24)
    got = c.detect_batch_device(buf.view(2, 80, 96), min_size=24)
    for a, b in zip(got, want):
        for k in ("bboxes", "scores", "shapes"):
            assert same(a[k], b[k]), k
    assert sum(len(g["scores"]) for g in got) > 0
    p8, _ = model_file((3, 20, 5, 4), 8, seed=3, cart_th=-1.0, norm_every=5)
    c8 = api.Cascador(p8)
    want_cpp = c8.detect_ragged_cpp(list(F))
    got_cpp = c8.detect_ragged_cpp_packed(*c8.pack_gray_reduced_device(dev, "bgr24", f, t))
    c8.close()
    assert sum(len(w["scores"]) for w in want_cpp) > 0
    for a, b in zip(got_cpp, want_cpp):
        for k in ("rects", "scores", "shapes"):
            assert same(a[k], b[k]), k
    back = api.reduce_back(S, "bgr24", f, t, got)
    M = 128                                                                   # boxes may leave the frame: a margin on every side
    for i in range(2):
        assert same(back[i]["scores"], got[i]["scores"])
        Fp, Sp = np.pad(F[i], M), np.pad(Sg[i], M * f)
        for (bx, by, bs), (x, y, s2) in zip(got[i]["bboxes"], back[i]["bboxes"]):
            assert s2 == bs * f and min(bx, by) > -M and max(bx, by) + bs < M + 80
            under = transform(rr.block_means(Sp[y + M * f:y + M * f + s2, x + M * f:x + M * f + s2], f), t)
            assert np.array_equal(under, Fp[by + M:by + M + bs, bx + M:bx + M + bs])
        for k in range(len(got[i]["shapes"])):
            assert same(back[i]["shapes"][k], rr.back_landmarks(got[i]["shapes"][k], f, t, (0, 0) + Sg[i].shape[::-1]))
    c.close()
