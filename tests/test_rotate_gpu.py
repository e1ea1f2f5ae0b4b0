"""jdaPackGrayRotatedDevice (include/jda.h, "frames whose faces are rolled"; k_rotate.hip): colour, pitched and cropped device
images -> dense 8-bit gray, every image rotated by its own angle, by one kernel launch.  Every comparison is device bytes ==
host form bytes (jdaPackGrayRotated, which tests/test_rotate_host.py ties to the restatement), exact: as in test_turn_gpu.py
every destination sits inside a patterned buffer and the WHOLE buffer is compared with what it must hold afterwards.  On the
bounds-check build (JDA_LIB_PATH=jda_amd/libjda_bounds.so) conftest.py's autouse fixture fails any test whose launch reported
a site: every source dword, every LDS access -- the covering of a tile's box among them -- and every store."""
import threading

import numpy as np
import pytest

import pack_ref as pr
import rotate_ref as ro
from conftest import same
from test_pack_gpu import pattern, source

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


def run(casc, views, tensors, fmts, degs, rects=None, dst_mis=None, hip_stream=None):
    """Packs rotated by degs into a patterned buffer -- image i at the first 16-byte boundary at least 32 bytes behind image
    i - 1, plus dst_mis[i] -- and compares the whole buffer with the host form's images in it; returns the statistics."""
    import torch
    from jda_amd import api
    n = len(views)
    rects = rects or [None] * n
    want = api.pack_gray_rotated(views, fmts, degs, rects)
    offs, end = [], 0
    for i, g in enumerate(want):
        o = (end + 32 + 15) // 16 * 16 + (dst_mis[i] if dst_mis else (i * 5) % 16)
        offs.append(o)
        end = o + g.size
    expect = pattern(end + 64)
    buf = torch.from_numpy(expect.copy()).cuda()
    for o, g in zip(offs, want):
        expect[o:o + g.size] = g.ravel()
    (b, o2, ws, hs), st = casc.pack_gray_rotated_device(tensors, fmts, degs, rects, stats=True, hip_stream=hip_stream, out=(buf, offs))
    if hip_stream is None:
        torch.cuda.synchronize()
    got = buf.cpu().numpy()
    bad = np.flatnonzero(got != expect)
    assert bad.size == 0, ("first wrong byte", int(bad[0]), "of", got.size, "image offsets", offs[:8], "wrong bytes", bad.size)
    assert ws == [g.shape[1] for g in want] and hs == [g.shape[0] for g in want] and list(o2) == offs
    assert st["launches"] == (1 if n else 0) and st["pixels"] == sum(g.size for g in want) == st["bytes_out"]
    fl = [fmts] * n if isinstance(fmts, int) else fmts
    sizes = [(v.shape[1], v.shape[0]) if r is None else r[2:] for v, r in zip(views, rects)]
    assert st["bytes_in"] == sum(w * h * pr.BPP[fm] for (w, h), fm in zip(sizes, fl))
    return st


SHAPES = ((130, 67), (67, 130), (1, 1), (64, 64), (65, 3), (2, 129))


def test_every_format_and_angle_in_one_call(casc):
    """Every format x every angle of the list in ONE ragged call, sizes up to 130 x 67 and 67 x 130 -- several tiles, partial
    tiles on both edges -- and 1 x 1."""
    rng = np.random.default_rng(0)
    srcs, fmts, degs = [], [], []
    for fmt in pr.FORMATS:
        for k, d in enumerate(ro.ANGLES):
            w, h = SHAPES[(k + fmt) % len(SHAPES)]
            srcs.append(source(rng, h, w, fmt, slack=(w + h + k) % 4, base=(3 * w + h + k) % 16)); fmts.append(fmt); degs.append(d)
    st = run(casc, [s[0] for s in srcs], [s[1] for s in srcs], fmts, degs)
    assert st["launches"] == 1


@pytest.mark.parametrize("fmt", [pr.GRAY8, pr.BGR24, pr.RGBA32])
def test_widths_round_a_tile_at_every_misalignment(casc, fmt):
    """Widths 63 / 64 / 65 x source misalignment 0..3 x destination offset 0..15."""
    rng = np.random.default_rng(fmt)
    srcs, degs, mis = [], [], []
    for w in (63, 64, 65):
        for sb in range(4):
            for k, d in enumerate((30, -0.5, 45, 89.5)):
                srcs.append(source(rng, 9 + k, w, fmt, (sb + k) % 3, sb)); degs.append(d); mis.append((4 * sb + k + w) % 16)
    run(casc, [s[0] for s in srcs], [s[1] for s in srcs], [fmt] * len(srcs), degs, dst_mis=mis)


def test_rectangles(casc):
    rng = np.random.default_rng(5)
    views, tensors, fmts, rects, degs = [], [], [], [], []
    for fmt in pr.FORMATS:
        for name in sorted(pr.RECTS):
            for d in (30, -33.3, 135):
                v, t = source(rng, 21, 37, fmt, 5, 1)
                views.append(v); tensors.append(t); fmts.append(fmt); rects.append(pr.RECTS[name](37, 21)); degs.append(d)
    v, t = source(rng, 150, 200, pr.BGRA32)              # a crop of more than one tile out of a frame
    views.append(v); tensors.append(t); fmts.append(pr.BGRA32); rects.append((51, 7, 141, 139)); degs.append(60)
    run(casc, views, tensors, fmts, degs, rects)


def test_source_ends_with_its_allocation(casc):
    """The rectangle's last pixel is the allocation's last byte, every start alignment and format (under the bounds-check
    build every dword read must hold a byte of a pixel of the rectangle's row)."""
    rng = np.random.default_rng(6)
    srcs, fmts, degs = [], [], []
    for fmt in pr.FORMATS:
        for k, (w, h) in enumerate(((67, 2), (5, 9), (2, 3), (1, 1), (66, 65))):
            srcs.append(source(rng, h, w, fmt, (k + w) % 3 * pr.BPP[fmt], (k + w) % 4)); fmts.append(fmt); degs.append(ro.ANGLES[(3 * k + fmt) % len(ro.ANGLES)] or 15)
    run(casc, [s[0] for s in srcs], [s[1] for s in srcs], fmts, degs)


def test_the_largest_box_and_the_smallest_angle(casc):
    """200 x 150 at 45 degrees, where a tile's source box is at its largest (92 x 92), and at 0.01 degrees, where it is a
    tile and its margin."""
    rng = np.random.default_rng(7)
    srcs = [source(rng, 150, 200, pr.BGR24, 1, 2), source(rng, 150, 200, pr.GRAY8, 0, 1), source(rng, 150, 200, pr.RGB24), source(rng, 150, 200, pr.GRAY8, 3, 3)]
    run(casc, [s[0] for s in srcs], [s[1] for s in srcs], [pr.BGR24, pr.GRAY8, pr.RGB24, pr.GRAY8], [45, -45, 0.01, -0.01])


def mixed(rng, n):
    views, tensors, fmts, rects, degs = [], [], [], [], []
    for i in range(n):
        fmt = pr.FORMATS[(i * 3 + 1) % 5]
        h, w = int(rng.integers(1, 90)), int(rng.integers(1, 90))
        v, d = source(rng, h, w, fmt, int(rng.integers(0, 9)), int(rng.integers(0, 16)))
        views.append(v); tensors.append(d); fmts.append(fmt)
        degs.append(float(rng.uniform(-180, 180)) if i % 4 else float(90 * int(rng.integers(0, 4))))
        rects.append(None if i % 3 or w < 2 or h < 3 else (w // 2, h // 3, w - w // 2, h - h // 3))
    return views, tensors, fmts, degs, rects


@pytest.mark.parametrize("n", [1, 2, 17])
def test_ragged_sets_are_one_launch(casc, n):
    views, tensors, fmts, degs, rects = mixed(np.random.default_rng(n), n)
    if n == 1:
        degs = [33.0]
    run(casc, views, tensors, fmts, degs, rects)


def test_both_stream_forms(casc):
    import torch
    views, tensors, fmts, degs, rects = mixed(np.random.default_rng(11), 9)
    run(casc, views, tensors, fmts, degs, rects)                             # hip_stream NULL: the lane's own stream
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):                                               # the pixels are produced on s, just before the call
        tensors = [d.clone() if d.is_contiguous() else d for d in tensors]
        run(casc, views, tensors, fmts, degs, rects, hip_stream=s.cuda_stream)
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


def test_quarter_turns_are_pack_gray_oriented_device(casc):
    """90 / 180 / 270 / 0 = jdaPackGrayOrientedDevice at 1 / 2 / 3 / 0: in a call of quarter turns only and -- the kernel's own
    bytes -- in a call that also holds another angle; an empty set touches nothing."""
    import torch
    rng = np.random.default_rng(3)
    srcs = [source(rng, h, w, fmt, 2, 1) for fmt in pr.FORMATS for (w, h) in ((37, 21), (66, 3), (2, 131), (70, 69))]
    fmts = [fmt for fmt in pr.FORMATS for _ in range(4)]
    degs = [(0, 90, 180, 270, -90, 450)[k % 6] for k in range(len(srcs))]
    ts = [int(d // 90) % 4 for d in degs]
    tensors = [s[1] for s in srcs]
    run(casc, [s[0] for s in srcs], tensors, fmts, degs)
    b = casc.pack_gray_oriented_device(tensors, fmts, ts)
    for extra in ([], [(source(rng, 5, 4, pr.GRAY8)[1], pr.GRAY8, 15.0)]):
        a = casc.pack_gray_rotated_device(tensors + [e[0] for e in extra], fmts + [e[1] for e in extra], degs + [e[2] for e in extra])
        assert a[2][:len(srcs)] == b[2] and a[3][:len(srcs)] == b[3]
        for oa, ob, w, h in zip(a[1], b[1], b[2], b[3]):
            assert torch.equal(a[0][int(oa):int(oa) + w * h], b[0][int(ob):int(ob) + w * h])
    buf = torch.from_numpy(pattern(64)).cuda()
    (_, offs, ws, hs), st = casc.pack_gray_rotated_device([], [], [], stats=True, out=(buf, []))
    assert len(offs) == 0 and ws == [] and hs == [] and st["launches"] == 0 and np.array_equal(buf.cpu().numpy(), pattern(64))


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
    cases = [(what, px, offs, n, words, (0.0, 0.0)) for what, px, offs, n, words in refusals(api, Dev(base), Dev(base + 1024))]
    ok = [api.jdaPixels(base, 24, 8, 6, pr.BGR24, 0, 0, 0, 0), api.jdaPixels(base + 1024, 24, 8, 6, pr.BGR24, 0, 0, 0, 0)]
    cases += [("nan", ok, [64, 256], 2, ["image 1", "nan"], (30.0, float("nan"))), ("inf", ok, [64, 256], 2, ["image 0", "inf"], (float("inf"), 30.0)),
              ("36001", ok, [64, 256], 2, ["image 1", "36001"], (30.0, -36001.0)),
              ("too wide", [ok[0], api.jdaPixels(base, 150000, 50000, 1, pr.BGR24, 0, 0, 0, 0)], [64, 256], 2, ["image 1", "50000 x 1", "32768"], (30.0, 45.0)),
              ("rotated destinations overlap", ok, [64, 163], 2, ["image 0", "image 1", "100 bytes", "overlap"], (30.0, 30.0))]
    for what, px, offs, n, words, degs in cases:
        arr = (api.jdaPixels * len(px))(*px)
        st = api.jdaPackStats(launches=7)
        rc = api.lib.jdaPackGrayRotatedDevice(casc.h, arr, (C.c_double * 2)(*degs), n, C.c_void_p(base + 4096), (C.c_size_t * len(offs))(*offs), None, C.byref(st))
        assert rc == -1 and st.launches == 7, what                           # (the statistics are not touched either)
        for w in words:
            assert w in api.last_error(), (what, api.last_error())
        assert "jdaPackGrayRotatedDevice" in api.last_error(), what
    two, degs, good = (api.jdaPixels * 2)(*ok), (C.c_double * 2)(30.0, -30.0), (C.c_size_t * 2)(4096, 5000)
    for args in ((None, two, degs, 2, C.c_void_p(base), good), (casc.h, None, degs, 2, C.c_void_p(base), good), (casc.h, two, None, 2, C.c_void_p(base), good),
                 (casc.h, two, degs, 2, None, good), (casc.h, two, degs, 2, C.c_void_p(base), None)):
        assert api.lib.jdaPackGrayRotatedDevice(*args, None, None) == -1 and "null" in api.last_error()
    # the destination inside the source rows of the image itself and of another image
    for offs, words in (((40, 5000), ["image 0", "source rows of image 0"]), ((5000, 100), ["image 1", "source rows of image 0"])):
        assert api.lib.jdaPackGrayRotatedDevice(casc.h, two, degs, 2, C.c_void_p(base), (C.c_size_t * 2)(*offs), None, None) == -1
        for w in words:
            assert w in api.last_error(), (offs, api.last_error())
    torch.cuda.synchronize()
    assert np.array_equal(pool.cpu().numpy(), pattern(8192))
    # ... and right behind them it is taken
    assert api.lib.jdaPackGrayRotatedDevice(casc.h, two, degs, 2, C.c_void_p(base), (C.c_size_t * 2)(144, 1024 + 144), None, None) == 0
    torch.cuda.synchronize()
    want = pattern(8192)
    for k, d in ((0, 30.0), (1024, -30.0)):
        src = want[k:k + 144].reshape(6, 8, 3).copy()
        want[k + 144:k + 244] = api.pack_gray_rotated([src], pr.BGR24, d)[0].ravel()
    assert np.array_equal(pool.cpu().numpy(), want)


# ---- into the ragged detect entry and back, on a synthetic model ------------------------------------------------------------

def test_end_to_end_back_to_the_source_frame(built, gpu, model_file):
    """One frame packed at -30, 0 and 30 degrees in one call, one ragged detect, rotate_back: equal, bit for bit, to the same
    steps on the host form's images; the angle-0 share equals detecting on pack_gray_device's image."""
    import torch
    from jda_amd import api, synth
    p, _ = model_file((3, 20, 5, 4), 4, seed=3, cart_th=-1.0)
    c = api.Cascador(p)
    F = synth.make_frames(1, 96, 80, seed=5)[0]
    S = np.ascontiguousarray(np.repeat(F[..., None], 3, 2))
    dev = torch.from_numpy(S).cuda()
    degs = [-30.0, 0.0, 30.0]
    packed = c.pack_gray_rotated_device([dev] * 3, "bgr24", degs)
    got = c.detect_ragged_packed(*packed, min_size=24)
    host = api.pack_gray_rotated([S] * 3, "bgr24", degs)
    for o, w, h, g in zip(packed[1], packed[2], packed[3], host):
        assert (h, w) == g.shape and np.array_equal(packed[0][int(o):int(o) + w * h].cpu().numpy().reshape(h, w), g)
    want = c.detect_ragged(list(host), min_size=24)
    assert sum(len(g["scores"]) for g in got) > 0
    back, back_want = api.rotate_back([S] * 3, "bgr24", degs, got), api.rotate_back([S] * 3, "bgr24", degs, want)
    for a, b in zip(back, back_want):
        for k in ("bboxes", "scores", "shapes"):
            assert same(a[k], b[k]), k
    flat = c.detect_ragged_packed(*c.pack_gray_device([dev], "bgr24"), min_size=24)[0]
    for k in ("bboxes", "scores", "shapes"):
        assert same(got[1][k], flat[k]), k
    assert np.array_equal(back[1]["bboxes"], got[1]["bboxes"])               # angle 0, the whole frame: boxes stay where they are
    c.close()
