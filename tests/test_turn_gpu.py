"""jdaPackGrayOrientedDevice (include/jda.h, "frames in any orientation"; k_turn.hip): colour, pitched and cropped device
images -> dense 8-bit gray, turned by one of the eight orientations, by one kernel launch.  As in test_pack_gpu.py every
destination sits inside a patterned buffer and the WHOLE buffer is compared with what it must hold afterwards -- the turned
gray images of tests/turn_ref.py where they belong, the pattern everywhere else -- and the host form must give the same
bytes.  Every comparison is exact.  On the bounds-check build (JDA_LIB_PATH=jda_amd/libjda_bounds.so) conftest.py's autouse
fixture fails any test whose launch reported a site."""
import threading

import numpy as np
import pytest

import pack_ref as pr
import turn_ref as tr
from conftest import same
from mining_ref import transform
from test_pack_gpu import colour_of, on_device, pattern, run, source

pytestmark = pytest.mark.gpu

WIDTHS = [1, 2, 3, 15, 16, 17, 63, 64, 65, 100]
HEIGHTS = [1, 2, 3, 63, 64, 65]


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


@pytest.mark.parametrize("shift", range(5))
def test_shape_grid_mixed(casc, shift):
    """Every width x height x orientation in ONE call, the formats dealt round: narrower than a unit, than a tile, one tile,
    one more; over the five cases every format meets every shape and orientation."""
    rng = np.random.default_rng(shift)
    srcs, fmts, ts = [], [], []
    for w in WIDTHS:
        for h in HEIGHTS:
            for t in tr.ORIENTS:
                fmt = pr.FORMATS[(len(srcs) + shift) % 5]
                srcs.append(source(rng, h, w, fmt, slack=(w + h) % 4, base=(3 * w + h + t) % 16)); fmts.append(fmt); ts.append(t)
    run(casc, [s[0] for s in srcs], [s[1] for s in srcs], fmts, ts=ts)


@pytest.mark.parametrize("fmt", [pr.BGR24, pr.GRAY8])
@pytest.mark.parametrize("t", [1, 4])
@pytest.mark.parametrize("wh", [(47, 3), (3, 47)])
def test_misalignments(casc, wh, t, fmt):
    """Source base 0..15 x destination offset 0..15, for a transposing and a mirroring orientation: every source shift
    against every head / tail length of every turned row."""
    rng = np.random.default_rng(t)
    srcs = [source(rng, wh[1], wh[0], fmt, sb % 3, sb) for sb in range(16) for _ in range(16)]
    run(casc, [s[0] for s in srcs], [s[1] for s in srcs], [fmt] * 256, ts=[t] * 256, dst_mis=[i % 16 for i in range(256)])


def test_rectangles(casc):
    rng = np.random.default_rng(5)
    views, tensors, fmts, rects, ts = [], [], [], [], []
    for fmt in pr.FORMATS:
        for name in sorted(pr.RECTS):
            for t in (1, 2, 5, 6):
                v, d = source(rng, 21, 37, fmt, 5, 1)
                views.append(v); tensors.append(d); fmts.append(fmt); rects.append(pr.RECTS[name](37, 21)); ts.append(t)
    v, d = source(rng, 300, 400, pr.BGRA32)             # a crop of more than one tile out of a frame
    views.append(v); tensors.append(d); fmts.append(pr.BGRA32); rects.append((201, 107, 150, 131)); ts.append(3)
    run(casc, views, tensors, fmts, rects, ts)


def mixed(rng, n):
    views, tensors, fmts, rects, ts = [], [], [], [], []
    for i in range(n):
        fmt = pr.FORMATS[(i * 3 + 1) % 5]
        h, w = int(rng.integers(1, 150)), int(rng.integers(1, 150))
        v, d = source(rng, h, w, fmt, int(rng.integers(0, 9)), int(rng.integers(0, 16)))
        views.append(v); tensors.append(d); fmts.append(fmt); ts.append(int(rng.integers(0, 8)))
        rects.append(None if i % 3 else (w // 2, h // 3, w - w // 2, h - h // 3))
    return views, tensors, fmts, rects, ts


@pytest.mark.parametrize("n", [1, 2, 5, 130])
def test_ragged_sets_are_one_launch(casc, n):
    run(casc, *mixed(np.random.default_rng(n), n))


def test_source_ends_with_its_allocation(casc):
    """No pitch slack, the last pixel the allocation's last byte, every start alignment, every orientation (under the
    bounds-check build every dword read must hold a byte of its row)."""
    rng = np.random.default_rng(6)
    srcs, fmts, ts = [], [], []
    for fmt in pr.FORMATS:
        for t in tr.ORIENTS:
            for w, h in ((67, 5), (5, 67)):
                srcs.append(source(rng, h, w, fmt, 0, (t + w) % 4)); fmts.append(fmt); ts.append(t)
    run(casc, [s[0] for s in srcs], [s[1] for s in srcs], fmts, ts=ts)


def test_upright_sets_are_pack_gray(casc):
    """Every orientation 0: jdaPackGrayDevice's bytes (and one launch); an empty set touches nothing."""
    import torch
    views, tensors, fmts, rects, ts = mixed(np.random.default_rng(3), 7)
    run(casc, views, tensors, fmts, rects, [0] * 7)
    buf = torch.from_numpy(pattern(64)).cuda()
    (b, offs, ws, hs), st = casc.pack_gray_oriented_device([], [], [], stats=True, out=(buf, []))
    assert len(offs) == 0 and ws == [] and hs == [] and st["launches"] == 0 and np.array_equal(buf.cpu().numpy(), pattern(64))


def test_both_stream_forms(casc):
    import torch
    views, tensors, fmts, rects, ts = mixed(np.random.default_rng(11), 9)
    run(casc, views, tensors, fmts, rects, ts)                               # hip_stream NULL: the lane's own stream
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):                                               # the pixels are produced on s, just before the call
        tensors = [d.clone() if d.is_contiguous() else d for d in tensors]
        run(casc, views, tensors, fmts, rects, ts, hip_stream=s.cuda_stream)
    s.synchronize()


def test_two_threads_on_one_cascador(casc):
    rng = np.random.default_rng(12)
    sets = [mixed(rng, 17), mixed(rng, 23)]
    errors = []

    def work(k):
        try:
            for _ in range(4):
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
    cases = [(what, px, offs, n, words, (1, 4)) for what, px, offs, n, words in refusals(api, Dev(base), Dev(base + 1024))]
    ok = [api.jdaPixels(base, 24, 8, 6, pr.BGR24, 0, 0, 0, 0), api.jdaPixels(base + 1024, 24, 8, 6, pr.BGR24, 0, 0, 0, 0)]
    cases += [("orientation 8", ok, [64, 112], 2, ["image 1", "orientation 8"], (0, 8)), ("orientation -1", ok, [64, 112], 2, ["image 0", "orientation -1"], (-1, 0))]
    for what, px, offs, n, words, ts in cases:
        arr = (api.jdaPixels * len(px))(*px)
        st = api.jdaPackStats(launches=7)
        rc = api.lib.jdaPackGrayOrientedDevice(casc.h, arr, (C.c_int * 2)(*ts), n, C.c_void_p(base + 4096), (C.c_size_t * len(offs))(*offs), None, C.byref(st))
        assert rc == -1 and st.launches == 7, what                           # (the statistics are not touched either)
        for w in words:
            assert w in api.last_error(), (what, api.last_error())
    two, ts, good = (api.jdaPixels * 2)(*ok), (C.c_int * 2)(1, 4), (C.c_size_t * 2)(4096, 5000)
    for args in ((None, two, ts, 2, C.c_void_p(base), good), (casc.h, None, ts, 2, C.c_void_p(base), good), (casc.h, two, None, 2, C.c_void_p(base), good),
                 (casc.h, two, ts, 2, None, good), (casc.h, two, ts, 2, C.c_void_p(base), None)):
        assert api.lib.jdaPackGrayOrientedDevice(*args, None, None) == -1 and "null" in api.last_error()
    # the destination inside the source rows of the image itself and of another image
    for offs, words in (((40, 5000), ["image 0", "source rows of image 0"]), ((5000, 100), ["image 1", "source rows of image 0"])):
        assert api.lib.jdaPackGrayOrientedDevice(casc.h, two, ts, 2, C.c_void_p(base), (C.c_size_t * 2)(*offs), None, None) == -1
        for w in words:
            assert w in api.last_error(), (offs, api.last_error())
    torch.cuda.synchronize()
    assert np.array_equal(pool.cpu().numpy(), pattern(8192))
    # ... and right behind them it is taken
    assert api.lib.jdaPackGrayOrientedDevice(casc.h, two, ts, 2, C.c_void_p(base), (C.c_size_t * 2)(144, 1024 + 144), None, None) == 0
    torch.cuda.synchronize()
    want = pattern(8192)
    for k, t in ((0, 1), (1024, 4)):
        src = want[k:k + 144].reshape(6, 8, 3).copy()
        want[k + 144:k + 192] = tr.turn(src, pr.BGR24, t).ravel()
    assert np.array_equal(pool.cpu().numpy(), want)


# ---- into the entries that take the packed images, on a synthetic model -----------------------------------------------------

def _eq_c(a, b):
    for k in ("bboxes", "scores", "shapes"):
        assert same(a[k], b[k]), k


def _eq_cpp(a, b):
    for k in ("rects", "scores", "shapes"):
        assert same(a[k], b[k]), k


def test_turned_frames_into_the_batch_entry(built, gpu, model_file):
    import torch
    from jda_amd import api, synth
    p, _ = model_file((3, 20, 5, 4), 4, seed=3, cart_th=-1.0)
    c = api.Cascador(p)
    rng = np.random.default_rng(21)
    colour = [colour_of(f, rng, pr.BGRA32) for f in synth.make_frames(3, 96, 80, seed=5)]
    for t in (1, 6):
        turned = np.stack(api.pack_gray([transform(pr.gray(x, pr.BGRA32), t) for x in colour], "gray8"))   # numpy turns, the host packs
        want = c.detect_batch(turned, min_size=24)
        assert sum(len(w["scores"]) for w in want) > 0
        buf, offs, ws, hs = c.pack_gray_oriented_device([torch.from_numpy(x).cuda() for x in colour], "bgra32", t, frame_stride=96 * 80)
        assert ws == [turned.shape[2]] * 3 and hs == [turned.shape[1]] * 3
        for a, b in zip(c.detect_batch_device(buf.view(3, hs[0], ws[0]), min_size=24), want):
            _eq_c(a, b)
    c.close()


def test_turned_set_into_the_ragged_entries(built, gpu, model_file):
    import torch
    from jda_amd import api, synth
    p, _ = model_file((3, 20, 5, 4), 8, seed=3, cart_th=-1.0, norm_every=5)
    c = api.Cascador(p)
    rng = np.random.default_rng(22)
    sizes, fmts, ts = [(96, 80), (101, 77), (64, 90), (96, 80)], [pr.RGB24, pr.BGRA32, pr.BGR24, pr.GRAY8], [3, 5, 4, 7]
    colour = [colour_of(synth.make_frames(1, w, h, seed=11, first=i)[0], rng, f) for i, ((w, h), f) in enumerate(zip(sizes, fmts))]
    colour[3] = colour[3][..., 0]
    grays = api.pack_gray([transform(pr.gray(x, f), t) for x, f, t in zip(colour, fmts, ts)], "gray8")
    packed = c.pack_gray_oriented_device([torch.from_numpy(x).cuda() for x in colour], fmts, ts)
    want_c, want_cpp = c.detect_ragged(grays, min_size=24), c.detect_ragged_cpp(grays)
    assert sum(len(w["scores"]) for w in want_c) > 0 and sum(len(w["scores"]) for w in want_cpp) > 0
    for a, b in zip(c.detect_ragged_packed(*packed, min_size=24), want_c):
        _eq_c(a, b)
    for a, b in zip(c.detect_ragged_cpp_packed(*packed), want_cpp):
        _eq_cpp(a, b)
    c.close()


def test_mining_a_turned_image_is_mining_under_the_transform(built, gpu, tmp_path):
    """k_mine remaps coordinates under transforms[i] = t; k_turn makes the turned image.  One definition: mining the source
    under t and mining the device-turned image under 0 find the same windows, scores, shapes, patches and counters."""
    import torch
    from jda_amd import api, synth
    from test_mining import _model
    c = api.Cascador(_model(tmp_path, True, None, False, cart_th=-1.5))
    bgs = [synth.make_frames(1, w, h, seed=3, first=i)[0] for i, (w, h) in enumerate([(70, 50), (53, 71), (64, 64)])]
    dev = [torch.from_numpy(b).cuda() for b in bgs]
    hits = 0
    for t in tr.ORIENTS:
        a = c.mine_negatives_cpp(bgs, [5] * 3, [1.2] * 3, [t] * 3, 10 ** 6, device=True)
        b = c.mine_negatives_cpp(c.pack_gray_oriented_device(dev, "gray8", t), [5] * 3, [1.2] * 3, [0] * 3, 10 ** 6)
        for k in ("hits", "score", "shape", "patches"):
            assert same(a[k], b[k]), (t, k)
        for k in ("nega_n", "carts_n", "next_start", "windows", "total_windows", "hits"):
            assert a["stats"][k] == b["stats"][k], (t, k)
        hits += len(a["hits"])
    assert hits > 0
    c.close()


@pytest.mark.parametrize("t", tr.ORIENTS)
def test_end_to_end_back_to_the_source_frame(built, gpu, model_file, t):
    """No rotation invariance assumed: S is the frame F turned back, so S turned by t IS F; detecting on the device-turned S
    gives F's results, and orient_back puts every box on the S pixels that, turned, are the F pixels under the box."""
    import torch
    from jda_amd import api, synth
    p, _ = model_file((3, 20, 5, 4), 4, seed=3, cart_th=-1.0)
    c = api.Cascador(p)
    F = synth.make_frames(1, 96, 80, seed=5)[0]
    inv = [s for s in tr.ORIENTS if np.array_equal(transform(transform(F, s), t), F)][0]
    S = transform(F, inv)
    buf, offs, ws, hs = c.pack_gray_oriented_device([torch.from_numpy(S).cuda()], "gray8", t, frame_stride=96 * 80)
    assert (ws, hs) == ([96], [80]) and np.array_equal(buf.cpu().numpy().reshape(80, 96), F)
    want = c.detect_batch(F[None], min_size=24)
    got = c.detect_batch_device(buf.view(1, 80, 96), min_size=24)
    _eq_c(got[0], want[0])
    assert len(got[0]["scores"]) > 0
    back = api.orient_back([S], "gray8", t, got)[0]
    assert same(back["scores"], got[0]["scores"])
    M = 128                                                                   # boxes may leave the frame: a margin on every side
    Fp, Sp = np.pad(F, M), np.pad(S, M)
    for (bx, by, bs), (x, y, s2) in zip(got[0]["bboxes"], back["bboxes"]):
        assert s2 == bs and min(bx, by, x, y) > -M and max(bx, by, x, y) + bs < M + 80
        assert np.array_equal(transform(Sp[y + M:y + M + bs, x + M:x + M + bs], t), Fp[by + M:by + M + bs, bx + M:bx + M + bs])
    lm = api.orient_back([S], "gray8", t, [0] * len(got[0]["scores"]), landmarks=got[0]["shapes"])[1]
    assert same(lm, back["shapes"])
    for f in range(len(lm)):
        assert same(lm[f], tr.back_landmarks(got[0]["shapes"][f], t, (0, 0) + S.shape[::-1]))
    c.close()
