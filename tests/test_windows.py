"""jdaValidateWindows / jdaValidateWindowsDevice (k_windows.hip): the cascade on caller-given windows, compared EXACTLY --
 (1) on the reference's grid, against the CPU oracle's trace permuted and the GPU's own jdaTraceBatch;
 (2) against the reference's own compiled c/jda.c at the shipped dimensions (ref_detect_raw's boxes, scores, shapes);
 (3) off the grid, against tests/windows_ref.py (pinned to the oracle by tests/test_windows_host.py);
 (4) host entry = device entry, LDS-tile form = global-read form, chunked = unchunked; th; statistics; refusals; threads."""
import ctypes as C
import threading

import numpy as np
import pytest

import windows_ref
from conftest import S_DIMS, same, bits
from test_windows_host import make_case

pytestmark = pytest.mark.gpu

OUT_KEYS = ("is_face", "score", "carts_n", "path_hash", "shapes", "landmarks")
SCAN = dict(scale=1.25, min_size=24, max_size=-1)


@pytest.fixture(scope="module")
def gpu():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    return torch.device("cuda", 0)


def assert_same(got, want, keys=OUT_KEYS, what=""):
    for k in keys:
        assert same(got[k], want[k]), (what, k, int((bits(got[k]) != bits(want[k])).reshape(len(got[k]), -1).any(1).sum()))


def relocate(shapes, xs, ys, sizes):
    """c/jda.c:471-472 in fp32: a multiply, then an add."""
    lm = (shapes * sizes.astype(np.float32)[:, None]).astype(np.float32)
    lm[:, 0::2] = lm[:, 0::2] + xs.astype(np.float32)[:, None]
    lm[:, 1::2] = lm[:, 1::2] + ys.astype(np.float32)[:, None]
    return lm


def face_of(m, carts_n, score, th):
    """c/jda.c:399 and 414 from the trace outputs: a window is a face when no cart rejected it -- carts_n == T*K alone does not say
    so, the LAST cart may have been the rejecting one (its index + 1 is T*K too) -- and the final threshold does not either."""
    last = np.float32(m.cth[-1, -1])
    return ((carts_n == m.T * m.K) & ~(score < last) & ~(score < np.float32(th))).astype(np.uint8)


def cascade_model(dims, multi, seed, frame_size):
    """A model whose thresholds make windows end everywhere: calibrated on the scale-0 copy of its nodes with a survival curve
    that is still falling in stage 1."""
    from jda_amd import synth
    m = synth.make_model(*dims, seed=seed, multi_scale=multi, norm_every=7)
    scale = m.scale.copy()
    m.scale[:] = 0
    synth.calibrate_thresholds(m, synth.make_frames(3, frame_size[0], frame_size[1], seed=seed + 50), tau=0.7 * dims[1], p_final=0.05, min_size=24)
    m.scale = scale
    return m


# ---------------------------------------------------------------- (1) on the grid

@pytest.mark.parametrize("multi", [False, True], ids=["scale0", "multiscale"])
@pytest.mark.parametrize("D", [2, 4])
@pytest.mark.parametrize("L", [5, 27])
@pytest.mark.parametrize("T,K", [(2, 3), (2, 64), (2, 65), (3, 130)])
def test_grid_windows_equal_oracle_and_gpu_trace(built, gpu, tmp_path, T, K, L, D, multi):
    from jda_amd import api, synth
    from oracle.pyoracle import Oracle
    m = cascade_model((T, K, L, D), multi, seed=T * 1000 + K + L + D, frame_size=(80, 64))
    p = str(tmp_path / "m.model")
    m.save(p, 8)
    c, orc = api.Cascador(p), Oracle(p)
    th = -0.5
    carts_seen = []
    for w, h in [(64, 48), (80, 64)]:
        frames = synth.make_frames(2, w, h, seed=w)
        g = np.array(windows_ref.grid(w, h, **SCAN), np.int32).reshape(-1, 3)
        nw = len(g)
        win = np.concatenate([np.column_stack([np.full(nw, f, np.int32), g]) for f in range(len(frames))])
        perm = np.random.default_rng(w + K).permutation(len(win))
        got = c.validate_windows(frames, win[perm], th=th)
        tr = [orc.trace(frames[f], **SCAN) for f in range(len(frames))]
        want = {k: np.concatenate([t[k] for t in tr])[perm] for k in ("carts_n", "score", "path_hash", "shapes")}
        want["is_face"] = face_of(m, want["carts_n"], want["score"], th)
        want["landmarks"] = relocate(want["shapes"], win[perm, 1], win[perm, 2], win[perm, 3])
        assert_same(got, want, what=(w, h, "oracle"))
        gt = c.trace(frames, **SCAN)
        assert_same(got, {k: gt[k][perm] for k in gt}, keys=("carts_n", "score", "path_hash", "shapes"), what=(w, h, "gpu trace"))
        carts_seen.append(want["carts_n"])
    cs = np.concatenate(carts_seen)
    assert (cs < T * K).any() and (cs == T * K).any(), "the case must hold rejected and complete walks"


# ---------------------------------------------------------------- (2) the compiled reference, shipped dimensions

def test_shipped_dims_equal_compiled_reference(built, gpu, tmp_path):
    """... and the compiled reference decides what is_face means for a window the LAST cart rejects: its carts_n is T*K and its
    score may well pass the final threshold, yet c/jda.c:399 sends it to `next` before c/jda.c:414 is reached.  The model's last
    cart gets a threshold inside the range of the final scores of this frame's complete walks (1.7 .. 45), so that such windows
    exist here; the test asserts that they do."""
    from jda_amd import api, synth
    from oracle import pyoracle
    assert pyoracle.reference_lib_path(*S_DIMS), "the reference build of the shipped dimensions (oracle.build) did not travel"
    m = synth.make_model(*S_DIMS, seed=1, cart_th=-2.0)
    m.cth[-1, -1] = 23.5
    p = str(tmp_path / "last_cart.model")
    m.save(p, 8)
    frame = synth.make_frames(1, 160, 120, seed=14)[0]
    th = -0.5
    ref = pyoracle.Reference(p, S_DIMS, 8).detect_raw(frame, th=th)          # scan order, before NMS and relocation
    g = np.array(windows_ref.grid(160, 120, scale=1.25, min_size=40), np.int32).reshape(-1, 3)
    win = np.column_stack([np.zeros(len(g), np.int32), g])
    got = api.Cascador(p, "double").validate_windows(frame[None], win, th=th)
    face = got["is_face"].astype(bool)
    assert len(ref["scores"]) > 0
    last_cart = (got["carts_n"] == m.T * m.K) & ~(got["score"] < np.float32(th)) & ~face
    assert last_cart.sum() > 0, "no window is rejected by the last cart with a score that passes th: the case decides nothing"
    assert (got["score"][last_cart] < np.float32(23.5)).all()
    assert np.array_equal(g[face], ref["bboxes"])
    assert same(got["score"][face], ref["scores"])
    assert same(got["shapes"][face], ref["shapes"])
    assert same(got["landmarks"][face], relocate(ref["shapes"], ref["bboxes"][:, 0], ref["bboxes"][:, 1], ref["bboxes"][:, 2]))


def test_trainer_snapshot_gets_the_trace_answer(built, gpu, tmp_path):
    """Dialect C ignores a file's training status (c/jda.c:499-505): a snapshot walks T x K carts, in jdaTraceBatch and here."""
    from jda_amd import api, synth
    from oracle.pyoracle import Oracle
    m = cascade_model((3, 20, 5, 4), True, seed=9, frame_size=(80, 64))
    p, full = str(tmp_path / "snap.model"), str(tmp_path / "full.model")
    m.save(p, 8, header_stage=1, header_cart=6)          # stage 1 in training, seven carts of it placed
    m.save(full, 8)
    frames = synth.make_frames(2, 80, 64, seed=2)
    g = np.array(windows_ref.grid(80, 64, **SCAN), np.int32).reshape(-1, 3)
    win = np.concatenate([np.column_stack([np.full(len(g), f, np.int32), g]) for f in range(2)])
    c = api.Cascador(p)
    got, gt = c.validate_windows(frames, win), c.trace(frames, **SCAN)
    assert_same(got, gt, keys=("carts_n", "score", "path_hash", "shapes"))
    assert (got["carts_n"] > 20 + 7).any(), "no window walks past the status the header names"
    tr = [Oracle(full).trace(frames[f], **SCAN) for f in range(2)]
    assert_same(got, {k: np.concatenate([t[k] for t in tr]) for k in tr[0]}, keys=("carts_n", "score", "path_hash", "shapes"))


# ---------------------------------------------------------------- (3) off the grid

OFF_W, OFF_H = 120, 96
COUNTS = [0, 1, 63, 64, 65, 257]


@pytest.fixture(scope="module", params=[False, True], ids=["scale0", "multiscale"])
def offgrid(request, built, tmp_path_factory):
    """Model, a 5-frame batch, 257 windows no grid would produce, and windows_ref's answer for them (computed once)."""
    from jda_amd import api, synth
    multi = request.param
    dims = (3, 20, 5, 4)
    m, _ = make_case(dims, (80, 64), 5, 9.0, multi)
    d = tmp_path_factory.mktemp("offgrid")
    frames = synth.make_frames(5, OFF_W, OFF_H, seed=21)
    limit = api.Cascador(m.save(str(d / "dims.model"), 8)).get_option("windows_tile_limit")      # (depends on the dimensions only)
    assert (limit == 0) if multi else (24 < limit < min(OFF_W, OFF_H) - 1), limit
    W, H = OFF_W, OFF_H
    win = [(0, 1, 3, 1), (2, 117, 95, 1), (4, 5, 7, 2), (0, 33, 17, 23), (2, 35, 19, 24), (4, 37, 21, 25),          # sizes 1, 2, 23, 24, 25
           (0, 0, 0, min(W, H)), (2, W - min(W, H), 0, min(W, H)),                                                 # size = min(W, H)
           (4, W - 24, H - 24, 24), (0, W - 25, H - 25, 25), (2, W - 61, H - 61, 61), (4, W - 95, H - 95, 95),      # flush right and bottom
           (0, W - 31, 9, 31), (2, 11, H - 47, 47),
           (2, 35, 19, 24), (2, 35, 19, 24), (0, 1, 3, 1)]                                                          # duplicates
    if limit:
        win += [(0, 3, 1, limit - 1), (2, 5, 3, limit), (4, 7, 5, limit + 1), (0, W - limit, H - limit, limit), (2, W - limit - 1, H - limit - 1, limit + 1)]
    rng = np.random.default_rng(77)
    while len(win) < COUNTS[-1]:
        s = int(rng.integers(1, min(W, H) + 1))
        win.append((int(rng.choice([0, 2, 4])), int(rng.integers(0, W - s + 1)), int(rng.integers(0, H - s + 1)), s))
    win = np.array(win, np.int32)
    assert set(win[:, 0]) == {0, 2, 4} and (win[:, 1] % 2 == 1).any() and (win[:, 2] % 2 == 1).any()
    th = -0.5
    # the last cart's threshold (never-reject as calibrated) -> the median final score of the complete walks: about half of them are
    # now rejected by the LAST cart, carts_n == T*K, some with a score that passes th -- is_face must be 0 for those (c/jda.c:399)
    first = windows_ref.validate(windows_ref.RefModel(m), frames, win, th=th)
    m.cth[-1, -1] = float(np.float32(np.median(first["score"][~first["rejected"]])))
    p = m.save(str(d / "m.model"), 8)
    c = api.Cascador(p)
    want = windows_ref.validate(windows_ref.RefModel(m), frames, win, th=th)
    last_cart = want["rejected"] & (want["carts_n"] == dims[0] * dims[1]) & ~(want["score"] < np.float32(th))
    assert last_cart.any() and not want["is_face"][last_cart].any() and want["is_face"].any()
    for k in want:
        want[k].setflags(write=False)
    cs = want["carts_n"]
    assert (cs == 1).any() and ((cs > dims[1]) & (cs < dims[0] * dims[1])).any() and (cs == dims[0] * dims[1]).any()
    assert np.array_equal(want["is_face"], face_of(m, cs, want["score"], th))
    return dict(c=c, path=p, frames=frames, win=win, want=want, th=th, limit=limit, dims=dims, model=m)


@pytest.mark.parametrize("n", COUNTS)
def test_offgrid_windows_equal_restatement(gpu, offgrid, n):
    o = offgrid
    got = o["c"].validate_windows(o["frames"], o["win"][:n], th=o["th"])
    assert len(got["score"]) == n
    assert_same(got, {k: o["want"][k][:n] for k in OUT_KEYS}, what=n)


# ---------------------------------------------------------------- (4) entries, forms, chunks

def test_host_entry_equals_device_entry(gpu, offgrid):
    import torch
    o = offgrid
    host = o["c"].validate_windows(o["frames"], o["win"], th=o["th"])
    dev = o["c"].validate_windows(torch.from_numpy(o["frames"]).to(gpu), o["win"], th=o["th"])
    dev2 = o["c"].validate_windows(o["frames"], o["win"], th=o["th"], device=True)
    assert_same(dev, host)
    assert_same(dev2, host)
    assert_same(host, o["want"])


def test_lds_tile_form_equals_global_read_form(gpu, offgrid):
    from jda_amd import api
    o = offgrid
    c0 = api.Cascador(o["path"])
    c0.set_option("windows_tile", 0)                     # every pixel from the frame
    c1 = api.Cascador(o["path"])
    c1.set_option("windows_tile", 30)                    # a tile limit of its own: sizes 30 and 31 sit on either side of it
    a, b, d = (c.validate_windows(o["frames"], o["win"], th=o["th"]) for c in (c0, c1, o["c"]))
    assert_same(a, d)
    assert_same(b, d)
    assert_same(a, o["want"])
    with pytest.raises(api.JdaError):
        c0.set_option("windows_tile_limit", 3)           # read-only


def test_chunked_call_equals_unchunked(built, gpu, tmp_path):
    from jda_amd import api, synth
    m = cascade_model((2, 65, 27, 4), False, seed=31, frame_size=(80, 64))
    p = str(tmp_path / "m.model")
    m.save(p, 8)
    frames = synth.make_frames(5, 80, 64, seed=5)
    g = np.array(windows_ref.grid(80, 64, **SCAN), np.int32).reshape(-1, 3)
    win = np.concatenate([np.column_stack([np.full(len(g), f, np.int32), g]) for f in range(5)])
    win = win[np.random.default_rng(3).permutation(len(win))]
    per_window = 16 + 13 + 2 * 4 * m.dim + 64            # windows.cpp: what a window takes of the workspace
    assert len(win) * per_window > 2 << 20, "the call must need at least three chunks of workspace_mb = 1"
    c = api.Cascador(p)
    whole = c.validate_windows(frames, win)
    small = api.Cascador(p)
    small.set_option("workspace_mb", 1)
    assert_same(small.validate_windows(frames, win), whole)
    assert_same(small.validate_windows(frames, win, device=True), whole)


def test_final_threshold_flips_only_is_face_and_stats_count_the_outputs(gpu, offgrid):
    o = offgrid
    i = int(np.flatnonzero(face_of(o["model"], o["want"]["carts_n"], o["want"]["score"], -3.0e38))[0])      # a window no cart rejects
    s = o["want"]["score"][i]
    lo, hi = np.nextafter(s, np.float32(-np.inf)), np.nextafter(s, np.float32(np.inf))
    a, sa = o["c"].validate_windows(o["frames"], o["win"], th=float(lo), stats=True)
    b, sb = o["c"].validate_windows(o["frames"], o["win"], th=float(hi), stats=True)
    e = o["c"].validate_windows(o["frames"], o["win"], th=float(s))
    assert a["is_face"][i] == 1 and e["is_face"][i] == 1 and b["is_face"][i] == 0          # c/jda.c:414: score < th rejects
    assert_same(a, b, keys=("score", "carts_n", "path_hash", "shapes", "landmarks"))
    for got, st, th in ((a, sa, lo), (b, sb, hi)):
        face = face_of(o["model"], got["carts_n"], got["score"], th).astype(bool)
        assert np.array_equal(got["is_face"], face.astype(np.uint8))
        assert st["patch_n"] == len(face) and st["face_patch_n"] == int(face.sum()) and st["nonface_patch_n"] == int((~face).sum())
        assert st["cart_gothrough_n"] == int(got["carts_n"][~face].astype(np.int64).sum())
        assert st["average_cart_n"] == st["cart_gothrough_n"] / st["nonface_patch_n"]
        assert st["call_ms"] > 0
    assert sa["face_patch_n"] > sb["face_patch_n"]


# ---------------------------------------------------------------- refusals

def raw_call(c, frames, win, n=None, n_windows=None, width=None, height=None, null=(), frame_ptrs=None, device_ptr=None, stride=None):
    """The C entry itself on canary-filled outputs -> (return code, message, outputs untouched?)."""
    from jda_amd import api
    lib = api.lib
    nf, h, w = frames.shape
    win = np.ascontiguousarray(win, np.int32).reshape(-1, 4)
    cap = max(len(win), 4)
    dim = c.dim
    outs = [np.full(cap, 0xA5, np.uint8), np.full(cap, -7.25, np.float32), np.full(cap, -77, np.int32), np.full(cap, 0xDEADBEEF, np.uint32),
            np.full((cap, dim), -3.5, np.float32), np.full((cap, dim), -9.5, np.float32)]
    before = [a.copy() for a in outs]
    st = api.jdaStats()
    st.patch_n = -123
    ty = [C.c_ubyte, C.c_float, C.c_int, C.c_uint, C.c_float, C.c_float]
    ptrs = [None if k in null else a.ctypes.data_as(C.POINTER(t)) for k, a, t in zip(OUT_KEYS, outs, ty)]
    tail = (nf if n is None else n, w if width is None else width, h if height is None else height,
            None if "windows" in null else win.ctypes.data_as(C.POINTER(C.c_int)), len(win) if n_windows is None else n_windows, -0.5,
            *ptrs, C.byref(st))
    if device_ptr is not None:
        rc = lib.jdaValidateWindowsDevice(c.h, C.c_void_p(device_ptr), w * h if stride is None else stride, *tail)
    else:
        fp = frame_ptrs if frame_ptrs is not None else (None if "frames" in null else api._frame_ptrs(frames))
        rc = lib.jdaValidateWindows(c.h, fp, *tail)
    untouched = all(np.array_equal(a, b) for a, b in zip(outs, before)) and st.patch_n == -123
    return rc, api.last_error(), untouched, outs


def test_refusals_name_the_window_and_touch_nothing(gpu, offgrid):
    import torch
    from jda_amd import api
    o = offgrid
    c, frames = o["c"], o["frames"]
    W, H, n = OFF_W, OFF_H, len(frames)
    good = [(0, 1, 3, 24), (2, 5, 7, 30), (4, 9, 11, 1)]
    bad_windows = [(-1, 0, 0, 24), (n, 0, 0, 24), (0, 0, 0, 0), (0, 0, 0, -5), (1, -1, 0, 24), (1, 0, -1, 24),
                   (3, W - 23, 0, 24), (3, 0, H - 23, 24), (0, 0, 0, H + 1), (0, 2 ** 31 - 1, 0, 24), (0, 0, 2 ** 31 - 1, 2 ** 31 - 1)]
    for pos in (0, 2, 3):
        for bw in bad_windows:
            win = list(good)
            win.insert(pos, bw)
            rc, msg, untouched, _ = raw_call(c, frames, win)
            assert rc == -1 and untouched, (bw, msg)
            assert "window %d " % pos in msg and "(%d, %d, %d, %d)" % bw in msg, (bw, msg)
    d_frames = torch.from_numpy(frames).to(gpu)
    null_ptrs = (C.c_void_p * n)(*([frames.ctypes.data] * (n - 1) + [None]))
    others = [dict(null=("windows",)), dict(null=("frames",)), dict(frame_ptrs=C.cast(null_ptrs, C.POINTER(C.POINTER(C.c_ubyte)))),
              dict(n=-1), dict(n_windows=-1), dict(n=0), dict(width=0), dict(height=0), dict(width=-3), dict(width=70000), dict(height=65536),
              dict(device_ptr=0), dict(device_ptr=d_frames.data_ptr(), stride=W * H - 1), dict(device_ptr=d_frames.data_ptr(), n_windows=-2)]
    for kw in others:
        rc, msg, untouched, _ = raw_call(c, frames, good, **kw)
        assert rc == -1 and untouched and msg, (kw, msg)
    with pytest.raises(api.JdaError, match="window 1 "):
        c.validate_windows(frames, [good[0], (0, W, 0, 1)])
    # accepted: no windows at all (nothing is touched, whatever else is passed); outputs the caller does not want
    for kw in (dict(), dict(null=("windows", "frames")), dict(n=0)):
        rc, msg, untouched, _ = raw_call(c, frames, np.zeros((0, 4), np.int32), **kw)
        assert rc == 0 and untouched, (kw, msg)
    rc, msg, untouched, outs = raw_call(c, frames, o["win"], null=("is_face", "path_hash", "shapes"))
    assert rc == 0 and not untouched, msg
    assert same(outs[1], o["want"]["score"]) and same(outs[2], o["want"]["carts_n"]) and same(outs[5], o["want"]["landmarks"])
    assert (outs[0] == 0xA5).all() and (outs[3] == 0xDEADBEEF).all() and (outs[4] == np.float32(-3.5)).all()
    # ... and a valid call right after the refusals
    assert_same(c.validate_windows(frames, o["win"], th=o["th"]), o["want"])


# ---------------------------------------------------------------- threads

def test_two_threads_on_one_cascador(gpu, offgrid):
    o = offgrid
    res, errs = [None, None], []

    def work(i):
        try:
            r = None
            for _ in range(4):
                r = o["c"].validate_windows(o["frames"], o["win"], th=o["th"], device=bool(i))
                assert_same(r, o["want"])
            res[i] = r
        except Exception as e:      # noqa: BLE001 -- reported by the main thread
            errs.append(e)
    ts = [threading.Thread(target=work, args=(i,)) for i in range(2)]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    assert not errs, errs
    assert_same(res[0], res[1])
