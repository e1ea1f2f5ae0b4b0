"""Dialect CPP's work counters against the oracle's, entry by entry: jdaStats carries the reference's DetectionStatisic
(include/jda/cascador.hpp:14-25 -- face_patch_n, nonface_patch_n, cart_gothrough_n, average_cart_n, as src/test.cpp:146-157
sums and prints them) plus cart_total_n and stage_done_n.  oracle/jda_oracle.c counts the same quantities window by window in
its walks of Validate (orc_detect_cpp, orc_detect_cpp_pyramid_ms; the second reading counts them too,
tests/test_cpp_second_reading.py); every entry's counters must equal the oracle's sums exactly, and its detections the
oracle's bit for bit.  Also method 0 (the image pyramid, cascador.cpp:216-308) on two lanes, in sub-batches, at its geometry
edges and under lane contention."""
import threading

import numpy as np
import pytest

from conftest import same

pytestmark = pytest.mark.gpu

KEYS = ("patch_n", "face_patch_n", "nonface_patch_n", "cart_gothrough_n", "cart_total_n")
# cart thresholds of the three regimes: every window rejected by its first cart, a calibrated mix, every window a face
REGIMES = {"reject_all": 1e30, "mix": -1.0, "pass_all": -3.0e38}
# model kinds: dims, multi-scale split nodes, trainer header (stage, cart) or None for a finished model
MODELS = {"single": ((3, 20, 5, 4), False, None), "multi": ((2, 8, 5, 3), True, None),
          "snap_1_6": ((3, 20, 5, 4), False, (1, 6)), "snap_0_-1": ((3, 20, 5, 4), False, (0, -1))}


@pytest.fixture(scope="module")
def gpu():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    return torch.device("cuda", 0)


def _model(tmp_path, kind, cart_th, seed=3):
    from jda_amd import synth
    dims, multi, hdr = MODELS[kind]
    mdl = synth.make_model(*dims, seed=seed, cart_th=cart_th, norm_every=5, multi_scale=multi)
    p = str(tmp_path / ("%s_%d.model" % (kind, seed)))
    if hdr:
        mdl.save(p, 8, header_stage=hdr[0], header_cart=hdr[1])
    else:
        mdl.save(p, 8)
    return p, dims, hdr


def _eq(a, b, what=""):
    for k in ("rects", "scores", "shapes"):
        assert same(a[k], b[k]), (what, k, a[k].shape, b[k].shape)


def _sum(stats):
    tot = {k: sum(s[k] for s in stats) for k in KEYS}
    tot["stage_done_n"] = [sum(s["stage_done_n"][t] for s in stats) for t in range(16)]
    return tot


def _pack(results, L, frame_offset=0):
    """Rows [frame, x, y, w, h, score, shape...] of per-image results (what jdaResultsDPack makes of them)."""
    rows = [np.empty((0, 6 + 2 * L), np.float64)]
    for i, r in enumerate(results):
        m = np.empty((len(r["scores"]), 6 + 2 * L), np.float64)
        m[:, 0] = frame_offset + i; m[:, 1:5] = r["rects"]; m[:, 5] = r["scores"]; m[:, 6:] = r["shapes"]
        rows.append(m)
    return np.concatenate(rows)


def _check(got, want, dims, hdr, what=""):
    """The product's jdaStats against the oracle's sums.  Face, non-face and reject-length counters are Validate's.  A trainer
    snapshot runs on tables padded with pass-through carts (model_dev.cpp): a face walks all T x K carts and completes every
    stage, so cart_total_n and stage_done_n differ from Validate's literal walk by exactly the padding (include/jda.h)."""
    T, K = dims[0], dims[1]
    full = hdr[0] if hdr else T
    ran = full * K + (min(K, hdr[1] + 1) if hdr else 0)          # carts Validate runs for a face (cascador.cpp:177-209)
    for k in ("patch_n", "face_patch_n", "nonface_patch_n", "cart_gothrough_n"):
        assert got[k] == want[k], (what, k, got[k], want[k])
    faces = want["face_patch_n"]
    assert got["cart_total_n"] == want["cart_total_n"] + faces * (T * K - ran), (what, "cart_total_n", got["cart_total_n"], want)
    assert got["cart_total_n"] == got["cart_gothrough_n"] + faces * T * K, what
    for t in range(16):
        pad = faces if full <= t < T else 0
        assert got["stage_done_n"][t] == want["stage_done_n"][t] + pad, (what, "stage_done_n", t, got["stage_done_n"], want)
    # average_cart_n: the exact double cart_gothrough_n / nonface_patch_n; 0.0 when there is no non-face window (the reference
    # divides 0 by 0 there, cascador.cpp:307,375)
    avg = got["cart_gothrough_n"] / got["nonface_patch_n"] if got["nonface_patch_n"] else 0.0
    assert same(np.float64(got["average_cart_n"]), np.float64(avg)), (what, got["average_cart_n"], avg)


@pytest.mark.parametrize("regime", sorted(REGIMES))
@pytest.mark.parametrize("kind", sorted(MODELS))
def test_every_cpp_entry_counts_what_validate_counts(built, gpu, tmp_path, kind, regime):
    import torch
    from jda_amd import api, synth
    from oracle.pyoracle import Oracle
    p, dims, hdr = _model(tmp_path, kind, REGIMES[regime])
    multi = MODELS[kind][1]
    c, o = api.Cascador(p), Oracle(p)
    # -- method 1: a uniform batch from host memory and from HBM
    frames = synth.make_frames(3, 120, 90, seed=5)
    want = [o.detect_cpp(f, stats=True) for f in frames]
    ws = _sum([w["stats"] for w in want])
    if regime == "reject_all" and kind != "snap_0_-1":
        assert ws["face_patch_n"] == 0 and ws["cart_gothrough_n"] == ws["patch_n"] > 0
    elif regime == "pass_all" or kind == "snap_0_-1":
        assert ws["nonface_patch_n"] == 0 and ws["patch_n"] > 0
    else:
        assert 0 < ws["face_patch_n"] < ws["patch_n"]
    got, st = c.detect_batch_cpp(frames, stats=True)
    for i in range(len(frames)):
        _eq(got[i], want[i], ("batch", i))
    _check(st, ws, dims, hdr, "detect_batch_cpp")
    d_frames = torch.from_numpy(frames).cuda()
    got, st = c.detect_batch_cpp_device(d_frames, stats=True)
    for i in range(len(frames)):
        _eq(got[i], want[i], ("device", i))
    _check(st, ws, dims, hdr, "detect_batch_cpp_device")
    # -- method 1: ragged jobs (a multi-scale model runs them image by image: the per-image statistics are summed back)
    sizes = [(131, 97), (64, 48), (19, 60), (47, 61), (90, 70)]
    imgs = [synth.make_frames(1, w, h, seed=7, first=i)[0] for i, (w, h) in enumerate(sizes)]
    want = [o.detect_cpp(im, stats=True) for im in imgs]
    ws = _sum([w["stats"] for w in want])
    got, st = c.detect_ragged_cpp(imgs, stats=True)
    for i in range(len(imgs)):
        _eq(got[i], want[i], ("ragged", i))
    _check(st, ws, dims, hdr, "detect_ragged_cpp")
    buf = np.concatenate([im.reshape(-1) for im in imgs])
    offs = np.cumsum([0] + [w * h for w, h in sizes[:-1]])
    wd, ht = [w for w, _ in sizes], [h for _, h in sizes]
    d_buf = torch.from_numpy(buf).cuda()
    rows_want = _pack(want, dims[2], frame_offset=4)
    for src, where in ((buf, "host"), (d_buf, "device")):
        got, st = c.detect_ragged_cpp_packed(src, offs, wd, ht, stats=True)
        for i in range(len(imgs)):
            _eq(got[i], want[i], ("ragged packed", where, i))
        _check(st, ws, dims, hdr, "detect_ragged_cpp_packed " + where)
        rows, st = c.detect_ragged_cpp_packed(src, offs, wd, ht, stats=True, keep_results="packed", frame_offset=4)
        assert same(np.array(rows), rows_want), ("rows", where, rows.shape, rows_want.shape)
        _check(st, ws, dims, hdr, "detect_ragged_cpp_packed rows " + where)
    # -- method 0: the image pyramid, with the config's patch sizes (jdaDetectBatchCppPyramidMS) and, for a model without
    # multi-scale nodes, without them (jdaDetectBatchCppPyramid)
    pframes = synth.make_frames(2, 150, 121, seed=9)
    for hs, qs in ((36, 24),) + (() if multi else ((0, 0),)):
        want = [o.detect_cpp_pyramid(f, 48, 5, 1.2, 0.3, True, half_size=hs, quarter_size=qs, stats=True) for f in pframes]
        ws = _sum([w["stats"] for w in want])
        assert ws["patch_n"] == sum(w["windows"] for w in want)
        got, st = c.detect_batch_cpp_pyramid(pframes, 48, 5, 1.2, 0.3, True, stats=True, half_size=hs, quarter_size=qs)
        for i in range(len(pframes)):
            _eq(got[i], want[i], ("pyramid", hs, i))
        _check(st, ws, dims, hdr, "detect_batch_cpp_pyramid %d/%d" % (hs, qs))
    c.close(); o.close()


@pytest.mark.parametrize("kind,patches,step", [("single", (48, 0, 0), 5), ("multi", (48, 36, 24), 8), ("multi", (40, 27, 20), 8)])
def test_method_0_on_two_lanes_and_in_sub_batches(built, gpu, tmp_path, kind, patches, step):
    """lanes_min_windows = 1: every level of four 640x480 frames is split over two lanes (sub-batches on their own streams,
    each level's scan ordered behind the resize that made it); workspace_mb = 1: every level also runs as several passes per
    lane.  A multi-scale model owns per-window half / quarter patches in each lane's buffer -- the shipped 48 / 36 / 24 and an
    odd set.  Detections and counters equal the oracle's either way."""
    from jda_amd import api, synth
    from oracle.pyoracle import Oracle
    p, dims, hdr = _model(tmp_path, kind, -1.0)
    c, o = api.Cascador(p), Oracle(p)
    os_, hs, qs = patches
    frames = synth.make_frames(4, 640, 480, seed=21)
    want = [o.detect_cpp_pyramid(f, os_, step, 1.2, 0.3, True, half_size=hs, quarter_size=qs, stats=True) for f in frames]
    ws = _sum([w["stats"] for w in want])
    assert 0 < ws["face_patch_n"] < ws["patch_n"]
    c.set_option("lanes_min_windows", 1)
    for ws_mb in (None, 1):
        if ws_mb:
            c.set_option("workspace_mb", ws_mb)
        got, st = c.detect_batch_cpp_pyramid(frames, os_, step, 1.2, 0.3, True, stats=True, half_size=hs, quarter_size=qs)
        for i in range(len(frames)):
            _eq(got[i], want[i], (ws_mb, i))
        _check(st, ws, dims, hdr, "two lanes, workspace_mb %s" % ws_mb)
    c.close(); o.close()


# (width, height, frames, origin_size, step, factor)
EDGES = [(48, 48, 2, 48, 5, 1.2),        # exactly one level of one window
         (40, 40, 2, 48, 5, 1.2),        # smaller than the window: nothing to scan
         (47, 300, 1, 48, 5, 1.2),       # one side short of the window
         (200, 150, 2, 48, 5, 1.05),     # over 20 levels: the ping-pong level buffer is reused many times
         (60, 50, 2, 48, 20, 1.2),       # step larger than w - origin_size: one window per row and column
         (131, 97, 3, 48, 5, 1.2),       # odd sizes
         (131, 97, 3, 31, 3, 1.3)]       # odd window, step and factor


@pytest.mark.parametrize("edge", EDGES)
def test_method_0_geometry_edges(built, gpu, tmp_path, edge):
    from jda_amd import api, synth
    from oracle.pyoracle import Oracle
    w, h, n, os_, step, factor = edge
    p, dims, hdr = _model(tmp_path, "single", -1.0)
    c, o = api.Cascador(p), Oracle(p)
    frames = synth.make_frames(n, w, h, seed=w + h)
    for hs, qs in ((0, 0), (36, 24)):
        want = [o.detect_cpp_pyramid(f, os_, step, factor, 0.3, True, half_size=hs, quarter_size=qs, stats=True) for f in frames]
        ws = _sum([x["stats"] for x in want])
        got, st = c.detect_batch_cpp_pyramid(frames, os_, step, factor, 0.3, True, stats=True, half_size=hs, quarter_size=qs)
        assert len(got) == n
        for i in range(n):
            _eq(got[i], want[i], (edge, hs, i))
        _check(st, ws, dims, hdr, (edge, hs))
        if min(w, h) < os_:
            assert st["patch_n"] == 0 and all(len(g["scores"]) == 0 for g in got)
            assert got[0]["rects"].shape == (0, 4) and got[0]["shapes"].shape == (0, 2 * dims[2])
        if edge[:2] == (48, 48):
            assert st["patch_n"] == n and want[0]["levels"] == 1
        if factor == 1.05:
            assert want[0]["levels"] >= 20
    c.close(); o.close()


def test_method_0_one_frame_next_to_five(built, gpu, tmp_path):
    """The same entry with n = 1 and n = 5 (the first frame shared): per-frame results do not depend on the batch."""
    from jda_amd import api, synth
    from oracle.pyoracle import Oracle
    p, dims, hdr = _model(tmp_path, "single", -1.0)
    c, o = api.Cascador(p), Oracle(p)
    frames = synth.make_frames(5, 161, 119, seed=4)
    want = [o.detect_cpp_pyramid(f, 48, 5, 1.2, 0.3, True, stats=True) for f in frames]
    got1, st1 = c.detect_batch_cpp_pyramid(frames[:1], stats=True)
    got5, st5 = c.detect_batch_cpp_pyramid(frames, stats=True)
    _eq(got1[0], want[0], "n=1")
    for i in range(5):
        _eq(got5[i], want[i], ("n=5", i))
    _check(st1, _sum([want[0]["stats"]]), dims, hdr, "n=1")
    _check(st5, _sum([x["stats"] for x in want]), dims, hdr, "n=5")
    c.close(); o.close()


def test_method_0_under_lane_contention(built, gpu, tmp_path):
    """max_lanes = 2 on one cascador and three threads: two make method-0 calls that each want two lanes, one submits and
    waits dialect-C tickets (a pending ticket holds a lane) and makes method-1 calls.  A level may then run on fewer lanes
    than the level before it, or take a lane the earlier levels did not have; every lane a level uses must still be
    ordered behind the resize that made the level.  Every result is compared with oracle answers computed beforehand.
    A regression guard: the timing window of that race cannot be forced from outside."""
    import torch
    from jda_amd import api, synth
    from oracle.pyoracle import Oracle
    p, dims, hdr = _model(tmp_path, "single", -1.0)
    c, o = api.Cascador(p), Oracle(p)
    c.set_option("max_lanes", 2)
    c.set_option("lanes_min_windows", 1)
    pyr = [synth.make_frames(4, 320, 240, seed=31 + t) for t in range(2)]
    want_pyr = [[o.detect_cpp_pyramid(f, stats=True) for f in fr] for fr in pyr]
    cframes = synth.make_frames(4, 200, 150, seed=41)
    d_cframes = torch.from_numpy(cframes).cuda()
    want_c = [o.detect(f) for f in cframes]
    want_cpp = [o.detect_cpp(f) for f in cframes]
    reps = 4
    errors = []

    def pyramid(t):
        try:
            for r in range(reps):
                got, st = c.detect_batch_cpp_pyramid(pyr[t], stats=True)
                for i, g in enumerate(got):
                    _eq(g, want_pyr[t][i], ("pyramid thread", t, r, i))
                _check(st, _sum([w["stats"] for w in want_pyr[t]]), dims, hdr, ("pyramid thread", t, r))
        except Exception as e:           # noqa: BLE001
            errors.append(repr(e))

    def tickets():
        try:
            for r in range(reps):
                tk = c.submit_batch_device(d_cframes)
                got = c.wait_batch(tk)
                for i, g in enumerate(got):
                    for k in ("bboxes", "scores", "shapes"):
                        assert same(g[k], want_c[i][k]), ("ticket", r, i, k)
                got = c.detect_batch_cpp(cframes)
                for i, g in enumerate(got):
                    _eq(g, want_cpp[i], ("cpp", r, i))
        except Exception as e:           # noqa: BLE001
            errors.append(repr(e))
    ths = [threading.Thread(target=pyramid, args=(t,)) for t in range(2)] + [threading.Thread(target=tickets)]
    for th in ths:
        th.start()
    for th in ths:
        th.join(timeout=240)
    assert not any(th.is_alive() for th in ths), "a caller did not finish"
    assert not errors, errors
    c.close(); o.close()
