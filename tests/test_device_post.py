"""k_post, the per-frame post-processing of a dialect-C batch on the device (jda_amd/csrc/k_post.hip: detections back into
scan order, the reference's score order, greedy NMS, scan-order output, relocation; c/jda.c:237-316), must give exactly
what the host form gives (post.cpp, itself checked against the compiled reference: tests/test_nms.py, golden `score_ties`)
-- boxes, score bits, landmark bits, frame by frame -- including where it declines (a frame with more than 1,024
detections, ties among more than 256) and the host takes the pass.  `device_post` is read at every call.

Which form delivered a call is read from jdaStats: `post_passes` (passes whose frames k_post delivered) and `post_declined`
(passes in which it was launched and raised its flag).  Every test says what it expects of them and prints what it saw:
a comparison of the host form with itself would pass as well."""
import numpy as np
import pytest

from conftest import S_DIMS, same

pytestmark = pytest.mark.gpu

ONE_LEVEL = dict(scale=1.25, min_size=30, max_size=30)      # one pyramid level: windows of 30 pixels, step 3
ALL = -3.0e38                                               # final threshold nothing fails (NaN does not fail any)


@pytest.fixture(scope="module")
def gpu():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    return torch.device("cuda", 0)


def _expect(what, st, tag):
    """what: "none" (k_post not launched), "posted", "declined", "both", "no_decline" (launched or not, never declined)."""
    pp, pd = st["post_passes"], st["post_declined"]
    print("  %-28s post_passes %d  post_declined %d  ws_regrows %d  dense_passes %d   (expected: %s)"
          % (tag, pp, pd, st["ws_regrows"], st["dense_passes"], what))
    ok = {"none": pp == 0 and pd == 0, "posted": pp >= 1 and pd == 0, "declined": pp == 0 and pd >= 1,
          "both": pp >= 1 and pd >= 1, "no_decline": pd == 0}[what]
    assert ok, (tag, what, pp, pd)


def _both(casc, dev, expect, first="none", **kw):
    """The same batch with device_post = 1 (three calls: the first pass on a plan has no prediction of its queues, so
    k_post is not launched; the later ones are `expect`) and with device_post = 0 (never launched): equal, bit for bit.
    -> the host form's results and the statistics of the last device_post = 1 call."""
    print()
    casc.set_option("device_post", 1)
    outs = []
    for i in range(3):
        got, st = casc.detect_batch_device(dev, stats=True, **kw)
        _expect(first if i == 0 else expect, st, "device_post=1 call %d" % i)
        outs.append(got)
    casc.set_option("device_post", 0)
    for i in range(2):
        host, st0 = casc.detect_batch_device(dev, stats=True, **kw)
        _expect("none", st0, "device_post=0 call %d" % i)
    for got in outs:
        assert len(got) == len(host)
        for i, (a, b) in enumerate(zip(host, got)):
            for k in ("bboxes", "scores", "shapes"):
                assert same(a[k], b[k]), (i, k, len(a["scores"]), len(b["scores"]))
    if expect in ("posted", "declined"):
        # the expectation follows from the kernel's documented limits and the batch's raw detections (host form, no NMS)
        raw = casc.detect_batch_device(dev, **dict(kw, nms=False))
        assert _k_post_takes([r["scores"] for r in raw], kw.get("nms", True)) == expect
    return host, st


def _k_post_takes(raw_scores, nms):
    """What k_post does with a pass, from its documented limits alone: it declines when a frame has more than 1,024
    detections or, under NMS (without it no order is needed), ties or NaN among more than 256."""
    for s in raw_scores:
        s = np.asarray(s, np.float32)
        tied = np.isnan(s).any() or len(np.unique(s)) < len(s)
        if len(s) > 1024 or (nms and len(s) > 256 and tied):
            return "declined"
    return "posted"


@pytest.mark.parametrize("nms", [True, False])
def test_device_post_equals_host_post_shipped_dimensions(built, gpu, model_file, nms):
    import torch
    from jda_amd import api, synth
    from oracle.pyoracle import Oracle
    p, _ = model_file(S_DIMS, 8, seed=3, cart_th=-2.0, norm_every=5)
    frames = synth.make_frames(40, 320, 240, seed=21)
    c = api.Cascador(p)
    c.set_option("dense", 0)       # (in auto mode this batch runs dense, k_stage, from its first call: k_post is never launched)
    host, _ = _both(c, torch.from_numpy(frames).cuda(), "posted", th=-0.5, nms=nms)
    assert sum(len(h["scores"]) for h in host) > 40
    o = Oracle(p)
    for i in ((0, 17, 39) if nms else ()):       # (the oracle's raw list is checked against the host form elsewhere)
        want = o.detect(frames[i], th=-0.5, nms=nms)
        for k in ("bboxes", "scores", "shapes"):
            assert same(want[k], host[i][k]), (i, k)
    c.close()


@pytest.mark.parametrize("dims,size,n", [((1, 4, 3, 2), (64, 64), 24),      # a handful of leaf values: ties everywhere, few windows (literal order on the device)
                                         ((1, 4, 3, 2), (200, 150), 20),   # ... and thousands of tied detections per frame (declined: host form)
                                         ((2, 8, 5, 3), (160, 120), 32)])
def test_ties_and_crowded_frames(built, gpu, model_file, dims, size, n):
    """Dense mode off: a model under which every window survives would otherwise go through k_stage (or, with too few
    windows for it, through the unpredicted path), and neither launches k_post -- see the test below."""
    import torch
    from jda_amd import api, synth
    from oracle.pyoracle import Oracle
    p, _ = model_file(dims, 8, seed=5, cart_th=synth.NEG_BIG)      # nothing is rejected: every window is a detection
    frames = synth.make_frames(n, size[0], size[1], seed=22)
    o = Oracle(p)
    expect = _k_post_takes([o.detect(f, th=ALL, nms=False)["scores"] for f in frames], True)
    assert expect == {(64, 64): "posted", (200, 150): "declined", (160, 120): "declined"}[size]     # (983 windows a frame, tied ones among them)
    c = api.Cascador(p)
    c.set_option("dense", 0)
    host, _ = _both(c, torch.from_numpy(frames).cuda(), expect, th=ALL)
    assert sum(len(h["scores"]) for h in host) > 0
    c.close()


def test_all_pass_model_in_auto_dense_mode_never_posts(built, gpu, model_file):
    """dense = 1 (the default) and a small model that rejects nothing: Pass::issue_rest leaves the predicted path -- the
    only one that launches k_post -- to whatever dense mode decides (here: 696 windows, too few for k_stage, finished
    window by window after a host wait).  The results are the host form's; written down so that it is not implicit."""
    import torch
    from jda_amd import api, synth
    p, _ = model_file((1, 4, 3, 2), 8, seed=5, cart_th=synth.NEG_BIG)
    frames = synth.make_frames(24, 64, 64, seed=22)
    c = api.Cascador(p)
    assert c.get_option("dense") == 1
    host, _ = _both(c, torch.from_numpy(frames).cuda(), "none", th=ALL)
    assert sum(len(h["scores"]) for h in host) > 0
    c.close()


def test_two_lanes_and_sub_batches(built, gpu, model_file, monkeypatch):
    """A batch that goes through two lanes in several sub-batches (workspace of 64 MB): every pass posts its own frames
    (in the first call the later rounds already have the first round's prediction: not pinned to 0 there).  Dense mode
    off (in auto mode every pass of this batch runs k_stage) and a final threshold that leaves every frame at most 256
    detections: at -0.5 most frames have more than 1,024, and some tied scores, and k_post declines every pass."""
    import torch
    from jda_amd import api, synth
    p, _ = model_file((3, 20, 5, 4), 8, seed=3, cart_th=-1.0, norm_every=5)
    frames = synth.make_frames(96, 200, 150, seed=23)
    monkeypatch.setenv("JDA_WORKSPACE_MB", "8"); monkeypatch.setenv("JDA_LANES_MIN_WINDOWS", "1000")
    c = api.Cascador(p)
    c.set_option("dense", 0)
    host, st = _both(c, torch.from_numpy(frames).cuda(), "posted", first="no_decline", th=5.0)
    assert st["post_passes"] >= 2                               # (more than one pass in the call, each posted)
    assert sum(len(h["scores"]) for h in host) > 96
    c.close()


def test_submit_wait_tickets_use_it_too(built, gpu, model_file):
    """Tickets 0-2 are submitted before any pass on the plan has been collected (no prediction: not launched), tickets
    3 and 4 after: posted.  Dense mode off and a final threshold of 5.0, as in test_two_lanes_and_sub_batches."""
    import torch
    from jda_amd import api, synth
    p, _ = model_file((3, 20, 5, 4), 8, seed=3, cart_th=-1.0, norm_every=5)
    frames = synth.make_frames(48, 200, 150, seed=24)
    dev = torch.from_numpy(frames).cuda()
    c = api.Cascador(p)
    c.set_option("dense", 0); c.set_option("device_post", 1)
    print()
    q = [c.submit_batch_device(dev, th=5.0) for _ in range(2)]
    results = []
    for k in range(5):
        if k < 3:
            q.append(c.submit_batch_device(dev, th=5.0))
        got, st = c.wait_batch(q.pop(0), stats=True)
        _expect("none" if k < 3 else "posted", st, "ticket %d" % k)
        results.append(got)
    c.set_option("device_post", 0)
    for i in range(2):
        want, st0 = c.detect_batch_device(dev, th=5.0, stats=True)
        _expect("none", st0, "device_post=0 call %d" % i)
    assert _k_post_takes([r["scores"] for r in c.detect_batch_device(dev, th=5.0, nms=False)], True) == "posted"
    for k, got in enumerate(results):
        assert len(got) == len(want)
        for a, b in zip(want, got):
            for key in ("bboxes", "scores", "shapes"):
                assert same(a[key], b[key]), (k, key)
    assert sum(len(w["scores"]) for w in want) > 48
    c.close()


def test_ragged_chunks_posted_and_declined(built, gpu, model_file):
    """The ragged branch of k_post (an image's gids are one range of the chunk, its window grids are re-derived on the
    device from its size) against the host form, bit for bit: images of mixed sizes in several chunks, one too small
    for any window (n_lv == 0), a flat image whose 1,998 windows all pass with ONE score (crowded and tied: its chunk
    is declined and goes through the host form while the other chunks are posted), a small flat image (ties replayed
    literally on the device), from host memory and from one packed device buffer."""
    import torch
    from jda_amd import api, synth
    p, _ = model_file((3, 20, 5, 4), 8, seed=2, cart_th=-0.5, norm_every=5)
    base = synth.make_frames(8, 200, 150, seed=22)
    rng = np.random.default_rng(4)
    imgs = []
    for i in range(64):
        w, h = int(rng.integers(120, 201)), int(rng.integers(100, 151))
        imgs.append(np.ascontiguousarray(base[i % 8][:h, :w]))
    imgs[5] = np.ascontiguousarray(base[0][:20, :20])                 # no window fits
    imgs[9] = np.full((150, 200), 128, np.uint8)                      # every window passes, every score equal
    imgs[44] = np.full((60, 70), 90, np.uint8)                        # a handful of tied detections
    c = api.Cascador(p)
    c.set_option("ragged_chunk_windows", 25000); c.set_option("ragged_chunk_min_windows", 1000)
    c.set_option("device_post_min_frames", 4)
    c.set_option("dense", 0)       # (in auto mode a chunk that keeps 40 % of its windows alive leaves the predicted path, and with it k_post)
    offs, tot = [], 0
    for im in imgs:
        offs.append(tot); tot += im.size
    buf = torch.from_numpy(np.concatenate([im.reshape(-1) for im in imgs])).cuda()
    ws, hs = [im.shape[1] for im in imgs], [im.shape[0] for im in imgs]
    print()
    for nms in (True, False):
        c.set_option("device_post", 0)
        for rep in range(2):
            host, st0 = c.detect_ragged(imgs, th=-0.5, nms=nms, stats=True)
            _expect("none", st0, "nms %d device_post=0 job %d" % (nms, rep))
        c.set_option("device_post", 1)
        for rep in range(3):
            # host images: several chunks, image 9's declined, others posted; the packed device buffer is ONE chunk
            # (ragged_single_windows), declined as a whole because of image 9
            for what, (got, st) in (("both", c.detect_ragged(imgs, th=-0.5, nms=nms, stats=True)),
                                    ("declined", c.detect_ragged_packed(buf, offs, ws, hs, th=-0.5, nms=nms, stats=True))):
                _expect(what, st, "nms %d job %d %s" % (nms, rep, "host images" if what == "both" else "packed"))
                assert len(got) == len(host) == 64
                for i, (a, b) in enumerate(zip(host, got)):
                    for k in ("bboxes", "scores", "shapes"):
                        assert same(a[k], b[k]), (nms, rep, i, k, len(a["scores"]), len(b["scores"]))
        assert len(host[5]["scores"]) == 0
        if not nms:
            assert len(host[9]["scores"]) == 1998 and len(np.unique(host[9]["scores"])) == 1
            assert 0 < len(host[44]["scores"]) <= 256 and len(np.unique(host[44]["scores"])) == 1
    # per image the ragged job is jdaDetect on that image
    full = c.detect_ragged(imgs, th=-0.5)
    for i in (0, 9, 44, 63):
        one = c.detect(imgs[i], th=-0.5)
        for k in ("bboxes", "scores", "shapes"):
            assert same(one[k], full[i][k]), (i, k)
    c.close()


# ---- k_post at its limits: the smallest frames that reach each of them -----------------------------------------------------
# One level of 30-pixel windows (ONE_LEVEL), a model that rejects nothing, dense mode off (the predicted path runs): a
# frame of w x h pixels has ((w - 30) // 3 + 1) * ((h - 30) // 3 + 1) detections.

DISTINCT = ((3, 20, 5, 4), dict(seed=3))       # 60 carts of 8 leaves: no two windows of a test frame share a score (asserted)
COARSE = ((1, 2, 3, 3), dict(seed=2))          # 2 carts of 4 leaves: a handful of scores, tie groups of different sizes

LIMITS = [  # id, frame w x h, windows, frames, model, what k_post does under NMS
    ("1024_distinct", 123, 123, 1024, "noise", DISTINCT, "posted"),       # kPostMaxDets is taken
    ("1025_distinct", 150, 102, 1025, "noise", DISTINCT, "declined"),     # ... one more is not
    ("256_flat", 75, 75, 256, "flat", COARSE, "posted"),                  # kPostLiteralMax tied scores: exchange sort replayed on the device
    ("256_coarse", 75, 75, 256, "noise", COARSE, "posted"),               # ... several tie groups: the survivors depend on the permutation
    ("257_flat", 798, 30, 257, "flat", COARSE, "declined"),               # ties among one more
    ("272_coarse", 78, 75, 272, "noise", COARSE, "declined"),
    ("272_distinct", 78, 75, 272, "noise", DISTINCT, "posted"),           # rank path: no ties found, no literal sort
]


def _frames(kind, n, w, h, seed):
    from jda_amd import synth
    if kind == "flat":
        return np.stack([np.full((h, w), 40 + 9 * i, np.uint8) for i in range(n)])
    return synth.make_frames(n, w, h, seed=seed)


def _limit_case(casc, path, frames, windows, expect_nms, nms, oracle_frames=(0, -1)):
    """One batch at a limit: device form == host form on every frame, host form == oracle on some, counters as expected.
    Without NMS k_post needs no score order: ties do not make it decline, only the 1,024 detections do."""
    import torch
    from oracle.pyoracle import Oracle
    n = len(frames)
    dev = torch.from_numpy(frames).cuda()
    casc.set_option("dense", 0)
    host, st = _both(casc, dev, expect_nms if nms else ("declined" if windows > 1024 else "posted"), th=ALL, nms=nms, **ONE_LEVEL)
    assert st["patch_n"] == windows * n
    raw = casc.detect_batch_device(dev, th=ALL, nms=False, **ONE_LEVEL)          # (device_post is 0 here: the host form)
    assert all(len(r["scores"]) == windows for r in raw)
    assert _k_post_takes([r["scores"] for r in raw], nms) == (expect_nms if nms else ("declined" if windows > 1024 else "posted"))
    if not nms:
        for a, b in zip(raw, host):
            assert same(a["scores"], b["scores"])
    else:
        assert all(0 < len(hh["scores"]) < windows for hh in host)
    o = Oracle(path)
    for i in oracle_frames:
        want = o.detect(frames[i], th=ALL, nms=nms, **ONE_LEVEL)
        if not nms:
            # (the oracle's restatement relocates the landmarks of the post-NMS list only, like c/jda.c:303-313 does; the
            # library relocates what it returns either way: multiply, then add, in float -- c/jda.c:471-472)
            sz = want["bboxes"][:, 2].astype(np.float32)[:, None]
            sh = want["shapes"].copy()
            sh[:, 0::2] = sh[:, 0::2] * sz + want["bboxes"][:, 0].astype(np.float32)[:, None]
            sh[:, 1::2] = sh[:, 1::2] * sz + want["bboxes"][:, 1].astype(np.float32)[:, None]
            want = dict(want, shapes=sh)
        for k in ("bboxes", "scores", "shapes"):
            assert same(want[k], host[i][k]), (i, k)
    return host, raw


@pytest.mark.parametrize("nms", [True, False])
@pytest.mark.parametrize("case", LIMITS, ids=[c[0] for c in LIMITS])
def test_limits_of_k_post(built, gpu, model_file, case, nms):
    from jda_amd import api, synth
    _, w, h, windows, kind, (dims, mkw), expect = case
    assert synth.levels_c(w, h, **ONE_LEVEL)[1] == windows and len(synth.levels_c(w, h, **ONE_LEVEL)[0]) == 1
    p, _ = model_file(dims, 8, cart_th=synth.NEG_BIG, **mkw)
    frames = _frames(kind, 16, w, h, seed=31)
    c = api.Cascador(p)
    host, raw = _limit_case(c, p, frames, windows, expect, nms)
    groups = [np.unique(r["scores"], return_counts=True)[1] for r in raw]
    if dims == DISTINCT[0]:
        assert all(len(g) == windows for g in groups)                         # no tied scores in any frame
    elif kind == "flat":
        assert all(len(g) == 1 for g in groups)                               # one score per frame
    else:
        assert all(2 <= len(g) <= 16 and len(set(g.tolist())) >= 2 for g in groups)      # several tie groups of different sizes
    c.close()


@pytest.mark.parametrize("nms", [True, False])
@pytest.mark.parametrize("w,h,windows,expect", [(75, 75, 256, "posted"), (78, 75, 272, "declined")])
def test_nan_and_signed_zero_scores(built, gpu, tmp_path, w, h, windows, expect, nms):
    """Scores NaN, +0.0, -0.0 and tied ones in one frame.  A NaN score fails no `score < th`: such windows are detections;
    NaN is never `<` anything and -0.0 == +0.0, so the exchange sort's permutation is its own -- the device replays it
    literally up to 256 detections and declines above, and the NaN's payload and the zeros' signs come through.
    The model: cart 0 with leaf values +0.0, 1.0, NaN, 0.5 and a std of -1 (scores -0.0, -1.0, NaN, -0.5), cart 1 adds
    -0.0, +0.0, 0.5 or 0.5: -0.0 + -0.0 = -0.0, -0.0 + 0.0 = +0.0, -0.5 + 0.5 = +0.0."""
    from jda_amd import api, synth
    m = synth.make_model(1, 2, 3, 3, seed=2, cart_th=synth.NEG_BIG)
    m.leaf[0, 0] = [0.0, 1.0, np.nan, 0.5]; m.cstd[0, 0] = -1.0
    m.leaf[0, 1] = [-0.0, 0.0, 0.5, 0.5]
    p = m.save(str(tmp_path / "nan_zero.model"), 8)
    frames = synth.make_frames(16, w, h, seed=34)
    c = api.Cascador(p)
    host, raw = _limit_case(c, p, frames, windows, expect, nms, oracle_frames=(0, 2, -1))
    bits = np.concatenate([r["scores"].view(np.uint32) for r in raw])
    assert (bits == 0x80000000).any() and (bits == 0).any() and np.isnan(bits.view(np.float32)).any()
    assert all(np.isnan(r["scores"]).any() and len(np.unique(r["scores"])) < windows for r in raw)      # every frame: NaN and ties
    c.close()


@pytest.mark.parametrize("nms", [True, False])
def test_prediction_falls_short(built, gpu, model_file, nms):
    """Three calls without a detection leave a row reservation of 64 (pred_out * windows * 1.25 + 64); then every window
    is one.  k_post declines through cap_rows (or the pass regrows and runs again): the host form's results, and the
    next call, sized by this one, posts again."""
    import torch
    from jda_amd import api, synth
    p, _ = model_file(DISTINCT[0], 8, cart_th=synth.NEG_BIG, **DISTINCT[1])
    frames = synth.make_frames(16, 75, 75, seed=36)
    dev = torch.from_numpy(frames).cuda()
    c = api.Cascador(p)
    c.set_option("dense", 0); c.set_option("device_post", 1)
    print()
    for i in range(3):
        got, st = c.detect_batch_device(dev, th=3.0e38, nms=nms, stats=True, **ONE_LEVEL)
        _expect("none" if i == 0 else "posted", st, "no detection, call %d" % i)
        assert st["patch_n"] == 256 * 16 and all(len(g["scores"]) == 0 for g in got)
    short, st = c.detect_batch_device(dev, th=ALL, nms=nms, stats=True, **ONE_LEVEL)
    _expect("declined" if st["ws_regrows"] == 0 else "none", st, "every window, 64 rows reserved")
    assert st["post_passes"] == 0 and st["post_declined"] + st["ws_regrows"] >= 1
    again, st = c.detect_batch_device(dev, th=ALL, nms=nms, stats=True, **ONE_LEVEL)
    _expect("posted", st, "every window, sized by the last")
    c.set_option("device_post", 0)
    host, st0 = c.detect_batch_device(dev, th=ALL, nms=nms, stats=True, **ONE_LEVEL)
    _expect("none", st0, "device_post=0")
    assert sum(len(hh["scores"]) for hh in host) == 256 * 16 if not nms else all(0 < len(hh["scores"]) < 256 for hh in host)
    for got in (short, again):
        for i, (a, b) in enumerate(zip(host, got)):
            for k in ("bboxes", "scores", "shapes"):
                assert same(a[k], b[k]), (i, k)
    c.close()


def test_two_levels_posted(built, gpu, model_file):
    """Detections of several pyramid levels in one frame (160 x 120, windows of 46 to 110 pixels): k_post finds a
    detection's level from the levels' first window ids."""
    import torch
    from jda_amd import api, synth
    from oracle.pyoracle import Oracle
    p, _ = model_file((3, 20, 5, 4), 8, seed=3, cart_th=-1.0, norm_every=5)
    frames = synth.make_frames(32, 160, 120, seed=25)
    c = api.Cascador(p)
    c.set_option("dense", 0)
    host, st = _both(c, torch.from_numpy(frames).cuda(), "posted", th=-0.5)
    assert st["post_passes"] >= 1 and st["patch_n"] == 983 * 32
    sizes = set(np.concatenate([hh["bboxes"][:, 2] for hh in host]).tolist())
    assert len(sizes) > 1 and sizes <= {46, 57, 71, 88, 110}
    assert max(len(set(hh["bboxes"][:, 2].tolist())) for hh in host) > 1        # ... within one frame, too
    o = Oracle(p)
    for i in (0, 31):
        want = o.detect(frames[i], th=-0.5)
        for k in ("bboxes", "scores", "shapes"):
            assert same(want[k], host[i][k]), (i, k)
    c.close()


def test_ragged_job_at_the_limits(built, gpu, model_file):
    """One ragged job whose chunks are cut (a job from host memory starts with a quarter and a half chunk) so that the
    crowded and the tied images have a chunk of their own: [1 x 1,024 distinct + 4 x 256 tied] posted,
    [3 x 1,025 + 3 x 257 tied] declined, [4 x 1,024 + 8 x 256 tied] posted.  Per image the job is jdaDetect on that image."""
    from jda_amd import api, synth
    p, _ = model_file(DISTINCT[0], 8, cart_th=synth.NEG_BIG, **DISTINCT[1])
    A = list(synth.make_frames(5, 123, 123, seed=31))
    B = list(synth.make_frames(3, 150, 102, seed=32))
    C256 = [np.full((75, 75), 50 + 10 * i, np.uint8) for i in range(12)]
    D257 = [np.full((30, 798), 60 + 20 * i, np.uint8) for i in range(3)]
    imgs = A[:1] + C256[:4] + B + D257 + A[1:] + C256[4:]
    wins = [synth.levels_c(im.shape[1], im.shape[0], **ONE_LEVEL)[1] for im in imgs]
    assert len(imgs) == 23 and sum(wins[:5]) == 2048 and sum(wins[5:11]) == 3846 and sum(wins[11:]) == 6144
    c = api.Cascador(p)
    c.set_option("dense", 0)
    c.set_option("ragged_chunk_windows", 8192); c.set_option("ragged_chunk_min_windows", 8192)
    c.set_option("device_post_min_frames", 4)
    print()
    c.set_option("device_post", 1)
    outs = []
    for rep in range(3):
        got, st = c.detect_ragged(imgs, th=ALL, stats=True, **ONE_LEVEL)
        _expect("none" if rep == 0 else "both", st, "job %d" % rep)       # (the first job's three chunks are all issued before one is collected)
        assert st["patch_n"] == sum(wins)
        outs.append(got)
    c.set_option("device_post", 0)
    host, st0 = c.detect_ragged(imgs, th=ALL, stats=True, **ONE_LEVEL)
    _expect("none", st0, "device_post=0")
    for got in outs:
        assert len(got) == len(host) == 23
        for i, (a, b) in enumerate(zip(host, got)):
            for k in ("bboxes", "scores", "shapes"):
                assert same(a[k], b[k]), (i, k, len(a["scores"]), len(b["scores"]))
    for i in (0, 1, 5, 8, 11, 22):
        one = c.detect(imgs[i], scale=1.25, min_size=30, max_size=30, th=ALL)
        assert 0 < len(one["scores"]) < wins[i]
        for k in ("bboxes", "scores", "shapes"):
            assert same(one[k], host[i][k]), (i, k)
    c.close()
