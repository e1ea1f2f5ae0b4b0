"""The five kernels of k_mine.hip and the host loops of mine.cpp at their limits (the table of
constants): every comparison is exact, against the restatements of tests/mining_ref.py on jobs of a few hundred windows and,
for the large jobs, between calls of the library one side of which is tied to the restatement, plus a restated sample.  Every
case that claims a limit reads it from the launch report (Cascador.mine_launches, jdaMineLaunches); the jobs are defined and
proved in tests/test_mine_limits_host.py."""
import ctypes as C

import numpy as np
import pytest

from conftest import same
import mining_ref
import test_mine_limits_host as J

pytestmark = pytest.mark.gpu

@pytest.fixture(scope="module")
def gpu():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    return torch.device("cuda", 0)


def _open(tmp, **kw):
    from jda_amd import api
    from oracle import cpp_reading2 as r2
    from oracle.pyoracle import Oracle
    p = J.model(tmp, **kw)
    c = api.Cascador(p)
    c.set_similarity_transform(bool(kw.get("sim")))
    return c, Oracle(p), r2.Model2(p)


def _ran(c, f):
    """f() and what the cascador's report says it launched: differences of the sums, the two maxima as they stand after."""
    a = c.mine_launches()
    r = f()
    b = c.mine_launches()
    return r, {k: b[k] if k in ("walk_batch_max", "walk_cap") else b[k] - a[k] for k in b}


def _mine(c, job, size, start=0, geom=(48, 36, 24), device=False, **kw):
    return c.mine_negatives_cpp(J.images(job["sizes"], job["seed"]), job["steps"], job["factors"], job["tfs"], size, start=start,
                                device=device, origin_size=geom[0], half_size=geom[1], quarter_size=geom[2], **kw)


def _flat(hits):
    return np.concatenate([q.ravel() for h in hits for q in h["patches"]]) if hits else np.zeros(0, np.uint8)


def _check(got, want, dim, start):
    hits = want["hits"]
    assert np.array_equal(got["hits"], np.array([h["row"] for h in hits], np.int32).reshape(-1, 4))
    assert same(got["score"], np.array([h["score"] for h in hits], np.float64).reshape(-1))
    assert same(got["shape"], np.array([h["shape"] for h in hits], np.float64).reshape(-1, dim))
    assert np.array_equal(got["patches"].ravel(), _flat(hits))             # every byte and every record boundary
    st = got["stats"]
    assert (st["hits"], st["nega_n"], st["carts_n"], st["next_start"]) == (len(hits), want["nega_n"], want["carts_n"], want["next_start"])
    assert st["windows"] == want["next_start"] - start


def _same_result(a, b, keys=("hits", "score", "shape", "patches")):
    for k in keys:
        assert same(a[k], b[k]), k
    assert {**a["stats"], "call_ms": 0} == {**b["stats"], "call_ms": 0}


def _validate_want(m2, resize, imgs, crops, mode, geom, shift, seed, sim=False):
    res = []
    for key, (i, x, y, w, h) in enumerate(crops):
        p = mining_ref.chain(resize, imgs[i][y:y + h, x:x + w], mode, *geom)
        dx, dy = mining_ref.shift_of(seed, key, shift)
        res.append(mining_ref.validate(m2, p, dx, dy, sim))
    return dict(is_face=np.array([r[0] for r in res], np.uint8), score=np.array([r[1] for r in res], np.float64),
                carts_n=np.array([r[3] for r in res], np.int32), shape=np.array([r[2] for r in res], np.float64))


def _check_validate(got, want, n=None):
    for k in ("is_face", "carts_n", "score", "shape"):
        assert same(got[k], want[k][:n]), k


# ---- lane and block tails ------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def tails(built, gpu, tmp_path_factory):
    c, o, m2 = _open(tmp_path_factory.mktemp("tails"))
    imgs = J.images([(40, 36), (33, 47)], 71)
    rng = np.random.default_rng(72)
    crops = []
    for k in range(257):                                                    # small crops of two images: the restatement stays cheap
        i = k & 1
        H, W = imgs[i].shape
        w, h = int(rng.integers(4, 20)), int(rng.integers(4, 20))
        crops.append((i, int(rng.integers(0, W - w + 1)), int(rng.integers(0, H - h + 1)), w, h))
    crops = np.array(crops, np.int32)
    want = {mode: _validate_want(m2, o.resize_cv, imgs, crops, mode, (48, 36, 24), 0.05, 5) for mode in (0, 1)}
    per = J.restate(m2, o.resize_cv, J.TAIL_JOB, 48, 36, 24, shift=0.04, seed=9)
    yield dict(c=c, imgs=imgs, crops=crops, want=want, per=per)
    c.close(); o.close()


@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257])
def test_validate_crop_count_tails(tails, n):
    c = tails["c"]
    for mode in (0, 1):
        got, ran = _ran(c, lambda: c.validate_cpp(tails["imgs"], tails["crops"][:n], mode=mode, shift_size=0.05, seed=5))
        _check_validate(got, tails["want"][mode], n)
        assert (ran["k_patches"], ran["k_walk"], ran["walk_batches"], ran["walk_cap"]) == (1, 1, 1, n) and ran["walk_batch_max"] >= n
        assert ran["k_scan"] == ran["k_items"] == ran["k_sum"] == ran["chunks"] == 0
    assert 0 < tails["want"][0]["is_face"].sum() < 257


@pytest.mark.parametrize("chunk", [1, 64, 65, 255, 256, 257])
def test_mine_chunk_length_tails(tails, chunk):
    c, per = tails["c"], tails["per"]
    total = len(per)
    c.set_option("mine_chunk_windows", chunk)
    try:
        got, ran = _ran(c, lambda: _mine(c, J.TAIL_JOB, total + 1, shift_size=0.04, seed=9))
    finally:
        c.set_option("mine_chunk_windows", 4194304)
    _check(got, J.expect(per, 0, total + 1), c.dim, 0)
    floored = max(64, chunk)                                                # the option's floor: 1 mines in chunks of 64
    assert ran["chunks"] == ran["k_scan"] == ran["k_sum"] == -(-total // floored)
    assert ran["scan_rejects"] + ran["walk_rejects"] == got["stats"]["nega_n"] and ran["sum_saturated"] == 0
    assert ran["walk_batches"] == ran["k_items"] == ran["k_walk"] == ran["k_patches"] <= ran["chunks"]


# ---- segments --------------------------------------------------------------------------------------------------------------

def test_segment_edges_starts_chunks_and_cuts(built, gpu, tmp_path):
    firsts = [t[0] for t in J.SEG_TABLE]
    lasts = [t[0] + t[3] * t[4] - 1 for t in J.SEG_TABLE]
    c, o, m2 = _open(tmp_path)
    per = J.restate(m2, o.resize_cv, J.SEG_JOB, 48, 36, 24)
    assert len(per) == J.SEG_TOTAL and 0 < sum(r["face"] for r in per) < J.SEG_TOTAL
    c.set_option("mine_chunk_windows", 64)
    # start on every segment's first and last ordinal; chunk edges on them: a chunk that begins on f starts 64 below it, one
    # that ends on l starts 63 below it
    starts = sorted(set(firsts + lasts + [f - 64 for f in firsts[1:]] + [l - 63 for l in lasts[1:]] + [J.SEG_TOTAL - 1, J.SEG_TOTAL]))
    assert starts[0] == 0
    for start in starts:
        for device in (False, True):
            got, ran = _ran(c, lambda: _mine(c, J.SEG_JOB, J.SEG_TOTAL, start=start, device=device))
            _check(got, J.expect(per, start, J.SEG_TOTAL), c.dim, start)
            assert ran["chunks"] == -(-(J.SEG_TOTAL - start) // 64), start
    # chaining through next_start, three hits a call, reproduces the one-call result
    one = _mine(c, J.SEG_JOB, J.SEG_TOTAL)
    parts, start, nega, carts = [], 0, 0, 0
    while start < J.SEG_TOTAL:
        r = _mine(c, J.SEG_JOB, 3, start=start)
        _check(r, J.expect(per, start, 3), c.dim, start)
        parts.append(r); nega += r["stats"]["nega_n"]; carts += r["stats"]["carts_n"]
        start = r["stats"]["next_start"]
    for k in ("hits", "score", "shape", "patches"):
        assert same(np.concatenate([r[k] for r in parts]), one[k]), k
    assert (nega, carts) == (one["stats"]["nega_n"], one["stats"]["carts_n"])
    c.close(); o.close()
    # every window a hit: the size-th hit is the last window of a segment, and the first of the next
    from jda_amd import synth
    c, o, m2 = _open(tmp_path, cart_th=synth.NEG_BIG)
    per = J.restate(m2, o.resize_cv, J.SEG_JOB, 48, 36, 24)
    assert all(r["face"] for r in per)
    for chunk in (64, 4194304):
        c.set_option("mine_chunk_windows", chunk)
        for edge in lasts:
            for size in (edge + 1, edge + 2):
                got = _mine(c, J.SEG_JOB, size)
                _check(got, J.expect(per, 0, size), c.dim, 0)
                assert got["stats"]["next_start"] == min(size, J.SEG_TOTAL) and tuple(got["hits"][-1]) == per[min(size, J.SEG_TOTAL) - 1]["row"]
    one_seg = dict(J.SEG_JOB, sizes=J.SEG_JOB["sizes"][:1], steps=[3], factors=[1.7], tfs=[0])      # an enumeration with one segment
    for start, size in ((0, 121), (120, 5), (0, 1), (57, 64)):
        _check(_mine(c, one_seg, size, start=start), J.expect(per[:121], start, size), c.dim, start)
    c.close(); o.close()


# ---- patch geometry --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("geom", J.GEOMS, ids=lambda g: "%d_%d_%d" % g)
def test_geometry_mining_and_validate(built, gpu, tmp_path, geom):
    from jda_amd import synth
    os_, hs, qs = geom
    job = J.geom_job(os_)
    pt = os_ * os_ + hs * hs + qs * qs
    tb = [mining_ref.transform(im, t) for im, t in zip(J.images(job["sizes"], job["seed"]), job["tfs"])]
    for th in (synth.NEG_BIG, J.REJECT_TH):
        c, o, m2 = _open(tmp_path, cart_th=th)
        per = J.restate(m2, o.resize_cv, job, os_, hs, qs, shift=0.03, seed=13)
        total = len(per)
        for device in (False, True):
            for size in (total, 2):
                got = _mine(c, job, size, geom=geom, device=device, shift_size=0.03, seed=13)
                want = J.expect(per, 0, size)
                _check(got, want, c.dim, 0)
                flat = got["patches"].ravel()
                for h in range(len(want["hits"]) - 1):                      # tight output against the 16-byte record stride
                    assert flat[(h + 1) * pt - 1] == want["hits"][h]["patches"][2][-1, -1]
                    assert flat[(h + 1) * pt] == want["hits"][h + 1]["patches"][0][0, 0]
        if th == synth.NEG_BIG:
            assert len(got["hits"]) == 2 and _mine(c, job, total, geom=geom)["stats"]["hits"] == total
        # Validate, both chains, on the windows as caller crops and on four that are not square
        crops = [(r["row"][0], r["row"][1], r["row"][2], r["row"][3], r["row"][3]) for r in per]
        for i, im in enumerate(tb):
            H, W = im.shape
            crops += [(i, 0, 0, W, H), (i, W - 1, H - 1, 1, 1), (i, 1, 0, W - 1, 2), (i, 0, 1, 3, H - 1)]
        crops = np.array(crops, np.int32)
        for mode in (0, 1):
            want = _validate_want(m2, o.resize_cv, tb, crops, mode, geom, 0.03, 13)
            for imgs in (tb, None):
                from jda_amd import api
                src = tb if imgs is not None else api._pack_images_device(tb)
                got = c.validate_cpp(src, crops, mode=mode, origin_size=os_, half_size=hs, quarter_size=qs, shift_size=0.03, seed=13)
                _check_validate(got, want)
        c.close(); o.close()


def test_sides_of_129_and_0_are_refused_outputs_untouched(built, gpu, tmp_path):
    from jda_amd import api
    c, o, _ = _open(tmp_path)
    o.close()
    imgs = J.images([(140, 140)], 81)
    dev, base, offs, ws, hs, n_img, keep = api._image_set(imgs)
    ip, dp, up = C.POINTER(C.c_int), C.POINTER(C.c_double), C.POINTER(C.c_ubyte)
    ks, steps = api._ivec([3])
    kf, factors = api._ivec([2.0], C.c_double, np.float64)
    kt, tfs = api._ivec([0])
    crops = np.array([(0, 0, 0, 50, 50), (0, 3, 4, 20, 30)], np.int32)
    for bad in [(129, 36, 24), (48, 129, 24), (48, 36, 129), (0, 36, 24), (48, 0, 24), (48, 36, 0), (-1, 36, 24)]:
        hits = np.full((4, 4), -77, np.int32)
        score = np.full(4, 7.25)
        shape = np.full((4, c.dim), 7.25)
        pat = np.full(4 * 3 * 129 * 129, 0xA5, np.uint8)
        st = api.jdaMineStats()
        rc = api.lib.jdaMineNegativesCpp(c.h, base, ws, hs, n_img, steps, factors, tfs, bad[0], bad[1], bad[2], 0, 4, 0.0, 0,
                                         hits.ctypes.data_as(ip), score.ctypes.data_as(dp), shape.ctypes.data_as(dp),
                                         pat.ctypes.data_as(up), C.byref(st))
        assert rc == -1 and "[1, 128]" in api.last_error(), bad
        assert (hits == -77).all() and (score == 7.25).all() and (shape == 7.25).all() and (pat == 0xA5).all(), bad
        assert st.hits == 0 and st.windows == 0 and st.nega_n == 0
        face = np.full(2, 0xA5, np.uint8)
        carts = np.full(2, -77, np.int32)
        for mode in (0, 1):
            rc = api.lib.jdaValidateCpp(c.h, base, ws, hs, n_img, crops.ctypes.data_as(ip), 2, bad[0], bad[1], bad[2], mode, 0.0, 0,
                                        face.ctypes.data_as(up), score.ctypes.data_as(dp), carts.ctypes.data_as(ip),
                                        shape.ctypes.data_as(dp), None)
            assert rc == -1 and "[1, 128]" in api.last_error(), bad
            assert (face == 0xA5).all() and (carts == -77).all() and (score == 7.25).all() and (shape == 7.25).all(), bad
    assert c.mine_launches() == dict.fromkeys(api.MINE_LAUNCH_FIELDS, 0)   # nothing was launched
    del keep, ks, kf, kt
    c.close()


# ---- more than one walk batch ------------------------------------------------------------------------------------------------

GEOM_B = (128, 96, 64)


def _ordinal_b(row):
    return (int(row[2]) // 2) * 60 + int(row[1]) // 2                       # BATCH_JOB: one level of 60 x 60 windows, step 2


@pytest.mark.parametrize("sim", [False, True], ids=["every_window_a_hit", "similarity_reject_mix"])
def test_more_than_one_walk_batch_in_a_chunk(built, gpu, tmp_path, sim):
    """sim off: no cart rejects (NEG_BIG), every window survives the scan and is a hit, so `size` can land exactly on a batch's
    last entry and on the next one's first.  sim on: the scan hands every window to the walk (carts0 = 0) with the reject-mix
    model, so the walk's nega_n / carts_n add up across batches."""
    from jda_amd import synth
    c, o, m2 = _open(tmp_path, cart_th=J.REJECT_TH if sim else synth.NEG_BIG, sim=sim)
    c.set_option("workspace_mb", 64)                                        # the smallest workspace: the smallest batches
    one, ran = _ran(c, lambda: _mine(c, J.BATCH_JOB, J.BATCH_TOTAL, geom=GEOM_B, device=True, shift_size=0.02, seed=3))
    cap = ran["walk_cap"]
    assert ran["chunks"] == 1 and ran["walk_batches"] >= 3 and ran["walk_batch_max"] == cap < J.BATCH_TOTAL / 2
    assert ran["k_items"] == ran["k_patches"] == ran["k_walk"] == ran["walk_batches"] == -(-J.BATCH_TOTAL // cap)
    assert ran["scan_rejects"] == 0 and ran["walk_rejects"] == one["stats"]["nega_n"] == J.BATCH_TOTAL - len(one["hits"])
    ords = [_ordinal_b(r) for r in one["hits"]]
    assert ords == sorted(ords) and one["stats"]["next_start"] == J.BATCH_TOTAL
    if sim:
        assert 0 < len(ords) < J.BATCH_TOTAL and one["stats"]["carts_n"] > one["stats"]["nega_n"] > 0
    else:
        assert ords == list(range(J.BATCH_TOTAL))
    # the same job, every chunk one batch
    small_chunk = 512
    assert small_chunk < cap
    c.set_option("mine_chunk_windows", small_chunk)
    small, ran = _ran(c, lambda: _mine(c, J.BATCH_JOB, J.BATCH_TOTAL, geom=GEOM_B, device=True, shift_size=0.02, seed=3))
    assert ran["chunks"] == ran["walk_batches"] == -(-J.BATCH_TOTAL // small_chunk) and c.mine_launches()["walk_batch_max"] == cap
    _same_result(one, small)
    # every 97th hit, restated
    pick = list(range(0, len(ords), 97))
    per = J.restate(m2, o.resize_cv, J.BATCH_JOB, *GEOM_B, shift=0.02, seed=3, sim=sim, only={ords[i] for i in pick})
    for i in pick:
        r = per[ords[i]]
        assert r["face"] and tuple(one["hits"][i]) == r["row"]
        assert same(one["score"][i], np.float64(r["score"])) and same(one["shape"][i], np.array(r["shape"], np.float64))
        assert np.array_equal(one["patches"][i], _flat([r]))
    # `size` on the last entry of a batch and on the first of the next (sim: on the hits next to those entries)
    for b in (1, 2):
        first_next = next(i for i, v in enumerate(ords) if v >= b * cap)    # the first hit of batch b
        for h in (first_next - 1, first_next):
            if not sim:
                assert ords[h] == b * cap - 1 + (h - first_next + 1)
            c.set_option("mine_chunk_windows", 4194304)
            got, ran = _ran(c, lambda: _mine(c, J.BATCH_JOB, h + 1, geom=GEOM_B, device=True, shift_size=0.02, seed=3))
            assert ran["chunks"] == 1 and ran["walk_batches"] == ords[h] // cap + 1
            assert got["stats"]["next_start"] == ords[h] + 1 and got["stats"]["hits"] == h + 1
            for k in ("hits", "score", "shape", "patches"):
                assert same(got[k], one[k][:h + 1]), k
            c.set_option("mine_chunk_windows", small_chunk)
            _same_result(got, _mine(c, J.BATCH_JOB, h + 1, geom=GEOM_B, device=True, shift_size=0.02, seed=3))
    c.close(); o.close()


def test_validate_more_crops_than_a_batch(built, gpu, tmp_path):
    c, o, m2 = _open(tmp_path)
    c.set_option("workspace_mb", 64)
    imgs = J.images([(150, 150), (97, 131)], 91)
    _, ran = _ran(c, lambda: _mine(c, dict(J.BATCH_JOB, sizes=[(131, 131)]), 1, geom=GEOM_B))
    cap = ran["walk_cap"]                                                   # what a batch holds at this geometry
    assert 64 < cap < 65536
    n = 2 * cap + 77
    rng = np.random.default_rng(92)
    crops = []
    for k in range(n):
        i = k % 2
        H, W = imgs[i].shape
        w, h = int(rng.integers(3, 40)), int(rng.integers(3, 40))
        crops.append((i, int(rng.integers(0, W - w + 1)), int(rng.integers(0, H - h + 1)), w, h))
    crops = np.array(crops, np.int32)
    kw = dict(origin_size=128, half_size=96, quarter_size=64)
    for mode in (0, 1):
        got, ran = _ran(c, lambda: c.validate_cpp(imgs, crops, mode=mode, **kw))
        assert ran["walk_batches"] == ran["k_walk"] == ran["k_patches"] == 3 and ran["walk_cap"] == ran["walk_batch_max"] == cap
        # the same crops a few hundred a call (shift 0: a crop's draw is keyed on its index in the call)
        parts = [c.validate_cpp(imgs, crops[at:at + 300], mode=mode, **kw) for at in range(0, n, 300)]
        for k in got:
            assert same(got[k], np.concatenate([p[k] for p in parts])), k
        pick = sorted(set(range(0, n, 97)) | {cap - 1, cap, 2 * cap - 1, 2 * cap, n - 1})
        want = _validate_want(m2, o.resize_cv, imgs, crops[pick], mode, GEOM_B, 0.0, 0)
        _check_validate({k: got[k][pick] for k in got}, want)
        assert 0 < got["is_face"].sum() < n
    c.close(); o.close()


# ---- k_mine_sum past its grid ---------------------------------------------------------------------------------------------

def test_sum_past_its_grid(built, gpu, tmp_path):
    from jda_amd import api
    W = J.big_width(lambda w, h: api.mine_windows(w, h, 48, J.BIG_STEP, J.BIG_FACTOR)[0])
    total = api.mine_windows(W, J.BIG_H, 48, J.BIG_STEP, J.BIG_FACTOR)[0]
    job = dict(sizes=[(W, J.BIG_H)], steps=[J.BIG_STEP], factors=[J.BIG_FACTOR], tfs=[0], seed=101)
    dev = api._pack_images_device(J.images(job["sizes"], job["seed"]))      # one resident image
    mine = lambda c, size: c.mine_negatives_cpp(dev, job["steps"], job["factors"], job["tfs"], size, patches=False)
    c, o, m2 = _open(tmp_path)
    room = total
    one, ran = _ran(c, lambda: mine(c, room))
    st = one["stats"]
    assert (ran["chunks"], ran["k_sum"], ran["sum_saturated"]) == (1, 1, 1)
    assert st["windows"] == st["total_windows"] == st["next_start"] == total and 0 < st["hits"] < room
    assert st["hits"] + st["nega_n"] == total and ran["scan_rejects"] + ran["walk_rejects"] == st["nega_n"] and ran["walk_rejects"] > 0
    c.set_option("mine_chunk_windows", 100000)
    parts, ran = _ran(c, lambda: mine(c, room))
    assert (ran["chunks"], ran["k_sum"], ran["sum_saturated"]) == (-(-total // 100000), -(-total // 100000), 0)
    _same_result(one, parts, keys=("hits", "score", "shape"))
    # a restated sample of the windows: hits keep their bits, rejects are no hits
    first, lv = {}, 0
    for win, nx, ny in mining_ref.levels(W, J.BIG_H, 48, J.BIG_STEP, J.BIG_FACTOR):
        first[win] = (lv, nx)
        lv += nx * ny
    ords = [first[int(r[3])][0] + (int(r[2]) // J.BIG_STEP) * first[int(r[3])][1] + int(r[1]) // J.BIG_STEP for r in one["hits"]]
    assert ords == sorted(ords)
    pick = set(range(0, total, 4099)) | {0, J.SUM_LANES - 1, J.SUM_LANES, total - 1} | set(ords[::97])
    per = J.restate(m2, o.resize_cv, job, 48, 36, 24, only=pick)
    at = {v: i for i, v in enumerate(ords)}
    for v in sorted(pick):
        assert per[v]["face"] == (v in at), v
        if v in at:
            i = at[v]
            assert tuple(one["hits"][i]) == per[v]["row"] and same(one["score"][i], np.float64(per[v]["score"]))
            assert same(one["shape"][i], np.array(per[v]["shape"], np.float64))
    # a size that cuts the chunk above the grid's lanes, and one that cuts it below: each equals the chained form
    above = next(i for i, v in enumerate(ords) if v >= J.SUM_LANES)       # its cut lies above the lanes: ordinal + 1 windows
    below = next(i for i, v in enumerate(ords) if v >= J.SUM_LANES // 2)
    assert ords[below] < J.SUM_LANES - 1
    for h, sat in ((above, 1), (below, 0)):
        c.set_option("mine_chunk_windows", 4194304)
        got, ran = _ran(c, lambda: mine(c, h + 1))
        assert (ran["chunks"], ran["k_sum"], ran["sum_saturated"]) == (1, 1, sat)
        assert got["stats"]["next_start"] == ords[h] + 1 and same(got["hits"], one["hits"][:h + 1])
        c.set_option("mine_chunk_windows", 100000)
        _same_result(got, mine(c, h + 1), keys=("hits", "score", "shape"))
    c.close(); o.close()
    # nothing passes its first cart: the counters in closed form
    c, o, _ = _open(tmp_path, cart_th=1e30)
    o.close()
    got, ran = _ran(c, lambda: mine(c, 10))
    st = got["stats"]
    assert st["hits"] == 0 and st["nega_n"] == st["carts_n"] == st["windows"] == total
    assert (ran["sum_saturated"], ran["scan_rejects"], ran["walk_rejects"], ran["walk_batches"]) == (1, total, 0, 0)
    c.close()


# ---- the split between scan and walk ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("hdr", [None, (0, 11)], ids=["full", "stage_0_in_training"])
def test_handoff_moves_rejects_between_scan_and_walk_only(built, gpu, tmp_path, hdr):
    c, o, m2 = _open(tmp_path, hdr=hdr)
    per = J.restate(m2, o.resize_cv, J.TAIL_JOB, 48, 36, 24, shift=0.04, seed=9)
    total = len(per)
    want = J.expect(per, 0, total)
    stage0 = J.K if hdr is None else hdr[1] + 1                             # Validate's carts of stage 0: K, or the snapshot's part
    shares = []
    for handoff in (1, 2, J.K - 1, J.K, J.K + 5):
        c.set_option("handoff", handoff)
        got, ran = _ran(c, lambda: _mine(c, J.TAIL_JOB, total, shift_size=0.04, seed=9))
        _check(got, want, c.dim, 0)
        by_scan = sum(1 for r in per if not r["face"] and r["n"] <= min(stage0, handoff))
        assert (ran["scan_rejects"], ran["walk_rejects"]) == (by_scan, want["nega_n"] - by_scan), handoff
        shares.append(by_scan)
    assert shares == sorted(shares) and shares[0] < shares[-1]
    assert shares[-1] == shares[-2] and (shares[-1] < want["nega_n"]) == (hdr is None)     # a snapshot of stage 0: the scan rejects them all
    c.set_option("handoff", 128)
    c.set_similarity_transform(True)                                        # carts0 = 0: the walk rejects them all
    got, ran = _ran(c, lambda: _mine(c, J.TAIL_JOB, total, shift_size=0.04, seed=9))
    assert ran["scan_rejects"] == 0 and ran["walk_rejects"] == got["stats"]["nega_n"] > 0
    c.close(); o.close()
