"""Validate on caller crops and hard-negative mining (jdaValidateCpp*, jdaMineNegativesCpp*) against this repo's own
restatements: oracle.pyoracle.Oracle.resize_cv (cv::resize) and Validate as oracle/cpp_reading2.py reads it, with the
initial-shape shift added (tests/mining_ref.py).  Dialect CPP is parity-unpinned: bit-exact against these, not against
the reference."""
import numpy as np
import pytest

from conftest import same
import mining_ref

pytestmark = pytest.mark.gpu

OS, HS, QS = 48, 36, 24
DIMS = (3, 20, 5, 4)
HDRS = [None, (1, 6), (0, 11), (2, -1), (0, -1), (2, 19)]


@pytest.fixture(scope="module")
def gpu():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    return torch.device("cuda", 0)


def _model(tmp_path, multi=False, hdr=None, sim=False, cart_th=-1.0, seed=3):
    from jda_amd import synth
    mdl = synth.make_model(*DIMS, seed=seed, cart_th=cart_th, norm_every=5, multi_scale=multi, w_sigma=2e-2 if sim else 2e-3)
    p = str(tmp_path / ("m_%d_%s_%d.model" % (multi, "full" if hdr is None else "%d_%d" % hdr, seed)))
    if hdr is None:
        mdl.save(p, 8)
    else:
        mdl.save(p, 8, header_stage=hdr[0], header_cart=hdr[1])
    return p


def _images(sizes, seed=0):
    from jda_amd import synth
    return [synth.make_frames(1, w, h, seed=seed, first=i)[0] for i, (w, h) in enumerate(sizes)]


def _crops(imgs, rng, n=14):
    out = []
    for i, im in enumerate(imgs):
        H, W = im.shape
        for (w, h) in [(OS, OS), (2 * OS, 2 * OS), (37, 61), (70, 53)][: n]:
            if w > W or h > H:
                continue
            for (x, y) in [(0, 0), (W - w, H - h), (int(rng.integers(0, W - w + 1)), int(rng.integers(0, H - h + 1)))]:
                out.append((i, x, y, w, h))
    return np.array(out, np.int32)


def _oracle_validate(m2, o, imgs, crops, mode, shift, seed, sim):
    res = []
    for key, (i, x, y, w, h) in enumerate(crops):
        p = mining_ref.chain(o.resize_cv, imgs[i][y:y + h, x:x + w], mode, OS, HS, QS)
        dx, dy = mining_ref.shift_of(seed, key, shift)
        res.append(mining_ref.validate(m2, p, dx, dy, sim))
    return (np.array([r[0] for r in res], np.uint8), np.array([r[1] for r in res]), np.array([r[3] for r in res], np.int32),
            np.array([r[2] for r in res]))


def _check_validate(got, want):
    assert np.array_equal(got["is_face"], want[0])
    assert np.array_equal(got["carts_n"], want[2])
    assert same(got["score"], want[1])
    assert same(got["shape"], want[3])


@pytest.mark.parametrize("sim", [False, True])
@pytest.mark.parametrize("hdr", HDRS)
@pytest.mark.parametrize("multi", [False, True])
def test_validate_cpp_equals_the_oracle(built, gpu, tmp_path, multi, hdr, sim):
    from jda_amd import api
    from oracle import cpp_reading2 as r2
    from oracle.pyoracle import Oracle
    p = _model(tmp_path, multi, hdr, sim)
    c, o, m2 = api.Cascador(p), Oracle(p), r2.Model2(p)
    c.set_similarity_transform(sim)
    imgs = _images([(131, 97), (64, 48), (200, 150)], seed=5)
    crops = _crops(imgs, np.random.default_rng(1))
    for mode in (0, 1):
        for shift, seed in ((0.0, 0), (0.06, 77)):
            got = c.validate_cpp(imgs, crops, mode=mode, shift_size=shift, seed=seed)
            _check_validate(got, _oracle_validate(m2, o, imgs, crops, mode, shift, seed, sim))
            if shift:
                again = c.validate_cpp(imgs, crops, mode=mode, shift_size=shift, seed=seed)
                for k in got:
                    assert same(got[k], again[k]), k
    if hdr is not None:
        ran = hdr[0] * DIMS[1] + hdr[1] + 1
        got = c.validate_cpp(imgs, crops)
        assert (got["carts_n"][got["is_face"] == 1] == ran).all()    # Validate's n, not the padded T x K
    c.close(); o.close()


def test_validate_shift_restatement_equals_cpp_reading2_at_zero(built, tmp_path):
    from oracle import cpp_reading2 as r2
    from oracle.pyoracle import Oracle
    for hdr in (None, (1, 6)):
        for sim in (False, True):
            p = _model(tmp_path, True, hdr, sim)
            o, m2 = Oracle(p), r2.Model2(p)
            im = _images([(131, 97)], seed=2)[0]
            for (x, y, w) in [(0, 0, 48), (40, 20, 77), (83, 49, 48)]:
                pt = mining_ref.chain(o.resize_cv, im[y:y + w, x:x + w], 0, OS, HS, QS)
                a = mining_ref.validate(m2, pt, 0.0, 0.0, sim)
                b = r2.validate(m2, None, patches=tuple((q, 0, 0, q.shape[1], q.shape[0]) for q in pt), similarity=sim)
                assert a[0] == b[0] and a[3] == b[3] and same(np.float64(a[1]), np.float64(b[1])) and same(np.array(a[2]), np.array(b[2]))
            o.close()


def _device_set(imgs):
    import torch
    offs, tot = [], 0
    for a in imgs:
        offs.append(tot)
        tot += (a.size + 255) // 256 * 256
    host = np.zeros(max(tot, 256), np.uint8)
    for a, off in zip(imgs, offs):
        host[off:off + a.size] = a.ravel()
    return torch.from_numpy(host).cuda(), offs, [a.shape[1] for a in imgs], [a.shape[0] for a in imgs]


def test_validate_host_and_device_entries_agree(built, gpu, tmp_path):
    from jda_amd import api
    c = api.Cascador(_model(tmp_path, True, None, False))
    imgs = _images([(131, 97), (64, 48), (200, 150)], seed=6)
    crops = _crops(imgs, np.random.default_rng(2))
    for mode in (0, 1):
        a = c.validate_cpp(imgs, crops, mode=mode, shift_size=0.05, seed=9)
        b = c.validate_cpp(_device_set(imgs), crops, mode=mode, shift_size=0.05, seed=9)
        for k in a:
            assert same(a[k], b[k]), k
    with pytest.raises(api.JdaError):
        c.validate_cpp(imgs, [(1, 20, 0, 48, 48)])                      # leaves its 64 x 48 image
    c.close()


@pytest.mark.parametrize("multi", [False, True])
def test_validate_mode1_equals_pyramid_first_level(built, gpu, tmp_path, multi):
    """detectSingleScale's chain at the windows of method 0's first level (nms off) gives exactly its faces."""
    from jda_amd import api
    c = api.Cascador(_model(tmp_path, multi, None, False, cart_th=-0.6))
    im = _images([(150, 120)], seed=8)[0]
    step = 6
    got = c.detect_batch_cpp_pyramid(im[None], origin_size=OS, step=step, factor=1.2, nms=False, half_size=HS, quarter_size=QS)[0]
    lv0 = got["rects"][:, 2] == OS
    crops = np.array([(0, x, y, OS, OS) for y in range(0, 120 - OS + 1, step) for x in range(0, 150 - OS + 1, step)], np.int32)
    v = c.validate_cpp([im], crops, mode=1)
    f = v["is_face"] == 1
    assert f.sum() == lv0.sum() > 0
    assert np.array_equal(got["rects"][lv0], np.c_[crops[f][:, 1:3], crops[f][:, 3:5]])
    assert same(got["scores"][lv0], v["score"][f])
    sh = v["shape"][f].copy()
    sh[:, 0::2] = crops[f][:, 1:2].astype(np.float64) + sh[:, 0::2] * float(OS)
    sh[:, 1::2] = crops[f][:, 2:3].astype(np.float64) + sh[:, 1::2] * float(OS)
    assert same(got["shapes"][lv0], sh)
    c.close()


def _bgs(n, seed, sizes=((97, 71), (64, 80), (120, 90), (71, 71), (50, 49))):
    return _images([sizes[i % len(sizes)] for i in range(n)], seed=seed)


def _check_mine(got, want, dim):
    assert np.array_equal(got["hits"], np.array(want["hits"], np.int32).reshape(-1, 4))
    assert same(got["score"], np.array(want["score"], np.float64).reshape(-1))
    assert same(got["shape"], np.array(want["shape"], np.float64).reshape(-1, dim))
    for j, k in enumerate("ohq"):
        assert np.array_equal(got[k], np.array([p[j] for p in want["patches"]], np.uint8).reshape(got[k].shape)), k
    st = got["stats"]
    assert (st["nega_n"], st["carts_n"], st["next_start"]) == (want["nega_n"], want["carts_n"], want["next_start"])


@pytest.mark.parametrize("sim,shift", [(False, 0.0), (False, 0.05), (True, 0.0)])
@pytest.mark.parametrize("multi", [False, True])
def test_mine_negatives_equals_the_restatement(built, gpu, tmp_path, multi, sim, shift):
    from jda_amd import api
    from oracle import cpp_reading2 as r2
    from oracle.pyoracle import Oracle
    p = _model(tmp_path, multi, (2, 7), sim, cart_th=-0.8)
    c, o, m2 = api.Cascador(p), Oracle(p), r2.Model2(p)
    c.set_similarity_transform(sim)
    bgs = _bgs(5, 11)
    steps, factors = api.mine_params(5, QS, seed=4)
    tfs = [0, 1, 2, 5, 7]
    for size, start in ((6, 0), (1000, 3)):
        want = mining_ref.mine(m2, o.resize_cv, bgs, steps, factors, tfs, size, start, OS, HS, QS, shift, 21, sim)
        got = c.mine_negatives_cpp(bgs, steps, factors, tfs, size, start=start, shift_size=shift, seed=21)
        _check_mine(got, want, c.dim)
        assert got["stats"]["windows"] == want["next_start"] - start
        assert len(want["hits"]) + want["nega_n"] == want["next_start"] - start
    c.close(); o.close()


def test_mine_transforms_remap_like_numpy(built, gpu, tmp_path):
    from jda_amd import api
    c = api.Cascador(_model(tmp_path, True, None, False, cart_th=-1.5))
    bg = _images([(103, 77)], seed=3)[0]
    for t in range(8):
        a = c.mine_negatives_cpp([bg], [5], [1.2], [t], 10 ** 6)
        b = c.mine_negatives_cpp([mining_ref.transform(bg, t)], [5], [1.2], [0], 10 ** 6)
        for k in ("hits", "score", "shape", "o", "h", "q"):
            assert same(a[k], b[k]), (t, k)
        assert a["stats"] == {**b["stats"], "call_ms": a["stats"]["call_ms"]}
        assert len(a["hits"]) > 0
    c.close()


def test_mine_cursor_chains_and_runs_out(built, gpu, tmp_path):
    from jda_amd import api
    c = api.Cascador(_model(tmp_path, False, None, False, cart_th=-0.9))
    bgs = _bgs(8, 5)
    steps, factors = api.mine_params(8, QS, seed=1)
    tfs = list(range(8))
    one = c.mine_negatives_cpp(bgs, steps, factors, tfs, 10 ** 6, device=True)
    total = one["stats"]["total_windows"]
    assert one["stats"]["next_start"] == total and one["stats"]["windows"] == total
    assert len(one["hits"]) + one["stats"]["nega_n"] == total
    parts, start, nega, carts = [], 0, 0, 0
    while start < total:
        r = c.mine_negatives_cpp(bgs, steps, factors, tfs, 3, start=start)
        parts.append(r); nega += r["stats"]["nega_n"]; carts += r["stats"]["carts_n"]
        assert r["stats"]["windows"] == r["stats"]["next_start"] - start
        start = r["stats"]["next_start"]
    for k in ("hits", "score", "shape", "o", "h", "q"):
        assert same(np.concatenate([r[k] for r in parts]), one[k]), k
    assert (nega, carts) == (one["stats"]["nega_n"], one["stats"]["carts_n"])
    # chunks of 100 windows: the counters and hits stay the same
    c.set_option("mine_chunk_windows", 100)
    small = c.mine_negatives_cpp(bgs, steps, factors, tfs, 10 ** 6, device=True)
    for k in ("hits", "score", "shape", "o"):
        assert same(small[k], one[k]), k
    assert {**small["stats"], "call_ms": 0} == {**one["stats"], "call_ms": 0}
    c.close()


def test_mine_extremes(built, gpu, tmp_path):
    from jda_amd import api, synth
    from oracle.pyoracle import Oracle
    bgs = _bgs(3, 9)
    steps, factors, tfs = [7, 9, 5], [1.3, 1.45, 1.2], [0, 3, 6]
    p = _model(tmp_path, True, None, False, cart_th=synth.NEG_BIG)
    c, o = api.Cascador(p), Oracle(p)
    r = c.mine_negatives_cpp(bgs, steps, factors, tfs, 10 ** 6)
    want = [(i, x, y, w) for i in range(3) for (x, y, w) in mining_ref.windows(*mining_ref.transform(bgs[i], tfs[i]).shape[::-1], OS,
                                                                                steps[i], factors[i])]
    assert np.array_equal(r["hits"], np.array(want, np.int32))
    assert r["stats"]["nega_n"] == 0 and r["stats"]["carts_n"] == 0
    for j in range(0, len(want), 7):
        i, x, y, w = want[j]
        pt = mining_ref.chain(o.resize_cv, mining_ref.transform(bgs[i], tfs[i])[y:y + w, x:x + w], 0, OS, HS, QS)
        for k, q in zip("ohq", pt):
            assert np.array_equal(r[k][j], q), (j, k)
    c.close(); o.close()
    c = api.Cascador(_model(tmp_path, False, None, False, cart_th=1e30))
    r = c.mine_negatives_cpp(bgs, steps, factors, tfs, 10)
    st = r["stats"]
    assert len(r["hits"]) == 0 and st["nega_n"] == st["windows"] == st["total_windows"] == len(want) and st["carts_n"] == st["nega_n"]
    c.close()


def test_mine_large_job_rechecked_by_validate(built, gpu, tmp_path):
    from jda_amd import api, synth
    m = synth.make_model(3, 60, 5, 4, seed=12, cart_th=-1.0)
    frames = synth.make_frames(4, 160, 120, seed=3)
    synth.calibrate_thresholds(m, frames, tau=8.0, p_final=2e-2, min_size=48)
    p = str(tmp_path / "cal.model")
    m.save(p, 8, header_stage=2, header_cart=30)
    c = api.Cascador(p)
    rng = np.random.default_rng(0)
    sizes = [(int(rng.integers(60, 200)), int(rng.integers(60, 200))) for _ in range(300)]
    bgs = _images(sizes, seed=17)
    steps, factors = api.mine_params(len(bgs), QS, seed=2)
    tfs = rng.integers(0, 8, len(bgs))
    r = c.mine_negatives_cpp(bgs, steps, factors, tfs, 10 ** 6, device=True)
    st = r["stats"]
    assert len(r["hits"]) + st["nega_n"] == st["windows"] == st["total_windows"] > 0
    assert 0 < len(r["hits"]) < st["windows"]
    # every hit, as a caller crop of its transformed image through the mining chain, is a face with the same bits
    tb = {}
    for i in set(int(v) for v in r["hits"][:, 0]):
        tb[i] = mining_ref.transform(bgs[i], int(tfs[i]))
    ids = sorted(tb)
    crops = np.array([(ids.index(int(i)), x, y, w, w) for (i, x, y, w) in r["hits"]], np.int32)
    v = c.validate_cpp([tb[i] for i in ids], crops, mode=0)
    assert v["is_face"].all()
    assert same(v["score"], r["score"]) and same(v["shape"], r["shape"])
    c.close()
