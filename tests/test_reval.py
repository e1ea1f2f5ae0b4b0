"""Validate on a resident sample set (jdaValidateSamplesCpp, k_reval.hip): both forms -- reval_form 0, a wave per sample, and
1, the lane-per-sample walk of jdaValidateCpp over the same records -- against tests/model_ref.validate_record, the
sequential restatement of JoinCascador::Validate (cascador.cpp:166-211), bit for bit and without a tolerance.  Dialect CPP is
parity-unpinned: bit-exact against the restatement, not against the reference."""
import ctypes as C

import numpy as np
import pytest

from conftest import same
import model_ref

pytestmark = pytest.mark.gpu

BIG = (48, 36, 24)
ODD = (9, 7, 5)                     # 81 + 49 + 25 = 155 bytes a record: no alignment at all


@pytest.fixture(scope="module")
def gpu():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    return torch.device("cuda", 0)


def _model(T, K, L, D, seed=1, multi=True, th=-np.inf, norm_every=7):
    from jda_amd import synth
    m = synth.make_model(T, K, L, D, seed=seed, cart_th=0.0, norm_every=norm_every, multi_scale=multi, w_sigma=2e-2, f32_exact=False)
    m.cth[:] = th
    return m


def _records(m, n, sizes, seed):
    rng = np.random.default_rng(seed)
    pb = sum(v * v for v in sizes)
    patches = rng.integers(0, 256, (n, pb), dtype=np.uint8)
    starts = m.mean_shape[None, :] + rng.normal(0, 0.06, (n, m.dim))
    starts[::7] += rng.uniform(-0.8, 0.8, (len(starts[::7]), m.dim))          # some landmarks leave the patch: clamping
    return patches, starts


def _split(row, sizes):
    o, h, q = sizes
    return row[:o * o].reshape(o, o), row[o * o:o * o + h * h].reshape(h, h), row[o * o + h * h:].reshape(q, q)


def _reference(blob, patches, starts, sizes):
    m2 = model_ref.model2_of(blob)
    res = [model_ref.validate_record(m2, *_split(patches[i], sizes), starts[i]) for i in range(len(patches))]
    return dict(is_face=np.array([r[0] for r in res], np.uint8), score=np.array([r[1] for r in res], np.float64),
                shape=np.array([r[2] for r in res], np.float64).reshape(len(res), -1), carts_n=np.array([r[3] for r in res], np.int32))


def _cascador(tmp_path, m, hdr=None, name="m.model"):
    from jda_amd import api
    p = str(tmp_path / name)
    with open(p, "wb") as f:
        f.write(m.tobytes(8) if hdr is None else m.tobytes(8, hdr[0], hdr[1]))
    return api.Cascador(p, "double", device=0), open(p, "rb").read()


def _both_forms(c, samples, want, sizes, forms=(0, 1)):
    out = None
    for form in forms:
        c.set_option("reval_form", form)
        got = c.validate_samples_cpp(samples, *sizes)
        for k in ("is_face", "carts_n", "score", "shape"):
            assert same(got[k], want[k]), (form, k)
        out = out or got
    c.set_option("reval_form", 0)
    return out


@pytest.mark.parametrize("K,n,D,L,sizes", [(1, 1, 2, 1, ODD), (63, 63, 4, 5, ODD), (64, 64, 2, 27, BIG), (65, 65, 6, 5, ODD),
                                           (130, 65, 4, 68, ODD), (5, 200, 4, 5, BIG)])
def test_lane_and_chunk_edges(built, gpu, tmp_path, K, n, D, L, sizes):
    """Carts at and around the 64 lanes of a wave, samples at and around the waves of a workgroup, tree depths with 1, 3 and
    5 node levels, shapes of 2 to 136 coordinates (more than one round of lane = coordinate), two stages so that stage 1 walks
    on regressed shapes.  A constant threshold cuts some samples somewhere.
    Two rows run once more from global memory (reval_lds_kb 0), the path k_reval shares with k_lbf: (65, 65, 6, 5) -- a second
    round of carts of one lane, K % 8 = 1 rows in the regression's last batch, odd patch offsets -- and (130, 65, 4, 68) -- three
    rounds of carts, three of coordinates, K % 8 = 2."""
    m = _model(2, K, L, D, seed=K + n, th=-0.4 * np.sqrt(K))
    c, blob = _cascador(tmp_path, m)
    patches, starts = _records(m, n, sizes, seed=n)
    want = _reference(blob, patches, starts, sizes)
    got = _both_forms(c, dict(patches=patches, shapes=starts), want, sizes)
    assert got["stats"]["lds_path"] == 1 and got["stats"]["chunks"] == 1
    if (K, n, D, L) in ((65, 65, 6, 5), (130, 65, 4, 68)):
        c.set_option("reval_lds_kb", 0)
        got = _both_forms(c, dict(patches=patches, shapes=starts), want, sizes, forms=(0,))
        assert got["stats"]["lds_path"] == 0 and got["stats"]["chunks"] == 1
    c.close()


def test_rejection_at_every_position_that_can_go_wrong(built, gpu, tmp_path):
    """K = 130, T = 2, a snapshot at (1, 3): thresholds at the first cart, at carts 63, 64 and 65 (the last lane of a round of 64,
    the first and second of the next), at the last cart of stage 0 (no regression may run), at the first cart of stage 1 and
    inside the partial stage; -inf everywhere else (never rejects).  Each threshold is the score of one of the samples still
    alive at that cart (about an eighth of them lie below it), so `score == th` occurs at every one of them and must pass.
    Normalising carts (every 7th) come before and after each rejecting cart."""
    K, n, sizes = 130, 48, ODD
    m = _model(2, K, 5, 3, seed=11)
    patches, starts = _records(m, n, sizes, seed=5)
    cut_at = [(0, 0), (0, 63), (0, 64), (0, 65), (0, K - 1), (1, 0), (1, 2)]
    for (t, k) in cut_at:                                  # the scores of the survivors right after cart (t, k)
        r = _reference(m.tobytes(8, t, k), patches, starts, sizes)
        alive = np.sort(r["score"][r["is_face"] == 1])
        below = np.searchsorted(alive, alive, side="left")            # samples strictly below each score
        m.cth[t, k] = alive[np.argmax(below >= max(1, len(alive) // 8))]    # (ties: the first cart has only four leaf values)
    c, blob = _cascador(tmp_path, m, hdr=(1, 3))
    want = _reference(blob, patches, starts, sizes)
    rejected = want["is_face"] == 0
    assert rejected.mean() >= 0.25 and (~rejected).mean() >= 0.25                  # the issue's shares, on the reference's output
    ends = {t * K + k + 1 for (t, k) in cut_at}
    assert set(want["carts_n"][rejected].tolist()) == ends                         # every position did reject somebody
    assert (want["carts_n"][~rejected] == K + 4).all()
    stage0_last = want["carts_n"] == K                                            # rejected by the last cart of stage 0:
    assert stage0_last.any() and same(want["shape"][stage0_last], starts[stage0_last])   # ... the shape as it stood
    _both_forms(c, dict(patches=patches, shapes=starts), want, sizes)
    c.close()


def test_equal_scores_pass_infinite_thresholds_and_nan_leaves(built, gpu, tmp_path):
    """`score == th` passes (a cart whose leaves are all 0.25 with th 0.25 on a zero score); th = -inf never rejects; a NaN
    score from a NaN leaf rejects nowhere afterwards, `score < th` being false -- even under th = +inf."""
    m = _model(2, 5, 5, 3, seed=3, norm_every=100)
    m.leaf[0, 0] = 0.25; m.cth[0, 0] = 0.25
    patches, starts = _records(m, 40, ODD, seed=9)
    c, blob = _cascador(tmp_path, m, name="eq.model")
    want = _reference(blob, patches, starts, ODD)
    assert want["is_face"].all() and (want["carts_n"] == 10).all()
    _both_forms(c, dict(patches=patches, shapes=starts), want, ODD)
    c.close()
    m.leaf[0, 2, 1] = np.nan                             # some samples reach this leaf
    m.cth[1, :] = np.inf
    m.cmean[0, 3], m.cstd[0, 3] = 0.125, 2.0             # a normalising cart right after it
    c, blob = _cascador(tmp_path, m, name="nan.model")
    want = _reference(blob, patches, starts, ODD)
    nan = np.isnan(want["score"])
    assert nan.any() and not nan.all() and want["is_face"][nan].all() and not want["is_face"][~nan].any()
    assert (want["carts_n"][~nan] == 6).all()            # +inf rejects every finite score at the first cart of stage 1
    _both_forms(c, dict(patches=patches, shapes=starts), want, ODD)
    c.close()


@pytest.mark.parametrize("hdr", [(0, -1), (0, 0), (1, -1), (1, 2), None])
def test_statuses(built, gpu, tmp_path, hdr):
    m = _model(2, 5, 5, 3, seed=8, th=-0.3)
    c, blob = _cascador(tmp_path, m, hdr)
    patches, starts = _records(m, 70, BIG, seed=2)
    want = _reference(blob, patches, starts, BIG)
    got = _both_forms(c, dict(patches=patches, shapes=starts), want, BIG)
    if hdr == (0, -1):                                   # nothing runs: everything passes with zero carts
        assert got["is_face"].all() and not got["carts_n"].any() and same(got["score"], np.zeros(70)) and same(got["shape"], starts)
    else:
        assert 0 < got["is_face"].sum() < 70
    c.close()


def test_device_patches_chunks_and_repeatability(built, gpu, tmp_path):
    """Host and device patches (a device view at an odd byte offset), a workspace that cuts the set into three chunks, the
    same call twice."""
    import torch
    m = _model(1, 3, 5, 3, seed=4, th=-0.5)
    c, blob = _cascador(tmp_path, m)
    n = 500
    patches, starts = _records(m, n, BIG, seed=6)
    want = _reference(blob, patches, starts, BIG)
    host = dict(patches=patches, shapes=starts)
    a = _both_forms(c, host, want, BIG)
    buf = torch.zeros(patches.size + 3, dtype=torch.uint8, device=gpu)
    buf[3:] = torch.from_numpy(patches.reshape(-1)).to(gpu)
    _both_forms(c, dict(patches=buf[3:], shapes=starts), want, BIG)
    _both_forms(c, dict(patches=buf[3:3 + 65 * patches.shape[1]], shapes=starts[:65]), {k: v[:65] for k, v in want.items()}, BIG)
    c.set_option("workspace_mb", 1)                      # 1 MB / (4,176 patch bytes + 249 of shapes, indicators, outputs) = 236 records a chunk: 500 are three
    b = _both_forms(c, host, want, BIG)
    assert a["stats"]["chunks"] == 1 and b["stats"]["chunks"] == 3
    again = c.validate_samples_cpp(host, *BIG)
    for k in ("is_face", "carts_n", "score", "shape"):
        assert same(again[k], b[k]), k
    c.close()


def test_lds_path_equals_global_path_at_the_edge(built, gpu, tmp_path):
    """A wave's slice at 48 / 36 / 24, L = 5, K = 5: 80 (shape) + 32 (indicators) + 4,192 (patches + 3, rounded to 16) = 4,304
    bytes.  Four waves by default; reval_lds_kb 5 (5,120 bytes) still fits one, 4 (4,096) fits none and the kernel works in
    global memory; 0 likewise."""
    m = _model(2, 5, 5, 3, seed=8, th=-0.9)
    c, blob = _cascador(tmp_path, m)
    patches, starts = _records(m, 67, BIG, seed=2)
    want = _reference(blob, patches, starts, BIG)
    s = dict(patches=patches, shapes=starts)
    st = _both_forms(c, s, want, BIG, forms=(0,))["stats"]
    assert (st["lds_path"], st["waves_per_group"], st["lds_bytes"]) == (1, 4, 4 * 4304)
    for kb, path, waves in ((5, 1, 1), (4, 0, 4), (0, 0, 4)):
        c.set_option("reval_lds_kb", kb)
        st = _both_forms(c, s, want, BIG, forms=(0,))["stats"]
        assert (st["lds_path"], st["waves_per_group"]) == (path, waves), kb
    c.close()


def test_refusals_leave_the_outputs_alone(built, gpu, tmp_path):
    from jda_amd import api
    m = _model(1, 3, 5, 3, seed=4)
    c, _ = _cascador(tmp_path, m)
    patches, starts = _records(m, 8, ODD, seed=1)
    face = np.full(8, 0xA5, np.uint8); score = np.full(8, 7.5); carts = np.full(8, -77, np.int32); shape = np.full((8, 10), 7.5)
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int)

    def call(sizes=ODD, shapes=starts, pats=patches, n=8):
        s = api.jdaSamplesCpp()
        s.patches = pats.ctypes.data if pats is not None else None
        s.shapes = shapes.ctypes.data_as(dp) if shapes is not None else None
        s.n = n
        return api.lib.jdaValidateSamplesCpp(c.h, C.byref(s), *sizes, face.ctypes.data_as(C.POINTER(C.c_ubyte)), score.ctypes.data_as(dp),
                                             carts.ctypes.data_as(ip), shape.ctypes.data_as(dp), None)

    c.set_similarity_transform(True)
    assert call() == -1 and "jdaSetSimilarityTransform" in api.last_error()
    c.set_similarity_transform(False)
    for sizes in ((0, 7, 5), (9, 129, 5), (9, 7, -1)):
        assert call(sizes) == -1 and "[1, 128]" in api.last_error()
    assert call(shapes=None) == -1 and "shapes" in api.last_error()
    assert call(pats=None) == -1 and call(n=-1) == -1
    assert api.lib.jdaValidateSamplesCpp(c.h, None, 9, 7, 5, None, None, None, None, None) == -1
    assert api.lib.jdaValidateSamplesCpp(None, None, 9, 7, 5, None, None, None, None, None) == -1
    assert (face == 0xA5).all() and (score == 7.5).all() and (carts == -77).all() and (shape == 7.5).all()
    assert call(n=0) == 0 and (face == 0xA5).all()
    assert call() == 0 and (carts == 3).all()                            # ... and the call itself works; any output may be NULL
    s = api.jdaSamplesCpp(); s.patches = patches.ctypes.data; s.shapes = starts.ctypes.data_as(dp); s.n = 8
    assert api.lib.jdaValidateSamplesCpp(c.h, C.byref(s), 9, 7, 5, None, None, None, None, None) == 0
    c.close()
