"""The carry of stage-0 leaves from k_filter0 to k_finish(survivors) (jda_amd/csrc/k_finish.hip, kernels.h: carry_pack):
a window that passes every cart of stage 0 in k_filter0 takes the leaves it found there along in the mid queue, and
k_finish reads them instead of walking the stage's trees a second time.  Nothing the reference computes changes
(c/jda.c:366-411): detections and the per-window trace -- carts evaluated, score bits, leaf-path hash, shape bits --
are the oracle's, and the compiled reference's where a build for the dimensions exists.  Every comparison is exact
(float bits viewed as integers), and a case whose precondition does not hold FAILS: it would not test the path.

The pack / unpack arithmetic itself needs no GPU: kernels.h states it as constexpr functions with static_asserts
(compiled into every build), and tests/c/carry_check.cpp runs the same functions on the host over whole words."""
import os
import subprocess

import numpy as np
import pytest

from conftest import S_DIMS, same, bits

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FINISH_MERGE = 4096          # host.h: hand-off queues up to this length take ONE k_finish launch, longer ones k_filter0 first
HANDOFF = 128                # option `handoff`: carts of stage 0 the scan evaluates
TILE_WIN = 72                # largest window k_finish copies to LDS with the shipped dimensions


@pytest.fixture(scope="module")
def gpu():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    return torch.device("cuda", 0)


def _fits(dims):
    """kernels.h: carry_fits -- bits = ceil(log2(leaf_n)), rounds = ceil(K / 64), one 32-bit word a lane."""
    _, K, _, D = dims
    leaf_n = 1 << (D - 1)
    b = 0
    while (1 << b) < leaf_n:
        b += 1
    return b * ((K + 63) // 64) <= 32


def _cascador(path, real="auto", env=None, **options):
    """A cascador whose passes go window by window through the queues (no dense mode, no whole-workgroup finisher)."""
    from jda_amd import api
    old = dict(os.environ)
    os.environ.update(env or {})
    try:
        c = api.Cascador(path, real)          # (the JDA_* environment is read here)
    finally:
        os.environ.clear(); os.environ.update(old)
    for k, v in dict(dict(dense=0, wide_max=0), **options).items():
        c.set_option(k, v)
    return c


def _window_sizes(c, w, h, **kw):
    return np.concatenate([np.full(l["nx"] * l["ny"], l["win"]) for l in c.plan_tiles(w, h, **kw)])


def _trace_vs_oracle(c, o, frames):
    """-> the device trace, compared row by row with the oracle's."""
    g = c.trace(frames)
    off = 0
    for i in range(len(frames)):
        r = o.trace(frames[i])
        n = len(r["carts_n"])
        for k in ("carts_n", "score", "path_hash", "shapes"):
            assert same(r[k], g[k][off:off + n]), (i, k, int((bits(r[k]) != bits(g[k][off:off + n])).sum()))
        off += n
    assert off == len(g["carts_n"])
    return g


def _launches(c, fn, *a, **kw):
    """-> (what the call returned, {FinishLaunch: count} and {form: count} of its passes: jdaFinishLaunches / jdaFinishForms
    after minus before, zeros left out)."""
    b_l, b_f = c.finish_launches(), c.finish_forms()
    r = fn(*a, **kw)
    a_l, a_f = c.finish_launches(), c.finish_forms()
    return r, {k: v - b_l.get(k, 0) for k, v in a_l.items() if v != b_l.get(k, 0)}, {k: a_f[k] - b_f[k] for k in a_f if a_f[k] != b_f[k]}


def _pair(dialect, trace, carry, groups=3, n=1):
    """The launches of n passes that take k_filter0 + k_finish(survivors) with the shipped dimensions: three cart groups a round
    (K = 540), windows up to the tile in LDS, both kernels with the carry or both without."""
    from jda_amd import api
    return {api.FinishLaunch("k_filter0", dialect, trace, 0, False, False, False, False, carry, False): n,
            api.FinishLaunch("k_finish", dialect, trace, groups, False, False, False, True, carry, True): n}


def _same_dets(a, b, keys=("bboxes", "scores", "shapes")):
    assert len(a) == len(b)
    for i, (x, y) in enumerate(zip(a, b)):
        for k in keys:
            assert same(x[k], y[k]), (i, k)


# ---------------------------------------------------------------- the arithmetic, on the host

def test_pack_unpack_on_the_host(tmp_path):
    """tests/c/carry_check.cpp includes csrc/kernels.h (whose static_asserts cover leaf_n in {2, 4, 8} x K in {64, 540,
    682}) and round-trips whole 64-lane queue entries through carry_pack / carry_unpack for the same sets."""
    from jda_amd import build as lib_build
    exe = str(tmp_path / "carry_check")
    r = subprocess.run([lib_build.hipcc(), "--offload-arch=gfx950", "-std=c++17", "-O1", "-I", os.path.join(ROOT, "jda_amd", "csrc"),
                        os.path.join(ROOT, "tests", "c", "carry_check.cpp"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    assert "carry ok" in r.stdout and "leaf_n 8 K 682 fits 0" in r.stdout and "leaf_n 8 K 540 fits 1" in r.stdout


# ---------------------------------------------------------------- cases 1 and 2: uniform batch, both tile classes; carry off

@pytest.mark.gpu
def test_carry_vs_oracle_and_reference_and_with_the_carry_off(built, gpu, model_file):
    import torch
    from jda_amd import synth
    from oracle import pyoracle
    assert _fits(S_DIMS)
    T, K = S_DIMS[0], S_DIMS[1]
    p, _ = model_file(S_DIMS, 8, seed=3, cart_th=-1.0, norm_every=5)
    frames = synth.make_frames(2, 640, 480, seed=11)
    o = pyoracle.Oracle(p)
    c = _cascador(p)
    assert c.get_option("fin_carry") == 1 and c.get_option("filter0") == 1 and c.get_option("handoff") == HANDOFF
    g = _trace_vs_oracle(c, o, frames)
    # preconditions: the pass is long enough for k_filter0, and its survivors come from both sides of the LDS tile limit
    win = np.tile(_window_sizes(c, 640, 480), len(frames))
    assert len(win) == len(g["carts_n"])
    assert int((g["carts_n"] > HANDOFF).sum()) > FINISH_MERGE
    passed0 = g["carts_n"] > K
    small, large = int((passed0 & (win <= TILE_WIN)).sum()), int((passed0 & (win > TILE_WIN)).sum())
    print("stage-0 survivors: %d windows up to %d pixels, %d larger; %d pass every stage" % (small, TILE_WIN, large, int((g["carts_n"] == T * K).sum())))
    assert small > 0 and large > 0
    assert int((g["carts_n"] == T * K).sum()) > 0
    d = torch.from_numpy(frames).to(gpu)
    before, l_before = c.finish_forms(), c.finish_launches()
    dets, st = c.detect_batch_device(d, stats=True)
    forms = {k: v - before[k] for k, v in c.finish_forms().items() if v != before[k]}
    launches = {k: v - l_before.get(k, 0) for k, v in c.finish_launches().items() if v != l_before.get(k, 0)}
    print("forms:", forms, sorted(launches.items()))
    # every launch of the call is k_filter0 or k_finish(survivors), both with the carry, k_finish with three cart groups (K = 540)
    assert launches and {k.kernel for k in launches} == {"k_filter0", "k_finish"}, launches
    assert all(k.carry and not k.trace and k.dialect == "C" for k in launches), launches
    assert all(k.survivors and k.groups == 3 and k.tile for k in launches if k.kernel == "k_finish"), launches
    assert forms and set(forms) <= {"FILTER0", "MID_DIRECT"}, forms      # k_filter0 + k_finish(survivors): the carry's path
    assert st["handoff_n"] > FINISH_MERGE and st["dense_passes"] == 0
    ref = pyoracle.Reference(p, S_DIMS, 8) if pyoracle.reference_lib_path(*S_DIMS) else None
    for i in range(len(frames)):
        want = o.detect(frames[i])
        for k in ("bboxes", "scores", "shapes"):
            assert same(dets[i][k], want[k]), (i, k)
            if ref is not None:
                assert same(dets[i][k], ref.detect(frames[i])[k]), (i, k)
    assert sum(len(x["scores"]) for x in dets) > 0
    # case 2: the same job with the carry switched off, and without k_filter0 altogether: identical rows
    for opts in (dict(fin_carry=0), dict(filter0=0)):
        c2 = _cascador(p, **opts)
        g2 = c2.trace(frames)
        for k in ("carts_n", "score", "path_hash", "shapes"):
            assert same(g[k], g2[k]), (opts, k)
        dets2, st2 = c2.detect_batch_device(d, stats=True)
        _same_dets(dets, dets2)
        for k in ("cart_total_n", "handoff_n", "face_patch_n", "stage_done_n"):
            assert st[k] == st2[k], (opts, k)
        c2.close()
    # ... and a hand-off that does not fall on a round of 64 carts (the first round k_filter0 walks is scored in part)
    c3 = _cascador(p, handoff=100)
    g3 = c3.trace(frames)
    for k in ("carts_n", "score", "path_hash", "shapes"):
        assert same(g[k], g3[k]), k
    c3.close(); c.close()


# ---------------------------------------------------------------- case 3: carried and sentinel entries in one launch

@pytest.mark.gpu
def test_entries_from_the_persistent_scan_mix_with_carried_ones(built, gpu, model_file):
    """k_scan_p up to cart K puts its stage-0 survivors into the mid queue itself (no leaves: m_k0 = K); the levels it
    does not cover go through the hand-off queue and k_filter0 (leaves carried): one k_finish(survivors) launch."""
    import torch
    from jda_amd import synth
    from oracle.pyoracle import Oracle
    K = S_DIMS[1]
    p, _ = model_file(S_DIMS, 8, seed=3, cart_th=-1.0, norm_every=5)
    frames = synth.make_frames(4, 640, 480, seed=12)
    d = torch.from_numpy(frames).to(gpu)
    base_env = {"JDA_MERGE_BLOCKS": "0"}
    c0 = _cascador(p, env=dict(base_env, JDA_SCAN_P="0"))
    want, st0 = c0.detect_batch_device(d, stats=True)
    o = Oracle(p)
    tr = o.trace(frames[0])
    wd = o.detect(frames[0])
    for k in wd:
        assert same(want[0][k], wd[k]), k
    # precondition from the oracle and the plan: stage-0 survivors on levels of the LDS-tiled mode (k_scan_p's) and of the
    # global-pixel mode (k_scan -> hand-off queue -> k_filter0)
    mode = np.concatenate([np.full(l["nx"] * l["ny"], l["mode"]) for l in c0.plan_tiles(640, 480)])
    assert int(((tr["carts_n"] > K) & (mode == 1)).sum()) > 0 and int(((tr["carts_n"] > K) & (mode != 1)).sum()) > 0
    env = dict(base_env, JDA_SCAN_P="2", JDA_SCAN_P_HANDOFF="100000", JDA_SCAN_P_B2="128", JDA_SCAN_P_B3="256", JDA_SCAN_P_LG="64478")
    c1 = _cascador(p, env=env)
    assert c1.get_option("scan_p_mid") == 1 and c1.get_option("fin_carry") == 1
    for rep in range(2):                                   # (the second pass sizes its launches from the first)
        scans_before = c1.scan_forms()
        (got, st1), launches, forms = _launches(c1, c1.detect_batch_device, d, stats=True)
        scans = {k: v - scans_before.get(k, 0) for k, v in c1.scan_forms().items() if v != scans_before.get(k, 0)}
        print("pass", rep, "forms:", forms, scans, sorted(launches.items()))
        assert forms and set(forms) == {"MID_DIRECT"}, forms       # k_filter0 + k_finish(survivors) fed from k_scan_p's mid queue
        # ... a k_filter0 and a k_finish(survivors) launch a pass, both with the carry (jdaFinishLaunches)
        assert launches == _pair("C", False, True, n=forms["MID_DIRECT"]), launches
        # ... and the scan that filled it was k_scan_p (jdaScanForms), next to k_scan's global-pixel launch
        assert any(k.kernel == "k_scan_p" and k.depth == 4 and not k.ragged for k in scans) and any(k.pix == "GLB" for k in scans), scans
        _same_dets(want, got)
        for k in ("cart_total_n", "face_patch_n", "stage_done_n", "patch_n"):
            assert st0[k] == st1[k], (rep, k)
        # the persistent scan did run past the common hand-off (its carts count as scan carts): its survivors are in the mid queue
        assert st1["scan_cart_n"] > st0["scan_cart_n"] and st1["scan_fallbacks"] == 0 and st1["dense_passes"] == 0
    c1o = _cascador(p, env=env, fin_carry=0)
    (got, _), launches, forms = _launches(c1o, c1o.detect_batch_device, d, stats=True)
    print("fin_carry = 0:", forms, sorted(launches.items()))
    assert set(forms) == {"MID_DIRECT"} and launches == _pair("C", False, False, n=forms["MID_DIRECT"]), (forms, launches)
    _same_dets(want, got)
    for c in (c0, c1, c1o):
        c.close()


# ---------------------------------------------------------------- case 4: a model whose leaves do not fit a word

@pytest.mark.gpu
def test_a_model_too_deep_for_the_word_walks_as_before(built, gpu, model_file):
    import torch
    from jda_amd import synth
    from oracle.pyoracle import Oracle
    dims = (2, 448, 5, 6)                      # 32 leaves = 5 bits, 7 rounds of 64 carts: 35 bits
    assert not _fits(dims)
    p, _ = model_file(dims, 8, seed=7, cart_th=-2.0, norm_every=5)
    frames = synth.make_frames(4, 400, 300, seed=13)
    c, o = _cascador(p), Oracle(p)
    assert c.get_option("fin_carry") == 1
    g = _trace_vs_oracle(c, o, frames)
    # k_filter0 and k_finish(survivors) ran, neither with the carry (jdaFinishLaunches); K = 448 walks four cart groups a round
    launches = c.finish_launches()
    print("launches:", sorted(launches.items()))
    assert {k.kernel for k in launches} == {"k_filter0", "k_finish"} and not any(k.carry for k in launches), launches
    assert all(k.survivors and k.groups == 4 and k.trace for k in launches if k.kernel == "k_finish"), launches
    assert int((g["carts_n"] > HANDOFF).sum()) > FINISH_MERGE and int((g["carts_n"] > dims[1]).sum()) > 0
    dets = c.detect_batch_device(torch.from_numpy(frames).to(gpu))
    for i in range(len(frames)):
        want = o.detect(frames[i])
        for k in want:
            assert same(dets[i][k], want[k]), (i, k)
    c.close()


# ---------------------------------------------------------------- case 5: a ragged job and a dialect-CPP call

@pytest.mark.gpu
def test_ragged_job_and_dialect_cpp(built, gpu, model_file):
    import torch
    from jda_amd import synth
    from oracle.pyoracle import Oracle
    K = S_DIMS[1]
    p, _ = model_file(S_DIMS, 8, seed=3, cart_th=-1.0, norm_every=5)
    o = Oracle(p)
    rng = np.random.default_rng(5)
    base = synth.make_frames(6, 400, 300, seed=15)
    imgs = [np.ascontiguousarray(base[i % 6][:int(rng.integers(150, 301)), :int(rng.integers(200, 401))]) for i in range(24)]
    c = _cascador(p)
    (got, st), launches, forms = _launches(c, c.detect_ragged, imgs, stats=True)
    print("ragged:", forms, sorted(launches.items()))
    assert st["handoff_n"] > FINISH_MERGE and st["dense_passes"] == 0
    # the job's passes took k_filter0 + k_finish(survivors), every launch with the carry
    assert forms and set(forms) <= {"FILTER0", "MID_DIRECT"} and launches == _pair("C", False, True, n=sum(forms.values())), (forms, launches)
    n_pass0 = 0
    for i in (0, 5, 11, 23):
        want = o.detect(imgs[i])
        for k in ("bboxes", "scores", "shapes"):
            assert same(got[i][k], want[k]), (i, k)
        n_pass0 += int((o.trace(imgs[i], want_shapes=False)["carts_n"] > K).sum())
    assert n_pass0 > 0 and sum(len(x["scores"]) for x in got) > 0
    c0 = _cascador(p, fin_carry=0)
    got0, launches, forms = _launches(c0, c0.detect_ragged, imgs)
    assert forms and set(forms) <= {"FILTER0", "MID_DIRECT"} and launches == _pair("C", False, False, n=sum(forms.values())), (forms, launches)
    _same_dets(got, got0)
    c0.close()
    # dialect CPP: the fp64 instantiation of the same two kernels
    frames = synth.make_frames(2, 400, 300, seed=16)
    kw = dict(minimum_size=20, step=5, factor=1.2)
    gt, launches, forms = _launches(c, c.trace_cpp, frames, **kw)
    print("trace_cpp:", forms, sorted(launches.items()))
    assert forms == {"FILTER0": 1} and launches == _pair("CPP", True, True), (forms, launches)
    off = 0
    for i in range(len(frames)):
        r = o.trace_cpp(frames[i], **kw)
        n = len(r["carts_n"])
        for k in ("carts_n", "score", "path_hash", "shapes"):
            assert same(r[k], gt[k][off:off + n]), (i, k)
        off += n
    assert off == len(gt["carts_n"])
    assert int((gt["carts_n"] > HANDOFF).sum()) > FINISH_MERGE and int((gt["carts_n"] > K).sum()) > 0
    (dets, stc), launches, forms = _launches(c, c.detect_batch_cpp_device, torch.from_numpy(frames).to(gpu), overlap=0.3, nms=True, stats=True, **kw)
    print("detect_cpp:", forms, sorted(launches.items()))
    assert forms == {"FILTER0": 1} and launches == _pair("CPP", False, True), (forms, launches)
    assert stc["handoff_n"] > FINISH_MERGE and stc["dense_passes"] == 0
    for i in range(len(frames)):
        want = o.detect_cpp(frames[i], overlap=0.3, nms=True, **kw)
        for k in ("rects", "scores", "shapes"):
            assert same(dets[i][k], want[k]), (i, k)
    assert sum(len(x["scores"]) for x in dets) > 0
    c.close()


# ---------------------------------------------------------------- case 6: the mid queue overflows and grows

@pytest.mark.gpu
def test_mid_queue_overflow_regrows_the_leaf_words_too(built, gpu, tmp_path):
    """A cascade whose scan keeps 7 % of the windows -- within the first pass's guess for the hand-off queue, an eighth --
    and whose stage 0 rejects nobody after the hand-off: the mid queue, guessed at 1 / 32 of the windows, overflows on its
    own.  The pass is run again with a grown workspace (jdaStats.ws_regrows), leaf words included: the oracle's rows."""
    import torch
    from jda_amd import api, synth
    from oracle.pyoracle import Oracle
    K = S_DIMS[1]
    m = synth.make_model(*S_DIMS, seed=3, cart_th=-0.1, norm_every=5)
    m.cth[0, HANDOFF:] = -1.0e30
    p = str(tmp_path / "mid_overflow.model")
    m.save(p, 8)
    frames = synth.make_frames(4, 640, 480, seed=17)
    d = torch.from_numpy(frames).to(gpu)
    o = Oracle(p)
    trs = [o.trace(f, want_shapes=False)["carts_n"] for f in frames]
    tail, mid, n = sum(int((t > HANDOFF).sum()) for t in trs), sum(int((t > K).sum()) for t in trs), sum(len(t) for t in trs)
    # preconditions (host.h: queue_caps without a prediction): the hand-off queue holds, the mid queue does not
    assert FINISH_MERGE < tail < n // 8 and mid > n // 32 + 64
    c = _cascador(p, ws_min_entries=1, ws_factor_pct=100)
    (got, st), launches, forms = _launches(c, c.detect_batch_device, d, th=-1.0e30, stats=True)
    print("first call:", forms, sorted(launches.items()), "ws_regrows", st["ws_regrows"])
    assert st["ws_regrows"] >= 1 and api.last_error() == ""
    # the pass that overflowed and every rerun launched the pair again: whole multiples, one more pass than regrows at least
    n = sum(forms.values())
    assert set(forms) == {"FILTER0"} and n >= 2 and launches == _pair("C", False, True, n=n), (forms, launches)
    assert st["handoff_n"] == tail and st["stage_done_n"][0] == mid
    (got2, st2), launches, forms = _launches(c, c.detect_batch_device, d, th=-1.0e30, stats=True)          # (the rerun taught the plan its fractions)
    assert st2["ws_regrows"] == 0
    assert set(forms) == {"FILTER0"} and launches == _pair("C", False, True, n=sum(forms.values())), (forms, launches)
    _same_dets(got, got2)
    for i in range(len(frames)):
        want = o.detect(frames[i], th=-1.0e30)
        for k in ("bboxes", "scores", "shapes"):
            assert same(got[i][k], want[k]), (i, k)
    c0 = _cascador(p, ws_bound=0, fin_carry=0)
    got0, launches, forms = _launches(c0, c0.detect_batch_device, d, th=-1.0e30)
    assert set(forms) == {"FILTER0"} and launches == _pair("C", False, False, n=sum(forms.values())), (forms, launches)
    _same_dets(got, got0)
    assert sum(len(x["scores"]) for x in got) > 0
    c.close(); c0.close()
