"""Which finishing form a pass took (jdaFinishForms, include/jda.h), and k_finish_wide at the limits of its loops.

After the stage-0 scan a pass finishes its windows in one of seven forms (Pass::launch_finishers, Pass::run_dense).
Every case here states the form it is about, reads the difference of the cascador's form counts around EACH call and
asserts it, so that no comparison below can be one kernel against itself.  What a case compares, bit for bit (`same`):

  * the per-window trace (carts evaluated, score, leaf-path hash, shape) of the form under test against the CPU oracle
    (dialect C: c/jda.c:357-426; dialect CPP: the repository's restatement, parity unpinned as everywhere),
  * the same trace against a second cascador with wide_max = 0 (k_finish, one wave per window),
  * detections and the work counters of the two cascadors.

The inputs of a case must make it mean something: the hand-off queue is short enough for the form and not empty, a
window passes every stage and the final threshold, a window dies inside a later stage (the replay rejects, the adders
drop their sums), and a normalising cart falls into every block of 64 carts.  These are conditions, evaluated from the
oracle's trace on the CPU (test_inputs_meet_their_conditions, no GPU needed) and again by the GPU case itself.

The hand-off queue holds the windows alive after min(K, handoff = 128) carts of stage 0 (k_scan), or every window where
the fast scan is off (kstart = 0).  WIDE_MAX bounds it for k_finish_wide; a later call on the same scan plan sizes its
launch from the earlier pass (Pass::issue_rest: fraction * windows * 1.1 + 64), so the cases keep it at or below
HANDOFF_MAX = (1024 - 64) / 1.1 = 872 and every call of a case takes the same form."""
import atexit
import copy
import functools
import shutil

import numpy as np
import pytest

from conftest import S_DIMS, same, bits

HANDOFF = 128               # option `handoff`
WIDE_MAX = 1024             # option `wide_max`
FINISH_MERGE = 4096         # host.h: Knobs::finish_merge
HANDOFF_MAX = 872           # see above
LDS_BUDGET = 160 * 1024     # k_wide.hip: launch_finish_wide_impl
TILE_CAP = 40 * 1024        # ... the window tile's share of it at most
MAX_STAGES = 16             # kernels.h: kMaxStages
CPP_KW = dict(minimum_size=40, step=6, factor=1.25)
STAT_KEYS = ("patch_n", "face_patch_n", "cart_gothrough_n", "cart_total_n", "handoff_n")


# ---------------------------------------------------------------- k_wide.hip restated

def wide_lds(dim, K, real_bytes, tile_bytes, budget=LDS_BUDGET):
    """k_wide.hip: WideLds -> (row_cap, total bytes)."""
    al = lambda o: (o + 15) & ~15
    k4 = (K + 3) & ~3
    o = al(((dim + 1) & ~1) * real_bytes)          # sh
    o += k4 * 4                                    # lbf
    o = al(o + k4 * real_bytes)                    # lsc
    o = al(o + k4 * real_bytes)                    # lth
    o += (K + 15) & ~15                            # lfi
    o += 64 + MAX_STAGES * 4                       # misc
    o += al(tile_bytes)                            # tile
    left = budget - o
    row_cap = min(K, left // (dim * real_bytes) if left > 0 else 0)
    return row_cap, o + row_cap * dim * real_bytes


def wide_launch(dims, real_bytes, wide_conc=1):
    """launch_finish_wide_impl and finish_wide_ok -> what the launch of a model looks like, or None where the model does
    not go through k_finish_wide at all."""
    T, K, L, D = dims
    dim, leaf_n = 2 * L, 1 << (D - 1)
    if dim > 4 * 256 or leaf_n > 128 or wide_lds(dim, K, real_bytes, 0)[0] < 1:
        return None
    tile_win = 0
    for tw in range(16, 256):
        tb = tw * ((tw + 3) & ~3) + 16
        if wide_lds(dim, K, real_bytes, tb)[0] >= min(K, 64) and tb <= TILE_CAP:
            tile_win = tw
    tile_bytes = tile_win * ((tile_win + 3) & ~3) + 16 if tile_win else 0
    row_cap, total = wide_lds(dim, K, real_bytes, tile_bytes)
    block = 1024 if K > 512 else (512 if K > 256 else 256)
    conc = bool(wide_conc) and 1 + (dim + 63) // 64 <= block // 64
    return dict(tile_win=tile_win, row_cap=row_cap, total=total, block=block, conc=conc,
                form="WIDE_CONC" if conc else "WIDE_SEQ", chunks=[min(row_cap, K - r) for r in range(0, K, row_cap)])


# ---------------------------------------------------------------- the cases

FRAME = (1, 260, 190, 7)     # (frames, width, height, seed)
SMALL = (1, 131, 97, 9)      # every window of it fits the hand-off queue of k_finish_wide: the frame of the kstart = 0 cases
MID = (1, 200, 150, 7)
SEQ = dict(wide_conc=0)
NOFAST = dict(no_fast_scan=1)     # the switch of test_scan_and_generic_walker_agree: every window is queued with kstart = 0


def _case(dims, z, norm_every, form, seed=5, frame=FRAME, opts=None, cpp_kw=None, c_kw=None, norm_last=False):
    return dict(dims=dims, z=z, norm_every=norm_every, seed=seed, frame=frame, opts=dict(opts or {}), form=form, form_cpp=form,
                cpp_kw=dict(cpp_kw or CPP_KW), c_kw=dict(c_kw or {}), norm_last=norm_last)


# One row a case: (T, K, L, D), z, norm_every, the form both dialects must count, then what differs from the defaults.
#   z           how many standard deviations up the gate carts ask the score to be (_gates).  Chosen with the oracle so that
#               the conditions hold in both dialects (hand-off counts between 40 and 600); another value, seed or frame means
#               another look at them -- test_inputs_meet_their_conditions says at once whether they still hold.
#   norm_every  carts whose 1-based index is a multiple normalise the score: one in EVERY block of 64 carts, the last,
#               shorter block included (K = 257 is prime: norm_last makes its cart 257 normalise as well).
CASES = {
    # block selection and the cart loop: 256 / 512 / 1,024 threads; K = 1,025 takes a second round of the thread-per-cart walk
    "block_K256": _case((2, 256, 5, 3), 1.3, 31, "WIDE_CONC", seed=6),
    "block_K257": _case((2, 257, 5, 3), 0.3, 31, "WIDE_CONC", norm_last=True),
    "block_K512": _case((2, 512, 5, 3), 1.3, 31, "WIDE_CONC"),
    "block_K513": _case((2, 513, 5, 3), 1.3, 27, "WIDE_CONC"),
    "block_K1024": _case((2, 1024, 1, 2), 1.5, 31, "WIDE_CONC"),
    "block_K1025": _case((2, 1025, 2, 2), 1.7, 25, "WIDE_CONC"),
    # replay edges: windows of tiled levels arrive with kstart = K (K <= handoff: stage 0's replay runs zero rounds where K is
    # a multiple of 64), windows without the fast scan with kstart = 0 -- two calls of one case, since no option leaves
    # single levels untiled.  The last cart of each normalises.
    "replay_K63_kstartK": _case((2, 63, 5, 3), 1.5, 21, "WIDE_CONC"),
    "replay_K63_kstart0": _case((2, 63, 5, 3), 0.9, 21, "WIDE_CONC", frame=SMALL, opts=NOFAST),
    "replay_K64_kstartK": _case((2, 64, 5, 3), 1.3, 16, "WIDE_CONC"),
    "replay_K64_kstart0": _case((2, 64, 5, 3), 1.3, 16, "WIDE_CONC", frame=SMALL, opts=NOFAST),
    "replay_K65_kstartK": _case((2, 65, 5, 3), 2.5, 13, "WIDE_CONC"),
    "replay_K65_kstart0": _case((2, 65, 5, 3), 2.5, 13, "WIDE_CONC", frame=SMALL, opts=NOFAST),
    "replay_K128_kstartK": _case((2, 128, 5, 3), 2.5, 16, "WIDE_CONC"),
    "replay_K128_kstart0": _case((2, 128, 5, 3), 2.5, 16, "WIDE_CONC", frame=SMALL, opts=NOFAST),
    # the concurrent adders' 24-row pipeline: under, at and off its multiples (K = 1, one cart of four leaves, keeps a quarter
    # of the windows at least: the small frame); 192 coordinates are the last that fit 256 threads, 194 fall to WIDE_SEQ
    "conc_K1": _case((2, 1, 9, 3), 1.1, 1, "WIDE_CONC", frame=SMALL),
    "conc_K23": _case((2, 23, 9, 3), 1.3, 5, "WIDE_CONC"),
    "conc_K24": _case((2, 24, 9, 3), 2.5, 5, "WIDE_CONC"),
    "conc_K25": _case((2, 25, 9, 3), 1.5, 5, "WIDE_CONC"),
    "conc_K47": _case((2, 47, 9, 3), 1.5, 5, "WIDE_CONC"),
    "conc_K48": _case((2, 48, 9, 3), 2.5, 5, "WIDE_CONC"),
    "conc_K49": _case((2, 49, 9, 3), 1.5, 5, "WIDE_CONC"),
    "conc_dim192": _case((2, 30, 96, 3), 1.3, 7, "WIDE_CONC"),
    "conc_dim194": _case((2, 30, 97, 3), 1.5, 7, "WIDE_SEQ"),
    # the sequential form's 12-row pipeline, chunked weight rows at the shipped dimensions, the 64-row floor of the tile search
    "seq_K11": _case((2, 11, 9, 3), 0.9, 5, "WIDE_SEQ", opts=SEQ),
    "seq_K12": _case((2, 12, 9, 3), 1.1, 5, "WIDE_SEQ", opts=SEQ),
    "seq_K13": _case((2, 13, 9, 3), 1.5, 5, "WIDE_SEQ", opts=SEQ),
    "seq_K25": _case((2, 25, 9, 3), 1.5, 5, "WIDE_SEQ", opts=SEQ),
    "seq_shipped": _case(S_DIMS, 1.5, 27, "WIDE_SEQ", opts=SEQ, frame=MID),
    "seq_rowcap64": _case((2, 70, 237, 3), 1.5, 7, "WIDE_SEQ", opts=SEQ, frame=MID),
    # wide shapes: 1,024 coordinates are the last finish_wide_ok accepts
    "dim1024": _case((2, 20, 512, 4), 1.5, 7, "WIDE_SEQ", frame=MID),
    "dim1026": _case((2, 20, 513, 4), 1.5, 7, "MERGED", frame=MID),
    # deep trees: 128 leaves share the leaf byte with the normalise flag; 256 are refused
    "leaf128": _case((2, 12, 5, 8), 1.5, 2, "WIDE_CONC"),
    "leaf256": _case((2, 12, 5, 9), 1.5, 2, "MERGED"),
    # windows on both sides of the LDS window tile (a frame has few windows of more than 200 pixels: the calls start at 100
    # pixels, so that a loose gate hands some of them off)
    "large_windows": _case((2, 70, 9, 4), 0.5, 7, "WIDE_CONC", frame=(1, 256, 256, 7), c_kw=dict(min_size=100),
                           cpp_kw=dict(minimum_size=100, step=6, factor=1.45)),
}


def _gates(m, z):
    """The cart thresholds of a case's model.  A constant threshold under a score that starts at zero rejects by the first
    few leaves and leaves hand-off counts that jump with every seed; here single carts reject, everything else passes:
      * the last cart the scan evaluates (cart min(K, handoff) - 1 of stage 0) keeps the scores z standard deviations up
        (leaf scores are N(0, 0.5^2)): the hand-off count,
      * where stage 0 goes on behind the hand-off, a cart half way to its end rejects inside k_finish_wide's stage 0,
      * the middle cart of stage 1 asks for a quarter of a standard deviation of the carts since then more: a good part of
        the survivors dies in a later stage."""
    from jda_amd import synth
    f32 = lambda v: float(np.float32(v))
    c0 = min(m.K, HANDOFF) - 1
    gate = f32(z * 0.5 * np.sqrt(c0 + 1.0))
    m.cth[:] = f32(synth.NEG_BIG)
    m.cth[0, c0] = gate
    if m.K - 1 > c0:
        m.cth[0, (c0 + m.K) // 2] = f32(0.9 * gate)
    if m.T > 1:
        m.cth[1, m.K // 2] = f32(gate + 0.125 * np.sqrt(m.K // 2 + 1.0))


@functools.lru_cache(maxsize=None)
def _inputs(name):
    """Model file, frames and the oracle's traces of a case: computed once, shared by the CPU and the GPU test."""
    import os
    import tempfile
    from jda_amd import synth
    from oracle import build as oracle_build
    from oracle.pyoracle import Oracle
    oracle_build.build_oracle()
    cs = CASES[name]
    T, K, L, D = cs["dims"]
    m = synth.make_model(T, K, L, D, seed=cs["seed"], norm_every=cs["norm_every"])
    if cs["norm_last"]:          # (values as make_model draws them: a mean of the order of 0.1, a deviation in [0.8, 1.25])
        m.cmean[:, K - 1] = float(np.float32(0.07)); m.cstd[:, K - 1] = float(np.float32(1.125))
    _gates(m, cs["z"])
    d = tempfile.mkdtemp(prefix="finish_forms_")
    atexit.register(shutil.rmtree, d, True)
    path = os.path.join(d, name + ".model")
    m.save(path, 8)
    n, w, h, seed = cs["frame"]
    frames = synth.make_frames(n, w, h, seed=seed)
    o = Oracle(path)
    tc = [o.trace(f, **cs["c_kw"]) for f in frames]
    tp = [o.trace_cpp(f, **cs["cpp_kw"]) for f in frames]
    win_c = np.tile(synth.window_table(w, h, **cs["c_kw"])[2], n)
    lv, _ = synth.levels_cpp(w, h, **cs["cpp_kw"])
    win_p = np.tile(np.concatenate([np.full(l["nx"] * l["ny"], l["win"]) for l in lv]), n)
    o.close()
    return dict(path=path, model=m, frames=frames, trace_c=tc, trace_cpp=tp, win_c=win_c, win_cpp=win_p)


def _conditions(name):
    """The numbers the conditions of a case are about, per dialect, from the oracle's trace."""
    cs, inp = CASES[name], _inputs(name)
    T, K, L, D = cs["dims"]
    out = {}
    for dial, tr, th in (("c", inp["trace_c"], np.float32(-0.5)), ("cpp", inp["trace_cpp"], None)):
        carts = np.concatenate([t["carts_n"] for t in tr])
        score = np.concatenate([t["score"] for t in tr])
        queued = np.ones(len(carts), bool) if cs["opts"].get("no_fast_scan") else carts > min(K, HANDOFF)
        # (a window rejected by the very last cart also counts T * K carts: its score is below that cart's threshold)
        walked = (carts == T * K) & (score >= inp["model"].cth[T - 1, K - 1])
        done = walked & (score >= th) if th is not None else walked
        out[dial] = dict(windows=len(carts), handoff=int(queued.sum()), faces=int(done.sum()),
                         late_rejects=int(((carts > K) & ~walked).sum()), queued=queued)
    return out


def _upper_leaf_under_the_flag(name, dial):
    """Per window: does a normalising cart of stage 1 end in a leaf of index 64 or more -- the leaf byte's 0x40 bit and
    the 0x80 flag set together?  Asked of the oracle with a probe model: the case's trees, weights and mean shape, so every
    window takes the paths it takes in the case (a stage's paths follow from the shape alone, c/jda.c:366-394), but nothing
    rejects, nothing normalises, and the only leaves that score are those in question, 1.0 each."""
    import os
    import tempfile
    from oracle.pyoracle import Oracle
    cs, inp = CASES[name], _inputs(name)
    m = copy.deepcopy(inp["model"])
    flagged = (m.cmean[1] != 0.0) | (m.cstd[1] != 1.0)
    m.leaf[:] = 0.0
    m.leaf[1, flagged, 64:] = 1.0
    m.cth[:] = float(np.float32(-3.0e38)); m.cmean[:] = 0.0; m.cstd[:] = 1.0
    d = tempfile.mkdtemp(prefix="finish_forms_")
    atexit.register(shutil.rmtree, d, True)
    path = os.path.join(d, "probe.model")
    m.save(path, 8)
    o = Oracle(path)
    tr = [o.trace(f, **cs["c_kw"]) if dial == "c" else o.trace_cpp(f, **cs["cpp_kw"]) for f in inp["frames"]]
    o.close()
    return np.concatenate([t["score"] for t in tr]) >= 1.0


def _check_conditions(name):
    cs, cond = CASES[name], _conditions(name)
    T, K, L, D = cs["dims"]
    for dial in ("c", "cpp"):
        c = cond[dial]
        print("%s %s: %d windows, hand-off %d, %d pass everything, %d rejected in a later stage" %
              (name, dial, c["windows"], c["handoff"], c["faces"], c["late_rejects"]))
        assert 1 <= c["handoff"] <= WIDE_MAX and c["handoff"] <= HANDOFF_MAX, (name, dial)
        assert c["faces"] >= 1, (name, dial)
        assert T < 2 or c["late_rejects"] >= 1, (name, dial)
    # a normalising cart in every block of 64 carts, the last, shorter one included -- read from the model itself
    m = _inputs(name)["model"]
    for t in range(T):
        normed = (m.cmean[t] != 0.0) | (m.cstd[t] != 1.0)
        assert all(normed[b:b + 64].any() for b in range(0, K, 64)), (name, t)
        if name.startswith("replay_") or name in ("block_K257", "block_K513", "block_K1025"):
            assert normed[K - 1], name
    return cond


# ---------------------------------------------------------------- CPU: the restatement and the inputs

def test_wide_lds_restatement_at_the_values_the_cases_rely_on():
    # shipped dimensions, sequential form: the rows do not fit the buffer at once in either dialect; fp32 leaves a last
    # chunk under the 12-row pipeline, fp64 takes three chunks
    f32, f64 = wide_launch(S_DIMS, 4, 0), wide_launch(S_DIMS, 8, 0)
    assert f32["row_cap"] < S_DIMS[1] and f64["row_cap"] < S_DIMS[1]
    assert len(f32["chunks"]) == 2 and f32["chunks"][-1] < 12
    assert len(f64["chunks"]) == 3
    assert f32["total"] <= LDS_BUDGET and f64["total"] <= LDS_BUDGET
    assert f32["block"] == 1024 and f32["form"] == "WIDE_SEQ" and wide_launch(S_DIMS, 4)["form"] == "WIDE_CONC"
    # the tile search's floor: exactly 64 rows, then a chunk of 6
    r = wide_launch(CASES["seq_rowcap64"]["dims"], 4, 0)
    assert r["row_cap"] == 64 and r["chunks"] == [64, 6] and r["tile_win"] > 0
    # block selection
    assert [wide_launch((2, K, 5, 3), 4)["block"] for K in (256, 257, 512, 513)] == [256, 512, 512, 1024]
    assert wide_launch((2, 1025, 2, 2), 4)["block"] == 1024
    # conc_ok at 256 threads: a wave for the replay and three for 192 coordinates, none left for 194
    assert wide_launch((2, 30, 96, 3), 4)["conc"] and not wide_launch((2, 30, 97, 3), 4)["conc"]
    assert wide_launch((2, 30, 96, 3), 8)["conc"] and not wide_launch((2, 30, 97, 3), 8)["conc"]
    # 1,024 coordinates: four accumulators a thread, BLOCK / dim = 0; fp64 has no room for a window tile and chunks its rows
    w32, w64 = wide_launch((2, 20, 512, 4), 4), wide_launch((2, 20, 512, 4), 8)
    assert w32["block"] == 256 and 4 * w32["block"] == 1024 and not w32["conc"]
    assert w64["tile_win"] == 0 and w64["row_cap"] < 20 and len(w64["chunks"]) > 1
    assert wide_launch((2, 20, 513, 4), 4) is None and wide_launch((2, 20, 513, 4), 8) is None
    # 128 leaves are the most the leaf byte holds next to the flag
    assert wide_launch((2, 12, 5, 8), 4) is not None and wide_launch((2, 12, 5, 9), 4) is None
    # the largest window tile: the 40 KB cap, not the row buffer, at small dimensions
    assert wide_launch((2, 70, 9, 4), 4)["tile_win"] == wide_launch((2, 70, 9, 4), 8)["tile_win"] == 200


def test_every_case_names_the_form_its_model_selects():
    for name, cs in CASES.items():
        for rb, key in ((4, "form"), (8, "form_cpp")):
            r = wide_launch(cs["dims"], rb, cs["opts"].get("wide_conc", 1))
            assert (r["form"] if r else "MERGED") == cs[key], (name, key)


@pytest.mark.parametrize("name", sorted(CASES))
def test_inputs_meet_their_conditions(name):
    cond = _check_conditions(name)
    cs, inp = CASES[name], _inputs(name)
    if name == "leaf128":
        for dial in ("c", "cpp"):
            hit = _upper_leaf_under_the_flag(name, dial) & cond[dial]["queued"]
            print("leaf128 %s: %d handed-off windows meet a leaf of index 64 or more in a normalising cart of stage 1" % (dial, int(hit.sum())))
            assert hit.sum() >= 1, dial
    if name == "large_windows":
        for dial, rb, win in (("c", 4, inp["win_c"]), ("cpp", 8, inp["win_cpp"])):
            tw = wide_launch(cs["dims"], rb)["tile_win"]
            q = cond[dial]["queued"]
            below, above = int((q & (win <= tw)).sum()), int((q & (win > tw)).sum())
            print("large_windows %s: tile_win %d, %d handed off at or below it, %d above" % (dial, tw, below, above))
            assert below >= 1 and above >= 1, dial


# ---------------------------------------------------------------- GPU

@pytest.fixture(scope="module")
def gpu():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    return torch.device("cuda", 0)


def _forms(c, fn, *a, **kw):
    """-> (what the call returned, the forms its passes took: {form: count}, zero counts left out)."""
    before = c.finish_forms()
    r = fn(*a, **kw)
    after = c.finish_forms()
    assert all(after[k] >= before[k] for k in after)
    return r, {k: after[k] - before[k] for k in after if after[k] != before[k]}


def _same_trace(want_frames, got, what):
    off = 0
    for i, r in enumerate(want_frames):
        n = len(r["carts_n"])
        for k in ("carts_n", "score", "path_hash", "shapes"):
            assert same(r[k], got[k][off:off + n]), (what, i, k, int((bits(r[k]) != bits(got[k][off:off + n])).sum()))
        off += n
    assert off == len(got["carts_n"]), what


def _same_stats(a, b, what):
    for k in STAT_KEYS:
        assert a[k] == b[k], (what, k)
    assert list(a["stage_done_n"]) == list(b["stage_done_n"]), what


def _run_case(name):
    from jda_amd import api
    cs, inp = CASES[name], _inputs(name)
    cond = _check_conditions(name)
    frames = inp["frames"]
    under, wave = api.Cascador(inp["path"]), api.Cascador(inp["path"])
    for k, v in cs["opts"].items():
        under.set_option(k, v); wave.set_option(k, v)
    wave.set_option("wide_max", 0)
    assert under.get_option("wide_max") == WIDE_MAX and under.get_option("handoff") == HANDOFF
    try:
        # dialect C: trace against the oracle and the wave-per-window kernel, then detections and counters
        tu, fu = _forms(under, under.trace, frames, **cs["c_kw"])
        tv, fv = _forms(wave, wave.trace, frames, **cs["c_kw"])
        print(name, "trace:", fu, fv)
        assert fu == {cs["form"]: 1} and fv == {"MERGED": 1}, (name, fu, fv)
        _same_trace(inp["trace_c"], tu, "oracle")
        for k in tu:
            assert same(tu[k], tv[k]), (name, k)
        for rep in range(2):            # (the second call is sized from the first one's hand-off: the same form)
            (du, su), fu = _forms(under, under.detect_batch, frames, stats=True, **cs["c_kw"])
            (dv, sv), fv = _forms(wave, wave.detect_batch, frames, stats=True, **cs["c_kw"])
            print(name, "detect:", fu, fv)
            assert fu == {cs["form"]: 1} and fv == {"MERGED": 1}, (name, rep, fu, fv)
            for a, b in zip(du, dv):
                for k in ("bboxes", "scores", "shapes"):
                    assert same(a[k], b[k]), (name, k)
            _same_stats(su, sv, name)
            assert su["handoff_n"] == cond["c"]["handoff"] and su["face_patch_n"] >= cond["c"]["faces"] >= 1, name
        # dialect CPP
        kw = cs["cpp_kw"]
        tu, fu = _forms(under, under.trace_cpp, frames, **kw)
        tv, fv = _forms(wave, wave.trace_cpp, frames, **kw)
        print(name, "trace_cpp:", fu, fv)
        assert fu == {cs["form_cpp"]: 1} and fv == {"MERGED": 1}, (name, fu, fv)
        _same_trace(inp["trace_cpp"], tu, "cpp oracle")
        for k in tu:
            assert same(tu[k], tv[k]), (name, "cpp", k)
        (du, su), fu = _forms(under, under.detect_batch_cpp, frames, stats=True, **kw)
        (dv, sv), fv = _forms(wave, wave.detect_batch_cpp, frames, stats=True, **kw)
        print(name, "detect_cpp:", fu, fv)
        assert fu == {cs["form_cpp"]: 1} and fv == {"MERGED": 1}, (name, fu, fv)
        for a, b in zip(du, dv):
            for k in ("rects", "scores", "shapes"):
                assert same(a[k], b[k]), (name, "cpp", k)
        _same_stats(su, sv, name + " cpp")
        assert su["handoff_n"] == cond["cpp"]["handoff"], name
    finally:
        under.close(); wave.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(CASES))
def test_form_under_test_vs_oracle_and_wave_finish(built, gpu, name):
    _run_case(name)


# ---------------------------------------------------------------- the other forms, at the smallest job that selects them

@functools.lru_cache(maxsize=None)
def _long_handoff():
    """Three 320 x 240 frames under a loose threshold: more than finish_merge windows reach the hand-off queue."""
    import os
    import tempfile
    from jda_amd import synth
    from oracle import build as oracle_build
    from oracle.pyoracle import Oracle
    oracle_build.build_oracle()
    dims = (2, 20, 5, 3)
    m = synth.make_model(*dims, seed=5, cart_th=-1.0, norm_every=7)
    d = tempfile.mkdtemp(prefix="finish_forms_")
    atexit.register(shutil.rmtree, d, True)
    path = os.path.join(d, "long.model")
    m.save(path, 8)
    frames = synth.make_frames(3, 320, 240, seed=7)
    o = Oracle(path)
    tr = [o.trace(f) for f in frames]
    o.close()
    return dict(dims=dims, path=path, frames=frames, trace=tr)


def _long_conditions():
    inp = _long_handoff()
    T, K = inp["dims"][:2]
    carts = np.concatenate([t["carts_n"] for t in inp["trace"]])
    handoff, late, full = int((carts > K).sum()), int(((carts > K) & (carts < T * K)).sum()), int((carts == T * K).sum())
    print("long hand-off: %d windows, %d handed off, %d rejected in stage 1, %d walk everything" % (len(carts), handoff, late, full))
    assert handoff > FINISH_MERGE and late >= 1 and full >= 1
    return handoff


def test_long_handoff_inputs_meet_their_conditions():
    _long_conditions()


@pytest.mark.gpu
@pytest.mark.parametrize("form,opts", [("MERGED", dict()), ("FILTER0", dict(filter0=1)), ("TWO_LAUNCH", dict(filter0=0))])
def test_k_finish_forms_vs_oracle(built, gpu, form, opts):
    """One k_finish launch for a short hand-off queue; k_filter0 + k_finish(survivors), or stage 0 and the rest in two
    launches, for a long one -- each against the oracle with its count asserted, twice (the second pass is sized from the
    first).  MID_DIRECT needs the persistent scan up to cart K: test_mid_direct_vs_oracle below."""
    from jda_amd import api
    inp = _long_handoff()
    handoff = _long_conditions()
    frames, want = (inp["frames"][:1], inp["trace"][:1]) if form == "MERGED" else (inp["frames"], inp["trace"])
    if form == "MERGED":
        K = inp["dims"][1]
        assert WIDE_MAX < int((want[0]["carts_n"] > K).sum()) * 1.1 + 64 <= FINISH_MERGE
    c = api.Cascador(inp["path"])
    c.set_option("dense", 0); c.set_option("wide_max", 0)
    for k, v in opts.items():
        c.set_option(k, v)
    # the launches behind the form (jdaFinishLaunches; tests/test_finish_launches.py): K = 20 walks two 64-cart groups a round,
    # stage 0 of TWO_LAUNCH one and without the window tile; the leaves of four-leaf trees fit the carry
    FL = api.FinishLaunch
    launches = lambda tr: {"MERGED": {FL("k_finish", "C", tr, 2, False, False, False, False, False, True): 1},
                           "FILTER0": {FL("k_filter0", "C", tr, 0, False, False, False, False, True, False): 1,
                                       FL("k_finish", "C", tr, 2, False, False, False, True, True, True): 1},
                           "TWO_LAUNCH": {FL("k_finish", "C", tr, 1, False, False, False, False, False, False): 1,
                                          FL("k_finish", "C", tr, 2, False, False, False, False, False, True): 1}}[form]
    try:
        for rep in range(2):
            before = c.finish_launches()
            got, f = _forms(c, c.trace, frames)
            fl = {k: v - before.get(k, 0) for k, v in c.finish_launches().items() if v != before.get(k, 0)}
            print(form, "pass", rep, f, sorted(fl.items()))
            assert f == {form: 1} and fl == launches(True), (rep, f, fl)
            _same_trace(want, got, form)
        before = c.finish_launches()
        (d, st), f = _forms(c, c.detect_batch, frames, stats=True)
        fl = {k: v - before.get(k, 0) for k, v in c.finish_launches().items() if v != before.get(k, 0)}
        assert f == {form: 1} and fl == launches(False), (f, fl)
        assert form == "MERGED" or st["handoff_n"] == handoff
    finally:
        c.close()


# ---------------------------------------------------------------- MID_DIRECT: the persistent scan fills the mid queue itself

# (the options of tests/test_scan_persistent.py's variant with its own hand-off: a launch per level, k_scan_p wherever it
# fits, all of stage 0 inside it -- its survivors then go to the mid queue, Pass::scan_persistent: cfg.to_mid)
MID_ENV = {"JDA_MERGE_BLOCKS": "0", "JDA_SCAN_P": "2", "JDA_SCAN_P_HANDOFF": "100000", "JDA_SCAN_P_B2": "128", "JDA_SCAN_P_B3": "256",
           "JDA_SCAN_P_LG": "64478"}
MID_DIMS = (3, 20, 5, 4)


def _cascador_under(path, env):
    import os
    from jda_amd import api
    old = dict(os.environ)
    os.environ.update(env)
    try:
        return api.Cascador(path)          # (the JDA_* environment is read here)
    finally:
        os.environ.clear(); os.environ.update(old)


@functools.lru_cache(maxsize=None)
def _mid_direct_inputs():
    import os
    import tempfile
    from jda_amd import synth
    from oracle import build as oracle_build
    from oracle.pyoracle import Oracle
    oracle_build.build_oracle()
    m = synth.make_model(*MID_DIMS, seed=3, cart_th=-1.0, norm_every=5)
    d = tempfile.mkdtemp(prefix="finish_forms_")
    atexit.register(shutil.rmtree, d, True)
    path = os.path.join(d, "mid.model")
    m.save(path, 8)
    frames = synth.make_frames(3, 200, 150, seed=11)
    o = Oracle(path)
    out = dict(path=path, frames=frames, trace=[o.trace(f) for f in frames],
               raw=[o.detect(f, nms=False) for f in frames], post=[o.detect(f) for f in frames])
    o.close()
    # (the reference relocates shapes to the frame after NMS only, c/jda.c:465-474; the library's lists without NMS are
    # relocated too: the same multiply, then add, on the oracle's rows -- as tests/test_gpu_parity.py does for the golden vectors)
    for r in out["raw"]:
        x, y, sz = (r["bboxes"][:, j].astype(np.float32)[:, None] for j in range(3))
        r["shapes"][:, 0::2] = r["shapes"][:, 0::2] * sz + x
        r["shapes"][:, 1::2] = r["shapes"][:, 1::2] * sz + y
    return out


def _mid_direct_conditions():
    """MID_DIRECT is the first branch of Pass::launch_finishers: it is taken whenever a k_scan_p launch filled the mid queue,
    whatever the length of the hand-off queue -- so the smallest job is a few small frames, and what has to hold is that
    BOTH queues feed k_finish(survivors): stage-0 survivors on the LDS-tiled levels (k_scan_p's, straight to the mid queue)
    and on the global-pixel levels (k_scan -> hand-off queue -> k_filter0), a reject in a later stage, and a face."""
    inp = _mid_direct_inputs()
    T, K = MID_DIMS[:2]
    c = _cascador_under(inp["path"], MID_ENV)
    assert c.get_option("scan_p") == 2 and c.get_option("scan_p_mid") == 1 and c.get_option("filter0") == 1
    mode = np.tile(np.concatenate([np.full(l["nx"] * l["ny"], l["mode"]) for l in c.plan_tiles(200, 150)]), len(inp["frames"]))
    c.close()
    carts = np.concatenate([t["carts_n"] for t in inp["trace"]])
    assert len(mode) == len(carts)
    lds, glb = int(((carts > K) & (mode == 1)).sum()), int(((carts > K) & (mode == 2)).sum())
    late, faces = int(((carts > K) & (carts < T * K)).sum()), sum(len(r["scores"]) for r in inp["raw"])
    print("mid_direct: %d windows, stage-0 survivors: %d on LDS-tiled levels, %d on global-pixel levels; %d rejected later, %d faces"
          % (len(carts), lds, glb, late, faces))
    assert (mode != 0).all() and lds >= 1 and glb >= 1 and late >= 1 and faces >= 1
    return carts


def test_mid_direct_inputs_meet_their_conditions(built):
    _mid_direct_conditions()


@pytest.mark.gpu
def test_mid_direct_vs_oracle(built, gpu):
    """k_filter0 + k_finish(survivors) fed from the mid queue k_scan_p filled: {MID_DIRECT: 1} on both passes (the second
    sized from the first).  The persistent scan declines a traced pass (Pass::scan_persistent), so no per-window trace can
    come from this form; what it computes is tied to the oracle on EVERY frame through everything a detect call returns:
    every window that passes, before NMS, with its score and shape bits (and so, by their absence, every reject), the
    detections after NMS, and the counters -- candidate windows, faces, the carts evaluated over all windows (the sum of
    the oracle's carts_n) and the windows that completed each stage -- also against a cascador without k_scan_p."""
    import torch
    inp = _mid_direct_inputs()
    carts = _mid_direct_conditions()
    T, K = MID_DIMS[:2]
    dev = torch.from_numpy(inp["frames"]).to(gpu)
    under = _cascador_under(inp["path"], MID_ENV)
    plain = _cascador_under(inp["path"], {"JDA_MERGE_BLOCKS": "0", "JDA_SCAN_P": "0"})
    for c in (under, plain):
        c.set_option("dense", 0); c.set_option("wide_max", 0)
    try:
        (want, st0), f0 = _forms(plain, plain.detect_batch_device, dev, nms=False, stats=True)
        assert f0 and "MID_DIRECT" not in f0 and not set(f0) & {"WIDE_CONC", "WIDE_SEQ", "DENSE"}, f0
        for rep in range(2):
            (raw, st), f = _forms(under, under.detect_batch_device, dev, nms=False, stats=True)
            print("mid_direct pass", rep, f, "scan carts", st["scan_cart_n"], "without k_scan_p", st0["scan_cart_n"])
            assert f == {"MID_DIRECT": 1}, (rep, f)
            post, fp = _forms(under, under.detect_batch_device, dev)
            assert fp == {"MID_DIRECT": 1}, (rep, fp)
            for i in range(len(inp["frames"])):
                for k in ("bboxes", "scores", "shapes"):
                    assert same(inp["raw"][i][k], raw[i][k]), (rep, i, k)
                    assert same(inp["post"][i][k], post[i][k]), (rep, i, "nms", k)
                    assert same(want[i][k], raw[i][k]), (rep, i, "k_scan", k)
            assert st["scan_fallbacks"] == 0 and st["dense_passes"] == 0 and st["ws_regrows"] == 0
            # (K <= handoff: either scan evaluates all of stage 0 and nothing else -- the oracle's carts up to cart K)
            assert st["scan_cart_n"] == st0["scan_cart_n"] == int(np.minimum(carts, K).sum())
            assert st["patch_n"] == len(carts) and st["face_patch_n"] == sum(len(r["scores"]) for r in inp["raw"])
            assert st["cart_total_n"] == int(carts.sum()) == st0["cart_total_n"]
            for t in range(T - 1):
                assert st["stage_done_n"][t] == int((carts > (t + 1) * K).sum()) == st0["stage_done_n"][t], t
            assert st["stage_done_n"][T - 1] == st0["stage_done_n"][T - 1]
    finally:
        under.close(); plain.close()
