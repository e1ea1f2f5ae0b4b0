"""Which k_finish / k_filter0 instantiations a pass launched (jdaFinishLaunches, include/jda.h), and
the two kernels at the limits of their own loops.

Every case names the launches it is about -- the FinishLaunch keys (kernel, dialect, trace, groups, multi, st, stream,
survivors, carry, tile) -- reads the difference of the cascador's counts around EACH call, prints it and asserts it, next to
the finishing form (jdaFinishForms).  What a case compares, bit for bit (`same`), in dialect C and in dialect CPP:

  * trace() / trace_cpp(), the TRACE instantiations: carts walked, score, leaf-path hash and shape per window against the
    CPU oracle (dialect C: c/jda.c:357-426; dialect CPP: the repository's restatement),
  * detect_batch() / detect_batch_cpp(), the instantiations without trace: detections against the oracle's,
  * the work counters cart_total_n, handoff_n, stage_done_n, face_patch_n against what the oracle's trace says they are.

Every cascador runs with dense = 0 and wide_max = 0: no dense mode, no whole-workgroup finisher.

The inputs of a case must make it mean something.  Its conditions are evaluated on the CPU from the oracle's trace
(test_inputs_meet_their_conditions, no GPU needed) and again by the GPU case; a case whose condition fails FAILS:
  * the hand-off queue is not empty and on the right side of finish_merge = 4,096 for the form,
  * a window passes every stage and the final threshold, a window dies in a stage >= 1,
  * a normalising cart falls in every block of 64 carts,
  * and what the case adds (CASES below).

The gate carts (_gates) are placed per case and their thresholds are read from the oracle: a gate cart is made to reject
everybody, the oracle reports the score every window has there, and the threshold is the score that keeps the wanted
share.  So the oracle alone decides the inputs before anything runs on a GPU.

Restated here from the host code: Pass::stage_groups (pass.cpp), finish_tile_win and its LDS sum (kernels.h),
carry_fits (kernels.h), DevModelT::w_stream and the padded row pitch (model_dev.cpp)."""
import atexit
import functools
import os
import shutil

import numpy as np
import pytest

from conftest import same, bits

HANDOFF = 128               # option `handoff`
FINISH_MERGE = 4096         # host.h: Knobs::finish_merge
LDS_PER_GROUP = 7680        # kernels.h: kFinishLdsPerGroup
MAX_STAGES = 16             # kernels.h: kMaxStages
CAP_L = 1 << 16             # kernels.h: kCarryCapMax


# ---------------------------------------------------------------- the host's decisions restated

def stage_groups(K):
    """pass.cpp: Pass::stage_groups -- the count in 4, 3, 2 that wastes the fewest walks past cart K - 1 (ties: the larger)."""
    best, best_waste = 4, 1 << 30
    for g in (4, 3, 2):
        per = 64 * g
        waste = -(-K // per) * per - K
        if waste < best_waste:
            best, best_waste = g, waste
    return best


def lds_base(dim, K, rb, st):
    dim_pad = (dim + 1) & ~1
    return dim_pad * rb + ((K + 3) & ~3) * 4 + MAX_STAGES * 4 + ((2 * dim_pad + 8) * rb if st else 0)


def tile_win(dims, rb, st=False, multi=False):
    """kernels.h: finish_tile_win with tile_win = -1."""
    T, K, L, D = dims
    if multi:
        return 0
    base, best = lds_base(2 * L, K, rb, st), 0
    for tw in range(16, 256):
        if base + tw * ((tw + 3) & ~3) + 16 <= LDS_PER_GROUP:
            best = tw
    return best


def carry_fits(dims):
    T, K, L, D = dims
    b = 0
    while (1 << b) < (1 << (D - 1)):
        b += 1
    return b * ((K + 63) // 64) <= 32


def carry_bits_rounds(dims):
    T, K, L, D = dims
    return D - 1, (K + 63) // 64


def w_stream(dims, rb, mb):
    """model_dev.cpp: rows padded to 128-byte lines where that changes the pitch; w_stream where a stage's rows exceed mb MB."""
    T, K, L, D = dims
    dim, leaf_n, line = 2 * L, 1 << (D - 1), 128 // rb
    pitch = -(-dim // line) * line
    if pitch == dim or K * leaf_n * pitch >= 1 << 32:
        pitch = dim
    return mb > 0 and K * leaf_n * pitch * rb > mb << 20


# ---------------------------------------------------------------- the cases

SMALL = dict(n=1, w=166, h=118, seed=7)               # dialect C: the 46-pixel level alone, 31 x 19 windows
LONG = dict(n=3, w=320, h=240, seed=7)                # the frames of test_finish_forms._long_handoff
C_LEVEL = dict(scale=1.25, min_size=40, max_size=50)
CPP_LEVEL = dict(minimum_size=46, step=4, factor=4.0)
C_ALL = dict()
CPP_ALL = dict(minimum_size=40, step=4, factor=1.25)


def _case(dims, form, keep=None, frame=None, c_kw=None, cpp_kw=None, opts=None, env=None, norm_every=31, seed=5, gate0=None,
          mid_gate=True, st=False, multi=False, cpp=True, cond=(), calls=None, first=None, handoff=HANDOFF, stage1_q=0.2):
    """dims (T, K, L, D); form: the finishing form every call must count; keep: windows the hand-off gate keeps (dialect C,
    over the frames of the first call); opts: options set on the cascador; env: JDA_* it is created under; gate0: the
    hand-off gate's cart where it is not cart min(K, handoff) - 1; st: dialect CPP runs under the similarity transform;
    multi: a multi-scale model (dialect C only: the oracle's dialect CPP has none); cond: names of the extra conditions;
    calls: per dialect a list of (frame, kw) where one call does not do; first: a frame set called BEFORE the case's own on
    the same plan."""
    long_form = form != "MERGED"
    frame = frame or (LONG if long_form else SMALL)
    c_kw = dict(c_kw if c_kw is not None else (C_ALL if long_form else C_LEVEL))
    cpp_kw = dict(cpp_kw if cpp_kw is not None else (CPP_ALL if long_form else CPP_LEVEL))
    keep = keep or (6001 if long_form else 301)
    calls = calls or dict(C=[(frame, c_kw)], CPP=[(frame, cpp_kw)])
    return dict(dims=dims, form=form, keep=keep, calls=calls, opts=dict(opts or {}), env=dict(env or {}), norm_every=norm_every,
                seed=seed, gate0=gate0, mid_gate=mid_gate, st=st, multi=multi, cpp=cpp and not multi, cond=tuple(cond), first=first,
                handoff=handoff, stage1_q=stage1_q)


def _level_calls(dims, st=False):
    """Window-tile cases: per dialect the calls whose plans hold a level of exactly tile_win pixels and one of tile_win + 1
    (tile_win = 0: 46 and 47), every level with a window in the frame's last row and last column.  Dialect C grows its
    windows from 24 pixels by int(win * scale): one step reaches any size, two neighbouring sizes never share a plan, so each
    level is a call of its own on its own frame; dialect CPP starts at minimum_size and grows by int(win * factor): with a
    step of one pixel a frame eight pixels wider than tile_win holds the levels tile_win .. tile_win + 6."""
    out = dict(C=[], CPP=[])
    tw = tile_win(dims, 4) or 46
    for win in (tw, tw + 1):
        step = int(np.float32(win) * np.float32(0.1))
        scale = float(np.float32((win + 0.5) / 24.0))
        assert int(np.float32(24) * np.float32(scale)) == win          # (the next size lies far beyond max_size = win)
        out["C"].append((dict(n=1, w=win + 11 * step, h=win + 7 * step, seed=7), dict(scale=scale, min_size=win, max_size=win)))
    tw = tile_win(dims, 8, st) or 46
    out["CPP"].append((dict(n=1, w=tw + 10, h=tw + 6, seed=7), dict(minimum_size=tw, step=1, factor=(tw + 1.5) / tw)))
    return out


CASES = {}
# ---- 1. the regression's row batch (64 rows in fp32, 32 in fp64) and its scalar tail: K at RB - 1, RB, RB + 1, 2 RB, 2 RB + 1
for _K in (31, 32, 33, 63, 64, 65, 127, 128, 129):
    CASES["rows_K%d" % _K] = _case((2, _K, 5, 3), "MERGED", norm_every=min(31, _K), cond=("last_row",))
# ---- 2. cart groups: kG = 3 with a partial and an empty group, kG = 4, two rounds; kG = 1 as stage 0 of TWO_LAUNCH
for _K in (192, 129, 256, 193, 385, 257):
    CASES["groups_K%d" % _K] = _case((2, _K, 5, 3), "MERGED", cond=("groups",), stage1_q=0.12)
CASES["groups_two_launch_K65"] = _case((2, 65, 5, 3), "TWO_LAUNCH", opts=dict(filter0=0), cond=("groups",))
# ---- 3. shape coordinates around 64 lanes, dialect CPP's lane pairing; the similarity transform's scratch behind dim_pad
for _L in (1, 31, 32, 33, 64, 65):
    CASES["shape_L%d" % _L] = _case((2, 20, _L, 3), "MERGED", norm_every=7)
for _L in (33, 65):
    CASES["shape_L%d_st" % _L] = _case((2, 20, _L, 3), "MERGED", norm_every=7, st=True)
# ---- 4. the LDS window tile: windows of exactly tile_win and tile_win + 1 pixels; no room for a tile; a multi-scale model
TILE_DIMS = {"tile_mult4": (2, 1040, 5, 2), "tile_odd": (2, 1000, 5, 2), "tile_none": (2, 1900, 5, 2)}
for _n, _d in TILE_DIMS.items():
    CASES[_n] = _case(_d, "MERGED", calls=_level_calls(_d), keep=40, cond=("tile",), stage1_q=0.1, seed=6 if _n == "tile_mult4" else 5)
CASES["tile_multi_K192"] = _case((2, 192, 5, 3), "MERGED", multi=True, cond=("groups",), stage1_q=0.12)
# ---- 5. the carry at the edge of its word: 32 bits used (bit 31 set by a leaf), 30 bits, and one cart more than fits
CARRY = {(3, 1024): 1, (3, 1025): 0, (5, 512): 1, (5, 513): 0, (9, 256): 1, (9, 257): 0, (4, 640): 1, (4, 641): 0}
for (_D, _K), _c in CARRY.items():
    CASES["carry_D%d_K%d" % (_D, _K)] = _case((2, _K, 2 if _D == 9 else 5, _D), "FILTER0", cond=("carry",) if _c else ())
# ---- 6. the hand-off position inside a round of 64 carts (m_k0 = kbeg & ~63; the re-walk of the scored carts)
for _H in (1, 63, 64, 65, 128, 192):
    CASES["handoff_%d" % _H] = _case((2, 200, 5, 4), "FILTER0", gate0=40, handoff=_H, opts=dict(handoff=_H))
# ---- 7. K <= hand-off: k_filter0 walks nothing and writes m_k0 = K, k_finish(survivors) walks all of stage 0 itself
for _K in (63, 64, 100, 128):
    CASES["sentinel_K%d" % _K] = _case((2, _K, 5, 3), "FILTER0", cond=("sentinel",))
# ---- 8. more stage-0 survivors than leaf words (cap_l = 65,536): carried and sentinel entries in one launch
CASES["cap_l"] = _case((2, 129, 1, 3), "FILTER0", frame=dict(n=12, w=320, h=240, seed=7), keep=68001, handoff=16, opts=dict(handoff=16),
                       mid_gate=False, cpp_kw=dict(minimum_size=40, step=3, factor=1.25), cond=("cap_l",), stage1_q=0.1)
# ---- 9. k_filter0 at every depth class (D = 4: the seven-records-up-front walk), an odd queue, a launch sized short
for _D in (2, 3, 4, 5, 6):
    CASES["filter0_D%d" % _D] = _case((2, 70, 5, _D), "FILTER0", handoff=16, opts=dict(handoff=16), keep=7501, cond=("odd",),
                                      first=dict(n=3, w=320, h=240, seed=7, blank=(2,)))
# ---- 10. STREAM: the smallest models whose stage rows exceed 1 MB at kG = 2, 3, 4, K off the row batch
for _K, _D in ((70, 8), (130, 7), (200, 7)):
    CASES["stream_kG%d" % stage_groups(_K)] = _case((2, _K, 5, _D), "MERGED", env={"JDA_W_STREAM_MB": "1"}, cond=("stream",))


def _frames(fr):
    from jda_amd import synth
    f = synth.make_frames(fr["n"], fr["w"], fr["h"], seed=fr["seed"])
    yy, xx = np.mgrid[0:fr["h"], 0:fr["w"]]
    for i in fr.get("blank", ()):
        # a frame without texture -- flat, or a ramp along x or y: every window of it takes the same paths, all pass or all fail
        f[i] = {"flat": 128, "ramp_x": xx * 255 // (fr["w"] - 1), "ramp_y": yy * 255 // (fr["h"] - 1),
                "ramp_x_down": 255 - xx * 255 // (fr["w"] - 1), "ramp_y_down": 255 - yy * 255 // (fr["h"] - 1)}[fr["kind"]]
    return f


def _trace_all(o, dial, frames, kw, want_shapes=True):
    if dial == "C":
        return [o.trace(f, want_shapes=want_shapes, **kw) for f in frames]
    return [o.trace_cpp(f, **kw) for f in frames]


def _gates(name, m, path):
    """The gate carts of a case, in walk order; the threshold of each is read from the oracle (dialect C, the first call's
    frames) with the earlier gates in force:
      * the hand-off gate -- cart min(K, handoff) - 1 of stage 0, or gate0 -- keeps the `keep` best windows: the hand-off count,
      * where stage 0 goes on behind it, a cart half way to the stage's end rejects a quarter inside k_filter0 / k_finish,
      * in stage 1, the middle cart of every 64-cart block of the first round and of the first block of the second round
        (the last cart where the block is shorter) rejects a share of those that reach it: a reject in every group index."""
    from oracle.pyoracle import Oracle
    from jda_amd import synth
    cs = CASES[name]
    T, K, L, D = cs["dims"]
    fr, kw = cs["calls"]["C"][0]
    frames = _frames(fr)
    m.cth[:] = float(np.float32(synth.NEG_BIG))
    c0 = cs["gate0"] if cs["gate0"] is not None else min(K, cs["handoff"]) - 1
    gates = [(0, c0, None)]
    if cs["mid_gate"] and K - 1 > c0 + 1:
        gates.append((0, (c0 + K) // 2, 0.25))
    kG = stage_groups(K)
    for b in range(min(kG + 1, (K + 63) // 64)):
        gates.append((1, min(64 * b + 32, K - 1), cs["stage1_q"]))
    for t, k, q in gates:
        m.cth[t, k] = 1e30
        m.save(path, 8)
        o = Oracle(path)
        tr = _trace_all(o, "C", frames, kw, want_shapes=False)
        o.close()
        carts, score = np.concatenate([x["carts_n"] for x in tr]), np.concatenate([x["score"] for x in tr])
        sc = np.sort(score[carts == t * K + k + 1])[::-1]           # the scores of the windows that reach the gate, best first
        n_keep = min(cs["keep"], len(sc) - 1) if q is None else int(len(sc) * (1 - q))
        assert 1 <= n_keep < len(sc), (name, t, k, len(sc))
        while n_keep > 1 and sc[n_keep - 1] == sc[n_keep]:          # (a tie: both sides of the threshold must differ)
            n_keep -= 1
        m.cth[t, k] = float(np.float32((float(sc[n_keep - 1]) + float(sc[n_keep])) / 2))
        if not sc[n_keep - 1] >= m.cth[t, k] > sc[n_keep]:
            m.cth[t, k] = float(sc[n_keep - 1])
    m.save(path, 8)


@functools.lru_cache(maxsize=None)
def _inputs(name):
    """Model file, frames and the oracle's traces and detections of a case: computed once, shared by the CPU and the GPU test."""
    import tempfile
    from jda_amd import synth
    from oracle import build as oracle_build
    from oracle.pyoracle import Oracle
    oracle_build.build_oracle()
    cs = CASES[name]
    T, K, L, D = cs["dims"]
    m = synth.make_model(T, K, L, D, seed=cs["seed"], norm_every=cs["norm_every"], multi_scale=cs["multi"])
    # (values as make_model draws them) the last cart of every stage normalises too: the last, shorter block of 64 has one
    m.cmean[:, K - 1] = float(np.float32(0.07)); m.cstd[:, K - 1] = float(np.float32(1.125))
    d = tempfile.mkdtemp(prefix="finish_launches_")
    atexit.register(shutil.rmtree, d, True)
    path = os.path.join(d, name + ".model")
    _gates(name, m, path)
    o = Oracle(path)
    out = dict(path=path, model=m, C=[], CPP=[])
    try:
        for dial in ("C", "CPP") if cs["cpp"] else ("C",):
            if dial == "CPP":
                o.set_similarity_transform(cs["st"])
            sets = [(fr, kw) for fr, kw in cs["calls"][dial]]
            if cs["first"]:
                sets = _pick_first(name, o, dial, sets[0])
            for fr, kw in sets:
                frames = _frames(fr)
                tr = _trace_all(o, dial, frames, kw)
                det = [o.detect(f, **kw) if dial == "C" else o.detect_cpp(f, **kw) for f in frames]
                if dial == "C":
                    win = np.tile(synth.window_table(fr["w"], fr["h"], **kw)[2], fr["n"])
                else:
                    lv, _ = synth.levels_cpp(fr["w"], fr["h"], **kw)
                    win = np.tile(np.concatenate([np.full(l["nx"] * l["ny"], l["win"]) for l in lv]), fr["n"])
                out[dial].append(dict(frames=frames, kw=kw, trace=tr, det=det, win=win, fr=fr))
    finally:
        o.set_similarity_transform(False)
        o.close()
    return out


def _pick_first(name, o, dial, main):
    """The job of an `odd` case, chosen with the oracle: the call in front -- the case's frames with the last one replaced by a
    frame without texture -- hands off a smaller share of its windows, yet more than finish_merge; dialect CPP's smallest
    window is moved until the hand-off count of the case's own call is odd, as dialect C's is by the gate's `keep`."""
    cs = CASES[name]
    K, H = cs["dims"][1], min(cs["dims"][1], cs["handoff"])
    fr, kw = main
    count = lambda f, k: sum(int((t["carts_n"] > H).sum()) for t in _trace_all(o, dial, _frames(f), k, want_shapes=dial != "C"))
    for ms in range(40, 48) if dial == "CPP" else (None,):
        kw2 = dict(kw, minimum_size=ms) if ms else kw
        n_main = count(fr, kw2)
        if n_main % 2 == 0:
            continue
        for kind in ("flat", "ramp_x", "ramp_y", "ramp_x_down", "ramp_y_down"):
            first = dict(cs["first"], kind=kind)
            n_first = count(first, kw2)
            if FINISH_MERGE < n_first and n_first * 1.1 + 64 < n_main:
                return [(first, kw2), (fr, kw2)]
    raise AssertionError((name, dial, "no job with an odd hand-off count behind a smaller one"))


def _numbers(name, dial, call):
    """What the conditions and the counters are about, from the oracle's trace of one call."""
    cs, m = CASES[name], _inputs(name)["model"]
    T, K, L, D = cs["dims"]
    H = 0 if cs["multi"] else min(K, cs["handoff"])     # (a multi-scale model has no stage-0 scan: every window is queued at cart 0)
    carts = np.concatenate([t["carts_n"] for t in call["trace"]])
    score = np.concatenate([t["score"] for t in call["trace"]])
    walked = (carts == T * K) & (score >= m.cth[T - 1, K - 1])      # (a reject by the very last cart also counts T * K carts)
    faces = walked & (score >= np.float32(-0.5)) if dial == "C" else walked
    done = [int((carts > (t + 1) * K).sum()) for t in range(T - 1)] + [int(walked.sum())]
    return dict(carts=carts, windows=len(carts), handoff=int((carts > H).sum()), total=int(carts.sum()), done=done, faces=int(faces.sum()),
                late=int(((carts > K) & ~walked).sum()), walked=walked, win=call["win"])


def _check_conditions(name):
    cs, inp = CASES[name], _inputs(name)
    T, K, L, D = cs["dims"]
    m = inp["model"]
    for t in range(T):
        normed = (m.cmean[t] != 0.0) | (m.cstd[t] != 1.0)
        assert all(normed[b:b + 64].any() for b in range(0, K, 64)), (name, t)
    kG = stage_groups(K)
    out = dict(C=[], CPP=[])
    for dial in ("C", "CPP") if cs["cpp"] else ("C",):
        rb = 4 if dial == "C" else 8
        for i, call in enumerate(inp[dial]):
            nb = _numbers(name, dial, call)
            out[dial].append(nb)
            print("%s %s call %d: %d windows, hand-off %d, stage-0 survivors %d, %d rejected in a later stage, %d pass everything" %
                  (name, dial, i, nb["windows"], nb["handoff"], nb["done"][0], nb["late"], nb["faces"]))
            if cs["first"] and i == 0:
                continue                      # (the call in front only has to take the same form: below)
            if cs["form"] == "MERGED":
                assert 1 <= nb["handoff"] and nb["handoff"] * 1.1 + 64 <= FINISH_MERGE, (name, dial, nb["handoff"])
            else:
                assert nb["handoff"] > FINISH_MERGE, (name, dial, nb["handoff"])
            assert nb["faces"] >= 1 and nb["late"] >= 1, (name, dial, nb["faces"], nb["late"])
            carts = nb["carts"]
            if "groups" in cs["cond"]:
                # a reject inside every 64-cart group of stage 1's first round, and in the second round where K has one
                for g in range(min(kG + 1, (K + 63) // 64)):
                    lo, hi = K + 64 * g, K + min(K, 64 * (g + 1))
                    n = int(((carts > lo) & (carts <= hi) & ~nb["walked"]).sum())
                    print("   stage 1, group %d (carts %d..%d): %d rejects" % (g, lo - K, hi - K - 1, n))
                    assert n >= 1, (name, dial, g)
            if "tile" in cs["cond"]:
                tw = tile_win(cs["dims"], rb, cs["st"] and dial == "CPP") or 46
                surv = carts > K
                at, above = int((surv & (nb["win"] == tw)).sum()), int((surv & (nb["win"] == tw + 1)).sum())
                print("   stage-0 survivors of %d pixels: %d, of %d pixels: %d" % (tw, at, tw + 1, above))
                if dial == "CPP":
                    assert at >= 1 and above >= 1, (name, dial)
                else:
                    assert (at if i == 0 else above) >= 1, (name, dial, i)
            if "cap_l" in cs["cond"]:
                assert nb["done"][0] > CAP_L and nb["done"][0] == nb["handoff"], (name, dial, nb["done"][0])
            if "odd" in cs["cond"]:
                assert nb["handoff"] % 2 == 1, (name, dial, nb["handoff"])
                # the call in front hands off fewer windows, yet enough for the same form: the second launch is sized short
                first = out[dial][0]
                assert FINISH_MERGE < first["handoff"] and first["handoff"] * 1.1 + 64 < nb["handoff"], (name, dial, first["handoff"], nb["handoff"])
            if "sentinel" in cs["cond"]:
                assert K <= cs["handoff"], name
    if "carry" in cs["cond"] or "last_row" in cs["cond"]:
        _check_leaves(name, out)
    if "stream" in cs["cond"]:
        assert w_stream(cs["dims"], 4, 1) and w_stream(cs["dims"], 8, 1) and K % 64 and K % 32, name
        # ... and the smallest depth that does: a level less stays under 1 MB
        assert not w_stream((T, K, L, D - 1), 4, 1), name
    return out


def _top_bit_in_last_round(name, dial, call):
    """Per window: does a cart of stage 0's LAST round of 64 end in a leaf whose top bit is set?  Asked of the oracle with a
    probe model: the case's trees and mean shape -- in stage 0 every window walks from the mean shape, so it takes the paths it
    takes in the case (c/jda.c:366-394) -- but nothing rejects, nothing normalises, and the only leaves that score are those
    in question, 1.0 each."""
    import copy
    import tempfile
    from oracle.pyoracle import Oracle
    cs, inp = CASES[name], _inputs(name)
    T, K, L, D = cs["dims"]
    m = copy.deepcopy(inp["model"])
    m.leaf[:] = 0.0
    m.leaf[0, 64 * ((K + 63) // 64 - 1):, m.leaf_n // 2:] = 1.0
    m.cth[:] = float(np.float32(-3.0e38)); m.cmean[:] = 0.0; m.cstd[:] = 1.0
    d = tempfile.mkdtemp(prefix="finish_launches_")
    atexit.register(shutil.rmtree, d, True)
    path = os.path.join(d, "probe.model")
    m.save(path, 8)
    o = Oracle(path)
    try:
        if dial == "CPP":
            o.set_similarity_transform(cs["st"])
        tr = _trace_all(o, dial, call["frames"], call["kw"], want_shapes=False)
    finally:
        o.set_similarity_transform(False)
        o.close()
    return np.concatenate([t["score"] for t in tr]) >= 1.0


def _check_leaves(name, out):
    """carry: a stage-0 survivor whose leaf in the LAST round of 64 carts has its top bit set -- the top bit the word uses,
    bit 31 where bits x rounds = 32.  last_row, read from the model alone: EVERY leaf of cart K - 1, in every stage, has a
    weight row that moves a coordinate by more than an fp32 ulp of a value in [0, 1) -- so whichever leaf a window that passes
    everything ends in there, a dropped tail row changes its shape bits (no window's own leaf is looked up)."""
    cs, inp = CASES[name], _inputs(name)
    T, K, L, D = cs["dims"]
    m = inp["model"]
    for dial in ("C", "CPP") if cs["cpp"] else ("C",):
        call, nb = inp[dial][-1], out[dial][-1]
        if "carry" in cs["cond"]:
            bits_, rounds = carry_bits_rounds(cs["dims"])
            assert carry_fits(cs["dims"]) and bits_ * (rounds + 1) > 32, name
            top = int((_top_bit_in_last_round(name, dial, call) & (nb["carts"] > K)).sum())
            print("   %s: %d stage-0 survivors set the top bit of the last round (bit %d of the word)" % (dial, top, bits_ * rounds - 1))
            assert top >= 1, (name, dial)
        if "last_row" in cs["cond"]:
            rows = m.w[:, (K - 1) * m.leaf_n:K * m.leaf_n]
            assert (np.abs(rows).max(axis=2) > 1e-6).all(), (name, dial)


def test_restatements_at_the_values_the_cases_rely_on():
    assert [stage_groups(K) for K in (20, 65, 128, 129, 192, 193, 256, 257, 385, 448, 540)] == [2, 2, 2, 3, 3, 4, 4, 3, 4, 4, 3]
    # (K = 448 = 7 x 64 wastes 64 walks with two groups and with four: the search keeps the larger)
    assert tile_win((5, 540, 27, 4), 4) == 72                           # the shipped model
    for dial_rb in (4, 8):
        tws = [tile_win(d, dial_rb) for d in TILE_DIMS.values()]
        assert tws[0] % 4 == 0 and tws[0] > 0 and tws[1] % 4 != 0 and tws[2] == 0, tws
    assert tile_win((2, 192, 5, 3), 4, multi=True) == 0
    assert tile_win((2, 20, 33, 3), 8, st=True) < tile_win((2, 20, 33, 3), 8)       # the transform's scratch takes from the tile
    assert [int(carry_fits((2, K, 5, D))) for (D, K) in CARRY] == list(CARRY.values())
    assert [b * r for b, r in (carry_bits_rounds((2, K, 5, D)) for (D, K) in CARRY)] == [32, 34, 32, 36, 32, 40, 30, 33]
    assert sorted(n for n in CASES if n.startswith("stream_")) == ["stream_kG2", "stream_kG3", "stream_kG4"]


@pytest.mark.parametrize("name", sorted(CASES))
def test_inputs_meet_their_conditions(built, name):
    _check_conditions(name)


# ---------------------------------------------------------------- GPU

@pytest.fixture(scope="module")
def gpu():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    return torch.device("cuda", 0)


def _launches(c, fn, *a, **kw):
    """-> (what the call returned, {FinishLaunch: count} and {form: count} of its passes)."""
    b_l, b_f = c.finish_launches(), c.finish_forms()
    r = fn(*a, **kw)
    a_l, a_f = c.finish_launches(), c.finish_forms()
    assert all(a_l.get(k, 0) >= v for k, v in b_l.items())
    return r, {k: v - b_l.get(k, 0) for k, v in a_l.items() if v != b_l.get(k, 0)}, {k: a_f[k] - b_f[k] for k in a_f if a_f[k] != b_f[k]}


def _cascador(path, env=None, **options):
    from jda_amd import api
    with pytest.MonkeyPatch.context() as mp:
        for k, v in (env or {}).items():
            mp.setenv(k, v)
        c = api.Cascador(path)          # (the JDA_* environment is read here)
    for k, v in dict(dict(dense=0, wide_max=0), **options).items():
        c.set_option(k, v)
    return c


def expected(name, dial, trace, fin_carry=1, stream_mb=None, form=None):
    """The launch keys one pass of a case must count, from the restatements above (form: where a cascador's options make the
    case's job take another form than the case's own)."""
    from jda_amd import api
    cs = CASES[name]
    T, K, L, D = cs["dims"]
    rb = 4 if dial == "C" else 8
    st, multi = bool(cs["st"]) and dial == "CPP", bool(cs["multi"])
    mb = int(cs["env"].get("JDA_W_STREAM_MB", 8)) if stream_mb is None else stream_mb
    stream = not trace and not multi and not st and w_stream(cs["dims"], rb, mb)
    kG, tile = stage_groups(K), tile_win(cs["dims"], rb, st, multi) > 0
    carry = bool(fin_carry) and carry_fits(cs["dims"])
    FL = api.FinishLaunch
    form = form or cs["form"]
    if form == "MERGED":
        return {FL("k_finish", dial, trace, kG, multi, st, stream, False, False, tile): 1}
    if form == "FILTER0":
        return {FL("k_filter0", dial, trace, 0, False, False, False, False, carry, False): 1,
                FL("k_finish", dial, trace, kG, multi, st, stream, True, carry, tile): 1}
    assert form == "TWO_LAUNCH"
    return {FL("k_finish", dial, trace, 1, multi, st, stream, False, False, False): 1,         # fin_g1 = 1, fin_tile1 = 0
            FL("k_finish", dial, trace, kG, multi, st, stream, False, False, tile): 1}


def _same_trace(want_frames, got, what):
    off = 0
    for i, r in enumerate(want_frames):
        n = len(r["carts_n"])
        for k in ("carts_n", "score", "path_hash", "shapes"):
            assert same(r[k], got[k][off:off + n]), (what, i, k, int((bits(r[k]) != bits(got[k][off:off + n])).sum()))
        off += n
    assert off == len(got["carts_n"]), what


def _same_counters(st, nb, T, what, regrows_ok=False):
    assert st["patch_n"] == nb["windows"], (what, st["patch_n"], nb["windows"])
    assert st["cart_total_n"] == nb["total"], (what, st["cart_total_n"], nb["total"])
    assert st["handoff_n"] == nb["handoff"], (what, st["handoff_n"], nb["handoff"])
    assert list(st["stage_done_n"][:T]) == nb["done"], (what, list(st["stage_done_n"][:T]), nb["done"])
    assert st["face_patch_n"] == nb["faces"], (what, st["face_patch_n"], nb["faces"])
    assert st["dense_passes"] == 0 and st["scan_fallbacks"] == 0 and (regrows_ok or st["ws_regrows"] == 0), what


def _assert_keys(what, fl, ff, want, form, regrown=False):
    """One pass: exactly the expected keys, once each.  regrown: a pass issued again after a queue overflow counts its launches
    again -- whole multiples of the expected keys, as many as the form counts."""
    n = ff.get(form, 0)
    assert set(ff) == {form} and (n >= 1 if regrown else n == 1) and fl == {k: v * n for k, v in want.items()}, (what, fl, ff)


def _run_dialect(name, c, dial, cond, fin_carry=1, rows=None, form=None):
    """Every call of a case in one dialect on cascador c; -> the traces (for a second cascador to be compared with).
    rows: the traces of the case's first cascador -- this one has to give the same rows (and the oracle's detections) under
    its own launch keys; form: the form its options make it take."""
    cs, inp = CASES[name], _inputs(name)
    T = cs["dims"][0]
    trace_fn, detect_fn = (c.trace, c.detect_batch) if dial == "C" else (c.trace_cpp, c.detect_batch_cpp)
    det_keys = ("bboxes", "scores", "shapes") if dial == "C" else ("rects", "scores", "shapes")
    regrows_ok = "cap_l" in cs["cond"]
    form = form or cs["form"]
    out = []
    for i, call in enumerate(inp[dial]):
        what = "%s %s call %d" % (name, dial, i)
        got, fl, ff = _launches(c, trace_fn, call["frames"], **call["kw"])
        print(what, "trace:", sorted(fl.items()), ff)
        _assert_keys(what, fl, ff, expected(name, dial, True, fin_carry, form=form), form, regrows_ok)
        _same_trace(call["trace"], got, what)
        out.append(got)
        for rep in range(1 if rows is not None else 2):              # (the second call is sized from the first one's hand-off)
            (dets, st), fl, ff = _launches(c, detect_fn, call["frames"], stats=True, **call["kw"])
            print(what, "detect:", sorted(fl.items()), ff)
            _assert_keys(what, fl, ff, expected(name, dial, False, fin_carry, form=form), form, regrows_ok and rep == 0)
            for want, g in zip(call["det"], dets):
                for k in det_keys:
                    assert same(want[k], g[k]), (what, rep, k)
            _same_counters(st, cond[dial][i], T, what, regrows_ok and rep == 0)
    if rows is not None:
        for a, b in zip(rows, out):
            for k in a:
                assert same(a[k], b[k]), (name, dial, "rows of the other cascador", k)
    return out


def _run_case(name):
    cs, inp = CASES[name], _inputs(name)
    cond = _check_conditions(name)
    dials = ("C", "CPP") if cs["cpp"] else ("C",)
    c = _cascador(inp["path"], cs["env"], **cs["opts"])
    try:
        assert c.finish_launches() == {}
        assert c.get_option("handoff") == cs["handoff"] and c.get_option("fin_carry") == 1
        if cs["st"]:
            c.set_similarity_transform(True)
        for dial, rb in (("C", 4), ("CPP", 8)):
            assert c.finish_tile_win(dial) == tile_win(cs["dims"], rb, cs["st"] and dial == "CPP", cs["multi"]), (name, dial)
        rows = {dial: _run_dialect(name, c, dial, cond) for dial in dials}
    finally:
        c.close()
    # the fitting carry cases and cap_l again without the carry, D = 4 of k_filter0 again without k_filter0: identical rows
    again = []
    if "carry" in cs["cond"] or "cap_l" in cs["cond"]:
        again.append((dict(fin_carry=0), 0))
    if name == "filter0_D4":
        again.append((dict(filter0=0), 1))
    for opts, fin_carry in again:
        c2 = _cascador(inp["path"], cs["env"], **dict(cs["opts"], **opts))
        try:
            for dial in dials:
                # (filter0 = 0: the same long queue in two k_finish launches -- kG = 1 without the tile for stage 0, then kG = 2)
                _run_dialect(name, c2, dial, cond, fin_carry=fin_carry, rows=rows[dial], form="TWO_LAUNCH" if "filter0" in opts else None)
        finally:
            c2.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(CASES))
def test_finish_launch_vs_oracle(built, gpu, name):
    """Which windows share a wave of k_filter0 (NW = 2 windows a wave, dealt a grid apart; an odd queue leaves the last wave
    with one) depends on the order the scan's workgroups filled the hand-off queue: it is not deterministic and is not
    asserted.  What is: the rows of every window, whatever wave took it."""
    _run_case(name)
