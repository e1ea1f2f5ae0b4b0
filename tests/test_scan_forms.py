"""Which stage-0 scan a pass launched (jdaScanForms, include/jda.h), and k_scan / k_scan_p at the
limits of their loops.

Every case names the scan instantiation it is about -- the ScanForm key (kernel, dialect, depth, pix, ragged, lean, trace,
merged) -- reads the difference of the cascador's counts around EACH call and asserts it, so that no comparison below can be
one instantiation standing in for another.  What a case compares, bit for bit (`same`):

  * trace(): carts walked, score, leaf hash and shape per window against the CPU oracle (dialect C: c/jda.c:357-426;
    dialect CPP: the repository's restatement),
  * detections against the oracle's, and the work counters handoff_n, scan_cart_n, scan_patch_n, cart_total_n against
    what the oracle's trace says they are (H = min(K, handoff) carts are the scan's):
        scan_patch_n = windows, scan_cart_n = sum(min(carts, H)), handoff_n = #(carts > H), cart_total_n = sum(carts).

Each case also states, as an assertion computed on the CPU from the oracle's trace and from plan_tiles(), the condition
that makes it the case it claims to be (test_inputs_meet_their_conditions runs them without a GPU; the GPU case checks
them again).  The frames are one pyramid level (min_size / max_size) of tens to a few hundred windows.

The kernel's constants restated here: first_phase = 16 carts before the first compaction, cp_max = 128 windows at or
below which a phase works on (window, cart) pairs, lds_win_max = 100, and scan_handoff_cap (k_scan_impl.h), the carts per
LDS table chunk."""
import atexit
import functools
import os
import shutil

import numpy as np
import pytest

from conftest import same, bits

FIRST_PHASE = 16
CP_MAX = 128
HANDOFF = 128
C_LEVEL = dict(scale=1.25, min_size=40, max_size=50)      # dialect C: the 46-pixel level alone, 4 pixels apart
CPP_LEVEL = dict(minimum_size=46, step=4, factor=4.0)     # dialect CPP: the same windows (the next size, 184, exceeds the frames)
WIN, STEP = 46, 4


def handoff_cap(D, real_bytes):
    """k_scan_impl.h: scan_handoff_cap."""
    node_n, leaf_n = (1 << (D - 1)) - 1, 1 << (D - 1)
    c = max(8, (16 * 1024) // (node_n * 8 + leaf_n * real_bytes + 4 * real_bytes))
    return c & ~63 if c >= 64 else c & ~7


def frame_of(nx, ny, win=WIN, step=STEP):
    """The smallest frame whose level of `win`-pixel windows is nx x ny."""
    return win + (nx - 1) * step, win + (ny - 1) * step


def _case(dims, frame, pix, z=1.6, norm=(5,), env=None, c_kw=None, cpp_kw=None, merged=True, kernel="k_scan", cond=None,
          n_frames=1, seed=5, fseed=7, cpp=True, tile=None, view=None, pix_cpp=None, only=None):
    # (only: "C" or "CPP" where the thresholds of a case are read from ONE dialect's oracle and the case runs that dialect alone)
    # (view: carts r whose neighbours r - 1 and r get a threshold read from the oracle, where the thresholds of _gates reject nobody)
    """dims (T, K, L, D); frame (width, height); pix: the pixel form both dialects must count; z: how far down, in
    standard deviations of the running score, every cart's threshold sits (_gates); norm: 1-based multiples of which a
    cart normalises, or a tuple of 0-based cart indices as a list; env: JDA_* options the cascador is created under;
    tile: (tw, th, tiles_x, tiles_y) the plan must give; cond: name of the condition beyond the common ones."""
    return dict(dims=dims, frame=frame, pix=pix, z=z, norm=norm, env=dict(env or {}), c_kw=dict(c_kw or C_LEVEL),
                cpp_kw=dict(cpp_kw or CPP_LEVEL), merged=merged, kernel=kernel, cond=cond, n_frames=n_frames, seed=seed,
                fseed=fseed, cpp=cpp, tile=tile, view=view, pix_cpp=pix_cpp or pix, only=only)


K_SWEEP = (1, 3, 7, 8, 15, 16, 17, 31, 33, 63, 65, 127, 128, 129)
CASES = {}
# ---- cart count K against first_phase, the 8/4/1 ladder, the hand-off and the table chunk: depth 4 (one chunk of 128),
#      depth 6 (chunks of 40 carts in fp32, 24 in fp64: the cuts fall inside phases), depth 8 (the floor of 8 carts)
for _K in K_SWEEP:
    CASES["K%d_depth4" % _K] = _case((2, _K, 5, 4), frame_of(27, 14), "T16_512", cond="cuts")
    CASES["K%d_depth6" % _K] = _case((2, _K, 5, 6), frame_of(27, 14), "T16_512", cond="cuts")
    CASES["K%d_depth8" % _K] = _case((2, _K, 3, 8), frame_of(16, 9), "T16_256", cond="cuts")
# ---- windows that die at the last cart before a chunk reload and at the first one after it (depth 4 reloads in fp64 only)
CASES["reload_depth4"] = _case((2, 129, 5, 4), frame_of(27, 14), "T16_512", z=2.5, cond="reload")
CASES["reload_depth6"] = _case((2, 65, 5, 6), frame_of(27, 14), "T16_512", z=2.5, cond="reload")
CASES["reload_depth8"] = _case((2, 33, 3, 8), frame_of(27, 14), "T16_512", z=2.5, cond="reload")
# ---- generic walk at depths 3 and 5, both block sizes
CASES["depth3_256"] = _case((2, 20, 5, 3), frame_of(16, 9), "T16_256")
CASES["depth3_512"] = _case((2, 20, 5, 3), frame_of(27, 14), "T16_512")
CASES["depth5_256"] = _case((2, 40, 5, 5), frame_of(16, 9), "T16_256", cond="cuts")
CASES["depth5_512"] = _case((2, 40, 5, 5), frame_of(27, 14), "T16_512", cond="cuts")
# ---- the hand-off option with K above it: k_filter0 / k_finish take over mid-stage
for _H, _K in ((16, 40), (24, 40), (128, 140)):
    for _D in (4, 6):
        CASES["handoff%d_depth%d" % (_H, _D)] = _case((2, _K, 5, _D), frame_of(27, 14), "T16_512", env={"JDA_HANDOFF": str(_H)},
                                                      cond="handoff")
# ---- tile occupancy: pair phases from the start at 128 windows and not at 129; the block changes above 256; 512; one
#      window; one column, one row; edge tiles narrower and lower than the nominal one in the same level
CASES["tile_128"] = _case((2, 40, 5, 4), frame_of(16, 8), "T16_256", tile=(16, 8, 1, 1), cond="n128")
CASES["tile_129"] = _case((2, 40, 5, 4), frame_of(43, 3), "T16_256", tile=(43, 3, 1, 1), cond="n129")
CASES["tile_256"] = _case((2, 40, 5, 6), frame_of(16, 16), "T16_256", tile=(16, 16, 1, 1))
CASES["tile_258"] = _case((2, 40, 5, 6), frame_of(43, 6), "T16_512", tile=(43, 6, 1, 1))     # (257 is prime and a tile at most 128 wide)
CASES["tile_512"] = _case((2, 40, 5, 4), frame_of(32, 16), "T16_512", tile=(32, 16, 1, 1))
CASES["one_window"] = _case((2, 40, 5, 4), frame_of(1, 1), "GLB", z=50.0, tile=(1, 1, 1, 1))
CASES["one_column"] = _case((2, 40, 5, 4), frame_of(1, 20), "T16_256", z=2.5, tile=(1, 20, 1, 1))
CASES["one_row"] = _case((2, 40, 5, 6), frame_of(30, 1), "T16_256", z=2.5, tile=(30, 1, 1, 1))
CASES["edge_tiles"] = _case((2, 40, 5, 4), (230, 207), "T16_512", cond="edges", n_frames=2, tile=(24, 21, 2, 2),
                            cpp_kw=dict(minimum_size=46, step=4, factor=5.0))      # (46 * 4 = 184 would fit this frame)
# ---- entering the pair phases late: 129 and then at most 128 survivors after a phase
for _dial in ("C", "CPP"):
    for _D, _K in ((4, 70), (6, 70), (5, 70), (9, 40), (10, 40)):
        # (depth 9: 256 leaves are the most the pair form takes, its leaf indices being bytes; depth 10: 512 leaves -- the model
        #  format admits depths up to 12 -- stay lane = window however few windows are left)
        CASES["late_pairs_depth%d_%s" % (_D, _dial)] = _case((2, _K, 5 if _D < 9 else 3, _D), frame_of(27, 14), "T16_512", cond="late",
                                                             only=_dial)
# ---- mode boundaries: 100-pixel windows in LDS (16-bit offsets at a pitch of 656, 21-bit at 672), 101 pixels global
CASES["win100_T16"] = _case((2, 20, 5, 4), frame_of(55, 1, 100, 10), "T16_256", z=2.0, n_frames=3, view=(6, 14), c_kw=dict(scale=4.17, min_size=25, max_size=100),
                            cpp_kw=dict(minimum_size=100, step=10, factor=8.0), tile=(55, 1, 1, 1), cond="off16")
# (dialect CPP: plan_tiles() shows the fp32 plan only; with fp64 tables the chooser cuts this level into narrower tiles, which stay
#  within 16 bits -- measured from jdaScanForms, so T21 in dialect CPP is not reached by this frame)
CASES["win100_T21"] = _case((2, 20, 5, 4), frame_of(57, 1, 100, 10), "T21", pix_cpp="T16_256", z=2.0, n_frames=3, view=(6, 14), c_kw=dict(scale=4.17, min_size=25, max_size=100),
                            cpp_kw=dict(minimum_size=100, step=10, factor=8.0), tile=(57, 1, 1, 1), cond="off21")
for _D in (4, 5, 6):
    CASES["win101_GLB_depth%d" % _D] = _case((2, 40, 5, _D), frame_of(57, 2, 101, 10), "GLB",
                                             c_kw=dict(scale=4.21, min_size=25, max_size=101),
                                             cpp_kw=dict(minimum_size=101, step=10, factor=8.0))
# ---- one launch per level against the merged launch
CASES["per_level_depth4"] = _case((2, 40, 5, 4), frame_of(27, 14), "T16_512", env={"JDA_MERGE_BLOCKS": "0"}, merged=False)
CASES["per_level_depth6"] = _case((2, 40, 5, 6), frame_of(16, 9), "T16_256", env={"JDA_MERGE_BLOCKS": "0"}, merged=False)
# ---- frames: 1, 7, 8 and 9 of them (the `frame >= n_frames` exit of the surplus workgroups); a width that is no multiple
#      of 16
for _n in (7, 8, 9):
    CASES["frames_%d" % _n] = _case((2, 40, 5, 4), (151, 99), "T16_512", n_frames=_n)
# ---- the lean line: the only normalising cart is cart handoff - 1 (not lean), cart handoff (lean), cart 0 (not lean)
for _name, _cart in (("before", 15), ("at", 16), ("first", 0)):
    for _D in (4, 6, 5):
        CASES["lean_%s_depth%d" % (_name, _D)] = _case((2, 40, 5, _D), frame_of(27, 14), "T16_512", norm=[_cart],
                                                      env={"JDA_HANDOFF": "16"}, cond="handoff")
# ---- k_scan_p, every instantiation a uniform pass has (depth 4, 6, generic), lean and not: scan_p = 2 so that a small job takes it
for _name, _cart in (("before", 15), ("at", 16)):
    for _D in (4, 6, 5):
        CASES["scan_p_%s_depth%d" % (_name, _D)] = _case((2, 40, 5, _D), frame_of(27, 14), "T16_512", norm=[_cart], n_frames=2,
                                                        env={"JDA_HANDOFF": "16", "JDA_SCAN_P": "2", "JDA_MERGE_BLOCKS": "0"},
                                                        kernel="k_scan_p", merged=False, cond="handoff")
# ---- the lean form (no cart of the scanned range normalises) of every pixel form, merged and per level
for _D in (4, 6, 5):
    CASES["lean_T16_256_depth%d" % _D] = _case((2, 40, 5, _D), frame_of(16, 9), "T16_256", norm=[])
    CASES["lean_per_level_depth%d" % _D] = _case((2, 40, 5, _D), frame_of(16, 9) if _D == 6 else frame_of(27, 14),
                                                 "T16_256" if _D == 6 else "T16_512", norm=[], env={"JDA_MERGE_BLOCKS": "0"}, merged=False)
    CASES["lean_GLB_depth%d" % _D] = _case((2, 40, 5, _D), frame_of(57, 2, 101, 10), "GLB", norm=[],
                                           c_kw=dict(scale=4.21, min_size=25, max_size=101), cpp_kw=dict(minimum_size=101, step=10, factor=8.0))
for _D in (4, 5):
    CASES["per_level_256_depth%d" % _D] = _case((2, 40, 5, _D), frame_of(16, 9), "T16_256", env={"JDA_MERGE_BLOCKS": "0"}, merged=False)
    CASES["lean_per_level_256_depth%d" % _D] = _case((2, 40, 5, _D), frame_of(16, 9), "T16_256", norm=[], env={"JDA_MERGE_BLOCKS": "0"},
                                                     merged=False)
CASES["lean_per_level_512_depth6"] = _case((2, 40, 5, 6), frame_of(27, 14), "T16_512", norm=[], env={"JDA_MERGE_BLOCKS": "0"}, merged=False)
for _D in (4, 6, 5):
    CASES["scan_p_at_256_threads_depth%d" % _D] = _case((2, 40, 5, _D), frame_of(27, 14), "T16_256", norm=[16], n_frames=2, kernel="k_scan_p",
                                                        merged=False, cond="handoff",
                                                        env={"JDA_HANDOFF": "16", "JDA_SCAN_P": "2", "JDA_MERGE_BLOCKS": "0", "JDA_SCAN_P_BLOCK": "256"})
CASES["lean_T21"] = _case((2, 20, 5, 4), frame_of(57, 1, 100, 10), "T21", pix_cpp="T16_256", z=2.0, n_frames=3, view=(6, 14), norm=[],
                          c_kw=dict(scale=4.17, min_size=25, max_size=100), cpp_kw=dict(minimum_size=100, step=10, factor=8.0),
                          tile=(57, 1, 1, 1), cond="off21")
# ---- 129, then 128 survivors in a tile of 256 windows: 256 threads, where 256 pair slots would not fit the pair scratch
for _dial in ("C", "CPP"):
    CASES["late_pairs_256_threads_%s" % _dial] = _case((2, 70, 5, 4), frame_of(16, 16), "T16_256", cond="late", only=_dial,
                                                       tile=(16, 16, 1, 1))
CASES["scan_p_block256"] = _case((2, 40, 5, 4), frame_of(27, 14), "T16_256", n_frames=2, kernel="k_scan_p", merged=False,
                                 env={"JDA_SCAN_P": "2", "JDA_MERGE_BLOCKS": "0", "JDA_SCAN_P_BLOCK": "256"})


def phase_ends(H, chunk, first=FIRST_PHASE):
    """k_scan_impl.h, the phase loop: the carts after which the survivors are compacted -- 16, then doubling up to 64 / 128
    carts a phase, every phase cut at the end of its table chunk."""
    ends, kb = [], 0
    while kb < H:
        ke, c0 = min(H, kb + chunk), kb
        while c0 < ke:
            plen = first - c0 if c0 < first else min(c0, 128 if c0 >= 128 else 64)
            c0 = min(ke, c0 + plen)
            ends.append(c0)
        kb += chunk
    return ends


def _reloads(D, H):
    """The carts in front of which a workgroup of either dialect reloads its table chunk."""
    return sorted({r for rb in (4, 8) for r in range(min(H, handoff_cap(D, rb)), H, min(H, handoff_cap(D, rb)))})


# cases that run in a child process of their own (test_forced_tile_shape_takes_21_bit_offsets): not in CASES' parametrisations
EXTRA_CASES = {"forced_T21_depth%d" % _D: dict(CASES["win100_T21"], dims=(2, 20, 5, _D)) for _D in (4, 6, 5)}
EXTRA_CASES.update({"forced_T21_lean_depth%d" % _D: dict(CASES["lean_T21"], dims=(2, 20, 5, _D)) for _D in (4, 6, 5)})


def _gates(m, z):
    """Every cart of stage 0 and 1 rejects a little: its threshold sits z standard deviations under a score that walks
    like a sum of k + 1 leaves of N(0, 0.5^2), so that windows die all along and some are alive at every cut."""
    f32 = lambda v: np.asarray(v, np.float32).astype(np.float64)
    k = np.arange(m.K)
    m.cth[:] = f32(-z * 0.5 * np.sqrt(k + 1.0))[None, :]


@functools.lru_cache(maxsize=None)
def _inputs(name):
    """Model file, frames and the oracle's traces of a case: computed once, shared by the CPU and the GPU test."""
    import tempfile
    from jda_amd import synth
    from oracle import build as oracle_build
    from oracle.pyoracle import Oracle
    oracle_build.build_oracle()
    cs = CASES.get(name) or EXTRA_CASES[name]
    T, K, L, D = cs["dims"]
    norm = cs["norm"]
    m = synth.make_model(T, K, L, D, seed=cs["seed"], norm_every=norm[0] if isinstance(norm, tuple) else 10 ** 6)
    if isinstance(norm, list):      # (values as make_model draws them: a mean of the order of 0.1, a deviation in [0.8, 1.25])
        for k in norm:
            m.cmean[0, k] = float(np.float32(0.07)); m.cstd[0, k] = float(np.float32(1.125))
    _gates(m, cs["z"])
    d = tempfile.mkdtemp(prefix="scan_forms_")
    atexit.register(shutil.rmtree, d, True)
    path = os.path.join(d, name + ".model")
    w, h = cs["frame"]
    frames = synth.make_frames(cs["n_frames"], w, h, seed=cs["fseed"])
    if cs["cond"] == "late":
        # nothing rejects but cart 15, which leaves exactly cp_max + 1 = 129 windows, and cart 16, which leaves 128: the phase that
        # ends at cart 16 hands 129 windows on (lane = window goes on), the next one 128 (the pair form takes over).  The
        # thresholds lie half way between two neighbouring scores the oracle reports for the windows that reach the cart.
        m.cth[:] = -1e30
        for c, keep in ((FIRST_PHASE - 1, CP_MAX + 1), (FIRST_PHASE, CP_MAX)):
            m.cth[0, c] = 1e30
            m.save(path, 8)
            o = Oracle(path)
            tr = [o.trace(f, want_shapes=False, **cs["c_kw"]) if cs["only"] == "C" else o.trace_cpp(f, **cs["cpp_kw"]) for f in frames]
            o.close()
            sc = np.sort(np.concatenate([t["score"] for t in tr])[np.concatenate([t["carts_n"] for t in tr]) == c + 1])[::-1]
            assert len(sc) > keep and sc[keep - 1] > sc[keep], (name, c, len(sc))
            m.cth[0, c] = float(np.float32((float(sc[keep - 1]) + float(sc[keep])) / 2))
            assert sc[keep - 1] >= m.cth[0, c] > sc[keep], (name, c)
        m.cth[1, K // 2] = m.cth[0, FIRST_PHASE]          # (... and stage 1 rejects somebody too)
    if cs["cond"] == "reload" or cs["view"]:
        # carts r - 1 and r around every chunk reload reject an eighth of the windows that reach them: the threshold is read from
        # the oracle, as the score those windows have there (a cart that rejects everybody reports it)
        for r in (_reloads(D, _handoff_of(cs)) if cs["cond"] == "reload" else cs["view"]):
            for c in (r - 1, r):
                if c >= K:
                    continue
                m.cth[0, c] = 1e30
                m.save(path, 8)
                o = Oracle(path)
                tr = [o.trace(f, want_shapes=False, **cs["c_kw"]) for f in frames]
                o.close()
                sc = np.concatenate([t["score"] for t in tr])[np.concatenate([t["carts_n"] for t in tr]) == c + 1]
                assert len(sc) >= 16, (name, c, len(sc))
                m.cth[0, c] = float(np.sort(sc)[len(sc) // 8])
    m.save(path, 8)
    o = Oracle(path)
    out = dict(path=path, model=m, frames=frames)
    if cs["only"] != "CPP":
        out.update(trace_c=[o.trace(f, **cs["c_kw"]) for f in frames], det_c=[o.detect(f, **cs["c_kw"]) for f in frames])
    if cs["cpp"] and cs["only"] != "C":
        out["trace_cpp"] = [o.trace_cpp(f, **cs["cpp_kw"]) for f in frames]
        out["det_cpp"] = [o.detect_cpp(f, **cs["cpp_kw"]) for f in frames]
    o.close()
    return out


def _handoff_of(cs):
    return min(cs["dims"][1], int(cs["env"].get("JDA_HANDOFF", HANDOFF)))


def _any_norm(cs, m, fp32):
    H = _handoff_of(cs)
    if fp32:
        return bool(((m.cmean[0, :H].astype(np.float32) != 0) | (m.cstd[0, :H].astype(np.float32) != 1)).any())
    return bool(((m.cmean[0, :H] != 0) | (m.cstd[0, :H] != 1)).any())


def _expected(name, dialect, trace):
    """The one ScanForm key every scan launch of a call of this case must count under."""
    from jda_amd import api
    cs, m = CASES[name], _inputs(name)["model"]
    D = cs["dims"][3]
    persistent = cs["kernel"] == "k_scan_p" and dialect == "C" and not trace      # (k_scan_p: dialect C, no trace)
    lean = not trace and not _any_norm(cs, m, dialect == "C")
    pix = cs["pix"] if dialect == "C" else cs["pix_cpp"]
    if cs["kernel"] == "k_scan_p" and not persistent:       # what k_scan takes for the level instead
        pix = "T16_512" if _plan(name)[0]["tw"] * _plan(name)[0]["th"] > 256 else "T16_256"
    return api.ScanForm("k_scan_p" if persistent else "k_scan", dialect, D if D in (4, 6) else 0, pix, False, lean, trace,
                        cs["merged"])


@functools.lru_cache(maxsize=None)
def _plan(name):
    from jda_amd import api
    cs, inp = CASES[name], _inputs(name)
    c = api.Cascador(inp["path"])
    try:
        w, h = cs["frame"]
        return c.plan_tiles(w, h, **cs["c_kw"])
    finally:
        c.close()


def _check_conditions(name):
    """The conditions of a case, from the plan and the oracle's trace; -> per dialect the numbers the GPU case needs."""
    cs, inp = CASES[name], _inputs(name)
    T, K, L, D = cs["dims"]
    H = _handoff_of(cs)
    plan = _plan(name)
    assert len(plan) == 1, (name, plan)           # one pyramid level
    lv = plan[0]
    n_tile = lv["tw"] * lv["th"]
    mode_pix = {1: "T16_512" if n_tile > 256 else "T16_256", 3: "T21", 2: "GLB"}[lv["mode"]]
    want_pix = cs["pix"] if cs["kernel"] == "k_scan" else ("T16_512" if n_tile > 256 else "T16_256")
    assert mode_pix == want_pix, (name, lv)
    if cs["tile"]:
        assert (lv["tw"], lv["th"], lv["tiles_x"], lv["tiles_y"]) == cs["tile"], (name, lv)
    if cs["kernel"] == "k_scan_p":
        assert lv["mode"] == 1, (name, lv)
    max_off = (lv["win"] - 1) * lv["pitch"] + lv["win"] - 1 + 15         # plans.cpp: choose_tile
    if cs["cond"] == "off16":
        assert lv["mode"] == 1 and max_off <= 65535 < max_off + 16 * (lv["win"] - 1), (name, lv, max_off)     # the last pitch that fits 16 bits
    if cs["cond"] == "off21":
        assert lv["mode"] == 3 and max_off > 65535, (name, lv, max_off)
    if cs["cond"] == "edges":
        assert lv["tiles_x"] > 1 and lv["tiles_y"] > 1 and lv["nx"] % lv["tw"] and lv["ny"] % lv["th"], (name, lv)
    if cs["cond"] == "n128":
        assert n_tile == lv["nx"] * lv["ny"] == CP_MAX
    if cs["cond"] == "n129":
        assert n_tile == lv["nx"] * lv["ny"] == CP_MAX + 1
    out = {}
    for dial, key, rb in (("C", "trace_c", 4), ("CPP", "trace_cpp", 8)):
        if key not in inp:
            continue
        carts = np.concatenate([t["carts_n"] for t in inp[key]])
        alive_after = lambda c: int((carts > c).sum())          # windows that passed carts 0 .. c - 1
        chunk = min(H, handoff_cap(D, rb))
        assert alive_after(H) >= 1 and alive_after(T * K - 1) >= 1, (name, dial, alive_after(H), alive_after(T * K - 1))        # the hand-off is not empty; a window walks everything
        assert int((carts <= H).sum()) >= 1 or H < 3 or len(carts) == 1, (name, dial, "the scan rejects")
        assert T < 2 or int(((carts > K) & (carts < T * K)).sum()) >= 1 or cs["cond"] != "late", (name, dial, "stage 1 rejects")
        if cs["cond"] in ("cuts", "handoff", "reload"):
            # windows alive at every cut of the scan
            assert all(alive_after(c) >= 1 for c in range(1, H + 1)), (name, dial)
        if cs["cond"] == "reload":
            # at every chunk reload a window that dies at the last cart before it and one at the first cart after it
            assert chunk < H or (dial, D) == ("C", 4), (name, dial)
            for r in range(chunk, H, chunk):
                assert int((carts == r).sum()) >= 1 and int((carts == r + 1).sum()) >= 1, (name, dial, "reload at cart", r)
        if cs["cond"] == "handoff":
            assert K > H and int(((carts > H) & (carts <= K)).sum()) >= 1, (name, dial)      # a window dies in stage 0 behind the hand-off
        if cs["cond"] == "late":
            # ONE tile of one frame that is left with exactly 129 windows after one phase and exactly 128 after the next one, at
            # the kernel's own phase ends for this dialect's chunk
            assert lv["tiles_x"] * lv["tiles_y"] == 1 and cs["n_frames"] == 1 and n_tile > CP_MAX, (name, lv)
            ends = phase_ends(H, chunk)
            n_at = [alive_after(c) for c in ends]
            i = ends.index(FIRST_PHASE)
            assert n_at[i] == CP_MAX + 1 and n_at[i + 1] == CP_MAX and (i == 0 or n_at[i - 1] > CP_MAX + 1), (name, dial, ends, n_at)
        out[dial] = dict(windows=len(carts), handoff=alive_after(H), scan_carts=int(np.minimum(carts, H).sum()),
                         total=int(carts.sum()), chunk=chunk)
        print("%s %s: %d windows, tile %dx%d mode %d, chunk %d, hand-off (after %d carts) %d" %
              (name, dial, len(carts), lv["tw"], lv["th"], lv["mode"], chunk, H, out[dial]["handoff"]))
    return out


@pytest.mark.parametrize("name", sorted(CASES))
def test_inputs_meet_their_conditions(built, name):
    _check_conditions(name)


def test_handoff_cap_restatement():
    # the chunks the K cases rely on: depth 4 one chunk of 128; depth 6 reloads inside phases; depth 8 at the floor
    assert [handoff_cap(4, 4), handoff_cap(4, 8)] == [128, 64]
    assert [handoff_cap(6, 4), handoff_cap(6, 8)] == [40, 24]
    assert [handoff_cap(8, 4), handoff_cap(8, 8), handoff_cap(9, 4)] == [8, 8, 8]
    assert [handoff_cap(5, 4), handoff_cap(3, 4)] == [64, 256]
    # the phase ends the late-pair cases rely on: 16 is one in every dialect and depth, the next one differs
    assert phase_ends(70, 70) == [16, 32, 64, 70] and phase_ends(70, 64) == [16, 32, 64, 70]
    assert phase_ends(70, 40) == [16, 32, 40, 70] and phase_ends(70, 24) == [16, 24, 48, 70]
    assert phase_ends(40, 8) == [8, 16, 24, 32, 40] and phase_ends(128, 128) == [16, 32, 64, 128]


def test_scan_form_index_round_trip(built):
    from jda_amd import api
    seen = set()
    for i in range(api.SCAN_FORM_N):
        f = api.ScanForm.of_index(i)
        assert f.index() == i
        seen.add(f)
    assert len(seen) == api.SCAN_FORM_N == 2 * 2 * 3 * 4 * 2 * 2 * 2 * 2
    # include/jda.h: JDA_SCAN_FORM(kernel, dialect, depth, pix, ragged, lean, trace, merged)
    assert api.ScanForm("k_scan", "C", 4, "T16_256", False, False, False, True).index() == 1
    assert api.ScanForm("k_scan_p", "C", 4, "T16_256", False, False, False, False).index() == 384
    assert api.ScanForm("k_scan", "CPP", 0, "GLB", True, True, False, False).index() == ((((((0 * 2 + 1) * 3 + 2) * 4 + 3) * 2 + 1) * 2 + 1) * 2 + 0) * 2


# ---------------------------------------------------------------- GPU

@pytest.fixture(scope="module")
def gpu():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    return torch.device("cuda", 0)


def _forms(c, fn, *a, **kw):
    """-> (what the call returned, the scan forms its passes launched: {ScanForm: count})."""
    before = c.scan_forms()
    r = fn(*a, **kw)
    after = c.scan_forms()
    assert all(after.get(k, 0) >= v for k, v in before.items())
    return r, {k: v - before.get(k, 0) for k, v in after.items() if v != before.get(k, 0)}


def _cascador(path, env):
    from jda_amd import api
    old = dict(os.environ)
    os.environ.update(env)
    try:
        return api.Cascador(path)          # (the options are read here)
    finally:
        os.environ.clear(); os.environ.update(old)


def _same_trace(want_frames, got, what):
    off = 0
    for i, r in enumerate(want_frames):
        n = len(r["carts_n"])
        for k in ("carts_n", "score", "path_hash", "shapes"):
            assert same(r[k], got[k][off:off + n]), (what, i, k, int((bits(r[k]) != bits(got[k][off:off + n])).sum()))
        off += n
    assert off == len(got["carts_n"]), what


def _same_counters(st, want, what):
    assert st["scan_patch_n"] == st["patch_n"] == want["windows"], (what, st["scan_patch_n"], st["patch_n"], want["windows"])
    assert st["handoff_n"] == want["handoff"], (what, st["handoff_n"], want["handoff"])
    assert st["scan_cart_n"] == want["scan_carts"], (what, st["scan_cart_n"], want["scan_carts"])
    assert st["cart_total_n"] == want["total"], (what, st["cart_total_n"], want["total"])
    assert st["scan_fallbacks"] == 0 and st["dense_passes"] == 0, what


def _run_cpp(name, c, cond):
    cs, inp = CASES[name], _inputs(name)
    frames = inp["frames"]
    got, f = _forms(c, c.trace_cpp, frames, **cs["cpp_kw"])
    print(name, "trace_cpp:", f)
    assert f == {_expected(name, "CPP", True): 1}, (name, f)
    _same_trace(inp["trace_cpp"], got, name + " cpp")
    (dets, st), f = _forms(c, c.detect_batch_cpp, frames, stats=True, **cs["cpp_kw"])
    print(name, "detect_cpp:", f)
    assert f == {_expected(name, "CPP", False): 1}, (name, f)
    for want, g in zip(inp["det_cpp"], dets):
        for k in ("rects", "scores", "shapes"):
            assert same(want[k], g[k]), (name, "cpp", k)
    _same_counters(st, cond["CPP"], name + " cpp")


def _run_case(name):
    cs, inp = CASES[name], _inputs(name)
    cond = _check_conditions(name)
    frames = inp["frames"]
    c = _cascador(inp["path"], dict(cs["env"], JDA_DENSE="0"))      # (dense mode counts no scan at all)
    try:
        assert c.scan_forms() == {}
        if cs["only"] == "CPP":
            return _run_cpp(name, c, cond)
        got, f = _forms(c, c.trace, frames, **cs["c_kw"])
        print(name, "trace:", f)
        assert f == {_expected(name, "C", True): 1}, (name, f)
        _same_trace(inp["trace_c"], got, name)
        for rep in range(2):            # (the second call is sized from the first one's hand-off)
            (dets, st), f = _forms(c, c.detect_batch, frames, stats=True, **cs["c_kw"])
            print(name, "detect:", f)
            assert f == {_expected(name, "C", False): 1}, (name, rep, f)
            for want, g in zip(inp["det_c"], dets):
                for k in want:
                    assert same(want[k], g[k]), (name, rep, k)
            _same_counters(st, cond["C"], name)
        if cs["cpp"] and cs["only"] != "C":
            _run_cpp(name, c, cond)
    finally:
        c.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(CASES))
def test_scan_form_vs_oracle(built, gpu, name):
    _run_case(name)


# ---------------------------------------------------------------- frames as the caller holds them

@pytest.mark.gpu
@pytest.mark.parametrize("how", ["unaligned_base", "long_stride"])
def test_device_frames_off_the_loaders_fast_path(built, gpu, how):
    """Resident frames whose base is not 16-byte aligned (a view three bytes into a larger buffer), and frames that lie
    further apart than width x height (a stride of w * h + 37 bytes: the tile loader takes its path without LDS-DMA).  Same detections and counters as the oracle, form asserted."""
    import torch
    name = "frames_7"
    cs, inp = CASES[name], _inputs(name)
    cond = _check_conditions(name)
    frames = inp["frames"]
    n, h, w = frames.shape
    c = _cascador(inp["path"], dict(cs["env"], JDA_DENSE="0"))
    try:
        if how == "unaligned_base":
            buf = torch.zeros(n * h * w + 64, dtype=torch.uint8, device="cuda")
            dev = buf[3:3 + n * h * w].view(n, h, w)
            dev.copy_(torch.from_numpy(frames))
            assert dev.data_ptr() % 16 == 3 and dev.is_contiguous()
            (dets, st), f = _forms(c, c.detect_batch_device, dev, stats=True, **cs["c_kw"])
        else:
            import ctypes as C
            from jda_amd import api
            stride = h * w + 37
            big = torch.zeros((n, stride), dtype=torch.uint8, device="cuda")
            big[:, :h * w].copy_(torch.from_numpy(frames).reshape(n, h * w))
            kw = cs["c_kw"]

            def call():
                res = (api.jdaResult * n)()
                o, st = c._opts(True, True)
                rc = api.lib.jdaDetectBatchDevice(c.h, C.c_void_p(big.data_ptr()), stride, n, w, h, kw["scale"], 0.1,
                                                  kw["min_size"], kw["max_size"], -0.5, C.byref(o), res)
                assert rc == 0, api.last_error()
                return [api._take(res[i]) for i in range(n)], st.asdict()
            (dets, st), f = _forms(c, call)
        print(how, f)
        assert f == {_expected(name, "C", False): 1}, f
        for want, g in zip(inp["det_c"], dets):
            for k in want:
                assert same(want[k], g[k]), (how, k)
        _same_counters(st, cond["C"], how)
    finally:
        c.close()


# ---------------------------------------------------------------- a rerun counts again

@pytest.mark.gpu
def test_recover_scan_rerun_counts_its_launches_again(built, gpu):
    """On the build whose persistent scan always trips its watchdog (libjda_wd.so, tests/test_scan_persistent.py) a pass
    launches k_scan_p, comes back short and is issued again with k_scan: both launches are counted, under their own keys."""
    import json
    import subprocess
    import sys
    from jda_amd import build as lib_build
    name = "scan_p_at_depth4"
    cs, inp = CASES[name], _inputs(name)
    assert lib_build.build_watchdog() == lib_build.WD_LIB and os.path.exists(lib_build.WD_LIB)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    script = (
        "import json, sys\n"
        "sys.path.insert(0, %r)\n"
        "import numpy as np\n"
        "from jda_amd import api, synth\n"
        "c = api.Cascador(%r)\n"
        "frames = synth.make_frames(%d, %d, %d, seed=%d)\n"
        "dets, st = c.detect_batch(frames, stats=True, **%r)\n"
        "print(json.dumps(dict(forms=[[list(k), v] for k, v in c.scan_forms().items()], fallbacks=st['scan_fallbacks'],\n"
        "                      n=[len(d['scores']) for d in dets], handoff=st['handoff_n'])))\n"
    ) % (root, inp["path"], cs["n_frames"], cs["frame"][0], cs["frame"][1], cs["fseed"], cs["c_kw"])
    env = dict(os.environ, JDA_LIB_PATH=lib_build.WD_LIB, JDA_DENSE="0", **cs["env"])
    r = subprocess.run([sys.executable, "-c", script], env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    out = json.loads(r.stdout.strip().splitlines()[-1])
    forms = {tuple(k): v for k, v in out["forms"]}
    print(forms, out["fallbacks"])
    cond = _check_conditions(name)
    assert out["fallbacks"] == 1 and out["handoff"] == cond["C"]["handoff"]
    assert out["n"] == [len(d["scores"]) for d in inp["det_c"]]
    assert forms == {tuple(_expected(name, "C", False)): 1,
                     tuple(_expected(name, "C", False)._replace(kernel="k_scan", pix="T16_512")): 1}, forms


# ---------------------------------------------------------------- ragged jobs

RAGGED_SIZES = [(150, 98), (131, 77), (150, 98), (97, 60), (46, 300)]      # (the last image lacks nothing but is one column wide)


@functools.lru_cache(maxsize=None)
def _ragged_inputs(D):
    import tempfile
    from jda_amd import synth
    from oracle import build as oracle_build
    from oracle.pyoracle import Oracle
    oracle_build.build_oracle()
    m = synth.make_model(2, 40, 5, D, seed=5, norm_every=5)
    _gates(m, 1.6)
    d = tempfile.mkdtemp(prefix="scan_forms_")
    atexit.register(shutil.rmtree, d, True)
    path = os.path.join(d, "ragged_%d.model" % D)
    m.save(path, 8)
    # images of different sizes: a narrower one re-cuts the nominal tile, the small ones lack the 57-pixel level the others have
    imgs = [synth.make_frames(1, w, h, seed=20 + i)[0] for i, (w, h) in enumerate(RAGGED_SIZES)]
    o = Oracle(path)
    kw = dict(scale=1.25, min_size=40, max_size=60)
    out = dict(path=path, imgs=imgs, kw=kw, det_c=[o.detect(im, **kw) for im in imgs], trace_c=[o.trace(im, **kw) for im in imgs],
               det_cpp=[o.detect_cpp(im, **CPP_LEVEL) for im in imgs], trace_cpp=[o.trace_cpp(im, **CPP_LEVEL) for im in imgs],
               levels=[len(synth.levels_c(im.shape[1], im.shape[0], **kw)[0]) for im in imgs])
    o.close()
    return out


def test_ragged_inputs_meet_their_conditions(built):
    inp = _ragged_inputs(4)
    assert sorted(set(inp["levels"])) == [1, 2]          # an image lacks a level others have
    # an image narrower than the nominal grid the tiles are chosen for (ragged.cpp: the mean windows per row, rounded up to 4)
    nx = [(im.shape[1] - WIN) // STEP + 1 for im in inp["imgs"]]
    assert min(nx) == 1 and -(-sum(nx) // len(nx) // 4) * 4 >= 16
    assert len({im.shape for im in inp["imgs"]}) >= 4


@pytest.mark.gpu
@pytest.mark.parametrize("D", [4, 6, 5])
@pytest.mark.parametrize("dialect", ["C", "CPP"])
def test_ragged_scan_forms_vs_oracle(built, gpu, D, dialect):
    inp = _ragged_inputs(D)
    c = _cascador(inp["path"], {"JDA_DENSE": "0", "JDA_RAGGED_SINGLE_WINDOWS": "0"})
    try:
        if dialect == "C":
            (dets, st), f = _forms(c, c.detect_ragged, inp["imgs"], stats=True, **inp["kw"])
            want_d, want_t, keys = inp["det_c"], inp["trace_c"], ("bboxes", "scores", "shapes")
        else:
            (dets, st), f = _forms(c, c.detect_ragged_cpp, inp["imgs"], stats=True, **CPP_LEVEL)
            want_d, want_t, keys = inp["det_cpp"], inp["trace_cpp"], ("rects", "scores", "shapes")
        print("RAGGED_FORMS", D, dialect, sorted((tuple(k), v) for k, v in f.items()))
        # five images are far fewer than merge_blocks workgroups: the chunk planner puts every LDS-tiled level into ONE merged
        # launch, which is always cut for 256 threads (ragged.cpp: merged()); no level here is global-pixel
        from jda_amd import api
        assert f == {api.ScanForm("k_scan", dialect, D if D in (4, 6) else 0, "T16_256", True, False, False, True): 1}, f
        for want, g in zip(want_d, dets):
            for k in keys:
                assert same(want[k], g[k]), (D, dialect, k)
        carts = np.concatenate([t["carts_n"] for t in want_t])
        _same_counters(st, dict(windows=len(carts), handoff=int((carts > 40).sum()), scan_carts=int(np.minimum(carts, 40).sum()),
                                total=int(carts.sum())), "ragged")
    finally:
        c.close()


# ---------------------------------------------------------------- a launch over several levels

TWO_LEVELS = dict(scale=1.25, min_size=40, max_size=60)      # the 46- and the 57-pixel level


@functools.lru_cache(maxsize=None)
def _two_level_inputs(D):
    import tempfile
    from jda_amd import api, synth
    from oracle import build as oracle_build
    from oracle.pyoracle import Oracle
    oracle_build.build_oracle()
    m = synth.make_model(2, 40, 5, D, seed=5, norm_every=5)
    _gates(m, 1.6)
    d = tempfile.mkdtemp(prefix="scan_forms_")
    atexit.register(shutil.rmtree, d, True)
    path = os.path.join(d, "two_levels_%d.model" % D)
    m.save(path, 8)
    frames = synth.make_frames(2, 150, 98, seed=7)
    o = Oracle(path)
    out = dict(path=path, frames=frames, trace=[o.trace(f, **TWO_LEVELS) for f in frames], det=[o.detect(f, **TWO_LEVELS) for f in frames])
    o.close()
    c = api.Cascador(path)
    out["plan"] = c.plan_tiles(150, 98, **TWO_LEVELS)
    c.close()
    return out


def _two_level_conditions(D):
    """One level whose tile holds more than 256 windows and one whose tile does not, both LDS-tiled with 16-bit offsets."""
    plan = _two_level_inputs(D)["plan"]
    assert [lv["mode"] for lv in plan] == [1, 1], plan
    n = [lv["tw"] * lv["th"] for lv in plan]
    assert n[0] > 256 >= n[1], plan
    return plan


@pytest.mark.parametrize("D", [4, 6])
def test_two_level_inputs_meet_their_conditions(built, D):
    _two_level_conditions(D)


@pytest.mark.gpu
@pytest.mark.parametrize("D", [4, 6])
@pytest.mark.parametrize("merge_blocks", [0, 1 << 20])
def test_merged_launch_against_a_launch_per_level(built, gpu, D, merge_blocks):
    """merge_blocks large: ONE launch over both levels, 512 threads because one of its levels has more than 256 windows a
    tile (scan_block_big's `any of its levels`), the other level's tiles filling half of them; merge_blocks = 0: a launch
    per level, 512 and 256 threads.  Both bit-exact against the oracle, traced and not."""
    from jda_amd import api
    inp = _two_level_inputs(D)
    _two_level_conditions(D)
    c = _cascador(inp["path"], {"JDA_DENSE": "0", "JDA_MERGE_BLOCKS": str(merge_blocks)})
    try:
        def want(trace):
            if merge_blocks:
                return {api.ScanForm("k_scan", "C", D, "T16_512", False, False, trace, True): 1}
            return {api.ScanForm("k_scan", "C", D, "T16_512", False, False, trace, False): 1,
                    api.ScanForm("k_scan", "C", D, "T16_256", False, False, trace, False): 1}
        got, f = _forms(c, c.trace, inp["frames"], **TWO_LEVELS)
        print("two levels, merge_blocks", merge_blocks, "trace:", f)
        assert f == want(True), f
        _same_trace(inp["trace"], got, "two levels")
        for rep in range(2):
            (dets, st), f = _forms(c, c.detect_batch, inp["frames"], stats=True, **TWO_LEVELS)
            assert f == want(False), f
            for w_, g in zip(inp["det"], dets):
                for k in w_:
                    assert same(w_[k], g[k]), (rep, k)
            carts = np.concatenate([t["carts_n"] for t in inp["trace"]])
            _same_counters(st, dict(windows=len(carts), handoff=int((carts > 40).sum()), scan_carts=int(np.minimum(carts, 40).sum()),
                                    total=int(carts.sum())), "two levels")
    finally:
        c.close()


# ---------------------------------------------------------------- a forced tile shape: T21 where the chooser does not pick it

TILES_SCRIPT = r"""
import json, sys
sys.path.insert(0, %(root)r)
import numpy as np
from jda_amd import api, synth
c = api.Cascador(%(model)r)
frames = synth.make_frames(%(n)d, %(w)d, %(h)d, seed=%(seed)d)
out, arrays = {}, {}
for name, call in (("trace", lambda: c.trace(frames, **%(c_kw)r)), ("detect", lambda: c.detect_batch(frames, stats=True, **%(c_kw)r)),
                   ("trace_cpp", lambda: c.trace_cpp(frames, **%(cpp_kw)r)), ("detect_cpp", lambda: c.detect_batch_cpp(frames, stats=True, **%(cpp_kw)r))):
    before = c.scan_forms()
    r = call()
    out[name] = [[list(k), v - before.get(k, 0)] for k, v in c.scan_forms().items() if v != before.get(k, 0)]
    if name.startswith("trace"):
        for k, a in r.items():
            arrays[name + "." + k] = a
    else:
        for i, d in enumerate(r[0]):
            for k, a in d.items():
                arrays["%%s.%%d.%%s" %% (name, i, k)] = a
        out[name + ".handoff"] = r[1]["handoff_n"]
np.savez(%(npz)r, **arrays)
print("RESULT " + json.dumps(out))
"""


@pytest.mark.gpu
@pytest.mark.parametrize("D", [4, 6, 5])
@pytest.mark.parametrize("lean", [False, True])
def test_forced_tile_shape_takes_21_bit_offsets(built, gpu, D, lean, tmp_path):
    """JDA_TILES is process-wide and read once, so a forced shape needs a fresh process.  100:57x1 makes the 100-pixel level
    of a 660 x 100 frame one tile 672 bytes wide in every dialect and depth: pixel mode 3 (T21), which the chooser itself
    picks for dialect C at depth 4 only.  The child's traces and detections are compared here with the oracle, bit for bit."""
    import json
    import subprocess
    import sys
    from jda_amd import api
    cs = EXTRA_CASES["forced_T21_%sdepth%d" % ("lean_" if lean else "", D)]
    inp = _inputs("forced_T21_%sdepth%d" % ("lean_" if lean else "", D))
    frames = inp["frames"]
    npz = str(tmp_path / "out.npz")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    script = TILES_SCRIPT % dict(root=root, model=inp["path"], n=cs["n_frames"], w=cs["frame"][0], h=cs["frame"][1], seed=cs["fseed"],
                                 c_kw=cs["c_kw"], cpp_kw=cs["cpp_kw"], npz=npz)
    r = subprocess.run([sys.executable, "-c", script], env=dict(os.environ, JDA_TILES="100:57x1", JDA_DENSE="0"), capture_output=True,
                       text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    out = json.loads([l for l in r.stdout.splitlines() if l.startswith("RESULT ")][-1][7:])
    print(out)
    depth = D if D in (4, 6) else 0
    for call, dial, trace in (("trace", "C", True), ("detect", "C", False), ("trace_cpp", "CPP", True), ("detect_cpp", "CPP", False)):
        assert {tuple(k): v for k, v in out[call]} == {tuple(api.ScanForm("k_scan", dial, depth, "T21", False, lean and not trace, trace, True)): 1}, (call, out[call])
    got = np.load(npz)
    for call, key in (("trace", "trace_c"), ("trace_cpp", "trace_cpp")):
        _same_trace(inp[key], {k: got[call + "." + k] for k in ("carts_n", "score", "path_hash", "shapes")}, call)
    for call, key, keys in (("detect", "det_c", ("bboxes", "scores", "shapes")), ("detect_cpp", "det_cpp", ("rects", "scores", "shapes"))):
        for i, want in enumerate(inp[key]):
            for k in keys:
                assert same(want[k], got["%s.%d.%s" % (call, i, k)]), (call, i, k)
    for call, key in (("detect", "trace_c"), ("detect_cpp", "trace_cpp")):
        carts = np.concatenate([t["carts_n"] for t in inp[key]])
        assert out[call + ".handoff"] == int((carts > 20).sum()) > 0, call


# ---------------------------------------------------------------- the ragged instantiations, one small job each

def _ragged_case(D, sizes, kernel, pix, merged, lean=False, kw=None, cpp_kw=None, env=None, dialects=("C", "CPP"), tiles=None):
    return dict(D=D, sizes=sizes, kernel=kernel, pix=pix, merged=merged, lean=lean, kw=dict(kw or C_LEVEL), cpp_kw=dict(cpp_kw or CPP_LEVEL),
                env=dict(env or {}), dialects=dialects, tiles=tiles)


BIG_TILES = [(150, 98), (146, 94), (150, 98), (138, 90)]         # 27 x 14 windows and a little less: tiles of more than 256 windows
SMALL_TILES = [(106, 78), (102, 74), (106, 78), (98, 70)]        # 16 x 9 windows and a little less
GLB_LEVEL = dict(scale=1.25, min_size=100, max_size=120)         # the 110-pixel level alone: too large for an LDS tile
GLB_LEVEL_CPP = dict(minimum_size=110, step=11, factor=8.0)
GLB_SIZES = [(330, 132), (286, 121), (330, 143), (264, 110)]
PER_LEVEL = {"JDA_MERGE_BLOCKS": "0"}                             # a chunk this small is one merged launch otherwise
SCAN_P = {"JDA_MERGE_BLOCKS": "0", "JDA_SCAN_P": "2"}
RAGGED_CASES = {}
for _D in (4, 6, 5):
    for _lean in (False, True):
        _t = "_lean" if _lean else ""
        # one level of its own occupancy class: a launch of that level alone, cut for the largest tile an image has
        RAGGED_CASES["per_level_512_depth%d%s" % (_D, _t)] = _ragged_case(_D, BIG_TILES, "k_scan", "T16_512", False, _lean, env=PER_LEVEL)
        RAGGED_CASES["per_level_256_depth%d%s" % (_D, _t)] = _ragged_case(_D, SMALL_TILES, "k_scan", "T16_256", False, _lean, env=PER_LEVEL)
        RAGGED_CASES["merged_depth%d%s" % (_D, _t)] = _ragged_case(_D, BIG_TILES, "k_scan", "T16_256", True, _lean)       # (a merged launch is 256 threads)
        RAGGED_CASES["glb_depth%d%s" % (_D, _t)] = _ragged_case(_D, GLB_SIZES, "k_scan", "GLB", True, _lean, kw=GLB_LEVEL, cpp_kw=GLB_LEVEL_CPP)
        # the persistent form's RAGGED instantiations (dialect C), 768 threads and 256
        RAGGED_CASES["scan_p_depth%d%s" % (_D, _t)] = _ragged_case(_D, BIG_TILES, "k_scan_p", "T16_512", False, _lean, env=SCAN_P, dialects=("C",))
        RAGGED_CASES["scan_p_256_depth%d%s" % (_D, _t)] = _ragged_case(_D, BIG_TILES, "k_scan_p", "T16_256", False, _lean, dialects=("C",),
                                                                       env=dict(SCAN_P, JDA_SCAN_P_BLOCK="256"))


@functools.lru_cache(maxsize=None)
def _ragged_case_inputs(name):
    import tempfile
    from jda_amd import synth
    from oracle import build as oracle_build
    from oracle.pyoracle import Oracle
    oracle_build.build_oracle()
    cs = RAGGED_CASES.get(name) or RAGGED_CHILD_CASES[name]
    m = synth.make_model(2, 40, 5, cs["D"], seed=5, norm_every=10 ** 6 if cs["lean"] else 5)
    _gates(m, 1.6)
    d = tempfile.mkdtemp(prefix="scan_forms_")
    atexit.register(shutil.rmtree, d, True)
    path = os.path.join(d, name + ".model")
    m.save(path, 8)
    imgs = [synth.make_frames(1, w, h, seed=40 + i)[0] for i, (w, h) in enumerate(cs["sizes"])]
    o = Oracle(path)
    out = dict(path=path, imgs=imgs, model=m)
    for dial in cs["dialects"]:
        if dial == "C":
            out["det_C"] = [o.detect(im, **cs["kw"]) for im in imgs]; out["trace_C"] = [o.trace(im, want_shapes=False, **cs["kw"]) for im in imgs]
        else:
            out["det_CPP"] = [o.detect_cpp(im, **cs["cpp_kw"]) for im in imgs]; out["trace_CPP"] = [o.trace_cpp(im, **cs["cpp_kw"]) for im in imgs]
    o.close()
    return out


def _ragged_conditions(name):
    """From the level lists and the oracle: every image has the one level of the case and a different grid; the scan hands
    windows on and rejects some; the lean cases' models normalise nowhere in the scanned range, the others do."""
    from jda_amd import synth
    cs = RAGGED_CASES.get(name) or RAGGED_CHILD_CASES[name]
    inp = _ragged_case_inputs(name)
    lv = [synth.levels_c(w, h, **cs["kw"])[0] for w, h in cs["sizes"]]
    assert all(len(l) == 1 for l in lv) and len({l[0]["win"] for l in lv}) == 1, (name, lv)
    lp = [synth.levels_cpp(w, h, **cs["cpp_kw"])[0] for w, h in cs["sizes"]]
    assert all(len(l) == 1 and (l[0]["win"], l[0]["step"]) == (lv[0][0]["win"], lv[0][0]["step"]) for l in lp), (name, lp)
    assert len({(l[0]["nx"], l[0]["ny"]) for l in lv}) >= 3, name
    n_max = max(l[0]["nx"] * l[0]["ny"] for l in lv)
    if cs["pix"] == "GLB":
        assert lv[0][0]["win"] > 100
    elif cs["kernel"] == "k_scan" and not cs["merged"]:
        assert (n_max > 256) == (cs["pix"] == "T16_512") and n_max <= 512, (name, n_max)      # the whole grid of an image is one tile at most
    m = inp["model"]
    assert bool(((m.cmean[0] != 0) | (m.cstd[0] != 1)).any()) == (not cs["lean"]), name
    out = {}
    for dial in cs["dialects"]:
        carts = np.concatenate([t["carts_n"] for t in inp["trace_" + dial]])
        out[dial] = dict(windows=len(carts), handoff=int((carts > 40).sum()), scan_carts=int(np.minimum(carts, 40).sum()), total=int(carts.sum()))
        assert 0 < out[dial]["handoff"] < len(carts), (name, dial)
    return out


@pytest.mark.parametrize("name", sorted(RAGGED_CASES))
def test_ragged_case_inputs_meet_their_conditions(built, name):
    _ragged_conditions(name)


def _ragged_expected(cs, dialect):
    from jda_amd import api
    return {api.ScanForm(cs["kernel"], dialect, cs["D"] if cs["D"] in (4, 6) else 0, cs["pix"], True, cs["lean"], False, cs["merged"]): 1}


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(RAGGED_CASES))
def test_ragged_instantiation_vs_oracle(built, gpu, name):
    cs, inp = RAGGED_CASES[name], _ragged_case_inputs(name)
    cond = _ragged_conditions(name)
    c = _cascador(inp["path"], dict(cs["env"], JDA_DENSE="0"))
    try:
        for dial in cs["dialects"]:
            for rep in range(2):
                if dial == "C":
                    (dets, st), f = _forms(c, c.detect_ragged, inp["imgs"], stats=True, **cs["kw"])
                    keys = ("bboxes", "scores", "shapes")
                else:
                    (dets, st), f = _forms(c, c.detect_ragged_cpp, inp["imgs"], stats=True, **cs["cpp_kw"])
                    keys = ("rects", "scores", "shapes")
                print("RAGGED_CASE", name, dial, sorted((tuple(k), v) for k, v in f.items()))
                assert f == _ragged_expected(cs, dial), (name, dial, f)
                for want, g in zip(inp["det_" + dial], dets):
                    for k in keys:
                        assert same(want[k], g[k]), (name, dial, k)
                _same_counters(st, cond[dial], name)
    finally:
        c.close()


# ... and the ragged forms that need a forced tile shape, in a child process (JDA_TILES): T21, and a tile origin 15 bytes
# past a 16-byte boundary (57-pixel windows 5 pixels apart in tiles 19 windows wide: the second tile column starts at byte 95)
T21_LEVEL = dict(scale=4.17, min_size=25, max_size=100)
T21_LEVEL_CPP = dict(minimum_size=100, step=10, factor=8.0)
L57_LEVEL = dict(scale=1.25, min_size=50, max_size=60)
L57_LEVEL_CPP = dict(minimum_size=57, step=5, factor=8.0)
RAGGED_CHILD_CASES = {}
for _D in (4, 6, 5):
    RAGGED_CHILD_CASES["T21_depth%d" % _D] = _ragged_case(_D, [(660, 100), (670, 100), (660, 109), (680, 100)], "k_scan", "T21", True,
                                                          kw=T21_LEVEL, cpp_kw=T21_LEVEL_CPP, tiles="100:57x1")
    RAGGED_CHILD_CASES["T21_lean_depth%d" % _D] = _ragged_case(_D, [(660, 100), (670, 100), (660, 109), (680, 100)], "k_scan", "T21", True, True,
                                                               kw=T21_LEVEL, cpp_kw=T21_LEVEL_CPP, tiles="100:57x1")
RAGGED_CHILD_CASES["lead_in_15"] = _ragged_case(4, [(242, 72), (242, 77), (247, 72), (242, 82)], "k_scan", "T16_256", True,
                                                kw=L57_LEVEL, cpp_kw=L57_LEVEL_CPP, tiles="57:19x4")

RAGGED_CHILD_SCRIPT = r"""
import json, sys
sys.path.insert(0, %(root)r)
import numpy as np
from jda_amd import api, synth
c = api.Cascador(%(model)r)
imgs = [synth.make_frames(1, w, h, seed=40 + i)[0] for i, (w, h) in enumerate(%(sizes)r)]
out, arrays = {}, {}
for name, call in (("C", lambda: c.detect_ragged(imgs, stats=True, **%(kw)r)), ("CPP", lambda: c.detect_ragged_cpp(imgs, stats=True, **%(cpp_kw)r))):
    before = c.scan_forms()
    dets, st = call()
    out[name] = [[list(k), v - before.get(k, 0)] for k, v in c.scan_forms().items() if v != before.get(k, 0)]
    out[name + ".stats"] = {k: st[k] for k in ("scan_patch_n", "patch_n", "handoff_n", "scan_cart_n", "cart_total_n", "scan_fallbacks", "dense_passes")}
    for i, d in enumerate(dets):
        for k, a in d.items():
            arrays["%%s.%%d.%%s" %% (name, i, k)] = a
np.savez(%(npz)r, **arrays)
print("RESULT " + json.dumps(out))
"""


def test_ragged_child_inputs_meet_their_conditions(built):
    from jda_amd import synth
    for name, cs in RAGGED_CHILD_CASES.items():
        _ragged_conditions(name)
        lv = [synth.levels_c(w, h, **cs["kw"])[0][0] for w, h in cs["sizes"]]
        win, tw = [int(x) for x in cs["tiles"].replace("x", ":").split(":")][:2]
        assert all(l["win"] == win for l in lv)
        if name == "lead_in_15":
            # every image has at least two columns of the forced tile, and the second one starts 15 bytes past a 16-byte boundary
            assert all(l["nx"] > tw for l in lv) and (tw * lv[0]["step"]) % 16 == 15
        else:
            # the forced tile's row (15 bytes of lead-in, the ragged chooser's worst case) takes offsets past 16 bits
            pitch = (15 + win + (tw - 1) * lv[0]["step"] + 15) & ~15
            assert (win - 1) * pitch + win - 1 + 15 > 65535 and all(l["nx"] >= tw for l in lv)


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(RAGGED_CHILD_CASES))
def test_ragged_forced_tile_shapes_vs_oracle(built, gpu, name, tmp_path):
    import json
    import subprocess
    import sys
    cs, inp = RAGGED_CHILD_CASES[name], _ragged_case_inputs(name)
    cond = _ragged_conditions(name)
    npz = str(tmp_path / "out.npz")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    script = RAGGED_CHILD_SCRIPT % dict(root=root, model=inp["path"], sizes=cs["sizes"], kw=cs["kw"], cpp_kw=cs["cpp_kw"], npz=npz)
    r = subprocess.run([sys.executable, "-c", script], env=dict(os.environ, JDA_TILES=cs["tiles"], JDA_DENSE="0"), capture_output=True,
                       text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    out = json.loads([l for l in r.stdout.splitlines() if l.startswith("RESULT ")][-1][7:])
    print("RAGGED_CHILD", name, out)
    got = np.load(npz)
    for dial, keys in (("C", ("bboxes", "scores", "shapes")), ("CPP", ("rects", "scores", "shapes"))):
        assert {tuple(k): v for k, v in out[dial]} == {tuple(k): v for k, v in _ragged_expected(cs, dial).items()}, (name, dial, out[dial])
        for i, want in enumerate(inp["det_" + dial]):
            for k in keys:
                assert same(want[k], got["%s.%d.%s" % (dial, i, k)]), (name, dial, i, k)
        _same_counters(out[dial + ".stats"], cond[dial], name)
