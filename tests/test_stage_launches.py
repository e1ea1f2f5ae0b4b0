"""Which k_stage instantiations a dense pass launched (jdaStageLaunches / jdaStageLaunchFor, include/jda.h, DESIGN.md
section 8d), and k_stage at the limits of its own loops.

CPU half: the launch choice (register width ACC of the regression sums, LDS tile or global pixels, cart chunk, dynamic LDS)
is restated here from DESIGN.md section 8d and the header comment and swept against Cascador.stage_launch_for over
dialects, shape dimensions, tree depths, cart counts and levels (test_launch_choice_sweep).

GPU half: every case names the StageLaunch keys (dialect, trace, glb, acc, chunk) it is about -- derived from the
restatement, never read back from the run -- takes the difference of stage_launches() around EACH call and asserts it is
exactly those keys, T x (levels of that kind) each, with finish_forms() showing DENSE alone.  What a case compares, bit for
bit (`same`), against the CPU oracle in dialect C and dialect CPP:
  * trace() / trace_cpp(): carts walked, score, leaf-path hash and shape per window,
  * detect_batch() / detect_batch_cpp(): the detections, and patch_n, cart_total_n, stage_done_n, face_patch_n against what
    the oracle's trace says they are.
Every case runs on a cascador with dense = 2 and then again with dense = 0, wide_max = 0 (k_finish): the same bits, no
k_stage launch.  The conditions a case's inputs must meet are evaluated from the oracle's trace
(test_inputs_meet_their_conditions, no GPU needed) and again by the GPU case before it looks at a GPU result."""
import atexit
import functools
import os
import shutil

import numpy as np
import pytest

from conftest import same, bits

LDS_MAX = 160 * 1024        # host.h: Knobs::dense_lds_max
PIX_MAX = 16 * 1024         # host.h: Knobs::dense_pix
TIERS = (32768, 40960, 53248, 81920, 163840)     # 5, 4, 3, 2, 1 workgroups on a CU
TILE = 16                   # k_stage.hip: kDenseTw = kDenseTh
ACCS = (12, 32, 64, 160)
CHUNKS = (4, 8, 16, 32, 64)
RB = {"C": 4, "CPP": 8}
NODE_BYTES = {4: 32, 8: 48}  # kernels.h: NodeF, NodeD


# ---------------------------------------------------------------- the host's decisions restated

def acc_of(dim):
    return next(a for a in ACCS if a >= dim)


def lds_total(pix_bytes, dim, D, chunk, rb):
    """k_stage's LDS: pixel tile, the tile's shapes [dim][256], then per chunk node records, leaf scores, cart
    parameters and weight rows + one register row of slack; each part padded to 16 bytes."""
    node_n, leaf_n, pad = (1 << (D - 1)) - 1, 1 << (D - 1), lambda b: (b + 15) & ~15
    return (pad(pix_bytes) + dim * TILE * TILE * rb + chunk * node_n * NODE_BYTES[rb] + pad(chunk * leaf_n * rb) + chunk * 4 * rb +
            pad((chunk * leaf_n * dim + acc_of(dim)) * rb))


def lds_floor(dim, D, rb):
    return lds_total(0, dim, D, 4, rb)


def model_ok(L, D, rb):
    """Pass::dense_ok's conditions on the model: dim <= 160, leaf_n <= 256, the LDS floor within 160 KB."""
    return 2 * L <= 160 and (1 << (D - 1)) <= 256 and lds_floor(2 * L, D, rb) <= LDS_MAX


def tile_bytes(win, step):
    """-> (row pitch, bytes) of the padded pixel tile of 16 x 16 windows: rows of a multiple of 16, never of 128, bytes."""
    side = win + (TILE - 1) * step
    pitch = (side + 15) & ~15
    if pitch % 128 == 0:
        pitch += 16
    return pitch, pitch * side


def chunk_of(pix_bytes, dim, D, rb):
    fits = lambda ch, budget: lds_total(pix_bytes, dim, D, ch, rb) <= min(budget, LDS_MAX)
    for tier in TIERS[:3]:                       # >= 3 workgroups a CU: the smallest tier that holds a 16-cart chunk, grown
        if fits(16, tier):
            return max(ch for ch in (16, 32, 64) if all(fits(c2, tier) for c2 in (16, 32, 64) if c2 <= ch))
    for tier in TIERS:                           # else the smallest tier that holds any chunk, the longest that fits
        for ch in reversed(CHUNKS):
            if fits(ch, tier):
                return ch
    return 0


def choice(dial, L, D, win, step):
    """-> dict(glb, acc, chunk, lds, pitch) of the launch over a level, None where dense mode declines the model."""
    rb, dim = RB[dial], 2 * L
    if not model_ok(L, D, rb):
        return None
    pitch, need = tile_bytes(win, step)
    glb = need > max(0, min(PIX_MAX, LDS_MAX - lds_floor(dim, D, rb)))
    pix = 0 if glb else need
    ch = chunk_of(pix, dim, D, rb)
    return dict(glb=glb, acc=acc_of(dim), chunk=ch, lds=lds_total(pix, dim, D, ch, rb), pitch=pitch)


def key_of(dial, trace, ch):
    from jda_amd import api
    return api.StageLaunch(dial, bool(trace), ch["glb"], ch["acc"], ch["chunk"])


# ---------------------------------------------------------------- CPU: the sweep

SWEEP_L = (1, 5, 6, 7, 16, 17, 32, 33, 40, 68, 80, 81)
SWEEP_K = (1, 3, 4, 5, 64, 65, 130)
# (win, step): 24/2 and 46/4 tiles; 53/4 a tile of pitch 128 -> 144 and 16,272 bytes, 54/4 at 16,416 just beyond the 16 KB
# cap; 57/5 and 150/15 beyond it; 8/1 the smallest tile a large model's cap still holds
SWEEP_LEVELS = ((24, 2), (46, 4), (53, 4), (54, 4), (57, 5), (150, 15), (8, 1))
LARGEST = {("C", 2): 77, ("C", 5): 62, ("CPP", 2): 38, ("CPP", 5): 31}      # largest L accepted at depth D


@functools.lru_cache(maxsize=None)
def _sweep(built=True):
    """The library's answers over the sweep: {(dial, L, D, K, win, step): (key, lds) or None}, asserted against the restatement."""
    import tempfile
    from jda_amd import api, synth
    out = {}
    d = tempfile.mkdtemp(prefix="stage_sweep_")
    try:
        for L in SWEEP_L:
            for D in range(2, 11):                                 # D = 10: 512 leaves, the first depth declined
                for K in SWEEP_K if D <= 3 else (3,):              # (K never enters the choice: swept where the model is small)
                    m = synth.Model(1, K, L, D)
                    p = os.path.join(d, "m.model")
                    m.save(p, 8)
                    c = api.Cascador(p)
                    for dial in ("C", "CPP"):
                        for win, step in SWEEP_LEVELS:
                            for trace in (False, True):
                                r = c.stage_launch_for(dial, trace, win, step)
                                assert r is None or r[0].trace == trace and r[0].dialect == dial
                                out[(dial, L, D, K, win, step, trace)] = r
                    c.close()
    finally:
        shutil.rmtree(d, True)
    return out


def test_launch_choice_sweep(built):
    sw = _sweep()
    assert tile_bytes(53, 4) == (144, 16272) and tile_bytes(54, 4) == (144, 16416) and tile_bytes(46, 4)[0] == 112
    seen = set()
    for (dial, L, D, K, win, step, trace), r in sw.items():
        want = choice(dial, L, D, win, step)
        what = (dial, L, D, K, win, step, trace, r, want)
        # -1 exactly where dense_ok's stated conditions fail
        assert (r is None) == (want is None), what
        assert (r is None) == (2 * L > 160 or (1 << (D - 1)) > 256 or lds_floor(2 * L, D, RB[dial]) > LDS_MAX), what
        if r is None:
            continue
        k, lds = r
        assert lds <= 163840, what
        assert k.acc == min(a for a in ACCS if a >= 2 * L), what
        assert k.glb == (tile_bytes(win, step)[1] > min(PIX_MAX, LDS_MAX - lds_floor(2 * L, D, RB[dial]))), what
        assert k.chunk in CHUNKS, what
        assert (k.glb, k.acc, k.chunk, lds) == (want["glb"], want["acc"], want["chunk"], want["lds"]), what
        seen.add(k)
    # every (dialect, trace, glb, acc) and every chunk class is reachable (DESIGN.md section 8d lists none as unreachable)
    assert {(k.dialect, k.trace, k.glb, k.acc) for k in seen} == {(d, t, g, a) for d in RB for t in (False, True) for g in (False, True) for a in ACCS}
    assert {(k.dialect, k.chunk) for k in seen} == {(d, c) for d in RB for c in CHUNKS}
    # the largest shape accepted per dialect at D = 2 and D = 5 (the first declined: one landmark more): the LDS floor
    # declines before dim <= 160 can (dim 156 / 78 already), so that condition never decides
    for (dial, D), L in LARGEST.items():
        assert model_ok(L, D, RB[dial]) and not model_ok(L + 1, D, RB[dial]), (dial, D, L)
        assert max(l for l in range(1, 100) if model_ok(l, D, RB[dial])) == L
    for dial in RB:
        assert max(D for D in range(2, 12) if model_ok(1, D, RB[dial])) == 9        # leaf_n = 256 is the deepest accepted
        assert max(l for l in range(1, 100) if model_ok(l, 9, RB[dial])) == {"C": 12, "CPP": 5}[dial]      # ... with this many landmarks
    # the library agrees at those edges (12 / 5 landmarks at D = 9 are outside SWEEP_L)
    import tempfile
    from jda_amd import api, synth
    with tempfile.TemporaryDirectory() as d:
        for dial, D, L in [(dl, D, L) for (dl, D), L in LARGEST.items()] + [("C", 9, 12), ("CPP", 9, 5)]:
            for l, accepted in ((L, True), (L + 1, False)):
                synth.Model(1, 3, l, D).save(os.path.join(d, "m.model"), 8)
                c = api.Cascador(os.path.join(d, "m.model"))
                assert (c.stage_launch_for(dial, False, 24, 2) is not None) == accepted, (dial, D, l)
                c.close()


# ---------------------------------------------------------------- the cases

def c_level(win):
    """Dialect C scans `win`-pixel windows alone: one growth step from 24 pixels reaches any size."""
    if win == 24:
        return dict(scale=1.25, min_size=24, max_size=24)
    scale = float(np.float32((win + 0.5) / 24.0))
    assert int(np.float32(24) * np.float32(scale)) == win
    return dict(scale=scale, min_size=win, max_size=win)


def frame_for(win, step, nx, ny):
    return win + (nx - 1) * step, win + (ny - 1) * step


# calls: (n_frames, width, height, dialect C's scan, dialect CPP's scan)
MIX = (1, 112, 80, dict(scale=1.25, min_size=40, max_size=60), dict(minimum_size=24, step=5, factor=2.4))
#   C: 46-pixel windows (tile) + 57 (global); CPP: 24 (tile) + 57 (global); the frame's rows are a multiple of 16 bytes
SMALL = (1, 88, 56, c_level(24), dict(minimum_size=24, step=2, factor=100.0))
#   33 x 17 windows of 24 pixels: tiles of 16 x 16, 1 x 16, 16 x 1 and 1 x 1 windows; rows of 88 bytes (load_tile's fallback)
NINE = (9,) + SMALL[1:]
EIGHT = (8,) + SMALL[1:]
ONE = (1, 24, 24, c_level(24), dict(minimum_size=24, step=2, factor=100.0))                         # 1 x 1 windows
SQUARE = (1, 54, 54, c_level(24), dict(minimum_size=24, step=2, factor=100.0))                      # 16 x 16 windows
BUMP = (1, 117, 54, c_level(40), dict(minimum_size=53, step=4, factor=1.02))
#   CPP: 17 x 1 windows of 53 pixels (tile, pitch 128 -> 144, 112 bytes under the cap) and 16 x 1 of 54 (32 bytes over it)
TINY = (1, 40, 30, c_level(24), dict(minimum_size=8, step=1, factor=100.0))                         # CPP: 8-pixel windows, 33 x 23


def _case(dims, calls=(MIX, SMALL), cart_th=-1.2, norm_every=3, seed=3, cond=(), opts=None, th=None, dials=("C", "CPP"), ticket=False,
          gates=None):
    """dims: (T, K, L, D), or {dialect: (T, K, L, D)}; K may be a function of the cart chunk of the case's FIRST call's
    first level (taken from the key).  th: "cut" = dialect C's final threshold is put among the survivors' scores.
    gates: (stage, cart or a function of (chunk, K), share kept) in walk order -- carts whose thresholds are read from the
    oracle (_gates)."""
    if not isinstance(dims, dict):
        dims = dict(C=dims, CPP=dims)
    return dict(dims=dims, calls=tuple(calls), cart_th=cart_th, norm_every=norm_every, seed=seed, cond=tuple(cond), opts=dict(opts or {}),
                th=th, dials=tuple(dials), ticket=ticket, gates=tuple(gates or ()))


CASES = {}
# ---- 1. every instantiation: models at 5 .. 33 landmarks (ACC boundaries dim 12 | 14, 32 | 34, 64 | 66: at the boundary a
#         row read ends with the table, one above it runs into the slack and the next rows) and the largest accepted; depths
#         chosen so that every chunk class is met; D = 9 (256 leaves) is the deepest accepted
CASES["inst_L5"] = _case(dict(C=(2, 6, 5, 2), CPP=(2, 6, 5, 9)))
CASES["inst_L6"] = _case(dict(C=(2, 6, 6, 9), CPP=(2, 6, 6, 5)))
CASES["inst_L7"] = _case(dict(C=(2, 6, 7, 6), CPP=(2, 6, 7, 4)))
CASES["inst_L16"] = _case(dict(C=(2, 10, 16, 4), CPP=(2, 10, 16, 3)))
CASES["inst_L17"] = _case(dict(C=(2, 6, 17, 3), CPP=(2, 6, 17, 2)), calls=(MIX, SMALL, TINY))
CASES["inst_L32"] = _case(dict(C=(2, 6, 32, 3), CPP=(2, 6, 32, 2)), calls=(MIX, SMALL, TINY))
CASES["inst_L33"] = _case(dict(C=(2, 6, 33, 2), CPP=(2, 6, 33, 2)), calls=(MIX, SMALL, TINY))
CASES["inst_largest_D2"] = _case(dict(C=(2, 6, LARGEST[("C", 2)], 2), CPP=(2, 6, LARGEST[("CPP", 2)], 2)), calls=(MIX, SMALL, TINY))
CASES["inst_largest_D5"] = _case(dict(C=(2, 6, LARGEST[("C", 5)], 5), CPP=(2, 6, LARGEST[("CPP", 5)], 5)), calls=(SMALL,))
CASES["chunk_a"] = _case(dict(C=(2, 70, 7, 2), CPP=(2, 70, 1, 2)), calls=(SMALL,), cart_th=-3.6)       # 64-cart chunks
CASES["chunk_b"] = _case(dict(C=(2, 40, 7, 3), CPP=(2, 40, 1, 4)), calls=(SMALL,), cart_th=-2.0)       # 32
CASES["chunk_c"] = _case(dict(C=(2, 20, 7, 4), CPP=(2, 20, 7, 6)), calls=(SMALL, MIX), cart_th=-1.6)   # 16 / 8
# ---- 2. dense_ok's edge: the first shape / depth it declines runs window by window
CASES["declined_dim"] = _case(dict(C=(2, 6, LARGEST[("C", 2)] + 1, 2), CPP=(2, 6, LARGEST[("CPP", 2)] + 1, 2)), calls=(SMALL,), cond=("declined",))
CASES["declined_leaves"] = _case((2, 3, 2, 10), calls=(SMALL,), cond=("declined",))
# ---- 3. the cart loops: a single partial group of G = 4; K = chunk; a last chunk of one cart; two chunks and a partial one
for _n, _K in (("1", 1), ("2", 2), ("3", 3), ("5", 5), ("chunk", lambda ch: ch), ("chunk_plus_1", lambda ch: ch + 1),
               ("2_chunks_plus_6", lambda ch: 2 * ch + 6)):
    CASES["carts_K_" + _n] = _case((2, _K, 5, 4), calls=(SMALL,), cart_th=0.0 if _n == "1" else (-0.9 if _n in "235" else -1.6), cond=("last_row",))
# ---- 4. rejection: where windows and whole tiles die; the final threshold among the survivors' scores; T = 4, nine frames
#         gates (their thresholds read from the oracle): the last cart of stage 0's second chunk keeps 30 windows of 5,049 -- whole
#         tiles die there --, then the last cart of stage 1, the first cart of a chunk in stage 2 and a cart of the last stage
CASES["reject"] = _case((4, lambda ch: 2 * ch + 6, 5, 4), calls=(NINE,), cart_th=-1.05, norm_every=5, cond=("reject",), th="cut",
                        gates=((0, lambda ch, K: 2 * ch - 1, 30), (1, lambda ch, K: K - 1, 0.85), (2, lambda ch, K: ch, 0.85), (3, 3, 0.85)))
# ---- 5. T = 1 (the stage is first and last), eight frames
CASES["T1"] = _case((1, 9, 5, 3), calls=(EIGHT, MIX), cart_th=-0.8)
# ---- 6. tiles: 1 x 1 and 16 x 16 windows; 17 x 1 on the pitch bump under the cap next to a level just over it
CASES["tiles"] = _case((2, 9, 5, 3), calls=(ONE, SQUARE, BUMP), cart_th=-1.0)
# ---- 7. two lanes; a ticket
CASES["lanes"] = _case((2, 9, 5, 3), calls=(NINE,), cart_th=-1.0, opts=dict(lanes=2, lanes_min_windows=1), cond=("lanes",))
CASES["ticket"] = _case((2, 9, 5, 3), calls=(NINE,), cart_th=-1.0, dials=("C",), ticket=True)


def _levels(dial, call):
    from jda_amd import synth
    n, w, h, ckw, pkw = call
    return synth.levels_c(w, h, **ckw)[0] if dial == "C" else synth.levels_cpp(w, h, **pkw)[0]


def _dims(name, dial):
    """The case's model in a dialect; K from the cart chunk of the first call's first level where the case asks for that."""
    T, K, L, D = CASES[name]["dims"][dial]
    if callable(K):
        lv = _levels(dial, CASES[name]["calls"][0])[0]
        K = K(choice(dial, L, D, lv["win"], lv["step"])["chunk"])
    return T, K, L, D


def expected(name, dial, call, trace):
    """{StageLaunch: count} of one dense pass over a call: T launches per level under the level's key."""
    T, K, L, D = _dims(name, dial)
    out = {}
    for lv in _levels(dial, call):
        ch = choice(dial, L, D, lv["win"], lv["step"])
        if ch is None:
            assert "declined" in CASES[name]["cond"], (name, dial, lv)        # only the cases that say so may be declined
            return {}
        k = key_of(dial, trace, ch)
        out[k] = out.get(k, 0) + T
    return out


def test_cases_cover_every_reachable_instantiation_and_chunk_class():
    """From the restatement alone: the keys the GPU cases assert, taken together, are every (dialect, trace, glb, acc) and every
    chunk class the sweep finds reachable -- all 32 and all five per dialect."""
    keys = set()
    for name, cs in CASES.items():
        for dial in cs["dials"]:
            for call in cs["calls"]:
                for trace in (False, True):
                    keys |= set(expected(name, dial, call, trace))
    missing = {(d, t, g, a) for d in RB for t in (False, True) for g in (False, True) for a in ACCS} - {(k.dialect, k.trace, k.glb, k.acc) for k in keys}
    assert not missing, sorted(missing)
    assert {(k.dialect, k.chunk) for k in keys} == {(d, c) for d in RB for c in CHUNKS}, sorted({(k.dialect, k.chunk) for k in keys})
    # the cart-loop cases take K from the chunk of their level, whatever it is
    for dial in RB:
        ch = choice(dial, 5, 4, 24, 2)["chunk"]
        assert [_dims("carts_K_" + n, dial)[1] for n in ("chunk", "chunk_plus_1", "2_chunks_plus_6")] == [ch, ch + 1, 2 * ch + 6] and ch in CHUNKS
    for dial in RB:
        lv = _levels(dial, BUMP)
        if dial == "CPP":
            assert [(l["win"], l["nx"], l["ny"]) for l in lv] == [(53, 17, 1), (54, 16, 1)]
        assert [(l["nx"], l["ny"]) for l in _levels(dial, SMALL)] == [(33, 17)] and [(l["nx"], l["ny"]) for l in _levels(dial, ONE)] == [(1, 1)]
        assert [(l["nx"], l["ny"]) for l in _levels(dial, SQUARE)] == [(16, 16)]


@functools.lru_cache(maxsize=None)
def _inputs(name):
    """Model files, frames and the oracle's traces and detections of a case: computed once, shared by the CPU and the GPU test."""
    import tempfile
    from jda_amd import synth
    from oracle import build as oracle_build
    from oracle.pyoracle import Oracle
    oracle_build.build_oracle()
    cs = CASES[name]
    d = tempfile.mkdtemp(prefix="stage_launches_")
    atexit.register(shutil.rmtree, d, True)
    out = {}
    for dial in cs["dials"]:
        T, K, L, D = _dims(name, dial)
        m = synth.make_model(T, K, L, D, seed=cs["seed"], cart_th=cs["cart_th"], norm_every=min(cs["norm_every"], K))
        path = os.path.join(d, "%s_%s.model" % (name, dial))
        m.save(path, 8)
        if cs["gates"]:
            m.cth[1:] = float(np.float32(synth.NEG_BIG))          # behind stage 0 only the gates reject
            _gates(name, dial, m, path)
        o = Oracle(path)
        calls = []
        try:
            for call in cs["calls"]:
                n, w, h, ckw, pkw = call
                kw = ckw if dial == "C" else pkw
                frames = synth.make_frames(n, w, h, seed=7)
                tr = [o.trace(f, **kw) if dial == "C" else o.trace_cpp(f, **kw) for f in frames]
                carts, score = np.concatenate([t["carts_n"] for t in tr]), np.concatenate([t["score"] for t in tr])
                walked = (carts == T * K) & (score >= m.cth[T - 1, K - 1])
                th = -0.5
                if cs["th"] == "cut" and dial == "C":
                    s = np.sort(score[walked])
                    assert len(s) >= 4 and s[0] < s[-1], (name, len(s))
                    th = float(np.float32((float(s[len(s) // 2 - 1]) + float(s[len(s) // 2])) / 2))
                dkw = dict(kw, th=th) if dial == "C" else kw
                det = [o.detect(f, **dkw) if dial == "C" else o.detect_cpp(f, **kw) for f in frames]
                faces = walked & (score >= np.float32(th)) if dial == "C" else walked
                nb = dict(windows=len(carts), total=int(carts.sum()), faces=int(faces.sum()), walked=walked, carts=carts, score=score,
                          done=[int((carts > (t + 1) * K).sum()) for t in range(T - 1)] + [int(walked.sum())])
                calls.append(dict(call=call, frames=frames, kw=kw, dkw=dkw, trace=tr, det=det, nb=nb, th=th))
        finally:
            o.close()
        out[dial] = dict(path=path, model=m, calls=calls)
    return out


def _gates(name, dial, m, path):
    """The gate carts of a case, in walk order: each is first made to reject everybody, the oracle reports the score every
    window has there (the case's first call), and its threshold becomes the score that keeps the wanted share (a count
    where it is 1 or more) of those that reach it.  So the oracle alone decides the inputs before anything runs on a GPU."""
    from jda_amd import synth
    from oracle.pyoracle import Oracle
    cs = CASES[name]
    T, K, L, D = _dims(name, dial)
    n, w, h, ckw, pkw = cs["calls"][0]
    lv = _levels(dial, cs["calls"][0])[0]
    ch = choice(dial, L, D, lv["win"], lv["step"])["chunk"]
    frames = synth.make_frames(n, w, h, seed=7)
    for t, k, keep in cs["gates"]:
        k = k(ch, K) if callable(k) else k
        m.cth[t, k] = 1e30
        m.save(path, 8)
        o = Oracle(path)
        tr = [o.trace(f, want_shapes=False, **ckw) if dial == "C" else o.trace_cpp(f, **pkw) for f in frames]
        o.close()
        carts, score = np.concatenate([x["carts_n"] for x in tr]), np.concatenate([x["score"] for x in tr])
        sc = np.sort(score[carts == t * K + k + 1])[::-1]           # the scores of the windows that reach the gate, best first
        n_keep = int(keep) if keep >= 1 else int(len(sc) * keep)
        assert 1 <= n_keep < len(sc), (name, dial, t, k, len(sc))
        while n_keep > 1 and sc[n_keep - 1] == sc[n_keep]:          # (a tie: both sides of the threshold must differ)
            n_keep -= 1
        th = float(np.float32((float(sc[n_keep - 1]) + float(sc[n_keep])) / 2))
        m.cth[t, k] = th if sc[n_keep - 1] >= th > sc[n_keep] else float(sc[n_keep - 1])
    m.save(path, 8)


def _tiles(call, dial):
    """Per window of a one-level call: the index of its (frame, 16 x 16 tile)."""
    (lv,) = _levels(dial, call)
    iy, ix = np.mgrid[0:lv["ny"], 0:lv["nx"]]
    tile = ((iy // TILE) * ((lv["nx"] + TILE - 1) // TILE) + ix // TILE).ravel()
    per = int(tile.max()) + 1
    return np.concatenate([tile + f * per for f in range(call[0])])


def _check_conditions(name):
    cs, inp = CASES[name], _inputs(name)
    for dial in cs["dials"]:
        T, K, L, D = _dims(name, dial)
        m = inp[dial]["model"]
        if "declined" not in cs["cond"]:
            # every case, over its calls: windows die, windows pass everything, and (T > 1) some die in a later stage
            carts = np.concatenate([c["nb"]["carts"] for c in inp[dial]["calls"]])
            walked = np.concatenate([c["nb"]["walked"] for c in inp[dial]["calls"]])
            assert (~walked).any() and walked.any(), (name, dial, int(walked.sum()), len(walked))
            if T > 1:
                assert ((carts > K) & ~walked).any(), (name, dial)
        for i, c in enumerate(inp[dial]["calls"]):
            nb = c["nb"]
            carts, walked = nb["carts"], nb["walked"]
            print("%s %s call %d: %d windows, stage survivors %s, %d detections" % (name, dial, i, nb["windows"], nb["done"], nb["faces"]))
            if "declined" in cs["cond"]:
                assert all(choice(dial, L, D, lv["win"], lv["step"]) is None for lv in _levels(dial, c["call"])), (name, dial)
                continue
            assert all(choice(dial, L, D, lv["win"], lv["step"]) is not None for lv in _levels(dial, c["call"])), (name, dial, "declined")
            if "last_row" in cs["cond"]:
                # every leaf of cart K - 1 has a weight row that moves a coordinate by more than an ulp of a value in [0, 1)
                assert (np.abs(m.w[:, (K - 1) * m.leaf_n:K * m.leaf_n]).max(axis=2) > 1e-6).all(), (name, dial)
            if cs["th"] == "cut" and dial == "C":
                assert 0 < nb["faces"] < int(walked.sum()), (name, nb["faces"], int(walked.sum()))
            if "reject" in cs["cond"]:
                (lv,) = _levels(dial, c["call"])
                ch = choice(dial, L, D, lv["win"], lv["step"])["chunk"]
                assert K == 2 * ch + 6 and T == 4
                g = carts - 1                                        # the cart that rejected a window that is not `walked`
                t, k, dead = g // K, g % K, ~walked
                normed = (m.cmean != 0.0) | (m.cstd != 1.0)
                assert normed[0, :K].any() and not normed[0, 0], name
                first_norm = int(np.argmax(normed[0]))
                n = dict(first_of_chunk=int((dead & (k % ch == 0)).sum()), last_of_chunk=int((dead & (k % ch == ch - 1)).sum()),
                         last_of_stage=int((dead & (k == K - 1)).sum()), last_stage=int((dead & (t == T - 1)).sum()),
                         before_norm=int((dead & (g < first_norm)).sum()), after_norm=int((dead & (g > first_norm)).sum()))
                tile = _tiles(c["call"], dial)
                n_tiles = int(tile.max()) + 1
                alive1 = np.bincount(tile, weights=(carts > K), minlength=n_tiles)          # alive at the entry of stage 1
                kept = np.bincount(tile, weights=walked, minlength=n_tiles)
                last_g = np.full(n_tiles, -1)
                np.maximum.at(last_g, tile, g)
                # a tile whose last window dies in a chunk that is not the stage's last one: the chunk loop breaks
                breaks = (kept == 0) & ((last_g % K) // ch < (K - 1) // ch)
                full = np.bincount(tile, minlength=n_tiles) == TILE * TILE                  # the tiles of 16 x 16 windows
                n.update(tiles_dead_at_stage_1=int((full & (alive1 == 0)).sum()), tiles_break=int((full & breaks).sum()),
                         tiles_keep_one=int((full & (kept == 1)).sum()), small_tiles_dead_at_stage_1=int((~full & (alive1 == 0)).sum()))
                print("   ", dial, n)
                assert all(v >= 1 for v in n.values()), (name, dial, n)
    return True


@pytest.mark.parametrize("name", sorted(CASES))
def test_inputs_meet_their_conditions(built, name):
    _check_conditions(name)


# ---------------------------------------------------------------- GPU

@pytest.fixture(scope="module")
def gpu():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    return torch.device("cuda", 0)


SEEN = set()          # every key a GPU case of this module counted


K_FINISH_FORMS = {"MERGED", "FILTER0", "MID_DIRECT", "TWO_LAUNCH"}      # the finishing forms made of k_finish / k_filter0 launches
FINISH = {}           # {FinishLaunch: count} of the last call _launches ran


def _launches(c, fn, *a, **kw):
    """-> (what the call returned, {StageLaunch: count} and {form: count} of its passes)."""
    b_l, b_f, b_k = c.stage_launches(), c.finish_forms(), c.finish_launches()
    r = fn(*a, **kw)
    a_l, a_f, a_k = c.stage_launches(), c.finish_forms(), c.finish_launches()
    assert all(a_l.get(k, 0) >= v for k, v in b_l.items())
    FINISH.clear()
    FINISH.update({k: v - b_k.get(k, 0) for k, v in a_k.items() if v != b_k.get(k, 0)})
    return r, {k: v - b_l.get(k, 0) for k, v in a_l.items() if v != b_l.get(k, 0)}, {k: a_f[k] - b_f[k] for k in a_f if a_f[k] != b_f[k]}


def _cascador(path, **options):
    from jda_amd import api
    c = api.Cascador(path)
    for k, v in options.items():
        c.set_option(k, v)
    return c


def _same_trace(want_frames, got, what):
    off = 0
    for i, r in enumerate(want_frames):
        n = len(r["carts_n"])
        for k in ("carts_n", "score", "path_hash", "shapes"):
            assert same(r[k], got[k][off:off + n]), (what, i, k, int((bits(r[k]) != bits(got[k][off:off + n])).sum()))
        off += n
    assert off == len(got["carts_n"]), what


def _same_detect(c_in, dets, st, dial, T, what):
    for want, g in zip(c_in["det"], dets):
        for k in ("bboxes", "scores", "shapes") if dial == "C" else ("rects", "scores", "shapes"):
            assert same(want[k], g[k]), (what, k)
    nb = c_in["nb"]
    assert st["patch_n"] == nb["windows"], (what, st["patch_n"], nb["windows"])
    assert st["cart_total_n"] == nb["total"], (what, st["cart_total_n"], nb["total"])
    assert list(st["stage_done_n"][:T]) == nb["done"], (what, list(st["stage_done_n"][:T]), nb["done"])
    assert st["face_patch_n"] == nb["faces"], (what, st["face_patch_n"], nb["faces"])


def _assert_keys(what, fl, ff, want, passes=1, queued=True, wide=False):
    """A dense call: exactly the expected keys, `passes` times each, and DENSE alone among the forms; a declined model (want
    empty): no k_stage launch and no DENSE."""
    print(what, sorted(fl.items()), ff)
    if want:
        assert fl == {k: v * passes for k, v in want.items()} and ff == {"DENSE": passes}, (what, fl, ff, want)
        assert FINISH == {}, (what, FINISH)
    else:
        # window by window: with wide_max = 0 the forms made of k_finish / k_filter0, and (queued: the oracle has windows that
        # pass all of stage 0, so the hand-off queue is not empty) launches of those kernels
        # (a model dense mode declines under dense = 2 keeps wide_max: it may take the whole-workgroup finisher instead)
        assert fl == {} and ff and "DENSE" not in ff and (wide or set(ff) <= K_FINISH_FORMS), (what, fl, ff)
        assert wide or (all(k.kernel in ("k_finish", "k_filter0") for k in FINISH) and (bool(FINISH) or not queued)), (what, FINISH)


def _run_dialect(name, dial, dense):
    import torch
    cs, inp = CASES[name], _inputs(name)[dial]
    T, K, L, D = _dims(name, dial)
    opts = dict(cs["opts"], dense=2) if dense else dict(cs["opts"], dense=0, wide_max=0)
    c = _cascador(inp["path"], **opts)
    try:
        assert c.stage_launches() == {}
        trace_fn, detect_fn = (c.trace, c.detect_batch) if dial == "C" else (c.trace_cpp, c.detect_batch_cpp)
        for i, ci in enumerate(inp["calls"]):
            what = "%s %s call %d dense=%d" % (name, dial, i, opts["dense"])
            passes = min(2, ci["call"][0]) if "lanes" in cs["cond"] else 1         # (two lanes: a pass each)
            queued = ci["nb"]["done"][0] > 0
            for trace in (True, False):
                want = expected(name, dial, ci["call"], trace) if dense else {}
                for lv in _levels(dial, ci["call"]):                                   # the library's own answer, level by level
                    ch, r = choice(dial, L, D, lv["win"], lv["step"]), c.stage_launch_for(dial, trace, lv["win"], lv["step"])
                    assert (r is None and ch is None) or r == (key_of(dial, trace, ch), ch["lds"]), (what, lv, r, ch)
                if trace:
                    got, fl, ff = _launches(c, trace_fn, ci["frames"], **ci["kw"])
                    _assert_keys(what + " trace", fl, ff, want, passes, queued, dense)
                    _same_trace(ci["trace"], got, what)
                elif cs["ticket"]:
                    def through_a_ticket():
                        f = torch.from_numpy(ci["frames"]).cuda()
                        return c.wait_batch(c.submit_batch_device(f, **ci["dkw"]), stats=True)
                    (dets, st), fl, ff = _launches(c, through_a_ticket)
                    _assert_keys(what + " ticket", fl, ff, want, 1, queued, dense)
                    _same_detect(ci, dets, st, dial, T, what)
                else:
                    (dets, st), fl, ff = _launches(c, detect_fn, ci["frames"], stats=True, **ci["dkw"])
                    _assert_keys(what + " detect", fl, ff, want, passes, queued, dense)
                    _same_detect(ci, dets, st, dial, T, what)
                    assert (st["dense_passes"] >= 1) == bool(want), (what, st["dense_passes"])
                if dense:
                    SEEN.update(fl)
        if not dense:
            assert c.stage_launches() == {} and c.finish_forms()["DENSE"] == 0
    finally:
        c.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(CASES))
def test_stage_launch_vs_oracle(built, gpu, name):
    _check_conditions(name)
    for dial in CASES[name]["dials"]:
        _run_dialect(name, dial, dense=True)
        _run_dialect(name, dial, dense=False)


@pytest.mark.gpu
def test_zz_the_module_ran_every_reachable_instantiation_and_chunk_class(built, gpu):
    """Runs last in this module: the keys the cases above COUNTED cover every (dialect, trace, glb, acc) -- all 32 k_stage
    instantiations of a build are reachable (test_launch_choice_sweep) -- and all five chunk classes in both dialects."""
    if len(SEEN) == 0:
        pytest.fail("run with the cases of this module: their counts are what this test reads")
    assert {(k.dialect, k.trace, k.glb, k.acc) for k in SEEN} == {(d, t, g, a) for d in RB for t in (False, True) for g in (False, True) for a in ACCS}
    assert {(k.dialect, k.chunk) for k in SEEN} == {(d, c) for d in RB for c in CHUNKS}
