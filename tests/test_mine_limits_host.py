"""The crafted jobs of tests/test_mine_limits.py, proved on the restatements alone (tests/mining_ref.py, oracle/cpp_reading2.py,
Oracle.resize_cv, api.mine_windows): each job is what the GPU file says it is -- segment tables, window totals, patch sums,
reject mix.  Fixed seeds, nothing is redrawn.  The job definitions live here; the GPU file imports them."""
import numpy as np
import pytest

import mining_ref

DIMS = (3, 20, 5, 4)                     # T, K, L, D of every model of the two files
K = DIMS[1]
SUM_LANES = 2048 * 256                   # k_mine_sum's largest grid in lanes: 524,288

# ---- models ------------------------------------------------------------------------------------------------------------
REJECT_TH = -0.8                         # the reject-mix model: every cart's threshold; leaf scores are N(0, 0.5)


def model(tmp_path, cart_th=REJECT_TH, hdr=None, sim=False, seed=4, multi=True):
    from jda_amd import synth
    m = synth.make_model(*DIMS, seed=seed, cart_th=cart_th, norm_every=5, multi_scale=multi, w_sigma=2e-2 if sim else 2e-3)
    p = str(tmp_path / ("lim_%g_%s_%d_%d_%d.model" % (cart_th, "full" if hdr is None else "%d_%d" % hdr, sim, seed, multi)))
    if hdr is None:
        m.save(p, 8)
    else:
        m.save(p, 8, header_stage=hdr[0], header_cart=hdr[1])
    return p


def images(sizes, seed):
    from jda_amd import synth
    return [synth.make_frames(1, w, h, seed=seed, first=i)[0] for i, (w, h) in enumerate(sizes)]


# ---- jobs: (image sizes (W, H), steps, factors, transforms) --------------------------------------------------------------
GEOMS = [(128, 96, 64), (128, 128, 128), (31, 17, 9), (1, 1, 1), (24, 36, 48), (48, 128, 1), (48, 36, 24)]


def geom_job(os_):
    """Two small backgrounds per geometry; image 1 is transposed (transform 3), factor 2 ends an image after a level or three."""
    return dict(sizes=[(os_ + 8, os_ + 6), (os_ + 5, os_ + 9)], steps=[3, 3], factors=[2.0, 2.0], tfs=[0, 3], seed=31)


# one job for the lane / chunk tails, the hand-off split and the reject mix: 48 / 36 / 24
TAIL_JOB = dict(sizes=[(80, 72), (58, 62)], steps=[2, 3], factors=[1.3, 1.25], tfs=[0, 6], seed=41)
# segments: A one segment of 121 windows | B exactly origin_size + 1 wide, step 3: nx = 1 | C skipped (W <= origin_size) |
# D one window | E two levels
SEG_JOB = dict(sizes=[(80, 80), (49, 70), (48, 90), (49, 49), (70, 66)], steps=[3, 3, 2, 5, 5], factors=[1.7, 1.2, 1.2, 1.2, 1.2],
               tfs=[0, 0, 0, 0, 0], seed=51)
SEG_TABLE = [(0, 0, 48, 11, 11), (121, 1, 48, 1, 8), (129, 3, 48, 1, 1), (130, 4, 48, 5, 4), (150, 4, 57, 3, 2)]   # first, image, win, nx, ny
SEG_TOTAL = 156
# more than one walk batch at (128, 96, 64): one level of 60 x 60 windows
BATCH_JOB = dict(sizes=[(246, 246)], steps=[2], factors=[2.0], tfs=[0], seed=61)
BATCH_TOTAL = 3600
# k_mine_sum past its grid: one 48-pixel-and-up enumeration a little above SUM_LANES + 256 windows
BIG_STEP, BIG_FACTOR, BIG_H = 2, 1.5, 900


def big_width(count):
    """The narrowest image BIG_H high whose enumeration has more than SUM_LANES + 256 windows; count(W, H) -> windows."""
    w = 600
    while count(w, BIG_H) <= SUM_LANES + 256:
        w += 1
    return w


def seg_table(job, os_):
    """[(first ordinal, image, win, nx, ny)] and the total, from mining_ref.levels on the transformed sizes."""
    out, total = [], 0
    for i, (w, h) in enumerate(job["sizes"]):
        W, H = (h, w) if job["tfs"][i] in (1, 3, 5, 7) else (w, h)
        for win, nx, ny in mining_ref.levels(W, H, os_, job["steps"][i], job["factors"][i]):
            out.append((total, i, win, nx, ny))
            total += nx * ny
    return out, total


def restate(m2, resize, job, os_, hs, qs, shift=0.0, seed=0, sim=False, only=None):
    """Every window of the job through the mining chain and Validate, in enumeration order: a list of dicts (ordinal, row =
    (image, x, y, win), face, score, shape, n, patches); only: the ordinals to restate (others are None)."""
    out, o = [], 0
    for i, im in enumerate(images(job["sizes"], job["seed"])):
        ti = mining_ref.transform(im, job["tfs"][i])
        H, W = ti.shape
        for (x, y, win) in mining_ref.windows(W, H, os_, job["steps"][i], job["factors"][i]):
            if only is not None and o not in only:
                out.append(None)
            else:
                p = mining_ref.chain(resize, ti[y:y + win, x:x + win], 0, os_, hs, qs)
                dx, dy = mining_ref.shift_of(seed, o, shift)
                face, sc, sh, n = mining_ref.validate(m2, p, dx, dy, sim)
                out.append(dict(ordinal=o, row=(i, x, y, win), face=bool(face), score=sc, shape=sh, n=n, patches=p))
            o += 1
    return out


def expect(per, start, size):
    """ParallelMining over the restated windows from ordinal `start`: what mining_ref.mine returns, from the table."""
    hits, nega, carts, nxt = [], 0, 0, len(per)
    for r in per[start:]:
        if r["face"]:
            hits.append(r)
            if len(hits) == size:
                nxt = r["ordinal"] + 1
                break
        else:
            nega += 1
            carts += r["n"]
    return dict(hits=hits, nega_n=nega, carts_n=carts, next_start=max(nxt, min(start, len(per))))


# ---- the proofs ----------------------------------------------------------------------------------------------------------

def test_segment_job_is_what_it_claims():
    tab, total = seg_table(SEG_JOB, 48)
    assert tab == SEG_TABLE and total == SEG_TOTAL
    assert mining_ref.levels(48, 90, 48, 2, 1.2) == []                       # C: skipped, between images that are taken
    assert [t[1] for t in tab] == [0, 1, 3, 4, 4]
    assert (49 - 48) // 3 + 1 == 1 and tab[1][3:] == (1, 8)                  # B: one column
    assert tab[2][3:] == (1, 1)                                              # D: one window
    one, total1 = seg_table(dict(sizes=[(80, 80)], steps=[3], factors=[1.7], tfs=[0]), 48)
    assert len(one) == 1 and total1 == 121                                   # A alone: an enumeration with one segment
    # chunks of 64 windows from these starts begin on a segment's first ordinal / end on its last
    firsts = [t[0] for t in tab]
    lasts = [t[0] + t[3] * t[4] - 1 for t in tab]
    assert lasts == [120, 128, 129, 149, 155]
    for f in firsts[1:]:
        assert f - 64 >= 0
    assert SEG_TOTAL - 64 > 0


def test_segment_table_equals_the_library_enumeration(built):
    from jda_amd import api
    tab, total = seg_table(SEG_JOB, 48)
    n = 0
    for i, (w, h) in enumerate(SEG_JOB["sizes"]):
        cnt, lv = api.mine_windows(w, h, 48, SEG_JOB["steps"][i], SEG_JOB["factors"][i])
        assert lv == sum(1 for t in tab if t[1] == i)
        assert cnt == sum(t[3] * t[4] for t in tab if t[1] == i)
        n += cnt
    assert n == total


def test_window_totals(built):
    from jda_amd import api
    count = lambda w, h: api.mine_windows(w, h, 48, BIG_STEP, BIG_FACTOR)[0]
    W = big_width(count)
    n = count(W, BIG_H)
    assert SUM_LANES + 256 < n < SUM_LANES + 256 + 4096, (W, n)            # a little above: one more column of windows at most
    assert count(W - 1, BIG_H) <= SUM_LANES + 256
    assert n == sum(nx * ny for _, nx, ny in mining_ref.levels(W, BIG_H, 48, BIG_STEP, BIG_FACTOR))
    assert seg_table(BATCH_JOB, 128) == ([(0, 0, 128, 60, 60)], BATCH_TOTAL)
    tab, total = seg_table(TAIL_JOB, 48)
    assert 257 < total < 400 and len(tab) >= 3, (tab, total)               # every chunk length of the tails test cuts it
    for os_, _, _ in GEOMS:
        tab, total = seg_table(geom_job(os_), os_)
        assert 10 <= total <= 60 and {t[1] for t in tab} == {0, 1}, (os_, tab)


def test_patch_sums_and_their_16_byte_stride():
    tight = {g: g[0] ** 2 + g[1] ** 2 + g[2] ** 2 for g in GEOMS}
    assert tight == {(128, 96, 64): 29696, (128, 128, 128): 49152, (31, 17, 9): 1331, (1, 1, 1): 3, (24, 36, 48): 4176,
                     (48, 128, 1): 18689, (48, 36, 24): 4176}
    assert {g: t % 16 for g, t in tight.items()} == {(128, 96, 64): 0, (128, 128, 128): 0, (31, 17, 9): 3, (1, 1, 1): 3,
                                                     (24, 36, 48): 0, (48, 128, 1): 1, (48, 36, 24): 0}
    assert sum(1 for t in tight.values() if t % 16) == 3                    # three geometries tell stride from tight size
    assert any(g[1] > g[0] for g in GEOMS) and any(g[2] > g[1] for g in GEOMS)     # the o -> h / q chain up-scales
    assert max(max(g) for g in GEOMS) == 128 and min(min(g) for g in GEOMS) == 1


@pytest.mark.parametrize("hdr", [None, (0, 11)])
def test_reject_mix_on_the_tail_job(built, tmp_path, hdr):
    """The reject-mix model on the tail job: at least four different reject lengths and a survivor, so carts_n is no multiple
    of nega_n by construction; on the full model some rejects come after stage 0 (the walk's share can never be empty)."""
    from oracle import cpp_reading2 as r2
    from oracle.pyoracle import Oracle
    p = model(tmp_path, hdr=hdr)
    o, m2 = Oracle(p), r2.Model2(p)
    per = restate(m2, o.resize_cv, TAIL_JOB, 48, 36, 24)
    o.close()
    ns = [r["n"] for r in per if not r["face"]]
    assert len(set(ns)) >= 4, sorted(set(ns))
    assert any(r["face"] for r in per) and len(ns) > 0
    assert sum(ns) % len(ns) != 0
    ran = K * 3 if hdr is None else hdr[0] * K + hdr[1] + 1
    assert all(r["n"] == ran for r in per if r["face"]) and max(ns) <= ran
    # both sides of every hand-off the GPU file runs: rejects at or below it, and rejects (or faces) above it
    stage0 = K if hdr is None else hdr[1] + 1
    for handoff in (1, 2, K - 1, K, K + 5):
        c0 = min(stage0, handoff)
        assert any(n <= c0 for n in ns), handoff
    if hdr is None:
        assert any(n == K - 1 for n in ns) and any(K < n <= K + 5 for n in ns) and any(n > K + 5 for n in ns)
    # expect() is mining_ref.mine, from the table
    want = mining_ref.mine(m2, Oracle(p).resize_cv, images(TAIL_JOB["sizes"], TAIL_JOB["seed"]), TAIL_JOB["steps"], TAIL_JOB["factors"],
                           TAIL_JOB["tfs"], 3, 5)
    got = expect(per, 5, 3)
    assert [h["row"] for h in got["hits"]] == want["hits"]
    assert (got["nega_n"], got["carts_n"], got["next_start"]) == (want["nega_n"], want["carts_n"], want["next_start"])
