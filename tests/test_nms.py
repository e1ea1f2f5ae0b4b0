"""Host NMS + relocation of libjda (no GPU): exact order semantics of reference
c/jda.c:237-316 and src/jda/cascador.cpp:387-429."""
import numpy as np
import pytest

import golden_util
from conftest import same


def _relocate(shapes, bboxes):
    out = shapes.copy()
    sz = bboxes[:, 2].astype(np.float32)[:, None]
    out[:, 0::2] = out[:, 0::2] * sz + bboxes[:, 0].astype(np.float32)[:, None]   # two roundings, c/jda.c:471-472
    out[:, 1::2] = out[:, 1::2] * sz + bboxes[:, 1].astype(np.float32)[:, None]
    return out


@pytest.mark.parametrize("name", golden_util.NAMES)
def test_nms_turns_reference_raw_into_reference_post(built, tmp_path, name):
    """jdaNmsC applied to the reference's pre-NMS survivors gives the reference's post-NMS list."""
    from jda_amd import api
    meta, g, _ = golden_util.load(name, tmp_path)
    keep = api.nms_c(g["raw_bboxes"], g["raw_scores"], 0.3)
    assert same(g["raw_bboxes"][keep], g["post_bboxes"])
    assert same(g["raw_scores"][keep], g["post_scores"])
    assert same(_relocate(g["raw_shapes"][keep], g["raw_bboxes"][keep]), g["post_shapes"])


def _literal_keep(bb, sc, overlap=0.3):
    """Literal restatement of the reference loops in Python: exchange sort under a strict `<` (c/jda.c:256-264), greedy
    suppression in that order (c/jda.c:267-284).  Scores as Python floats: NaN compares false, -0.0 == +0.0, like C."""
    n = len(sc)
    s = [float(v) for v in sc]
    box = [tuple(int(v) for v in b) for b in bb]
    idx = list(range(n))
    for i in range(n - 1):
        for j in range(i + 1, n):
            if s[idx[i]] < s[idx[j]]:
                idx[i], idx[j] = idx[j], idx[i]
    keep = np.ones(n, bool)
    for i in range(n - 1):
        a = idx[i]
        if not keep[a]:
            continue
        for j in range(i + 1, n):
            b = idx[j]
            if not keep[b]:
                continue
            x1, y1 = max(box[a][0], box[b][0]), max(box[a][1], box[b][1])
            x2 = min(box[a][0] + box[a][2], box[b][0] + box[b][2]); y2 = min(box[a][1] + box[a][2], box[b][1] + box[b][2])
            w, h = max(0, x2 - x1), max(0, y2 - y1)
            ov = np.float32(w * h) / np.float32(box[a][2] ** 2 + box[b][2] ** 2 - w * h)
            if ov > np.float32(overlap):
                keep[b] = False
    return keep


def test_ties_replay_the_exchange_sort(built):
    """Equal scores: the survivor set depends on the exchange sort's permutation (c/jda.c:256-264)."""
    from jda_amd import api
    rng = np.random.default_rng(0)
    for trial in range(30):
        n = int(rng.integers(2, 60))
        bb = np.c_[rng.integers(0, 40, n), rng.integers(0, 40, n), rng.integers(20, 40, n)].astype(np.int32)
        sc = rng.integers(0, 4, n).astype(np.float32)          # many ties
        assert np.array_equal(api.nms_c(bb, sc, 0.3), _literal_keep(bb, sc)), trial


@pytest.mark.parametrize("n", [256, 257, 1024])
@pytest.mark.parametrize("alphabet", ["ties", "nan_and_zeros"])
def test_literal_order_at_the_device_limits(built, n, alphabet):
    """The host form at the sizes where k_post hands over to it or stops replaying the sort itself (256 and 257 tied
    detections, 1,024 detections; tests/test_device_post.py compares the kernel with this form): scores from a small
    alphabet -- tie groups of different sizes, and with NaN, +0.0 and -0.0 among them (NaN is never `<` anything, the
    two zeros are equal: the permutation of the strict-`<` exchange sort decides who suppresses whom) -- on a window
    grid like a scan's (step 3, size 30: neighbours overlap by more than 0.3)."""
    from jda_amd import api
    rng = np.random.default_rng(n)
    nx = 16 if n <= 256 else (257 if n == 257 else 32)
    ix = np.arange(n)
    bb = np.c_[(ix % nx) * 3, (ix // nx) * 3, np.full(n, 30)].astype(np.int32)
    if alphabet == "ties":
        values = np.array([-1.0, -0.5, 0.25, 0.25, 0.5, 1.0, 2.0], np.float32)
        pr = [0.3, 0.05, 0.2, 0.1, 0.2, 0.1, 0.05]
    else:
        values = np.array([np.nan, 0.0, -0.0, 0.5, 0.5, -1.0, 1.0], np.float32)
        pr = [0.2, 0.15, 0.15, 0.15, 0.1, 0.15, 0.1]
    sc = values[rng.choice(len(values), n, p=pr)]
    if alphabet == "nan_and_zeros":
        assert np.isnan(sc).any() and (sc.view(np.uint32) == 0x80000000).any() and (sc.view(np.uint32) == 0).any()
    want = _literal_keep(bb, sc)
    got = api.nms_c(bb, sc, 0.3)
    assert np.array_equal(got, want)
    assert 0 < want.sum() < n


def test_nms_edge_cases(built):
    from jda_amd import api
    assert api.nms_c(np.zeros((0, 3), np.int32), np.zeros(0, np.float32)).shape == (0,)
    assert api.nms_c([[0, 0, 30]], [1.0]).tolist() == [True]
    assert api.nms_cpp(np.zeros((0, 4), np.int32), np.zeros(0)).shape == (0,)


def test_nms_cpp_matches_oracle(built, model_file):
    """Dialect CPP NMS of libjda vs the oracle's restatement of the multimap loop."""
    from jda_amd import api
    rng = np.random.default_rng(1)
    for trial in range(20):
        n = int(rng.integers(1, 80))
        s = rng.integers(10, 40, n)
        rc = np.c_[rng.integers(0, 50, n), rng.integers(0, 50, n), s, s].astype(np.int32)
        sc = np.round(rng.normal(0, 1, n), 1)       # ties likely
        # Python restatement of cascador.cpp:387-429
        order = sorted(range(n), key=lambda i: sc[i])    # stable ascending == multimap order
        alive, picked = list(order), []
        while alive:
            last = alive[-1]
            picked.append(last)
            nxt = []
            for i in alive:
                x1 = max(rc[i, 0], rc[last, 0]); y1 = max(rc[i, 1], rc[last, 1])
                x2 = min(rc[i, 0] + rc[i, 2], rc[last, 0] + rc[last, 2]); y2 = min(rc[i, 1] + rc[i, 3], rc[last, 1] + rc[last, 3])
                w, h = max(0., float(x2 - x1)), max(0., float(y2 - y1))
                ov = w * h / (float(rc[i, 2] * rc[i, 3]) + float(rc[last, 2] * rc[last, 3]) - w * h)
                if not ov > 0.3:
                    nxt.append(i)
            alive = nxt
        assert api.nms_cpp(rc, sc, 0.3).tolist() == picked, trial
