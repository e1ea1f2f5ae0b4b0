"""Moving a sample set into a new order on the device (jdaGatherSamplesCpp, k_gather.hip) against numpy fancy indexing on
the host copy, byte for byte, and one loop of three carts -- weights, jdaTrainCartCpp, scores, order and cut, the gather,
the rows along -- against the sequential restatement tests/boost_ref.py, bit for bit.  No tolerance anywhere.
tests/test_boost_host.py holds the host entries' own cases.  Dialect CPP is parity-unpinned: bit-exact against this
repo's restatement of the reference's source, not against the reference."""
import numpy as np
import pytest

from conftest import same
import boost_ref
import stage_ref
import train_ref

pytestmark = pytest.mark.gpu

SHIPPED = (48, 36, 24)
ODD = (31, 17, 9)                          # P = 1331: every other record starts at an odd address


@pytest.fixture(scope="module")
def gpu():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    return torch.device("cuda", 0)


@pytest.fixture()
def casc(built, gpu, model_file):
    from jda_amd import api
    p, _ = model_file((1, 2, 5, 3))
    c = api.Cascador(p, "double", device=0)
    yield c
    c.close()


def _pb(sizes):
    return sum(v * v for v in sizes)


def _records(seed, n, sizes):
    return np.random.default_rng(seed).integers(0, 256, (n, _pb(sizes)), dtype=np.uint8)


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).reshape(-1)).cuda()


CANARY = 64


def _canary_dst(n_records, pb, offset=0, device=True):
    """A destination of n_records records at byte `offset` of a larger buffer filled with a pattern -> (buffer, view, host
    copy of the pattern)."""
    total = offset + n_records * pb + 2 * CANARY + 16
    pat = ((np.arange(total) * 37 + 11) % 251).astype(np.uint8)
    buf = _dev(pat) if device else pat.copy()
    lo = CANARY + offset
    return buf, buf[lo:lo + n_records * pb], pat, lo


def _check_dst(buf, pat, lo, want, device=True):
    """The written range equals `want` ([keep, pb]); every other byte of the buffer is the pattern's."""
    got = buf.cpu().numpy() if device else buf
    n = want.size
    assert np.array_equal(got[lo:lo + n], want.reshape(-1))
    assert np.array_equal(got[:lo], pat[:lo]) and np.array_equal(got[lo + n:], pat[lo + n:])


def _indices(seed, n):
    rng = np.random.default_rng(seed)
    rep = rng.integers(0, n, n + 3)
    return [("identity", np.arange(n), n), ("reversal", np.arange(n)[::-1], n), ("permutation", rng.permutation(n), n),
            ("repeats", rep, rep.size), ("keep < n", rng.permutation(n), max(n - 2, 0)), ("keep = 0", rng.permutation(n), 0)]


# ---- 1. sizes, counts, index lists -------------------------------------------------------------------------------------

@pytest.mark.parametrize("sizes", [(1, 1, 1), ODD, SHIPPED, (47, 35, 23)])
def test_sizes_counts_and_index_lists(casc, sizes):
    pb = _pb(sizes)
    for n in (1, 63, 64, 65, 67):
        src = _records(n + pb, n, sizes)
        d_src = _dev(src)
        for name, idx, keep in _indices(n, n):
            buf, view, pat, lo = _canary_dst(len(idx), pb)
            _, st = casc.gather_samples_cpp(d_src, idx, view, keep, *sizes, stats=True)
            _check_dst(buf, pat, lo, src[idx[:keep]])
            assert st["launches"] == (1 if keep else 0) and st["bytes"] == keep * pb and st["chunks"] == 0, (name, n)


def test_largest_record(casc):
    sizes, n = (128, 128, 128), 3
    src = _records(9, n, sizes)
    buf, view, pat, lo = _canary_dst(4, _pb(sizes), offset=5)
    casc.gather_samples_cpp(_dev(src), [2, 0, 1, 2], view, None, *sizes)
    _check_dst(buf, pat, lo, src[[2, 0, 1, 2]])


# ---- 2. misalignment ---------------------------------------------------------------------------------------------------

def test_every_pair_of_misalignments(casc):
    """Source and destination as views at byte offsets 0 .. 15 of larger device tensors, all 16 x 16 pairs.  The canary
    before and after the written range and the records beyond `keep` stay as they were."""
    n, keep, pb = 5, 4, _pb(ODD)
    src = _records(3, n, ODD)
    idx = np.array([3, 0, 4, 1, 2])
    for so in range(16):
        sbuf = _dev(np.concatenate([np.zeros(so, np.uint8), src.reshape(-1), np.zeros(16, np.uint8)]))
        sview = sbuf[so:so + n * pb]
        assert sview.data_ptr() % 16 == (sbuf.data_ptr() + so) % 16
        for do in range(16):
            buf, view, pat, lo = _canary_dst(n, pb, offset=do)
            assert view.data_ptr() % 16 == (buf.data_ptr() + CANARY + do) % 16
            casc.gather_samples_cpp(sview, idx, view, keep, *ODD)
            _check_dst(buf, pat, lo, src[idx[:keep]])                         # (record 4 of dst is still the canary)


# ---- 3. segments, host and device --------------------------------------------------------------------------------------

def _edge_index(counts, seed):
    """Indices on both sides of every segment edge, the first and the last record, and some random ones."""
    total, edges, at = sum(counts), set(), 0
    for c in counts:
        edges |= {at - 1, at, at + c - 1, at + c}
        at += c
    idx = sorted(e for e in edges if 0 <= e < total)
    rng = np.random.default_rng(seed)
    return np.concatenate([idx, rng.integers(0, total, 7)]).astype(np.int64)[rng.permutation(len(idx) + 7)]


@pytest.mark.parametrize("layout", [("dh", (5, 4)), ("hd", (4, 5)), ("hdd", (3, 0, 6)), ("hhd", (4, 5, 3)), ("dhd", (2, 0, 3)), ("hh", (3, 2))])
@pytest.mark.parametrize("host_dst", [False, True])
def test_segments(casc, layout, host_dst):
    kinds, counts = layout
    pb = _pb(ODD)
    parts = [_records(40 + i, c, ODD) for i, c in enumerate(counts)]
    segs = [_dev(p) if k == "d" else p.reshape(-1) for k, p in zip(kinds, parts)]
    whole = np.concatenate(parts)
    idx = _edge_index(counts, len(kinds))
    buf, view, pat, lo = _canary_dst(len(idx), pb, offset=3, device=not host_dst)
    casc.gather_samples_cpp(segs, idx, view, None, *ODD)
    _check_dst(buf, pat, lo, whole[idx], device=not host_dst)
    # "append": an identity index over two or three segments
    ident = np.arange(len(whole))
    buf, view, pat, lo = _canary_dst(len(whole), pb, device=not host_dst)
    casc.gather_samples_cpp(segs, ident, view, None, *ODD)
    _check_dst(buf, pat, lo, whole, device=not host_dst)


def test_host_segments_in_chunks(casc):
    """workspace_mb = 1: a host segment of 3.3 MB goes through the workspace in at least 3 chunks, a host dst likewise."""
    n, pb = 800, _pb(SHIPPED)
    host, dev_part = _records(1, n, SHIPPED), _records(2, 10, SHIPPED)
    whole = np.concatenate([host, dev_part])
    idx = np.random.default_rng(3).permutation(n + 10)
    buf, view, pat, lo = _canary_dst(n + 10, pb)
    _, st1 = casc.gather_samples_cpp([host.reshape(-1), _dev(dev_part)], idx, view, None, *SHIPPED, stats=True)
    _check_dst(buf, pat, lo, whole[idx])
    assert st1["chunks"] == 1
    casc.set_option("workspace_mb", 1)
    buf, view, pat, lo = _canary_dst(n + 10, pb)
    _, st = casc.gather_samples_cpp([host.reshape(-1), _dev(dev_part)], idx, view, None, *SHIPPED, stats=True)
    _check_dst(buf, pat, lo, whole[idx])
    assert st["chunks"] >= 3 and st["launches"] == st["chunks"] + 1
    out = np.zeros((n, pb), np.uint8)                                         # device records to a host dst, in chunks too
    _, st = casc.gather_samples_cpp(_dev(host), idx[idx < n], out.reshape(-1), None, *SHIPPED, stats=True)
    assert np.array_equal(out, host[idx[idx < n]]) and st["chunks"] >= 3


# ---- 4. refused before anything is launched ----------------------------------------------------------------------------

def test_refusals(casc):
    from jda_amd import api
    n, pb = 6, _pb(ODD)
    src = _records(8, n, ODD)
    d_src = _dev(src)
    buf, view, pat, lo = _canary_dst(n, pb)

    def refused(segs, idx, dst, sizes=ODD, keep=None):
        with pytest.raises(api.JdaError) as e:
            casc.gather_samples_cpp(segs, idx, dst, keep, *sizes)
        assert api.last_error() and str(e.value) == api.last_error()
        return api.last_error()
    assert "index[1]" in refused(d_src, [0, n], view)                         # an index equal to the total record count
    assert "index[2]" in refused(d_src, [0, 1, -1], view)
    assert "index[0]" in refused([d_src, src[:2].reshape(-1)], [n + 2], view)
    assert "overlaps" in refused(d_src, [0, 1], d_src[pb:3 * pb])             # dst inside the device segment
    assert "overlaps" in refused(d_src[:3 * pb], [0, 1, 2], d_src[3 * pb - 1:6 * pb - 1])       # ... by one byte
    assert "n_segs" in refused([d_src] * 9, [0], view)
    one = _dev(np.zeros(3 * 129 * 129, np.uint8))
    for sizes in ((0, 17, 9), (31, 0, 9), (31, 17, 0), (129, 17, 9), (31, 129, 9), (31, 17, 129)):
        rc = api.lib.jdaGatherSamplesCpp(casc.h, (api.jdaGatherSegCpp * 1)(api.jdaGatherSegCpp(one.data_ptr(), 1, 1)), 1, *sizes,
                                         None, 0, None, 1, None)
        assert rc == -1 and "[1, 128]" in api.last_error(), sizes
    _check_dst(buf, pat, lo, np.zeros((0, pb), np.uint8))                     # nothing was written
    # neighbours that do not overlap are fine: dst right behind the segment
    casc.gather_samples_cpp(d_src[:3 * pb], [2, 1, 0], d_src[3 * pb:], None, *ODD)
    assert np.array_equal(d_src.cpu().numpy().reshape(n, pb), np.concatenate([src[:3], src[[2, 1, 0]]]))


def test_similarity_transform_does_not_matter(casc):
    src = _records(12, 9, ODD)
    casc.set_similarity_transform(True)
    out = np.zeros_like(src)
    casc.gather_samples_cpp(_dev(src), np.arange(9)[::-1], out.reshape(-1), None, *ODD)
    assert np.array_equal(out, src[::-1])


# ---- 5. one loop of three carts ----------------------------------------------------------------------------------------

def _feature_rows(got):
    return [(int(f["scale"]), int(f["landmark_id1"]), int(f["landmark_id2"]), float(f["offset1_x"]), float(f["offset1_y"]),
             float(f["offset2_x"]), float(f["offset2_y"])) for f in got]


def test_three_carts_end_to_end(built, gpu, model_file):
    import torch
    from jda_amd import api
    L, D, F, sizes, drop_n, norm_step = 5, 3, 16, ODD, 2, 2
    pb = _pb(sizes)
    pd = train_ref.make_samples(71, 67, L, sizes)
    nd = train_ref.make_samples(171, 131, L, sizes)
    xd = train_ref.make_samples(271, 40, L, sizes)                            # the negatives that arrive after cart 2
    rng = np.random.default_rng(5)
    quant = lambda v: np.round(v * 2) / 2                                     # quantised scores: ties exist
    pos_scores, neg_scores, x_scores = quant(rng.normal(1, 1, 67)), quant(rng.normal(-1, 1, 131)), quant(rng.normal(-0.5, 1, 40))
    modes = [1, 0, 1]
    pools = [[train_ref.gen_feature_pool(F, L, train_ref.RADIUS, True, 71 + k, node) for node in range(1, 4)] for k in range(3)]

    # ---- the restatement's run, and what it must have met for this test to mean anything
    rp = boost_ref.RefSet(pd["patches"], pd["shapes"], pos_scores, pd["residual"])
    rn = boost_ref.RefSet(nd["patches"], nd["shapes"], neg_scores)
    ref_carts = [([train_ref.pool_of(p) for p, _ in pools[k]], modes, [u for _, u in pools[k]]) for k in range(3)]
    want, final_w = boost_ref.boost_loop(D, sizes, rp, rn, ref_carts, drop_n, norm_step, {2: (xd["patches"], xd["shapes"], x_scores)})
    assert all(w["neg_drop"] >= 1 and w["neg_drop"] == w["will_removed"] for w in want)
    assert any(a == b for w in want for s in (w["pos"]["scores"], w["neg"]["scores"]) for a, b in zip(s, s[1:]))
    sorts = rp.orders + rn.orders
    assert len(sorts) == 9                                                    # the unsorted start and 3 carts per set, and the negatives once more after the append
    assert any(order != np.argsort(-np.array(before), kind="stable").tolist() for before, order in sorts)
    assert want[1]["std"] != 1. and want[0]["std"] == 1. and want[2]["start"]["neg_n"] == len(want[1]["neg"]["scores"]) + 40

    # ---- the product's run: patches resident on the device, two buffers per set
    p, _ = model_file((1, 2, L, D))
    c = api.Cascador(p, "double", device=0)
    cap = {"pos": 67, "neg": 131 + 40}
    bufs = {k: [torch.zeros(cap[k] * pb + 1, dtype=torch.uint8, device="cuda")[1:] for _ in range(2)] for k in cap}      # (odd base addresses)
    st = {"pos": dict(shapes=pd["shapes"].copy(), residual=pd["residual"].copy(), scores=pos_scores.copy(), last=pos_scores.copy(), n=67, cur=0),
          "neg": dict(shapes=nd["shapes"].copy(), scores=neg_scores.copy(), last=neg_scores.copy(), n=131, cur=0)}
    bufs["pos"][0][:67 * pb] = _dev(pd["patches"])
    bufs["neg"][0][:131 * pb] = _dev(nd["patches"])

    def patches(k):
        return bufs[k][st[k]["cur"]][:st[k]["n"] * pb]

    def carry(k, segs, rows, order, keep, scores_sorted):
        """The gather into the other buffer and the host rows along."""
        s = st[k]
        c.gather_samples_cpp(segs, order, bufs[k][1 - s["cur"]], keep, *sizes)
        for name, extra in rows.items():
            s[name] = api.gather_rows_cpp([s[name]] + extra, order, keep)
        s["scores"], s["n"], s["cur"] = scores_sorted[:keep].copy(), keep, 1 - s["cur"]

    def check_state(k, w):
        s = st[k]
        assert np.array_equal(patches(k).cpu().numpy().reshape(-1, pb), np.stack(w["patches"]))
        assert same(s["shapes"], np.array(w["shapes"])) and same(s["scores"], np.array(w["scores"])) and same(s["last"], np.array(w["last"]))
        if k == "pos":
            assert same(s["residual"], np.array(w["residual"]))

    for k in ("pos", "neg"):                                                  # the sets start unsorted: btcart.cpp:154 sorts them
        order, srt = api.sample_order_cpp(st[k]["scores"])
        carry(k, patches(k), {name: [] for name in st[k] if name in ("shapes", "residual", "last")}, order, order.size, srt)
    for k in range(3):
        w = want[k]
        if k == 2:                                                            # MoreNegSamples, then QSort over the whole set
            s = st["neg"]
            order, srt = api.sample_order_cpp(np.concatenate([s["scores"], x_scores]))
            carry("neg", [patches("neg"), xd["patches"].reshape(-1)], dict(shapes=[xd["shapes"]], last=[x_scores]), order, order.size, srt)
            assert np.array_equal(patches("neg").cpu().numpy().reshape(-1, pb), np.stack(w["start"]["neg_patches"]))
        pw, nw = api.update_weights_cpp(st["pos"]["scores"], st["neg"]["scores"])
        assert same(pw, np.array(w["start"]["pos_weights"])) and same(nw, np.array(w["start"]["neg_weights"]))
        flat = stage_ref.pool_array([r for pl, _ in pools[k] for r in pl])
        got = c.train_cart_cpp(dict(patches=patches("pos"), shapes=st["pos"]["shapes"], weights=pw, residual=st["pos"]["residual"], has_gt=None),
                               dict(patches=patches("neg"), shapes=st["neg"]["shapes"], weights=nw, residual=None, has_gt=None),
                               flat, modes, np.array([u for _, u in pools[k]]), *sizes)
        assert _feature_rows(got["features"]) == [pools[k][i][0][fi] for i, fi in enumerate(w["cart"]["features"])]
        assert got["thresholds"].tolist() == w["cart"]["thresholds"] and same(got["scores"], np.array(w["cart"]["scores"]))
        sc = api.boost_scores_cpp(got["scores"], got["pos_leaf"], got["neg_leaf"], st["pos"]["scores"], st["neg"]["scores"],
                                  normalize=(k + 1) % norm_step == 0)
        assert same(np.array([sc["mean"], sc["std"]]), np.array([w["mean"], w["std"]]))
        st["pos"]["last"], st["neg"]["last"] = sc["pos_last"], sc["neg_last"]
        op, sp = api.sample_order_cpp(sc["pos_scores"])
        on, sn = api.sample_order_cpp(sc["neg_scores"])
        th = api.score_threshold_cpp(sp, drop_n)
        keep_p, _ = api.score_cut_cpp(sp, th)
        keep_n, will_removed = api.score_cut_cpp(sn, th)
        assert same(np.float64(th), np.float64(w["th"])) and will_removed == w["will_removed"]
        carry("pos", patches("pos"), dict(shapes=[], residual=[], last=[]), op, keep_p, sp)
        carry("neg", patches("neg"), dict(shapes=[], last=[]), on, keep_n, sn)
        check_state("pos", w["pos"]); check_state("neg", w["neg"])
    pw, nw = api.update_weights_cpp(st["pos"]["scores"], st["neg"]["scores"])
    assert same(pw, np.array(final_w[0])) and same(nw, np.array(final_w[1]))
    c.close()
