"""Closing a training stage on the device (jdaGenLbfCpp, jdaStageUpdateShapesCpp) against the sequential restatement
tests/stage_ref.py, bit for bit: every comparison is exact (`same`), there is no tolerance anywhere.
tests/test_stage_close_host.py holds the control that the cart order these tests pin is visible in the bits.  Dialect CPP
is parity-unpinned: bit-exact against this repo's restatement of the reference's source, not against the reference."""
import numpy as np
import pytest

from conftest import same
import stage_ref
import train_ref

pytestmark = pytest.mark.gpu

SHIPPED = (48, 36, 24)


@pytest.fixture(scope="module")
def gpu():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    return torch.device("cuda", 0)


def _cascador(model_file, L, D):
    from jda_amd import api
    p, _ = model_file((1, 2, L, D))
    return api.Cascador(p, "double", device=0)


def _case(seed, n, K, D, L, sizes=SHIPPED, multi=True, outside=0.3):
    d = train_ref.make_samples(seed, n, L, sizes, outside=outside)
    rows, th = stage_ref.make_carts(seed, K, D, L, multi)
    w = stage_ref.make_w(seed, K, D, L)
    shapes, lbf = stage_ref.stage_update(D, stage_ref.carts_of(D, rows, th), train_ref.ref_set(d), w.tolist())
    return d, rows, th, w, np.array(shapes, np.float64).reshape(n, 2 * L), np.array(lbf, np.int32).reshape(n, K)


def _check(c, case, sizes=SHIPPED):
    """Every path of the two entries on one case: the fused pass, the indicators alone, given indicators."""
    d, rows, th, w, want_shapes, want_lbf = case
    pool = stage_ref.pool_array(rows)
    got_lbf = c.gen_lbf_cpp(d, pool, th, *sizes)
    assert same(got_lbf, want_lbf)
    shapes, out_lbf, st = c.stage_update_shapes_cpp(d, pool, th, w, None, *sizes, want_lbf=True, stats=True)
    assert same(shapes, want_shapes)
    assert same(out_lbf, got_lbf)                                             # out_lbf equals gen_lbf_cpp
    assert same(c.stage_update_shapes_cpp(d, None, None, w, got_lbf, *sizes), shapes)    # lbf_in given equals the walked result
    assert same(c.stage_update_shapes_cpp(d, pool, th, w, None, *sizes), shapes)         # (out_lbf NULL)
    return st


# ---- 1. the smallest case ----------------------------------------------------------------------------------------------

def test_smallest_case(built, gpu, model_file):
    c = _cascador(model_file, 1, 2)
    st = _check(c, _case(3, 1, 1, 2, 1))
    assert st["chunks"] == 1 and st["lds_path"] == 1
    c.close()


# ---- 2. lane boundaries ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("K,n,L,D", [(64, 3, 5, 4), (65, 3, 5, 4), (130, 3, 5, 4), (7, 67, 5, 4), (20, 3, 32, 4), (20, 3, 68, 4),
                                     (20, 5, 5, 2), (20, 5, 5, 6)])
def test_lane_boundaries(built, gpu, model_file, K, n, L, D):
    c = _cascador(model_file, L, D)
    case = _case(100 + K + n + L + D, n, K, D, L)
    _check(c, case)
    assert len(set((case[5] % (1 << (D - 1))).reshape(-1).tolist())) > 1      # a real walk: the samples spread over the leaves
    c.set_option("lbf_lds_kb", 0)                                             # the same from global memory
    assert _check(c, case)["lds_path"] == 0
    c.close()


# ---- 3. patches --------------------------------------------------------------------------------------------------------

def _border_reads(d, rows, sizes, L):
    """Root-node reads that the clamp moved onto a patch border (data.cpp:40-54), counted with the restatement's arithmetic."""
    from oracle import cpp_reading2 as r2
    hits = 0
    for shape in d["shapes"]:
        for (scale, lm1, lm2, o1x, o1y, o2x, o2y) in rows:
            side = sizes[scale]
            for lm, ox, oy in ((lm1, o1x, o1y), (lm2, o2x, o2y)):
                x, y = int(r2.c_round((shape[2 * lm] + ox) * side)), int(r2.c_round((shape[2 * lm + 1] + oy) * side))
                hits += x < 0 or y < 0 or x >= side or y >= side
    return hits


@pytest.mark.parametrize("sizes,n", [((48, 36, 24), 9), ((31, 17, 9), 9), ((128, 128, 128), 2)])
def test_patch_sizes_and_scales(built, gpu, model_file, sizes, n):
    K, D, L = 20, 4, 5
    c = _cascador(model_file, L, D)
    case = _case(7 + sizes[0], n, K, D, L, sizes)
    d, rows, th = case[0], case[1], case[2]
    assert {r[0] for r in rows} == {0, 1, 2}                                  # the nodes read all three patches
    # shapes pushed outside the patch: reads land on both kinds of border, and the values spread over the range
    assert _border_reads(d, rows, sizes, L) > 0
    vals = np.array(train_ref.calc_feature_values(train_ref.ref_set(d), train_ref.pool_of(rows), list(range(n))))
    assert (vals == 0).mean() < 0.5 and np.abs(vals).max() > 200
    st = _check(c, case, sizes)
    assert st["lds_path"] == 1
    if sizes[0] == 128:
        # the LDS limit: a sample's slice is 3 * 128^2 bytes + shape + indicators, three of them fit the CU's 160 KB
        assert st["waves_per_group"] == 3 and 3 * 3 * 128 * 128 < st["lds_bytes"] <= 160 * 1024
        c.set_option("lbf_lds_kb", 32)                                        # ... and none fits 32 KB: the global path
        st = _check(c, case, sizes)
        assert (st["lds_path"], st["lds_bytes"]) == (0, 0)
    else:
        assert st["waves_per_group"] == 4
    c.close()


# ---- 4. order control --------------------------------------------------------------------------------------------------

def test_rows_are_added_in_cart_order(built, gpu, model_file):
    seed, n, K, D, L = stage_ref.ORDER_CASE
    c = _cascador(model_file, L, D)
    case = _case(seed, n, K, D, L, outside=0.15)
    d, rows, th, w, want_shapes, want_lbf = case
    # on the CPU first: reversed cart order changes bits of this very data
    rev, _ = stage_ref.stage_update(D, None, train_ref.ref_set(d), w.tolist(), lbf=want_lbf, reverse=True)
    rev = np.array(rev, np.float64)
    changed = int((rev.view(np.uint64) != want_shapes.view(np.uint64)).sum())
    print("coordinates whose bits change under reversed cart order: %d of %d" % (changed, rev.size))
    assert changed >= 1
    _check(c, case)                                                           # the device equals the forward order
    c.close()


# ---- 6. against the trainer --------------------------------------------------------------------------------------------

def test_leaves_equal_the_trainers(built, gpu, model_file):
    D, L, F, K = 3, 5, 24, 3
    c = _cascador(model_file, L, D)
    pd = train_ref.make_samples(61, 200, L, gt_drop=0.2)
    nd = train_ref.make_samples(161, 200, L)
    feats, ths, pos_leaf, neg_leaf = [], [], [], []
    for k in range(K):
        pools = [train_ref.gen_feature_pool(F, L, train_ref.RADIUS, True, 61 + k, node) for node in range(1, 4)]
        flat = stage_ref.pool_array([r for p, _ in pools for r in p])
        got = c.train_cart_cpp(pd, nd, flat, [1, 0, 1], np.array([u for _, u in pools]))
        feats.append(got["features"]); ths.append(got["thresholds"]); pos_leaf.append(got["pos_leaf"]); neg_leaf.append(got["neg_leaf"])
    feats, ths = np.concatenate(feats), np.concatenate(ths)
    base = np.arange(K, dtype=np.int32)[None, :] * (1 << (D - 1))
    assert same(c.gen_lbf_cpp(pd, feats, ths), base + np.stack(pos_leaf, 1).astype(np.int32))
    assert same(c.gen_lbf_cpp(nd, feats, ths), base + np.stack(neg_leaf, 1).astype(np.int32))
    assert len(set(np.stack(neg_leaf, 1).reshape(-1).tolist())) > 2           # a real tree
    c.close()


# ---- 7. against Validate -----------------------------------------------------------------------------------------------

def test_update_equals_validates_first_stage(built, gpu, model_file):
    """A complete T = 1 model whose carts pass everything: the shape Validate leaves for a crop is the mean shape moved
    by stage 0's regression -- what stage_update_shapes_cpp computes from the crop's mode-0 patches."""
    from jda_amd import api, synth
    from oracle import cpp_reading2 as r2
    K, L, D = 70, 5, 4
    p, _ = model_file((1, K, L, D), multi_scale=True)
    m2 = r2.Model2(p)
    c = api.Cascador(p, "double", device=0)
    imgs = [synth.make_frames(1, 160, 120, seed=4)[0], synth.make_frames(1, 131, 97, seed=5)[0]]
    crops = [(0, 0, 0, 48, 48), (0, 30, 21, 77, 77), (0, 100, 50, 37, 61), (1, 5, 9, 70, 53), (1, 83, 49, 48, 48)]
    v = c.validate_cpp(imgs, crops, mode=0)
    assert v["is_face"].all() and (v["carts_n"] == K).all()
    pats = []
    for (i, x, y, w, h) in crops:                                             # resize_mode 0: crop -> o, o -> h, o -> q
        o = c.resize_cv(imgs[i][y:y + h, x:x + w], 48, 48)
        pats.append(np.concatenate([o.reshape(-1), c.resize_cv(o, 36, 36).reshape(-1), c.resize_cv(o, 24, 24).reshape(-1)]))
    inner = (1 << (D - 1)) - 1
    rows = [(ct.scale[i], ct.lm1[i], ct.lm2[i], ct.o1x[i], ct.o1y[i], ct.o2x[i], ct.o2y[i]) for ct in m2.carts[0] for i in range(1, inner + 1)]
    ths = np.array([ct.nth[i] for ct in m2.carts[0] for i in range(1, inner + 1)], np.int32)
    d = dict(patches=np.stack(pats), shapes=np.tile(np.array(m2.mean_shape), (len(crops), 1)), weights=None, residual=None, has_gt=None)
    got = c.stage_update_shapes_cpp(d, stage_ref.pool_array(rows), ths, np.array(m2.w[0]))
    assert same(got, v["shape"])
    assert np.abs(got - d["shapes"]).max() > 0                                # (the regression moved the shapes)
    c.close()


# ---- 8. residency and chunking -----------------------------------------------------------------------------------------

def test_device_patches_and_chunks(built, gpu, model_file):
    import torch
    K, D, L, n = 5, 3, 5, 700
    c = _cascador(model_file, L, D)
    case = _case(23, n, K, D, L)
    d, rows, th, w, want_shapes, want_lbf = case
    pool = stage_ref.pool_array(rows)
    assert _check(c, case)["chunks"] == 1
    dev = dict(d, patches=torch.from_numpy(d["patches"]).cuda())
    shapes, lbf = c.stage_update_shapes_cpp(dev, pool, th, w, want_lbf=True)
    assert same(shapes, want_shapes) and same(lbf, want_lbf)
    assert same(c.gen_lbf_cpp(dev, pool, th), want_lbf)
    c.set_option("workspace_mb", 1)                                           # several chunks of host patches ...
    assert _check(c, case)["chunks"] > 1
    shapes, lbf, st = c.stage_update_shapes_cpp(dev, pool, th, w, want_lbf=True, stats=True)     # ... and of resident ones
    assert same(shapes, want_shapes) and same(lbf, want_lbf) and st["chunks"] >= 1
    c.close()
