"""Building the positive sample set on the device (jdaBuildPositivesCpp*, k_faces.hip) against the restatement
tests/positives_ref.py -- getFace's padded canvas built and sliced, the oracle's resize_cv, numpy's mirror -- byte for byte;
there is no tolerance anywhere.  tests/test_positives_host.py holds the refusals that need no device, the host-only
entries and the record that no flip-after-resize control exists in the searched range.  Dialect CPP is parity-unpinned:
bit-exact against this repo's restatements of the reference's source, not against the reference."""
import numpy as np
import pytest

from conftest import same
import positives_ref as pr
import train_ref

pytestmark = pytest.mark.gpu

TRIPLES = [(48, 36, 24), (5, 3, 2), (7, 5, 3), (128, 128, 128)]      # P = 4176, 38, 83 (odd: every other record misaligned), 49152
COUNTS = [1, 3, 4, 5, 67]                                           # every n_faces mod 4
IMG_SIZES = [(140, 110), (97, 71), (64, 48), (33, 50), (120, 100)]  # (w, h); the last one is referenced by no face


@pytest.fixture(scope="module")
def gpu():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    return torch.device("cuda", 0)


def _images():
    return [pr.noise(40 + i, w, h) for i, (w, h) in enumerate(IMG_SIZES)]


def _faces(sizes):
    """67 face rows for a patch-size triple; the first ones are the named cases (image 0 is 140 x 110: its canvas admits
    x in [-70, 350 - w], y in [-55, 275 - h])."""
    o, h, q = sizes
    f = [(0, -7, -9, 2 * o, 2 * o),                # exactly 2x the o patch, partly outside: zeros enter the box average
         (0, 10, 5, o, o),                         # the o patch's own size: identity
         (0, 60, -11, 2 * h, 2 * h), (0, -5, 15, 2 * q, 2 * q),      # exactly 2x h and 2x q, partly outside
         (0, 17, 23, 1, 1), (0, 30, 40, max(1, q // 2), max(1, q - 1)),      # 1 x 1 and smaller than q: up-scaling
         (0, 20, 10, 37, 61), (1, 5, 3, 70, 53),   # not square
         (0, -10, 20, 50, 50), (0, 110, 20, 50, 50), (0, 40, -12, 50, 50), (0, 40, 80, 50, 50),      # leaves on one side
         (0, -10, -12, 50, 50), (0, 110, 80, 50, 40),                # ... on two at once
         (0, -60, 10, 50, 40),                     # wholly outside the image, inside the canvas: all zeros
         (0, 90, 30, 50, 50), (0, 30, 60, 50, 50), (1, 57, 41, 40, 30),      # x + w == cols, y + h == rows, both
         (0, -70, -55, 30, 30), (0, 320, 250, 30, 25),               # on the canvas limit
         (2, 0, 0, 64, 48), (3, -3, 2, 36, 36), (0, 10, 10, h, h), (1, 1, 1, q, q)]
    rng = np.random.default_rng(sum(sizes))
    while len(f) < 67:
        im = int(rng.integers(0, 4))
        W, H = IMG_SIZES[im]
        w, hh = int(rng.integers(1, min(130, 3 * W) + 1)), int(rng.integers(1, min(130, 3 * H) + 1))
        f.append((im, int(rng.integers(-(W // 2), 3 * W - W // 2 - w + 1)), int(rng.integers(-(H // 2), 3 * H - H // 2 - hh + 1)), w, hh))
    return f


_CACHE = {}


def _want(sizes):
    """(images, faces, records [2 * 67, P] of the restatement with augmentation), computed once per triple."""
    if sizes not in _CACHE:
        from jda_amd import synth
        from oracle.pyoracle import Oracle
        import os
        p = os.path.join(synth.cache_dir(), "positives_1_2_5_3.model")
        synth.make_model(1, 2, 5, 3, seed=1).save(p, 8)
        o = Oracle(p)
        imgs, faces = _images(), _faces(sizes)
        ref = pr.build(o.resize_cv, imgs, faces, sizes, True)
        ref.setflags(write=False)
        o.close()
        _CACHE[sizes] = (imgs, faces, ref)
    return _CACHE[sizes]


def _ref(sizes, n, augment):
    _, _, ref = _want(sizes)
    return np.concatenate([ref[:n], ref[67:67 + n]]) if augment else ref[:n]


def _cascador(model_file):
    from jda_amd import api
    p, _ = model_file((1, 2, 5, 3))
    return api.Cascador(p, "double", device=0)


@pytest.mark.parametrize("augment", [False, True])
@pytest.mark.parametrize("sizes", TRIPLES)
def test_records_equal_the_restatement(built, gpu, model_file, sizes, augment):
    c = _cascador(model_file)
    imgs, faces, ref = _want(sizes)
    for n in COUNTS:
        got, st = c.build_positives_cpp(imgs, faces[:n], None, augment, *sizes, stats=True)
        want = _ref(sizes, n, augment)
        assert got.shape == want.shape and np.array_equal(got, want), (sizes, n)
        assert st["images_uploaded"] == len(set(f[0] for f in faces[:n])) and st["bytes"] == want.size
    P = sum(s * s for s in sizes)
    o2 = sizes[0] ** 2
    assert not ref[14].any() and ref[0].any()                        # the box wholly outside the image is black
    assert np.array_equal(ref[1, :o2].reshape(sizes[0], sizes[0])[:min(sizes[0], 105), :],
                          imgs[0][5:5 + min(sizes[0], 105), 10:10 + sizes[0]])      # identity: the image's own bytes
    assert ref.shape == (134, P)
    c.close()


@pytest.mark.parametrize("sizes", [(48, 36, 24), (7, 5, 3)])
def test_device_images_and_device_dst_with_canaries(built, gpu, model_file, sizes):
    """Host against resident images, host against device dst; dst starts at an odd address inside a larger buffer whose
    other bytes must stay as they were."""
    import torch
    from jda_amd import api
    c = _cascador(model_file)
    imgs, faces, _ = _want(sizes)
    P = sum(s * s for s in sizes)
    dev_imgs = api._pack_images_device(imgs)
    for n, augment in ((67, True), (5, False), (4, True)):
        want = _ref(sizes, n, augment)
        size = want.shape[0]
        for images in (imgs, dev_imgs):
            buf = torch.full((61 + size * P + 77,), 0xA5, dtype=torch.uint8, device="cuda")
            got = c.build_positives_cpp(images, faces[:n], buf[61:61 + size * P], augment, *sizes)
            assert got.data_ptr() == buf.data_ptr() + 61
            host = buf.cpu().numpy()
            assert np.array_equal(host[61:61 + size * P].reshape(size, P), want)
            assert (host[:61] == 0xA5).all() and (host[61 + size * P:] == 0xA5).all()
            hbuf = np.full(61 + size * P + 77, 0xA5, np.uint8)
            c.build_positives_cpp(images, faces[:n], hbuf[61:61 + size * P], augment, *sizes)
            assert np.array_equal(hbuf, host)
    c.close()


def test_one_pixel_past_the_canvas_is_refused_and_dst_untouched(built, gpu, model_file):
    import torch
    from jda_amd import api
    c = _cascador(model_file)
    imgs, faces, _ = _want((48, 36, 24))
    P = 48 * 48 + 36 * 36 + 24 * 24
    for bad in ((0, -71, -55, 30, 30), (0, 321, 250, 30, 25), (0, -70, -56, 30, 30), (0, 320, 251, 30, 25)):
        rows = faces[:5] + [bad]
        buf = torch.full((6 * P + 128,), 0x5A, dtype=torch.uint8, device="cuda")
        hbuf = np.full(6 * P + 128, 0x5A, np.uint8)
        for dst in (buf[64:64 + 6 * P], hbuf[64:64 + 6 * P]):
            with pytest.raises(api.JdaError, match="leaves getFace's padded canvas"):
                c.build_positives_cpp(imgs, rows, dst, False, 48, 36, 24)
        assert (buf.cpu().numpy() == 0x5A).all() and (hbuf == 0x5A).all()
    c.close()


def test_small_workspace_gives_the_same_records_in_chunks(built, gpu, model_file):
    """workspace_mb = 1: 134 records of 49,152 B come back to a host dst in at least 3 chunks; the 71 referenced ones of 80 host images of 15 KB
    are uploaded in at least 3 chunks.  Equal to the one-chunk result."""
    from jda_amd import synth
    from oracle.pyoracle import Oracle
    import os
    c = _cascador(model_file)
    sizes = (128, 128, 128)
    imgs, faces, _ = _want(sizes)
    one, st1 = c.build_positives_cpp(imgs, faces, None, True, *sizes, stats=True)
    assert st1["chunks"] == 1 and st1["image_chunks"] == 1
    many_imgs = [pr.noise(900 + i, 140, 110) for i in range(80)]
    many_faces = [(i, (i * 7) % 60 - 20, (i * 5) % 50 - 15, 20 + i, 95 - i) for i in range(80) if i % 9 != 4]
    one_m, stm1 = c.build_positives_cpp(many_imgs, many_faces, None, True, 5, 3, 2, stats=True)
    c.set_option("workspace_mb", 1)
    got, st = c.build_positives_cpp(imgs, faces, None, True, *sizes, stats=True)
    print("128/128/128, 67 faces, augment, host dst: %d chunks, %d image chunks" % (st["chunks"], st["image_chunks"]))
    assert st["chunks"] >= 3 and np.array_equal(got, one) and np.array_equal(got, _ref(sizes, 67, True))
    got_m, stm = c.build_positives_cpp(many_imgs, many_faces, None, True, 5, 3, 2, stats=True)
    print("80 images of 140 x 110, 71 referenced: %d image chunks" % stm["image_chunks"])
    assert stm["image_chunks"] >= 3 and stm1["image_chunks"] == 1 and stm["images_uploaded"] == stm1["images_uploaded"] == 71
    assert np.array_equal(got_m, one_m)
    p = os.path.join(synth.cache_dir(), "positives_1_2_5_3.model")
    o = Oracle(p)
    assert np.array_equal(got_m, pr.build(o.resize_cv, many_imgs, many_faces, (5, 3, 2), True))
    o.close()
    c.close()


def test_o_patch_of_an_in_image_face_equals_resize_cv_of_the_crop(built, gpu, model_file):
    """Cross-check against an existing entry: for faces inside their image the o patch is Cascador.resize_cv of the numpy crop."""
    c = _cascador(model_file)
    sizes = (48, 36, 24)
    imgs, faces, _ = _want(sizes)
    inside = [f for f in faces if f[1] >= 0 and f[2] >= 0 and f[1] + f[3] <= IMG_SIZES[f[0]][0] and f[2] + f[4] <= IMG_SIZES[f[0]][1]]
    assert len(inside) >= 6
    got = c.build_positives_cpp(imgs, inside, None, False, *sizes)
    for (im, x, y, w, h), rec in zip(inside, got):
        crop = imgs[im][y:y + h, x:x + w]
        assert np.array_equal(rec[:48 * 48].reshape(48, 48), c.resize_cv(crop, 48, 48)), (im, x, y, w, h)
        assert np.array_equal(rec[48 * 48:48 * 48 + 36 * 36].reshape(36, 36), c.resize_cv(crop, 36, 36))
    c.close()


def test_built_positives_train_a_cart(built, gpu, tmp_path):
    """End to end: the built positives (resident, as they are) and 40 mined negatives go into train_cart_cpp; the shapes come
    from random_shapes_cpp, the residual and has_gt from shape_residual_cpp; the cart equals train_ref's on the same inputs."""
    import torch
    from jda_amd import api, synth
    sizes, L, D, F, lid = (48, 36, 24), 5, 3, 64, 2
    p = str(tmp_path / "e2e.model")
    synth.make_model(3, 20, L, D, seed=3, cart_th=synth.NEG_BIG, norm_every=5, multi_scale=True).save(p, 8)
    c = api.Cascador(p, "double", device=0)
    imgs, faces, _ = _want(sizes)
    n, P = len(faces), sum(s * s for s in sizes)
    dst = torch.zeros(2 * n * P, dtype=torch.uint8, device="cuda")
    pos_patches = c.build_positives_cpp(api._pack_images_device(imgs), faces, dst, True, *sizes)
    lm = pr.make_landmarks(8, faces, L, unmasked=(2, 40))
    s = api.positive_shapes_cpp(faces, lm, True, [0, 3], [1, 4])
    cur = api.random_shapes_cpp(s["mean_shape"], 2 * n, 0.05, seed=11)
    res, has_gt = api.shape_residual_cpp(s["gt_shapes"], cur, landmark_id=lid, shape_mask=s["shape_mask"])
    assert has_gt.sum() == 2 * n - 4 and np.isfinite(cur).all()
    rng = np.random.default_rng(4)
    wp = np.exp(-rng.uniform(-4, 4, 2 * n))
    bgs = [synth.make_frames(1, w, h, seed=9, first=i)[0] for i, (w, h) in enumerate([(160, 120), (131, 97)])]
    mined = c.mine_negatives_cpp(bgs, [3, 4], [1.2, 1.25], [0, 3], 40, device=True)
    assert len(mined["score"]) == 40
    wn = np.exp(rng.uniform(-4, 4, 40))
    tot = wp.sum() + wn.sum()
    pd = dict(patches=pos_patches.reshape(-1), shapes=cur, weights=wp / tot, residual=res, has_gt=has_gt, sizes=sizes)
    nd = dict(patches=mined["patches"], shapes=mined["shape"], weights=wn / tot, residual=None, has_gt=None, sizes=sizes)
    pools, us = zip(*[train_ref.gen_feature_pool(F, L, train_ref.RADIUS, True, 8, node) for node in range(1, 4)])
    modes = [1, 0, 1]
    pool = np.zeros(3 * F, api.FEATURE_DTYPE)
    for i, r in enumerate([r for q in pools for r in q]):
        pool[i] = (r[0], r[1], r[2], 0, r[3], r[4], r[5], r[6])
    got = c.train_cart_cpp(pd, nd, pool, modes, np.array(us), *sizes)
    pos = train_ref.ref_set(dict(pd, patches=pos_patches.cpu().numpy().reshape(2 * n, P)))
    neg = train_ref.ref_set(dict(nd, residual=np.zeros((40, 2)), has_gt=np.ones(40, np.uint8)))
    want = train_ref.train_cart(D, pos, neg, [train_ref.pool_of(q) for q in pools], modes, us)
    assert np.array_equal(got["nodes"]["feature_idx"], np.array(want["features"], np.int32))
    assert np.array_equal(got["thresholds"], np.array(want["thresholds"], np.int32))
    assert same(got["scores"], np.array(want["scores"]))
    assert np.array_equal(got["pos_leaf"], np.array(want["pos_leaf"], np.int32))
    assert np.array_equal(got["neg_leaf"], np.array(want["neg_leaf"], np.int32))
    assert len(set(got["pos_leaf"].tolist())) > 1
    c.close()
