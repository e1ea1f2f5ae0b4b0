"""The kernels that carry dialect CPP's restated numerics, run against tests/exact_ref.py DIRECTLY -- not through the oracle
or a *_ref.py restatement by this repository's author: cv_resize_px (k_resize_cv, the mining patches, the positive patches)
against real-valued bilinear interpolation and the rounded 2 x 2 mean, stp_side / stp_rot (k_stp) against the Kabsch fit,
k_rotate against the real-valued rotation, k_chips against the mean of real-valued bilinear samples under the least-squares
fit -- no host form and no tests/chips_ref.py in between --, and jdaRotateBack against k_rotate's own pixels: images that
hold their own coordinates come back rotated, and every landmark of the rotated image must return to what its pixel
holds; then the chain a caller runs, rotate_back into face_chips_device.  The cases, the derived bounds and the measured
tolerances are those of tests/test_exact_host.py, where they are explained; every case here takes well under a second.  What
this does not establish: bit-level parity with OpenCV, anything integer-valued (tree walks, NMS, the enumeration of windows),
the choice of n as a matter of quality, jdaOrientBack / jdaReduceBack beyond their same-pixel tests, k_chips' 64-bit division
path (calls of 2^32 output bytes and more)."""
import math

import numpy as np
import pytest

import chips_ref as cr
import exact_ref as ex
import test_exact_host as th

pytestmark = pytest.mark.gpu

# k_resize_cv takes 256 destination columns per workgroup: one column short of, exactly, and one column into a second group
RESIZE_PAIRS = th.RESIZE_PAIRS + [(131, 7, 255, 5), (128, 7, 256, 5), (130, 5, 257, 4), (200, 3, 255, 2), (200, 3, 256, 2)]
OS, HS, QS = 48, 36, 24


@pytest.fixture(scope="module")
def gpu():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def casc(built, gpu, tmp_path_factory):
    """A multi-scale model that rejects nothing (the test_mine_extremes setup): every window of the mining walk is a hit."""
    from jda_amd import api, synth
    p = str(tmp_path_factory.mktemp("exact_gpu") / "pass.model")
    synth.make_model(3, 20, 5, 4, seed=3, cart_th=synth.NEG_BIG, norm_every=5, multi_scale=True).save(p, 8)
    c = api.Cascador(p, "double", device=0)
    yield c
    c.close()


# ---- cv_resize_px ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("sw,sh,dw,dh", RESIZE_PAIRS)
def test_resize_kernel_is_bilinear_interpolation(casc, sw, sh, dw, dh):
    for kind in th.KINDS:
        img = th.resize_image(kind, sw, sh)
        th.check_resize(casc.resize_cv(img, dw, dh), img, dw, dh, (kind, sw, sh, dw, dh))


def _background(kind, w, h):
    return th.resize_image(kind, w, h)


def test_mining_patches_are_interpolations_of_their_windows(casc):
    """o is the window resized to 48; h and q are resizes of the kernel's own o to 36 and 24, and 48 -> 24 is the exact 2x
    routing: the rounded block mean.  Upright backgrounds (transform 0), so a hit's window is a plain slice of its image."""
    bgs = [_background("noise", 97, 71), _background("checker", 71, 64)]
    r = casc.mine_negatives_cpp(bgs, [7, 5], [1.3, 1.2], [0, 0], 10 ** 6)
    hits = r["hits"]
    assert len(hits) == r["stats"]["total_windows"] > 40 and r["stats"]["nega_n"] == 0
    assert set(int(v) for v in hits[:, 0]) == {0, 1} and len(set(int(v) for v in hits[:, 3])) >= 3      # both images, 48 and two larger windows
    for j, (i, x, y, w) in enumerate(hits):
        crop = bgs[i][y:y + w, x:x + w]
        assert crop.shape == (w, w), (j, i, x, y, w)
        o = r["o"][j]
        th.check_resize(o, crop, OS, OS, ("o", j, i, x, y, w))
        th.check_resize(r["h"][j], o, HS, HS, ("h", j, i, x, y, w))
        th.check_resize(r["q"][j], o, QS, QS, ("q", j, i, x, y, w))
        assert np.array_equal(r["q"][j], ex.box2(o)), ("q is the 2 x 2 mean of o", j)


def test_positive_patches_are_interpolations_of_their_boxes(casc):
    """Every patch of a positive is a resize of the face box itself (boxes inside their image: nothing is padded): sides 25
    (up-scaling), 48 (o is the box, q its block mean), 96 (o is the block mean) and a box that is not square."""
    imgs = [_background("noise", 140, 120), _background("checker", 140, 120)]
    faces = [(0, 3, 5, 25, 25), (0, 10, 7, 48, 48), (0, 20, 11, 96, 96), (0, 30, 13, 37, 61),
             (1, 50, 40, 25, 25), (1, 1, 1, 48, 48), (1, 43, 23, 96, 96), (1, 2, 3, 61, 37)]
    got = casc.build_positives_cpp(imgs, faces, None, False, OS, HS, QS)
    assert got.shape == (len(faces), OS * OS + HS * HS + QS * QS)
    for row, (i, x, y, w, h) in zip(got, faces):
        crop = imgs[i][y:y + h, x:x + w]
        assert crop.shape == (h, w)
        at = 0
        for s in (OS, HS, QS):
            th.check_resize(row[at:at + s * s].reshape(s, s), crop, s, s, ("positive", i, x, y, w, h, s))
            at += s * s


# ---- stp_side / stp_rot ------------------------------------------------------------------------------------------------------

ST_NS = (1, 63, 64, 65, 130)


@pytest.mark.parametrize("L", th.ST_LS)
def test_st_parameters_kernel_is_the_kabsch_fit(built, gpu, L):
    """jdaCalcSTParametersCpp on the host test's shapes, cycled to n = 1, 63, 64, 65 and 130 samples (a wave is 64), against
    the SVD reference in both directions at the host test's tolerance.  Every seventh sample has all its landmarks in one
    point, and with L = 1 every sample has: zero norm, where only the NaN pattern of 0 / 0 is asserted (see the host test)."""
    from jda_amd import api
    mean = th.st_mean(L)
    centred = mean.reshape(L, 2) - mean.reshape(L, 2).mean(axis=0)
    mean_norm = float(np.linalg.norm(centred))
    cases = th.st_cases(L)
    c = api.Cascador.create_training_cpp(1, 1, L, 2, mean, device=0)
    c.set_similarity_transform(True)
    worst = 0.0
    for n in ST_NS:
        shapes, flat = [], []
        for k in range(n):
            point = L == 1 or k % 7 == 6
            shapes.append(np.full(2 * L, 0.5) if point and L > 1 else cases[k % len(cases)][1])
            flat.append(point)
        mc, cm = c.calc_st_parameters_cpp(np.array(shapes))
        assert mc.shape == (n, 5) and cm.shape == (n, 5)
        for k in range(n):
            if flat[k]:
                assert th.same_fields(mc[k], th.degenerate_fields(0.0, mean_norm)), (L, n, k, mc[k])
                assert th.same_fields(cm[k], th.degenerate_fields(mean_norm, 0.0)), (L, n, k, cm[k])
                continue
            for got, want in ((mc[k], ex.similarity(shapes[k], mean, L)), (cm[k], ex.similarity(mean, shapes[k], L))):
                d = th.st_diff(got, want)
                worst = max(worst, d)
                assert d <= th.ST_TOL, (L, n, k, d, got, want)
    print("k_stp against the SVD reference, L = %d: largest difference %.3e (tolerance %.3e)" % (L, worst, th.ST_TOL))
    c.close()


# ---- k_rotate ----------------------------------------------------------------------------------------------------------------

def test_rotation_kernel_is_the_rotation(casc):
    """The host test's angles and sizes in ONE ragged call, as GRAY8 and as BGR24 with B = G = R (the gray conversion is then
    the identity -- the weights sum to 2^14 -- and drops out), noise and checkerboard."""
    import torch
    cases = th.rot_cases()
    grays, tensors, fmts, degs = [], [], [], []
    for kind in ("noise", "checker"):
        for k, (w, h, d) in enumerate(cases):
            g = th.rot_image(kind, w, h)
            colour = (k + (kind == "noise")) % 2 == 1
            src = np.ascontiguousarray(np.repeat(g[:, :, None], 3, axis=2)) if colour else g
            grays.append(g); tensors.append(torch.from_numpy(src).cuda()); fmts.append(1 if colour else 0); degs.append(d)
    assert set(zip(fmts, degs)) == {(f, d) for f in (0, 1) for d in th.ROT_ANGLES + th.ROT_QUARTERS}
    (buf, offs, ws, hs), st = casc.pack_gray_rotated_device(tensors, fmts, degs, stats=True)
    torch.cuda.synchronize()
    assert st["launches"] == 1
    out = buf.cpu().numpy()
    worst = 0.0
    for g, o, w, h, d in zip(grays, offs, ws, hs, degs):
        got = out[int(o):int(o) + w * h].reshape(h, w)
        e, _ = th.check_rotated(got, g, d, (g.shape, d))
        worst = max(worst, e)
        if d in th.ROT_QUARTERS:
            assert e < 1e-9, (g.shape, d, e)
    print("k_rotate against the float64 rotation: worst |diff| = %.4f (bound %.4f)" % (worst, th.ROT_BOUND))
    assert math.isfinite(worst)


# ---- k_chips -----------------------------------------------------------------------------------------------------------------

# (image, scale = source pixels per chip pixel, angle, the template's mean in the image's rectangle): both sides of every
# threshold of n, 0.1 away (chip_face keeps the fitted scale 0.05 away); no angle a multiple of 90 degrees; the last face
# hangs over the bottom right corner of the smallest image, whose last pixel is the last byte of its buffer
CHIP_FACES = [(1, 0.9, 14.0, (30.0, 22.0)), (1, 1.1, -33.0, (36.0, 25.0)), (2, 1.9, 47.0, (25.0, 19.0)), (2, 2.1, 171.0, (24.0, 21.0)),
              (1, 2.9, -101.0, (35.0, 24.0)), (1, 3.1, 62.0, (33.0, 26.0)), (0, 0.8, 29.0, (30.0, 18.0))]
CHIP_NS = [1, 2, 2, 3, 3, 4, 1]


def chips_ragged(cw, ch):
    """3 noise images (33 x 21 GRAY8, 97 x 64 RGBA32 with a rectangle, 51 x 40 BGR24) and CHIP_FACES with noisy landmarks
    -> (images, formats, rectangles, image index per face, landmarks, template)."""
    imgs = [th.chip_source("noise", cr.GRAY8, 33, 21), th.chip_source("noise", cr.RGBA32, 97, 64), th.chip_source("noise", cr.BGR24, 51, 40)]
    tmpl = th.chip_template(cw, ch)
    lm = np.stack([th.chip_face(tmpl, cw, ch, sc, ang, c, 500 + 10 * cw + f) for f, (_, sc, ang, c) in enumerate(CHIP_FACES)])
    return imgs, [cr.GRAY8, cr.RGBA32, cr.BGR24], [None, (10, 6, 70, 50), None], [f[0] for f in CHIP_FACES], lm, tmpl


def pattern(n):
    return ((np.arange(n, dtype=np.int64) * 7 + 13) % 251).astype(np.uint8)


def cut_on_device(casc, imgs, fmts, rects, fi, lm, tmpl, cw, ch, chip_fmt, mis=0, supersample=0):
    """jdaFaceChipsDevice -- ONE launch -- into a patterned buffer, the destination mis bytes behind a 256-byte boundary; the
    guard bytes in front and behind must come back as they were.  Every source is a buffer of its pixels and nothing else.
    -> the chips, uint8 [faces, ch, cw(, 3)]."""
    import torch
    tensors = [torch.from_numpy(np.ascontiguousarray(im)).cuda() for im in imgs]
    shape = (len(fi), ch, cw) + (() if chip_fmt == cr.GRAY8 else (3,))
    nbytes = int(np.prod(shape))
    guard = pattern(256 + mis + nbytes + 64)
    buf = torch.from_numpy(guard.copy()).cuda()
    assert buf.data_ptr() % 256 == 0
    _, st = casc.face_chips_device(tensors, fmts, fi, lm, tmpl, cw, ch, chip_fmt, rects=rects, supersample=supersample, stats=True,
                                   out=buf[256 + mis:256 + mis + nbytes])
    torch.cuda.synchronize()
    assert st["launches"] == 1 and st["faces"] == len(fi) and st["chip_bytes"] == nbytes
    res = buf.cpu().numpy()
    assert np.array_equal(res[:256 + mis], guard[:256 + mis]) and np.array_equal(res[256 + mis + nbytes:], guard[256 + mis + nbytes:])
    return res[256 + mis:256 + mis + nbytes].reshape(shape)


def check_cut(chips, imgs, fmts, rects, fi, lm, tmpl, chip_fmt, supersample=0):
    """Every chip of a call against ex.chip under ex.chip_fit of its landmarks (th.check_chip: the host test's bound and
    conditions) -> (the largest |chip - exact| under each of the two bounds, the reference's n per face, the shares outside)."""
    worst, ns, outside = {False: 0.0, True: 0.0}, [], []
    for f, im in enumerate(fi):
        M = th.exact_fit(lm[f], tmpl, None, rects[im])
        ns.append(supersample or ex.chip_n(M))
        e, gray, out = th.check_chip(chips[f], imgs[im], fmts[im], chip_fmt, M, ns[-1], (chip_fmt, chips.shape, f))
        worst[gray] = max(worst[gray], e)
        outside.append(out)
    return worst, ns, outside


@pytest.mark.parametrize("cw,ch", [(16, 16), (17, 9)])
@pytest.mark.parametrize("chip_fmt", [cr.GRAY8, cr.BGR24])
def test_chip_kernel_cuts_means_of_bilinear_samples(casc, chip_fmt, cw, ch):
    """The ragged set: gray from gray, gray from colour (the Q14 leg), colour from gray, BGR from RGBA and from BGR, at
    n = 1 .. 4, one chip over an image's last corner."""
    s = chips_ragged(cw, ch)
    worst, ns, outside = check_cut(cut_on_device(casc, *s, cw, ch, chip_fmt, mis=7), *s, chip_fmt)
    assert ns == CHIP_NS and outside[-1] >= 0.2
    print("k_chips against the float64 chip: worst |diff| = %.4f (bound %.4f), from colour to gray %.4f (bound %.4f)" %
          (worst[False], th.CHIP_BOUND, worst[True], th.CHIP_GRAY_BOUND))


@pytest.mark.parametrize("cw,ch,mis", [(5, 3, 3), (5, 3, 25), (1, 1, 1)])
def test_chip_kernel_unit_walk(casc, cw, ch, mis):
    """45-byte BGR24 chips: a 16-byte unit begins and ends inside a face and crosses into the next face's record, the
    destination 3 and 25 bytes off a boundary; and 3-byte chips, several faces to a unit."""
    s = chips_ragged(cw, ch)
    _, ns, _ = check_cut(cut_on_device(casc, *s, cw, ch, cr.BGR24, mis=mis), *s, cr.BGR24)
    assert ns == CHIP_NS


def chip_large():
    """One 64 x 64 chip at 3.5 source pixels per chip pixel (n = 4) and 30 degrees out of 300 x 280 BGR24."""
    img = th.chip_source("noise", cr.BGR24, 300, 280)
    tmpl = cr.template(5, 64, 64, np.random.default_rng(64))
    return [img], [cr.BGR24], [None], [0], th.chip_face(tmpl, 64, 64, 3.5, 30.0, (150.0, 140.0), 640)[None], tmpl


def test_chip_kernel_one_large_chip_at_n_4(casc):
    s = chip_large()
    worst, ns, _ = check_cut(cut_on_device(casc, *s, 64, 64, cr.RGB24, mis=5), *s, cr.RGB24)
    assert ns == [4]
    print("k_chips, 64 x 64 at n = 4: worst |diff| = %.4f (bound %.4f)" % (worst[False], th.CHIP_BOUND))


# ---- the rolled-frame way back -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("origin", [(0, 0), (3, 5)])
def test_rotate_back_returns_what_the_rotated_pixels_hold(casc, origin):
    """A[y, x] = x and B[y, x] = y, 130 x 67, packed rotated on the device by 30, -33.3 and 135 degrees in one call.  Bilinear
    interpolation reproduces a linear function, so wherever all four taps lie inside the rectangle the rotated A holds the
    source column and the rotated B the source row of that pixel, to within ROT_BOUND -- k_rotate's own account of where the
    pixel came from.  jdaRotateBack, given the landmark (u, v) of every such pixel, must answer within ROT_BOUND of
    (A'[v, u] + rx, B'[v, u] + ry): a negated angle, a swapped centre or a dropped origin is wrong by pixels.  Once as whole
    images, once as the rectangle at (3, 5) of larger images (200 around it).  The map is also held to ex.rotate_coords itself
    (a dozen float64 roundings of numbers below 2^8: 1e-10, as in ROT_BOUND)."""
    import torch
    from jda_amd import api
    w, h, (rx, ry) = th.WAY_W, th.WAY_H, origin
    A = np.tile(np.arange(w, dtype=np.uint8)[None, :], (h, 1))
    B = np.tile(np.arange(h, dtype=np.uint8)[:, None], (1, w))
    rect = None
    if origin != (0, 0):
        rect = (rx, ry, w, h)
        big = [np.full((h + 11, w + 9), 200, np.uint8) for _ in range(2)]
        big[0][ry:ry + h, rx:rx + w], big[1][ry:ry + h, rx:rx + w] = A, B
        A, B = big
    srcs = [A, B] * len(th.WAY_ANGLES)
    degs = [d for d in th.WAY_ANGLES for _ in range(2)]
    (buf, offs, ws, hs), st = casc.pack_gray_rotated_device([torch.from_numpy(s).cuda() for s in srcs], cr.GRAY8, degs,
                                                            rects=[rect] * len(srcs), stats=True)
    torch.cuda.synchronize()
    assert st["launches"] == 1
    out = buf.cpu().numpy()
    for k, d in enumerate(th.WAY_ANGLES):
        tw, t_h, sx, sy, inside = th.way_interior(d)
        assert (ws[2 * k], hs[2 * k], ws[2 * k + 1], hs[2 * k + 1]) == (tw, t_h, tw, t_h)
        Ar, Br = (out[int(offs[i]):int(offs[i]) + tw * t_h].reshape(t_h, tw).astype(np.float64) for i in (2 * k, 2 * k + 1))
        assert inside.sum() >= 0.9 * (w - 2) * (h - 2), d
        assert np.abs(Ar - sx)[inside].max() <= th.ROT_BOUND and np.abs(Br - sy)[inside].max() <= th.ROT_BOUND, d
        v, u = np.nonzero(inside)
        lm = np.stack([u, v], 1).astype(np.float64)
        for dtype in (np.float64, np.float32):
            _, back = api.rotate_back([A], cr.GRAY8, [d], np.zeros(len(lm), np.int32), landmarks=lm.astype(dtype), rects=[rect])
            assert back.dtype == dtype and back.shape == lm.shape
            assert np.abs(back[:, 0] - (Ar[v, u] + rx)).max() <= th.ROT_BOUND and np.abs(back[:, 1] - (Br[v, u] + ry)).max() <= th.ROT_BOUND, (d, dtype)
            if dtype == np.float64:
                assert np.abs(back[:, 0] - (sx[v, u] + rx)).max() <= 1e-10 and np.abs(back[:, 1] - (sy[v, u] + ry)).max() <= 1e-10, d


def test_chain_back_from_a_rolled_frame_to_chips(casc):
    """The chain a caller runs (th.chain_case): landmarks in the source frame -> the rotated images by the exact inverse of
    ex.rotate_coords -> rotate_back -> face_chips_device on the SOURCE, against ex.chip under ex.chip_fit of the original
    landmarks."""
    from jda_amd import api
    img, tmpl, lm, fi, degs, rot = th.chain_case()
    _, back = api.rotate_back([img, img], cr.BGR24, degs, fi, landmarks=rot)
    chips = cut_on_device(casc, [img, img], [cr.BGR24] * 2, [None, None], fi, back, tmpl, 16, 16, cr.RGB24, mis=9)
    d = th.check_chain(chips, back, img, tmpl, lm, "k_chips")
    print("rotate_back after the exact inverse: largest landmark difference %.3e (tolerance %.3e)" % (d, th.WAY_BACK_TOL))
