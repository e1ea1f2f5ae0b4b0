"""Controls of dialect CPP's restated numerics against definitions nobody here wrote (tests/exact_ref.py): the two
restatements of cv::resize(INTER_LINEAR) against real-valued bilinear interpolation (and torch's, as a third party), the
restated STParameter::Calc against a Kabsch fit through numpy's SVD, and the rotated pack against a real-valued rotation.
The kernels are bit-exact against these restatements (tests/test_gpu_parity.py, test_train_st.py, test_rotate_*.py); what is
asserted here is that the restatements MEAN what they are read to mean -- a misread coordinate convention, border rule, sign or
rounding step moves a result by whole gray levels or by 1e-3 and more, far outside the bounds below.  The bounds on the integer
recipes are derived from their fixed-point steps, not tuned; the one tolerance that had to be measured
(two floating-point routes to the same rotation) carries its measurement.  Not established: bit-level parity with OpenCV.
No GPU.  tests/test_exact_gpu.py runs the kernels against the same definitions and takes its cases from here."""
import math

import numpy as np
import pytest

import exact_ref as ex

# ---- cv::resize(INTER_LINEAR) ------------------------------------------------------------------------------------------------

# (sw, sh, dw, dh)
RESIZE_PAIRS = [(33, 21, 1, 1), (1, 1, 7, 5), (1, 9, 4, 3), (9, 1, 3, 4), (60, 40, 90, 70), (5, 5, 128, 128), (128, 128, 1, 1),
                (99, 80, 50, 40), (100, 80, 50, 40), (101, 80, 50, 40), (48, 48, 36, 36), (48, 48, 24, 24), (77, 77, 48, 48),
                (37, 61, 48, 48), (200, 3, 257, 2), (48, 48, 48, 48), (37, 61, 37, 61)]
KINDS = ("noise", "checker", "white")

# The bound, derived ("What the restated numerics are tied to"), in gray levels.  v is the real-valued bilinear
# value, v' the same with the 11-bit coefficients the recipe uses in place of the real weights:
#   the final step  out = (S + 2) >> 2  with  S = ((b0 * (H0 >> 4)) >> 16) + ((b1 * (H1 >> 4)) >> 16),  4 v' = (b0 H0 + b1 H1) / 2^20:
#     H >> 4 drops less than 1 of H / 16, twice weighed by b0 + b1 = 2048: at most 2048 * (15/16) / 2^16 of S; each >> 16
#     drops less than 1: 4 v' - S lies in [0, 2 + 1920/65536); (S + 2) >> 2 is S / 4 + 1/2 minus one of 0, 1/4, 1/2, 3/4:
#       out - v' in (-(1/2 + 480/65536) - 3/4 + 1/2, +1/2]            |out - v'| < 3/4 + 480/65536
#   the coefficients: round(2048 f) moves a weight by at most 1/4096, the float32 coordinate (below 256, spacing 2^-16) by at
#     most 2^-17; a bilinear surface over values in 0..255 rises by at most 255 per pixel along an axis; two axes:
#       |v' - v| <= 2 * 255 * (1/4096 + 2^-17)
# Sources up to 256 pixels a side (the float32 term).  0.8857 -- below one level, so this and not 1 is asserted.
RESIZE_BOUND = 0.75 + 480 / 65536 + 2 * 255 * (1 / 4096 + 2.0 ** -17)
# the worst |got - exact| measured over every pair x kind below, both restatements (they agree bit for bit): noise, 60x40 -> 90x70.
# Written down for the reader; nothing is asserted against it but that the derived bound lies above it.
RESIZE_MEASURED = 0.7738


def resize_image(kind, sw, sh):
    if kind == "noise":
        return np.random.default_rng(1000 * sw + sh).integers(0, 256, (sh, sw), dtype=np.uint8)
    if kind == "checker":                                   # 0 / 255 from pixel to pixel: the largest gradients there are
        return (((np.arange(sh)[:, None] + np.arange(sw)[None, :]) & 1) * 255).astype(np.uint8)
    return np.full((sh, sw), 255, np.uint8)                 # a constant must come back as a constant


def check_resize(got, img, dw, dh, what):
    """One resized image against the definition: within RESIZE_BOUND everywhere, the rounded block mean at exact 2x, the
    image itself at equal sizes, a constant from a constant.  -> the largest |got - exact|."""
    sh, sw = img.shape
    got = np.asarray(got, np.int64)
    assert got.shape == (dh, dw), what
    worst = float(np.abs(got - ex.bilinear_resize(img, dw, dh)).max())
    assert worst < RESIZE_BOUND, (what, worst)
    if (sw, sh) == (2 * dw, 2 * dh):
        assert np.array_equal(got, ex.box2(img)), what
    if (sw, sh) == (dw, dh):
        assert np.array_equal(got, img), what
    if img.min() == img.max():
        assert (got == int(img[0, 0])).all(), what
    return worst


@pytest.fixture(scope="module")
def oracle(built, tmp_path_factory):
    from jda_amd import synth
    from oracle.pyoracle import Oracle
    p = str(tmp_path_factory.mktemp("exact") / "m.model")
    synth.make_model(2, 8, 5, 3, seed=1).save(p, 8)
    o = Oracle(p)
    yield o
    o.close()


def test_the_bounds_are_the_derived_ones():
    assert RESIZE_MEASURED < RESIZE_BOUND < 1 and abs(RESIZE_BOUND - 0.8857) < 1e-4
    assert ROT_MEASURED < ROT_BOUND and abs(ROT_BOUND - 0.7490) < 1e-4


@pytest.mark.parametrize("which", ["oracle", "reading2"])
def test_resize_restatements_are_bilinear_interpolation(oracle, which):
    from oracle import cpp_reading2 as r2
    resize = oracle.resize_cv if which == "oracle" else r2.resize_cv2
    worst = (-1.0, None)
    for (sw, sh, dw, dh) in RESIZE_PAIRS:
        for kind in KINDS:
            img = resize_image(kind, sw, sh)
            e = check_resize(resize(img, dw, dh), img, dw, dh, (which, kind, sw, sh, dw, dh))
            worst = max(worst, (e, (kind, sw, sh, dw, dh)), key=lambda t: t[0])
    print("%s against float64 bilinear interpolation: worst |diff| = %.4f at %s (bound %.4f)" % (which, worst[0], worst[1], RESIZE_BOUND))


def test_resize_definition_is_torchs_too(oracle):
    """The third party: torch's float64 bilinear interpolation (align_corners=False, no antialias) is the same function as
    exact_ref.bilinear_resize, and both restatements stay within the bound of it as well."""
    import torch
    import torch.nn.functional as F
    from oracle import cpp_reading2 as r2
    gap = 0.0
    for (sw, sh, dw, dh) in RESIZE_PAIRS:
        for kind in KINDS:
            img = resize_image(kind, sw, sh)
            t = F.interpolate(torch.from_numpy(img.astype(np.float64))[None, None], size=(dh, dw), mode="bilinear", align_corners=False,
                              antialias=False)[0, 0].numpy()
            gap = max(gap, float(np.abs(t - ex.bilinear_resize(img, dw, dh)).max()))
            for resize in (oracle.resize_cv, r2.resize_cv2):
                assert np.abs(np.asarray(resize(img, dw, dh), np.int64) - t).max() < RESIZE_BOUND, (kind, sw, sh, dw, dh)
    print("torch float64 interpolate against exact_ref.bilinear_resize: max |diff| = %.3e" % gap)
    assert gap < 1e-9                                       # (255 * a few dozen roundings of float64: 4e-12 measured)


# ---- STParameter::Calc -------------------------------------------------------------------------------------------------------

ST_LS = (1, 2, 3, 5, 27, 68)          # 2L mod 4 is 2 (L = 1, 3, 5, 27) and 0 (2, 68): cv::norm's four-at-a-time loop with and without its tail
# largest difference measured between oracle.cpp_reading2.st_calc and the SVD reference over every case below, both directions:
# the scale relative to the scale, the four rotation entries absolutely (they are entries of a matrix of norm 1).  The two
# routes -- num / den / sqrt against LAPACK's 2 x 2 SVD -- round differently; a misreading (a sign, a transposed matrix, the
# ratio upside down) shows at 1e-3 and more.
ST_MEASURED = 5.56e-16          # (L = 2, a noisy shape, the rotation's sine)
ST_TOL = 16 * ST_MEASURED


def rot_about(shape, deg, scale=1.0, shift=(0.0, 0.0)):
    """The shape turned by deg about its own centroid, scaled about it and moved."""
    p = np.asarray(shape, np.float64).reshape(-1, 2)
    m = p.mean(axis=0)
    c, s = math.cos(math.radians(deg)), math.sin(math.radians(deg))
    q = (p - m) @ np.array([[c, s], [-s, c]]) * scale + m + np.asarray(shift)
    return q.reshape(-1)


def st_mean(L):
    from jda_amd import synth
    return synth.make_mean_shape(L, np.random.default_rng(L))


def st_cases(L):
    """(name, shape) for the mean shape st_mean(L); every one of non-zero norm for L >= 2."""
    mean = st_mean(L)
    rng = np.random.default_rng(100 + L)
    out = [("the mean itself", mean.copy()), ("0 degrees, moved", rot_about(mean, 0, 1.0, (0.25, -0.125)))]
    out += [("%g degrees" % d, rot_about(mean, d, 1.0, (0.01, 0.02))) for d in (90, -90, 179.9, 180)]
    out += [("x 1e-3", rot_about(mean, 20, 1e-3)), ("x 1e3", rot_about(mean, -20, 1e3))]
    for k in range(3):
        noisy = rot_about(mean, rng.uniform(-30, 30), rng.uniform(0.7, 1.4), rng.uniform(-0.1, 0.1, 2))
        out.append(("noisy %d" % k, noisy + rng.normal(0, 0.02, noisy.shape)))
    return out


def st_diff(got, want):
    """The figure ST_MEASURED is about: max(|scale - scale'| / scale', max |r - r'|)."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    return max(abs(got[0] - want[0]) / want[0], float(np.abs(got[1:] - want[1:]).max()))


def degenerate_fields(n1, n2):
    """What IEEE arithmetic leaves of Calc where a centred shape has norm 0: scale = n1 / n2 as it comes (0 / 0 = NaN,
    0 / x = 0, x / 0 = inf); the centred zeros times 1 / 0 = inf are NaN, and so is every rotation entry made of them."""
    with np.errstate(all="ignore"):
        return (float(np.float64(n1) / np.float64(n2)),) + (float("nan"),) * 4


def same_fields(got, want):
    return all((math.isnan(g) and math.isnan(w)) or g == w for g, w in zip(got, want))


def test_st_calc_is_the_kabsch_fit():
    from oracle import cpp_reading2 as r2
    worst = (-1.0, None)
    for L in ST_LS[1:]:
        mean = st_mean(L)
        for name, shape in st_cases(L):
            for a, b, way in ((shape, mean, "mc"), (mean, shape, "cm")):
                got = r2.st_calc([float(v) for v in a], [float(v) for v in b], L)
                want = ex.similarity(a, b, L)
                d = st_diff(got, want)
                worst = max(worst, (d, (L, name, way)), key=lambda t: t[0])
                assert d <= ST_TOL, (L, name, way, d, got, want)
                assert got[1] == got[4] and got[2] == -got[3]            # a rotation matrix, by construction
                # Apply(Calc(a, b)) takes centred b onto centred a as well as the least-squares rotation does; a parameter off
                # by ST_TOL moves scale * R b, a point set of a's norm, by at most 2 * ST_TOL of that norm
                na = float(np.linalg.norm(np.asarray(a).reshape(L, 2) - np.asarray(a).reshape(L, 2).mean(axis=0)))
                assert ex.similarity_residual(a, b, L, got) <= ex.similarity_residual(a, b, L, want) + 2 * ST_TOL * na, (L, name, way)
                # ... through the restatement's own Apply, landmark by landmark
                bc = np.asarray(b, np.float64).reshape(L, 2) - np.asarray(b, np.float64).reshape(L, 2).mean(axis=0)
                ac = np.asarray(a, np.float64).reshape(L, 2) - np.asarray(a, np.float64).reshape(L, 2).mean(axis=0)
                ap = np.array([r2.st_apply(got, float(x), float(y)) for x, y in bc])
                assert np.linalg.norm(ac - ap) <= ex.similarity_residual(a, b, L, want) + 2 * ST_TOL * na, (L, name, way)
    print("st_calc against the SVD reference: largest difference %.3e at %s (tolerance %.3e)" % (worst[0], worst[1], ST_TOL))
    assert worst[0] > 0                                                  # two routes: a bit-equal result would mean one route


def test_st_calc_known_rotations():
    """The reference of the reference: a shape turned by a known angle comes back as that angle, in the header's sense."""
    for L in ST_LS[1:]:
        mean = st_mean(L)
        for d, sc in ((0, 1.0), (90, 1.0), (-90, 2.0), (180, 0.5), (33, 1.0)):
            s, r00, r01, r10, r11 = ex.similarity(rot_about(mean, d, sc), mean, L)
            # rot_about takes a centred point (x, y) to (cx - sy, sx + cy): R = [[c, -s], [s, c]]
            c, sn = math.cos(math.radians(d)), math.sin(math.radians(d))
            assert abs(s - sc) < 1e-12 and max(abs(r00 - c), abs(r01 + sn), abs(r10 - sn), abs(r11 - c)) < 1e-12, (L, d)


def test_st_calc_zero_norm_is_ieee_zero_by_zero():
    """L = 1 and a shape whose landmarks all coincide have zero norm once centred: the reference divides 0 by 0.  Nothing
    there has a meaning to compare with; asserted is only that the restatement returns NaN in the fields where 0 / 0
    would leave one (degenerate_fields), and the scale IEEE division gives."""
    from oracle import cpp_reading2 as r2
    got = r2.st_calc([0.375, 0.625], [0.5, 0.5], 1)
    assert same_fields(got, degenerate_fields(0.0, 0.0)), got
    for L in ST_LS[1:]:
        mean = [float(v) for v in st_mean(L)]
        point = [0.5] * (2 * L)                                          # (L * 0.5 / L is exact: the centred shape is 0.)
        n = float(np.linalg.norm(np.asarray(mean).reshape(L, 2) - np.asarray(mean).reshape(L, 2).mean(axis=0)))
        assert same_fields(r2.st_calc(point, mean, L), degenerate_fields(0.0, n)), L
        assert same_fields(r2.st_calc(mean, point, L), degenerate_fields(n, 0.0)), L
        assert same_fields(r2.st_calc(point, point, L), degenerate_fields(0.0, 0.0)), L


# ---- the rotated pack --------------------------------------------------------------------------------------------------------

ROT_ANGLES = (0.01, 30, 45, -33.3, 135)
ROT_QUARTERS = (0, 90, 180, 270, -90)
ROT_SIZES = ((1, 1), (65, 3), (2, 129), (130, 67))     # (w, h)
# The bound, derived, in gray levels.  The recipe snaps each source coordinate to the nearest 1/1024: at most
# 1/2048 pixel per axis; the bilinear surface over values in 0..255 (0 outside the rectangle) is continuous and rises by at
# most 255 per pixel along an axis: 2 * 255 / 2048.  From the snapped coordinate on the integer weights are the exact ones
# (fx, fy are multiples of 1/1024 and the products are kept whole), so what is left is the final rounding: 1/2.  The float64
# map itself (a dozen roundings of numbers below 2^8, times 255 per pixel) is below 1e-10.
ROT_BOUND = 0.5 + 2 * 255 / 2048 + 1e-10
# the worst |got - exact| measured over every angle x size x image below: the checkerboard, 2 x 129 at 30 degrees (for the reader, as above)
ROT_MEASURED = 0.6620
ROT_EDGE_SHARE = 0.02


def rot_image(kind, w, h):
    if kind == "noise":
        return np.random.default_rng(7 * w + h).integers(0, 256, (h, w), dtype=np.uint8)
    return (((np.arange(h)[:, None] + np.arange(w)[None, :]) & 1) * 255).astype(np.uint8)


def rot_cases():
    return [(w, h, d) for (w, h) in ROT_SIZES for d in ROT_ANGLES + ROT_QUARTERS]


def edge_share(w, h, tw, th, deg):
    """The share of output pixels whose exact source coordinate lies within 1/1024 of the acceptance edge (sx > -1, sx < w,
    sy > -1, sy < h): where the recipe and the definition may decide differently whether the pixel is sampled at all."""
    sx, sy = ex.rotate_coords(w, h, tw, th, deg)
    e = 1.0 / 1024
    near = (np.abs(sx + 1) < e) | (np.abs(sx - w) < e) | (np.abs(sy + 1) < e) | (np.abs(sy - h) < e)
    return float(near.mean()), near


def check_rotated(got, gray, deg, what):
    """One rotated image against the definition.  No pixel is skipped: the definition is 0 beyond the acceptance edge and
    continuous across it (there the only taps left are the zeros outside the rectangle), so a pixel decided the other way is
    wrong by less than 255 / 1024 and stays inside the bound.  The share of such pixels is reported and held below 2 %.
    -> (largest |got - exact|, that share)."""
    h, w = gray.shape
    want = ex.rotate(gray, deg)
    assert got.shape == want.shape and got.dtype == np.uint8, what
    share, _ = edge_share(w, h, want.shape[1], want.shape[0], deg)
    assert share <= ROT_EDGE_SHARE, (what, share)
    worst = float(np.abs(got.astype(np.float64) - want).max())
    assert worst <= ROT_BOUND, (what, worst)
    return worst, share


def test_rotated_pack_is_the_rotation():
    """The host form -- and tests/rotate_ref.py, the restatement both forms are byte-exact against -- on every case."""
    from jda_amd import api
    import rotate_ref as ro
    worst = (-1.0, None)
    for kind in ("noise", "checker"):
        cases = rot_cases()
        imgs = [rot_image(kind, w, h) for (w, h, _) in cases]
        got = api.pack_gray_rotated(imgs, 0, [d for (_, _, d) in cases])
        for g, img, (w, h, d) in zip(got, imgs, cases):
            e, share = check_rotated(g, img, d, (kind, w, h, d))
            check_rotated(ro.rotate_gray(img, api.rotation_plan(w, h, d)), img, d, ("rotate_ref", kind, w, h, d))
            worst = max(worst, (e, (kind, w, h, d)), key=lambda t: t[0])
            if share:
                print("%s %d x %d at %g degrees: %.2f %% of the pixels within 1/1024 of the acceptance edge" % (kind, w, h, d, 100 * share))
            if d in ROT_QUARTERS:
                assert e < 1e-9, (kind, w, h, d, e)          # a quarter turn moves pixels and mixes none
    print("pack_gray_rotated against the float64 rotation: worst |diff| = %.4f at %s (bound %.4f)" % (worst[0], worst[1], ROT_BOUND))


def test_rotation_turns_clockwise_as_displayed():
    """The definition's own sense, on a picture: a bright pixel right of the centre is found below it after +90 degrees (rows
    grow downwards: clockwise as displayed), left of it after 180, above it after 270."""
    img = np.zeros((9, 9), np.uint8)
    img[4, 7] = 200
    for d, (row, col) in ((0, (4, 7)), (90, (7, 4)), (180, (4, 1)), (270, (1, 4)), (-90, (1, 4))):
        r = ex.rotate(img, d)
        assert abs(r[row, col] - 200) < 1e-9 and abs(r.sum() - 200) < 1e-9, d
    r = ex.rotate(img, 45)                                   # 13 x 13; 3 pixels from the centre, towards bottom right
    v, u = np.unravel_index(np.argmax(r), r.shape)
    assert abs(u - (6 + 3 / math.sqrt(2))) <= 0.5 and abs(v - (6 + 3 / math.sqrt(2))) <= 0.5
