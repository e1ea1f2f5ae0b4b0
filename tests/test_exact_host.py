"""Controls of dialect CPP's restated numerics against definitions nobody here wrote (tests/exact_ref.py): the two
restatements of cv::resize(INTER_LINEAR) against real-valued bilinear interpolation (and torch's, as a third party), the
restated STParameter::Calc against a Kabsch fit through numpy's SVD, and the rotated pack against a real-valued rotation.
The kernels are bit-exact against these restatements (tests/test_gpu_parity.py, test_train_st.py, test_rotate_*.py); what is
asserted here is that the restatements MEAN what they are read to mean -- a misread coordinate convention, border rule, sign or
rounding step moves a result by whole gray levels or by 1e-3 and more, far outside the bounds below.  The bounds on the integer
recipes are derived from their fixed-point steps, not tuned; the one tolerance that had to be measured
(two floating-point routes to the same rotation) carries its measurement.  Not established: bit-level parity with OpenCV.
Likewise the face chips ("faces as they leave"): the host form's and tests/chips_ref.py's fit against the least-squares
solution through np.linalg.lstsq (a measured tolerance, CHIP_FIT_MEASURED), their pixels against the mean of real-valued
bilinear samples under the REFERENCE's own matrix (a derived bound, CHIP_BOUND).
No GPU.  tests/test_exact_gpu.py runs the kernels against the same definitions and takes its cases from here."""
import math
import os
import re

import numpy as np
import pytest

import chips_ref as cr
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


# ---- face chips: the fit -----------------------------------------------------------------------------------------------------

CHIP_FIT_LS = (2, 3, 5, 27, 68)
# (scale = source pixels per chip pixel, angle in degrees)
CHIP_FIT_POSES = ((0.3, 0), (0.7, 13), (1.05, -31), (1.3, 90), (1.9, 77), (2.2, -90), (2.6, 160), (0.55, 179.9), (3.1, 180), (3.7, -100))
# largest difference measured between an implementation's matrix (jdaFaceChips and chips_ref.fit give the same bits) and
# ex.chip_fit over every case of fit_cases(): a, b relative to the scale hypot(a, b), tx, ty relative to the largest landmark
# coordinate in the whole image (fit_diff).  The two routes -- means / den / sa / sb against LAPACK's SVD of the uncentred
# 2m x 4 system -- round differently; a misreading (a sign, the transpose, a dropped origin) shows at 1e-2 and more.
CHIP_FIT_MEASURED = 9.21e-14         # (L = 2, x 0.55 at 179.9 degrees, float32 landmarks: two template points 1.8 chip pixels apart, 13 from the origin)
CHIP_FIT_TOL = 16 * CHIP_FIT_MEASURED


def fit_cases():
    """(name, landmarks [2L] float32 or float64 in the rectangle's coordinates, template [2L], use or None, rectangle or None):
    every L x every pose, the template's mean placed at 20..56 x 15..42 of the rectangle, each landmark moved by up to 2 % of
    the face's size, so that no similarity passes through them; masks (from L = 3 on; two landmarks stay at L = 3),
    rectangle origins and the landmarks' type alternate so that every L and every pose meets each."""
    out = []
    for L in CHIP_FIT_LS:
        rng = np.random.default_rng(200 + L)
        tmpl = cr.template(L, 16, 16, rng)
        for k, (sc, ang) in enumerate(CHIP_FIT_POSES):
            lm = cr.place(tmpl, sc, ang, (20.0 + 4 * k, 15.0 + 3 * k), rng, 0.02 * sc * 16)
            lm = lm.astype(np.float32) if (k + L) % 2 else lm
            use = np.array([i % 3 != 1 for i in range(L)], np.uint8) if L >= 3 and k % 2 == 1 else None
            rect = (6, 4, 100, 90) if (k + L) % 3 == 2 else None
            out.append(("L = %d, x %g at %g degrees, %s%s%s" % (L, sc, ang, lm.dtype.name, ", masked" if use is not None else "", ", rectangle" if rect else ""),
                        lm, tmpl, use, rect))
    return out


def exact_fit(lm, tmpl, use=None, rect=None):
    """ex.chip_fit on the landmarks as the implementation reads them (floats widened), the rectangle's origin added as a plain
    translation -> M, float64 [6]."""
    M = ex.chip_fit(np.asarray(lm).astype(np.float64), tmpl, use)
    if rect is not None:
        M[2] += rect[0]
        M[5] += rect[1]
    return M


def fit_scale(M):
    return math.hypot(M[0], M[3])


def fit_pmax(lm, rect=None):
    """The largest landmark coordinate, in the whole image."""
    p = np.abs(np.asarray(lm, np.float64).reshape(-1, 2) + (np.asarray(rect[:2], np.float64) if rect is not None else 0.0))
    return float(p.max())


def fit_diff(got, want, pmax):
    """The figure CHIP_FIT_MEASURED is about: max(|a - a'|, |b - b'|) / scale' and max(|tx - tx'|, |ty - ty'|) / pmax, the larger."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    return max(float(np.abs(got[[0, 1, 3, 4]] - want[[0, 1, 3, 4]]).max()) / fit_scale(want), float(np.abs(got[[2, 5]] - want[[2, 5]]).max()) / pmax)


def check_fit(got, lm, tmpl, use, rect, what):
    """One implementation's matrix against the least-squares solution: within CHIP_FIT_TOL, a similarity by construction, and
    with a residual sum_i ||p_i - M q_i||^2 no larger than the solution's plus what a matrix off by the tolerance adds: every
    coordinate of M q_i then moves by at most e_i = CHIP_FIT_TOL * (scale * (|qx_i| + |qy_i|) + pmax), the residual VECTOR by at
    most E = sqrt(2 sum_i e_i^2) in norm, so the sum of squares is at most (sqrt(S') + E)^2.  -> fit_diff."""
    want = exact_fit(lm, tmpl, use, rect)
    pmax = fit_pmax(lm, rect)
    got = np.asarray(got, np.float64)
    d = fit_diff(got, want, pmax)
    assert d <= CHIP_FIT_TOL, (what, d, got, want)
    assert got[0] == got[4] and got[1] == -got[3], what
    whole = np.asarray(lm).astype(np.float64).reshape(-1, 2) + (np.asarray(rect[:2], np.float64) if rect is not None else 0.0)
    q = np.abs(np.asarray(tmpl, np.float64).reshape(-1, 2))[np.ones(len(tmpl) // 2, bool) if use is None else np.asarray(use) != 0]
    e = CHIP_FIT_TOL * (fit_scale(want) * q.sum(axis=1) + pmax)
    E = math.sqrt(2 * float((e * e).sum()))
    assert ex.chip_residual(whole, tmpl, got, use) <= (math.sqrt(ex.chip_residual(whole, tmpl, want, use)) + E) ** 2, what
    return d


def test_chip_fit_is_the_least_squares_similarity(built):
    """jdaFaceChips' matrices and chips_ref.fit against np.linalg.lstsq on every case of fit_cases()."""
    from jda_amd import api
    img = np.zeros((100, 110), np.uint8)
    worst = (-1.0, None)
    for name, lm, tmpl, use, rect in fit_cases():
        _, M = api.face_chips([img], "gray8", [0], lm[None], tmpl, 1, 1, "gray8", rects=[rect], use=use, matrices=True)
        d = check_fit(M[0], lm, tmpl, use, rect, ("host form", name))
        worst = max(worst, (d, name), key=lambda t: t[0])
        check_fit(cr.fit([float(v) for v in lm], tmpl, use, rect[:2] if rect else (0, 0)), lm, tmpl, use, rect, ("chips_ref", name))
        residual = ex.chip_residual(np.asarray(lm, np.float64), tmpl, ex.chip_fit(np.asarray(lm, np.float64), tmpl, use), use)
        if (len(tmpl) // 2 if use is None else int(use.sum())) > 2:      # a genuine least-squares fit: no similarity passes through
            assert residual > 1e-3 * fit_scale(M[0]) ** 2, name          # (through two points one always does)
    print("chip fit against np.linalg.lstsq: largest difference %.3e at %s (tolerance %.3e)" % (worst[0], worst[1], CHIP_FIT_TOL))
    assert worst[0] > 0                                                  # two routes: a bit-equal result would mean one route


def test_chip_fit_known_maps():
    """The reference of the reference: landmarks that ARE a similarity of the template come back as that similarity, in the
    header's sense -- chip pixel (u, v) lies at (a u - b v + tx, b u + a v + ty) -- and the mask leaves a landmark out."""
    rng = np.random.default_rng(5)
    tmpl = cr.template(5, 16, 16, rng)
    q = tmpl.reshape(-1, 2)
    for sc, ang, t in ((1.0, 0, (0.0, 0.0)), (2.0, 90, (30.0, 20.0)), (0.5, -90, (3.0, 4.0)), (1.5, 180, (40.0, 40.0)), (3.0, 33, (-5.0, 7.5))):
        a, b = sc * math.cos(math.radians(ang)), sc * math.sin(math.radians(ang))
        p = np.stack([a * q[:, 0] - b * q[:, 1] + t[0], b * q[:, 0] + a * q[:, 1] + t[1]], 1)
        assert np.abs(ex.chip_fit(p, tmpl) - np.array([a, -b, t[0], b, a, t[1]])).max() < 1e-12, (sc, ang)
        assert abs(ex.chip_residual(p, tmpl, ex.chip_fit(p, tmpl))) < 1e-20
        moved = p.copy()
        moved[2] += 5.0
        assert np.abs(ex.chip_fit(moved, tmpl, [1, 1, 0, 1, 1]) - np.array([a, -b, t[0], b, a, t[1]])).max() < 1e-12
        assert np.abs(ex.chip_fit(moved, tmpl) - np.array([a, -b, t[0], b, a, t[1]])).max() > 0.1


# ---- face chips: the pixels --------------------------------------------------------------------------------------------------

CHIP_SRC_W, CHIP_SRC_H = 61, 47
CHIP_SIZES = ((1, 1), (5, 3), (16, 16), (17, 9))                 # (cw, ch)
CHIP_POSES = ((0.7, 13), (1.05, -31), (1.9, 77), (2.6, 160), (3.7, -100))
CHIP_CORNERS = ((1.3, 20, (5.0, 4.0)), (2.4, -50, (55.0, 42.0)))  # (scale, angle, centre): 16 x 16 chips over two corners of the image
# (source format, chip format)
CHIP_LEGS = ((cr.GRAY8, cr.GRAY8), (cr.BGR24, cr.BGR24), (cr.BGR24, cr.RGB24), (cr.GRAY8, cr.BGR24), (cr.BGRA32, cr.GRAY8))
CHIP_RECT = (4, 3, 50, 40)                                       # the checkerboard's faces are given in this rectangle's coordinates
# What every case keeps to, so that the slack below covers it (asserted per chip in check_chip; the 64 x 64 chip out of a
# 300 x 280 source of tests/test_exact_gpu.py included): scale below 4, chip sides up to 64, landmarks below 512.
CHIP_SCALE_MAX, CHIP_SIDE_MAX, CHIP_P_MAX = 4.0, 64, 512.0
# The bound, derived, in gray levels, between a chip byte and ex.chip under the REFERENCE's matrix M':
#   (1) the matrix.  The implementation's M is within CHIP_FIT_TOL of M' in the sense of fit_diff, so a sample's source
#       coordinate  sx = a cu - b cv + tx  differs by at most CHIP_FIT_TOL * (scale * (|cu| + |cv|) + pmax) per axis, below
#       CHIP_FIT_TOL * (CHIP_SCALE_MAX * 2 * CHIP_SIDE_MAX + CHIP_P_MAX) =: dm  (the dozen float64 roundings of the map itself,
#       2^-53 of numbers below 2^11 each, are below 1e-11 and inside the 1e-10 added at the end);
#   (2) the recipe snaps each coordinate to the nearest 1/1024: at most 1/2048 per axis;
#   (3) the bilinear surface of an image over 0..255 extended by zeros is continuous and rises by at most 255 per pixel along
#       an axis, so a sample taken (1/2048 + dm) away per axis is off by at most 2 * 255 * (1/2048 + dm).  From the snapped
#       coordinate on the integer weights are the exact ones (fx, fy are multiples of 1/1024, the products are kept whole) and a
#       tap outside the image is the zero of the extension.  A sample the recipe refuses (sx <= -1, sx >= W, ...) lies where the
#       surface is 0 by itself, and one it accepts within 1/2048 of that edge snaps onto the edge, where the surface is 0 too:
#       the acceptance test changes no value, and no pixel needs to be left out;
#   (4) the mean of the n^2 samples is off by no more than each of them;
#   (5) the last step: with S the sum of tap * weight (the samples times 2^20) and N = n^2,
#       ((S + N 2^19) >> 20) / N = floor(floor(S / 2^20 + N / 2) / N) = floor((S / 2^20 + N / 2) / N) = floor(S / (2^20 N) + 1/2)
#       (floor(floor(x) / N) = floor(x / N) for an integer N): the snapped samples' mean rounded to nearest, off by at most 1/2.
CHIP_SLACK = 2 * 255 * CHIP_FIT_TOL * (CHIP_SCALE_MAX * 2 * CHIP_SIDE_MAX + CHIP_P_MAX)
CHIP_BOUND = 0.5 + 2 * 255 / 2048 + CHIP_SLACK + 1e-10
# A colour source cut to a gray chip: every TAP is made gray first, t = (B kB + G kG + R kR + 2^13) >> 14 = floor(g + 1/2) for
# g = (B kB + G kG + R kR) / 2^14: off by at most 1/2 from g; the bilinear weights of a sample are non-negative and sum to 1
# (the taps outside are 0 either way), so are a pixel's: the chip moves by at most 1/2.  g against gray601: the image of
# g - gray601 has values within 255 * (|kB / 2^14 - 0.114| + |kG / 2^14 - 0.587| + |kR / 2^14 - 0.299|), and so has its chip.
GRAY_Q14 = (1868, 9617, 4899)                                    # kernels.h: kGrayB, kGrayG, kGrayR (test_the_chip_bounds_are_the_derived_ones reads them there)
GRAY_WEIGHT_GAP = 255 * sum(abs(k / 16384 - w) for k, w in zip(GRAY_Q14, (0.114, 0.587, 0.299)))
CHIP_GRAY_BOUND = CHIP_BOUND + 0.5 + GRAY_WEIGHT_GAP
# the worst |got - exact| measured over every case below (host form and restatement alike): for the reader, as ROT_MEASURED
CHIP_MEASURED = 0.6079          # (noise, BGR24 -> RGB24, 16 x 16, x 1.9 at 77 degrees with n forced to 1)
CHIP_GRAY_MEASURED = 0.8516     # (noise, BGRA32 -> GRAY8, 16 x 16, x 1.05 at -31 degrees)
CHIP_EDGE_SHARE = 0.02


def test_the_chip_bounds_are_the_derived_ones():
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "jda_amd", "csrc", "kernels.h")).read()
    m = re.search(r"kGrayB = (\d+), kGrayG = (\d+), kGrayR = (\d+)", text)
    assert m and tuple(int(v) for v in m.groups()) == GRAY_Q14 and sum(GRAY_Q14) == 1 << 14
    assert 0 < CHIP_FIT_MEASURED < 1e-12 and CHIP_SLACK < 1e-5
    assert CHIP_MEASURED < CHIP_BOUND and abs(CHIP_BOUND - 0.7490) < 1e-4
    assert abs(GRAY_WEIGHT_GAP - 0.0127) < 1e-4
    assert CHIP_GRAY_MEASURED < CHIP_GRAY_BOUND and abs(CHIP_GRAY_BOUND - 1.2617) < 1e-4


def chip_source(kind, fmt, w=CHIP_SRC_W, h=CHIP_SRC_H):
    """uint8 [h, w] (GRAY8) or [h, w, 3 or 4]: noise, or a 0 / 255 checkerboard; a colour image has three visibly different
    channels (independent noise; checkerboards of phase 0, of phase 1 and of 2-pixel columns), alpha is noise never to be read."""
    c = cr.pr.BPP[fmt]
    if kind == "noise":
        img = np.random.default_rng(1000 * w + 10 * h + fmt).integers(0, 256, (h, w, c), dtype=np.uint8)
    else:
        y, x = np.arange(h)[:, None], np.arange(w)[None, :]
        planes = [((x + y) & 1) * 255, ((x + y + 1) & 1) * 255, (((x >> 1) + y) & 1) * 255, (x * 7 + y * 13) & 255]
        img = np.stack(planes[:c], 2).astype(np.uint8)
    return np.ascontiguousarray(img[..., 0] if fmt == cr.GRAY8 else img)


def chip_exact_source(img, src_fmt, chip_fmt):
    """What the chip is a warp of, from the formats' meaning: float64 [H, W] or [H, W, 3] in the chip's channel order ->
    (that image, the bound that applies)."""
    a = np.asarray(img, np.float64)
    if src_fmt == cr.GRAY8:
        return (a if chip_fmt == cr.GRAY8 else np.repeat(a[..., None], 3, 2)), CHIP_BOUND
    bgr = a[..., :3] if src_fmt in (cr.BGR24, cr.BGRA32) else a[..., 2::-1]
    if chip_fmt == cr.GRAY8:
        return ex.gray601(bgr), CHIP_GRAY_BOUND
    return (bgr if chip_fmt == cr.BGR24 else bgr[..., ::-1]), CHIP_BOUND


def chip_template(cw, ch):
    return cr.template(5, cw, ch, np.random.default_rng(300 + 17 * cw + ch))


def chip_face(tmpl, cw, ch, scale, angle, centre, seed):
    """Noisy landmarks (each moved by up to 2 % of the face's size) for a face of the given pose.  The noise is redrawn until
    the REFERENCE's own fit keeps the scale at least 0.05 away from 1, 2 and 3, so that n is not under test at its thresholds
    (tests/test_chips_host.py walks those)."""
    for k in range(64):
        lm = cr.place(tmpl, scale, angle, centre, np.random.default_rng(10000 * seed + k), 0.02 * scale * max(cw, ch))
        if min(abs(fit_scale(ex.chip_fit(lm, tmpl)) - t) for t in (1, 2, 3)) >= 0.05:
            return lm
    raise AssertionError("no noise keeps x %g away from the thresholds" % scale)


def chip_faces(cw, ch, rect=None):
    """(template, landmarks [faces, 10] in the rectangle's coordinates): CHIP_POSES about the image's centre, and for 16 x 16
    chips CHIP_CORNERS."""
    tmpl = chip_template(cw, ch)
    poses = [(sc, ang, (CHIP_SRC_W / 2 - 0.5 + k, CHIP_SRC_H / 2 - 1.25 * k)) for k, (sc, ang) in enumerate(CHIP_POSES)]
    poses += list(CHIP_CORNERS) if (cw, ch) == (16, 16) else []
    o = np.asarray(rect[:2] if rect else (0, 0), np.float64)
    return tmpl, np.stack([chip_face(tmpl, cw, ch, sc, ang, np.asarray(c) - o, 100 * cw + ch + f) for f, (sc, ang, c) in enumerate(poses)])


def chip_edge_share(M, W, H, cw, ch, n):
    """The share of samples whose exact source coordinate lies within 1/1024 of the acceptance edge (sx > -1, sx < W, sy > -1,
    sy < H), and the share outside the image's pixels altogether."""
    sx, sy = ex.chip_coords(M, cw, ch, n)
    e = 1.0 / 1024
    near = (np.abs(sx + 1) < e) | (np.abs(sx - W) < e) | (np.abs(sy + 1) < e) | (np.abs(sy - H) < e)
    out = (sx < -0.5) | (sx > W - 0.5) | (sy < -0.5) | (sy > H - 0.5)
    return float(near.mean()), float(out.mean())


def fit_gain(tmpl, cw, ch, use=None):
    """How far a sample of a cw x ch chip can move per unit of landmark error: the fit is linear in the landmarks, so a source
    coordinate of chip point q is sum_j G_j(q) p_j over the 2L landmark values, and landmarks off by at most d move it by at
    most d * sum_j |G_j(q)| -- a convex function of q, largest at a corner of the sampled area [-1/2, cw - 1/2] x [-1/2, ch - 1/2].
    From ex.chip_fit alone: G_j is the fit of the j-th unit vector."""
    cols = np.stack([ex.chip_fit(np.eye(len(tmpl))[j], tmpl, use) for j in range(len(tmpl))])
    return max(float(np.abs(cols[:, k] * cu + cols[:, k + 1] * cv + cols[:, k + 2]).sum())
               for cu in (-0.5, cw - 0.5) for cv in (-0.5, ch - 0.5) for k in (0, 3))


def check_chip(got, img, src_fmt, chip_fmt, M, n, what, extra=0.0):
    """One chip against the definition under the reference's own M (and n = ex.chip_n(M) unless forced).  No pixel is
    skipped.  The shares are the reference's alone: samples near the acceptance edge below 2 %, non-zero pixels at least a
    third.  extra: what a caller has derived on top of the bound (landmarks that went through another step first).
    -> (largest |got - exact|, whether the gray-conversion bound applied, the share of samples outside the image)."""
    src, bound = chip_exact_source(img, src_fmt, chip_fmt)
    nonzero = 1 / 3
    H, W = src.shape[:2]
    ch, cw = got.shape[:2]
    assert got.dtype == np.uint8 and got.shape == (ch, cw) + src.shape[2:], what
    assert fit_scale(M) < CHIP_SCALE_MAX and max(cw, ch) <= CHIP_SIDE_MAX and max(W, H) <= CHIP_P_MAX, what
    assert min(abs(fit_scale(M) - t) for t in (1, 2, 3)) >= 0.05, what
    want = ex.chip(src, M, cw, ch, n)
    near, outside = chip_edge_share(M, W, H, cw, ch, n)
    if near:
        print("%s: %.2f %% of the samples within 1/1024 of the acceptance edge" % (what, 100 * near))
    assert near <= CHIP_EDGE_SHARE, (what, near)
    assert (want.reshape(ch * cw, -1).max(axis=1) > 0).mean() >= nonzero, what
    worst = float(np.abs(got.astype(np.float64) - want).max())
    assert worst <= bound + extra, (what, worst, bound + extra)
    return worst, bound == CHIP_GRAY_BOUND, outside


def chip_set(kind, src_fmt, cw, ch):
    """One call's worth: (image, rectangle or None, template, landmarks, the reference's matrices)."""
    img = chip_source(kind, src_fmt)
    rect = CHIP_RECT if kind == "checker" else None
    tmpl, lm = chip_faces(cw, ch, rect)
    return img, rect, tmpl, lm, [exact_fit(p, tmpl, None, rect) for p in lm]


@pytest.mark.parametrize("leg", CHIP_LEGS, ids=lambda l: "%d-%d" % l)
@pytest.mark.parametrize("kind", ["noise", "checker"])
def test_chips_are_means_of_bilinear_samples(built, kind, leg):
    """The host form on every chip size, and tests/chips_ref.py (pure Python: the 16 x 16 and 17 x 9 chips only) with its OWN fit
    and n, against ex.chip under ex.chip_fit."""
    from jda_amd import api
    src_fmt, chip_fmt = leg
    worst, outside = {False: (-1.0, None), True: (-1.0, None)}, []
    for cw, ch in CHIP_SIZES:
        img, rect, tmpl, lm, Ms = chip_set(kind, src_fmt, cw, ch)
        forms = [("host form", api.face_chips([img], src_fmt, [0] * len(lm), lm, tmpl, cw, ch, chip_fmt, rects=[rect]))]
        if cw * ch > 100:
            forms.append(("chips_ref", cr.chips([img], [src_fmt], [rect], [0] * len(lm), lm, tmpl, cw, ch, chip_fmt)[0]))
        for form, got in forms:
            for f, M in enumerate(Ms):
                e, gray, out = check_chip(got[f], img, src_fmt, chip_fmt, M, ex.chip_n(M), (form, kind, leg, cw, ch, f))
                worst[gray] = max(worst[gray], (e, (form, cw, ch, f)), key=lambda t: t[0])
                outside += [out] if form == "host form" else []
    assert sum(o >= 0.2 for o in outside) >= 2 and min(outside) == 0.0       # faces that leave the image, and faces that do not
    for gray, (e, at) in worst.items():
        if at:
            print("%s %s: worst |chip - exact| = %.4f at %s (bound %.4f); samples outside the image %.2f ... %.2f" %
                  (kind, leg, e, at, CHIP_GRAY_BOUND if gray else CHIP_BOUND, min(outside), max(outside)))


@pytest.mark.parametrize("n", [1, 2, 3, 4])
def test_chips_with_forced_n_are_means_of_n_by_n_samples(built, n):
    """x 1.9 at 77 degrees with n forced 1..4 (the reference takes the same n: it is an argument, not a result)."""
    from jda_amd import api
    for leg in (CHIP_LEGS[0], CHIP_LEGS[2]):
        for cw, ch in CHIP_SIZES[2:]:
            img, rect, tmpl, lm, Ms = chip_set("noise", leg[0], cw, ch)
            got = api.face_chips([img], leg[0], [0], lm[2:3], tmpl, cw, ch, leg[1], supersample=n)
            ref = cr.chips([img], [leg[0]], None, [0], lm[2:3], tmpl, cw, ch, leg[1], supersample=n)[0]
            check_chip(got[0], img, leg[0], leg[1], Ms[2], n, ("host form", leg, cw, ch, n))
            check_chip(ref[0], img, leg[0], leg[1], Ms[2], n, ("chips_ref", leg, cw, ch, n))
            if n != ex.chip_n(Ms[2]):                                          # (n matters: the test can tell them apart)
                assert np.abs(ex.chip(chip_exact_source(img, *leg)[0], Ms[2], cw, ch, n) - ex.chip(chip_exact_source(img, *leg)[0], Ms[2], cw, ch, ex.chip_n(Ms[2]))).max() > 1


# ---- the rolled-frame way back -----------------------------------------------------------------------------------------------

WAY_W, WAY_H = 130, 67
WAY_ANGLES = (30, -33.3, 135)
# the largest coordinate difference, in pixels, that jdaRotateBack leaves on chain_case()'s landmarks after ex.rotate_inverse
# took them to the rotated images (coordinates below 128: two float64 routes through a rotation and back)
WAY_BACK_MEASURED = 7.11e-15
WAY_BACK_TOL = 16 * WAY_BACK_MEASURED


def way_interior(deg, w=WAY_W, h=WAY_H):
    """(tw, th, sx, sy, inside) for a w x h rectangle rotated by deg: the exact source coordinates of every pixel of the rotated
    image and which of them have all four taps inside the rectangle -- where bilinear interpolation reproduces a linear image."""
    from jda_amd import api
    plan = api.rotation_plan(w, h, deg)
    sx, sy = ex.rotate_coords(w, h, plan["tw"], plan["th"], deg)
    return plan["tw"], plan["th"], sx, sy, (sx >= 0) & (sx <= w - 1) & (sy >= 0) & (sy <= h - 1)


def test_way_back_angles_keep_the_interior(built):
    """A condition of tests/test_exact_gpu.py's way-back test, on the definition alone: at each angle at least
    0.9 (w - 2)(h - 2) pixels of the rotated image have their four taps inside (the rotation preserves area)."""
    for d in WAY_ANGLES:
        inside = way_interior(d)[4]
        print("%g degrees: %d pixels with four taps inside, %d asked for" % (d, inside.sum(), 0.9 * (WAY_W - 2) * (WAY_H - 2)))
        assert inside.sum() >= 0.9 * (WAY_W - 2) * (WAY_H - 2), d


def chain_case():
    """What a caller of the rolled-frame entries runs: a 97 x 64 BGR24 frame, CHIP_POSES' faces about its centre with noisy
    landmarks (chip_face), the frame rotated by 30 and by -33.3 degrees and each face found on one of the two: -> (image,
    template, landmarks in the source frame [5, 10], image index per face, angles, the landmarks in the rotated images by the
    exact inverse of ex.rotate_coords)."""
    from jda_amd import api
    W, H, degs = 97, 64, (30.0, -33.3)
    img = chip_source("noise", cr.BGR24, W, H)
    tmpl = chip_template(16, 16)
    lm = np.stack([chip_face(tmpl, 16, 16, sc, ang, (W / 2 - 0.5 + 2 * k, H / 2 - k), 900 + k) for k, (sc, ang) in enumerate(CHIP_POSES)])
    fi = [k % 2 for k in range(len(lm))]
    rot = np.empty_like(lm)
    for f, p in enumerate(lm):
        plan = api.rotation_plan(W, H, degs[fi[f]])
        rot[f, 0::2], rot[f, 1::2] = ex.rotate_inverse(W, H, plan["tw"], plan["th"], degs[fi[f]], p[0::2], p[1::2])
    return img, tmpl, lm, fi, degs, rot


def check_chain(chips, back, img, tmpl, lm, what):
    """The chain's end: rotate_back's landmarks within WAY_BACK_TOL of the originals, and the chips cut with them within the
    chip bound of ex.chip under ex.chip_fit of the ORIGINAL landmarks, the bound widened by what landmarks off by WAY_BACK_TOL
    move a sample (fit_gain) times the surface's 255 per pixel and axis.  -> the largest landmark difference."""
    d = float(np.abs(np.asarray(back, np.float64) - lm).max())
    assert d <= WAY_BACK_TOL, (what, d)
    extra = 2 * 255 * fit_gain(tmpl, 16, 16) * WAY_BACK_TOL
    assert extra < 1e-6
    for f, p in enumerate(lm):
        M = exact_fit(p, tmpl)
        check_chip(chips[f], img, cr.BGR24, cr.RGB24, M, ex.chip_n(M), (what, f), extra)
    return d


def test_chain_back_from_a_rolled_frame_to_chips_on_the_host(built):
    """Landmarks in the source frame -> the rotated images (exactly) -> jdaRotateBack -> jdaFaceChips on the SOURCE."""
    from jda_amd import api
    img, tmpl, lm, fi, degs, rot = chain_case()
    _, back = api.rotate_back([img, img], cr.BGR24, degs, fi, landmarks=rot)
    assert np.abs(rot - lm).max() > 5                                    # (the rotated frame's coordinates are other coordinates)
    chips = api.face_chips([img, img], cr.BGR24, fi, back, tmpl, 16, 16, cr.RGB24)
    d = check_chain(chips, back, img, tmpl, lm, "host form")
    print("rotate_back after the exact inverse: largest landmark difference %.3e (tolerance %.3e)" % (d, WAY_BACK_TOL))


def test_chip_definition_on_pictures():
    """The definition's own sense: under the identity the chip is the crop, under a translation by half a pixel the mean of
    two neighbours, a pixel outside the image is 0 and one half a pixel outside half its neighbour, n = 2 at a 2x reduction
    averages the 2 x 2 block whose centre the pixel's centre maps to, and a colour image is warped channel by channel."""
    img = np.arange(35, dtype=np.float64).reshape(5, 7) * 3
    assert np.abs(ex.chip(img, [1, 0, 2, 0, 1, 1], 4, 3, 1) - img[1:4, 2:6]).max() < 1e-12
    assert np.abs(ex.chip(img, [1, 0, 2.5, 0, 1, 1], 4, 3, 1) - (img[1:4, 2:6] + img[1:4, 3:7]) / 2).max() < 1e-12
    edge = ex.chip(img, [1, 0, -1.5, 0, 1, 0], 3, 1, 1)[0]                   # sx = -1.5, -0.5, 0.5
    assert edge[0] == 0 and abs(edge[1] - img[0, 0] / 2) < 1e-12 and abs(edge[2] - (img[0, 0] + img[0, 1]) / 2) < 1e-12
    # chip pixel (u, v) -> (2u + 0.5, 2v + 0.5): samples at +-1/4 chip pixel = +-1/2 source pixel: the pixels 2u, 2u + 1
    block = (img[0:4:2, 0:6:2] + img[0:4:2, 1:7:2] + img[1:5:2, 0:6:2] + img[1:5:2, 1:7:2]) / 4
    assert np.abs(ex.chip(img, [2, 0, 0.5, 0, 2, 0.5], 3, 2, 2) - block).max() < 1e-12
    # a quarter turn, in the header's sense (a = 0, b = 1: u runs down the source, v to the left)
    assert np.abs(ex.chip(img, [0, -1, 6, 1, 0, 0], 5, 7, 1) - np.rot90(img, 1)).max() < 1e-12
    col = np.stack([img, 2 * img, 255 - img], 2)
    got = ex.chip(col, [0.8, -0.3, 1.2, 0.3, 0.8, 0.4], 4, 3, 2)
    for c in range(3):
        assert np.abs(got[..., c] - ex.chip(col[..., c], [0.8, -0.3, 1.2, 0.3, 0.8, 0.4], 4, 3, 2)).max() < 1e-12
    assert abs(ex.gray601([[255.0, 255.0, 255.0]])[0] - 255) < 1e-12 and abs(ex.gray601([[10.0, 0.0, 0.0]])[0] - 1.14) < 1e-12
