"""The kernels that carry dialect CPP's restated numerics, run against tests/exact_ref.py DIRECTLY -- not through the oracle
or a *_ref.py restatement by this repository's author: cv_resize_px (k_resize_cv, the mining patches, the positive patches)
against real-valued bilinear interpolation and the rounded 2 x 2 mean, stp_side / stp_rot (k_stp) against the Kabsch fit,
k_rotate against the real-valued rotation.  The cases, the derived bounds and the one measured tolerance are those of
tests/test_exact_host.py, where they are explained; every case here takes well under a second.  What this does not establish:
bit-level parity with OpenCV, anything integer-valued (tree walks, NMS, the enumeration of windows), k_chips."""
import math

import numpy as np
import pytest

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
