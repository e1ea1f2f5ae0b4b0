"""The definition of "faces as they leave" (include/jda.h) restated from the header: the fit in Python floats (IEEE doubles,
one rounding per operation, the header's order), the coordinates likewise, everything behind a coordinate's rounding to
1/1024 pixel in Python integers / numpy int64.  Also the helpers both test files build their cases with."""
import math

import numpy as np

import pack_ref as pr

GRAY8, BGR24, RGB24, BGRA32, RGBA32 = range(5)
CHIP_FORMATS = (GRAY8, BGR24, RGB24)


def fit(p, q, use=None, rect_xy=(0, 0)):
    """p: the face's landmarks [2L] (floats already widened to double), q: the template [2L] -> M, six Python floats."""
    L = len(q) // 2
    idx = [i for i in range(L) if use is None or use[i]]
    m = len(idx)
    assert m >= 2
    sqx = sqy = spx = spy = 0.0
    for i in idx:
        sqx = sqx + float(q[2 * i]); sqy = sqy + float(q[2 * i + 1])
        spx = spx + float(p[2 * i]); spy = spy + float(p[2 * i + 1])
    mqx, mqy, mpx, mpy = sqx / float(m), sqy / float(m), spx / float(m), spy / float(m)
    den = sa = sb = 0.0
    for i in idx:
        cqx, cqy = float(q[2 * i]) - mqx, float(q[2 * i + 1]) - mqy
        cpx, cpy = float(p[2 * i]) - mpx, float(p[2 * i + 1]) - mpy
        den = den + (cqx * cqx + cqy * cqy)
        sa = sa + (cqx * cpx + cqy * cpy)
        sb = sb + (cqx * cpy - cqy * cpx)
    assert den != 0.0
    a, b = sa / den, sb / den
    tx = (mpx - (a * mqx - b * mqy)) + float(rect_xy[0])
    ty = (mpy - (b * mqx + a * mqy)) + float(rect_xy[1])
    return [a, -b, tx, b, a, ty]


def auto_n(M):
    s2 = M[0] * M[0] + M[3] * M[3]
    return 1 if s2 <= 1.0 else 2 if s2 <= 4.0 else 3 if s2 <= 9.0 else 4


def channels(img, src_fmt, chip_fmt):
    """The source as int64 [H, W, C] in the chip's channels: what a tap reads (colour -> gray goes through the Q14 formula
    per tap, gray -> colour replicates, colour -> colour reorders; alpha is dropped)."""
    img = np.asarray(img)
    if chip_fmt == GRAY8:
        return pr.gray(img, src_fmt).astype(np.int64)[..., None]
    if src_fmt == GRAY8:
        return np.repeat(img.reshape(img.shape[0], img.shape[1], 1).astype(np.int64), 3, 2)
    c = img[..., :3].astype(np.int64)
    src_rgb, chip_rgb = src_fmt in (RGB24, RGBA32), chip_fmt == RGB24
    return c[..., ::-1] if src_rgb != chip_rgb else c


def chip(img, src_fmt, M, cw, ch, chip_fmt, n):
    """One chip, uint8 [ch, cw] or [ch, cw, 3]; img is the WHOLE source image."""
    src = channels(img, src_fmt, chip_fmt)
    H, W, C = src.shape
    out = np.zeros((ch, cw, C), np.uint8)
    for v in range(ch):
        for u in range(cw):
            acc = [0] * C
            for j in range(n):
                cv = float(v) + float((2 * j + 1) - n) / float(2 * n)
                for i in range(n):
                    cu = float(u) + float((2 * i + 1) - n) / float(2 * n)
                    sx = (M[0] * cu + M[1] * cv) + M[2]
                    sy = (M[3] * cu + M[4] * cv) + M[5]
                    if not (sx > -1.0 and sx < W and sy > -1.0 and sy < H):
                        continue
                    X, Y = int(math.floor(sx * 1024.0 + 0.5)), int(math.floor(sy * 1024.0 + 0.5))
                    x0, fx, y0, fy = X >> 10, X & 1023, Y >> 10, Y & 1023
                    for (x, y, wgt) in ((x0, y0, (1024 - fx) * (1024 - fy)), (x0 + 1, y0, fx * (1024 - fy)),
                                        (x0, y0 + 1, (1024 - fx) * fy), (x0 + 1, y0 + 1, fx * fy)):
                        if 0 <= x < W and 0 <= y < H:
                            for c in range(C):
                                acc[c] += int(src[y, x, c]) * wgt
            for c in range(C):
                assert acc[c] < 1 << 32
                out[v, u, c] = ((acc[c] + n * n * (1 << 19)) >> 20) // (n * n)
    return out[..., 0] if chip_fmt == GRAY8 else out


def chips(images, fmts, rects, face_image, landmarks, tmpl, cw, ch, chip_fmt, use=None, supersample=0):
    """-> (chips uint8 [n, ch, cw(, 3)], matrices float64 [n, 6]).  landmarks: [n, 2L] float32 or float64."""
    out, mats = [], []
    for f, im in enumerate(face_image):
        r = rects[im] if rects is not None and rects[im] is not None else (0, 0, 0, 0)
        M = fit([float(x) for x in np.asarray(landmarks)[f]], tmpl, use, (r[0], r[1]))
        n = supersample if supersample else auto_n(M)
        out.append(chip(images[im], fmts[im], M, cw, ch, chip_fmt, n))
        mats.append(M)
    shape = (0, ch, cw) if chip_fmt == GRAY8 else (0, ch, cw, 3)
    return (np.stack(out) if out else np.zeros(shape, np.uint8)), np.array(mats, np.float64).reshape(-1, 6)


# ---- helpers of the test files ---------------------------------------------------------------------------------------------

def template(L, cw, ch, rng):
    """L distinct template points inside the chip (chip pixels, not integers)."""
    t = np.empty(2 * L)
    t[0::2] = rng.uniform(0.15, 0.85, L) * cw
    t[1::2] = rng.uniform(0.15, 0.85, L) * ch
    return t


def place(tmpl, scale, angle_deg, centre, rng=None, noise=0.0):
    """Landmarks for a face whose chip -> source map has the given scale (source pixels per chip pixel) and rotation and puts
    the template's mean at `centre`; noise makes the fit a genuine least-squares one."""
    q = np.asarray(tmpl, np.float64).reshape(-1, 2)
    a, b = scale * math.cos(math.radians(angle_deg)), scale * math.sin(math.radians(angle_deg))
    c = q - q.mean(0)
    p = np.stack([a * c[:, 0] - b * c[:, 1], b * c[:, 0] + a * c[:, 1]], 1) + np.asarray(centre, np.float64)
    if rng is not None and noise:
        p += rng.uniform(-noise, noise, p.shape)
    return p.reshape(-1)
