"""The definition of "frames larger than the faces need" (include/jda.h) restated in numpy on top of pack_ref.pack (the gray
image of a rectangle, rounded per pixel) and mining_ref.transform (the eight orientations): the w % f rightmost columns and
h % f bottom rows dropped, the rest reshaped to (rh, f, rw, f), summed, (S + f*f//2) // (f*f), turned.  And the way back
restated from the header on top of turn_ref: boxes in integers, landmarks in the type's own precision."""
import numpy as np

import pack_ref as pr
import turn_ref as tr
from mining_ref import transform

FACTORS = tuple(range(1, 9))


def block_means(gray, f):
    """uint8 [h, w] -> uint8 [h // f, w // f]."""
    rh, rw = gray.shape[0] // f, gray.shape[1] // f
    S = gray[:rh * f, :rw * f].astype(np.int64).reshape(rh, f, rw, f).sum(axis=(1, 3))
    return ((S + f * f // 2) // (f * f)).astype(np.uint8)


def reduce(img, fmt, f, t=0, rect=None):
    """uint8 [H, W(, C)] -> the rectangle's gray image reduced by f and turned by t, uint8 [H', W']."""
    return np.ascontiguousarray(transform(block_means(pr.pack(img, fmt, rect), f), t))


def size(w, h, f, t=0):
    return tr.size(w // f, h // f, t)


def back_box(box, f, t, rect):
    """(x, y, size) or (x, y, w, h) in the turned, reduced rectangle -> the same in the whole source image."""
    rx, ry, w, h = rect
    b = tr.back_box(box, t, (0, 0, w // f, h // f))
    return (b[0] * f + rx, b[1] * f + ry) + tuple(v * f for v in b[2:])


def back_landmarks(lm, f, t, rect, left=(), right=()):
    """[2L] of one face, float32 or float64 -> a new array of the same type."""
    real = lm.dtype.type
    rx, ry, w, h = rect
    out = tr.back_landmarks(lm, t, (0, 0, w // f, h // f), left, right)
    # (turn_ref adds real(0) where this definition adds nothing: x + 0 is x but for -0, and -0 * f + c is c either way)
    c = real(real(f - 1) / real(2))
    for i in range(len(out)):
        v = real(out[i] * real(f))
        v = real(v + c)
        out[i] = real(v + real(rx if i % 2 == 0 else ry))
    return out


def block_sum_image(f):
    """One gray image whose f x f blocks take every sum 0 .. 255 f^2 (block k: sum k, spread as evenly as integers allow, the
    larger pixels dealt round the block from position k on), padded with random blocks to a rectangle of blocks."""
    sums = np.arange(255 * f * f + 1, dtype=np.int64)
    side = int(np.ceil(np.sqrt(len(sums))))
    rng = np.random.default_rng(f)
    allsums = np.concatenate([sums, rng.integers(0, 255 * f * f + 1, side * side - len(sums))])
    base, extra = allsums // (f * f), allsums % (f * f)
    pos = (np.arange(f * f)[None, :] - np.arange(len(allsums))[:, None]) % (f * f)          # where position p of block k stands in the deal
    blocks = (base[:, None] + (pos < extra[:, None])).astype(np.uint8)                       # [k, f*f], row sums == allsums
    assert np.array_equal(blocks.astype(np.int64).sum(1), allsums)
    img = blocks.reshape(side, side, f, f).transpose(0, 2, 1, 3).reshape(side * f, side * f)
    return np.ascontiguousarray(img), allsums.reshape(side, side)
