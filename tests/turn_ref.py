"""The definition of "frames in any orientation" (include/jda.h) restated in numpy on top of pack_ref.pack (the gray image of
a rectangle) and mining_ref.transform (the eight orientations as the reference composes them from flips and a transpose), and
the way back restated from the header: boxes in integers, landmarks in the type's own precision."""
import numpy as np

import pack_ref as pr
from mining_ref import transform

ORIENTS = tuple(range(8))
SWAP = {1, 3, 5, 7}
FLIP_X = {2, 3, 4, 5}
FLIP_Y = {1, 2, 5, 6}
MIRROR = {4, 5, 6, 7}
EXIF = {1: 0, 2: 4, 3: 2, 4: 6, 5: 7, 6: 1, 7: 5, 8: 3}


def turn(img, fmt, t, rect=None):
    """uint8 [H, W(, C)] -> the rectangle's gray image turned by t, uint8 [H', W']."""
    return transform(pr.pack(img, fmt, rect), t)


def size(w, h, t):
    return (h, w) if t in SWAP else (w, h)


def rect_of(img, rect):
    if rect is None or (rect[2] == 0 and rect[3] == 0):
        return 0, 0, img.shape[1], img.shape[0]
    return tuple(rect)


def back_box(box, t, rect):
    """(x, y, size) or (x, y, w, h) in the turned rectangle -> the same in the whole source image."""
    rx, ry, w, h = rect
    x, y, bw = box[0], box[1], box[2]
    bh = box[3] if len(box) == 4 else bw
    if t in SWAP:
        x, y, bw, bh = y, x, bh, bw
    if t in FLIP_X:
        x = w - bw - x
    if t in FLIP_Y:
        y = h - bh - y
    return (x + rx, y + ry, bw) + ((bh,) if len(box) == 4 else ())


def back_landmarks(lm, t, rect, left=(), right=()):
    """[2L] of one face, float32 or float64 -> a new array of the same type."""
    real = lm.dtype.type
    rx, ry, w, h = rect
    out = lm.copy()
    for i in range(len(lm) // 2):
        x, y = lm[2 * i], lm[2 * i + 1]
        if t in SWAP:
            x, y = y, x
        if t in FLIP_X:
            x = real(real(w - 1) - x)
        if t in FLIP_Y:
            y = real(real(h - 1) - y)
        out[2 * i], out[2 * i + 1] = real(x + real(rx)), real(y + real(ry))
    if t in MIRROR:
        for a, b in zip(left, right):
            for c in (0, 1):
                out[2 * a + c], out[2 * b + c] = out[2 * b + c], out[2 * a + c]
    return out
