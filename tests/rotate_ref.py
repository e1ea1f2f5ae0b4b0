"""The definition of "frames whose faces are rolled" (include/jda.h) restated in numpy on top of pack_ref.pack (the gray image
of a rectangle, rounded per pixel): c, s, tw, th come from the plan (jdaRotationPlan -- the one place that asks libm), the map
is float64 with one operation per step (numpy never fuses), and from X, Y on everything is int64.  And the way back restated
from the header: all in float64, rounded once to the landmark's type."""
import numpy as np

import pack_ref as pr

ANGLES = (0, 90, 180, 270, 0.5, -0.5, 15, 30, 45, -33.3, 60, 89.5, 135, 359)


def plan_size(w, h, c, s):
    """(tw, th) by the header's formula, from the plan's c and s."""
    ew = (np.float64(w) * abs(np.float64(c)) + np.float64(h) * abs(np.float64(s))) - np.float64(1) / 1024
    eh = (np.float64(w) * abs(np.float64(s)) + np.float64(h) * abs(np.float64(c))) - np.float64(1) / 1024
    return max(1, int(np.ceil(ew))), max(1, int(np.ceil(eh)))


def source_xy(u, v, plan):
    """Turned (u, v), float64 arrays -> the rectangle's (sx, sy)."""
    c, s = np.float64(plan["c"]), np.float64(plan["s"])
    cu, cv = np.float64(plan["tw"] - 1) / 2, np.float64(plan["th"] - 1) / 2
    cx, cy = np.float64(plan["w"] - 1) / 2, np.float64(plan["h"] - 1) / 2
    du, dv = u - cu, v - cv
    return (c * du + s * dv) + cx, (c * dv - s * du) + cy


def rotate_gray(g, plan):
    """uint8 [h, w] (the rectangle's gray image) -> uint8 [th, tw]."""
    h, w = g.shape
    assert (w, h) == (plan["w"], plan["h"])
    v, u = np.meshgrid(np.arange(plan["th"], dtype=np.float64), np.arange(plan["tw"], dtype=np.float64), indexing="ij")
    sx, sy = source_xy(u, v, plan)
    inside = (sx > -1) & (sx < w) & (sy > -1) & (sy < h)
    X = np.floor(np.where(inside, sx, 0.0) * 1024 + 0.5).astype(np.int64)
    Y = np.floor(np.where(inside, sy, 0.0) * 1024 + 0.5).astype(np.int64)
    x0, fx, y0, fy = X >> 10, X & 1023, Y >> 10, Y & 1023
    pad = np.zeros((h + 3, w + 3), np.int64)                     # rows / columns -1 .. h + 1, w + 1: black outside the rectangle
    pad[1:h + 1, 1:w + 1] = g

    def tap(x, y):
        return pad[y + 1, x + 1]
    total = tap(x0, y0) * ((1024 - fx) * (1024 - fy)) + tap(x0 + 1, y0) * (fx * (1024 - fy)) + tap(x0, y0 + 1) * ((1024 - fx) * fy) + \
        tap(x0 + 1, y0 + 1) * (fx * fy)
    assert total.max(initial=0) < 1 << 32
    return np.where(inside, (total + (1 << 19)) >> 20, 0).astype(np.uint8)


def rotate(img, fmt, plan, rect=None):
    """uint8 [H, W(, C)] -> the rectangle's gray image rotated by the plan, uint8 [th, tw]."""
    return rotate_gray(pr.pack(img, fmt, rect), plan)


def back_landmarks(lm, plan, rect):
    """[2L] of one face in the turned rectangle, float32 or float64 -> a new array of the same type, in the whole image."""
    x, y = source_xy(lm[0::2].astype(np.float64), lm[1::2].astype(np.float64), plan)
    out = np.empty_like(lm)
    out[0::2] = (x + np.float64(rect[0])).astype(lm.dtype)
    out[1::2] = (y + np.float64(rect[1])).astype(lm.dtype)
    return out


def back_box(box, plan, rect):
    """(x, y, size) or (x, y, w, h) in the turned rectangle -> the same in the whole source image."""
    bw, bh = box[2], box[3] if len(box) == 4 else box[2]
    hw, hh = np.float64(bw - 1) / 2, np.float64(bh - 1) / 2
    mx, my = source_xy(np.float64(box[0]) + hw, np.float64(box[1]) + hh, plan)
    return (int(np.floor((mx - hw) + 0.5)) + rect[0], int(np.floor((my - hh) + 0.5)) + rect[1]) + tuple(box[2:])
