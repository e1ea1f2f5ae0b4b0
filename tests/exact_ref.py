"""TEST INFRASTRUCTURE, not product: what dialect CPP's restated numerics, the rotated pack and the face chips MEAN, in plain
numpy on float64, written from the mathematical definition and from nobody's code -- not OpenCV's, not the reference's, not
this repository's oracle or *_ref.py files, none of which is imported here (nothing under jda_amd/ imports this either).
Nothing is rounded, snapped or ordered to match an implementation: the tests that use these (tests/test_exact_host.py,
tests/test_exact_gpu.py) assert a DERIVED distance between an implementation's integers and these real numbers, or 16 x a
recorded difference between two floating-point routes to one number.

  bilinear_resize   cv::resize(INTER_LINEAR) as an interpolation: half-pixel centres, replicated borders
  box2              the rounded mean of 2 x 2 blocks: the documented routing of an exact 2x down-scale
  similarity        STParameter::Calc as a least-squares fit: scale from the Frobenius norms, the proper rotation by Kabsch
  rotate            "frames whose faces are rolled" (include/jda.h) as a real-valued map and real-valued bilinear taps
  rotate_inverse    the inverse of that map: where a point of the rectangle lies in the rotated image
  chip_fit          "faces as they leave": the chip -> source similarity as the least-squares solution of its linear system
  chip              the chip as the mean of n x n real-valued bilinear samples of the zero-extended image
  gray601           0.114 B + 0.587 G + 0.299 R, which the Q14 weights of "frames as they arrive" are a rounding of
"""
import math

import numpy as np


def _axis(n_dst, n_src):
    """Destination index d samples the source axis at (d + 0.5) * n_src / n_dst - 0.5 -> (tap, tap + 1, weight of tap + 1),
    the two taps clamped to the image."""
    c = (np.arange(n_dst, dtype=np.float64) + 0.5) * np.float64(n_src) / np.float64(n_dst) - 0.5
    i0 = np.floor(c)
    f = c - i0
    lo = np.clip(i0, 0, n_src - 1).astype(np.int64)
    hi = np.clip(i0 + 1, 0, n_src - 1).astype(np.int64)
    return lo, hi, f


def bilinear_resize(img, dw, dh):
    """[sh, sw] -> float64 [dh, dw]: bilinear interpolation of the image, not rounded."""
    src = np.asarray(img, np.float64)
    sh, sw = src.shape
    x0, x1, fx = _axis(dw, sw)
    y0, y1, fy = _axis(dh, sh)
    top = src[y0][:, x0] * (1 - fx) + src[y0][:, x1] * fx
    bot = src[y1][:, x0] * (1 - fx) + src[y1][:, x1] * fx
    return top * (1 - fy)[:, None] + bot * fy[:, None]


def box2(img):
    """[2h, 2w] -> int64 [h, w]: the mean of every 2 x 2 block, rounded to nearest (a mean of four integers never lies
    halfway between two: .5 rounds up and is the only tie)."""
    src = np.asarray(img, np.float64)
    h, w = src.shape[0] // 2, src.shape[1] // 2
    src = src[:2 * h, :2 * w]
    mean = (src[0::2, 0::2] + src[0::2, 1::2] + src[1::2, 0::2] + src[1::2, 1::2]) / 4
    return np.floor(mean + 0.5).astype(np.int64)


def similarity(shape1, shape2, L):
    """The similarity that takes centred shape2 onto centred shape1 -> (scale, r00, r01, r10, r11), float64.
    scale = ||a|| / ||b|| (Frobenius); R = the proper rotation minimising ||a - R b||, by Kabsch: the SVD of the 2 x 2
    cross-covariance with the determinant forced to +1.  Shapes are (x0, y0, x1, y1, ...)."""
    a = np.asarray(shape1, np.float64).reshape(L, 2)
    b = np.asarray(shape2, np.float64).reshape(L, 2)
    a = a - a.mean(axis=0)
    b = b - b.mean(axis=0)
    scale = np.linalg.norm(a) / np.linalg.norm(b)
    u, _, vt = np.linalg.svd(b.T @ a)               # H = sum_i b_i a_i^T = U S V^T;  R = V diag(1, d) U^T
    d = 1.0 if np.linalg.det(vt.T @ u.T) >= 0 else -1.0
    r = vt.T @ np.diag([1.0, d]) @ u.T
    return (float(scale), float(r[0, 0]), float(r[0, 1]), float(r[1, 0]), float(r[1, 1]))


def similarity_residual(shape1, shape2, L, stp):
    """||a - scale * R b|| (Frobenius) for centred a = shape1, b = shape2 under any (scale, r00, r01, r10, r11)."""
    a = np.asarray(shape1, np.float64).reshape(L, 2)
    b = np.asarray(shape2, np.float64).reshape(L, 2)
    a = a - a.mean(axis=0)
    b = b - b.mean(axis=0)
    r = np.array([[stp[1], stp[2]], [stp[3], stp[4]]], np.float64)
    return float(np.linalg.norm(a - stp[0] * (b @ r.T)))


def rotate_coords(w, h, tw, th, deg):
    """The header's map with the angle from math.cos / math.sin: output pixel (column u, row v) of the tw x th image samples
    the w x h rectangle at (sx, sy); both about the images' centres -> float64 [th, tw] sx, sy."""
    c, s = math.cos(deg * (math.pi / 180)), math.sin(deg * (math.pi / 180))
    v, u = np.meshgrid(np.arange(th, dtype=np.float64), np.arange(tw, dtype=np.float64), indexing="ij")
    du, dv = u - (tw - 1) / 2, v - (th - 1) / 2
    return c * du + s * dv + (w - 1) / 2, c * dv - s * du + (h - 1) / 2


def rotate(gray, deg):
    """[h, w] -> float64 [th, tw]: the rectangle rotated by deg degrees (positive: clockwise as displayed), every output
    pixel the real-valued bilinear mix of its four neighbours, each 0 outside the rectangle; nothing is snapped to 1/1024
    and no weight is an integer.  (tw, th) is the header's own definition (jdaRotationPlan) and not under test."""
    from jda_amd import api
    g = np.asarray(gray, np.float64)
    h, w = g.shape
    plan = api.rotation_plan(w, h, deg)
    sx, sy = rotate_coords(w, h, plan["tw"], plan["th"], deg)
    x0, y0 = np.floor(sx), np.floor(sy)
    fx, fy = sx - x0, sy - y0
    pad = np.zeros((h + 2, w + 2), np.float64)      # rows / columns -1 .. h, w: zero outside the rectangle
    pad[1:h + 1, 1:w + 1] = g

    def tap(x, y):
        inside = (x >= -1) & (x <= w) & (y >= -1) & (y <= h)
        xi = np.clip(x, -1, w).astype(np.int64) + 1
        yi = np.clip(y, -1, h).astype(np.int64) + 1
        return np.where(inside, pad[yi, xi], 0.0)
    return (tap(x0, y0) * (1 - fx) + tap(x0 + 1, y0) * fx) * (1 - fy) + (tap(x0, y0 + 1) * (1 - fx) + tap(x0 + 1, y0 + 1) * fx) * fy


def rotate_inverse(w, h, tw, th, deg, sx, sy):
    """The inverse of rotate_coords (the matrix [[c, s], [-s, c]] is a rotation: its inverse is its transpose): the point
    (sx, sy) of the w x h rectangle lies at (u, v) of the tw x th rotated image -> float64 u, v."""
    c, s = math.cos(deg * (math.pi / 180)), math.sin(deg * (math.pi / 180))
    dx, dy = np.asarray(sx, np.float64) - (w - 1) / 2, np.asarray(sy, np.float64) - (h - 1) / 2
    return c * dx - s * dy + (tw - 1) / 2, s * dx + c * dy + (th - 1) / 2


def chip_fit(landmarks, template, use=None):
    """The similarity that takes the template's points q_i (chip pixels) onto the landmarks p_i in the least-squares sense
    -> the chip -> source map [a, -b, tx, b, a, ty], float64.  p_i = (a qx_i - b qy_i + tx, b qx_i + a qy_i + ty) is linear in
    (a, b, tx, ty): two rows per used landmark, solved by np.linalg.lstsq (an SVD), nothing centred and no closed form.  The
    origin of a rectangle is the caller's to add to tx, ty."""
    p = np.asarray(landmarks, np.float64).reshape(-1, 2)
    q = np.asarray(template, np.float64).reshape(-1, 2)
    keep = np.ones(len(q), bool) if use is None else np.asarray(use).reshape(-1) != 0
    p, q = p[keep], q[keep]
    m = len(q)
    A = np.zeros((2 * m, 4), np.float64)
    A[0::2] = np.stack([q[:, 0], -q[:, 1], np.ones(m), np.zeros(m)], 1)
    A[1::2] = np.stack([q[:, 1], q[:, 0], np.zeros(m), np.ones(m)], 1)
    (a, b, tx, ty), _, rank, _ = np.linalg.lstsq(A, p.reshape(-1), rcond=None)
    assert rank == 4
    return np.array([a, -b, tx, b, a, ty], np.float64)


def chip_residual(landmarks, template, M, use=None):
    """sum_i ||p_i - M q_i||^2 over the used landmarks, for any chip -> source map M."""
    p = np.asarray(landmarks, np.float64).reshape(-1, 2)
    q = np.asarray(template, np.float64).reshape(-1, 2)
    keep = np.ones(len(q), bool) if use is None else np.asarray(use).reshape(-1) != 0
    M = np.asarray(M, np.float64)
    r = p[keep] - np.stack([M[0] * q[keep, 0] + M[1] * q[keep, 1] + M[2], M[3] * q[keep, 0] + M[4] * q[keep, 1] + M[5]], 1)
    return float((r * r).sum())


def chip_n(M):
    """Samples per axis: min(4, max(1, ceil(hypot(a, b)))), the reduction rounded up and stopped at 4."""
    return min(4, max(1, math.ceil(math.hypot(M[0], M[3]))))


def chip_coords(M, cw, ch, n):
    """Where the n x n samples of every chip pixel lie in the source -> float64 sx, sy [n, n, ch, cw] (j, i, v, u): chip
    coordinates (u + ((2i + 1) - n) / 2n, v + ((2j + 1) - n) / 2n), the centres of the n x n equal cells of the pixel's unit
    square around (u, v), sent through M."""
    o = (2.0 * np.arange(n) + 1 - n) / (2.0 * n)
    cu = np.arange(cw, dtype=np.float64)[None, None, None, :] + o[None, :, None, None]
    cv = np.arange(ch, dtype=np.float64)[None, None, :, None] + o[:, None, None, None]
    cu, cv = np.broadcast_arrays(cu, cv)
    return M[0] * cu + M[1] * cv + M[2], M[3] * cu + M[4] * cv + M[5]


def bilinear_zero(image, sx, sy):
    """The bilinear surface of the image extended by zeros, at real coordinates of any shape -> float64 sx.shape (+ (C,)).
    0 at and beyond sx <= -1, sx >= W, sy <= -1, sy >= H by itself: every tap there is one of the zeros."""
    g = np.asarray(image, np.float64)
    H, W = g.shape[:2]
    pad = np.zeros((H + 2, W + 2) + g.shape[2:], np.float64)      # rows / columns -1 .. H, W
    pad[1:H + 1, 1:W + 1] = g
    x0, y0 = np.floor(sx), np.floor(sy)
    fx, fy = sx - x0, sy - y0

    def tap(x, y):
        inside = (x >= -1) & (x <= W) & (y >= -1) & (y <= H)
        t = pad[np.clip(y, -1, H).astype(np.int64) + 1, np.clip(x, -1, W).astype(np.int64) + 1]
        return np.where(inside.reshape(inside.shape + (1,) * (t.ndim - inside.ndim)), t, 0.0)
    if g.ndim == 3:
        fx, fy = fx[..., None], fy[..., None]
    return (tap(x0, y0) * (1 - fx) + tap(x0 + 1, y0) * fx) * (1 - fy) + (tap(x0, y0 + 1) * (1 - fx) + tap(x0 + 1, y0 + 1) * fx) * fy


def chip(image, M, cw, ch, n):
    """float64 [H, W] or [H, W, 3] -> float64 [ch, cw(, 3)]: every chip pixel the mean of its n x n real-valued bilinear samples
    of the zero-extended image, each channel alone.  Nothing is snapped, no weight is an integer, no sample is refused."""
    sx, sy = chip_coords(np.asarray(M, np.float64), cw, ch, n)
    return bilinear_zero(image, sx, sy).mean(axis=(0, 1))


def gray601(bgr):
    """[..., 3] in the order B, G, R -> 0.114 B + 0.587 G + 0.299 R, real-valued."""
    c = np.asarray(bgr, np.float64)
    return 0.114 * c[..., 0] + 0.587 * c[..., 1] + 0.299 * c[..., 2]
