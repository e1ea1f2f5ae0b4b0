"""TEST INFRASTRUCTURE, not product: what three of dialect CPP's restated numerics MEAN, in plain numpy on float64, written
from the mathematical definition and from nobody's code -- not OpenCV's, not the reference's, not this repository's oracle
or *_ref.py files, none of which is imported here (nothing under jda_amd/ imports this either).  Nothing is rounded, snapped
or ordered to match an implementation: the tests that use these (tests/test_exact_host.py, tests/test_exact_gpu.py) assert a
DERIVED distance between an implementation's integers and these real numbers.

  bilinear_resize   cv::resize(INTER_LINEAR) as an interpolation: half-pixel centres, replicated borders
  box2              the rounded mean of 2 x 2 blocks: the documented routing of an exact 2x down-scale
  similarity        STParameter::Calc as a least-squares fit: scale from the Frobenius norms, the proper rotation by Kabsch
  rotate            "frames whose faces are rolled" (include/jda.h) as a real-valued map and real-valued bilinear taps
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
