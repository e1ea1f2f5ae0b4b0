"""Plain-Python restatement of the positive sample set that the positives tests compare the product with (test
infrastructure, not product; nothing under jda_amd/ imports it), written from the reference's source: getFace
(src/jda/data.cpp:542-565), the patches and their mirrors (data.cpp:630-640), the shapes and masks (589-598, 625-628,
641-661), CalcMeanShape (210-223), RandomShapes (237-253) on include/jda.h's generator and CalcShapeResidual (175-208).
The face is padded the way getFace pads -- the 3 cols x 3 rows canvas is BUILT and sliced -- which is deliberately another
route than the kernel's "0 outside the image".  The resize is the caller's (the oracle's resize_cv, as in mining_ref); the
shapes are sequential arithmetic on Python floats (IEEE doubles).  Dialect CPP is parity-unpinned."""
import numpy as np

import mining_ref
from train_ref import fdiv


class CanvasError(ValueError):
    """OpenCV would throw: the box leaves getFace's canvas (or is empty)."""


def get_face(img, box):
    """getFace (data.cpp:542-565), literally."""
    rows, cols = img.shape
    bx, by, bw, bh = box
    if bx >= 0 and by >= 0 and bx + bw < cols and by + bh < rows:
        if bw <= 0 or bh <= 0:
            raise CanvasError(box)
        return img[by:by + bh, bx:bx + bw].copy()
    rows_, cols_ = 3 * rows, 3 * cols
    img_ = np.zeros((rows_, cols_), np.uint8)
    x, y = cols // 2, rows // 2
    img_[y:y + rows, x:x + cols] = img
    x_, y_ = bx + x, by + y
    if bw <= 0 or bh <= 0 or x_ < 0 or y_ < 0 or x_ + bw > cols_ or y_ + bh > rows_:       # cv::Mat::operator()(Rect) asserts
        raise CanvasError(box)
    return img_[y_:y_ + bh, x_:x_ + bw].copy()


def patches_of(resize, face, sizes):
    """data.cpp:630-632: each patch is a resize of the face itself."""
    return [resize(face, s, s) for s in sizes]


def build(resize, images, faces, sizes, augment):
    """The set's records [size, o*o + h*h + q*q]: record i the face's three patches, record i + n their cv::flip(.., 1)."""
    n = len(faces)
    P = sum(s * s for s in sizes)
    out = np.zeros((2 * n if augment else n, P), np.uint8)
    for i, (im, x, y, w, h) in enumerate(faces):
        pt = patches_of(resize, get_face(images[im], (x, y, w, h)), sizes)
        out[i] = np.concatenate([p.ravel() for p in pt])
        if augment:
            out[i + n] = np.concatenate([np.ascontiguousarray(p[:, ::-1]).ravel() for p in pt])
    return out


def shapes(faces, landmarks, augment, left=(), right=(), reverse=False):
    """-> (gt_shapes [size][2L], shape_mask [size], mean_shape [2L]) as lists of Python floats / ints.  reverse: the mean's
    masked-in samples are added in descending order (the order control; not what the reference does)."""
    n = len(faces)
    L = len(landmarks[0]) // 2
    size = 2 * n if augment else n
    gt = [None] * size
    mask = [0] * size
    for i in range(n):
        _, x, y, w, h = (int(v) for v in faces[i])
        raw = [float(v) for v in landmarks[i]]
        no_shape = True
        for v in raw:
            if v >= 0:
                no_shape = False
        mask[i] = -1 if no_shape else 1
        g = list(raw)
        for j in range(L):
            g[2 * j] = (g[2 * j] - x) / w
            g[2 * j + 1] = (g[2 * j + 1] - y) / h
        gt[i] = g
        if augment:
            m = list(g)
            for j in range(L):
                m[2 * j] = 1 - m[2 * j]
            for j in range(len(left)):
                idx1, idx2 = left[j], right[j]
                x1, y1, x2, y2 = m[2 * idx2], m[2 * idx2 + 1], m[2 * idx1], m[2 * idx1 + 1]
                m[2 * idx1], m[2 * idx1 + 1] = x1, y1
                m[2 * idx2], m[2 * idx2 + 1] = x2, y2
            gt[i + n] = m
            mask[i + n] = mask[i]
    mean = list(gt[0])                                  # CalcMeanShape: sample 0 whatever its mask ...
    valid_n = 0
    order = range(size - 1, 0, -1) if reverse else range(1, size)
    for i in order:
        if mask[i] > 0:
            for j in range(2 * L):
                mean[j] += gt[i][j]
            valid_n += 1                                # ... and never counted
    r = fdiv(1., float(valid_n))                        # Mat /= double: times the reciprocal, plus a zero shift
    mean = [v * r + 0. for v in mean]
    return gt, mask, mean


def random_shapes(mean, n, shift, seed, first_key=0):
    out = []
    for i in range(n):
        x, y = mining_ref.shift_of(seed, first_key + i, shift)
        out.append([mean[j] + (y if j & 1 else x) for j in range(len(mean))])
    return out


def residual(gt, cur, idx, landmark_id=None):
    if landmark_id is None:
        return [[gt[i][j] - cur[i][j] for j in range(len(gt[i]))] for i in idx]
    return [[gt[i][2 * landmark_id] - cur[i][2 * landmark_id], gt[i][2 * landmark_id + 1] - cur[i][2 * landmark_id + 1]] for i in idx]


def has_gt(mask, idx):
    return [1 if mask[i] > 0 else 0 for i in idx]


# ---- test data shared by the host and the GPU tests ---------------------------------------------------------------------

def noise(seed, w, h):
    return np.random.default_rng(seed).integers(0, 256, (h, w), dtype=np.uint8)


def make_landmarks(seed, faces, L, unmasked=()):
    """Landmarks in image coordinates for the face rows: inside the box, with magnitudes spread over 2^-20 .. 1 of the
    box (so that the order of the mean's sum is visible in its bits); the samples in `unmasked` get all-negative values."""
    rng = np.random.default_rng(seed)
    n = len(faces)
    f = np.asarray(faces, np.float64).reshape(n, 5)
    rel = rng.uniform(0.05, 0.95, (n, 2 * L)) * np.exp2(rng.integers(-20, 1, (n, 1)).astype(np.float64))
    lm = rel.copy()
    lm[:, 0::2] = f[:, 1:2] + rel[:, 0::2] * f[:, 3:4]
    lm[:, 1::2] = f[:, 2:3] + rel[:, 1::2] * f[:, 4:5]
    lm = np.abs(lm)                                     # (a box left of the image: still "has a shape")
    for i in unmasked:
        lm[i] = -1.0 - rng.uniform(0, 5, 2 * L)
    return lm


def flip_search(resize, sizes=(48, 36, 24), seed=1):
    """The order control that was looked for: the first (w, h, side) over box sizes 25 .. 130, square boxes and then
    w x (w + 7), whose noise face has mirror(resize(face)) != resize(mirror(face)); None if there is none."""
    for dh in (0, 7):
        for w in range(25, 131):
            face = noise(seed + w, w, w + dh)
            for s in sizes:
                a = resize(face, s, s)[:, ::-1]
                b = resize(np.ascontiguousarray(face[:, ::-1]), s, s)
                if not np.array_equal(a, b):
                    return (w, w + dh, s)
    return None
