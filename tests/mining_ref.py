"""Plain-Python restatements the mining tests compare the product with (test infrastructure, not product):
NegGenerator::NextImage's enumeration and background transforms (reference src/jda/data.cpp:885-967), the initial-shape
draw of include/jda.h, Validate with that shift (oracle/cpp_reading2.validate plus RandomShape's global shift,
data.cpp:225-236) and the mining walk (ParallelMining, data.cpp:969-1016) on explicit patches."""
import numpy as np

from oracle import cpp_reading2 as r2
from train_ref import G, M64, splitmix64


def levels(W, H, origin_size, step, factor):
    """NextImage's levels of one transformed W x H image: [(win, nx, ny)]."""
    out = []
    if W <= origin_size or H <= origin_size:
        return out
    win = origin_size
    while True:
        out.append((win, (W - win) // step + 1, (H - win) // step + 1))
        win = int(win * factor)                     # s.win_size *= s.factor, an int
        if win >= W or win >= H:
            return out


def windows(W, H, origin_size, step, factor):
    """(x, y, win) in NextImage's order: level by level, row by row."""
    out = []
    for win, nx, ny in levels(W, H, origin_size, step, factor):
        for y in range(0, H - win + 1, step):
            for x in range(0, W - win + 1, step):
                out.append((x, y, win))
    return out


def transform(img, t):
    """data.cpp:930-963 as composed there: cv::flip(0) = up-down, flip(1) = left-right, flip(-1) = both, transpose."""
    ud, lr, T = np.flipud, np.fliplr, (lambda a: a.T)
    ops = {0: [], 1: [ud, T], 2: [ud, lr], 3: [lr, T], 4: [lr], 5: [ud, lr, T], 6: [ud, lr, lr], 7: [ud, T, lr]}[t]
    for f in ops:
        img = f(img)
    return np.ascontiguousarray(img)


def draw(seed, c, shift):
    """include/jda.h's counter-based draw c of the initial-shape shift (the generator: train_ref.splitmix64)."""
    u = float(splitmix64((seed + (c + 1) * G) & M64) >> 11) * 2.0 ** -53
    return -shift + (shift - -shift) * u


def shift_of(seed, key, shift):
    if shift == 0:
        return 0.0, 0.0
    return draw(seed, 2 * key, shift), draw(seed, 2 * key + 1, shift)


def validate(m, patches, dx=0.0, dy=0.0, similarity=False):
    """cpp_reading2.validate with RandomShape's global shift: the initial shape is mean_shape + (dx, dy).  patches: (o, h, q)
    numpy arrays.  -> (is_face, score, shape, n)."""
    pt = tuple((p, 0, 0, p.shape[1], p.shape[0]) for p in patches)
    return r2.validate(m, None, patches=pt, similarity=similarity, shift=(dx, dy))[:4]


def chain(resize, crop, mode, os_, hs, qs):
    """The three patches: crop -> o, then o (mode 0, mining) or the crop (mode 1, detectSingleScale) -> h, q."""
    o = resize(crop, os_, os_)
    src = o if mode == 0 else crop
    return o, resize(src, hs, hs), resize(src, qs, qs)


def mine(m, resize, images, steps, factors, transforms, size, start=0, os_=48, hs=36, qs=24, shift=0.0, seed=0,
         similarity=False):
    """ParallelMining over NextImage's walk, one thread, in order, from window ordinal `start`: the first `size` faces
    and the counters of [start, next_start)."""
    hits, scores, shapes, pats = [], [], [], []
    nega = carts = 0
    o = 0
    nxt = None
    for i, im in enumerate(images):
        ti = transform(im, transforms[i])
        H, W = ti.shape
        for (x, y, win) in windows(W, H, os_, steps[i], factors[i]):
            if o < start or nxt is not None:
                o += 1
                continue
            p = chain(resize, ti[y:y + win, x:x + win], 0, os_, hs, qs)
            dx, dy = shift_of(seed, o, shift)
            face, sc, sh, n = validate(m, p, dx, dy, similarity)
            if face:
                hits.append((i, x, y, win)); scores.append(sc); shapes.append(sh); pats.append(p)
                if len(hits) == size:
                    nxt = o + 1
            else:
                nega += 1
                carts += n
            o += 1
    if nxt is None:
        nxt = o
    return dict(hits=hits, score=scores, shape=shapes, patches=pats, nega_n=nega, carts_n=carts, next_start=nxt, total=o)
