"""Plain-Python restatements the mining tests compare the product with (test infrastructure, not product):
NegGenerator::NextImage's enumeration and background transforms (reference src/jda/data.cpp:885-967), the initial-shape
draw of include/jda.h, Validate with that shift (oracle/cpp_reading2.validate plus RandomShape's global shift,
data.cpp:225-236) and the mining walk (ParallelMining, data.cpp:969-1016) on explicit patches."""
import numpy as np

from oracle import cpp_reading2 as r2

M64 = (1 << 64) - 1


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
    """include/jda.h's counter-based draw c of the initial-shape shift."""
    z = (seed + (c + 1) * 0x9E3779B97F4A7C15) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    z ^= z >> 31
    u = float(z >> 11) * 2.0 ** -53
    return -shift + (shift - -shift) * u


def shift_of(seed, key, shift):
    if shift == 0:
        return 0.0, 0.0
    return draw(seed, 2 * key, shift), draw(seed, 2 * key + 1, shift)


def validate(m, patches, dx=0.0, dy=0.0, similarity=False):
    """cpp_reading2.validate with RandomShape's global shift: the initial shape is mean_shape + (dx, dy); Calc keeps the
    stored mean_shape.  patches: (o, h, q) numpy arrays.  -> (is_face, score, shape, n)."""
    pt = tuple((p, 0, 0, p.shape[1], p.shape[0]) for p in patches)
    shape = [v + (dy if j & 1 else dx) for j, v in enumerate(m.mean_shape)]
    score, n = 0.0, 0
    base = 1 << (m.D - 1)
    stp = r2.IDENTITY
    for t in range(m.stage_idx if m.stage_idx < m.T else m.T):
        stp = r2.st_calc(shape, m.mean_shape, m.L) if similarity else r2.IDENTITY
        lbf = [0] * m.K
        for k in range(m.K):
            c = m.carts[t][k]
            idx = r2.forward(m, c, pt, shape, stp)
            score += c.scores[idx]
            score = (score - c.mean) / c.std
            n += 1
            if score < c.th:
                return False, score, shape, n
            lbf[k] = k * base + idx
        delta = [0.0] * (2 * m.L)
        for k in range(m.K):
            row = m.w[t][lbf[k]]
            for j in range(2 * m.L):
                delta[j] += row[j]
        if similarity:
            for i in range(m.L):
                delta[2 * i], delta[2 * i + 1] = r2.st_apply(stp, delta[2 * i], delta[2 * i + 1])
        for j in range(2 * m.L):
            shape[j] = shape[j] + delta[j]
    if m.stage_idx < m.T:
        for k in range(m.cart_idx + 1):
            c = m.carts[m.stage_idx][k]
            idx = r2.forward(m, c, pt, shape, stp)
            score += c.scores[idx]
            score = (score - c.mean) / c.std
            n += 1
            if score < c.th:
                return False, score, shape, n
    return True, score, shape, n


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
