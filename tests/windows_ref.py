"""A plain numpy-fp32 restatement of the reference's window loop for ONE caller-given window, written from the reference's
source (c/jda.c), not from the kernel:
  grid()      the enumeration of c/jda.c:320-339 (+459-460): `win_size *= scale` is an int times a float, truncated
  pyramid()   jdaImageResize, c/jda.c:203-230, for the half / quarter pair of c/jda.c:450-457
  walk()      the loop body c/jda.c:340-414: views, cart walks, the score chain, the stage regression -- with the multi-scale
              read clamped into the half / quarter image (the project's documented divergence from the reference's
              out-of-bounds read) -- plus the trace outputs jdaTraceBatch defines (carts_n, path_hash)
  validate()  walk() over a window list, with is_face (c/jda.c:414) and the relocated landmarks (c/jda.c:471-472)
Every real is an np.float32 and every operation one fp32 operation, in the reference's order.  tests/test_windows_host.py pins
this file to the oracle (itself pinned to the compiled reference); tests/test_windows.py compares the GPU entry against it for
windows no grid contains."""
import numpy as np

f32 = np.float32
FNV_SEED, FNV_PRIME = 2166136261, 16777619
INT_MIN = -2 ** 31


def _int(v):
    """(int)v of an fp32 value as the reference build does it (cvttss2si: truncation; INT_MIN for NaN and out of range)."""
    v = float(v)
    if v != v or abs(v) >= 2147483648.0:
        return INT_MIN
    return int(v)


class RefModel:
    """A synth.Model narrowed to fp32 the way c/jda.c:509-552 reads a double file (plain casts)."""

    def __init__(self, m):
        self.T, self.K, self.L, self.D = m.T, m.K, m.L, m.D
        self.node_n, self.leaf_n, self.dim = m.node_n, m.leaf_n, m.dim
        self.mean_shape = m.mean_shape.astype(f32)
        self.scale, self.lm1, self.lm2, self.nth = m.scale, m.lm1, m.lm2, m.nth
        self.off = m.off.astype(f32)
        self.leaf = m.leaf.astype(f32)
        self.cth, self.cmean, self.cstd = m.cth.astype(f32), m.cmean.astype(f32), m.cstd.astype(f32)
        self.w = m.w.astype(f32)
        self.multi = bool(m.scale.any())


def grid(width, height, scale=1.25, min_size=40, max_size=-1):
    """[(x, y, size)] in the reference's scan order (c/jda.c:320-339, 459-460)."""
    min_size = max(min_size, 24)
    if max_size <= 0:
        max_size = min(width, height)
    max_size = min(max_size, width, height)
    scale = f32(scale)
    win = 24
    out = []
    assert _int(f32(win) * scale) > win, "the reference loop would not terminate"
    while win < min_size:
        win = _int(f32(win) * scale)
    while win <= max_size:
        step = _int(f32(win) * f32(0.1))
        for y in range(0, height - win + 1, step):
            for x in range(0, width - win + 1, step):
                out.append((x, y, win))
        win = _int(f32(win) * scale)
    return out


def _resize(img, w, h):
    """jdaImageResize, c/jda.c:203-230."""
    H, W = img.shape
    xr, yr = f32(W - 1) / f32(w), f32(H - 1) / f32(h)
    fx = (xr * np.arange(w, dtype=f32)).astype(f32)[None, :]
    fy = (yr * np.arange(h, dtype=f32)).astype(f32)[:, None]
    x, y = np.trunc(fx).astype(np.int64), np.trunc(fy).astype(np.int64)
    xd, yd = (fx - x.astype(f32)).astype(f32), (fy - y.astype(f32)).astype(f32)
    flat = img.reshape(-1)
    idx = y * W + x
    a, b, c, d = (flat[idx + o].astype(f32) for o in (0, 1, W, W + 1))
    one = f32(1)
    v = a * (one - xd) * (one - yd)
    v = v + b * xd * (one - yd)
    v = v + c * (one - xd) * yd
    v = v + d * xd * yd
    assert v.dtype == f32
    return np.trunc(v).astype(np.uint8)


def pyramid(frame):
    """(half, quarter) of c/jda.c:450-457, or None for an image that is empty."""
    H, W = frame.shape
    r = f32(1) / np.sqrt(f32(2))
    hw, hh = _int(f32(W) * r), _int(f32(H) * r)
    qw, qh = W // 2, H // 2
    return (_resize(frame, hw, hh) if hw > 0 and hh > 0 else None, _resize(frame, qw, qh) if qw > 0 and qh > 0 else None)


def walk(rm, frame, pyr, x, y, size):
    """One window through the cascade (c/jda.c:340-412).  pyr: pyramid(frame), needed by multi-scale models only."""
    r = f32(1) / np.sqrt(f32(2))
    # (image, origin x, origin y) per scale; every patch side is `size` (c/jda.c:342-354)
    views = [(frame, x, y)]
    if rm.multi:
        views += [(pyr[0], _int(f32(x) * r), _int(f32(y) * r)), (pyr[1], x // 2, y // 2)]
    fsize = f32(size)
    shape = rm.mean_shape.copy()
    score = f32(0)
    hsh = FNV_SEED
    carts_n = 0
    lbf = [0] * rm.K

    def pixel(v):
        c = _int(v * fsize)
        return 0 if c < 0 else (size - 1 if c >= size else c)

    for t in range(rm.T):
        for k in range(rm.K):
            node = 0
            for _ in range(rm.D - 1):
                l1, l2 = 2 * int(rm.lm1[t, k, node]), 2 * int(rm.lm2[t, k, node])
                o = rm.off[t, k, node]
                x1, y1 = pixel(shape[l1] + o[0]), pixel(shape[l1 + 1] + o[1])
                x2, y2 = pixel(shape[l2] + o[2]), pixel(shape[l2 + 1] + o[3])
                img, ox, oy = views[int(rm.scale[t, k, node])]
                ih, iw = img.shape
                # the clamped multi-scale read: the reference indexes past the half / quarter image here
                a = int(img[min(oy + y1, ih - 1), min(ox + x1, iw - 1)])
                b = int(img[min(oy + y2, ih - 1), min(ox + x2, iw - 1)])
                node = 2 * node + 1 if a - b <= int(rm.nth[t, k, node]) else 2 * node + 2
            leaf = node - rm.node_n
            carts_n += 1
            hsh = ((hsh ^ leaf) * FNV_PRIME) & 0xffffffff
            score = score + rm.leaf[t, k, leaf]
            score = (score - rm.cmean[t, k]) / rm.cstd[t, k]
            if score < rm.cth[t, k]:
                return dict(carts_n=carts_n, score=f32(score), path_hash=hsh, shapes=shape, rejected=True)    # `goto next`
            lbf[k] = k * rm.leaf_n + leaf
        for k in range(rm.K):
            shape = shape + rm.w[t, lbf[k]]
    return dict(carts_n=carts_n, score=f32(score), path_hash=hsh, shapes=shape, rejected=False)               # c/jda.c:414 is reached


def validate(rm, frames, windows, th=-0.5):
    """jdaValidateWindows' outputs for rows of (frame, x, y, size)."""
    windows = np.asarray(windows, np.int64).reshape(-1, 4)
    n = len(windows)
    out = dict(rejected=np.zeros(n, bool), is_face=np.zeros(n, np.uint8), score=np.zeros(n, f32), carts_n=np.zeros(n, np.int32), path_hash=np.zeros(n, np.uint32),
               shapes=np.zeros((n, rm.dim), f32), landmarks=np.zeros((n, rm.dim), f32))
    pyrs = {}
    for i, (fr, x, y, size) in enumerate(windows):
        fr, x, y, size = int(fr), int(x), int(y), int(size)
        if rm.multi and fr not in pyrs:
            pyrs[fr] = pyramid(frames[fr])
        r = walk(rm, frames[fr], pyrs.get(fr), x, y, size)
        assert r["shapes"].dtype == f32 and r["score"].dtype == f32
        out["rejected"][i] = r["rejected"]
        out["carts_n"][i], out["score"][i], out["path_hash"][i], out["shapes"][i] = r["carts_n"], r["score"], r["path_hash"], r["shapes"]
        # c/jda.c:414 is reached by a window no cart rejected -- carts_n == T*K does not say that: the LAST cart's reject counts
        # T*K carts too -- and passed with !(score < th)
        out["is_face"][i] = 0 if r["rejected"] or r["score"] < f32(th) else 1
        lm = r["shapes"] * f32(size)                                                                        # c/jda.c:471-472
        lm[0::2] = lm[0::2] + f32(x)
        lm[1::2] = lm[1::2] + f32(y)
        out["landmarks"][i] = lm
    return out
