"""The definition of "frames as they arrive" (include/jda.h) restated in numpy, int64 arithmetic:
gray = (B * 1868 + G * 9617 + R * 4899 + 8192) >> 14, alpha ignored, GRAY8 a copy; a rectangle (x, y, w, h) is cut first.
Written from the header, not from jda_amd.fddb.bgr2gray (tests/test_pack_host.py shows that the two agree).  Also the
helpers both test files build their sources with."""
import numpy as np

GRAY8, BGR24, RGB24, BGRA32, RGBA32 = range(5)
FORMATS = (GRAY8, BGR24, RGB24, BGRA32, RGBA32)
BPP = {GRAY8: 1, BGR24: 3, RGB24: 3, BGRA32: 4, RGBA32: 4}
WB, WG, WR = 1868, 9617, 4899


def gray(img, fmt):
    """uint8 [H, W] (GRAY8) or [H, W, C] -> uint8 [H, W]."""
    img = np.asarray(img)
    if fmt == GRAY8:
        return np.array(img.reshape(img.shape[0], img.shape[1]), np.uint8)
    v = img.astype(np.int64)
    b, r = (v[..., 0], v[..., 2]) if fmt in (BGR24, BGRA32) else (v[..., 2], v[..., 0])
    return ((b * WB + v[..., 1] * WG + r * WR + 8192) >> 14).astype(np.uint8)


def pack(img, fmt, rect=None):
    g = gray(img, fmt)
    if rect is None or (rect[2] == 0 and rect[3] == 0):
        return g
    x, y, w, h = rect
    return np.ascontiguousarray(g[y:y + h, x:x + w])


def shape_of(h, w, fmt):
    return (h, w) if fmt == GRAY8 else (h, w, BPP[fmt])


def pitched(rng, h, w, fmt, slack=0, base=0):
    """A random image whose rows lie w * bpp + slack bytes apart, pixel (0, 0) at byte `base` of a flat buffer that ENDS with
    the last row's last pixel.  -> (flat uint8 buffer, the [H, W(, C)] view into it, element strides of that view)."""
    bpp = BPP[fmt]
    pitch = w * bpp + slack
    flat = rng.integers(0, 256, base + (h - 1) * pitch + w * bpp, dtype=np.uint8)
    strides = (pitch, 1) if fmt == GRAY8 else (pitch, bpp, 1)
    view = np.lib.stride_tricks.as_strided(flat[base:], shape_of(h, w, fmt), strides, writeable=False)
    return flat, view, strides


def all_colours():
    """Every 24-bit colour once, as one 4096 x 4096 x 3 image (byte 0 fastest)."""
    v = np.arange(1 << 24, dtype=np.uint32)
    img = np.empty((1 << 24, 3), np.uint8)
    img[:, 0] = v & 255; img[:, 1] = (v >> 8) & 255; img[:, 2] = v >> 16
    return img.reshape(4096, 4096, 3)


RECTS = {"whole": lambda w, h: (0, 0, w, h), "pixel": lambda w, h: (w // 3, h // 2, 1, 1), "last row": lambda w, h: (0, h - 1, w, 1),
         "last column": lambda w, h: (w - 1, 0, 1, h), "interior": lambda w, h: (3, 2, w - 7, h - 5)}
