"""Which refusal wins when a call to a frame entry has TWO faults (include/jda.h: jdaPackGray[Oriented|Reduced|Rotated][Device],
jdaOrientBack, jdaReduceBack, jdaRotateBack).  The other host tests pin every refusal on its own; this one pins their order,
and that a refused call leaves dst, boxes, landmarks and stats as they were.  No GPU: the device entries refuse all of this
before they open the device."""
import ctypes as C

import numpy as np
import pytest

import pack_ref as pr

KINDS = ["pack", "turn", "reduce", "rotate"]
PACK_NAME = {"pack": "jdaPackGray", "turn": "jdaPackGrayOriented", "reduce": "jdaPackGrayReduced", "rotate": "jdaPackGrayRotated"}
BACK_NAME = {"turn": "jdaOrientBack", "reduce": "jdaReduceBack", "rotate": "jdaRotateBack"}
NAN = float("nan")


@pytest.fixture(scope="module")
def api(built):
    from jda_amd import api
    return api


@pytest.fixture(scope="module")
def casc(api, tmp_path_factory):
    from jda_amd import synth
    p = str(tmp_path_factory.mktemp("refusals") / "m.model")
    synth.make_model(1, 4, 3, 2).save(p, 8)
    c = api.Cascador(p)
    yield c
    c.close()


def _ints(v):
    return None if v is None else (C.c_int * len(v))(*v)


class Frames:
    """Two good images -- a: 4 x 4 BGR24, b: 8 x 8 gray -- and a 512-byte destination; what a case changes, it changes here."""

    def __init__(self, api):
        rng = np.random.default_rng(5)
        self.api = api
        self.a = rng.integers(0, 256, (4, 4, 3), dtype=np.uint8)
        self.b = rng.integers(0, 256, (8, 8), dtype=np.uint8)
        self.dst = np.full(512, 0xA5, np.uint8)

    def img(self, i, **kw):
        arr, fmt, bpp = ((self.a, pr.BGR24, 3), (self.b, pr.GRAY8, 1))[i]
        f = dict(data=arr.ctypes.data, pitch=arr.shape[1] * bpp, width=arr.shape[1], height=arr.shape[0], format=fmt, x=0, y=0, w=0, h=0)
        f.update(kw)
        return self.api.jdaPixels(*[f[k] for k in ("data", "pitch", "width", "height", "format", "x", "y", "w", "h")])

    def wide(self):                                       # 50000 x 1: refused (or not looked at) before a byte of it is read
        return self.api.jdaPixels(self.a.ctypes.data, 50000, 50000, 1, pr.GRAY8, 0, 0, 0, 0)


def _pack_call(fr, kind, casc, stats, images="good", n=2, dst="good", offs=(16, 128), orients=(0, 1), factors=(1, 2), degrees=(0.0, 30.0)):
    api = fr.api
    if images == "good":
        images = [fr.img(0), fr.img(1)]
    px = None if images is None else (api.jdaPixels * len(images))(*images)
    d = fr.dst.ctypes.data if isinstance(dst, str) else dst
    o = None if offs is None else (C.c_size_t * len(offs))(*offs)
    g = None if degrees is None else (C.c_double * len(degrees))(*degrees)
    mid = {"pack": (), "turn": (_ints(orients),), "reduce": (_ints(factors), _ints(orients)), "rotate": (g,)}[kind]
    if casc is None:
        return getattr(api.lib, PACK_NAME[kind])(px, *mid, n, d, o)
    return getattr(api.lib, PACK_NAME[kind] + "Device")(casc.h, px, *mid, n, d, o, None, stats)


def _pack_cases(fr):
    """(what, kinds, what the call changes, a piece of the message of the fault that wins, a piece it must not hold)"""
    bad0 = {"pack": dict(images=[fr.img(0, x=1), fr.img(1, data=None)]), "turn": dict(orients=(8, 0), images=[fr.img(0), fr.img(1, data=None)]),
            "reduce": dict(factors=(0, 1), images=[fr.img(0), fr.img(1, data=None)]), "rotate": dict(degrees=(NAN, 0.0), images=[fr.img(0), fr.img(1, data=None)])}
    bad1 = {"pack": dict(images=[fr.img(0), fr.img(1, data=None)]), "turn": dict(orients=(0, 8)), "reduce": dict(factors=(1, 9)), "rotate": dict(degrees=(0.0, NAN))}
    need = {"pack": ("offs", "null destination"), "turn": ("orients", "null orients"), "reduce": ("factors", "null factors"), "rotate": ("degrees", "null degrees")}
    cases = [("n < 0 beats null images", KINDS, dict(n=-3, images=None), "negative number of images (n = -3)", "null"),
             ("null images beats null destination", KINDS, dict(images=None, dst=None), "null images", "destination"),
             ("null dst_offsets beats image 0", KINDS, dict(offs=None, images=[fr.img(0, data=None), fr.img(1)]), "null dst_offsets", "image 0"),
             ("null data beats the format", KINDS, dict(images=[fr.img(0, data=None, format=9), fr.img(1)]), "image 0: null data", "format"),
             ("the format beats the size", KINDS, dict(images=[fr.img(0, format=9, width=0), fr.img(1)]), "image 0: unknown format 9", "at least one pixel"),
             ("the size beats the pitch", KINDS, dict(images=[fr.img(0, width=0, pitch=-1), fr.img(1)]), "image 0: width x height = 0 x 4", "pitch"),
             ("the pitch beats the rectangle", KINDS, dict(images=[fr.img(0, pitch=1, x=1), fr.img(1)]), "image 0: pitch 1 is smaller than a row", "rectangle"),
             ("the image beats its orientation", ["turn", "reduce"], dict(images=[fr.img(0, format=9), fr.img(1)], orients=(9, 0)), "image 0: unknown format 9", "orientation"),
             ("the image beats its factor", ["reduce"], dict(images=[fr.img(0, format=9), fr.img(1)], factors=(0, 1)), "image 0: unknown format 9", "factor"),
             ("the image beats its angle", ["rotate"], dict(images=[fr.img(0, format=9), fr.img(1)], degrees=(NAN, 0.0)), "image 0: unknown format 9", "angle"),
             ("the orientation beats the factor", ["reduce"], dict(orients=(9, 0), factors=(0, 1)), "image 0: unknown orientation 9 (0..7)", "factor"),
             ("the factor's range beats 'has no pixel'", ["reduce"], dict(factors=(9, 1)), "image 0: factor 9 (1..8)", "has no pixel"),
             ("'has no pixel' in image 0 beats image 1", ["reduce"], dict(factors=(5, 1), images=[fr.img(0), fr.img(1, data=None)]),
              "image 0: a rectangle of 4 x 4 reduced by factor 5 has no pixel", "image 1"),
             ("the plan in image 0 beats the side in image 1", ["rotate"], dict(degrees=(NAN, 0.0), images=[fr.img(0), fr.wide()]), "image 0: angle", "a side"),
             ("the side in image 0 beats image 1", ["rotate"], dict(degrees=(0.0, 0.0), images=[fr.wide(), fr.img(1, data=None)]),
              "image 0: a rectangle of 50000 x 1 rotated by", "image 1")]
    for k in KINDS:
        field, msg = need[k]
        cases.append(("null destination beats what %s needs next" % k, [k], {"dst": None, field: None}, "null destination", field if k != "pack" else "dst_offsets"))
        if k != "pack":
            cases.append(("%s beats null dst_offsets" % msg, [k], {field: None, "offs": None}, msg, "dst_offsets"))
        cases.append(("image 0 beats image 1 (%s)" % k, [k], bad0[k], "image 0: ", "image 1"))
        cases.append(("image 1 beats overlapping destinations (%s)" % k, [k], dict(bad1[k], offs=(16, 17)), "image 1: ", "overlap"))
    return cases


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_pack_entries_refuse_the_earlier_fault(api, casc, device):
    fr = Frames(api)
    st = api.jdaPackStats()
    for what, kinds, change, first, never in _pack_cases(fr):
        for kind in kinds:
            C.memset(C.byref(st), 0x5A, C.sizeof(st))
            assert _pack_call(fr, kind, casc if device else None, C.byref(st), **change) == -1, (what, kind)
            err = api.last_error()
            assert err.startswith(PACK_NAME[kind] + ("Device: " if device else ": ")) and first in err and never not in err, (what, kind, err)
            assert (fr.dst == 0xA5).all() and bytes(st) == b"\x5A" * C.sizeof(st), (what, kind)


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_pack_entries_overlap_beats_source_rows(api, casc, device):
    # both destinations overlap each other, and image 0's lies in its own source rows
    src = np.random.default_rng(6).integers(0, 256, 256, dtype=np.uint8)
    keep = src.copy()
    fr = Frames(api)
    imgs = [api.jdaPixels(src.ctypes.data + 64 * i, 4, 4, 4, pr.GRAY8, 0, 0, 0, 0) for i in range(2)]
    st = api.jdaPackStats()
    for kind in KINDS:
        C.memset(C.byref(st), 0x5A, C.sizeof(st))
        rc = _pack_call(fr, kind, casc if device else None, C.byref(st), images=imgs, dst=src.ctypes.data, offs=(0, 8), orients=(0, 0), factors=(1, 1), degrees=(0.0, 0.0))
        err = api.last_error()
        assert rc == -1 and "the destinations of image 0" in err and "overlap" in err and "source rows" not in err, (kind, err)
        assert np.array_equal(src, keep) and bytes(st) == b"\x5A" * C.sizeof(st), kind


def test_pack_entries_counts_come_first(api, casc):
    fr = Frames(api)
    st = api.jdaPackStats()
    for kind in KINDS:
        none = dict(images=None, n=0, dst=None, offs=None, orients=None, factors=None, degrees=None)
        assert _pack_call(fr, kind, None, None, **none) == 0, kind                       # n == 0 touches nothing
        C.memset(C.byref(st), 0x5A, C.sizeof(st))
        assert _pack_call(fr, kind, casc, C.byref(st), **none) == 0 and bytes(st) == bytes(C.sizeof(st)), kind   # ... and reports nothing done
        # a null cascador is refused before anything else is looked at
        C.memset(C.byref(st), 0x5A, C.sizeof(st))
        mid = {"pack": (), "turn": (None,), "reduce": (None, None), "rotate": (None,)}[kind]
        assert getattr(api.lib, PACK_NAME[kind] + "Device")(None, None, *mid, -3, None, None, None, C.byref(st)) == -1
        assert api.last_error() == PACK_NAME[kind] + "Device: null cascador" and bytes(st) == b"\x5A" * C.sizeof(st)


# ---- the way back -------------------------------------------------------------------------------------------------------------
def _back_call(fr, kind, keep, images="good", n_images=2, orients=(0, 1), factors=(1, 2), degrees=(0.0, 30.0), face_image=(0, 1, 1), n_faces=3,
               boxes=True, box_ints=4, landmarks=True, real_bytes=8, landmark_n=2, left=(0,), right=(1,), sym_n=1):
    api = fr.api
    if images == "good":
        images = [fr.img(0), fr.img(1)]
    px = None if images is None else (api.jdaPixels * len(images))(*images)
    g = None if degrees is None else (C.c_double * len(degrees))(*degrees)
    ip = C.POINTER(C.c_int)
    b, lm = keep
    tail = (n_images, _ints(face_image), n_faces, b.ctypes.data_as(ip) if boxes else None, box_ints, lm.ctypes.data if landmarks else None, real_bytes, landmark_n)
    if kind == "rotate":
        return api.lib.jdaRotateBack(px, g, *tail)
    head = (px, _ints(orients)) if kind == "turn" else (px, _ints(factors), _ints(orients))
    return getattr(api.lib, BACK_NAME[kind])(*head, *tail, _ints(left), _ints(right), sym_n)


def _back_cases(fr):
    TR, ALL = ["turn", "reduce"], ["turn", "reduce", "rotate"]
    null0 = [fr.img(0, data=None), fr.img(1)]
    return [("null factors beats a negative count", ["reduce"], dict(factors=None, n_images=-1), "null factors", "negative"),
            ("null degrees beats a negative count", ["rotate"], dict(degrees=None, n_images=-1), "null degrees", "negative"),
            ("... but only with faces to take back", ["reduce"], dict(factors=None, n_faces=-1), "negative number of faces (n_faces = -1)", "null"),
            ("... but only with faces to take back", ["rotate"], dict(degrees=None, n_faces=-1), "negative number of faces (n_faces = -1)", "null"),
            ("n_faces < 0 beats n_images < 0", ALL, dict(n_faces=-1, n_images=-2), "negative number of faces (n_faces = -1)", "n_images"),
            ("n_images < 0 beats no faces", ALL, dict(n_faces=0, n_images=-2), "negative number of images (n_images = -2)", "n_faces"),
            ("n_images < 0 beats null images", ALL, dict(n_images=-2, images=None), "negative number of images (n_images = -2)", "null"),
            ("null images beats null orients", TR, dict(images=None, orients=None), "null images", "orients"),
            ("null images beats null face_image", ALL, dict(images=None, face_image=None), "null images", "face_image"),
            ("null orients beats null face_image", TR, dict(orients=None, face_image=None), "null orients", "face_image"),
            ("null face_image beats box_ints", ALL, dict(face_image=None, box_ints=5), "null face_image", "box_ints"),
            ("box_ints beats real_bytes", ALL, dict(box_ints=5, real_bytes=3), "box_ints = 5", "real_bytes"),
            ("real_bytes beats landmark_n", ALL, dict(real_bytes=3, landmark_n=0), "real_bytes = 3", "landmark_n"),
            ("landmark_n beats sym_n", TR, dict(landmark_n=0, sym_n=-1), "landmark_n = 0", "pairs"),
            ("landmark_n beats image 0", ALL, dict(landmark_n=0, images=null0), "landmark_n = 0", "image 0"),
            ("sym_n beats image 0", TR, dict(sym_n=-1, images=null0), "negative number of pairs (sym_n = -1)", "image 0"),
            ("null left beats image 0", TR, dict(left=None, images=null0), "null left or right", "image 0"),
            ("a pair's range beats image 0", TR, dict(left=(7,), images=null0), "pair 0 = (7, 1) names a landmark outside [0, 2)", "image 0"),
            ("the image beats its orientation", TR, dict(images=[fr.img(0, format=9), fr.img(1)], orients=(9, 0)), "image 0: unknown format 9", "orientation"),
            ("the image beats its factor", ["reduce"], dict(images=[fr.img(0, format=9), fr.img(1)], factors=(0, 1)), "image 0: unknown format 9", "factor"),
            ("the image beats its angle", ["rotate"], dict(images=[fr.img(0, format=9), fr.img(1)], degrees=(NAN, 0.0)), "image 0: unknown format 9", "angle"),
            ("the orientation beats the factor", ["reduce"], dict(orients=(9, 0), factors=(0, 1)), "image 0: unknown orientation 9 (0..7)", "factor"),
            ("the factor's range beats 'has no pixel'", ["reduce"], dict(factors=(9, 1)), "image 0: factor 9 (1..8)", "has no pixel"),
            ("'has no pixel' in image 0 beats image 1", ["reduce"], dict(factors=(5, 1), images=[fr.img(0), fr.img(1, data=None)]),
             "image 0: a rectangle of 4 x 4 reduced by factor 5 has no pixel", "image 1"),
            ("the orientation of image 0 beats image 1", TR, dict(orients=(8, 0), images=[fr.img(0), fr.img(1, data=None)]), "image 0: unknown orientation 8", "image 1"),
            ("the angle of image 0 beats image 1", ["rotate"], dict(degrees=(NAN, 0.0), images=[fr.img(0), fr.img(1, data=None)]), "image 0: angle", "image 1"),
            ("image 1 beats a face's image", ALL, dict(images=[fr.img(0), fr.img(1, data=None)], face_image=(0, 5, 1)), "image 1: null data", "face 1"),
            ("a face's image comes last", ALL, dict(face_image=(0, 5, 1)), "face 1: face_image 5 is outside [0, 2)", "image 1")]


def test_way_back_refuses_the_earlier_fault(api):
    fr = Frames(api)
    b0 = np.arange(12, dtype=np.int32).reshape(3, 4) % 3
    lm0 = np.arange(12, dtype=np.float64).reshape(3, 4) / 4
    for what, kinds, change, first, never in _back_cases(fr):
        for kind in kinds:
            b, lm = b0.copy(), lm0.copy()
            assert _back_call(fr, kind, (b, lm), **change) == -1, (what, kind)
            err = api.last_error()
            assert err.startswith(BACK_NAME[kind] + ": ") and first in err and never not in err, (what, kind, err)
            assert np.array_equal(b, b0) and np.array_equal(lm, lm0), (what, kind)


def test_way_back_counts_come_first(api):
    fr = Frames(api)
    keep = (np.zeros((1, 4), np.int32), np.zeros((1, 4)))
    for kind in BACK_NAME:                               # no faces: nothing is looked at, not even a NULL pointer
        assert _back_call(fr, kind, keep, images=None, n_images=0, orients=None, factors=None, degrees=None, face_image=None, n_faces=0, boxes=False,
                          landmarks=False, left=None, right=None) == 0, kind
    # jdaRotateBack takes back from a rotated image of any side: the limit is the pack entries'
    assert _pack_call(fr, "rotate", None, None, images=[fr.wide()], n=1, offs=(0,), degrees=(0.0,)) == -1 and "a side" in api.last_error()
    assert _back_call(fr, "rotate", keep, images=[fr.wide()], n_images=1, degrees=(0.0,), face_image=(0,), n_faces=1, boxes=False, landmarks=False) == 0
