"""ctypes binding of libjda.so -- the host-side mirror of the reference's C API.

The function names, argument order and ownership rules are the reference's
(reference c/jda.h:31-68): jdaCascadorCreateDouble / jdaCascadorCreateFloat /
jdaCascadorSerializeTo / jdaCascadorRelease / jdaDetect / jdaResultRelease.
On top of that sit thin numpy-friendly wrappers for the additive batch and
trace entry points of include/jda.h.

There is no fallback: if libjda.so is missing this module raises at import
time, and if no HIP device is usable every detect call raises JdaError.
"""
import collections
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("JDA_LIB_PATH") or os.path.join(_HERE, "libjda.so")

JDA_DIALECT_C = 0
JDA_DIALECT_CPP = 1
# include/jda.h: JDA_FINISH_*, the finishing forms a pass can take, in the order of jdaFinishForms' counts
FINISH_FORMS = ("WIDE_CONC", "WIDE_SEQ", "MERGED", "FILTER0", "MID_DIRECT", "TWO_LAUNCH", "DENSE")


def _launch_key(name, fields, doc):
    """The namedtuple of one launch report's key: `fields` are (name, values in index order) in the order of the header's
    index macro, whose mixed-radix index the class computes (index) and takes apart (of_index)."""
    def index(self):
        i = 0
        for (_, values), v in zip(fields, self):
            i = i * len(values) + values.index(v)
        return i

    def of_index(cls, i):
        out = []
        for _, values in reversed(fields):
            out.append(values[i % len(values)])
            i //= len(values)
        return cls(*reversed(out))

    base = collections.namedtuple(name, [f for f, _ in fields])
    return type(name, (base,), dict(__slots__=(), __doc__=doc, index=index, of_index=classmethod(of_index)))


# include/jda.h: the fields of a scan form's key in the order of JDA_SCAN_FORM, each with its values in index order
SCAN_FORM_FIELDS = (("kernel", ("k_scan", "k_scan_p")), ("dialect", ("C", "CPP")), ("depth", (4, 6, 0)),
                    ("pix", ("T16_256", "T16_512", "T21", "GLB")), ("ragged", (False, True)), ("lean", (False, True)),
                    ("trace", (False, True)), ("merged", (False, True)))
SCAN_FORM_N = 768
ScanForm = _launch_key("ScanForm", SCAN_FORM_FIELDS,
                       "The key of one scan instantiation (include/jda.h: JDA_SCAN_FORM); depth 0 = the generic walk.")
# include/jda.h: the fields of a finishing launch's key in the order of JDA_FINISH_LAUNCH, each with its values in index order
FINISH_LAUNCH_FIELDS = (("kernel", ("k_finish", "k_filter0")), ("dialect", ("C", "CPP")), ("trace", (False, True)),
                        ("groups", (0, 1, 2, 3, 4)), ("multi", (False, True)), ("st", (False, True)), ("stream", (False, True)),
                        ("survivors", (False, True)), ("carry", (False, True)), ("tile", (False, True)))
FINISH_LAUNCH_N = 2560
FinishLaunch = _launch_key("FinishLaunch", FINISH_LAUNCH_FIELDS,
                           "The key of one k_finish / k_filter0 launch (include/jda.h: JDA_FINISH_LAUNCH); groups 0 = k_filter0.")
# include/jda.h: the fields of a k_stage launch's key in the order of JDA_STAGE_LAUNCH, each with its values in index order
STAGE_LAUNCH_FIELDS = (("dialect", ("C", "CPP")), ("trace", (False, True)), ("glb", (False, True)), ("acc", (12, 32, 64, 160)),
                       ("chunk", (4, 8, 16, 32, 64)))
STAGE_LAUNCH_N = 160
StageLaunch = _launch_key("StageLaunch", STAGE_LAUNCH_FIELDS, "The key of one k_stage launch (include/jda.h: JDA_STAGE_LAUNCH).")
# include/jda.h: jdaMineLaunches' counts in index order (JDA_MINE_K_SCAN .. JDA_MINE_WALK_CAP, lower case without the prefix)
MINE_LAUNCH_FIELDS = ("k_scan", "k_items", "k_patches", "k_walk", "k_sum", "chunks", "walk_batches", "sum_saturated", "scan_rejects",
                      "walk_rejects", "walk_batch_max", "walk_cap")
MINE_LAUNCH_N = 12


class JdaError(RuntimeError):
    pass


class jdaResult(C.Structure):
    _fields_ = [("n", C.c_int), ("landmark_n", C.c_int), ("bboxes", C.POINTER(C.c_int)),
                ("shapes", C.POINTER(C.c_float)), ("scores", C.POINTER(C.c_float))]


class jdaResultD(C.Structure):
    _fields_ = [("n", C.c_int), ("landmark_n", C.c_int), ("rects", C.POINTER(C.c_int)),
                ("shapes", C.POINTER(C.c_double)), ("scores", C.POINTER(C.c_double))]


class jdaModelInfo(C.Structure):
    _fields_ = [("T", C.c_int), ("K", C.c_int), ("landmark_n", C.c_int), ("tree_depth", C.c_int),
                ("multi_scale", C.c_int), ("source_real_bytes", C.c_int)]


class jdaStats(C.Structure):
    _fields_ = [("patch_n", C.c_longlong), ("face_patch_n", C.c_longlong), ("nonface_patch_n", C.c_longlong),
                ("cart_gothrough_n", C.c_longlong), ("stage_done_n", C.c_longlong * 16),
                ("average_cart_n", C.c_double), ("gpu_ms", C.c_double), ("scan_ms", C.c_double),
                ("host_ms", C.c_double), ("scan_cart_n", C.c_longlong), ("scan_patch_n", C.c_longlong),
                ("scan_launches", C.c_int), ("handoff_n", C.c_longlong), ("cart_total_n", C.c_longlong),
                ("call_ms", C.c_double), ("dense_passes", C.c_int), ("scan_lds_ms", C.c_double),
                ("scan_lds_cart_n", C.c_longlong), ("scan_fallbacks", C.c_int),
                ("ws_regrows", C.c_int), ("post_passes", C.c_int), ("post_declined", C.c_int)]

    def asdict(self):
        d = {k: getattr(self, k) for k, _ in self._fields_ if k != "stage_done_n"}
        d["stage_done_n"] = list(self.stage_done_n)
        return d


class jdaMineStats(C.Structure):
    _fields_ = [("windows", C.c_longlong), ("nega_n", C.c_longlong), ("carts_n", C.c_longlong), ("next_start", C.c_longlong),
                ("total_windows", C.c_longlong), ("hits", C.c_int), ("call_ms", C.c_double)]

    def asdict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class jdaSamplesCpp(C.Structure):
    _fields_ = [("patches", C.c_void_p), ("patches_on_device", C.c_int), ("shapes", C.POINTER(C.c_double)),
                ("weights", C.POINTER(C.c_double)), ("residual", C.POINTER(C.c_double)), ("has_gt", C.POINTER(C.c_ubyte)),
                ("n", C.c_int)]


class jdaFeatureCpp(C.Structure):
    _fields_ = [("scale", C.c_int), ("landmark_id1", C.c_int), ("landmark_id2", C.c_int), ("offset1_x", C.c_double),
                ("offset1_y", C.c_double), ("offset2_x", C.c_double), ("offset2_y", C.c_double)]


class jdaTrainNodeCpp(C.Structure):
    _fields_ = [("pos_n", C.c_int), ("neg_n", C.c_int), ("feature_idx", C.c_int), ("threshold", C.c_int), ("mode", C.c_int),
                ("pad", C.c_int), ("criterion", C.c_double)]


class jdaTrainStatsCpp(C.Structure):
    _fields_ = [("call_ms", C.c_double), ("setup_ms", C.c_double), ("device_ms", C.c_double), ("sweep_ms", C.c_double),
                ("partition_ms", C.c_double), ("feature_evals", C.c_longlong), ("feature_chunks", C.c_int),
                ("nodes", C.POINTER(jdaTrainNodeCpp))]


class jdaSplitSumsCpp(C.Structure):
    _fields_ = [("pos_values", C.POINTER(C.c_short)), ("neg_values", C.POINTER(C.c_short)),
                ("pos_hist_w", C.POINTER(C.c_double)), ("neg_hist_w", C.POINTER(C.c_double)),
                ("pos_hist_c", C.POINTER(C.c_int)), ("neg_hist_c", C.POINTER(C.c_int)), ("var_sums", C.POINTER(C.c_double)),
                ("var_n_left", C.POINTER(C.c_int)), ("var_n_right", C.POINTER(C.c_int)), ("var_th", C.POINTER(C.c_int)),
                ("chunks", C.c_int)]


class jdaStageCartsCpp(C.Structure):
    _fields_ = [("features", C.POINTER(jdaFeatureCpp)), ("thresholds", C.POINTER(C.c_int)), ("K", C.c_int)]


class jdaStageStatsCpp(C.Structure):
    _fields_ = [("call_ms", C.c_double), ("upload_ms", C.c_double), ("device_ms", C.c_double), ("download_ms", C.c_double),
                ("chunks", C.c_int), ("lds_path", C.c_int), ("waves_per_group", C.c_int), ("lds_bytes", C.c_int)]

    def asdict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class jdaFitParamsCpp(C.Structure):
    _fields_ = [("C", C.c_double), ("eps", C.c_double), ("max_iter", C.c_int), ("seed", C.c_uint64)]


class jdaFitStatsCpp(C.Structure):
    _fields_ = [("call_ms", C.c_double), ("shuffle_ms", C.c_double), ("upload_ms", C.c_double), ("device_ms", C.c_double),
                ("epochs_launched", C.c_int), ("lds_path", C.c_int), ("lds_bytes", C.c_int)]

    def asdict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class jdaGatherSegCpp(C.Structure):
    _fields_ = [("patches", C.c_void_p), ("on_device", C.c_int), ("n", C.c_int)]


class jdaGatherStatsCpp(C.Structure):
    _fields_ = [("call_ms", C.c_double), ("upload_ms", C.c_double), ("device_ms", C.c_double), ("download_ms", C.c_double),
                ("bytes", C.c_longlong), ("chunks", C.c_int), ("launches", C.c_int)]

    def asdict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class jdaPositivesStatsCpp(C.Structure):
    _fields_ = [("call_ms", C.c_double), ("upload_ms", C.c_double), ("device_ms", C.c_double), ("download_ms", C.c_double),
                ("bytes", C.c_longlong), ("image_chunks", C.c_int), ("images_uploaded", C.c_int), ("chunks", C.c_int),
                ("launches", C.c_int)]

    def asdict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class jdaPixels(C.Structure):
    _fields_ = [("data", C.c_void_p), ("pitch", C.c_longlong), ("width", C.c_int), ("height", C.c_int), ("format", C.c_int),
                ("x", C.c_int), ("y", C.c_int), ("w", C.c_int), ("h", C.c_int)]


class jdaRotation(C.Structure):
    _fields_ = [("c", C.c_double), ("s", C.c_double), ("w", C.c_int), ("h", C.c_int), ("tw", C.c_int), ("th", C.c_int)]

    def asdict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class jdaPackStats(C.Structure):
    _fields_ = [("pixels", C.c_longlong), ("bytes_in", C.c_longlong), ("bytes_out", C.c_longlong), ("launches", C.c_int),
                ("device_ms", C.c_double), ("call_ms", C.c_double)]

    def asdict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class jdaChipStats(C.Structure):
    _fields_ = [("faces", C.c_longlong), ("chip_bytes", C.c_longlong), ("taps", C.c_longlong), ("launches", C.c_int),
                ("device_ms", C.c_double), ("call_ms", C.c_double)]

    def asdict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


# include/jda.h, "frames as they arrive": JDA_PIX_* and their bytes per pixel
JDA_PIX_GRAY8, JDA_PIX_BGR24, JDA_PIX_RGB24, JDA_PIX_BGRA32, JDA_PIX_RGBA32 = range(5)
PIX_FORMATS = {"gray8": JDA_PIX_GRAY8, "bgr24": JDA_PIX_BGR24, "rgb24": JDA_PIX_RGB24, "bgra32": JDA_PIX_BGRA32,
               "rgba32": JDA_PIX_RGBA32}
PIX_BYTES = {JDA_PIX_GRAY8: 1, JDA_PIX_BGR24: 3, JDA_PIX_RGB24: 3, JDA_PIX_BGRA32: 4, JDA_PIX_RGBA32: 4}


# numpy view of jdaFeatureCpp arrays (same layout: three ints, four bytes of padding, four doubles)
FEATURE_DTYPE = np.dtype([("scale", np.int32), ("landmark_id1", np.int32), ("landmark_id2", np.int32), ("pad", np.int32),
                          ("offset1_x", np.float64), ("offset1_y", np.float64), ("offset2_x", np.float64),
                          ("offset2_y", np.float64)])
NODE_DTYPE = np.dtype([("pos_n", np.int32), ("neg_n", np.int32), ("feature_idx", np.int32), ("threshold", np.int32),
                       ("mode", np.int32), ("pad", np.int32), ("criterion", np.float64)])
assert FEATURE_DTYPE.itemsize == C.sizeof(jdaFeatureCpp) and NODE_DTYPE.itemsize == C.sizeof(jdaTrainNodeCpp)


class jdaDetectOptions(C.Structure):
    _fields_ = [("dialect", C.c_int), ("nms", C.c_int), ("nms_overlap", C.c_float), ("cpp_step", C.c_int),
                ("hip_stream", C.c_void_p), ("stats", C.POINTER(jdaStats))]


def _load():
    if not os.path.exists(LIB_PATH):
        raise ImportError("jda_amd: %s is missing -- build it with `python -m jda_amd.build` "
                          "(there is no pure-Python or CPU fallback)" % LIB_PATH)
    # If torch is going to share device pointers with us it must be the one to
    # load the HIP runtime first (both resolve to the same libamdhip64.so.7).
    try:
        import torch  # noqa: F401
    except Exception:
        pass
    lib = C.CDLL(LIB_PATH)
    u8p = C.POINTER(C.c_ubyte)
    lib.jdaCascadorCreateDouble.restype = C.c_void_p
    lib.jdaCascadorCreateDouble.argtypes = [C.c_char_p]
    lib.jdaCascadorCreateFloat.restype = C.c_void_p
    lib.jdaCascadorCreateFloat.argtypes = [C.c_char_p]
    lib.jdaCascadorCreate.restype = C.c_void_p
    lib.jdaCascadorCreate.argtypes = [C.c_char_p]
    lib.jdaDebugPlanTiles.restype = C.c_int
    lib.jdaDebugPlanTiles.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_float, C.c_int, C.c_int, C.POINTER(C.c_int), C.c_int]
    lib.jdaCascadorSerializeTo.restype = None
    lib.jdaCascadorSerializeTo.argtypes = [C.c_void_p, C.c_char_p]
    lib.jdaCascadorRelease.restype = None
    lib.jdaCascadorRelease.argtypes = [C.c_void_p]
    lib.jdaDetect.restype = jdaResult
    lib.jdaDetect.argtypes = [C.c_void_p, u8p, C.c_int, C.c_int, C.c_float, C.c_float, C.c_int, C.c_int, C.c_float]
    lib.jdaResultRelease.restype = None
    lib.jdaResultRelease.argtypes = [jdaResult]
    lib.jdaGetLastError.restype = C.c_char_p
    lib.jdaCascadorInfo.argtypes = [C.c_void_p, C.POINTER(jdaModelInfo)]
    lib.jdaSetDevice.argtypes = [C.c_void_p, C.c_int]
    lib.jdaSetOption.argtypes = [C.c_void_p, C.c_char_p, C.c_longlong]
    lib.jdaGetOption.restype = C.c_longlong
    lib.jdaGetOption.argtypes = [C.c_void_p, C.c_char_p]
    lib.jdaFinishForms.argtypes = [C.c_void_p, C.POINTER(C.c_longlong)]
    lib.jdaScanForms.argtypes = [C.c_void_p, C.POINTER(C.c_longlong)]
    lib.jdaFinishLaunches.argtypes = [C.c_void_p, C.POINTER(C.c_longlong)]
    lib.jdaFinishTileWin.argtypes = [C.c_void_p, C.c_int]
    lib.jdaStageLaunches.argtypes = [C.c_void_p, C.POINTER(C.c_longlong)]
    lib.jdaStageLaunchFor.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int)]
    if hasattr(lib, "jdaMineLaunches"):             # (older builds, loaded through JDA_LIB_PATH for A/B runs, lack it)
        lib.jdaMineLaunches.argtypes = [C.c_void_p, C.POINTER(C.c_longlong)]
    lib.jdaCountWindows.argtypes = [C.c_int, C.c_int, C.c_float, C.c_int, C.c_int,
                                    C.POINTER(C.c_longlong), C.POINTER(C.c_int)]
    lib.jdaDetectOptionsInit.restype = None
    lib.jdaDetectOptionsInit.argtypes = [C.POINTER(jdaDetectOptions)]
    lib.jdaDetectBatch.argtypes = [C.c_void_p, C.POINTER(u8p), C.c_int, C.c_int, C.c_int, C.c_float, C.c_float,
                                   C.c_int, C.c_int, C.c_float, C.POINTER(jdaDetectOptions), C.POINTER(jdaResult)]
    lib.jdaDetectBatchDevice.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_int, C.c_int, C.c_float,
                                         C.c_float, C.c_int, C.c_int, C.c_float, C.POINTER(jdaDetectOptions),
                                         C.POINTER(jdaResult)]
    if hasattr(lib, "jdaDetectBatchRagged"):        # (older builds, loaded through JDA_LIB_PATH for A/B runs, lack it)
      lib.jdaDetectBatchRagged.argtypes = [C.c_void_p, C.POINTER(u8p), C.POINTER(C.c_int), C.POINTER(C.c_int), C.c_int,
                                         C.c_float, C.c_float, C.c_int, C.c_int, C.c_float, C.POINTER(jdaDetectOptions),
                                         C.POINTER(jdaResult)]
      lib.jdaDetectBatchRaggedDevice.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_size_t), C.POINTER(C.c_int),
                                               C.POINTER(C.c_int), C.c_int, C.c_float, C.c_float, C.c_int, C.c_int,
                                               C.c_float, C.POINTER(jdaDetectOptions), C.POINTER(jdaResult)]
    if hasattr(lib, "jdaDetectBatchRaggedDeviceRows"):     # (r06: the job's detections as one matrix of rows)
        lib.jdaDetectBatchRaggedRows.argtypes = [C.c_void_p, C.POINTER(u8p), C.POINTER(C.c_int), C.POINTER(C.c_int), C.c_int,
                                                 C.c_float, C.c_float, C.c_int, C.c_int, C.c_float, C.POINTER(jdaDetectOptions),
                                                 C.c_int, C.POINTER(C.POINTER(C.c_float)), C.POINTER(C.c_int)]
        lib.jdaDetectBatchRaggedDeviceRows.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_size_t), C.POINTER(C.c_int),
                                                       C.POINTER(C.c_int), C.c_int, C.c_float, C.c_float, C.c_int, C.c_int,
                                                       C.c_float, C.POINTER(jdaDetectOptions), C.c_int,
                                                       C.POINTER(C.POINTER(C.c_float)), C.POINTER(C.c_int)]
        lib.jdaRowsRelease.restype = None
        lib.jdaRowsRelease.argtypes = [C.POINTER(C.c_float)]
    if hasattr(lib, "jdaDetectBatchCppRaggedDeviceRows"):
        dpp = C.POINTER(C.POINTER(C.c_double))
        lib.jdaDetectBatchCppRaggedRows.argtypes = [C.c_void_p, C.POINTER(u8p), C.POINTER(C.c_int), C.POINTER(C.c_int), C.c_int,
                                                    C.c_int, C.c_int, C.c_double, C.c_double, C.c_int, C.POINTER(jdaStats),
                                                    C.c_int, dpp, C.POINTER(C.c_int)]
        lib.jdaDetectBatchCppRaggedDeviceRows.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_size_t), C.POINTER(C.c_int),
                                                          C.POINTER(C.c_int), C.c_int, C.c_int, C.c_int, C.c_double, C.c_double,
                                                          C.c_int, C.POINTER(jdaStats), C.c_int, dpp, C.POINTER(C.c_int)]
        lib.jdaRowsDRelease.restype = None
        lib.jdaRowsDRelease.argtypes = [C.POINTER(C.c_double)]
    lib.jdaDetectBatchSubmit.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_int, C.c_int, C.c_float,
                                         C.c_float, C.c_int, C.c_int, C.c_float, C.POINTER(jdaDetectOptions)]
    lib.jdaDetectBatchSubmitHost.argtypes = [C.c_void_p, C.POINTER(u8p), C.c_int, C.c_int, C.c_int, C.c_float,
                                             C.c_float, C.c_int, C.c_int, C.c_float, C.POINTER(jdaDetectOptions)]
    lib.jdaDetectBatchWait.argtypes = [C.c_void_p, C.c_int, C.POINTER(jdaStats), C.POINTER(jdaResult)]
    lib.jdaTraceBatch.argtypes = [C.c_void_p, C.POINTER(u8p), C.c_int, C.c_int, C.c_int, C.c_float, C.c_int, C.c_int,
                                  C.POINTER(C.c_int), C.POINTER(C.c_float), C.POINTER(C.c_uint), C.POINTER(C.c_float)]
    if hasattr(lib, "jdaValidateWindows"):          # (older builds, loaded through JDA_LIB_PATH for A/B runs, lack it)
        win_tail = [C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int), C.c_int, C.c_float, u8p, C.POINTER(C.c_float), C.POINTER(C.c_int),
                    C.POINTER(C.c_uint), C.POINTER(C.c_float), C.POINTER(C.c_float), C.POINTER(jdaStats)]
        lib.jdaValidateWindows.argtypes = [C.c_void_p, C.POINTER(u8p)] + win_tail
        lib.jdaValidateWindowsDevice.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t] + win_tail
    lib.jdaBuildPyramid.argtypes = [C.c_void_p, u8p, C.c_int, C.c_int, u8p, C.POINTER(C.c_int), C.POINTER(C.c_int),
                                    u8p, C.POINTER(C.c_int), C.POINTER(C.c_int)]
    lib.jdaResultDRelease.restype = None
    lib.jdaResultDRelease.argtypes = [jdaResultD]
    lib.jdaDetectBatchCpp.argtypes = [C.c_void_p, C.POINTER(u8p), C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                      C.c_double, C.c_double, C.c_int, C.POINTER(jdaStats), C.POINTER(jdaResultD)]
    if hasattr(lib, "jdaDetectBatchCppDevice"):     # (r06; older builds loaded through JDA_LIB_PATH lack them)
        lib.jdaDetectBatchCppDevice.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                                C.c_double, C.c_double, C.c_int, C.POINTER(jdaStats), C.POINTER(jdaResultD)]
        lib.jdaDetectBatchCppRagged.argtypes = [C.c_void_p, C.POINTER(u8p), C.POINTER(C.c_int), C.POINTER(C.c_int), C.c_int,
                                                C.c_int, C.c_int, C.c_double, C.c_double, C.c_int, C.POINTER(jdaStats),
                                                C.POINTER(jdaResultD)]
        lib.jdaDetectBatchCppRaggedDevice.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_size_t), C.POINTER(C.c_int),
                                                      C.POINTER(C.c_int), C.c_int, C.c_int, C.c_int, C.c_double, C.c_double,
                                                      C.c_int, C.POINTER(jdaStats), C.POINTER(jdaResultD)]
        lib.jdaResultsDRelease.restype = None
        lib.jdaResultsDRelease.argtypes = [C.POINTER(jdaResultD), C.c_int]
        lib.jdaResultsDPack.argtypes = [C.POINTER(jdaResultD), C.c_int, C.c_int, C.POINTER(C.c_double), C.c_int]
    lib.jdaDetectBatchCppPyramid.argtypes = [C.c_void_p, C.POINTER(u8p), C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                             C.c_double, C.c_double, C.c_int, C.POINTER(jdaStats), C.POINTER(jdaResultD)]
    if hasattr(lib, "jdaDetectBatchCppPyramidMS"):
        lib.jdaDetectBatchCppPyramidMS.argtypes = [C.c_void_p, C.POINTER(u8p), C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                                   C.c_double, C.c_double, C.c_int, C.POINTER(jdaStats), C.POINTER(jdaResultD)]
    lib.jdaResizeCv.argtypes = [C.c_void_p, u8p, C.c_int, C.c_int, u8p, C.c_int, C.c_int]
    lib.jdaSetSimilarityTransform.argtypes = [C.c_void_p, C.c_int]
    lib.jdaNmsC.argtypes = [C.POINTER(C.c_int), C.POINTER(C.c_float), C.c_int, C.c_float, u8p]
    lib.jdaNmsCpp.argtypes = [C.POINTER(C.c_int), C.POINTER(C.c_double), C.c_int, C.c_double, C.POINTER(C.c_int)]
    lib.jdaResultsRelease.restype = None
    lib.jdaResultsRelease.argtypes = [C.POINTER(jdaResult), C.c_int]
    lib.jdaResultsPack.argtypes = [C.POINTER(jdaResult), C.c_int, C.c_int, C.POINTER(C.c_float), C.c_int]
    lib.jdaModelStreamBytes.restype = C.c_longlong
    lib.jdaModelStreamBytes.argtypes = [C.c_int] * 5
    if hasattr(lib, "jdaTraceBatchCpp"):
        lib.jdaTraceBatchCpp.argtypes = [C.c_void_p, C.POINTER(u8p), C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                         C.c_double, C.POINTER(C.c_int), C.POINTER(C.c_double),
                                         C.POINTER(C.c_uint), C.POINTER(C.c_double)]
    if hasattr(lib, "jdaValidateCpp"):
        crop_tail = [C.POINTER(C.c_int), C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_double, C.c_uint64,
                     u8p, C.POINTER(C.c_double), C.POINTER(C.c_int), C.POINTER(C.c_double), C.POINTER(jdaStats)]
        lib.jdaValidateCpp.argtypes = [C.c_void_p, C.POINTER(u8p), C.POINTER(C.c_int), C.POINTER(C.c_int), C.c_int] + crop_tail
        lib.jdaValidateCppDevice.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_size_t), C.POINTER(C.c_int),
                                             C.POINTER(C.c_int), C.c_int] + crop_tail
        mine_tail = [C.POINTER(C.c_int), C.POINTER(C.c_double), C.POINTER(C.c_int), C.c_int, C.c_int, C.c_int, C.c_longlong,
                     C.c_int, C.c_double, C.c_uint64, C.POINTER(C.c_int), C.POINTER(C.c_double), C.POINTER(C.c_double), u8p,
                     C.POINTER(jdaMineStats)]
        lib.jdaMineNegativesCpp.argtypes = [C.c_void_p, C.POINTER(u8p), C.POINTER(C.c_int), C.POINTER(C.c_int), C.c_int] + mine_tail
        lib.jdaMineNegativesCppDevice.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_size_t), C.POINTER(C.c_int),
                                                  C.POINTER(C.c_int), C.c_int] + mine_tail
        lib.jdaMineWindows.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.c_double, C.POINTER(C.c_longlong), C.POINTER(C.c_int)]
        lib.jdaMineWindowList.restype = C.c_longlong
        lib.jdaMineWindowList.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.c_double, C.POINTER(C.c_int), C.c_longlong]
    if hasattr(lib, "jdaTrainCartCpp"):
        sp, fp, dp, ip = C.POINTER(jdaSamplesCpp), C.POINTER(jdaFeatureCpp), C.POINTER(C.c_double), C.POINTER(C.c_int)
        lib.jdaGenFeaturePoolCpp.argtypes = [C.c_int, C.c_int, C.c_double, C.c_int, C.c_uint64, C.c_uint64, fp, dp]
        lib.jdaCalcFeatureValuesCpp.argtypes = [C.c_void_p, sp, C.c_int, C.c_int, C.c_int, fp, C.c_int, ip]
        lib.jdaSplitNodeCpp.argtypes = [C.c_void_p, sp, sp, C.c_int, C.c_int, C.c_int, fp, C.c_int, C.c_int, dp, ip, ip, dp, ip]
        lib.jdaTrainCartCpp.argtypes = [C.c_void_p, sp, sp, C.c_int, C.c_int, C.c_int, fp, C.c_int, ip, dp, fp, ip, dp, ip, ip,
                                        C.POINTER(jdaTrainStatsCpp)]
    if hasattr(lib, "jdaSplitNodeSumsCpp"):
        lib.jdaSplitNodeSumsCpp.argtypes = [C.c_void_p, sp, sp, C.c_int, C.c_int, C.c_int, fp, C.c_int, C.c_int, dp, ip, C.c_int, ip,
                                            C.c_int, ip, ip, dp, ip, C.POINTER(jdaSplitSumsCpp)]
    if hasattr(lib, "jdaStageUpdateShapesCpp"):
        sp, dp, ip, cp = C.POINTER(jdaSamplesCpp), C.POINTER(C.c_double), C.POINTER(C.c_int), C.POINTER(jdaStageCartsCpp)
        lib.jdaGenLbfCpp.argtypes = [C.c_void_p, sp, C.c_int, C.c_int, C.c_int, cp, ip]
        lib.jdaStageUpdateShapesCpp.argtypes = [C.c_void_p, sp, C.c_int, C.c_int, C.c_int, cp, dp, ip, dp, ip,
                                                C.POINTER(jdaStageStatsCpp)]
        lib.jdaMeanErrorCpp.argtypes = [dp, dp, C.c_int, C.c_int, ip, C.c_int, ip, C.c_int, dp]
    if hasattr(lib, "jdaGlobalRegressionCpp"):
        dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int)
        lib.jdaGlobalRegressionCpp.argtypes = [C.c_void_p, ip, dp, C.c_int, C.c_int, ip, C.c_int, C.POINTER(jdaFitParamsCpp), dp, ip, dp,
                                               C.POINTER(jdaFitStatsCpp)]
        lib.jdaFitShuffleCpp.argtypes = [ip, C.c_int, C.c_uint64, C.c_int]
    if hasattr(lib, "jdaGatherSamplesCpp"):
        dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int)
        lib.jdaBoostScoresCpp.argtypes = [dp, C.c_int, ip, C.c_int, ip, C.c_int, C.c_int, dp, dp, dp, dp, dp, dp]
        lib.jdaSampleOrderCpp.argtypes = [dp, C.c_int, ip, dp]
        lib.jdaScoreThresholdCpp.argtypes = [dp, C.c_int, C.c_int, dp]
        lib.jdaScoreCutCpp.argtypes = [dp, C.c_int, C.c_double, ip, ip]
        lib.jdaUpdateWeightsCpp.argtypes = [dp, C.c_int, dp, C.c_int, dp, dp]
        lib.jdaGatherRowsCpp.argtypes = [C.POINTER(C.c_void_p), ip, C.c_int, C.c_size_t, ip, C.c_int, C.c_void_p]
        lib.jdaGatherSamplesCpp.argtypes = [C.c_void_p, C.POINTER(jdaGatherSegCpp), C.c_int, C.c_int, C.c_int, C.c_int, ip, C.c_int,
                                            C.c_void_p, C.c_int, C.POINTER(jdaGatherStatsCpp)]
    if hasattr(lib, "jdaBuildPositivesCpp"):
        dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int)
        faces_tail = [ip, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.POINTER(jdaPositivesStatsCpp)]
        lib.jdaBuildPositivesCpp.argtypes = [C.c_void_p, C.POINTER(u8p), ip, ip, C.c_int] + faces_tail
        lib.jdaBuildPositivesCppDevice.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_size_t), ip, ip, C.c_int] + faces_tail
        lib.jdaPositiveShapesCpp.argtypes = [ip, dp, C.c_int, C.c_int, C.c_int, ip, ip, C.c_int, dp, ip, dp]
        lib.jdaRandomShapesCpp.argtypes = [dp, C.c_int, C.c_int, C.c_double, C.c_uint64, C.c_uint64, dp]
        lib.jdaShapeResidualCpp.argtypes = [dp, dp, ip, C.c_int, C.c_int, ip, C.c_int, C.c_int, dp, u8p]
    if hasattr(lib, "jdaCalcSTParametersCpp"):      # (older builds, loaded through JDA_LIB_PATH for A/B runs, lack them)
        dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int)
        lib.jdaCalcSTParametersCpp.argtypes = [C.c_void_p, dp, C.c_int, dp, dp]
        lib.jdaShapeResidualStCpp.argtypes = [dp, dp, ip, C.c_int, C.c_int, ip, C.c_int, C.c_int, dp, dp, u8p]
    if hasattr(lib, "jdaModelPutCartCpp"):
        dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int)
        lib.jdaCascadorCreateTrainingCpp.restype = C.c_void_p
        lib.jdaCascadorCreateTrainingCpp.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, dp]
        lib.jdaModelStatusCpp.argtypes = [C.c_void_p, ip, ip]
        lib.jdaModelPutCartCpp.argtypes = [C.c_void_p, C.c_int, C.POINTER(jdaFeatureCpp), ip, dp, C.c_double, C.c_double, C.c_double]
        lib.jdaModelCloseStageCpp.argtypes = [C.c_void_p, dp]
        lib.jdaCascadorSerializeToCpp.argtypes = [C.c_void_p, C.c_char_p]
    if hasattr(lib, "jdaValidateSamplesCpp"):
        dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int)
        lib.jdaValidateSamplesCpp.argtypes = [C.c_void_p, C.POINTER(jdaSamplesCpp), C.c_int, C.c_int, C.c_int, u8p, dp, ip, dp,
                                              C.POINTER(jdaStageStatsCpp)]
    if hasattr(lib, "jdaPackGrayDevice"):           # (older builds, loaded through JDA_LIB_PATH for A/B runs, lack them)
        lib.jdaPackGray.argtypes = [C.POINTER(jdaPixels), C.c_int, C.c_void_p, C.POINTER(C.c_size_t)]
        lib.jdaPackGrayDevice.argtypes = [C.c_void_p, C.POINTER(jdaPixels), C.c_int, C.c_void_p, C.POINTER(C.c_size_t), C.c_void_p,
                                          C.POINTER(jdaPackStats)]
    if hasattr(lib, "jdaFaceChipsDevice"):
        chips = [C.POINTER(jdaPixels), C.c_int, C.POINTER(C.c_int), C.c_void_p, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_double),
                 C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.POINTER(C.c_double)]
        lib.jdaFaceChips.argtypes = chips
        lib.jdaFaceChipsDevice.argtypes = [C.c_void_p] + chips + [C.c_void_p, C.POINTER(jdaChipStats)]
        lib.jdaCascadorMeanShape.argtypes = [C.c_void_p, C.POINTER(C.c_double)]
    if hasattr(lib, "jdaPackGrayOrientedDevice"):
        ip = C.POINTER(C.c_int)
        lib.jdaOrientSize.argtypes = [C.c_int, C.c_int, C.c_int, ip, ip]
        lib.jdaPackGrayOriented.argtypes = [C.POINTER(jdaPixels), ip, C.c_int, C.c_void_p, C.POINTER(C.c_size_t)]
        lib.jdaPackGrayOrientedDevice.argtypes = [C.c_void_p, C.POINTER(jdaPixels), ip, C.c_int, C.c_void_p, C.POINTER(C.c_size_t),
                                                  C.c_void_p, C.POINTER(jdaPackStats)]
        lib.jdaOrientBack.argtypes = [C.POINTER(jdaPixels), ip, C.c_int, ip, C.c_int, ip, C.c_int, C.c_void_p, C.c_int, C.c_int, ip, ip,
                                      C.c_int]
    if hasattr(lib, "jdaPackGrayReducedDevice"):
        ip = C.POINTER(C.c_int)
        lib.jdaReduceSize.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, ip, ip]
        lib.jdaPackGrayReduced.argtypes = [C.POINTER(jdaPixels), ip, ip, C.c_int, C.c_void_p, C.POINTER(C.c_size_t)]
        lib.jdaPackGrayReducedDevice.argtypes = [C.c_void_p, C.POINTER(jdaPixels), ip, ip, C.c_int, C.c_void_p, C.POINTER(C.c_size_t),
                                                 C.c_void_p, C.POINTER(jdaPackStats)]
        lib.jdaReduceBack.argtypes = [C.POINTER(jdaPixels), ip, ip, C.c_int, ip, C.c_int, ip, C.c_int, C.c_void_p, C.c_int, C.c_int, ip,
                                      ip, C.c_int]
    if hasattr(lib, "jdaPackGrayRotatedDevice"):
        ip, dp = C.POINTER(C.c_int), C.POINTER(C.c_double)
        lib.jdaRotationPlan.argtypes = [C.c_int, C.c_int, C.c_double, C.POINTER(jdaRotation)]
        lib.jdaPackGrayRotated.argtypes = [C.POINTER(jdaPixels), dp, C.c_int, C.c_void_p, C.POINTER(C.c_size_t)]
        lib.jdaPackGrayRotatedDevice.argtypes = [C.c_void_p, C.POINTER(jdaPixels), dp, C.c_int, C.c_void_p, C.POINTER(C.c_size_t), C.c_void_p,
                                                 C.POINTER(jdaPackStats)]
        lib.jdaRotateBack.argtypes = [C.POINTER(jdaPixels), dp, C.c_int, ip, C.c_int, ip, C.c_int, C.c_void_p, C.c_int, C.c_int]
    return lib


lib = _load()

# reference-named entry points, callable exactly like the C functions
jdaCascadorCreateDouble = lib.jdaCascadorCreateDouble
jdaCascadorCreateFloat = lib.jdaCascadorCreateFloat
jdaCascadorCreate = lib.jdaCascadorCreate
jdaCascadorSerializeTo = lib.jdaCascadorSerializeTo
jdaCascadorRelease = lib.jdaCascadorRelease
jdaDetect = lib.jdaDetect
jdaResultRelease = lib.jdaResultRelease


def last_error():
    return (lib.jdaGetLastError() or b"").decode()


def mine_windows(width, height, origin_size, step, factor, listing=False):
    """The mining enumeration of one (transformed) image, NextImage's walk (jdaMineWindows): (windows, levels), or with
    listing=True an [n, 3] int32 array of (x, y, win) in enumeration order."""
    if not listing:
        n, nl = C.c_longlong(), C.c_int()
        if lib.jdaMineWindows(width, height, origin_size, step, factor, C.byref(n), C.byref(nl)) != 0:
            raise JdaError(last_error())
        return n.value, nl.value
    n = lib.jdaMineWindowList(width, height, origin_size, step, factor, None, 0)
    if n < 0:
        raise JdaError(last_error())
    out = np.zeros((max(n, 1), 3), np.int32)
    lib.jdaMineWindowList(width, height, origin_size, step, factor, out.ctypes.data_as(C.POINTER(C.c_int)), n)
    return out[:n]


def mine_params(n_images, quarter_size=24, seed=0):
    """Per-image step in [2, quarter_size) and factor in [1.1, 1.5), drawn the way NegGenerator's Load / NextImage draw
    them (reference data.cpp:910-911, 1093-1094: rng.uniform(2, img_q_size), rng.uniform(1.1, 1.5)) -- with numpy's seeded
    generator instead of cv::RNG(getTickCount()).  Returns (steps int32, factors float64)."""
    rng = np.random.default_rng(seed)
    steps = rng.integers(2, quarter_size, size=n_images).astype(np.int32)
    factors = rng.uniform(1.1, 1.5, size=n_images)
    return steps, factors


def gen_feature_pool_cpp(F, landmark_n, radius, multi_scale=False, seed=0, key=0):
    """Cart::GenFeaturePool (reference cart.cpp:352-390) on the counter-based generator of include/jda.h
    (jdaGenFeaturePoolCpp, host only) -> (features [F] of FEATURE_DTYPE, u [F] the regression draws)."""
    feats = np.zeros(max(int(F), 1), FEATURE_DTYPE)
    u = np.zeros(max(int(F), 1), np.float64)
    if lib.jdaGenFeaturePoolCpp(int(F), int(landmark_n), float(radius), 1 if multi_scale else 0, int(seed) & 0xffffffffffffffff,
                                int(key) & 0xffffffffffffffff, feats.ctypes.data_as(C.POINTER(jdaFeatureCpp)),
                                u.ctypes.data_as(C.POINTER(C.c_double))) != 0:
        raise JdaError(last_error())
    return feats[:F], u[:F]


def mean_error_cpp(gt_shapes, cur_shapes, left_pupils, right_pupils):
    """calcMeanError (reference common.cpp:41-77), the "Regression Mean Error" a stage reports, in the reference's own
    summation order (jdaMeanErrorCpp, host only).  gt_shapes / cur_shapes: [n, 2L]; the pupil lists are landmark ids."""
    gt = np.ascontiguousarray(gt_shapes, np.float64)
    cur = np.ascontiguousarray(cur_shapes, np.float64)
    assert gt.ndim == 2 and gt.shape == cur.shape and gt.shape[1] % 2 == 0
    kl, lp = _ivec(left_pupils)
    kr, rp = _ivec(right_pupils)
    out = C.c_double()
    dp = C.POINTER(C.c_double)
    if lib.jdaMeanErrorCpp(gt.ctypes.data_as(dp), cur.ctypes.data_as(dp), gt.shape[0], gt.shape[1] // 2, lp, int(np.asarray(left_pupils).size), rp,
                           int(np.asarray(right_pupils).size),
                           C.byref(out)) != 0:
        raise JdaError(last_error())
    return out.value


def fit_shuffle_cpp(index, seed, iter):
    """One epoch's shuffle of the global regression's sample order (jdaFitShuffleCpp, host only): index (int32, any
    length) -> a new array, the epoch-`iter` permutation step of include/jda.h applied to it.  Epochs chain: feed the
    result of epoch iter - 1 in."""
    a = np.array(index, np.int32).reshape(-1)
    if lib.jdaFitShuffleCpp(a.ctypes.data_as(C.POINTER(C.c_int)) if a.size else None, int(a.size), int(seed) & 0xffffffffffffffff,
                            int(iter)) != 0:
        raise JdaError(last_error())
    return a


# -- from one cart to the next (include/jda.h, "Dialect CPP: from one cart to the next"): host only, no cascador ----

def _dvec(a):
    a = np.ascontiguousarray(a, np.float64).reshape(-1)
    return a, (a.ctypes.data_as(C.POINTER(C.c_double)) if a.size else None)


def boost_scores_cpp(cart_scores, pos_leaf, neg_leaf, pos_scores, neg_scores, normalize=False):
    """DataSet::UpdateScores for both sets and, with normalize, CalcMeanAndStd / ApplyMeanAndStd (reference data.cpp:305-317,
    420-448; jdaBoostScoresCpp) -> dict(pos_scores, neg_scores, pos_last, neg_last, mean, std).  The inputs are not changed.
    The sums run over the order the arrays have now, before the sort."""
    cs, csp = _dvec(cart_scores)
    kp, pl = _ivec(pos_leaf)
    kn, nl = _ivec(neg_leaf)
    ps, psp = _dvec(np.array(pos_scores, np.float64))
    ns, nsp = _dvec(np.array(neg_scores, np.float64))
    assert ps.size == np.asarray(pos_leaf).size and ns.size == np.asarray(neg_leaf).size, "one leaf per sample"
    plast, plp = _dvec(np.zeros(ps.size))
    nlast, nlp = _dvec(np.zeros(ns.size))
    mean, std = C.c_double(), C.c_double()
    if lib.jdaBoostScoresCpp(csp, cs.size, pl if ps.size else None, ps.size, nl if ns.size else None, ns.size, 1 if normalize else 0,
                             psp, nsp, plp, nlp, C.byref(mean), C.byref(std)) != 0:
        raise JdaError(last_error())
    return dict(pos_scores=ps, neg_scores=ns, pos_last=plast, neg_last=nlast, mean=mean.value, std=std.value)


def sample_order_cpp(scores):
    """DataSet::_QSort_ (reference data.cpp:385-410; jdaSampleOrderCpp) on one set's scores -> (order int32 [n], sorted
    scores [n]): order[i] is the original index of the sample now at position i.  Not a stable sort; NaN is refused."""
    sc, scp = _dvec(scores)
    order = np.zeros(sc.size, np.int32)
    out = np.zeros(sc.size, np.float64)
    if lib.jdaSampleOrderCpp(scp, sc.size, order.ctypes.data_as(C.POINTER(C.c_int)), out.ctypes.data_as(C.POINTER(C.c_double))) != 0:
        raise JdaError(last_error())
    return order, out


def score_threshold_cpp(sorted_scores, drop_n):
    """DataSet::CalcThresholdByNumber (reference data.cpp:340-345; jdaScoreThresholdCpp) on sorted scores -> th."""
    sc, scp = _dvec(sorted_scores)
    th = C.c_double()
    if lib.jdaScoreThresholdCpp(scp, sc.size, int(drop_n), C.byref(th)) != 0:
        raise JdaError(last_error())
    return th.value


def score_cut_cpp(sorted_scores, th):
    """DataSet::PreRemove / Remove (reference data.cpp:347-378; jdaScoreCutCpp) on sorted scores -> (keep, will_removed)."""
    sc, scp = _dvec(sorted_scores)
    keep, gone = C.c_int(), C.c_int()
    if lib.jdaScoreCutCpp(scp, sc.size, float(th), C.byref(keep), C.byref(gone)) != 0:
        raise JdaError(last_error())
    return keep.value, gone.value


def update_weights_cpp(pos_scores, neg_scores):
    """DataSet::UpdateWeights(pos, neg) (reference data.cpp:255-303; jdaUpdateWeightsCpp) with the host C library's exp ->
    (pos_weights, neg_weights)."""
    ps, psp = _dvec(pos_scores)
    ns, nsp = _dvec(neg_scores)
    pw, pwp = _dvec(np.zeros(ps.size))
    nw, nwp = _dvec(np.zeros(ns.size))
    if lib.jdaUpdateWeightsCpp(psp, ps.size, nsp, ns.size, pwp, nwp) != 0:
        raise JdaError(last_error())
    return pw, nw


def gather_rows_cpp(rows, index, keep=None):
    """The per-sample rows that travel with the patches (jdaGatherRowsCpp, host only): rows is one array [n, ...] or a list
    of up to 8 of them with equal row shape and dtype (their concatenation is the source); -> [keep, ...] with row i the
    source row index[i]."""
    segs = [np.ascontiguousarray(a) for a in (rows if isinstance(rows, (list, tuple)) else [rows])]
    assert segs and all(a.ndim >= 1 and a.shape[1:] == segs[0].shape[1:] and a.dtype == segs[0].dtype for a in segs)
    idx = np.ascontiguousarray(index, np.int32).reshape(-1)
    keep = idx.size if keep is None else int(keep)
    assert keep <= idx.size
    row_bytes = int(np.prod(segs[0].shape[1:], dtype=np.int64)) * segs[0].dtype.itemsize
    out = np.zeros((max(keep, 0),) + segs[0].shape[1:], segs[0].dtype)
    ptrs = (C.c_void_p * len(segs))(*[a.ctypes.data if a.size else None for a in segs])
    ns = (C.c_int * len(segs))(*[a.shape[0] for a in segs])
    if lib.jdaGatherRowsCpp(ptrs, ns, len(segs), row_bytes, idx.ctypes.data_as(C.POINTER(C.c_int)) if idx.size else None, keep,
                            out.ctypes.data if out.size else None) != 0:
        raise JdaError(last_error())
    return out


# -- the positive sample set (include/jda.h, "Dialect CPP: the positive sample set"): host only, no cascador ----

def positive_shapes_cpp(faces, landmarks, augment=False, left=(), right=()):
    """Ground-truth shapes, masks and the mean shape of the positive set (reference data.cpp:589-598, 625-628, 641-661,
    CalcMeanShape 210-223; jdaPositiveShapesCpp).  faces: [n, 5] rows of (image, x, y, w, h); landmarks: [n, 2L] in image
    coordinates; left / right: the symmetric pairs.  -> dict(gt_shapes [size, 2L], shape_mask [size] int32, mean_shape [2L]),
    size = 2 n with augment.  CalcMeanShape's quirk is kept: sample 0 is summed whatever its mask and not counted."""
    fa = np.ascontiguousarray(np.asarray(faces, np.int32).reshape(-1, 5))
    n = fa.shape[0]
    lm = np.ascontiguousarray(landmarks, np.float64).reshape(n, -1) if n else np.zeros((0, 2), np.float64)
    assert lm.shape[1] % 2 == 0 and lm.shape[1] > 0, "landmarks must be [n, 2L]"
    L = lm.shape[1] // 2
    kl, lp = _ivec(left)
    kr, rp = _ivec(right)
    sym_n = int(np.asarray(left).size)
    assert sym_n == int(np.asarray(right).size), "left and right must pair up"
    size = 2 * n if augment else n
    gt = np.zeros((max(size, 1), 2 * L), np.float64)
    mask = np.zeros(max(size, 1), np.int32)
    mean = np.zeros(2 * L, np.float64)
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int)
    if lib.jdaPositiveShapesCpp(fa.ctypes.data_as(ip) if n else None, lm.ctypes.data_as(dp) if n else None, n, L, 1 if augment else 0,
                                lp if sym_n else None, rp if sym_n else None, sym_n, gt.ctypes.data_as(dp), mask.ctypes.data_as(ip),
                                mean.ctypes.data_as(dp)) != 0:
        raise JdaError(last_error())
    return dict(gt_shapes=gt[:size], shape_mask=mask[:size], mean_shape=mean)


def random_shapes_cpp(mean_shape, n, shift_size=0.0, seed=0, first_key=0):
    """DataSet::RandomShapes (reference data.cpp:237-253; jdaRandomShapesCpp) on include/jda.h's counter-based generator:
    [n, 2L] initial shapes, sample i drawing with key first_key + i (a set built in pieces equals one built at once)."""
    ms, msp = _dvec(mean_shape)
    assert ms.size % 2 == 0 and ms.size > 0
    out = np.zeros((max(int(n), 1), ms.size), np.float64)
    if lib.jdaRandomShapesCpp(msp, ms.size // 2, int(n), float(shift_size), int(seed) & 0xffffffffffffffff,
                              int(first_key) & 0xffffffffffffffff, out.ctypes.data_as(C.POINTER(C.c_double))) != 0:
        raise JdaError(last_error())
    return out[:max(int(n), 0)]


def shape_residual_cpp(gt_shapes, cur_shapes, idx=None, landmark_id=None, shape_mask=None, stp_cm=None):
    """DataSet::CalcShapeResidual (reference data.cpp:175-208; jdaShapeResidualCpp): gt - current over the index list
    (default: every sample) -- [n, 2L] for all landmarks, [n, 2] for one landmark_id (what a sample set's "residual"
    takes).  With shape_mask also has_gt [n] uint8 (DataSet::HasGtShape): -> (residual, has_gt).  stp_cm ([size, 5],
    Cascador.calc_st_parameters_cpp's): row idx[i] is applied to sample i's residual (jdaShapeResidualStCpp); None: the
    identity transform."""
    gt = np.ascontiguousarray(gt_shapes, np.float64)
    cur = np.ascontiguousarray(cur_shapes, np.float64)
    assert gt.ndim == 2 and gt.shape == cur.shape and gt.shape[1] % 2 == 0 and gt.shape[1] > 0
    size, L = gt.shape[0], gt.shape[1] // 2
    ix = np.ascontiguousarray(np.arange(size) if idx is None else idx, np.int32).reshape(-1)
    lid = -1 if landmark_id is None else int(landmark_id)
    out = np.zeros((max(ix.size, 1), 2 * L if landmark_id is None else 2), np.float64)
    mk = None if shape_mask is None else np.ascontiguousarray(shape_mask, np.int32).reshape(-1)
    assert mk is None or mk.size == size
    hg = None if mk is None else np.zeros(max(ix.size, 1), np.uint8)
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int)
    head = (gt.ctypes.data_as(dp), cur.ctypes.data_as(dp), None if mk is None else mk.ctypes.data_as(ip), size, L,
            ix.ctypes.data_as(ip) if ix.size else None, ix.size, lid)
    tail = (out.ctypes.data_as(dp), None if hg is None else _u8(hg))
    if stp_cm is None:
        rc = lib.jdaShapeResidualCpp(*head, *tail)
    else:
        cm = np.ascontiguousarray(stp_cm, np.float64)
        assert cm.shape == (size, 5), "stp_cm must be [size, 5]"
        rc = lib.jdaShapeResidualStCpp(*head, cm.ctypes.data_as(dp), *tail)
    if rc != 0:
        raise JdaError(last_error())
    return out[:ix.size] if mk is None else (out[:ix.size], hg[:ix.size])


def _byte_buffer(a, what):
    """A numpy uint8 array or a torch uint8 device tensor (any view with a byte offset: its data pointer is what counts) ->
    (pointer, on_device, bytes)."""
    if hasattr(a, "is_cuda"):
        assert a.is_cuda and a.dtype.itemsize == 1 and a.is_contiguous(), "%s: a contiguous uint8 device tensor" % what
        return (a.data_ptr() if a.numel() else None), 1, a.numel()
    assert isinstance(a, np.ndarray) and a.dtype == np.uint8 and a.flags.c_contiguous, "%s: a contiguous uint8 array" % what
    return (a.ctypes.data if a.size else None), 0, a.size


def _stage_carts(features, thresholds, inner, K=None):
    """A stage's carts -- features [K, nodes_n/2 - 1] of FEATURE_DTYPE and thresholds, the outputs of K train_cart_cpp
    calls stacked -- as a jdaStageCartsCpp (and what keeps its arrays alive)."""
    c = jdaStageCartsCpp()
    if features is None:
        c.K = int(K)
        return c, []
    fa, fp = _features(features)
    th = np.ascontiguousarray(thresholds, np.int32).reshape(-1)
    assert len(fa) == th.size, "one threshold per split node"
    if inner > 0:
        assert len(fa) % inner == 0, "carts must hold K * (nodes_n/2 - 1) split nodes"
        c.K = len(fa) // inner
        c.features, c.thresholds = fp, th.ctypes.data_as(C.POINTER(C.c_int))
    else:
        c.K = int(K)
    return c, [fa, th]


def _patch_bytes(origin_size, half_size, quarter_size):
    """Bytes of one sample's o, h, q patches back to back (jdaSamplesCpp's layout)."""
    return origin_size * origin_size + half_size * half_size + quarter_size * quarter_size


def _features(pool):
    a = np.ascontiguousarray(pool, FEATURE_DTYPE).reshape(-1)
    return a, a.ctypes.data_as(C.POINTER(jdaFeatureCpp))


def _samples(samples, dim, pbytes):
    """dict(patches=[n, pbytes] uint8 numpy array or torch CUDA tensor, shapes=[n, 2L], weights=[n], residual=[n, 2] or
    None, has_gt=[n] or None) -> (jdaSamplesCpp, keep-alive)."""
    pa = samples["patches"]
    sh = np.ascontiguousarray(samples["shapes"], np.float64).reshape(-1, dim)
    n = sh.shape[0]
    s = jdaSamplesCpp()
    keep = [sh]
    if hasattr(pa, "is_cuda"):
        assert pa.is_cuda and pa.dtype.itemsize == 1 and pa.is_contiguous() and pa.numel() == n * pbytes
        s.patches, s.patches_on_device = pa.data_ptr() if n else None, 1
    else:
        pa = np.ascontiguousarray(pa, np.uint8)
        assert pa.size == n * pbytes, "patches must hold n * (o*o + h*h + q*q) bytes"
        s.patches, s.patches_on_device = pa.ctypes.data if n else None, 0
    keep.append(pa)
    dp = C.POINTER(C.c_double)
    s.shapes = sh.ctypes.data_as(dp)
    if samples.get("weights") is not None:
        w = np.ascontiguousarray(samples["weights"], np.float64).reshape(-1)
        assert w.size == n
        s.weights = w.ctypes.data_as(dp); keep.append(w)
    if samples.get("residual") is not None:
        r = np.ascontiguousarray(samples["residual"], np.float64).reshape(-1)
        assert r.size == 2 * n
        s.residual = r.ctypes.data_as(dp); keep.append(r)
    if samples.get("has_gt") is not None:
        g = np.ascontiguousarray(samples["has_gt"], np.uint8).reshape(-1)
        assert g.size == n
        s.has_gt = g.ctypes.data_as(C.POINTER(C.c_ubyte)); keep.append(g)
    s.n = n
    return s, keep


def _image_set(images):
    """A list of 2-D uint8 arrays (host) or (torch uint8 CUDA buffer, offsets, widths, heights) (device) ->
    (device?, base or pointer array, offsets or None, widths, heights, keep-alive)."""
    if isinstance(images, tuple):
        buf, offsets, widths, heights = images
        assert buf.is_cuda and buf.dtype.itemsize == 1 and buf.is_contiguous()
        ko, offs = _ivec(offsets, C.c_size_t, np.uint64)
        kw, ws = _ivec(widths)
        kh, hs = _ivec(heights)
        return True, C.c_void_p(buf.data_ptr()), offs, ws, hs, len(offsets), (ko, kw, kh, buf)
    imgs = [np.ascontiguousarray(a, np.uint8) for a in images]
    ptrs = (C.c_void_p * max(len(imgs), 1))(*[a.ctypes.data for a in imgs])
    kw, ws = _ivec([a.shape[1] for a in imgs])
    kh, hs = _ivec([a.shape[0] for a in imgs])
    return False, C.cast(ptrs, C.POINTER(C.POINTER(C.c_ubyte))), None, ws, hs, len(imgs), (imgs, ptrs, kw, kh)


def _pack_images_device(images):
    """A list of host images -> _image_set's device form: one torch CUDA buffer, every image at a 256-byte aligned offset."""
    import torch
    imgs = [np.ascontiguousarray(a, np.uint8) for a in images]
    offs = np.zeros(len(imgs), np.uint64)
    tot = 0
    for i, a in enumerate(imgs):
        offs[i] = tot
        tot += (a.size + 255) // 256 * 256
    host = np.zeros(max(tot, 256), np.uint8)
    for i, a in enumerate(imgs):
        host[int(offs[i]):int(offs[i]) + a.size] = a.ravel()
    return torch.from_numpy(host).cuda(), offs, [a.shape[1] for a in imgs], [a.shape[0] for a in imgs]


def _pixel_format(f):
    return PIX_FORMATS[f.lower()] if isinstance(f, str) else int(f)


def _pixel_table(images, formats, rects, address, strides):
    """jdaPixels[n] for arrays / tensors of shape [H, W, C] or [H, W] (strides in BYTES; a view's row stride is the pitch)
    and the (w, h) every image's rectangle comes out as.  What the library refuses is left to it; only what a jdaPixels
    cannot say is refused here: pixels whose bytes do not lie back to back inside a row."""
    n = len(images)
    if isinstance(formats, (str, int)):
        formats = [formats] * n
    if len(formats) != n or (rects is not None and len(rects) != n):
        raise ValueError("pack_gray: one format (and one rectangle) per image")
    px = (jdaPixels * max(n, 1))()
    sizes = []
    for i, im in enumerate(images):
        f = _pixel_format(formats[i])
        st, shape = strides(im), tuple(im.shape)
        chans = shape[2] if len(shape) == 3 else 1
        if len(shape) not in (2, 3) or chans != PIX_BYTES.get(f, chans):
            raise ValueError("pack_gray: image %d has shape %s, format %d needs [H, W%s]" % (i, shape, f, ", %d" % PIX_BYTES[f] if PIX_BYTES[f] > 1 else ""))
        if (len(shape) == 3 and chans > 1 and st[2] != 1) or (shape[1] > 1 and st[1] != chans) or (shape[0] > 1 and st[0] < 0):
            raise ValueError("pack_gray: image %d: a pixel's bytes and a row's pixels must lie back to back (strides %s)" % (i, st))
        r = (0, 0, 0, 0) if rects is None or rects[i] is None else tuple(int(v) for v in rects[i])
        pitch = st[0] if shape[0] > 1 else shape[1] * chans
        px[i] = jdaPixels(address(im), pitch, shape[1], shape[0], f, *r)
        sizes.append((shape[1], shape[0]) if r[2] == 0 and r[3] == 0 else (r[2], r[3]))
    return px, sizes


def _pixels(who, images, formats, rects, device):
    """What every pack / chips call does with its images first: numpy uint8 arrays (device: torch uint8 CUDA tensors), or a
    ValueError in the caller's name -> (the images as a list, their jdaPixels table, the (w, h) of their rectangles)."""
    if device:
        import torch
        images = list(images)
        ok = all(im.is_cuda and im.dtype == torch.uint8 for im in images)
        address, strides = (lambda t: t.data_ptr()), (lambda t: tuple(t.stride()))
    else:
        images = [np.asarray(im) for im in images]
        ok = all(im.dtype == np.uint8 for im in images)
        address, strides = (lambda a: a.ctypes.data), (lambda a: a.strides)
    if not ok:
        raise ValueError("%s: %s" % (who, "torch uint8 CUDA tensors" if device else "uint8 images"))
    return (images,) + _pixel_table(images, formats, rects, address, strides)


def _offsets(sizes, align=1, frame_stride=None):
    """Where images of the given (w, h) start in one destination, uint64 [max(n, 1)], and the bytes of it: back to back, each
    at a multiple of align, or -- with frame_stride -- image i at i * frame_stride."""
    offs = np.zeros(max(len(sizes), 1), np.uint64)
    tot = 0
    for i, (w, h) in enumerate(sizes):
        offs[i] = tot if frame_stride is None else i * int(frame_stride)
        tot = int(offs[i]) + (w * h if frame_stride is None else max(w * h, int(frame_stride)))
        if frame_stride is None:
            tot = (tot + align - 1) // align * align
    return offs, tot


def _device_buffer(buf, tot, images):
    """The destination of a device call: the caller's own (checked), or a new one of tot bytes on the images' device."""
    import torch
    if buf is None:
        return torch.empty(max(tot, 1), dtype=torch.uint8, device=images[0].device if images else "cuda")
    assert buf.is_cuda and buf.dtype == torch.uint8 and buf.is_contiguous()
    return buf


# the entries of each kind of frame call: host form, device form, way back (include/jda.h)
FRAME_ENTRIES = {"pack": ("jdaPackGray", "jdaPackGrayDevice", None),
                 "turn": ("jdaPackGrayOriented", "jdaPackGrayOrientedDevice", "jdaOrientBack"),
                 "reduce": ("jdaPackGrayReduced", "jdaPackGrayReducedDevice", "jdaReduceBack"),
                 "rotate": ("jdaPackGrayRotated", "jdaPackGrayRotatedDevice", "jdaRotateBack")}


def _frame_call(sizes, orients, factors, degrees, n):
    """How a frame call transforms its n images (each: one value for all images or one per image; None: not given) -> (the
    entries of its kind, the kind's arrays as those entries take them behind the images, the (w, h) rectangles of the given
    sizes come out as).  degrees: rotated; else factors: reduced (orients None: upright); else orients: turned; else packed."""
    o = None if orients is None else _orients(orients, n)
    f = None if factors is None else _factors(factors, n)
    g = None if degrees is None else _degrees(degrees, n)
    kind = "rotate" if g is not None else "reduce" if f is not None else "pack" if o is None else "turn"
    arrays = {"pack": (), "turn": (o,), "reduce": (f, o), "rotate": (g,)}[kind]
    ptrs = tuple(None if a is None else a.ctypes.data_as(C.POINTER(C.c_double if a.dtype == np.float64 else C.c_int)) for a in arrays)
    return FRAME_ENTRIES[kind], ptrs, _rotated_sizes(_turned_sizes(_reduced_sizes(sizes, f), o), g)


def _pack_gray(who, images, formats, orients, rects, factors=None, degrees=None):
    """pack_gray (orients None), pack_gray_oriented, with factors pack_gray_reduced and, with degrees, pack_gray_rotated."""
    images, px, sizes = _pixels(who, images, formats, rects, False)
    n = len(images)
    (host, _, _), arrays, sizes = _frame_call(sizes, orients, factors, degrees, n)
    offs, tot = _offsets(sizes)
    dst = np.empty(max(tot, 1), np.uint8)
    rc = getattr(lib, host)(px, *arrays, n, dst.ctypes.data, offs.ctypes.data_as(C.POINTER(C.c_size_t)))
    if rc != 0:
        raise JdaError(last_error())
    return [dst[int(offs[i]):int(offs[i]) + w * h].reshape(h, w) for i, (w, h) in enumerate(sizes)]


def pack_gray(images, formats, rects=None):
    """jdaPackGray: numpy uint8 arrays [H, W, C] or [H, W] (row-strided views allowed) of the given formats ("bgr24", ... or
    JDA_PIX_*; one for all or one per image), each cut to its rectangle (x, y, w, h) (None: the whole image) -> a list of
    uint8 [h, w] gray arrays.  Host only: no cascador, no GPU."""
    return _pack_gray("pack_gray", images, formats, None, rects)


# ---- frames in any orientation (include/jda.h) ------------------------------------------------------------------------------
EXIF_ORIENT = {1: 0, 2: 4, 3: 2, 4: 6, 5: 7, 6: 1, 7: 5, 8: 3}


def orient_from_exif(tag):
    """The orientation code t that turns the STORED image into the image as it should be displayed, for an EXIF Orientation
    tag 1..8 (include/jda.h, "frames in any orientation")."""
    if int(tag) not in EXIF_ORIENT:
        raise ValueError("orient_from_exif: EXIF Orientation is 1..8, not %r" % (tag,))
    return EXIF_ORIENT[int(tag)]


def orient_size(w, h, orient):
    """jdaOrientSize: (W', H') of a w x h rectangle turned by orient."""
    tw, th = C.c_int(), C.c_int()
    if lib.jdaOrientSize(int(w), int(h), int(orient), C.byref(tw), C.byref(th)) != 0:
        raise JdaError(last_error())
    return tw.value, th.value


def _orients(orients, n):
    """One orientation for all images or one per image -> int32 [max(n, 1)]."""
    o = np.full(n, int(orients), np.int32) if np.ndim(orients) == 0 else np.ascontiguousarray(orients, np.int32).reshape(-1)
    if len(o) != n:
        raise ValueError("orients: one orientation for all images or one per image")
    return o if n else np.zeros(1, np.int32)


def _turned_sizes(sizes, orients):
    """The (w, h) of rectangles turned by their orientations (None: none is); odd codes swap."""
    return [(max(h, 0), max(w, 0)) if int(t) & 1 else (max(w, 0), max(h, 0)) for (w, h), t in zip(sizes, [0] * len(sizes) if orients is None else orients)]


def pack_gray_oriented(images, formats, orients, rects=None):
    """jdaPackGrayOriented: pack_gray with every image written turned by its orientation (0..7: one for all or one per image)
    -> a list of uint8 [H', W'] gray arrays.  Host only: no cascador, no GPU."""
    return _pack_gray("pack_gray_oriented", images, formats, orients, rects)


def orient_back(images, formats, orients, faces, boxes=None, landmarks=None, rects=None, left=(), right=(), factors=None, degrees=None):
    """jdaOrientBack (with factors: jdaReduceBack, see reduce_back; with degrees: jdaRotateBack, see rotate_back): what a detect call found on images TURNED by orients (pack_gray_oriented[_device]) -> the coordinates of
    the whole source images.  images / formats / rects as the pack call got them (numpy arrays or torch tensors: only their
    shapes are read).  Either faces = the image index of every face with boxes (int [n, 3] (x, y, size) or [n, 4]
    (x, y, w, h), or None) and landmarks (float32 / float64 [n, 2L], or None) -> (boxes, landmarks), new arrays; or faces = one
    detect result per image (a dict with "bboxes" or "rects", "scores", "shapes"; None: no face) -> a list of new dicts.
    left / right: the landmark pairs a mirroring orientation (4..7) exchanges."""
    images = list(images)
    tensor = bool(images) and hasattr(images[0], "data_ptr")
    px, _ = _pixel_table(images, formats, rects, (lambda t: t.data_ptr()) if tensor else (lambda a: np.asarray(a).ctypes.data),
                         (lambda t: tuple(int(v) * t.element_size() for v in t.stride())) if tensor else (lambda a: np.asarray(a).strides))
    n_img = len(images)
    if orients is None:
        raise TypeError("orient_back: orients is needed (one orientation for all images or one per image)")
    (_, _, back), arrays, _ = _frame_call([], orients, factors, degrees, n_img)
    results = boxes is None and landmarks is None and len(faces) == n_img and all(r is None or isinstance(r, dict) for r in faces)
    if results:
        key = ["bboxes" if r is not None and "bboxes" in r else "rects" for r in faces]
        full = [(i, r) for i, r in enumerate(faces) if r is not None and len(r["scores"])]
        fi = np.concatenate([np.full(len(r["scores"]), i, np.int32) for i, r in full]) if full else np.zeros(0, np.int32)
        boxes = np.concatenate([np.asarray(r[key[i]], np.int32) for i, r in full]) if full else np.zeros((0, 3), np.int32)
        landmarks = np.concatenate([np.asarray(r["shapes"]) for i, r in full]) if full else np.zeros((0, 2), np.float32)
    else:
        fi = np.asarray(faces, np.int32).reshape(-1)
    fi = np.ascontiguousarray(fi, np.int32)
    n = len(fi)
    b = None if boxes is None else np.array(boxes, np.int32).reshape(n, -1)
    lm = None if landmarks is None else np.asarray(landmarks)
    if lm is not None:
        lm = np.array(lm if lm.dtype in (np.float32, np.float64) else lm.astype(np.float64)).reshape(n, -1)
    le, ri = np.ascontiguousarray(left, np.int32).reshape(-1), np.ascontiguousarray(right, np.int32).reshape(-1)
    if len(le) != len(ri):
        raise ValueError("orient_back: left and right name the two landmarks of every pair")
    ip = C.POINTER(C.c_int)
    tail = (n_img, fi.ctypes.data_as(ip), n, None if b is None else b.ctypes.data_as(ip),
            b.shape[1] if b is not None else 0, None if lm is None else lm.ctypes.data,
            lm.dtype.itemsize if lm is not None else 0, lm.shape[1] // 2 if lm is not None else 0,
            le.ctypes.data_as(ip) if len(le) else None, ri.ctypes.data_as(ip) if len(le) else None, len(le))
    rc = getattr(lib, back)(px, *arrays, *(tail[:8] if degrees is not None else tail))   # (nothing mirrors a rotation: no pairs)
    if rc != 0:
        raise JdaError(last_error())
    if not results:
        return b, lm
    out, at = [], 0
    for i, r in enumerate(faces):
        if r is None:
            out.append(None)
            continue
        m = len(r["scores"])
        d = dict(r)
        d[key[i]], d["shapes"], d["scores"] = b[at:at + m].copy(), lm[at:at + m].copy(), np.array(r["scores"])
        out.append(d)
        at += m
    return out


# ---- frames larger than the faces need (include/jda.h) ------------------------------------------------------------------------
def reduce_size(w, h, factor, orient=0):
    """jdaReduceSize: (W', H') of a w x h rectangle reduced by factor (1..8), then turned by orient."""
    rw, rh = C.c_int(), C.c_int()
    if lib.jdaReduceSize(int(w), int(h), int(factor), int(orient), C.byref(rw), C.byref(rh)) != 0:
        raise JdaError(last_error())
    return rw.value, rh.value


def _factors(factors, n):
    """One factor for all images or one per image -> int32 [max(n, 1)]."""
    f = np.full(n, int(factors), np.int32) if np.ndim(factors) == 0 else np.ascontiguousarray(factors, np.int32).reshape(-1)
    if len(f) != n:
        raise ValueError("factors: one factor for all images or one per image")
    return f if n else np.ones(1, np.int32)


def _reduced_sizes(sizes, factors):
    """The (w, h) of rectangles reduced by their factors (None: none is; a factor the library will refuse: as it is)."""
    return sizes if factors is None else [(w // max(int(f), 1), h // max(int(f), 1)) for (w, h), f in zip(sizes, factors)]


def pack_gray_reduced(images, formats, factors, orients=None, rects=None):
    """jdaPackGrayReduced: pack_gray_oriented with every image reduced by its factor first (1..8: one for all or one per image;
    block means, include/jda.h, "frames larger than the faces need"); orients None: every image upright -> a list of uint8
    [H', W'] gray arrays.  Host only: no cascador, no GPU."""
    return _pack_gray("pack_gray_reduced", images, formats, orients, rects, factors)


def reduce_back(images, formats, factors, orients, faces, boxes=None, landmarks=None, rects=None, left=(), right=()):
    """jdaReduceBack: what a detect call found on images REDUCED by factors and turned by orients (pack_gray_reduced[_device];
    orients None: upright) -> the coordinates of the whole source images, e.g. to cut chips from the full-resolution frames
    (face_chips[_device] on the original images).  Both calling forms of orient_back."""
    return orient_back(images, formats, 0 if orients is None else orients, faces, boxes, landmarks, rects, left, right, factors)


# ---- frames whose faces are rolled (include/jda.h) ----------------------------------------------------------------------------
def rotation_plan(w, h, degrees):
    """jdaRotationPlan: the plan of a w x h rectangle rotated by degrees (positive: clockwise as displayed) -> a dict with
    c, s (the exact table at multiples of 90, the host's cos / sin otherwise), w, h and the rotated size tw, th."""
    rot = jdaRotation()
    if lib.jdaRotationPlan(int(w), int(h), float(degrees), C.byref(rot)) != 0:
        raise JdaError(last_error())
    return rot.asdict()


def _degrees(degrees, n):
    """One angle for all images or one per image -> float64 [max(n, 1)]."""
    g = np.full(n, float(degrees), np.float64) if np.ndim(degrees) == 0 else np.ascontiguousarray(degrees, np.float64).reshape(-1)
    if len(g) != n:
        raise ValueError("degrees: one angle for all images or one per image")
    return g if n else np.zeros(1, np.float64)


def _rotated_sizes(sizes, degrees):
    """The (tw, th) of rectangles rotated by their angles (None: none is; what the plan refuses: as it is, the call will say)."""
    if degrees is None:
        return sizes
    out, rot = [], jdaRotation()
    for (w, h), g in zip(sizes, degrees):
        out.append((rot.tw, rot.th) if lib.jdaRotationPlan(int(w), int(h), float(g), C.byref(rot)) == 0 else (max(w, 0), max(h, 0)))
    return out


def pack_gray_rotated(images, formats, degrees, rects=None):
    """jdaPackGrayRotated: pack_gray with every image written rotated by its angle in degrees (any angle, positive: clockwise
    as displayed; one for all or one per image; include/jda.h, "frames whose faces are rolled") -> a list of uint8 [th, tw]
    gray arrays, black where the rotated canvas leaves the rectangle.  Host only: no cascador, no GPU."""
    return _pack_gray("pack_gray_rotated", images, formats, None, rects, None, degrees)


def rotate_back(images, formats, degrees, faces, boxes=None, landmarks=None, rects=None):
    """jdaRotateBack: what a detect call found on images ROTATED by degrees (pack_gray_rotated[_device]) -> the coordinates of
    the whole source images: landmarks through the rotation, boxes as the upright box of the same size around the rolled
    face's centre.  Both calling forms of orient_back; nothing mirrors, so there are no pairs."""
    return orient_back(images, formats, 0, faces, boxes, landmarks, rects, degrees=degrees)


def lib_landmarks(casc):
    info = jdaModelInfo()
    return info.landmark_n if lib.jdaCascadorInfo(casc.h, C.byref(info)) == 0 else 1


def _chip_faces(faces, landmarks, n_images):
    """(face_image int32 [n], landmarks float32 / float64 [n, 2L], real_bytes) from either form a caller has: face_image and
    a landmark array, or -- landmarks None -- one detect() result per image (a dict with "shapes", or None for no face)."""
    if landmarks is None:
        if len(faces) != n_images:
            raise ValueError("face_chips: one detect() result (or None) per image")
        shapes = [np.zeros((0, 0)) if r is None else np.asarray(r["shapes"] if isinstance(r, dict) else r) for r in faces]
        shapes = [s.reshape(len(s), -1) if len(s) else s.reshape(0, 0) for s in shapes]
        full = [s for s in shapes if len(s)]
        fi = np.concatenate([np.full(len(s), i, np.int32) for i, s in enumerate(shapes)]) if shapes else np.zeros(0, np.int32)
        lm = np.concatenate(full) if full else np.zeros((0, 2), np.float32)
    else:
        fi, lm = np.asarray(faces, np.int32).reshape(-1), np.asarray(landmarks)
        lm = lm.reshape(len(fi), -1) if len(fi) else np.zeros((0, 2), lm.dtype)
    if lm.dtype not in (np.float32, np.float64):
        lm = lm.astype(np.float64)
    return np.ascontiguousarray(fi, np.int32), np.ascontiguousarray(lm), lm.dtype.itemsize


def _chip_args(px, n_images, fi, lm, rb, L, tmpl, use, chip_w, chip_h, chip_format, supersample, dst, mats):
    t = None if tmpl is None else np.ascontiguousarray(tmpl, np.float64).reshape(-1)
    if t is not None and len(fi) and t.size != 2 * L:
        raise ValueError("face_chips: the template has %d values, the landmarks %d" % (t.size, 2 * L))
    u = None if use is None else np.ascontiguousarray(use, np.uint8).reshape(-1)
    if u is not None and len(fi) and u.size != L:
        raise ValueError("face_chips: one `use` byte per landmark")
    keep = (t, u, fi, lm)
    return keep, [px, n_images, fi.ctypes.data_as(C.POINTER(C.c_int)), lm.ctypes.data, rb, len(fi), L,
                  None if t is None else t.ctypes.data_as(C.POINTER(C.c_double)), None if u is None else u.ctypes.data,
                  int(chip_w), int(chip_h), _pixel_format(chip_format), int(supersample), dst,
                  mats.ctypes.data_as(C.POINTER(C.c_double))]


def face_chips(images, formats, faces, landmarks, tmpl, chip_w, chip_h, chip_format="gray8", rects=None, use=None, supersample=0,
               matrices=False):
    """jdaFaceChips (include/jda.h, "faces as they leave"): numpy uint8 images like pack_gray's, faces = the image index of
    every face and landmarks [n, 2L] float32 / float64 in the coordinates of the image's rectangle (or faces = one detect()
    result per image and landmarks None), tmpl [2L] chip pixels -> uint8 chips [n, chip_h, chip_w] (gray8) or
    [n, chip_h, chip_w, 3]; matrices=True: (chips, float64 [n, 6], chip -> source pixel).  Host only: no cascador, no GPU."""
    images, px, _ = _pixels("face_chips", images, formats, rects, False)
    fi, lm, rb = _chip_faces(faces, landmarks, len(images))
    n, bpp = len(fi), PIX_BYTES.get(_pixel_format(chip_format), 1)
    dst = np.zeros((n, int(chip_h), int(chip_w)) + ((bpp,) if bpp > 1 else ()), np.uint8)
    mats = np.zeros((max(n, 1), 6), np.float64)
    keep, args = _chip_args(px, len(images), fi, lm, rb, lm.shape[1] // 2, tmpl, use, chip_w, chip_h, chip_format, supersample,
                            dst.ctypes.data, mats)
    if lib.jdaFaceChips(*args) != 0:
        raise JdaError(last_error())
    del keep
    return (dst, mats[:n]) if matrices else dst


def count_windows(width, height, scale=1.25, min_size=40, max_size=-1):
    n, nl = C.c_longlong(), C.c_int()
    if lib.jdaCountWindows(width, height, scale, min_size, max_size, C.byref(n), C.byref(nl)) != 0:
        raise JdaError(last_error())
    return n.value, nl.value


def nms_c(bboxes, scores, overlap=0.3):
    """Host NMS of dialect C (reference c/jda.c:237-316): boolean keep mask in scan order."""
    bboxes = np.ascontiguousarray(bboxes, np.int32).reshape(-1, 3)
    scores = np.ascontiguousarray(scores, np.float32)
    keep = np.zeros(len(scores), np.uint8)
    if lib.jdaNmsC(bboxes.ctypes.data_as(C.POINTER(C.c_int)), scores.ctypes.data_as(C.POINTER(C.c_float)),
                   len(scores), overlap, keep.ctypes.data_as(C.POINTER(C.c_ubyte))) < 0:
        raise JdaError("jdaNmsC failed")
    return keep.astype(bool)


def nms_cpp(rects, scores, overlap=0.3):
    """Host NMS of dialect CPP (reference cascador.cpp:387-429): picked indices, best first."""
    rects = np.ascontiguousarray(rects, np.int32).reshape(-1, 4)
    scores = np.ascontiguousarray(scores, np.float64)
    picked = np.zeros(max(len(scores), 1), np.int32)
    n = lib.jdaNmsCpp(rects.ctypes.data_as(C.POINTER(C.c_int)), scores.ctypes.data_as(C.POINTER(C.c_double)),
                      len(scores), overlap, picked.ctypes.data_as(C.POINTER(C.c_int)))
    if n < 0:
        raise JdaError("jdaNmsCpp failed")
    return picked[:n].copy()


def _frame_ptrs(frames):
    """unsigned char*[n] for the frames of a contiguous [n,h,w] array.  From integer addresses: a ctypes cast per frame
    costs more than a millisecond per 256-frame batch, which is the order of the whole GPU pass."""
    n = frames.shape[0]
    base, stride = frames.ctypes.data, frames.strides[0]
    arr = (C.c_void_p * max(n, 1))(*[base + i * stride for i in range(n)])
    return C.cast(arr, C.POINTER(C.POINTER(C.c_ubyte)))


def _image_ptrs(images):
    arr = (C.c_void_p * max(len(images), 1))(*[im.ctypes.data for im in images])
    return C.cast(arr, C.POINTER(C.POINTER(C.c_ubyte)))


def _u8(a):
    return a.ctypes.data_as(C.POINTER(C.c_ubyte))


def _ivec(v, ctype=C.c_int, dtype=np.int32):
    """A sequence of integers as a C array argument without a Python loop (a job of thousands of images passes three of
    them per call).  Returns (keep-alive array, pointer)."""
    a = np.ascontiguousarray(v, dtype)
    if a.size == 0:
        a = np.zeros(1, dtype)
    return a, a.ctypes.data_as(C.POINTER(ctype))


class _RowsOwner:
    """Keeps the library's malloc'd row matrix until the last numpy view of it is gone, then gives it back
    (jdaRowsRelease / jdaRowsDRelease)."""
    def __init__(self, ptr, release):
        self._ptr, self._release = ptr, release

    def __del__(self):
        if self._ptr:
            self._release(self._ptr)
            self._ptr = None


def _owned_rows(ptr, n_rows, width, release, dtype):
    """The library's rows as a numpy array WITHOUT a copy (15 MB per dialect-CPP FDDB job): the array's base holds a
    _RowsOwner.  (numpy arrays are not garbage-collector tracked: the owner must not point back at the array.)"""
    owner = _RowsOwner(ptr, release)
    if n_rows <= 0:
        return np.empty((0, width), dtype)

    class _Holder:
        pass
    h = _Holder()
    h.__array_interface__ = np.ctypeslib.as_array(ptr, (n_rows, width)).__array_interface__
    h._owner = owner
    return np.asarray(h)


def _take(r):
    """jdaResult -> dict of numpy copies, then release the C arrays."""
    n, dim = r.n, 2 * r.landmark_n
    out = dict(
        bboxes=np.ctypeslib.as_array(r.bboxes, (n, 3)).copy() if n else np.zeros((0, 3), np.int32),
        scores=np.ctypeslib.as_array(r.scores, (n,)).copy() if n else np.zeros(0, np.float32),
        shapes=np.ctypeslib.as_array(r.shapes, (n, dim)).copy() if n else np.zeros((0, dim), np.float32))
    lib.jdaResultRelease(r)
    return out


def _take_d(r):
    n, dim = r.n, 2 * r.landmark_n
    out = dict(
        rects=np.ctypeslib.as_array(r.rects, (n, 4)).copy() if n else np.zeros((0, 4), np.int32),
        scores=np.ctypeslib.as_array(r.scores, (n,)).copy() if n else np.zeros(0, np.float64),
        shapes=np.ctypeslib.as_array(r.shapes, (n, dim)).copy() if n else np.zeros((0, dim), np.float64))
    lib.jdaResultDRelease(r)
    return out


class Cascador:
    """Owning handle around the opaque void* of the C API."""

    def __init__(self, model_path, real="auto", device=None):
        p = os.fsencode(model_path)
        if real == "double":
            self.h = lib.jdaCascadorCreateDouble(p)
        elif real == "float":
            self.h = lib.jdaCascadorCreateFloat(p)
        else:
            self.h = lib.jdaCascadorCreate(p)
        if not self.h:
            raise JdaError("cannot load model %s: %s" % (model_path, last_error()))
        self._read_info()
        if device is not None and lib.jdaSetDevice(self.h, int(device)) != 0:
            raise JdaError(last_error())

    def _read_info(self):
        info = jdaModelInfo()
        lib.jdaCascadorInfo(self.h, C.byref(info))
        self.T, self.K, self.L, self.D = info.T, info.K, info.landmark_n, info.tree_depth
        self.multi_scale = bool(info.multi_scale)
        self.source_real_bytes = info.source_real_bytes
        self.dim = 2 * self.L

    # -- the model in training (include/jda.h, "Dialect CPP: the model in training") ---------------------------------
    @classmethod
    def create_training_cpp(cls, T, K, L, D, mean_shape, device=None):
        """jdaCascadorCreateTrainingCpp: a cascador on JoinCascador::JoinCascador()'s model, status (0, -1), that
        put_cart_cpp / close_stage_cpp grow in place."""
        ms = np.ascontiguousarray(mean_shape, np.float64).reshape(-1)
        assert ms.size == 2 * int(L), "mean_shape must hold 2L doubles"
        self = cls.__new__(cls)
        self.h = lib.jdaCascadorCreateTrainingCpp(int(T), int(K), int(L), int(D), ms.ctypes.data_as(C.POINTER(C.c_double)))
        if not self.h:
            raise JdaError("cannot create a training cascador: %s" % last_error())
        self._read_info()
        if device is not None and lib.jdaSetDevice(self.h, int(device)) != 0:
            raise JdaError(last_error())
        return self

    def model_status_cpp(self):
        """(stage, cart): carts [0, cart] of `stage` are written, stages [0, stage) closed; (T, -1) is the complete model."""
        s, c = C.c_int(), C.c_int()
        if lib.jdaModelStatusCpp(self.h, C.byref(s), C.byref(c)) != 0:
            raise JdaError(last_error())
        return s.value, c.value

    def put_cart_cpp(self, k, features, thresholds, leaf_scores, th, mean=0., std=1.):
        """jdaModelPutCartCpp: cart k of the stage in training from train_cart_cpp's features, thresholds and scores as they
        are; k == cart + 1 appends, k == cart replaces the last cart."""
        inner, half = (1 << (self.D - 1)) - 1, 1 << (self.D - 1)
        fa, fp = _features(features)
        ta = np.ascontiguousarray(thresholds, np.int32).reshape(-1)
        la = np.ascontiguousarray(leaf_scores, np.float64).reshape(-1)
        assert len(fa) == inner and ta.size == inner and la.size == half, "one cart: nodes_n/2 - 1 split nodes, nodes_n/2 leaves"
        if lib.jdaModelPutCartCpp(self.h, int(k), fp, ta.ctypes.data_as(C.POINTER(C.c_int)), la.ctypes.data_as(C.POINTER(C.c_double)),
                                  float(th), float(mean), float(std)) != 0:
            raise JdaError(last_error())
        self._read_info()

    def close_stage_cpp(self, w):
        """jdaModelCloseStageCpp: the stage's [K * leafNum, 2L] weights (global_regression_cpp's w); status -> (stage + 1, -1)."""
        wa = np.ascontiguousarray(w, np.float64).reshape(-1)
        assert wa.size == self.K * (1 << (self.D - 1)) * self.dim, "w must hold K * leafNum rows of 2L doubles"
        if lib.jdaModelCloseStageCpp(self.h, wa.ctypes.data_as(C.POINTER(C.c_double))) != 0:
            raise JdaError(last_error())

    def validate_samples_cpp(self, samples, origin_size=48, half_size=36, quarter_size=24):
        """jdaValidateSamplesCpp: Validate (reference cascador.cpp:166-211) under the model as it stands on every record of a
        resident sample set -- dict(patches=[n, o*o + h*h + q*q] uint8 numpy array or torch CUDA tensor, shapes=[n, 2L] the
        start shapes) -> dict of is_face, score, carts_n, shape, stats."""
        pb = _patch_bytes(origin_size, half_size, quarter_size)
        s, keep = _samples(samples, self.dim, pb)
        n = s.n
        face = np.zeros(max(n, 1), np.uint8)
        score = np.zeros(max(n, 1), np.float64)
        carts = np.zeros(max(n, 1), np.int32)
        shape = np.zeros((max(n, 1), self.dim), np.float64)
        st = jdaStageStatsCpp()
        rc = lib.jdaValidateSamplesCpp(self.h, C.byref(s), origin_size, half_size, quarter_size, _u8(face),
                                       score.ctypes.data_as(C.POINTER(C.c_double)), carts.ctypes.data_as(C.POINTER(C.c_int)),
                                       shape.ctypes.data_as(C.POINTER(C.c_double)), C.byref(st))
        del keep
        if rc != 0:
            raise JdaError(last_error())
        return dict(is_face=face[:n], score=score[:n], carts_n=carts[:n], shape=shape[:n], stats=st.asdict())

    def serialize_to_cpp(self, path):
        """jdaCascadorSerializeToCpp: the trainer's f64 file with the status in its header (refused at (s, K - 1))."""
        if lib.jdaCascadorSerializeToCpp(self.h, os.fsencode(path)) != 0:
            raise JdaError(last_error())

    def close(self):
        if getattr(self, "h", None):
            lib.jdaCascadorRelease(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def set_similarity_transform(self, on):
        """Dialect CPP: Config face.similarity_transform (reference common.cpp:214)."""
        if lib.jdaSetSimilarityTransform(self.h, 1 if on else 0) != 0:
            raise JdaError("jdaSetSimilarityTransform failed")

    def set_option(self, key, value):
        """jdaSetOption: tuning knobs of this cascador (include/jda.h); never changes results."""
        if lib.jdaSetOption(self.h, key.encode(), int(value)) != 0:
            raise JdaError(last_error())

    def get_option(self, key):
        return int(lib.jdaGetOption(self.h, key.encode()))

    def finish_forms(self):
        """jdaFinishForms: how often this cascador's passes have issued each finishing form since it was created
        (include/jda.h: JDA_FINISH_*, in that order).  The counts only grow; take the difference around a call."""
        counts = (C.c_longlong * len(FINISH_FORMS))()
        if lib.jdaFinishForms(self.h, counts) != 0:
            raise JdaError(last_error())
        return dict(zip(FINISH_FORMS, (int(x) for x in counts)))

    def scan_forms(self):
        """jdaScanForms: how often this cascador's passes have launched each stage-0 scan instantiation since it was
        created -> {ScanForm(kernel, dialect, depth, pix, ragged, lean, trace, merged): count}, zeros left out.  The
        counts only grow; take the difference around a call."""
        counts = (C.c_longlong * SCAN_FORM_N)()
        if lib.jdaScanForms(self.h, counts) != 0:
            raise JdaError(last_error())
        return {ScanForm.of_index(i): int(x) for i, x in enumerate(counts) if x}

    def finish_launches(self):
        """jdaFinishLaunches: how often this cascador's passes have launched each k_finish / k_filter0 instantiation since it
        was created -> {FinishLaunch(kernel, dialect, trace, groups, multi, st, stream, survivors, carry, tile): count},
        zeros left out.  One count per launch; the counts only grow; take the difference around a call."""
        counts = (C.c_longlong * FINISH_LAUNCH_N)()
        if lib.jdaFinishLaunches(self.h, counts) != 0:
            raise JdaError(last_error())
        return {FinishLaunch.of_index(i): int(x) for i, x in enumerate(counts) if x}

    def finish_tile_win(self, dialect):
        """jdaFinishTileWin: the largest window side k_finish copies to LDS with this model in `dialect` ("C" / "CPP", or
        JDA_DIALECT_*); 0: none."""
        r = int(lib.jdaFinishTileWin(self.h, {"C": JDA_DIALECT_C, "CPP": JDA_DIALECT_CPP}.get(dialect, dialect)))
        if r < 0:
            raise JdaError(last_error())
        return r

    def stage_launches(self):
        """jdaStageLaunches: how often this cascador's dense passes have launched each k_stage instantiation and cart chunk
        since it was created -> {StageLaunch(dialect, trace, glb, acc, chunk): count}, zeros left out.  One count per launch
        (stages x levels a pass); the counts only grow; take the difference around a call."""
        counts = (C.c_longlong * STAGE_LAUNCH_N)()
        if lib.jdaStageLaunches(self.h, counts) != 0:
            raise JdaError(last_error())
        return {StageLaunch.of_index(i): int(x) for i, x in enumerate(counts) if x}

    def mine_launches(self):
        """jdaMineLaunches: what this cascador's mining and Validate calls have launched since it was created -> a dict with
        every name of MINE_LAUNCH_FIELDS: launches of the five k_mine.hip kernels, chunks, walk batches, saturated
        k_mine_sum launches, the scan's and the walk's rejects (cumulative: take the difference around a call), the largest
        walk batch so far and the batch cap of the last call."""
        counts = (C.c_longlong * MINE_LAUNCH_N)()
        if lib.jdaMineLaunches(self.h, counts) != 0:
            raise JdaError(last_error())
        return {k: int(x) for k, x in zip(MINE_LAUNCH_FIELDS, counts)}

    def stage_launch_for(self, dialect, trace, win, step):
        """jdaStageLaunchFor: (the StageLaunch key, the dynamic LDS bytes) of the k_stage launch a level of `win`-pixel
        windows `step` pixels apart would take with this model in `dialect` ("C" / "CPP", or JDA_DIALECT_*); None where
        dense mode declines the model or the dialect; an unknown dialect, or a window or step below 1, raises JdaError.
        Runs nothing, needs no device."""
        lds = C.c_int(0)
        d = {"C": JDA_DIALECT_C, "CPP": JDA_DIALECT_CPP}.get(dialect, dialect)
        r = int(lib.jdaStageLaunchFor(self.h, d, 1 if trace else 0, int(win), int(step), C.byref(lds)))
        if r < 0 and (d not in (JDA_DIALECT_C, JDA_DIALECT_CPP) or int(win) < 1 or int(step) < 1):
            raise JdaError(last_error())
        return None if r < 0 else (StageLaunch.of_index(r), int(lds.value))

    def serialize(self, path):
        lib.jdaCascadorSerializeTo(self.h, os.fsencode(path))

    # -- single frame, exactly the reference call -----------------------------
    def detect(self, img, scale=1.25, step=0.1, min_size=40, max_size=-1, th=-0.5):
        img = np.ascontiguousarray(img, np.uint8)
        h, w = img.shape
        r = lib.jdaDetect(self.h, _u8(img), w, h, scale, step, min_size, max_size, th)
        err = last_error()
        if r.n == 0 and err:
            lib.jdaResultRelease(r)
            raise JdaError(err)
        return _take(r)

    def _opts(self, nms, stats):
        o = jdaDetectOptions()
        lib.jdaDetectOptionsInit(C.byref(o))
        o.nms = 1 if nms else 0
        st = jdaStats() if stats else None
        if st is not None:
            o.stats = C.pointer(st)
        return o, st

    # -- batch of host frames ---------------------------------------------------
    def detect_batch(self, frames, scale=1.25, min_size=40, max_size=-1, th=-0.5, nms=True, stats=False):
        frames = np.ascontiguousarray(frames, np.uint8)
        n, h, w = frames.shape
        ptrs = _frame_ptrs(frames)
        res = (jdaResult * max(n, 1))()
        o, st = self._opts(nms, stats)
        rc = lib.jdaDetectBatch(self.h, ptrs, n, w, h, scale, 0.1, min_size, max_size, th, C.byref(o), res)
        if rc != 0:
            raise JdaError(last_error())
        out = [_take(res[i]) for i in range(n)]
        return (out, st.asdict()) if stats else out

    # -- batch resident in device memory (torch uint8 CUDA tensor [n,h,w]) ------------
    def detect_batch_device(self, d_frames, scale=1.25, min_size=40, max_size=-1, th=-0.5, nms=True,
                            stats=False, keep_results=True, frame_offset=0, hip_stream=None):
        assert d_frames.is_cuda and d_frames.dtype.itemsize == 1 and d_frames.is_contiguous()
        n, h, w = d_frames.shape
        res = (jdaResult * max(n, 1))()
        o, st = self._opts(nms, stats)
        if hip_stream is not None:      # a hipStream_t handle (e.g. torch.cuda.Stream().cuda_stream): work is ordered on it
            o.hip_stream = C.c_void_p(hip_stream)
        rc = lib.jdaDetectBatchDevice(self.h, C.c_void_p(d_frames.data_ptr()), h * w, n, w, h, scale, 0.1,
                                      min_size, max_size, th, C.byref(o), res)
        if rc != 0:
            raise JdaError(last_error())
        if keep_results == "packed":
            # one C call: rows [frame, x, y, size, score, shape...] of every detection of the batch
            rows = lib.jdaResultsPack(res, n, frame_offset, None, 0)
            out = np.empty((max(rows, 0), 5 + self.dim), np.float32)
            if rows > 0:
                lib.jdaResultsPack(res, n, frame_offset, out.ctypes.data_as(C.POINTER(C.c_float)), rows)
            lib.jdaResultsRelease(res, n)
        elif keep_results:
            out = [_take(res[i]) for i in range(n)]
        else:
            out = [res[i].n for i in range(n)]
            lib.jdaResultsRelease(res, n)
        return (out, st.asdict()) if stats else out

    # -- images of different sizes in one job --------------------------------------------
    def _collect(self, res, n, keep_results, frame_offset=0):
        if keep_results == "packed":
            rows = lib.jdaResultsPack(res, n, frame_offset, None, 0)
            out = np.empty((max(rows, 0), 5 + self.dim), np.float32)
            if rows > 0:
                lib.jdaResultsPack(res, n, frame_offset, out.ctypes.data_as(C.POINTER(C.c_float)), rows)
            lib.jdaResultsRelease(res, n)
        elif keep_results:
            out = [_take(res[i]) for i in range(n)]
        else:
            out = [res[i].n for i in range(n)]
            lib.jdaResultsRelease(res, n)
        return out

    def detect_ragged(self, images, scale=1.25, min_size=40, max_size=-1, th=-0.5, nms=True, stats=False,
                      keep_results=True):
        """jdaDetectBatchRagged: a list of uint8 [h, w] arrays of different sizes in host memory."""
        images = [np.ascontiguousarray(im, np.uint8) for im in images]
        n = len(images)
        ptrs = _image_ptrs(images)
        ws = (C.c_int * max(n, 1))(*[im.shape[1] for im in images])
        hs = (C.c_int * max(n, 1))(*[im.shape[0] for im in images])
        res = (jdaResult * max(n, 1))()
        o, st = self._opts(nms, stats)
        rc = lib.jdaDetectBatchRagged(self.h, ptrs, ws, hs, n, scale, 0.1, min_size, max_size, th, C.byref(o), res)
        if rc != 0:
            raise JdaError(last_error())
        out = self._collect(res, n, keep_results)
        return (out, st.asdict()) if stats else out

    def detect_ragged_packed(self, buf, offsets, widths, heights, scale=1.25, min_size=40, max_size=-1, th=-0.5,
                             nms=True, stats=False, keep_results=True, frame_offset=0):
        """The same for images packed in ONE buffer (image i = buf[offsets[i] : offsets[i] + w*h], rows back to
        back): a numpy uint8 array (host entry, jdaDetectBatchRagged) or a torch uint8 CUDA tensor
        (jdaDetectBatchRaggedDevice)."""
        n = len(offsets)
        _kw, ws = _ivec(widths)
        _kh, hs = _ivec(heights)
        o, st = self._opts(nms, stats)
        host = isinstance(buf, np.ndarray)
        if host:
            assert buf.dtype == np.uint8 and buf.flags.c_contiguous
            _ko, ptrs = _ivec(np.asarray(offsets, np.uint64) + np.uint64(buf.ctypes.data), C.POINTER(C.c_ubyte), np.uint64)
        else:
            assert buf.is_cuda and buf.dtype.itemsize == 1 and buf.is_contiguous()
            _ko, offs = _ivec(offsets, C.c_size_t, np.uint64)
        if keep_results == "packed" and hasattr(lib, "jdaDetectBatchRaggedDeviceRows"):
            # rows straight from the library (jdaDetectBatchRagged[Device]Rows): no jdaResult per image in between
            rp, nr = C.POINTER(C.c_float)(), C.c_int(0)
            if host:
                rc = lib.jdaDetectBatchRaggedRows(self.h, ptrs, ws, hs, n, scale, 0.1, min_size, max_size, th, C.byref(o),
                                                  frame_offset, C.byref(rp), C.byref(nr))
            else:
                rc = lib.jdaDetectBatchRaggedDeviceRows(self.h, C.c_void_p(buf.data_ptr()), offs, ws, hs, n, scale, 0.1,
                                                        min_size, max_size, th, C.byref(o), frame_offset, C.byref(rp), C.byref(nr))
            if rc != 0:
                raise JdaError(last_error())
            out = _owned_rows(rp, nr.value, 5 + self.dim, lib.jdaRowsRelease, np.float32)
            return (out, st.asdict()) if stats else out
        res = (jdaResult * max(n, 1))()
        if host:
            rc = lib.jdaDetectBatchRagged(self.h, ptrs, ws, hs, n, scale, 0.1, min_size, max_size, th, C.byref(o), res)
        else:
            rc = lib.jdaDetectBatchRaggedDevice(self.h, C.c_void_p(buf.data_ptr()), offs, ws, hs, n, scale, 0.1,
                                                min_size, max_size, th, C.byref(o), res)
        if rc != 0:
            raise JdaError(last_error())
        out = self._collect(res, n, keep_results, frame_offset)
        return (out, st.asdict()) if stats else out

    # -- frames as they arrive: colour / pitched / cropped device images -> dense gray ----------
    def _pack_gray_device(self, who, images, formats, orients, rects, frame_stride, stats, hip_stream, out, factors=None, degrees=None):
        """pack_gray_device (orients None), pack_gray_oriented_device, with factors pack_gray_reduced_device and, with degrees,
        pack_gray_rotated_device."""
        images, px, sizes = _pixels(who, images, formats, rects, True)
        n = len(images)
        (_, device, _), arrays, sizes = _frame_call(sizes, orients, factors, degrees, n)
        offs, tot = _offsets(sizes, 256, frame_stride)
        if out is not None:
            offs = np.ascontiguousarray(out[1], np.uint64)
            assert len(offs) == n
        buf = _device_buffer(None if out is None else out[0], tot, images)
        st = jdaPackStats() if stats else None
        tail = (C.c_void_p(buf.data_ptr()), offs.ctypes.data_as(C.POINTER(C.c_size_t)),
                C.c_void_p(hip_stream) if hip_stream is not None else None, C.byref(st) if stats else None)
        rc = getattr(lib, device)(self.h, px, *arrays, n, *tail)
        if rc != 0:
            raise JdaError(last_error())
        res = (buf, offs[:n], [w for w, _ in sizes], [h for _, h in sizes])
        return (res, st.asdict()) if stats else res

    def pack_gray_device(self, images, formats, rects=None, frame_stride=None, stats=False, hip_stream=None, out=None):
        """jdaPackGrayDevice: torch uint8 CUDA tensors [H, W, C] or [H, W] (strided views allowed: a view's row stride is the
        pitch) of the given formats, each cut to its rectangle (x, y, w, h) (None: the whole image), packed to gray by ONE
        kernel launch.  -> (buffer, offsets, widths, heights): a torch uint8 CUDA tensor and where every image lies in it --
        the arguments of detect_ragged_packed / detect_ragged_cpp_packed and the device image set of validate_cpp,
        mine_negatives_cpp and build_positives_cpp.  Image i starts at a multiple of 256 bytes, or with frame_stride at
        i * frame_stride: buffer.view(n, h, w) then goes into detect_batch_device / submit_batch_device where frame_stride ==
        w * h.  hip_stream: a hipStream_t handle (torch.cuda.Stream().cuda_stream) the pixels were produced on.
        out = (buffer, offsets): the caller's own destination.  stats=True: (that tuple, jdaPackStats as a dict)."""
        return self._pack_gray_device("pack_gray_device", images, formats, None, rects, frame_stride, stats, hip_stream, out)

    def pack_gray_oriented_device(self, images, formats, orients, rects=None, frame_stride=None, stats=False, hip_stream=None, out=None):
        """jdaPackGrayOrientedDevice: pack_gray_device with every image written turned by its orientation (0..7: one for all
        or one per image; include/jda.h, "frames in any orientation") by ONE kernel launch.  -> (buffer, offsets, widths,
        heights) of the TURNED images, like pack_gray_device's; api.orient_back takes what a detect call finds on them back
        to the source images."""
        return self._pack_gray_device("pack_gray_oriented_device", images, formats, orients, rects, frame_stride, stats, hip_stream, out)

    def pack_gray_reduced_device(self, images, formats, factors, orients=None, rects=None, frame_stride=None, stats=False, hip_stream=None,
                                 out=None):
        """jdaPackGrayReducedDevice: pack_gray_oriented_device with every image reduced by its factor first (1..8: one for all
        or one per image; block means; include/jda.h, "frames larger than the faces need") by ONE kernel launch; orients
        None: every image upright.  -> (buffer, offsets, widths, heights) of the REDUCED, turned images, like
        pack_gray_device's; api.reduce_back takes what a detect call finds on them back to the source images."""
        return self._pack_gray_device("pack_gray_reduced_device", images, formats, orients, rects, frame_stride, stats, hip_stream, out, factors)

    def pack_gray_rotated_device(self, images, formats, degrees, rects=None, frame_stride=None, stats=False, hip_stream=None, out=None):
        """jdaPackGrayRotatedDevice: pack_gray_device with every image written rotated by its angle in degrees (any angle,
        positive: clockwise as displayed; one for all or one per image; include/jda.h, "frames whose faces are rolled") by ONE
        kernel launch.  -> (buffer, offsets, widths, heights) of the ROTATED images, like pack_gray_device's;
        api.rotate_back takes what a detect call finds on them back to the source images."""
        return self._pack_gray_device("pack_gray_rotated_device", images, formats, None, rects, frame_stride, stats, hip_stream, out, None, degrees)

    # -- faces as they leave: upright chips cut from device images ---------------------------------
    def mean_shape(self):
        """jdaCascadorMeanShape: the model's mean shape, float64 [2L], normalised to the detection window."""
        info = jdaModelInfo()
        if lib.jdaCascadorInfo(self.h, C.byref(info)) != 0:
            raise JdaError("jdaCascadorInfo failed")
        out = np.zeros(2 * info.landmark_n, np.float64)
        if lib.jdaCascadorMeanShape(self.h, out.ctypes.data_as(C.POINTER(C.c_double))) != 0:
            raise JdaError(last_error())
        return out

    def face_chips_device(self, images, formats, faces, landmarks=None, tmpl=None, chip_w=112, chip_h=112, chip_format="gray8",
                          rects=None, use=None, supersample=0, matrices=False, stats=False, hip_stream=None, out=None):
        """jdaFaceChipsDevice: torch uint8 CUDA tensors like pack_gray_device's, faces / landmarks like face_chips' (one
        detect() result per image with landmarks None), tmpl None: the model's mean shape at the chip's size -> a torch
        uint8 CUDA tensor [n, chip_h, chip_w(, 3)], cut by ONE kernel launch.  out: the caller's own destination, a
        contiguous uint8 CUDA tensor of n * chip_h * chip_w * bytes per pixel elements at any address.  matrices=True /
        stats=True append the float64 [n, 6] matrices / jdaChipStats as a dict to the returned tuple."""
        images, px, _ = _pixels("face_chips_device", images, formats, rects, True)
        fi, lm, rb = _chip_faces(faces, landmarks, len(images))
        n, bpp = len(fi), PIX_BYTES.get(_pixel_format(chip_format), 1)
        shape = (n, int(chip_h), int(chip_w)) + ((bpp,) if bpp > 1 else ())
        assert out is None or out.numel() == int(np.prod(shape))
        buf = _device_buffer(out, int(np.prod(shape)), images)
        mats = np.zeros((max(n, 1), 6), np.float64)
        L = lm.shape[1] // 2 if n else lib_landmarks(self)
        keep, args = _chip_args(px, len(images), fi, lm, rb, L, tmpl, use, chip_w, chip_h, chip_format, supersample,
                                C.c_void_p(buf.data_ptr()), mats)
        st = jdaChipStats() if stats else None
        rc = lib.jdaFaceChipsDevice(self.h, *args, C.c_void_p(hip_stream) if hip_stream is not None else None,
                                    C.byref(st) if stats else None)
        del keep
        if rc != 0:
            raise JdaError(last_error())
        res = (buf.view(-1)[:int(np.prod(shape))].view(shape),)
        if matrices:
            res += (mats[:n],)
        if stats:
            res += (st.asdict(),)
        return res[0] if len(res) == 1 else res

    # -- two batches in flight from one thread -----------------------------------
    def submit_batch_device(self, d_frames, scale=1.25, min_size=40, max_size=-1, th=-0.5, nms=True, stats=False):
        """Queues the scan of a batch and returns a ticket; collect it with wait_batch (the frames are kept
        alive until then).  Submit batch i+1 before waiting for batch i to overlap host and device work.
        stats=True: the pass is bracketed with timing events, so wait_batch(stats=True) reports gpu_ms / scan_ms
        (the counters are reported either way)."""
        assert d_frames.is_cuda and d_frames.dtype.itemsize == 1 and d_frames.is_contiguous()
        n, h, w = d_frames.shape
        o, _ = self._opts(nms, stats)
        t = lib.jdaDetectBatchSubmit(self.h, C.c_void_p(d_frames.data_ptr()), h * w, n, w, h, scale, 0.1,
                                     min_size, max_size, th, C.byref(o))
        if t < 0:
            raise JdaError(last_error())
        if not hasattr(self, "_pending"):
            self._pending = {}
        self._pending[t] = (d_frames, n)
        return t

    def submit_batch_host(self, frames, scale=1.25, min_size=40, max_size=-1, th=-0.5, nms=True, stats=False):
        """Submit for frames in host memory (numpy uint8 [n,h,w]; kept alive until wait_batch)."""
        frames = np.ascontiguousarray(frames, np.uint8)
        n, h, w = frames.shape
        ptrs = _frame_ptrs(frames)
        o, _ = self._opts(nms, stats)
        t = lib.jdaDetectBatchSubmitHost(self.h, ptrs, n, w, h, scale, 0.1, min_size, max_size, th, C.byref(o))
        if t < 0:
            raise JdaError(last_error())
        if not hasattr(self, "_pending"):
            self._pending = {}
        self._pending[t] = ((frames, ptrs), n)
        return t

    def wait_batch(self, ticket, stats=False, keep_results=True, frame_offset=0):
        d_frames, n = self._pending.pop(ticket)
        res = (jdaResult * max(n, 1))()
        st = jdaStats() if stats else None
        rc = lib.jdaDetectBatchWait(self.h, ticket, C.byref(st) if stats else None, res)
        if rc != 0:
            raise JdaError(last_error())
        if keep_results == "packed":
            rows = lib.jdaResultsPack(res, n, frame_offset, None, 0)
            out = np.empty((max(rows, 0), 5 + self.dim), np.float32)
            if rows > 0:
                lib.jdaResultsPack(res, n, frame_offset, out.ctypes.data_as(C.POINTER(C.c_float)), rows)
            lib.jdaResultsRelease(res, n)
        elif keep_results:
            out = [_take(res[i]) for i in range(n)]
        else:
            out = [res[i].n for i in range(n)]
            lib.jdaResultsRelease(res, n)
        return (out, st.asdict()) if stats else out

    def plan_tiles(self, width, height, scale=1.25, min_size=40, max_size=-1):
        """How k_scan would tile each pyramid level of a dialect-C call (no GPU needed)."""
        out = np.zeros((64, 10), np.int32)
        n = lib.jdaDebugPlanTiles(self.h, width, height, scale, min_size, max_size,
                                  out.ctypes.data_as(C.POINTER(C.c_int)), 64)
        if n < 0:
            raise JdaError(last_error())
        keys = ("win", "step", "nx", "ny", "mode", "tw", "th", "pitch", "tiles_x", "tiles_y")
        return [dict(zip(keys, (int(v) for v in row))) for row in out[:n]]

    # -- parity instrumentation ---------------------------------------------------
    def trace(self, frames, scale=1.25, min_size=40, max_size=-1):
        frames = np.ascontiguousarray(frames, np.uint8)
        if frames.ndim == 2:
            frames = frames[None]
        n, h, w = frames.shape
        wpf, _ = count_windows(w, h, scale, min_size, max_size)
        tot = n * wpf
        carts = np.zeros(tot, np.int32)
        score = np.zeros(tot, np.float32)
        hsh = np.zeros(tot, np.uint32)
        shapes = np.zeros((tot, self.dim), np.float32)
        ptrs = _frame_ptrs(frames)
        rc = lib.jdaTraceBatch(self.h, ptrs, n, w, h, scale, min_size, max_size,
                               carts.ctypes.data_as(C.POINTER(C.c_int)), score.ctypes.data_as(C.POINTER(C.c_float)),
                               hsh.ctypes.data_as(C.POINTER(C.c_uint)), shapes.ctypes.data_as(C.POINTER(C.c_float)))
        if rc != 0:
            raise JdaError(last_error())
        return dict(carts_n=carts, score=score, path_hash=hsh, shapes=shapes)

    def validate_windows(self, frames, windows, th=-0.5, device=False, stats=False):
        """The cascade on caller-given windows, rows of (frame, x, y, size) (jdaValidateWindows; the body of the reference's
        window loop, c/jda.c:340-414, with the relocation of c/jda.c:471-472).  frames: [n, h, w] uint8, a numpy array (host
        entry) or a torch CUDA tensor (jdaValidateWindowsDevice); device=True with a numpy array stages it on the device
        first (torch) and calls the device entry.  -> dict of is_face, score, carts_n, path_hash, shapes, landmarks (numpy,
        the caller's order)."""
        if not hasattr(lib, "jdaValidateWindows"):
            raise JdaError("this libjda.so has no jdaValidateWindows (a build from before the entry, loaded through JDA_LIB_PATH)")
        if device and isinstance(frames, np.ndarray):
            import torch
            frames = torch.from_numpy(np.ascontiguousarray(frames, np.uint8)).cuda()
        dev = not isinstance(frames, np.ndarray)
        if dev:
            assert frames.is_cuda and frames.dtype.itemsize == 1 and frames.is_contiguous()
        else:
            frames = np.ascontiguousarray(frames, np.uint8)
        if frames.ndim == 2:
            frames = frames[None]
        n, h, w = frames.shape
        win = np.ascontiguousarray(np.asarray(windows, np.int32).reshape(-1, 4))
        nw = win.shape[0]
        face = np.zeros(max(nw, 1), np.uint8)
        score = np.zeros(max(nw, 1), np.float32)
        carts = np.zeros(max(nw, 1), np.int32)
        hsh = np.zeros(max(nw, 1), np.uint32)
        shapes = np.zeros((max(nw, 1), self.dim), np.float32)
        lms = np.zeros((max(nw, 1), self.dim), np.float32)
        st = jdaStats()
        tail = (n, w, h, win.ctypes.data_as(C.POINTER(C.c_int)), nw, th, _u8(face), score.ctypes.data_as(C.POINTER(C.c_float)),
                carts.ctypes.data_as(C.POINTER(C.c_int)), hsh.ctypes.data_as(C.POINTER(C.c_uint)),
                shapes.ctypes.data_as(C.POINTER(C.c_float)), lms.ctypes.data_as(C.POINTER(C.c_float)), C.byref(st))
        if dev:
            rc = lib.jdaValidateWindowsDevice(self.h, C.c_void_p(frames.data_ptr()), h * w, *tail)
        else:
            rc = lib.jdaValidateWindows(self.h, _frame_ptrs(frames), *tail)
        if rc != 0:
            raise JdaError(last_error())
        out = dict(is_face=face[:nw], score=score[:nw], carts_n=carts[:nw], path_hash=hsh[:nw], shapes=shapes[:nw], landmarks=lms[:nw])
        return (out, st.asdict()) if stats else out

    def build_pyramid(self, img):
        img = np.ascontiguousarray(img, np.uint8)
        h, w = img.shape
        d = [C.c_int() for _ in range(4)]
        if lib.jdaBuildPyramid(self.h, _u8(img), w, h, None, C.byref(d[0]), C.byref(d[1]), None,
                               C.byref(d[2]), C.byref(d[3])) != 0:
            raise JdaError(last_error())
        hw, hh, qw, qh = [x.value for x in d]
        half = np.zeros((max(hh, 0), max(hw, 0)), np.uint8)
        quarter = np.zeros((max(qh, 0), max(qw, 0)), np.uint8)
        if lib.jdaBuildPyramid(self.h, _u8(img), w, h, _u8(half), C.byref(d[0]), C.byref(d[1]), _u8(quarter),
                               C.byref(d[2]), C.byref(d[3])) != 0:
            raise JdaError(last_error())
        return half, quarter

    # -- dialect CPP ----------------------------------------------------------------
    def detect_batch_cpp(self, frames, minimum_size=20, step=5, factor=1.2, overlap=0.3, nms=True, stats=False):
        frames = np.ascontiguousarray(frames, np.uint8)
        if frames.ndim == 2:
            frames = frames[None]
        n, h, w = frames.shape
        ptrs = _frame_ptrs(frames)
        res = (jdaResultD * max(n, 1))()
        st = jdaStats()
        rc = lib.jdaDetectBatchCpp(self.h, ptrs, n, w, h, minimum_size, step, factor, overlap, 1 if nms else 0,
                                   C.byref(st), res)
        if rc != 0:
            raise JdaError(last_error())
        out = [_take_d(res[i]) for i in range(n)]
        return (out, st.asdict()) if stats else out

    def _collect_d(self, res, n, keep_results, frame_offset=0):
        if keep_results == "packed":
            # one C call: rows [frame, x, y, w, h, score, shape...] (float64) of every detection of the batch
            rows = lib.jdaResultsDPack(res, n, frame_offset, None, 0)
            out = np.empty((max(rows, 0), 6 + self.dim), np.float64)
            if rows > 0:
                lib.jdaResultsDPack(res, n, frame_offset, out.ctypes.data_as(C.POINTER(C.c_double)), rows)
            lib.jdaResultsDRelease(res, n)
            return out
        if keep_results:
            return [_take_d(res[i]) for i in range(n)]
        out = [res[i].n for i in range(n)]
        lib.jdaResultsDRelease(res, n)
        return out

    def detect_batch_cpp_device(self, d_frames, minimum_size=20, step=5, factor=1.2, overlap=0.3, nms=True, stats=False,
                                keep_results=True, frame_offset=0):
        """jdaDetectBatchCppDevice: a torch uint8 CUDA tensor [n, h, w] resident in HBM."""
        assert d_frames.is_cuda and d_frames.dtype.itemsize == 1 and d_frames.is_contiguous()
        n, h, w = d_frames.shape
        res = (jdaResultD * max(n, 1))()
        st = jdaStats()
        rc = lib.jdaDetectBatchCppDevice(self.h, C.c_void_p(d_frames.data_ptr()), h * w, n, w, h, minimum_size, step, factor,
                                         overlap, 1 if nms else 0, C.byref(st) if stats else None, res)
        if rc != 0:
            raise JdaError(last_error())
        out = self._collect_d(res, n, keep_results, frame_offset)
        return (out, st.asdict()) if stats else out

    def detect_ragged_cpp(self, images, minimum_size=20, step=5, factor=1.2, overlap=0.3, nms=True, stats=False,
                          keep_results=True):
        """jdaDetectBatchCppRagged: a list of uint8 [h, w] arrays of different sizes in host memory -- the reference's
        `jda fddb` loop (one joincascador.Detect per image, src/test.cpp:142) as one job."""
        images = [np.ascontiguousarray(im, np.uint8) for im in images]
        n = len(images)
        ptrs = _image_ptrs(images)
        ws = (C.c_int * max(n, 1))(*[im.shape[1] for im in images])
        hs = (C.c_int * max(n, 1))(*[im.shape[0] for im in images])
        res = (jdaResultD * max(n, 1))()
        st = jdaStats()
        rc = lib.jdaDetectBatchCppRagged(self.h, ptrs, ws, hs, n, minimum_size, step, factor, overlap, 1 if nms else 0,
                                         C.byref(st) if stats else None, res)
        if rc != 0:
            raise JdaError(last_error())
        out = self._collect_d(res, n, keep_results)
        return (out, st.asdict()) if stats else out

    def detect_ragged_cpp_packed(self, buf, offsets, widths, heights, minimum_size=20, step=5, factor=1.2, overlap=0.3,
                                 nms=True, stats=False, keep_results=True, frame_offset=0):
        """The same for images packed in ONE buffer (image i = buf[offsets[i] : offsets[i] + w*h]): a numpy uint8 array
        (jdaDetectBatchCppRagged) or a torch uint8 CUDA tensor (jdaDetectBatchCppRaggedDevice)."""
        n = len(offsets)
        _kw, ws = _ivec(widths)
        _kh, hs = _ivec(heights)
        st = jdaStats()
        sp = C.byref(st) if stats else None
        host = isinstance(buf, np.ndarray)
        if host:
            assert buf.dtype == np.uint8 and buf.flags.c_contiguous
            _ko, ptrs = _ivec(np.asarray(offsets, np.uint64) + np.uint64(buf.ctypes.data), C.POINTER(C.c_ubyte), np.uint64)
        else:
            assert buf.is_cuda and buf.dtype.itemsize == 1 and buf.is_contiguous()
            _ko, offs = _ivec(offsets, C.c_size_t, np.uint64)
        if keep_results == "packed" and hasattr(lib, "jdaDetectBatchCppRaggedDeviceRows"):
            # rows straight from the library: no jdaResultD per image, no second copy of 15 MB of rows
            rp, nr = C.POINTER(C.c_double)(), C.c_int(0)
            if host:
                rc = lib.jdaDetectBatchCppRaggedRows(self.h, ptrs, ws, hs, n, minimum_size, step, factor, overlap, 1 if nms else 0, sp,
                                                     frame_offset, C.byref(rp), C.byref(nr))
            else:
                rc = lib.jdaDetectBatchCppRaggedDeviceRows(self.h, C.c_void_p(buf.data_ptr()), offs, ws, hs, n, minimum_size, step,
                                                           factor, overlap, 1 if nms else 0, sp, frame_offset, C.byref(rp), C.byref(nr))
            if rc != 0:
                raise JdaError(last_error())
            out = _owned_rows(rp, nr.value, 6 + self.dim, lib.jdaRowsDRelease, np.float64)
            return (out, st.asdict()) if stats else out
        res = (jdaResultD * max(n, 1))()
        if host:
            rc = lib.jdaDetectBatchCppRagged(self.h, ptrs, ws, hs, n, minimum_size, step, factor, overlap, 1 if nms else 0, sp, res)
        else:
            rc = lib.jdaDetectBatchCppRaggedDevice(self.h, C.c_void_p(buf.data_ptr()), offs, ws, hs, n, minimum_size, step,
                                                   factor, overlap, 1 if nms else 0, sp, res)
        if rc != 0:
            raise JdaError(last_error())
        out = self._collect_d(res, n, keep_results, frame_offset)
        return (out, st.asdict()) if stats else out

    def detect_batch_cpp_pyramid(self, frames, origin_size=48, step=5, factor=1.2, overlap=0.3, nms=True, stats=False,
                                 half_size=0, quarter_size=0):
        """Dialect CPP, detect method 0: the true image pyramid (reference cascador.cpp:216-308).  half_size /
        quarter_size > 0: jdaDetectBatchCppPyramidMS, the per-window patches of a multi-scale model."""
        frames = np.ascontiguousarray(frames, np.uint8)
        if frames.ndim == 2:
            frames = frames[None]
        n, h, w = frames.shape
        ptrs = _frame_ptrs(frames)
        res = (jdaResultD * max(n, 1))()
        st = jdaStats()
        if half_size or quarter_size:
            rc = lib.jdaDetectBatchCppPyramidMS(self.h, ptrs, n, w, h, origin_size, half_size, quarter_size, step, factor, overlap,
                                                1 if nms else 0, C.byref(st), res)
        else:
            rc = lib.jdaDetectBatchCppPyramid(self.h, ptrs, n, w, h, origin_size, step, factor, overlap, 1 if nms else 0,
                                              C.byref(st), res)
        if rc != 0:
            raise JdaError(last_error())
        out = [_take_d(res[i]) for i in range(n)]
        return (out, st.asdict()) if stats else out

    def resize_cv(self, img, out_width, out_height):
        img = np.ascontiguousarray(img, np.uint8)
        h, w = img.shape
        out = np.zeros((out_height, out_width), np.uint8)
        if lib.jdaResizeCv(self.h, _u8(img), w, h, _u8(out), out_width, out_height) != 0:
            raise JdaError(last_error())
        return out

    def validate_cpp(self, images, crops, mode=0, origin_size=48, half_size=36, quarter_size=24, shift_size=0.0, seed=0,
                     stats=False):
        """Validate (reference cascador.cpp:166-211) on caller crops, rows of (image, x, y, w, h): jdaValidateCpp for a list
        of host images, jdaValidateCppDevice for (torch uint8 CUDA buffer, offsets, widths, heights).  mode 0: the mining
        patch chain, 1: detectSingleScale's.  -> dict of is_face, score, carts_n, shape (numpy)."""
        dev, base, offs, ws, hs, n_img, keep = _image_set(images)
        cr = np.ascontiguousarray(np.asarray(crops, np.int32).reshape(-1, 5))
        n = cr.shape[0]
        face = np.zeros(max(n, 1), np.uint8)
        score = np.zeros(max(n, 1), np.float64)
        carts = np.zeros(max(n, 1), np.int32)
        shape = np.zeros((max(n, 1), self.dim), np.float64)
        st = jdaStats()
        args = (cr.ctypes.data_as(C.POINTER(C.c_int)), n, origin_size, half_size, quarter_size, mode, float(shift_size),
                int(seed) & 0xffffffffffffffff, _u8(face), score.ctypes.data_as(C.POINTER(C.c_double)),
                carts.ctypes.data_as(C.POINTER(C.c_int)), shape.ctypes.data_as(C.POINTER(C.c_double)), C.byref(st))
        if dev:
            rc = lib.jdaValidateCppDevice(self.h, base, offs, ws, hs, n_img, *args)
        else:
            rc = lib.jdaValidateCpp(self.h, base, ws, hs, n_img, *args)
        del keep
        if rc != 0:
            raise JdaError(last_error())
        out = dict(is_face=face[:n], score=score[:n], carts_n=carts[:n], shape=shape[:n])
        return (out, st.asdict()) if stats else out

    def mine_negatives_cpp(self, images, steps, factors, transforms, size, start=0, device=False, origin_size=48, half_size=36,
                           quarter_size=24, shift_size=0.0, seed=0, patches=True):
        """Hard-negative mining (reference data.cpp:885-1065): the first `size` windows of NextImage's walk over the
        background images (from window ordinal `start` on) that Validate calls faces.  images: a list of host images, or
        (torch uint8 CUDA buffer, offsets, widths, heights) -- the device entry.  device=True with a host list stages the
        images on the device first (torch) and calls the device entry.  -> dict of hits [n, 4] (image, x, y, win), score,
        shape, o / h / q patch bytes and stats (windows, nega_n, carts_n, next_start, total_windows, hits)."""
        if device and not isinstance(images, tuple):
            images = _pack_images_device(images)
        dev, base, offs, ws, hs, n_img, keep = _image_set(images)
        ks, sp = _ivec(steps)
        kf, fp = _ivec(factors, C.c_double, np.float64)
        kt, tp = _ivec(transforms)
        cap = max(int(size), 1)
        hits = np.zeros((cap, 4), np.int32)
        score = np.zeros(cap, np.float64)
        shape = np.zeros((cap, self.dim), np.float64)
        pt = _patch_bytes(origin_size, half_size, quarter_size)
        pat = np.zeros((cap, pt), np.uint8) if patches else None
        st = jdaMineStats()
        args = (sp, fp, tp, origin_size, half_size, quarter_size, int(start), int(size), float(shift_size),
                int(seed) & 0xffffffffffffffff, hits.ctypes.data_as(C.POINTER(C.c_int)),
                score.ctypes.data_as(C.POINTER(C.c_double)), shape.ctypes.data_as(C.POINTER(C.c_double)),
                _u8(pat) if patches else None, C.byref(st))
        if dev:
            rc = lib.jdaMineNegativesCppDevice(self.h, base, offs, ws, hs, n_img, *args)
        else:
            rc = lib.jdaMineNegativesCpp(self.h, base, ws, hs, n_img, *args)
        del keep, ks, kf, kt
        if rc < 0:
            raise JdaError(last_error())
        out = dict(hits=hits[:rc], score=score[:rc], shape=shape[:rc], stats=st.asdict())
        if patches:
            o2, h2 = origin_size * origin_size, half_size * half_size
            out["patches"] = pat[:rc]       # o, h, q back to back per hit: jdaSamplesCpp's layout (train_cart_cpp)
            out["o"] =pat[:rc, :o2].reshape(rc, origin_size, origin_size)
            out["h"] = pat[:rc, o2:o2 + h2].reshape(rc, half_size, half_size)
            out["q"] = pat[:rc, o2 + h2:].reshape(rc, quarter_size, quarter_size)
        return out

    # -- training one CART (include/jda.h, "Dialect CPP: training one CART") ------------------------------------
    def calc_st_parameters_cpp(self, shapes):
        """jdaCalcSTParametersCpp: DataSet::CalcSTParameters (reference data.cpp:131-146) for [n, 2L] shapes against the
        cascador's mean shape -> (stp_mc, stp_cm), each [n, 5] rows of (scale, rot00, rot01, rot10, rot11); the default
        parameter (1, 1, 0, 0, 1) with the similarity transform off."""
        sh = np.ascontiguousarray(shapes, np.float64).reshape(-1, self.dim)
        n = sh.shape[0]
        mc, cm = np.zeros((max(n, 1), 5), np.float64), np.zeros((max(n, 1), 5), np.float64)
        dp = C.POINTER(C.c_double)
        if lib.jdaCalcSTParametersCpp(self.h, sh.ctypes.data_as(dp) if n else None, n, mc.ctypes.data_as(dp), cm.ctypes.data_as(dp)) != 0:
            raise JdaError(last_error())
        return mc[:n], cm[:n]

    def calc_feature_values_cpp(self, samples, pool, origin_size=48, half_size=36, quarter_size=24):
        """DataSet::CalcFeatureValues (reference data.cpp:148-173): [F, n] int32, row = feature.  samples: dict of patches
        ([n, o*o + h*h + q*q] uint8, numpy or a torch CUDA tensor -- the layout mine_negatives_cpp returns), shapes
        [n, 2L]; pool: FEATURE_DTYPE array."""
        pb = _patch_bytes(origin_size, half_size, quarter_size)
        s, keep = _samples(samples, self.dim, pb)
        fa, fp = _features(pool)
        out = np.zeros((len(fa), s.n), np.int32)
        if lib.jdaCalcFeatureValuesCpp(self.h, C.byref(s), origin_size, half_size, quarter_size, fp, len(fa),
                                       out.ctypes.data_as(C.POINTER(C.c_int))) != 0:
            raise JdaError(last_error())
        del keep
        return out

    def split_node_cpp(self, pos, neg, pool, mode, u=None, origin_size=48, half_size=36, quarter_size=24):
        """Cart::SplitNode's choice over the full sets (reference cart.cpp:176-350): mode 1 classification, 0 regression
        (u: one draw per pool feature) -> dict(feature_idx, threshold, criterion [F] es_ / vs_, thresholds [F] ths_)."""
        pb = _patch_bytes(origin_size, half_size, quarter_size)
        sp, kp = _samples(pos, self.dim, pb)
        sn, kn = _samples(neg, self.dim, pb)
        fa, fp = _features(pool)
        F = len(fa)
        ua = None if u is None else np.ascontiguousarray(u, np.float64).reshape(-1)
        assert ua is None or ua.size == F
        crit = np.zeros(F, np.float64)
        ths = np.zeros(F, np.int32)
        fi, th = C.c_int(), C.c_int()
        rc = lib.jdaSplitNodeCpp(self.h, C.byref(sp), C.byref(sn), origin_size, half_size, quarter_size, fp, F, int(mode),
                                 None if ua is None else ua.ctypes.data_as(C.POINTER(C.c_double)), C.byref(fi), C.byref(th),
                                 crit.ctypes.data_as(C.POINTER(C.c_double)), ths.ctypes.data_as(C.POINTER(C.c_int)))
        del kp, kn
        if rc != 0:
            raise JdaError(last_error())
        return dict(feature_idx=fi.value, threshold=th.value, criterion=crit, thresholds=ths)

    def split_node_sums_cpp(self, pos, neg, pool, mode, u=None, pos_list=None, neg_list=None, origin_size=48, half_size=36,
                            quarter_size=24):
        """jdaSplitNodeSumsCpp: split_node_cpp on the lists pos_list / neg_list (strictly ascending sample indices; None: all
        samples), with what the device wrote for the node -> split_node_cpp's dict plus pos_values [F, P] int16 and
        pos_hist_c [F, 511] int32; mode 1: neg_values [F, N], pos_hist_w / neg_hist_w [F, 511] float64, neg_hist_c; mode 0:
        var_sums [F, 8] float64, var_n_left / var_n_right / var_th [F] int32; chunks."""
        pb = _patch_bytes(origin_size, half_size, quarter_size)
        sp, kp = _samples(pos, self.dim, pb)
        sn, kn = _samples(neg, self.dim, pb)
        fa, fp = _features(pool)
        F = len(fa)
        ua = None if u is None else np.ascontiguousarray(u, np.float64).reshape(-1)
        assert ua is None or ua.size == F
        ip, dp = C.POINTER(C.c_int), C.POINTER(C.c_double)
        pl = None if pos_list is None else np.ascontiguousarray(pos_list, np.int32).reshape(-1)
        nl = None if neg_list is None else np.ascontiguousarray(neg_list, np.int32).reshape(-1)
        P, N = (sp.n if pl is None else pl.size), (sn.n if nl is None else nl.size)
        out = dict(pos_values=np.zeros((F, P), np.int16), pos_hist_c=np.zeros((F, 511), np.int32))
        if mode == 1:
            out.update(neg_values=np.zeros((F, N), np.int16), pos_hist_w=np.zeros((F, 511), np.float64),
                       neg_hist_w=np.zeros((F, 511), np.float64), neg_hist_c=np.zeros((F, 511), np.int32))
        else:
            out.update(var_sums=np.zeros((F, 8), np.float64), var_n_left=np.zeros(F, np.int32), var_n_right=np.zeros(F, np.int32),
                       var_th=np.zeros(F, np.int32))
        sums = jdaSplitSumsCpp()
        for k, a in out.items():
            setattr(sums, k, a.ctypes.data_as(dict(jdaSplitSumsCpp._fields_)[k]))
        crit = np.zeros(F, np.float64)
        ths = np.zeros(F, np.int32)
        fi, th = C.c_int(), C.c_int()
        rc = lib.jdaSplitNodeSumsCpp(self.h, C.byref(sp), C.byref(sn), origin_size, half_size, quarter_size, fp, F, int(mode),
                                     None if ua is None else ua.ctypes.data_as(dp),
                                     None if pl is None else pl.ctypes.data_as(ip), P, None if nl is None else nl.ctypes.data_as(ip), N,
                                     C.byref(fi), C.byref(th), crit.ctypes.data_as(dp), ths.ctypes.data_as(ip), C.byref(sums))
        del kp, kn
        if rc != 0:
            raise JdaError(last_error())
        out.update(feature_idx=fi.value, threshold=th.value, criterion=crit, thresholds=ths, chunks=sums.chunks)
        return out

    def train_cart_cpp(self, pos, neg, pools, modes, us=None, origin_size=48, half_size=36, quarter_size=24):
        """Cart::Train (reference cart.cpp:41-162) with the caller's pools [nodes_n/2 - 1, F], modes [nodes_n/2 - 1] and
        regression draws us [nodes_n/2 - 1, F] -> dict(features, thresholds, scores [leaves], pos_leaf, neg_leaf, nodes
        (NODE_DTYPE per internal node), stats)."""
        pb = _patch_bytes(origin_size, half_size, quarter_size)
        sp, kp = _samples(pos, self.dim, pb)
        sn, kn = _samples(neg, self.dim, pb)
        half = 1 << (self.D - 1)
        inner = half - 1
        fa, fp = _features(pools)
        assert inner > 0 and len(fa) % inner == 0, "pools must hold (nodes_n/2 - 1) * F features"
        F = len(fa) // inner
        md = np.ascontiguousarray(modes, np.int32).reshape(-1)
        assert md.size == inner
        ua = None if us is None else np.ascontiguousarray(us, np.float64).reshape(-1)
        assert ua is None or ua.size == inner * F
        feats = np.zeros(inner, FEATURE_DTYPE)
        ths = np.zeros(inner, np.int32)
        scores = np.zeros(half, np.float64)
        pleaf = np.zeros(max(sp.n, 1), np.int32)
        nleaf = np.zeros(max(sn.n, 1), np.int32)
        nodes = np.zeros(inner, NODE_DTYPE)
        st = jdaTrainStatsCpp()
        st.nodes = nodes.ctypes.data_as(C.POINTER(jdaTrainNodeCpp))
        ip, dp = C.POINTER(C.c_int), C.POINTER(C.c_double)
        rc = lib.jdaTrainCartCpp(self.h, C.byref(sp), C.byref(sn), origin_size, half_size, quarter_size, fp, F,
                                 md.ctypes.data_as(ip), None if ua is None else ua.ctypes.data_as(dp),
                                 feats.ctypes.data_as(C.POINTER(jdaFeatureCpp)), ths.ctypes.data_as(ip), scores.ctypes.data_as(dp),
                                 pleaf.ctypes.data_as(ip), nleaf.ctypes.data_as(ip), C.byref(st))
        del kp, kn
        if rc != 0:
            raise JdaError(last_error())
        stats = {k: getattr(st, k) for k, _ in st._fields_ if k != "nodes"}
        return dict(features=feats, thresholds=ths, scores=scores, pos_leaf=pleaf[:sp.n], neg_leaf=nleaf[:sn.n], nodes=nodes,
                    stats=stats)

    # -- closing a stage (include/jda.h, "Dialect CPP: closing a stage") ------------------------------------------
    def gen_lbf_cpp(self, samples, features, thresholds, origin_size=48, half_size=36, quarter_size=24, K=None):
        """BoostCart::GenLBF (reference btcart.cpp:390-405) over a sample set: [n, K] int32, lbf[i, k] = k * leafNum + the
        leaf of cart k on sample i (the zero-based liblinear index).  samples: the dict calc_feature_values_cpp takes
        (patches numpy or a torch CUDA tensor; weights are not needed); features [K * (nodes_n/2 - 1)] of FEATURE_DTYPE and
        thresholds: K times train_cart_cpp's.  K: only for a cascador of tree_depth 1, whose carts have no split node."""
        pb = _patch_bytes(origin_size, half_size, quarter_size)
        s, keep = _samples(samples, self.dim, pb)
        carts, kc = _stage_carts(features, thresholds, (1 << (self.D - 1)) - 1, K)
        out = np.zeros((s.n, max(carts.K, 0)), np.int32)
        rc = lib.jdaGenLbfCpp(self.h, C.byref(s), origin_size, half_size, quarter_size, C.byref(carts),
                              out.ctypes.data_as(C.POINTER(C.c_int)))
        del keep, kc
        if rc != 0:
            raise JdaError(last_error())
        return out

    def stage_update_shapes_cpp(self, samples, features, thresholds, w, lbf=None, origin_size=48, half_size=36,
                                quarter_size=24, want_lbf=False, stats=False, K=None):
        """The shape update that closes a stage (reference btcart.cpp:285-292, 407-424): shapes + the K rows of w
        [K * leafNum, 2L] the sample's leaf indicators select, added in cart order -> [n, 2L] float64.  lbf=None: the carts
        (features / thresholds as in gen_lbf_cpp) are walked in the same device pass; otherwise lbf [n, K] is used and
        features / thresholds may be None.  want_lbf: also return the indicators; stats: also the call's jdaStageStatsCpp.
        -> shapes, or a tuple (shapes[, lbf][, stats])."""
        pb = _patch_bytes(origin_size, half_size, quarter_size)
        s, keep = _samples(samples, self.dim, pb)
        leaf_n = 1 << (self.D - 1)
        wa = np.ascontiguousarray(w, np.float64)
        if lbf is not None:
            la = np.ascontiguousarray(lbf, np.int32).reshape(s.n, -1) if s.n else np.zeros((0, wa.size // (leaf_n * self.dim)), np.int32)
            if features is None and K is None:
                K = la.shape[1]
        carts, kc = _stage_carts(features, thresholds, leaf_n - 1, K)
        assert wa.size == max(carts.K, 0) * leaf_n * self.dim, "w must hold K * leafNum rows of 2L doubles"
        assert lbf is None or la.shape[1] == carts.K
        out = np.zeros((s.n, self.dim), np.float64)
        olbf = np.zeros((s.n, max(carts.K, 0)), np.int32) if want_lbf else None
        st = jdaStageStatsCpp()
        ip, dp = C.POINTER(C.c_int), C.POINTER(C.c_double)
        rc = lib.jdaStageUpdateShapesCpp(self.h, C.byref(s), origin_size, half_size, quarter_size, C.byref(carts),
                                         wa.ctypes.data_as(dp), None if lbf is None else la.ctypes.data_as(ip),
                                         out.ctypes.data_as(dp), None if olbf is None else olbf.ctypes.data_as(ip), C.byref(st))
        del keep, kc
        if rc != 0:
            raise JdaError(last_error())
        res = (out,) + ((olbf,) if want_lbf else ()) + ((st.asdict(),) if stats else ())
        return res[0] if len(res) == 1 else res

    # -- a stage's global regression (include/jda.h, "Dialect CPP: a stage's global regression") -------------------
    def global_regression_cpp(self, lbf, residual, rows=None, C=0., eps=0., max_iter=0, seed=0):
        """BoostCart::GlobalRegression (reference btcart.cpp:328-388) as include/jda.h defines the fit: lbf [n, K] int32 as
        gen_lbf_cpp writes it, residual [n, 2L] as shape_residual_cpp writes it, rows the used samples in the order they
        enter the problem (None: all n).  C, eps, max_iter <= 0: the reference's defaults (1 / n_rows, 1e-4, 1000).
        -> (w [K * leafNum, 2L] as stage_update_shapes_cpp takes it, iters [2L] int32, gnorm1 [2, 2L], stats dict)."""
        import ctypes                                                   # (the parameter C, named like the reference's, hides the module's alias)
        la = np.ascontiguousarray(lbf, np.int32)
        ra = np.ascontiguousarray(residual, np.float64)
        assert la.ndim == 2 and ra.ndim == 2 and la.shape[0] == ra.shape[0] and ra.shape[1] == self.dim
        n, K = la.shape
        ia = None if rows is None else np.ascontiguousarray(rows, np.int32).reshape(-1)
        n_rows = n if ia is None else int(ia.size)
        par = jdaFitParamsCpp(float(C), float(eps), int(max_iter), int(seed) & 0xffffffffffffffff)
        w = np.zeros((max(K, 0) * (1 << (self.D - 1)), self.dim), np.float64)
        iters = np.zeros(self.dim, np.int32)
        gn = np.zeros((2, self.dim), np.float64)
        st = jdaFitStatsCpp()
        ip, dp = ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_double)
        rc = lib.jdaGlobalRegressionCpp(self.h, la.ctypes.data_as(ip) if la.size else None, ra.ctypes.data_as(dp) if ra.size else None,
                                        n, K, None if ia is None else (ia if ia.size else np.zeros(1, np.int32)).ctypes.data_as(ip), n_rows, ctypes.byref(par),
                                        w.ctypes.data_as(dp), iters.ctypes.data_as(ip), gn.ctypes.data_as(dp), ctypes.byref(st))
        if rc != 0:
            raise JdaError(last_error())
        return w, iters, gn, st.asdict()

    # -- the positive sample set (include/jda.h, "Dialect CPP: the positive sample set") ---------------------------
    def build_positives_cpp(self, images, faces, dst=None, augment=False, origin_size=48, half_size=36, quarter_size=24,
                            stats=False):
        """The patches of the positive set (reference data.cpp:542-565, 623-640; jdaBuildPositivesCpp*): per face row
        (image, x, y, w, h) the o, h and q patches, each a cv::resize of getFace(image, box) (black outside the image),
        and with augment their horizontal mirrors as records n .. 2n - 1.  images: a list of host images, or (torch uint8
        CUDA buffer, offsets, widths, heights).  dst: None (a new numpy array), a writable numpy uint8 array or a torch
        uint8 device tensor of at least size * (o*o + h*h + q*q) bytes -- jdaSamplesCpp's "patches", as train_cart_cpp
        takes them.  -> dst as [size, P] (a view of the caller's buffer), or (dst, stats dict)."""
        pb = _patch_bytes(origin_size, half_size, quarter_size)
        dev, base, offs, ws, hs, n_img, keep = _image_set(images)
        fa = np.ascontiguousarray(np.asarray(faces, np.int32).reshape(-1, 5))
        n = fa.shape[0]
        size = 2 * n if augment else n
        if dst is None:
            dst = np.zeros((size, pb), np.uint8)
        dptr, ddev, dbytes = _byte_buffer(dst, "dst")
        assert dbytes >= size * pb, "dst is too small for the set's records"
        assert ddev or dst.flags.writeable
        st = jdaPositivesStatsCpp()
        args = (fa.ctypes.data_as(C.POINTER(C.c_int)) if n else None, n, origin_size, half_size, quarter_size, 1 if augment else 0,
                dptr, ddev, C.byref(st))
        if dev:
            rc = lib.jdaBuildPositivesCppDevice(self.h, base, offs, ws, hs, n_img, *args)
        else:
            rc = lib.jdaBuildPositivesCpp(self.h, base, ws, hs, n_img, *args)
        del keep
        if rc != 0:
            raise JdaError(last_error())
        out = dst.reshape(-1)[:size * pb].reshape(size, pb)
        return (out, st.asdict()) if stats else out

    # -- from one cart to the next (include/jda.h, "Dialect CPP: from one cart to the next") -----------------------
    def gather_samples_cpp(self, segments, index, dst, keep=None, origin_size=48, half_size=36, quarter_size=24, stats=False):
        """A new dense sample set (jdaGatherSamplesCpp): dst record i = record index[i] of the concatenation of `segments`
        (one buffer or a list of up to 8; each a numpy uint8 array -- a host segment -- or a torch uint8 device tensor, read
        in place, of n * (o*o + h*h + q*q) bytes) for i < keep (default: len(index)).  dst: the caller's buffer of at least
        keep records, a torch device tensor or a writable numpy array; it must not overlap a segment.  Views at any byte
        offset work: the data pointer is what is passed.  -> dst, or (dst, stats dict)."""
        pb = _patch_bytes(origin_size, half_size, quarter_size)
        bufs = list(segments) if isinstance(segments, (list, tuple)) else [segments]
        segs = (jdaGatherSegCpp * max(len(bufs), 1))()
        for i, b in enumerate(bufs):
            ptr, dev, nbytes = _byte_buffer(b, "segment %d" % i)
            assert nbytes % pb == 0, "segment %d does not hold whole records" % i
            segs[i].patches, segs[i].on_device, segs[i].n = ptr, dev, nbytes // pb
        idx = np.ascontiguousarray(index, np.int32).reshape(-1)
        keep = idx.size if keep is None else int(keep)
        assert keep <= idx.size
        dptr, ddev, dbytes = _byte_buffer(dst, "dst")
        assert dbytes >= max(keep, 0) * pb, "dst is too small for keep records"
        assert ddev or dst.flags.writeable
        st = jdaGatherStatsCpp()
        rc = lib.jdaGatherSamplesCpp(self.h, segs, len(bufs), origin_size, half_size, quarter_size,
                                     idx.ctypes.data_as(C.POINTER(C.c_int)) if idx.size else None, keep, dptr, ddev, C.byref(st))
        del bufs
        if rc != 0:
            raise JdaError(last_error())
        return (dst, st.asdict()) if stats else dst

    def trace_cpp(self, frames, minimum_size=20, step=5, factor=1.2):
        frames = np.ascontiguousarray(frames, np.uint8)
        if frames.ndim == 2:
            frames = frames[None]
        n, h, w = frames.shape
        from . import synth
        wpf = synth.count_windows_cpp(w, h, minimum_size, step, factor)
        tot = n * wpf
        carts = np.zeros(tot, np.int32)
        score = np.zeros(tot, np.float64)
        hsh = np.zeros(tot, np.uint32)
        shapes = np.zeros((tot, self.dim), np.float64)
        ptrs = _frame_ptrs(frames)
        rc = lib.jdaTraceBatchCpp(self.h, ptrs, n, w, h, minimum_size, step, factor,
                                  carts.ctypes.data_as(C.POINTER(C.c_int)), score.ctypes.data_as(C.POINTER(C.c_double)),
                                  hsh.ctypes.data_as(C.POINTER(C.c_uint)), shapes.ctypes.data_as(C.POINTER(C.c_double)))
        if rc != 0:
            raise JdaError(last_error())
        return dict(carts_n=carts, score=score, path_hash=hsh, shapes=shapes)
