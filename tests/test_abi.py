"""The C-ABI shared library: loads without a GPU, exports every symbol that
include/jda.h declares, the header is valid C, and a plain C program can link it."""
import ctypes as C
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "jda.h")

REFERENCE_SYMBOLS = ["jdaCascadorCreateDouble", "jdaCascadorCreateFloat", "jdaCascadorSerializeTo",
                     "jdaCascadorRelease", "jdaDetect", "jdaResultRelease"]    # reference c/jda.h:31-68


def declared_symbols():
    src = open(HEADER).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return re.findall(r"JDA_API\s+[^;(]*?\b(jda\w+)\s*\(", src)


def test_every_declared_symbol_is_exported(built):
    from jda_amd import api
    names = declared_symbols()
    assert set(REFERENCE_SYMBOLS) <= set(names)
    assert len(names) >= 15
    assert {"jdaSplitNodeCpp", "jdaSplitNodeSumsCpp", "jdaTrainCartCpp"} <= set(names)
    for n in names:
        assert hasattr(api.lib, n), n


def test_finish_forms_entry_and_its_python_mirror(built, model_file):
    """jdaFinishForms (include/jda.h): exported, JDA_FINISH_FORM_N counts in the header's order, all zero on a cascador
    that has run nothing, null arguments refused.  No GPU needed: the counts live in the host object."""
    from jda_amd import api
    assert "jdaFinishForms" in declared_symbols()
    src = open(HEADER).read()
    names = re.findall(r"\bJDA_FINISH_(\w+?)\s*(?:=\s*0\s*)?,", src[src.index("JDA_FINISH_WIDE_CONC"):src.index("JDA_FINISH_FORM_N")])
    assert tuple(names) == api.FINISH_FORMS and len(names) == 7
    p, _ = model_file((2, 8, 5, 3), 8, seed=1)
    c = api.Cascador(p)
    assert c.finish_forms() == dict.fromkeys(api.FINISH_FORMS, 0)
    assert api.lib.jdaFinishForms(c.h, None) == -1 and api.lib.jdaFinishForms(None, (C.c_longlong * 7)()) == -1
    c.close()


def test_scan_forms_entry_and_its_python_mirror(built, model_file):
    """jdaScanForms (include/jda.h): exported, JDA_SCAN_FORM_N counts indexed by JDA_SCAN_FORM, which the Python mirror
    (api.ScanForm.index) restates field for field; all zero on a cascador that has run nothing; null arguments refused."""
    from jda_amd import api
    assert "jdaScanForms" in declared_symbols()
    src = open(HEADER).read()
    assert int(re.search(r"#define JDA_SCAN_FORM_N (\d+)", src).group(1)) == api.SCAN_FORM_N
    args = re.search(r"#define JDA_SCAN_FORM\(([^)]*)\)", src).group(1).replace(" ", "").split(",")
    assert tuple(args) == tuple(f for f, _ in api.SCAN_FORM_FIELDS) == api.ScanForm._fields
    for field, values, enum in (("kernel", ("k_scan", "k_scan_p"), ("JDA_SCAN_K_SCAN", "JDA_SCAN_K_SCAN_P")),
                                ("depth", (4, 6, 0), ("JDA_SCAN_DEPTH_4", "JDA_SCAN_DEPTH_6", "JDA_SCAN_DEPTH_GENERIC")),
                                ("pix", ("T16_256", "T16_512", "T21", "GLB"), ("JDA_SCAN_T16_256", "JDA_SCAN_T16_512", "JDA_SCAN_T21", "JDA_SCAN_GLB"))):
        assert dict(api.SCAN_FORM_FIELDS)[field] == values
        for i, e in enumerate(enum):
            assert int(re.search(r"\b%s = (\d+)" % e, src).group(1)) == i, e
    p, _ = model_file((2, 8, 5, 3), 8, seed=1)
    c = api.Cascador(p)
    assert c.scan_forms() == {}
    assert api.lib.jdaScanForms(c.h, None) == -1 and api.lib.jdaScanForms(None, (C.c_longlong * api.SCAN_FORM_N)()) == -1
    c.close()


def test_finish_launches_entries_and_their_python_mirror(built, model_file):
    """jdaFinishLaunches and jdaFinishTileWin (include/jda.h): exported; JDA_FINISH_LAUNCH_N counts indexed by
    JDA_FINISH_LAUNCH, which the Python mirror (api.FinishLaunch.index) restates field for field -- checked against the
    macro itself, evaluated from the header's text; all zero on a cascador that has run nothing; null arguments and an unknown
    dialect refused.  No GPU needed: counts and model live in the host object."""
    from jda_amd import api
    assert {"jdaFinishLaunches", "jdaFinishTileWin"} <= set(declared_symbols())
    src = open(HEADER).read()
    assert int(re.search(r"#define JDA_FINISH_LAUNCH_N (\d+)", src).group(1)) == api.FINISH_LAUNCH_N == 2 * 2 * 2 * 5 * 2 ** 6
    mac = re.search(r"#define JDA_FINISH_LAUNCH\(([^)]*)\)\s*\\\n(.*)\n", src)
    args = mac.group(1).replace(" ", "").split(",")
    assert tuple(args) == tuple(f for f, _ in api.FINISH_LAUNCH_FIELDS) == api.FinishLaunch._fields
    for i, e in enumerate(("JDA_FINISH_K_FINISH", "JDA_FINISH_K_FILTER0")):
        assert int(re.search(r"\b%s = (\d+)" % e, src).group(1)) == i, e
    assert dict(api.FINISH_LAUNCH_FIELDS)["kernel"] == ("k_finish", "k_filter0") and dict(api.FINISH_LAUNCH_FIELDS)["groups"] == (0, 1, 2, 3, 4)
    body = re.sub(r"\b(%s)\b" % "|".join(args), lambda m_: "a[%r]" % m_.group(1), mac.group(2))      # the macro's body is integer arithmetic
    seen = set()
    for i in range(api.FINISH_LAUNCH_N):
        f = api.FinishLaunch.of_index(i)
        a = {n: dict(api.FINISH_LAUNCH_FIELDS)[n].index(v) for n, v in zip(api.FinishLaunch._fields, f)}
        assert f.index() == i == eval(body, {"a": a}), f
        seen.add(f)
    assert len(seen) == api.FINISH_LAUNCH_N
    p, _ = model_file((2, 8, 5, 3), 8, seed=1)
    c = api.Cascador(p)
    assert c.finish_launches() == {}
    assert api.lib.jdaFinishLaunches(c.h, None) == -1 and api.lib.jdaFinishLaunches(None, (C.c_longlong * api.FINISH_LAUNCH_N)()) == -1
    # dim 10, K 8: (10 * real + 8 * 4 + 64) bytes in front of the tile, the largest tw with tw * ((tw + 3) & ~3) + 16 <= 7,680 - that
    want = {rb: max(tw for tw in range(16, 256) if 10 * rb + 8 * 4 + 64 + tw * ((tw + 3) & ~3) + 16 <= 7680) for rb in (4, 8)}
    assert want == {4: 85, 8: 85}          # (85 x 88 + 16 = 7,496 fits either; 86 x 88 + 16 = 7,584 neither)
    assert c.finish_tile_win("C") == want[4] and c.finish_tile_win("CPP") == want[8]
    assert api.lib.jdaFinishTileWin(None, 0) == -1 and api.lib.jdaFinishTileWin(c.h, 2) == -1
    c.close()


def test_mine_launches_entry_and_its_python_mirror(built, model_file):
    """jdaMineLaunches (include/jda.h): exported, JDA_MINE_LAUNCH_N counts in the header's order, which api.MINE_LAUNCH_FIELDS
    restates name for name; all zero on a cascador that has run nothing; null arguments refused.  No GPU needed."""
    from jda_amd import api
    assert "jdaMineLaunches" in declared_symbols()
    src = open(HEADER).read()
    enum = src[src.index("enum { JDA_MINE_K_SCAN"):src.index("JDA_API int jdaMineLaunches")]
    names = re.findall(r"\bJDA_MINE_(\w+) = (\d+)", enum)
    assert [int(v) for _, v in names] == list(range(len(names)))
    assert names[-1] == ("LAUNCH_N", str(api.MINE_LAUNCH_N)) and api.MINE_LAUNCH_N == 12
    assert tuple(n.lower() for n, _ in names[:-1]) == api.MINE_LAUNCH_FIELDS
    p, _ = model_file((2, 8, 5, 3), 8, seed=1)
    c = api.Cascador(p)
    assert c.mine_launches() == dict.fromkeys(api.MINE_LAUNCH_FIELDS, 0)
    assert api.lib.jdaMineLaunches(c.h, None) == -1 and api.lib.jdaMineLaunches(None, (C.c_longlong * api.MINE_LAUNCH_N)()) == -1
    c.close()


def test_stage_launches_entries_and_their_python_mirror(built, model_file):
    """jdaStageLaunches and jdaStageLaunchFor (include/jda.h): exported; JDA_STAGE_LAUNCH_N counts indexed by JDA_STAGE_LAUNCH,
    which the Python mirror (api.StageLaunch.index) restates field for field -- checked against the macro itself, evaluated
    from the header's text; nothing counted on a cascador that has run nothing; null arguments, an unknown dialect, a window
    or step below 1, a declined model and a declined dialect refused.  No GPU needed."""
    from jda_amd import api, synth
    assert {"jdaStageLaunches", "jdaStageLaunchFor"} <= set(declared_symbols())
    src = open(HEADER).read()
    assert int(re.search(r"#define JDA_STAGE_LAUNCH_N (\d+)", src).group(1)) == api.STAGE_LAUNCH_N == 2 * 2 * 2 * 4 * 5
    mac = re.search(r"#define JDA_STAGE_LAUNCH\(([^)]*)\)\s*\\\n(.*)\n", src)
    args = mac.group(1).replace(" ", "").split(",")
    assert tuple(args) == tuple(f for f, _ in api.STAGE_LAUNCH_FIELDS) == api.StageLaunch._fields
    for field, values, fmt in (("acc", (12, 32, 64, 160), "JDA_STAGE_ACC_%d"), ("chunk", (4, 8, 16, 32, 64), "JDA_STAGE_CHUNK_%d")):
        assert dict(api.STAGE_LAUNCH_FIELDS)[field] == values
        for i, v in enumerate(values):
            assert int(re.search(r"\b%s = (\d+)" % (fmt % v), src).group(1)) == i, (field, v)
    body = re.sub(r"\b(%s)\b" % "|".join(args), lambda m_: "a[%r]" % m_.group(1), mac.group(2))      # the macro's body is integer arithmetic
    seen = set()
    for i in range(api.STAGE_LAUNCH_N):
        f = api.StageLaunch.of_index(i)
        a = {n: dict(api.STAGE_LAUNCH_FIELDS)[n].index(v) for n, v in zip(api.StageLaunch._fields, f)}
        assert f.index() == i == eval(body, {"a": a}), f
        seen.add(f)
    assert len(seen) == api.STAGE_LAUNCH_N
    p, _ = model_file((2, 8, 5, 3), 8, seed=1)
    c = api.Cascador(p)
    assert c.stage_launches() == {}
    assert api.lib.jdaStageLaunches(c.h, None) == -1 and api.lib.jdaStageLaunches(None, (C.c_longlong * api.STAGE_LAUNCH_N)()) == -1
    lds = C.c_int(-7)
    # dim 10, 3 nodes and 4 leaves a tree, 24-pixel windows 2 apart: a 64 x 54 byte tile; the smallest tier (32 KB) holds
    # 64-cart chunks in fp32 (32,176 bytes) and 16-cart chunks in fp64 (32,480; 32 carts: 40,928)
    lds_of = lambda rb, nb, ch: 3456 + 10 * 256 * rb + ch * 3 * nb + ch * 4 * rb + ch * 4 * rb + (((ch * 4 * 10 + 12) * rb + 15) & ~15)
    assert (lds_of(4, 32, 64), lds_of(8, 48, 16), lds_of(8, 48, 32)) == (32176, 32480, 40928) and 32480 <= 32768 < 40928
    for dial, rb, nb, ch in (("C", 4, 32, 64), ("CPP", 8, 48, 16)):
        for trace in (False, True):
            assert c.stage_launch_for(dial, trace, 24, 2) == (api.StageLaunch(dial, trace, False, 12, ch), lds_of(rb, nb, ch)), (dial, trace)
    assert c.stage_launch_for("C", False, 150, 15)[0] == api.StageLaunch("C", False, True, 12, 64)
    assert api.lib.jdaStageLaunchFor(c.h, 0, 0, 24, 2, None) == api.StageLaunch("C", False, False, 12, 64).index()     # (lds_bytes may be null)
    for bad in ((None, 0, 0, 24, 2), (c.h, 2, 0, 24, 2), (c.h, -1, 0, 24, 2), (c.h, 0, 0, 0, 2), (c.h, 0, 0, 24, 0)):
        assert api.lib.jdaStageLaunchFor(*bad, C.byref(lds)) == -1 and lds.value == -7, bad
    for bad in (("C", False, 0, 2), ("C", False, 24, 0), (2, False, 24, 2)):      # the Python mirror: bad arguments raise, a declined model is None
        with pytest.raises(api.JdaError):
            c.stage_launch_for(*bad)
    c.set_similarity_transform(True)                       # declines dialect CPP alone
    assert c.stage_launch_for("CPP", False, 24, 2) is None and c.stage_launch_for("C", False, 24, 2) is not None
    c.close()
    for dims, kw in (((2, 3, 78, 2), {}), ((2, 3, 2, 10), {}), ((2, 3, 5, 3), dict(multi_scale=True))):      # LDS floor, 512 leaves, multi-scale
        p, _ = model_file(dims, 8, seed=1, **kw)
        c = api.Cascador(p)
        assert c.stage_launch_for("C", False, 24, 2) is None and c.stage_launch_for("CPP", True, 24, 2) is None, dims
        c.close()


def test_header_is_plain_c_and_links(built, tmp_path):
    """What a maintainer of the reference would do: compile a C caller against
    include/jda.h and link libjda.so (no torch, no C++)."""
    from jda_amd import api
    src = tmp_path / "caller.c"
    src.write_text(r'''
#include <stdio.h>
#include "jda.h"
int main(void) {
  void *c = jdaCascadorCreateDouble("/nonexistent.model");
  if (c != NULL) return 1;                      /* NULL on a missing file, c/jda.c:487-488 */
  long long n = 0; int levels = 0;
  if (jdaCountWindows(640, 480, 1.25f, 40, -1, &n, &levels) != 0) return 2;
  printf("%lld %d\n", n, levels);
  jdaResult r = {0, 0, NULL, NULL, NULL};
  jdaResultRelease(r);                          /* free(NULL) is fine */
  jdaCascadorRelease(NULL);
  return 0;
}
''')
    exe = tmp_path / "caller"
    libdir = os.path.dirname(api.LIB_PATH)
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src),
                           "-o", str(exe), "-L", libdir, "-l:libjda.so", "-Wl,-rpath," + libdir])
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    assert out.stdout.split() == ["38245", "11"]


def test_stats_struct_matches_its_ctypes_mirror(built, tmp_path):
    """jdaStats grows at its end only (callers compiled against an older header keep their offsets): the last fields in
    the order they were added, and every field of jda_amd.api.jdaStats at the offset a C compiler gives it."""
    from jda_amd import api
    names = [k for k, _ in api.jdaStats._fields_]
    assert names[-4:] == ["scan_fallbacks", "ws_regrows", "post_passes", "post_declined"]
    src = tmp_path / "stats.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "jda.h"\nint main(void) {\n' +
                   "".join('  printf("%s %%zu\\n", offsetof(jdaStats, %s));\n' % (k, k) for k in names) +
                   '  printf("sizeof %zu\\n", sizeof(jdaStats));\n  return 0;\n}\n')
    exe = tmp_path / "stats"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    out = dict(l.split() for l in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines())
    for k in names:
        assert int(out[k]) == getattr(api.jdaStats, k).offset, k
    assert int(out["sizeof"]) == C.sizeof(api.jdaStats)
    st = api.jdaStats()
    assert st.post_passes == 0 and st.post_declined == 0 and {"post_passes", "post_declined"} <= set(st.asdict())


def test_detect_without_gpu_fails_loudly(built, model_file):
    """No CPU fallback: on a box without a HIP device the detect entry must raise, not
    quietly compute elsewhere."""
    import numpy as np
    import torch
    from jda_amd import api
    if torch.cuda.is_available():
        pytest.skip("a HIP device is present")
    p, _ = model_file((2, 8, 5, 3), 8)
    c = api.Cascador(p)
    with pytest.raises(api.JdaError, match="no usable HIP device"):
        c.detect(np.zeros((64, 64), np.uint8))
    with pytest.raises(api.JdaError):
        c.detect_batch(np.zeros((2, 64, 64), np.uint8))
    with pytest.raises(api.JdaError):
        c.trace(np.zeros((64, 64), np.uint8))


def test_product_never_touches_the_oracle():
    """oracle/ is test infrastructure: nothing under jda_amd/ may import or load it."""
    pkg = os.path.join(ROOT, "jda_amd")
    for dp, _, fs in os.walk(pkg):
        for f in fs:
            if f.endswith((".py", ".cpp", ".hip", ".h")):
                txt = open(os.path.join(dp, f), errors="ignore").read()
                assert "pyoracle" not in txt and "libjda_oracle" not in txt and "oracle/_ref" not in txt, f
                assert not re.search(r"^\s*(from|import)\s+oracle\b", txt, flags=re.M), f
    deps = subprocess.run(["readelf", "-d", os.path.join(pkg, "libjda.so")], capture_output=True, text=True).stdout
    assert "oracle" not in deps


def test_cmake_target_builds_the_same_library(tmp_path):
    """CMakeLists.txt (shape of reference c/CMakeLists.txt:19-22): one shared library exporting c/jda.h
    plus the demo driver, built without Python."""
    import shutil
    if not shutil.which("cmake") or not os.path.exists("/opt/rocm/bin/hipcc"):
        pytest.skip("cmake or hipcc not available")
    b = str(tmp_path / "b")
    gen = ["-G", "Ninja"] if shutil.which("ninja") else []
    subprocess.check_call(["cmake", "-S", ROOT, "-B", b] + gen, stdout=subprocess.DEVNULL)
    subprocess.check_call(["cmake", "--build", b, "-j", "8"], stdout=subprocess.DEVNULL)
    lib = C.CDLL(os.path.join(b, "libjda.so"))
    for n in declared_symbols():
        assert hasattr(lib, n), n
    assert os.path.exists(os.path.join(b, "jda-test"))


def test_dist_library_exports_its_header(built):
    """libjda_dist.so (RCCL gather of detection rows): loads without a GPU and exports every symbol of include/jda_dist.h;
    libjda.so itself does not depend on RCCL."""
    from jda_amd import build as lib_build
    from jda_amd import dist as jd
    lib_build.build_dist()
    src = open(os.path.join(ROOT, "include", "jda_dist.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    names = re.findall(r"JDA_API\s+[^;(]*?\b(jda\w+)\s*\(", src)
    assert len(names) >= 9
    L = jd.dist_lib()
    for n in names:
        assert hasattr(L, n), n
    deps = subprocess.run(["readelf", "-d", os.path.join(ROOT, "jda_amd", "libjda.so")], capture_output=True, text=True).stdout
    assert "rccl" not in deps and "torch" not in deps


def test_options_round_trip_and_start_from_the_environment(built, model_file, monkeypatch):
    """jdaSetOption / jdaGetOption (include/jda.h): per cascador, seeded ONCE from JDA_<KEY> when the cascador is created,
    unknown keys refused.  No GPU needed: the options live in the host object."""
    from jda_amd import api
    p, _ = model_file((2, 8, 5, 3), 8, seed=1)
    documented = {"handoff": 128, "lanes": 2, "dense": 1, "plan_cache": 64, "predict": 1, "wide_max": 1024,
                  "ragged_chunk_windows": 4000000, "ragged_chunk_windows_cpp": 8000000, "filter0": 1,
                  "kernel_d2h": 1, "h2d_stream": 1, "h2d_min_bytes": 8 << 20,
                  "ragged_chunk_min_windows": 1500000, "ragged_split": 3, "ragged_single_windows": 5000000,
                  "scan_p": 1, "scan_p_slots": 5, "device_post": 1, "device_post_min_frames": 16,
                  "w_pad": 1, "w_stream_mb": 8, "lm_deep": 1, "max_lanes": 16, "hwq_place": 1, "ws_bound": 1, "ws_factor_pct": 400, "ws_min_entries": 65536}
    for k in list(os.environ):
        if k.startswith("JDA_") and k not in ("JDA_LIB_PATH",):
            monkeypatch.delenv(k)
    c = api.Cascador(p)
    for k, v in documented.items():
        assert c.get_option(k) == v, k
    monkeypatch.setenv("JDA_HANDOFF", "96"); monkeypatch.setenv("JDA_H2D_STREAM", "2")
    c2 = api.Cascador(p)                                   # the environment is read when the cascador is created ...
    assert c2.get_option("handoff") == 96 and c2.get_option("h2d_stream") == 2
    assert c.get_option("handoff") == 128                  # ... and only then
    monkeypatch.setenv("JDA_HANDOFF", "64")
    assert c2.get_option("handoff") == 96
    c2.set_option("handoff", 112)
    assert c2.get_option("handoff") == 112 and c.get_option("handoff") == 128
    for k in ("scan_p_tile_kb", "scan_p_grid", "ragged_chunk_min_windows", "workspace_mb"):      # sizes and counts: no negative values
        with pytest.raises(api.JdaError):
            c.set_option(k, -1)
    with pytest.raises(api.JdaError):
        c.set_option("no_such_option", 1)
    assert api.lib.jdaGetOption(c.h, b"no_such_option") == -1
    c.close(); c2.close()


def test_no_exception_crosses_the_c_abi(built, tmp_path):
    """Reference behaviour on an allocation failure: NULL / nothing, never a crash (c/jda.c:487-493).  Every extern "C"
    entry of abi.cpp is a function-try-block; the `test_throw` option makes jdaDetectBatch throw inside it -- the call
    returns -1 (jdaDetect: an empty result), jdaGetLastError says why, and the process lives."""
    import numpy as np
    from jda_amd import api, synth
    p = str(tmp_path / "m.model")
    synth.make_model(2, 8, 5, 3, seed=1).save(p, 8)
    c = api.Cascador(p)
    frames = synth.make_frames(2, 64, 48, seed=1)
    for code, text in ((1, "out of host memory"), (2, "injected by test_throw")):
        c.set_option("test_throw", code)
        with pytest.raises(api.JdaError, match=text):
            c.detect_batch(frames)
        assert "jdaDetectBatch" in api.last_error()
        img = np.ascontiguousarray(frames[0])
        r = api.lib.jdaDetect(c.h, img.ctypes.data_as(C.POINTER(C.c_ubyte)), 64, 48, 1.25, 0.1, 24, -1, -0.5)
        assert r.n == 0 and r.landmark_n == 5 and text in api.last_error()
        api.lib.jdaResultRelease(r)
    c.set_option("test_throw", 0)
    # the cascador is still usable: nothing was left locked or pinned by the unwinding
    assert c.get_option("test_throw") == 0
    c.set_option("handoff", 64)
    c.close()
    # a model file that cannot be read is NULL + a reason, as before
    with pytest.raises(api.JdaError):
        api.Cascador(str(tmp_path / "missing.model"))
