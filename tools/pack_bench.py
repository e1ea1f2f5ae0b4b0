"""Times the pack of frames as they arrive into dense gray (jdaPackGrayDevice, k_pack) on three sets resident in device memory:
256 x 640x480 BGR24 at a tight pitch; the same frames as BGRA32 at a pitch of width * 4 + 64; an FDDB-shaped set of 2,845
images of mixed sizes (<= 450 x 450, the size draw of jda_amd.fddb.make_synthetic_fddb) as RGB24.  Per leg one warm-up call, then
the median (min - max) of `--repeats` calls of device_ms (HIP events around the one launch).  In the same run it times
hipMemcpyDtoD of (bytes_in + bytes_out) / 2 bytes -- a copy that moves the same traffic: the yardstick, since the parent commit
has no such path and the reference converts on the CPU -- and reports the ratio to it.  The first leg's pack time is also set
next to the jdaDetectBatchDevice step (gpu_ms and call_ms) on the 256 gray frames it produced, cascade-regime model of the
shipped dimensions.

    python tools/pack_bench.py [--repeats 5] [--out profiles/pack_bench.json]
    python tools/pack_bench.py --resources profiles/pack_bench.json     (no GPU: compiles k_pack.hip with
        -Rpass-analysis=kernel-resource-usage and adds its VGPRs / SGPRs / scratch / waves per SIMD to that file)
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from kernel_resources import kernel_resources  # noqa: E402  (tools/kernel_resources.py)


def summary(ms):
    return dict(median=statistics.median(ms), min=min(ms), max=max(ms), all=ms)


def fddb_sizes(n=2845, seed=0, max_side=450):
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n):
        long_side = int(rng.integers(max_side * 2 // 3, max_side + 1))
        short = int(rng.integers(max_side // 2, long_side + 1))
        out.append((long_side, short) if rng.random() < 0.5 else (short, long_side))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--resources", default=None, help="JSON file to add k_pack's compile-time resource figures to (no GPU needed)")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.resources:
        with open(a.resources) as f:
            res = json.load(f)
        res["k_pack_resources"] = kernel_resources("k_pack.hip", "k_pack")
        with open(a.resources, "w") as f:
            json.dump(res, f, indent=1)
        print(json.dumps(res["k_pack_resources"]))
        return
    import torch
    import bench
    from jda_amd import api, synth
    assert torch.cuda.is_available(), "pack_bench needs a HIP device"
    W, H, n = 640, 480, a.frames
    gray = bench.make_frames(n, W, H, seed=0)
    path = bench.model_path((5, 540, 27, 4), "cascade", 1, gray[:4])
    c = api.Cascador(path, device=0)
    hip = C.CDLL("libamdhip64.so")
    hip.hipMemcpyDtoD.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
    res = dict(repeats=a.repeats, legs={})

    def leg(name, images, fmt, frame_stride=None):
        packs, copies, st = [], [], None
        out = None
        for r in range(a.repeats + 1):
            out, st = c.pack_gray_device(images, fmt, frame_stride=frame_stride, stats=True)
            nbytes = (st["bytes_in"] + st["bytes_out"]) // 2
            if r == 0:
                src = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
                dst = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            assert hip.hipMemcpyDtoD(dst.data_ptr(), src.data_ptr(), nbytes) == 0
            e1.record()
            torch.cuda.synchronize()
            if r:
                packs.append(st["device_ms"]); copies.append(e0.elapsed_time(e1))
        one = dict(images=len(images), format=fmt, pixels=st["pixels"], bytes_in=st["bytes_in"], bytes_out=st["bytes_out"], launches=st["launches"],
                   memcpy_bytes=nbytes, pack_device_ms=summary(packs), memcpy_dtod_ms=summary(copies))
        one["ratio_to_memcpy"] = one["pack_device_ms"]["median"] / one["memcpy_dtod_ms"]["median"]
        one["pack_GBps_read_plus_write"] = (st["bytes_in"] + st["bytes_out"]) / (one["pack_device_ms"]["median"] * 1e-3) / 1e9
        res["legs"][name] = one
        print(name, json.dumps(one), flush=True)
        return out

    # 1. BGR24, tight pitch: every channel the gray frame, so the pack gives the frames back and the detect step sees real frames
    d_gray = torch.from_numpy(gray).cuda()
    bgr = d_gray.unsqueeze(-1).expand(n, H, W, 3).contiguous()
    buf, offs, ws, hs = leg("bgr24_256x640x480_tight", [bgr[i] for i in range(n)], "bgr24", frame_stride=W * H)
    packed = buf.view(n, H, W)
    assert torch.equal(packed, d_gray)
    steps = []
    for r in range(a.repeats + 1):
        _, st = c.detect_batch_device(packed, keep_results=False, stats=True)
        if r:
            steps.append((st["gpu_ms"], st["call_ms"]))
    res["detect_step_same_frames"] = dict(gpu_ms=summary([s[0] for s in steps]), call_ms=summary([s[1] for s in steps]))
    res["pack_over_detect_gpu_ms"] = res["legs"]["bgr24_256x640x480_tight"]["pack_device_ms"]["median"] / res["detect_step_same_frames"]["gpu_ms"]["median"]
    print("detect", json.dumps(res["detect_step_same_frames"]), flush=True)
    del bgr

    # 2. BGRA32, rows width * 4 + 64 bytes apart
    pitch = W * 4 + 64
    plane = torch.zeros(n * H * pitch, dtype=torch.uint8, device="cuda")
    rows = torch.as_strided(plane, (n, H, W, 4), (H * pitch, pitch, 4, 1))
    rows.copy_(d_gray.unsqueeze(-1).expand(n, H, W, 4))
    buf, offs, ws, hs = leg("bgra32_256x640x480_pitch_plus_64", [rows[i] for i in range(n)], "bgra32", frame_stride=W * H)
    assert torch.equal(buf.view(n, H, W), d_gray)
    del plane, rows, buf, packed, d_gray

    # 3. FDDB-shaped: 2,845 images of mixed sizes, RGB24, back to back in one allocation
    sizes = fddb_sizes()
    starts, tot = [], 0
    for w, h in sizes:
        starts.append(tot); tot += w * h * 3
    g = torch.Generator(device="cuda").manual_seed(1)
    pool = torch.randint(0, 256, (tot,), dtype=torch.uint8, device="cuda", generator=g)
    images = [torch.as_strided(pool, (h, w, 3), (w * 3, 3, 1), s) for (w, h), s in zip(sizes, starts)]
    buf, offs, ws, hs = leg("rgb24_fddb_2845_mixed", images, "rgb24")
    for i in (0, 1, 1422, 2844):                          # a sample against the definition
        v = images[i].cpu().numpy().astype(np.int64)
        want = ((v[..., 0] * 4899 + v[..., 1] * 9617 + v[..., 2] * 1868 + 8192) >> 14).astype(np.uint8)
        o = int(offs[i])
        assert np.array_equal(buf[o:o + want.size].cpu().numpy().reshape(want.shape), want)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
    c.close()


if __name__ == "__main__":
    main()
