"""Times packing frames to gray AND reducing them (jdaPackGrayReducedDevice, k_reduce) on 256 x 1920x1080 BGR24 frames resident
in device memory: factors 2, 3 and 4 upright and factor 2 at orientation 1 (a quarter turn).  Per leg one warm-up round, then
the median (min - max) of `--repeats` calls of device_ms (HIP events around the one launch); every leg once per round in one
process.  The yardsticks are taken in the same run -- the parent commit has no reducing path: jdaPackGrayDevice on the same
frames (it reads the same source bytes) and, per leg, a hipMemcpyDtoD of (bytes_in + bytes_out) / 2 bytes, a copy that moves
the traffic the leg moves.  Also reported: the end the feature serves -- the same 256 frames through detect_batch_device at
full resolution and reduced by 2 with min_size halved (windows scanned, ms per batch, the pack's time) -- and, with --headline,
bench.py's headline from a child process of the same session, to show the detect path untouched.

    python tools/reduce_bench.py [--repeats 5] [--headline] [--out profiles/reduce_bench.json]
    python tools/reduce_bench.py --resources profiles/reduce_bench.json     (no GPU: compiles k_reduce.hip with
        -Rpass-analysis=kernel-resource-usage and adds its VGPRs / SGPRs / LDS / scratch / waves per SIMD to that file)
"""
import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from kernel_resources import kernel_resources  # noqa: E402  (tools/kernel_resources.py)

LEGS = ((2, 0), (3, 0), (4, 0), (2, 1))                             # (factor, orientation)


def summary(ms):
    return dict(median=statistics.median(ms), min=min(ms), max=max(ms), all=ms)


def block_means(a, f):
    """include/jda.h's definition on a gray image."""
    rh, rw = a.shape[0] // f, a.shape[1] // f
    S = a[:rh * f, :rw * f].astype(np.int64).reshape(rh, f, rw, f).sum(axis=(1, 3))
    return ((S + f * f // 2) // (f * f)).astype(np.uint8)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--resources", default=None, help="JSON file to add k_reduce's compile-time resource figures to (no GPU needed)")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--headline", action="store_true", help="run bench.py --gpus 1 --steps 50 --warmup 8 --no-cpu afterwards and keep its result line")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.resources:
        res = {}
        if os.path.exists(a.resources):
            with open(a.resources) as f:
                res = json.load(f)
        res["k_reduce_resources"] = kernel_resources("k_reduce.hip", "k_reduce")
        with open(a.resources, "w") as f:
            json.dump(res, f, indent=1)
        print(json.dumps(res["k_reduce_resources"]))
        return
    import torch
    from jda_amd import api, synth
    assert torch.cuda.is_available(), "reduce_bench needs a HIP device"
    W, H, n = 1920, 1080, a.frames
    # bench.py's configs[2] data and model: 32 synthesised frames and cyclic shifts of each, made on the device
    n_base = min(32, n)
    f2 = synth.make_frames(n_base, W, H, seed=0)
    mp2 = os.path.join(synth.cache_dir(), "config2_5_540_27_4.model")
    if not os.path.exists(mp2):
        m2 = synth.make_model(5, 540, 27, 4, seed=1)
        synth.calibrate_thresholds(m2, f2[:4], scale=1.5)
        m2.save(mp2 + ".tmp", 8); os.replace(mp2 + ".tmp", mp2)
    c = api.Cascador(mp2, device=0)
    b2 = torch.from_numpy(f2).cuda()
    d_gray = torch.cat([b2] + [torch.roll(b2, shifts=(131 * j, 257 * j), dims=(1, 2)) for j in range(1, (n + n_base - 1) // n_base)])[:n].contiguous()
    del b2
    bgr = d_gray.unsqueeze(-1).expand(n, H, W, 3).contiguous()      # every channel the gray frame: the pack gives the frames back
    images = [bgr[i] for i in range(n)]
    hip = C.CDLL("libamdhip64.so")
    hip.hipMemcpyDtoD.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
    bytes_in = n * W * H * 3
    src = torch.empty((bytes_in + n * W * H) // 2, dtype=torch.uint8, device="cuda")
    dst = torch.empty_like(src)
    res = dict(repeats=a.repeats, frames=n, width=W, height=H, format="bgr24", legs={})
    packs = []
    times = {leg: [] for leg in LEGS}
    copies = {leg: [] for leg in LEGS}
    stats = {}

    def copy_ms(nbytes):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        assert hip.hipMemcpyDtoD(dst.data_ptr(), src.data_ptr(), nbytes) == 0
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1)
    for r in range(a.repeats + 1):                                   # every leg once per round: the same conditions for all
        _, st = c.pack_gray_device(images, "bgr24", frame_stride=W * H, stats=True)
        assert st["launches"] == 1 and st["bytes_in"] == bytes_in
        if r:
            packs.append(st["device_ms"])
        for leg in LEGS:
            f, t = leg
            rw, rh = api.reduce_size(W, H, f, t)
            (buf, offs, ws, hs), st = c.pack_gray_reduced_device(images, "bgr24", f, t, frame_stride=rw * rh, stats=True)
            assert st["launches"] == 1 and ws == [rw] * n and hs == [rh] * n
            ms = copy_ms((st["bytes_in"] + st["bytes_out"]) // 2)
            if r:
                times[leg].append(st["device_ms"]); copies[leg].append(ms)
            else:                                                    # the warm-up round is also the check against the definition
                stats[leg] = st
                gray = d_gray[[0, n - 1]].cpu().numpy()
                for k, i in enumerate((0, n - 1)):
                    o = int(offs[i])
                    want = block_means(gray[k], f)
                    want = np.ascontiguousarray(np.rot90(want, -1)) if t == 1 else want
                    assert np.array_equal(buf[o:o + rw * rh].cpu().numpy().reshape(rh, rw), want), (leg, i)
    res["pack_gray_device_ms"] = summary(packs)
    res["pack_gray_device_bytes"] = dict(bytes_in=bytes_in, bytes_out=n * W * H)
    for leg in LEGS:
        f, t = leg
        st = stats[leg]
        one = dict(factor=f, orientation=t, bytes_in=st["bytes_in"], bytes_out=st["bytes_out"], reduce_device_ms=summary(times[leg]),
                   memcpy_bytes=(st["bytes_in"] + st["bytes_out"]) // 2, memcpy_dtod_ms=summary(copies[leg]))
        one["ratio_to_pack_gray_device"] = one["reduce_device_ms"]["median"] / res["pack_gray_device_ms"]["median"]
        one["ratio_to_memcpy"] = one["reduce_device_ms"]["median"] / one["memcpy_dtod_ms"]["median"]
        one["GBps_read_plus_written"] = (st["bytes_in"] + st["bytes_out"]) / (one["reduce_device_ms"]["median"] * 1e-3) / 1e9
        res["legs"]["factor_%d_orientation_%d" % leg] = one

    # ---- the end the feature serves: detect at full resolution against pack reduced by 2 + detect with min_size halved
    def detect(frames, min_size):
        for _ in range(2):
            c.detect_batch_device(frames, 1.5, min_size=min_size, keep_results=False)
        torch.cuda.synchronize(); t0 = time.perf_counter()
        for _ in range(3):
            rows, st = c.detect_batch_device(frames, 1.5, min_size=min_size, keep_results="packed", stats=True)
        torch.cuda.synchronize()
        return dict(ms_per_batch=(time.perf_counter() - t0) / 3 * 1e3, windows=int(st["patch_n"]), gpu_ms=st["gpu_ms"], min_size=min_size, max_size=-1,
                    faces=int(len(rows)))
    full = detect(d_gray, 40)
    (buf, offs, ws, hs), st = c.pack_gray_reduced_device(images, "bgr24", 2, 0, frame_stride=(W // 2) * (H // 2), stats=True)
    half = detect(buf[:n * (W // 2) * (H // 2)].view(n, H // 2, W // 2), 20)
    half["pack_device_ms"] = st["device_ms"]; half["pack_call_ms"] = st["call_ms"]
    res["detect"] = dict(scale=1.5, full_resolution=full, reduced_by_2=half,
                         note="max_size -1 is the frame's own bound, which halves with the frame; ms_per_batch is wall time of detect_batch_device alone")
    c.close()
    del bgr, images, d_gray, src, dst, buf
    torch.cuda.empty_cache()
    if a.headline:                                                   # a child of its own: this process holds the GPU open, but idle
        out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "50", "--warmup", "8", "--no-cpu"],
                             capture_output=True, text=True, cwd=ROOT)
        line = [ln for ln in out.stdout.splitlines() if ln.startswith("{")]
        head = json.loads(line[-1]) if line else dict(error=out.stderr[-2000:])
        res["bench_headline"] = {k: head[k] for k in ("metric", "value", "unit", "ms_per_step", "steps", "warmup", "error") if k in head}
    print(json.dumps(res), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
