"""Times packing frames to gray AND rotating them (jdaPackGrayRotatedDevice, k_rotate) on 256 x 640x480 BGR24 frames resident in
device memory, at 30 and at 45 degrees.  One warm-up round -- which also checks two frames per leg against the host form
(jdaPackGrayRotated) --, then the median (min - max) of `--repeats` calls of device_ms (HIP events around the one launch); every
leg once per round in one process.  The yardsticks are taken in the same run -- the parent commit has no rotating path:
jdaPackGrayOrientedDevice at orientation 1 (a quarter turn) on the same frames and, per leg, a hipMemcpyDtoD of
(bytes_in + bytes_out) / 2 bytes, a copy that moves the traffic the leg moves.  With --headline, bench.py's headline from a
child process of the same session, to show the detect path untouched.

    python tools/rotate_bench.py [--repeats 5] [--headline] [--out profiles/rotate_bench.json]
    python tools/rotate_bench.py --resources profiles/rotate_bench.json     (no GPU: compiles k_rotate.hip with
        -Rpass-analysis=kernel-resource-usage and adds its VGPRs / SGPRs / LDS / scratch / waves per SIMD to that file)
"""
import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from kernel_resources import kernel_resources  # noqa: E402  (tools/kernel_resources.py)

LEGS = (30.0, 45.0)                                                  # degrees


def summary(ms):
    return dict(median=statistics.median(ms), min=min(ms), max=max(ms), all=ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--resources", default=None, help="JSON file to add k_rotate's compile-time resource figures to (no GPU needed)")
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
        res["k_rotate_resources"] = kernel_resources("k_rotate.hip", "k_rotate")
        with open(a.resources, "w") as f:
            json.dump(res, f, indent=1)
        print(json.dumps(res["k_rotate_resources"]))
        return
    import torch
    from jda_amd import api, synth
    assert torch.cuda.is_available(), "rotate_bench needs a HIP device"
    W, H, n = 640, 480, a.frames
    n_base = min(32, n)
    f0 = synth.make_frames(n_base, W, H, seed=0)
    mp = os.path.join(synth.cache_dir(), "rotate_bench_2_8_5_3.model")   # (no model is read by a pack entry: any cascador serves)
    if not os.path.exists(mp):
        synth.make_model(2, 8, 5, 3, seed=1).save(mp + ".tmp", 8); os.replace(mp + ".tmp", mp)
    c = api.Cascador(mp, device=0)
    b0 = torch.from_numpy(f0).cuda()
    d_gray = torch.cat([b0] + [torch.roll(b0, shifts=(131 * j, 257 * j), dims=(1, 2)) for j in range(1, (n + n_base - 1) // n_base)])[:n].contiguous()
    del b0
    rng = np.random.default_rng(0)
    bgr = torch.from_numpy(rng.integers(0, 256, (n, H, W, 3), dtype=np.uint8)).cuda()   # real colour: the gray of every tap is computed
    bgr[..., 1] = d_gray
    images = [bgr[i] for i in range(n)]
    hip = C.CDLL("libamdhip64.so")
    hip.hipMemcpyDtoD.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
    bytes_in = n * W * H * 3
    src = torch.empty(bytes_in, dtype=torch.uint8, device="cuda")
    dst = torch.empty_like(src)
    res = dict(repeats=a.repeats, frames=n, width=W, height=H, format="bgr24", legs={})
    turns, turn_copies = [], []
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
        _, st = c.pack_gray_oriented_device(images, "bgr24", 1, frame_stride=W * H, stats=True)
        assert st["launches"] == 1 and st["bytes_in"] == bytes_in
        ms = copy_ms((st["bytes_in"] + st["bytes_out"]) // 2)
        if r:
            turns.append(st["device_ms"]); turn_copies.append(ms)
        for leg in LEGS:
            p = api.rotation_plan(W, H, leg)
            tw, th = p["tw"], p["th"]
            (buf, offs, ws, hs), st = c.pack_gray_rotated_device(images, "bgr24", leg, frame_stride=tw * th, stats=True)
            assert st["launches"] == 1 and ws == [tw] * n and hs == [th] * n and st["bytes_in"] == bytes_in
            ms = copy_ms((st["bytes_in"] + st["bytes_out"]) // 2)
            if r:
                times[leg].append(st["device_ms"]); copies[leg].append(ms)
            else:                                                    # the warm-up round is also the check against the host form
                stats[leg] = st
                for i in (0, n - 1):
                    o = int(offs[i])
                    want = api.pack_gray_rotated([bgr[i].cpu().numpy()], "bgr24", leg)[0]
                    assert np.array_equal(buf[o:o + tw * th].cpu().numpy().reshape(th, tw), want), (leg, i)
    res["pack_gray_oriented_device_ms"] = summary(turns)
    res["pack_gray_oriented_device"] = dict(orientation=1, bytes_in=bytes_in, bytes_out=n * W * H, memcpy_dtod_ms=summary(turn_copies))
    for leg in LEGS:
        st = stats[leg]
        one = dict(degrees=leg, bytes_in=st["bytes_in"], bytes_out=st["bytes_out"], rotate_device_ms=summary(times[leg]),
                   memcpy_bytes=(st["bytes_in"] + st["bytes_out"]) // 2, memcpy_dtod_ms=summary(copies[leg]))
        one["ratio_to_pack_gray_oriented_device"] = one["rotate_device_ms"]["median"] / res["pack_gray_oriented_device_ms"]["median"]
        one["ratio_to_memcpy"] = one["rotate_device_ms"]["median"] / one["memcpy_dtod_ms"]["median"]
        one["GBps_read_plus_written"] = (st["bytes_in"] + st["bytes_out"]) / (one["rotate_device_ms"]["median"] * 1e-3) / 1e9
        one["Gpixels_per_s"] = st["pixels"] / (one["rotate_device_ms"]["median"] * 1e-3) / 1e9
        res["legs"]["degrees_%g" % leg] = one
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
