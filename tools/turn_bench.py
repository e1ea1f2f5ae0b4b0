"""Times packing frames to gray AND turning them (jdaPackGrayOrientedDevice, k_turn) on 256 x 640x480 BGR24 frames resident in
device memory at orientations 0 (forwards to k_pack), 4 (mirror), 1 (a quarter turn) and 7 (transpose).  Per leg one warm-up
call, then the median (min - max) of `--repeats` calls of device_ms (HIP events around the one launch).  In the same run it
times jdaPackGrayDevice on the same frames -- the yardstick: the parent commit has no turning path and the reference turns on
the CPU -- and hipMemcpyDtoD of (bytes_in + bytes_out) / 2 bytes, a copy that moves the same traffic, and reports both ratios.

    python tools/turn_bench.py [--repeats 5] [--out profiles/turn_bench.json]
    python tools/turn_bench.py --resources profiles/turn_bench.json     (no GPU: compiles k_turn.hip with
        -Rpass-analysis=kernel-resource-usage and adds its VGPRs / SGPRs / LDS / scratch / waves per SIMD to that file)
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


def transform(a, t):
    """include/jda.h's numpy equivalents of the orientations timed here."""
    return np.ascontiguousarray({0: a, 4: np.fliplr(a), 1: np.rot90(a, -1), 7: a.T}[t])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--resources", default=None, help="JSON file to add k_turn's compile-time resource figures to (no GPU needed)")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.resources:
        res = {}
        if os.path.exists(a.resources):
            with open(a.resources) as f:
                res = json.load(f)
        res["k_turn_resources"] = kernel_resources("k_turn.hip", "k_turn")
        with open(a.resources, "w") as f:
            json.dump(res, f, indent=1)
        print(json.dumps(res["k_turn_resources"]))
        return
    import torch
    import bench
    from jda_amd import api
    assert torch.cuda.is_available(), "turn_bench needs a HIP device"
    W, H, n = 640, 480, a.frames
    gray = bench.make_frames(n, W, H, seed=0)
    path = bench.model_path((5, 540, 27, 4), "cascade", 1, gray[:4])
    c = api.Cascador(path, device=0)
    hip = C.CDLL("libamdhip64.so")
    hip.hipMemcpyDtoD.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
    d_gray = torch.from_numpy(gray).cuda()
    bgr = d_gray.unsqueeze(-1).expand(n, H, W, 3).contiguous()      # every channel the gray frame: the pack gives the frames back
    images = [bgr[i] for i in range(n)]
    nbytes = n * W * H * 4 // 2
    src = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    dst = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    res = dict(repeats=a.repeats, frames=n, width=W, height=H, format="bgr24", memcpy_bytes=nbytes, legs={})
    packs, copies = [], []
    turns = {t: [] for t in (0, 4, 1, 7)}
    for r in range(a.repeats + 1):                                   # every leg once per round: the same conditions for all
        _, st = c.pack_gray_device(images, "bgr24", frame_stride=W * H, stats=True)
        assert st["launches"] == 1 and (st["bytes_in"] + st["bytes_out"]) // 2 == nbytes
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        assert hip.hipMemcpyDtoD(dst.data_ptr(), src.data_ptr(), nbytes) == 0
        e1.record()
        torch.cuda.synchronize()
        if r:
            packs.append(st["device_ms"]); copies.append(e0.elapsed_time(e1))
        for t in turns:
            (buf, offs, ws, hs), st = c.pack_gray_oriented_device(images, "bgr24", t, frame_stride=W * H, stats=True)
            assert st["launches"] == 1
            if r:
                turns[t].append(st["device_ms"])
            else:                                                    # the warm-up round is also the check against the definition
                for i in (0, n - 1):
                    o = int(offs[i])
                    assert np.array_equal(buf[o:o + W * H].cpu().numpy().reshape(hs[i], ws[i]), transform(gray[i], t)), (t, i)
    res["pack_gray_device_ms"] = summary(packs)
    res["memcpy_dtod_ms"] = summary(copies)
    for t, ms in turns.items():
        one = dict(orientation=t, turn_device_ms=summary(ms))
        one["ratio_to_pack_gray_device"] = one["turn_device_ms"]["median"] / res["pack_gray_device_ms"]["median"]
        one["ratio_to_memcpy"] = one["turn_device_ms"]["median"] / res["memcpy_dtod_ms"]["median"]
        one["GBps_read_plus_write"] = 2 * nbytes / (one["turn_device_ms"]["median"] * 1e-3) / 1e9
        res["legs"]["orientation_%d" % t] = one
    print(json.dumps(res), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
    c.close()


if __name__ == "__main__":
    main()
