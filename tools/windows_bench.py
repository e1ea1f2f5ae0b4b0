"""Measurements for DESIGN.md section 18 -> profiles/windows_bench.json.

jdaValidateWindowsDevice on 256 frames of 640x480 resident in HBM, the shipped-dimension synthetic model (T = 5, K = 540,
L = 27, D = 4) in the cascade regime (bench.py's model), random valid windows (side uniform in [24, 240], position uniform):
  tracking   64 windows per frame (16,384 in all): a tracker re-checking its boxes
  bulk       10^5 windows in all, frames drawn at random
one warm-up, then median (min - max) of 5 calls: call_ms (wall clock of the C call) and gpu_ms (the kernels' device time).
The yardstick is the only route the entry's answers had before it, timed in the same run on the same frames:
  jdaTraceBatch          every window of the scan grid with per-window outputs (host frames in, host arrays out)
  jdaDetectBatchDevice   faces only
and the ratios of their call_ms to the tracking load's.  Also recorded: the LDS-tile form against the global-read form
(option windows_tile = 0) on the tracking load, identical bits asserted.

    python tools/windows_bench.py [--out profiles/windows_bench.json] [--model FILE]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

DIMS = (5, 540, 27, 4)
N_FRAMES, W, H = 256, 640, 480
CALL = dict(scale=1.25, min_size=40, max_size=-1, th=-0.5)


def med(v):
    return dict(median_ms=statistics.median(v), min_ms=min(v), max_ms=max(v), runs=v)


def random_windows(rng, frames_of, lo=24, hi=240):
    n = len(frames_of)
    s = rng.integers(lo, hi + 1, n)
    x = (rng.random(n) * (W - s + 1)).astype(np.int64)
    y = (rng.random(n) * (H - s + 1)).astype(np.int64)
    return np.column_stack([frames_of, x, y, s]).astype(np.int32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "windows_bench.json"))
    ap.add_argument("--model", default=None, help="a model file to use instead of building bench.py's cascade model")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--trace-reps", type=int, default=2, help="timed jdaTraceBatch calls (each returns 2 GB of per-window outputs)")
    args = ap.parse_args()
    import torch
    import bench
    from jda_amd import api, synth
    path = args.model or bench.model_path(DIMS, "cascade", 1, synth.make_frames(8, W, H, seed=0, first=10_000_000))
    frames = bench.make_frames(N_FRAMES, W, H, seed=0)
    d_frames = torch.from_numpy(frames).cuda()
    c = api.Cascador(path, "double", device=0)
    rng = np.random.default_rng(11)
    loads = dict(tracking=random_windows(rng, np.repeat(np.arange(N_FRAMES), 64)),
                 bulk=random_windows(rng, rng.integers(0, N_FRAMES, 100000)))

    def timed(fn, reps):
        call, gpu, last, st = [], [], None, None
        for r in range(reps + 1):                      # the first call is the warm-up
            t0 = time.perf_counter()
            last, st = fn()
            wall = (time.perf_counter() - t0) * 1e3
            if r:
                call.append(st["call_ms"] if st else wall); gpu.append(st["gpu_ms"] if st else 0.0)
        return dict(call=med(call), gpu=med(gpu)), last, st

    out = dict(model=dict(T=DIMS[0], K=DIMS[1], L=DIMS[2], D=DIMS[3], regime="cascade"), frames="%d x %dx%d in HBM" % (N_FRAMES, W, H),
               windows="side uniform in [24, 240], position uniform", tile_limit=int(c.get_option("windows_tile_limit")), loads={})
    keep = {}
    for name, win in loads.items():
        res, got, st = timed(lambda: c.validate_windows(d_frames, win, th=CALL["th"], stats=True), args.reps)
        res.update(n_windows=int(len(win)), faces=int(st["face_patch_n"]), average_cart_n=st["average_cart_n"],
                   tiled_windows=int((win[:, 3] <= out["tile_limit"]).sum()))
        out["loads"][name] = res
        keep[name] = got
    # the global-read form on the tracking load
    c.set_option("windows_tile", 0)
    res, got, st = timed(lambda: c.validate_windows(d_frames, loads["tracking"], th=CALL["th"], stats=True), args.reps)
    assert all(np.array_equal(got[k].view(np.uint8), keep["tracking"][k].view(np.uint8)) for k in got), "the two forms differ"
    out["loads"]["tracking_global_read"] = res
    c.set_option("windows_tile", -1)
    # the parent's routes
    res, _, st = timed(lambda: c.detect_batch_device(d_frames, stats=True, keep_results=False, **CALL), args.reps)
    res.update(windows=int(st["patch_n"]), faces=int(st["face_patch_n"]))
    out["jdaDetectBatchDevice"] = res
    kw = {k: CALL[k] for k in ("scale", "min_size", "max_size")}
    n_grid = int(st["patch_n"])
    res, _, _ = timed(lambda: (c.trace(frames, **kw), None), args.trace_reps)
    res.pop("gpu")
    res.update(windows=n_grid, note="wall clock of the Python call: host frames in, carts_n / score / path_hash / shapes of every window out")
    out["jdaTraceBatch"] = res
    t = out["loads"]["tracking"]["call"]["median_ms"]
    out["ratios_to_tracking_call_ms"] = dict(jdaTraceBatch=out["jdaTraceBatch"]["call"]["median_ms"] / t,
                                             jdaDetectBatchDevice=out["jdaDetectBatchDevice"]["call"]["median_ms"] / t)
    out["walk_fraction"] = len(loads["tracking"]) / float(n_grid)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps({k: (v["call"]["median_ms"], v["gpu"]["median_ms"]) for k, v in out["loads"].items()}))
    print(json.dumps(dict(detect=out["jdaDetectBatchDevice"]["call"]["median_ms"], trace=out["jdaTraceBatch"]["call"]["median_ms"],
                          ratios=out["ratios_to_tracking_call_ms"])))


if __name__ == "__main__":
    main()
