"""Times the move of a resident sample set into a new order (jdaGatherSamplesCpp, k_gather) at the shipped sizes: 2 * 10^5
records of 48 / 36 / 24 patches (4,176 bytes) in device memory, a random permutation as the index, keep = n and keep = n/2.
One warm-up call, then `--repeats` timed calls; reports the median (min - max) of device_ms (HIP events around the
launch).  In the same run it times hipMemcpyDtoD of the same number of bytes: the yardstick -- the parent commit has no such
path and the reference's swap moves cv::Mat headers, not bytes -- and reports the ratio to it.

    python tools/boost_step_bench.py [--n 200000] [--repeats 5] [--out profiles/boost_step_bench.json]
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

OS, HS, QS = 48, 36, 24


def summary(ms):
    return dict(median=statistics.median(ms), min=min(ms), max=max(ms), all=ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=200000)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from jda_amd import api, synth
    assert torch.cuda.is_available(), "boost_step_bench needs a HIP device"
    path = os.path.join(synth.cache_dir(), "boost_step_bench_1_2_5_3.model")
    synth.make_model(1, 2, 5, 3, seed=1).save(path, 8)
    c = api.Cascador(path, "double", device=0)
    n, pb = a.n, OS * OS + HS * HS + QS * QS
    g = torch.Generator(device="cuda").manual_seed(1)
    src = torch.randint(0, 256, (n * pb,), dtype=torch.uint8, device="cuda", generator=g)
    dst = torch.zeros(n * pb, dtype=torch.uint8, device="cuda")
    perm = np.random.default_rng(1).permutation(n).astype(np.int32)
    hip = C.CDLL("libamdhip64.so")
    hip.hipMemcpyDtoD.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
    res = dict(n=n, record_bytes=pb, repeats=a.repeats, cases={})
    for name, keep in (("keep_n", n), ("keep_half", n // 2)):
        nbytes = keep * pb
        gather, copy = [], []
        for r in range(a.repeats + 1):
            _, st = c.gather_samples_cpp(src, perm, dst, keep, OS, HS, QS, stats=True)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            assert hip.hipMemcpyDtoD(dst.data_ptr(), src.data_ptr(), nbytes) == 0
            e1.record()
            torch.cuda.synchronize()
            if r:
                gather.append(st["device_ms"]); copy.append(e0.elapsed_time(e1))
        one = dict(bytes=nbytes, gather_device_ms=summary(gather), memcpy_dtod_ms=summary(copy))
        one["ratio_to_memcpy"] = one["gather_device_ms"]["median"] / one["memcpy_dtod_ms"]["median"]
        one["gather_GBps_read_plus_write"] = 2 * nbytes / (one["gather_device_ms"]["median"] * 1e-3) / 1e9
        res["cases"][name] = one
        print(name, json.dumps(one), flush=True)
    # the gather moved what numpy would: a sample of records
    c.gather_samples_cpp(src, perm, dst, n, OS, HS, QS)
    pick = np.random.default_rng(2).integers(0, n, 64)
    d2, s2 = dst.view(n, pb), src.view(n, pb)
    assert all(torch.equal(d2[int(i)], s2[int(perm[i])]) for i in pick)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
    c.close()


if __name__ == "__main__":
    main()
