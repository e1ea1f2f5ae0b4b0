"""Times a stage's global regression (jdaGlobalRegressionCpp, k_fit) at the shipped sizes: 10^5 rows, K = 540 carts of depth
4 (f = 4,320 weights per coordinate), L = 27 (54 coordinates); random leaves, y = X w* + noise.  One warm-up call, then
`--repeats` timed calls; reports the median (min - max) of call_ms, device_ms (HIP events around the launches, summed) and
shuffle_ms, the epochs per coordinate (min / median / max) and device_ms per launched epoch.  There is no yardstick to
divide by: the reference's fit is liblinear, which is not in its tree, and the parent commit has no such path.

Every GPU step runs under a time limit of its own, chained with &&:

    timeout -k 10 600 python tools/fit_bench.py [--n 100000] [--K 540] [--repeats 3] [--max-iter 0] --out profiles/fit_bench.json \\
      && timeout -k 10 700 python tools/fit_bench.py --profile DIR [--limit 600]

--once      one call, no warm-up (the body of a profiler run)
--profile   starts `rocprofv3 --kernel-trace --stats -d DIR -- python tools/fit_bench.py --once` as a run of its own, in a
            process group of its own: when --limit seconds run out the whole group is killed, the profiled child with it
"""
import argparse
import json
import os
import signal
import statistics
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def summary(v):
    return dict(median=statistics.median(v), min=min(v), max=max(v), all=v)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=100000)
    ap.add_argument("--K", type=int, default=540)
    ap.add_argument("--depth", type=int, default=4)
    ap.add_argument("--L", type=int, default=27)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--max-iter", type=int, default=0)
    ap.add_argument("--noise", type=float, default=0.01)
    ap.add_argument("--once", action="store_true")
    ap.add_argument("--profile", default=None)
    ap.add_argument("--limit", type=int, default=600, help="seconds the profiled child may take")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.profile:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "-d", a.profile, "--", sys.executable, os.path.abspath(__file__), "--once",
               "--n", str(a.n), "--K", str(a.K), "--depth", str(a.depth), "--L", str(a.L), "--max-iter", str(a.max_iter)]
        child = subprocess.Popen(cmd, start_new_session=True)                 # its own process group: the limit ends rocprofv3 AND what it started
        try:
            sys.exit(child.wait(timeout=a.limit))
        except subprocess.TimeoutExpired:
            os.killpg(child.pid, signal.SIGKILL)
            child.wait()
            sys.exit(124)
    import torch
    from jda_amd import api, synth
    assert torch.cuda.is_available(), "fit_bench needs a HIP device"
    path = os.path.join(synth.cache_dir(), "fit_bench_1_2_%d_%d.model" % (a.L, a.depth))
    synth.make_model(1, 2, a.L, a.depth, seed=1).save(path, 8)
    c = api.Cascador(path, "double", device=0)
    leaf_n, dim = 1 << (a.depth - 1), 2 * a.L
    rng = np.random.default_rng(1)
    lbf = (np.arange(a.K, dtype=np.int64)[None, :] * leaf_n + rng.integers(0, leaf_n, (a.n, a.K))).astype(np.int32)
    w_star = rng.standard_normal((a.K * leaf_n, dim)) * 0.05
    res = np.zeros((a.n, dim))
    for k in range(a.K):                                                      # y = X w* + noise, a cart at a time
        res += w_star[lbf[:, k]]
    res += a.noise * rng.standard_normal(res.shape)
    out = dict(n=a.n, K=a.K, depth=a.depth, L=a.L, repeats=a.repeats, max_iter=a.max_iter, calls=[])
    runs = 1 if a.once else a.repeats + 1
    for r in range(runs):
        w, iters, gn, st = c.global_regression_cpp(lbf, res, max_iter=a.max_iter, seed=1)
        one = dict(st, iters_min=int(iters.min()), iters_median=float(np.median(iters)), iters_max=int(iters.max()),
                   device_ms_per_epoch=st["device_ms"] / max(1, st["epochs_launched"]), warm_up=bool(r == 0 and not a.once))
        print(json.dumps(one), flush=True)
        out["calls"].append(one)
    timed = [o for o in out["calls"] if not o["warm_up"]]
    for key in ("call_ms", "device_ms", "shuffle_ms", "device_ms_per_epoch"):
        out[key] = summary([o[key] for o in timed])
    print(json.dumps({k: v for k, v in out.items() if k != "calls"}), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
    c.close()


if __name__ == "__main__":
    main()
