"""Times the stage close (jdaStageUpdateShapesCpp, jdaGenLbfCpp) at the shipped sizes (reference model/config.json: K = 540
carts of depth 4, 27 landmarks, 48 / 36 / 24 patches) on 2 * 10^5 samples whose patches are resident in device memory:
the fused walk + update, the update from given indicators and the walk alone, for scale-0 and multi-scale carts.  One
warm-up call, then `--repeats` timed calls per configuration; reports the median (min - max) of the wall clock of a call,
the entry's own split (upload / k_lbf by HIP events / download) and the bytes the algorithm moves, computed from the
shapes.  The shapes and the indicators cross the host link in every call (they are host arrays of the C ABI): the
kernel's time is device_ms.  There is no reference time to compare with: the reference's trainer needs OpenCV and
liblinear and cannot be built here, and the parent commit has no such entry.

    python tools/stage_bench.py [--n 200000] [--K 540] [--repeats 3] [--out profiles/stage_close_bench.json]
    python tools/stage_bench.py --once fused_multi        (one call of one configuration: for a kernel trace)
    python tools/stage_bench.py --similarity              (jdaSetSimilarityTransform(1) with the option train_similarity: every
                                                           sample under its own STParameter)
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

OS, HS, QS = 48, 36, 24
L, D = 27, 4
CONFIGS = {"fused_scale0": ("fused", False), "fused_multi": ("fused", True), "update_only": ("update", False),
           "walk_scale0": ("walk", False), "walk_multi": ("walk", True)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=200000)
    ap.add_argument("--K", type=int, default=540)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--once", default=None)
    ap.add_argument("--out", default=None)
    ap.add_argument("--similarity", action="store_true")
    a = ap.parse_args()
    import torch
    from jda_amd import api, synth
    assert torch.cuda.is_available(), "stage_bench needs a HIP device"
    path = os.path.join(synth.cache_dir(), "stage_bench_1_2_%d_%d.model" % (L, D))
    synth.make_model(1, 2, L, D, seed=1).save(path, 8)
    c = api.Cascador(path, "double", device=0)
    if a.similarity:
        c.set_similarity_transform(True)
        c.set_option("train_similarity", 1)
    n, K, dim, leaf_n, inner = a.n, a.K, 2 * L, 1 << (D - 1), (1 << (D - 1)) - 1
    pbytes = OS * OS + HS * HS + QS * QS
    g = torch.Generator(device="cuda").manual_seed(1)
    patches = torch.randint(0, 256, (n, pbytes), dtype=torch.uint8, device="cuda", generator=g)
    rng = np.random.default_rng(1)
    shapes = rng.uniform(0.15, 0.85, (1, dim)) + rng.normal(0, 0.05, (n, dim))
    d = dict(patches=patches, shapes=shapes, weights=None, residual=None, has_gt=None)
    w = rng.normal(0, 2e-3, (K * leaf_n, dim))
    th = rng.integers(-60, 61, K * inner).astype(np.int32)
    # what the algorithm moves per call, from the shapes alone
    traffic = dict(patch_bytes=n * pbytes, shape_bytes_in=n * dim * 8, shape_bytes_out=n * dim * 8, lbf_bytes=n * K * 4,
                   w_row_bytes_read=n * K * dim * 8, w_table_bytes=K * leaf_n * dim * 8, node_table_bytes=K * inner * 48,
                   node_evaluations=n * K * (D - 1), fp64_adds=n * K * dim)
    res = dict(n=n, K=K, depth=D, landmarks=L, sizes=[OS, HS, QS], repeats=a.repeats, similarity=bool(a.similarity), traffic=traffic, configs={})
    lbf = None
    for name, (what, multi) in CONFIGS.items():
        if a.once and name != a.once:
            continue
        pool, _ = api.gen_feature_pool_cpp(K * inner, L, 0.3, multi, 7, 1)
        if what == "update" and lbf is None:
            lbf = c.gen_lbf_cpp(d, pool, th)
        runs = []
        for r in range(1 if a.once else a.repeats + 1):
            if what == "fused":
                _, st = c.stage_update_shapes_cpp(d, pool, th, w, stats=True)
            elif what == "update":
                _, st = c.stage_update_shapes_cpp(d, None, None, w, lbf, stats=True)
            else:
                import time
                t0 = time.perf_counter()
                c.gen_lbf_cpp(d, pool, th)
                st = dict(call_ms=(time.perf_counter() - t0) * 1e3)
            if r or a.once:
                runs.append(st)
        ms = [s["call_ms"] for s in runs]
        one = dict(call_ms_median=statistics.median(ms), call_ms_min=min(ms), call_ms_max=max(ms), call_ms_all=ms)
        for k in ("upload_ms", "device_ms", "download_ms"):
            if k in runs[0]:
                v = [s[k] for s in runs]
                one[k + "_median"], one[k + "_min"], one[k + "_max"] = statistics.median(v), min(v), max(v)
        for k in ("chunks", "lds_path", "waves_per_group", "lds_bytes"):
            if k in runs[0]:
                one[k] = runs[0][k]
        if "device_ms_median" in one and what != "walk":
            one["w_row_read_TBps"] = traffic["w_row_bytes_read"] / (one["device_ms_median"] * 1e-3) / 1e12
        res["configs"][name] = one
        print(name, json.dumps(one), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
    c.close()


if __name__ == "__main__":
    main()
