"""Times jdaTrainCartCpp at the shipped sizes (reference model/config.json: 2,000 pool features, depth 4, 27 landmarks,
48 / 36 / 24 patches) on 10^5 positives + 10^5 negatives resident in device memory: classification-only and
regression-only carts, scale-0 and multi-scale pools.  One warm-up call, then `--repeats` timed calls per configuration;
reports the median and the spread of the wall clock per cart, the entry's own split (setup / device / host sweep /
partition) and feature evaluations per second.  There is no reference time to compare with: the reference's trainer
needs OpenCV and cannot be built here, and the parent commit has no such entry.

    python tools/train_bench.py [--n 100000] [--features 2000] [--repeats 3] [--out profiles/train_bench.json]
    python tools/train_bench.py --once cls_scale0        (one call of one configuration: for a kernel trace)
    python tools/train_bench.py --similarity             (jdaSetSimilarityTransform(1) with the option train_similarity: every
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
CONFIGS = {"cls_scale0": (1, False), "cls_multi": (1, True), "reg_scale0": (0, False), "reg_multi": (0, True)}


def sample_set(torch, n, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    patches = torch.randint(0, 256, (n, OS * OS + HS * HS + QS * QS), dtype=torch.uint8, device="cuda", generator=g)
    rng = np.random.default_rng(seed)
    shapes = rng.uniform(0.15, 0.85, (1, 2 * L)) + rng.normal(0, 0.05, (n, 2 * L))
    w = np.exp(-rng.uniform(-8, 8, n))
    return dict(patches=patches, shapes=shapes, weights=w / w.sum(), residual=rng.normal(0, 0.05, (n, 2)), has_gt=None)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=100000)
    ap.add_argument("--features", type=int, default=2000)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--once", default=None)
    ap.add_argument("--out", default=None)
    ap.add_argument("--similarity", action="store_true")
    a = ap.parse_args()
    import torch
    from jda_amd import api, synth
    path = os.path.join(synth.cache_dir(), "train_bench_1_2_%d_%d.model" % (L, D))
    synth.make_model(1, 2, L, D, seed=1).save(path, 8)
    c = api.Cascador(path, "double", device=0)
    if a.similarity:
        c.set_similarity_transform(True)
        c.set_option("train_similarity", 1)
    pos, neg = sample_set(torch, a.n, 1), sample_set(torch, a.n, 2)
    inner = (1 << (D - 1)) - 1
    res = dict(n_pos=a.n, n_neg=a.n, features=a.features, depth=D, landmarks=L, sizes=[OS, HS, QS], repeats=a.repeats, similarity=bool(a.similarity), configs={})
    for name, (mode, multi) in CONFIGS.items():
        if a.once and name != a.once:
            continue
        pools, us = zip(*[api.gen_feature_pool_cpp(a.features, L, 0.3, multi, 7, node) for node in range(1, inner + 1)])
        pools, us = np.concatenate(pools), np.concatenate(us)
        runs = []
        for r in range(1 if a.once else a.repeats + 1):
            out = c.train_cart_cpp(pos, neg, pools, [mode] * inner, us)
            if r or a.once:
                runs.append(out["stats"])
        ms = [s["call_ms"] for s in runs]
        med = statistics.median(ms)
        one = dict(ms_per_cart_median=med, ms_per_cart_min=min(ms), ms_per_cart_max=max(ms), ms_all=ms,
                   feature_evals=runs[0]["feature_evals"], feature_evals_per_s=runs[0]["feature_evals"] / (med * 1e-3),
                   nodes=[[int(v["pos_n"]), int(v["neg_n"])] for v in out["nodes"]])
        for k in ("setup_ms", "device_ms", "sweep_ms", "partition_ms"):
            one[k + "_median"] = statistics.median(s[k] for s in runs)
        one["feature_chunks"] = runs[0]["feature_chunks"]
        res["configs"][name] = one
        print(name, json.dumps(one), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
    c.close()


if __name__ == "__main__":
    main()
