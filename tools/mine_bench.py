"""Throughput of the hard-negative mining entry (jdaMineNegativesCppDevice) on device-resident synthetic backgrounds.

    python tools/mine_bench.py [--images 2000] [--reps 3] [--out profiles/mine_bench.json]

Model: T=5, K=540, L=27, D=4, thresholds from synth.calibrate_thresholds (scale-0 nodes; the multi-scale variant redraws
the node scales of the same model, so its rejection is only roughly calibrated), saved as a trainer snapshot at stage 2,
cart 100 -- what MoreNegSamples mines with before a new cart.  Backgrounds: 640 x 480 synthetic frames, step / factor
from api.mine_params, transforms 0..7 in turn.  Every run walks the whole enumeration (size = all).  There is no CPU
baseline: the reference's mining needs OpenCV and cannot be built here."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=2000)
    ap.add_argument("--unique", type=int, default=32, help="distinct synthetic frames the background set cycles through")
    ap.add_argument("--sim-images", type=int, default=200, help="backgrounds of the similarity-transform runs (every window is walked)")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import torch
    from jda_amd import api, synth
    tmp = os.path.join(synth.cache_dir(), "mine_bench")
    os.makedirs(tmp, exist_ok=True)
    m = synth.make_model(5, 540, 27, 4, seed=1, cart_th=synth.NEG_BIG)
    synth.calibrate_thresholds(m, synth.make_frames(8, 640, 480, seed=2), min_size=48)
    p0 = os.path.join(tmp, "scale0.model")
    m.save(p0, 8, header_stage=2, header_cart=100)
    rng = np.random.default_rng(3)
    m.scale = rng.integers(0, 3, m.scale.shape).astype(np.int32)
    pm = os.path.join(tmp, "multi.model")
    m.save(pm, 8, header_stage=2, header_cart=100)

    uniq = synth.make_frames(a.unique, 640, 480, seed=4)
    n = a.images
    stride = 640 * 480
    buf = torch.empty(n * stride, dtype=torch.uint8, device="cuda")
    u = torch.from_numpy(uniq.reshape(a.unique, -1)).cuda()
    for i in range(n):
        buf[i * stride:(i + 1) * stride] = u[i % a.unique]
    torch.cuda.synchronize()
    steps, factors = api.mine_params(n, 24, seed=5)
    tfs = np.arange(n) % 8
    offs = np.arange(n, dtype=np.uint64) * stride
    rows = []
    for name, path, sim, k in (("scale0", p0, False, n), ("multi", pm, False, n), ("scale0_sim", p0, True, min(n, a.sim_images)),
                               ("multi_sim", pm, True, min(n, a.sim_images))):
        c = api.Cascador(path)
        c.set_similarity_transform(sim)
        dev = (buf, offs[:k], [640] * k, [480] * k)
        c.mine_negatives_cpp(dev, steps[:k], factors[:k], tfs[:k], 1, patches=False)         # warm-up (model upload)
        best = None
        for _ in range(a.reps):
            t0 = time.perf_counter()
            r = c.mine_negatives_cpp(dev, steps[:k], factors[:k], tfs[:k], 1 << 30, patches=False)
            dt = time.perf_counter() - t0
            best = dt if best is None else min(best, dt)
        st = r["stats"]
        row = dict(run=name, images=k, windows=st["windows"], hits=st["hits"], nega_n=st["nega_n"],
                   avg_carts_to_reject=st["carts_n"] / max(1, st["nega_n"]), seconds=best, windows_per_s=st["windows"] / best)
        print(json.dumps(row), flush=True)
        rows.append(row)
        c.close()
    if a.out:
        with open(a.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
