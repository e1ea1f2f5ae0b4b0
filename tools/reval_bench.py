"""Measurements for DESIGN.md section 17 -> profiles/reval_bench.json.

1. The round trip the model in training removes.  At the shipped sizes (T = 5, K = 540, D = 4, L = 27), an all-pass model
loaded at status (2, 268) and brought to (2, 269) by one append; then, timed, the last cart is put again (a replace: the same
copies as an append, not measured apart) and the next mining call made
  in place:    put_cart_cpp + the first mine_negatives_cpp after it, on the cascador that already mined
  round trip:  serialize_to_cpp + Cascador(path) + the first mine_negatives_cpp on the fresh cascador
one warm-up, then median (min - max) of 3, wall clock.

and close_stage_cpp + the first mining call after it (at (2, 539); the model is reloaded for every repetition).
2. validate_samples_cpp at 10^5 resident records (48 / 36 / 24, in device memory) of the same all-pass model, so that every
sample walks everything, at statuses (1, -1), (2, 269) and complete, reval_form 0 against 1 in the same run: call_ms and
device_ms, one warm-up, then median (min - max) of 3.

    python tools/reval_bench.py [--out profiles/reval_bench.json]
    python tools/reval_bench.py --reval-only [--similarity]     (part 2 alone; --similarity: jdaSetSimilarityTransform(1) with the
                                                                  option train_similarity)
"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def med(v):
    return dict(median_ms=statistics.median(v), min_ms=min(v), max_ms=max(v), runs=v)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "reval_bench.json"))
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--reval-only", action="store_true")
    ap.add_argument("--similarity", action="store_true")
    args = ap.parse_args()
    assert not args.similarity or args.reval_only, "--similarity times part 2 only: give --reval-only"
    from jda_amd import api, synth
    import model_ref
    T, K, L, D = 5, 540, 27, 4
    src = synth.make_model(T, K, L, D, seed=1)                       # all-pass: every window walks every cart
    ref = model_ref.GrowModel(T, K, L, D, src.mean_shape)
    ref.m, ref.stage, ref.cart = src, 2, 268
    tmp = tempfile.mkdtemp()
    snap = ref.save(os.path.join(tmp, "snap.model"))
    if not args.reval_only:
        imgs = [synth.make_frames(1, 320, 240, seed=3, first=i)[0] for i in range(4)]
        cart = model_ref.cart_of(src, 2, 269)

        def mine(c):
            return c.mine_negatives_cpp(imgs, [5] * 4, [1.2] * 4, [0] * 4, size=2048, patches=False)

        a = api.Cascador(snap, "double", device=0)
        mine(a)                                                          # builds the mining tables
        a.put_cart_cpp(269, *cart)                                       # append: status (2, 269)
        want = mine(a)
        put_ms, mine_ms, both_ms = [], [], []
        for r in range(args.reps + 1):
            t0 = time.perf_counter()
            a.put_cart_cpp(269, *cart)                                   # replace: the same work as an append
            t1 = time.perf_counter()
            got = mine(a)
            t2 = time.perf_counter()
            assert np.array_equal(got["hits"], want["hits"]) and np.array_equal(got["score"].view(np.uint64), want["score"].view(np.uint64))
            if r:
                put_ms.append((t1 - t0) * 1e3); mine_ms.append((t2 - t1) * 1e3); both_ms.append((t2 - t0) * 1e3)
        ser_ms, create_ms, fmine_ms, trip_ms = [], [], [], []
        path = os.path.join(tmp, "trip.model")
        for r in range(args.reps + 1):
            t0 = time.perf_counter()
            a.serialize_to_cpp(path)
            t1 = time.perf_counter()
            b = api.Cascador(path, "double", device=0)
            t2 = time.perf_counter()
            got = mine(b)
            t3 = time.perf_counter()
            b.close()
            assert np.array_equal(got["hits"], want["hits"]) and np.array_equal(got["score"].view(np.uint64), want["score"].view(np.uint64))
            if r:
                ser_ms.append((t1 - t0) * 1e3); create_ms.append((t2 - t1) * 1e3); fmine_ms.append((t3 - t2) * 1e3); trip_ms.append((t3 - t0) * 1e3)
        a.close()
        # close + the first mining call after it: stage 2 complete but open, (2, 539)
        ref.cart = K - 1
        full = ref.save(os.path.join(tmp, "full.model"))
        close_ms, cmine_ms = [], []
        for r in range(args.reps + 1):
            b = api.Cascador(full, "double", device=0)
            mine(b)
            t0 = time.perf_counter()
            b.close_stage_cpp(src.w[2])
            t1 = time.perf_counter()
            mine(b)
            t2 = time.perf_counter()
            b.close()
            if r:
                close_ms.append((t1 - t0) * 1e3); cmine_ms.append((t2 - t1) * 1e3)
    # Validate on 10^5 resident records
    import torch
    n = 100000
    pb = 48 * 48 + 36 * 36 + 24 * 24
    gen = torch.Generator(device="cuda"); gen.manual_seed(5)
    d_pat = torch.randint(0, 256, (n, pb), dtype=torch.uint8, device="cuda", generator=gen)
    starts = src.mean_shape[None, :] + np.random.default_rng(5).normal(0, 0.05, (n, 2 * L))
    reval = {}
    for tag, hdr in (("1_-1", (1, -1)), ("2_269", (2, 269)), ("complete", (T, -1))):
        ref.stage, ref.cart = hdr
        c = api.Cascador(ref.save(os.path.join(tmp, "reval.model")), "double", device=0)
        if args.similarity:
            c.set_similarity_transform(True)
            c.set_option("train_similarity", 1)
        res, keep = {}, {}
        for form in (0, 1):
            c.set_option("reval_form", form)
            call, dev = [], []
            for r in range(args.reps + 1):
                t0 = time.perf_counter()
                got = c.validate_samples_cpp(dict(patches=d_pat, shapes=starts))
                if r:
                    call.append((time.perf_counter() - t0) * 1e3); dev.append(got["stats"]["device_ms"])
            keep[form] = got
            res["form%d" % form] = dict(call=med(call), device=med(dev), lds_path=got["stats"]["lds_path"], chunks=got["stats"]["chunks"])
        assert all(np.array_equal(keep[0][k].view(np.uint8), keep[1][k].view(np.uint8)) for k in ("is_face", "score", "carts_n", "shape"))
        res["carts_per_sample"] = int(keep[0]["carts_n"][0]); res["faces"] = int(keep[0]["is_face"].sum())
        reval[tag] = res
        c.close()
    if args.reval_only:
        out = dict(model=dict(T=T, K=K, L=L, D=D, all_pass=True), similarity=bool(args.similarity),
                   validate_samples_cpp=dict(records=n, sizes=[48, 36, 24], statuses=reval))
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
        print(json.dumps({t: {f: (v[f]["call"]["median_ms"], v[f]["device"]["median_ms"]) for f in ("form0", "form1")} for t, v in reval.items()}))
        return
    out = dict(model=dict(T=T, K=K, L=L, D=D, status=[2, 269], all_pass=True), images="4 x 320x240, step 5, factor 1.2, size 2048",
               hits=int(len(want["hits"])), windows=int(want["stats"]["windows"]),
               in_place=dict(put_cart_cpp=med(put_ms), first_mine_after_put=med(mine_ms), total=med(both_ms)),
               round_trip=dict(serialize_to_cpp=med(ser_ms), create=med(create_ms), first_mine=med(fmine_ms), total=med(trip_ms)),
               close=dict(close_stage_cpp=med(close_ms), first_mine_after_close=med(cmine_ms)),
               validate_samples_cpp=dict(records=n, sizes=[48, 36, 24], statuses=reval))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps({k: out[k]["total"]["median_ms"] for k in ("in_place", "round_trip")}))
    print(json.dumps({t: {f: (v[f]["call"]["median_ms"], v[f]["device"]["median_ms"]) for f in ("form0", "form1")} for t, v in reval.items()}))


if __name__ == "__main__":
    main()
