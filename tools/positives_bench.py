"""Times the build of the positive sample set's patches (jdaBuildPositivesCppDevice, k_faces) at the shipped sizes: 10^5
faces with boxes of 60 - 400 px (a share of them leaving their image) on resident 640 x 480 noise images, 48 / 36 / 24
patches, augmentation on (2 * 10^5 records of 4,176 bytes into a device dst).  One warm-up call, then `--repeats` timed
calls; reports the median (min - max) of call_ms (wall clock, the call ends in a stream wait) and of device_ms (HIP events
around the launches).  There is no yardstick to beat -- the parent commit has no such path and the reference needs OpenCV;
for scale the k_mine_patches time per record of profiles/mine_kernel_trace.txt is reported alongside (mining's patches of
one crop: the o patch from the image, h and q from the o patch in LDS).

    python tools/positives_bench.py [--faces 100000] [--images 256] [--repeats 5] [--out profiles/positives_bench.json]
"""
import argparse
import json
import os
import re
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

OS, HS, QS = 48, 36, 24
W, H = 640, 480


def summary(ms):
    return dict(median=statistics.median(ms), min=min(ms), max=max(ms), all=ms)


def mine_patches_us_per_record():
    """k_mine_patches' total time over the crops it built in profiles/mine_kernel_trace.txt (the crops of a launch: the grid
    of the k_mine_walk launch that follows it, lanes rounded up to 64 -- an upper bound on the crops, so a lower bound on
    the time per record)."""
    try:
        txt = open(os.path.join(ROOT, "profiles", "mine_kernel_trace.txt")).read()
        total_ms = float(re.search(r"k_mine_patches\s+\d+\s+([\d.]+)", txt).group(1))
        walk = txt.split("k_mine_walk vgpr")[1].split("\n")[1]
        crops = sum(int(g.split(":")[0]) for g in walk.split(","))
        return dict(total_ms=total_ms, crops_at_most=crops, us_per_record_at_least=total_ms * 1e3 / crops)
    except Exception as e:          # the profile is documentation: its absence does not stop the measurement
        return dict(error=str(e))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--faces", type=int, default=100000)
    ap.add_argument("--images", type=int, default=256)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from jda_amd import api, synth
    assert torch.cuda.is_available(), "positives_bench needs a HIP device"
    path = os.path.join(synth.cache_dir(), "positives_bench_1_2_5_3.model")
    synth.make_model(1, 2, 5, 3, seed=1).save(path, 8)
    c = api.Cascador(path, "double", device=0)
    n, pb = a.faces, OS * OS + HS * HS + QS * QS
    g = torch.Generator(device="cuda").manual_seed(1)
    buf = torch.randint(0, 256, (a.images * W * H,), dtype=torch.uint8, device="cuda", generator=g)
    images = (buf, [i * W * H for i in range(a.images)], [W] * a.images, [H] * a.images)
    rng = np.random.default_rng(1)
    side = rng.integers(60, 401, n)
    faces = np.c_[np.sort(rng.integers(0, a.images, n)), rng.integers(-40, W - 20, n) - side // 4, rng.integers(-40, H - 20, n) - side // 4,
                  side, side].astype(np.int32)
    dst = torch.zeros(2 * n * pb, dtype=torch.uint8, device="cuda")
    call, dev = [], []
    for r in range(a.repeats + 1):
        _, st = c.build_positives_cpp(images, faces, dst, True, OS, HS, QS, stats=True)
        if r:
            call.append(st["call_ms"]); dev.append(st["device_ms"])
    res = dict(faces=n, records=2 * n, record_bytes=pb, images=a.images, image_size=[W, H], repeats=a.repeats, launches=st["launches"],
               call_ms=summary(call), device_ms=summary(dev))
    res["device_us_per_record"] = res["device_ms"]["median"] * 1e3 / (2 * n)
    res["device_us_per_face"] = res["device_ms"]["median"] * 1e3 / n
    res["k_mine_patches_for_scale"] = mine_patches_us_per_record()
    # the records are what the host entry gives for a sample of the faces (mirrors included)
    pick = np.sort(rng.integers(0, n, 32))
    host_imgs = [buf[i * W * H:(i + 1) * W * H].cpu().numpy().reshape(H, W) for i in range(a.images)]
    sub = c.build_positives_cpp(host_imgs, faces[pick], None, True, OS, HS, QS)
    d2 = dst.view(2 * n, pb)
    for j, i in enumerate(pick):
        assert np.array_equal(d2[int(i)].cpu().numpy(), sub[j]) and np.array_equal(d2[n + int(i)].cpu().numpy(), sub[32 + j])
    print(json.dumps(res), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
    c.close()


if __name__ == "__main__":
    main()
