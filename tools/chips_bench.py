"""Times the cut of upright face chips (jdaFaceChipsDevice, k_chips) on frames resident in device memory: `--faces-per-frame`
faces of 80 - 200 px (the chip's side in source pixels; rotations within +-30 degrees, centres anywhere a face of that size
still lies inside the frame) from each of 256 x 640x480 BGR24 frames into 112 x 112 BGR24 chips, n chosen by the face's
scale, and the same faces into GRAY8 chips.  Per leg one warm-up call, then the median (min - max) of `--repeats` calls of
device_ms (HIP events around the one launch).  In the same run it times hipMemcpyDtoD of the chips' bytes -- the floor of any
kernel that writes them -- and reports the ratio to it, and it runs the host form (jdaFaceChips, one CPU thread) on the first
`--host-faces` faces, checking that both forms give the same bytes.

    python tools/chips_bench.py [--repeats 5] [--out profiles/chips_bench.json]
    python tools/chips_bench.py --resources profiles/chips_bench.json     (no GPU: compiles k_chips.hip with
        -Rpass-analysis=kernel-resource-usage and adds its VGPRs / SGPRs / scratch / waves per SIMD to that file)
"""
import argparse
import ctypes as C
import json
import math
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from kernel_resources import kernel_resources  # noqa: E402  (tools/kernel_resources.py)

# five points (eyes, nose, mouth corners) of an upright face in a 112 x 112 chip
TEMPLATE = np.array([38.0, 46.0, 74.0, 46.0, 56.0, 66.0, 42.0, 86.0, 70.0, 86.0])


def summary(ms):
    return dict(median=statistics.median(ms), min=min(ms), max=max(ms), all=ms)


def make_faces(n_frames, per_frame, W, H, chip, seed=0):
    """(face_image, landmarks [n, 10] float32, sizes): the template under a random similarity, plus a pixel of noise."""
    rng = np.random.default_rng(seed)
    q = TEMPLATE.reshape(-1, 2)
    c = q - q.mean(0)
    fi, lm, sizes = [], [], []
    for f in range(n_frames):
        for _ in range(per_frame):
            size = float(rng.uniform(80.0, 200.0))
            s, ang = size / chip, math.radians(float(rng.uniform(-30.0, 30.0)))
            a, b = s * math.cos(ang), s * math.sin(ang)
            r = 0.5 * size
            centre = np.array([rng.uniform(r, W - r), rng.uniform(r, H - r)])
            p = np.stack([a * c[:, 0] - b * c[:, 1], b * c[:, 0] + a * c[:, 1]], 1) + centre + rng.uniform(-1.0, 1.0, c.shape)
            fi.append(f); lm.append(p.reshape(-1)); sizes.append(size)
    return np.array(fi, np.int32), np.array(lm, np.float32), sizes


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--resources", default=None, help="JSON file to add k_chips' compile-time resource figures to (no GPU needed)")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--faces-per-frame", type=int, default=4)
    ap.add_argument("--host-faces", type=int, default=32)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.resources:
        with open(a.resources) as f:
            res = json.load(f)
        res["k_chips_resources"] = kernel_resources("k_chips.hip", "k_chips")
        with open(a.resources, "w") as f:
            json.dump(res, f, indent=1)
        print(json.dumps(res["k_chips_resources"]))
        return
    import torch
    from jda_amd import api, synth
    assert torch.cuda.is_available(), "chips_bench needs a HIP device"
    W, H, n, chip = 640, 480, a.frames, 112
    import tempfile
    with tempfile.TemporaryDirectory() as d:                  # the cascador supplies the device and a lane; its model is not read
        path = os.path.join(d, "m.model")
        synth.make_model(2, 8, 5, 3, seed=1).save(path, 8)
        c = api.Cascador(path, device=0)
    g = torch.Generator(device="cuda").manual_seed(1)
    frames = torch.randint(0, 256, (n, H, W, 3), dtype=torch.uint8, device="cuda", generator=g)
    images = [frames[i] for i in range(n)]
    fi, lm, sizes = make_faces(n, a.faces_per_frame, W, H, chip)
    hip = C.CDLL("libamdhip64.so")
    hip.hipMemcpyDtoD.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
    res = dict(repeats=a.repeats, frames=n, faces=len(fi), face_px=dict(min=min(sizes), max=max(sizes)), chip=chip, legs={})

    def leg(name, chip_fmt):
        cuts, copies, st, out = [], [], None, None
        for r in range(a.repeats + 1):
            out, mats, st = c.face_chips_device(images, "bgr24", fi, lm, TEMPLATE, chip, chip, chip_fmt, matrices=True, stats=True)
            nbytes = st["chip_bytes"]
            if r == 0:
                src = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
                dst = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            assert hip.hipMemcpyDtoD(dst.data_ptr(), src.data_ptr(), nbytes) == 0
            e1.record()
            torch.cuda.synchronize()
            if r:
                cuts.append(st["device_ms"]); copies.append(e0.elapsed_time(e1))
        ns = [1 if m[0] * m[0] + m[3] * m[3] <= 1.0 else 2 if m[0] * m[0] + m[3] * m[3] <= 4.0 else 3 for m in mats]
        one = dict(chip_format=chip_fmt, faces=st["faces"], chip_bytes=st["chip_bytes"], taps=st["taps"], launches=st["launches"],
                   faces_by_n={str(k): ns.count(k) for k in sorted(set(ns))}, chips_device_ms=summary(cuts), memcpy_dtod_ms=summary(copies),
                   call_ms_last=st["call_ms"])
        one["ratio_to_memcpy"] = one["chips_device_ms"]["median"] / one["memcpy_dtod_ms"]["median"]
        one["Gtaps_per_s"] = st["taps"] / (one["chips_device_ms"]["median"] * 1e-3) / 1e9
        one["faces_per_s"] = st["faces"] / (one["chips_device_ms"]["median"] * 1e-3)
        # the host form, one thread, on the first faces -- and the same bytes
        k = min(a.host_faces, len(fi))
        host_imgs = [frames[i].cpu().numpy() for i in range(int(fi[k - 1]) + 1)]
        t0 = time.perf_counter()
        host = api.face_chips(host_imgs, "bgr24", fi[:k], lm[:k], TEMPLATE, chip, chip, chip_fmt)
        one["host_form_ms_per_face"] = (time.perf_counter() - t0) * 1e3 / k
        one["host_form_faces"] = k
        assert np.array_equal(out[:k].cpu().numpy(), host)
        res["legs"][name] = one
        print(name, json.dumps(one), flush=True)

    leg("bgr24_to_bgr24_112", "bgr24")
    leg("bgr24_to_gray8_112", "gray8")
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
    c.close()


if __name__ == "__main__":
    main()
