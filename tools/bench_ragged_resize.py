"""The first tensor of a judge batch from 64 images of unequal size: Resize((224,
224)) + ToTensor + Normalize(ImageNet) (18:28-32) as fp32 [64, 3, 224, 224].

The batch is a STAND-IN for GTSRB, which is not on the machine: 64 synthetic
images with sides drawn from 25..250 (GTSRB's range) by a fixed seed, aspect
ratio within +-15 %, random pixels.

Timed, with device events around a window of at least 0.5 s after a warm-up:
  (a) the ragged call: RaggedBatch.resize -> rr_resize_ragged_u8, two launches;
  (b) the same 64 images one by one through the dense ops.resize_bilinear_u8
      plus torch.stack: three launches and a workspace per image.
and, with the host clock (it is host work), read_ppm of the same 64 images from
a temporary directory the tool writes: files -> RaggedBatch on the device.

Writes profiles/ragged_resize_b64.json: both times, their ratio, the launch
counts, the algorithmic bytes (every input byte read once, every output byte
written once) and GB/s against the 6.29 TB/s float4-copy figure of the MI355X,
for information.  (a) and (b) are compared bit for bit first.

    python tools/bench_ragged_resize.py [--out profiles/ragged_resize_b64.json]
"""
import argparse
import json
import math
import os
import sys
import tempfile
import time

R_ = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, os.path.join(R_, "image-restoration-for-road-sign-recognition-in-autonomous-driving_amd"))
import numpy as np  # noqa: E402
import torch  # noqa: E402
from roadrestore import imgproc, ops  # noqa: E402

COPY_TBPS = 6.29
BATCH = 64
OUT_HW = (224, 224)
WINDOW_S = 0.5
SEED = 1234


def synthetic_images():
    rng = np.random.default_rng(SEED)
    imgs = []
    for _ in range(BATCH):
        h = int(rng.integers(25, 251))
        w = int(np.clip(round(h * rng.uniform(0.85, 1.15)), 25, 250))
        imgs.append(rng.integers(0, 256, (h, w, 3), dtype=np.uint8))
    return imgs


def window(fn, min_s=WINDOW_S):
    """ms per call of fn: warm-up, then device events around >= min_s of calls"""
    for _ in range(3):
        fn()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(3):
        fn()
    e.record()
    torch.cuda.synchronize()
    per = max(s.elapsed_time(e) / 3, 1e-3)
    reps = max(3, math.ceil(min_s * 1e3 / per))
    s.record()
    for _ in range(reps):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / reps, reps


def host_window(fn, min_s=WINDOW_S):
    """ms per call of host-bound fn (device work included: synchronised)"""
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    reps, t0 = 0, time.perf_counter()
    while True:
        fn()
        torch.cuda.synchronize()
        reps += 1
        dt = time.perf_counter() - t0
        if dt >= min_s and reps >= 3:
            return dt * 1e3 / reps, reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(R_, "profiles", "ragged_resize_b64.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_ragged_resize needs the GPU (no CPU timing)")
    dev = torch.device("cuda:0")
    imgs = synthetic_images()
    oh, ow = OUT_HW
    mean, std = imgproc.IMAGENET_MEAN, imgproc.IMAGENET_STD

    batch = imgproc.RaggedBatch.from_arrays(imgs, dev)
    singles = [torch.from_numpy(im).unsqueeze(0).to(dev) for im in imgs]

    def ragged():
        return batch.resize(oh, ow, out="f32", mean=mean, std=std)

    def one_by_one():
        return torch.stack([ops.resize_bilinear_u8(x, oh, ow, out="f32", mean=mean, std=std)[0]
                            for x in singles])

    equal = bool(torch.equal(ragged(), one_by_one()))
    a_ms, a_reps = window(ragged)
    b_ms, b_reps = window(one_by_one)

    in_bytes = sum(im.size for im in imgs)
    out_bytes = BATCH * 3 * oh * ow * 4
    nbytes = in_bytes + out_bytes
    b_launches = sum(1 if im.shape[:2] == OUT_HW else 3 for im in imgs) + 1     # + torch.stack

    with tempfile.TemporaryDirectory() as d:
        paths = []
        for i, im in enumerate(imgs):
            p = os.path.join(d, f"{i:05d}.ppm")
            with open(p, "wb") as f:
                f.write(b"P6\n%d %d\n255\n" % (im.shape[1], im.shape[0]) + im.tobytes())
            paths.append(p)
        got = imgproc.read_ppm(paths, dev)
        read_equal = bool(torch.equal(got.resize(oh, ow), batch.resize(oh, ow)))
        r_ms, r_reps = host_window(lambda: imgproc.read_ppm(paths, dev))

    def gbps(ms):
        return nbytes / (ms * 1e-3) / 1e9

    res = {
        "workload": "64 images of unequal size -> Resize((224, 224)) + ToTensor + Normalize, fp32 "
                    "[64, 3, 224, 224] (18:28-32)",
        "data": f"synthetic stand-in for GTSRB: sides 25..250, aspect within 15 %, seed {SEED}",
        "device": torch.cuda.get_device_name(0), "window_s": WINDOW_S, "copy_tbps": COPY_TBPS,
        "sizes_hw": [list(im.shape[:2]) for im in imgs],
        "algorithmic_bytes": {"in": int(in_bytes), "out": int(out_bytes), "total": int(nbytes)},
        "a_ragged": {"ms": round(a_ms, 4), "reps": a_reps, "launches": 2, "gbps": round(gbps(a_ms), 1),
                     "vs_copy": round(gbps(a_ms) / (COPY_TBPS * 1e3), 4)},
        "b_one_by_one": {"ms": round(b_ms, 4), "reps": b_reps, "launches": b_launches,
                         "gbps": round(gbps(b_ms), 1),
                         "vs_copy": round(gbps(b_ms) / (COPY_TBPS * 1e3), 4)},
        "b_over_a": round(b_ms / a_ms, 2),
        "a_le_b": bool(a_ms <= b_ms),
        "a_equals_b_bitwise": equal,
        "read_ppm": {"ms": round(r_ms, 4), "reps": r_reps, "files": BATCH, "file_bytes": int(in_bytes),
                     "clock": "host, synchronised", "equals_from_arrays": read_equal},
    }
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))
    if not (equal and read_equal and a_ms <= b_ms):
        raise SystemExit("bench_ragged_resize: (a) must equal (b) bit for bit and be no slower")


if __name__ == "__main__":
    main()
