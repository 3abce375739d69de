#!/usr/bin/env python
"""profiles/micro/otsu_threshold.txt: what the device part of calculate_threshold costs on a ThermoScenes-sized dataset — 100
thermal images of 640 x 480 — beside a numpy restatement (np.bincount + the recurrence in Python floats) of the same pixels.

    python tools/otsu_bench.py [--images 100] [--out FILE]

The device figures are HIP-event times after a warm-up call, median and range of --repeats calls: (a) the tn_otsu_thresholds
call alone on pixels already packed on the device, (b) otsu_thresholds() = packing (torch.cat on the device) + the call.  The
upload of the decoded files and the PNG decoding themselves are host work common to both routes and are not timed.  A figure,
not a target: the threshold is computed once per evaluation.
"""
from __future__ import annotations

import argparse
import ctypes
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def thermal_like(n_images: int, h: int, w: int, seed: int = 0):
    """flat background with sensor noise of a grey level or two + a warm object: the statistics the run merging is built for"""
    import numpy as np

    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    out = []
    for i in range(n_images):
        cx, cy, r = rng.uniform(0.3, 0.7) * w, rng.uniform(0.3, 0.7) * h, rng.uniform(0.15, 0.3) * h
        inside = (xx - cx) ** 2 + (yy - cy) ** 2 < r * r
        img = np.where(inside, 170.0 + 40.0 * np.cos((xx + yy) / 37.0), 48.0) + rng.normal(0.0, 0.6, (h, w))
        out.append(np.clip(np.rint(img), 0, 255).astype(np.uint8))
    return out


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--images", type=int, default=100)
    ap.add_argument("--height", type=int, default=480)
    ap.add_argument("--width", type=int, default=640)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args(argv)
    import numpy as np
    import torch

    from tests.otsu_reference import otsu_restated
    from thermo_nerf_amd import _hip
    from thermo_nerf_amd.thermal_nerf.calculate_threshold import otsu_thresholds

    images = thermal_like(args.images, args.height, args.width)
    dev = [torch.from_numpy(im).cuda() for im in images]
    n = len(dev)

    def timed(fn):
        fn()  # warm-up
        torch.cuda.synchronize()
        ms = []
        for _ in range(args.repeats):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            ms.append(a.elapsed_time(b))
        return statistics.median(ms), min(ms), max(ms)

    packed = torch.cat([d.reshape(-1) for d in dev])
    offsets = (ctypes.c_int64 * (n + 1))(*([0] + list(np.cumsum([d.numel() for d in dev]))))
    hist = torch.empty((n, 256), dtype=torch.int32, device="cuda")
    thr = torch.empty((n,), dtype=torch.int32, device="cuda")
    lib = _hip.load()

    def call_only():
        _hip.check(lib.tn_otsu_thresholds(packed.data_ptr(), offsets, n, hist.data_ptr(), thr.data_ptr(), _hip.current_stream()), "tn_otsu_thresholds")

    t_call = timed(call_only)
    t_full = timed(lambda: otsu_thresholds(dev))
    got = thr.cpu().tolist()

    t0 = time.perf_counter()
    hists = [np.bincount(im.reshape(-1), minlength=256) for im in images]
    t1 = time.perf_counter()
    want = [otsu_restated(h) for h in hists]
    t2 = time.perf_counter()
    assert got == want and np.array_equal(hist.cpu().numpy(), np.stack(hists)), "device and restatement disagree"

    mb = packed.numel() / 1e6
    lines = [
        f"command: python tools/otsu_bench.py --images {args.images} --height {args.height} --width {args.width} --repeats {args.repeats}",
        f"device: {torch.cuda.get_device_name(0)}; {n} images of {args.width}x{args.height} uint8 = {mb:.1f} MB; thresholds {min(got)}..{max(got)} (equal to the restatement)",
        f"(a) tn_otsu_thresholds alone (memset + histogram launch(es) + threshold launch), HIP events: median {t_call[0] * 1e3:.1f} us (range {t_call[1] * 1e3:.1f} .. {t_call[2] * 1e3:.1f}) = {mb / t_call[0]:.1f} GB/s of pixels",
        f"(b) otsu_thresholds(): torch.cat packing + output allocation + (a): median {t_full[0] * 1e3:.1f} us (range {t_full[1] * 1e3:.1f} .. {t_full[2] * 1e3:.1f})",
        f"(c) numpy restatement on the host, one thread: np.bincount {1e3 * (t1 - t0):.1f} ms + recurrence in Python floats {1e3 * (t2 - t1):.1f} ms = {1e3 * (t2 - t0):.1f} ms",
    ]
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
