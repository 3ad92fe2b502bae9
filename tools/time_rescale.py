#!/usr/bin/env python3
"""Timing of NuSeT's rescale step at the reference's default ``scale_ratio`` 0.3 on a 1040 x 1392 image: device time of
ecseg_rescale_down and ecseg_rescale_mask_up (ECSEG_T_COUNT) and their wall time, the numpy restatement (tests/rescale_ref.py) on one
core, and ``NuSeT.segment`` end to end on seeded base-64 weights at ``scale_ratio`` 1 against 0.3: median, minimum and maximum of
``--reps`` passes after a warm-up.  Prints one JSON line.

    python tools/time_rescale.py [--base 64] [--reps 5] [--size 1040x1392] [--scale-ratio 0.3]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..')
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import rescale_ref as ref                                # noqa: E402
from ecseg_amd import _lib, nuset, synth                 # noqa: E402


def stats(v):
    return dict(median=float(np.median(v)), min=float(np.min(v)), max=float(np.max(v)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--base', type=int, default=64)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--size', default='1040x1392')
    ap.add_argument('--scale-ratio', type=float, default=0.3)
    ap.add_argument('--min-score', type=float, default=0.5)
    args = ap.parse_args()
    if args.reps < 3:
        ap.error('--reps must be at least 3')
    H, W = (int(v) for v in args.size.split('x'))
    s = args.scale_ratio
    h = _lib.Handle(0)
    img = np.ascontiguousarray(synth.dapi_image(3, H, W), np.uint8)
    small = h.rescale_down(img, s)[0]                        # warm-up
    cleaned = (small[:small.shape[0] // 16 * 16, :small.shape[1] // 16 * 16] > small.mean()).astype(np.uint8)
    h.rescale_mask_up(cleaned, 1 / s, 100)
    down_ms, down_wall, up_ms, up_wall = [], [], [], []
    for _ in range(args.reps):
        t0 = time.perf_counter()
        out, filtered = h.rescale_down(img, s)
        down_wall.append((time.perf_counter() - t0) * 1e3)
        down_ms.append(h.timings()['count'])
        t0 = time.perf_counter()
        up = h.rescale_mask_up(cleaned, 1 / s, 100)
        up_wall.append((time.perf_counter() - t0) * 1e3)
        up_ms.append(h.timings()['count'])
    t0 = time.perf_counter()
    want, want_f = ref.rescale_down(img, s)
    numpy_down_ms = (time.perf_counter() - t0) * 1e3
    t0 = time.perf_counter()
    want_up = ref.rescale_mask_up(cleaned, 1 / s, 100)
    numpy_up_ms = (time.perf_counter() - t0) * 1e3
    same = bool(np.array_equal(filtered, want_f) and out.tobytes() == want.tobytes() and np.array_equal(up, want_up))

    weights = nuset.synth_weights(nuset.nuset_config(16, 16, args.base), seed=0)
    net = nuset.NuSeT(weights, base=args.base, handle=h)
    seg = {}
    for ratio in (1, s):
        net.segment(img, args.min_score, 0.1, 100, scale_ratio=ratio)      # loads the plan, warms up
        wall = []
        for _ in range(args.reps):
            t0 = time.perf_counter()
            m = net.segment(img, args.min_score, 0.1, 100, scale_ratio=ratio)
            wall.append((time.perf_counter() - t0) * 1e3)
        seg[str(ratio)] = dict(wall_ms=stats(wall), mask_shape=list(m.shape), foreground=float((m != 0).mean()))
    print(json.dumps(dict(size=[H, W], scale_ratio=s, small=list(out.shape), base=args.base, device=h.device_name, reps=args.reps,
                          down_device_ms=stats(down_ms), down_wall_ms=stats(down_wall), up_device_ms=stats(up_ms), up_wall_ms=stats(up_wall),
                          numpy_down_ms=numpy_down_ms, numpy_up_ms=numpy_up_ms, same_as_numpy=same, segment=seg)), flush=True)
    h.close()


if __name__ == '__main__':
    main()
