#!/usr/bin/env python3
"""Randomised parity campaign of the interSeg region and crop kernels (ecseg_nuclei_regions / ecseg_nucleus_crops) against
the exact CPU reference oracle/interseg.py, bit for bit, beyond the fixed seeds of tests/test_gpu_interseg_kernels.py:
cases come from that module's seeded generator ``_interseg_case(seed)`` (blob / speckle / lattice / thin / shape masks of
random size, 1 / 3 / 4 channels, random channel orders, up to a few hundred crops).  Runs for --seconds, prints one line
per failure and a summary; exit code 1 on any mismatch.  A failing seed becomes a fixed case in the test module.

    python tools/fuzz_interseg.py --seconds 300 [--seed0 0] [--seeds 3,17]
"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--seconds', type=float, default=300)
    ap.add_argument('--seed0', type=int, default=0)
    ap.add_argument('--seeds', default=None, help='comma-separated list: run exactly these seeds')
    a = ap.parse_args()
    import test_gpu_interseg_kernels as T
    from ecseg_amd._lib import Handle
    gpu = Handle(0)
    t0 = time.time()
    seed = a.seed0
    todo = [int(x) for x in a.seeds.split(',')] if a.seeds else None
    n_cases = n_regions = n_crops = fails = 0
    while time.time() - t0 < a.seconds:
        if todo is not None:
            if not todo:
                break
            seed = todo.pop(0)
        seg, img, channel0, desc, order = T._interseg_case(seed)
        H, W = seg.shape
        bad, rec, _, crops = T._mismatches(gpu, seg, img, channel0, desc, order)
        for b in bad:
            print('FAIL seed %d %dx%d C=%d channel0=%d order=%s: %s' % (seed, H, W, img.shape[2], channel0, order, b), flush=True)
        fails += len(bad) > 0
        n_cases += 1
        n_regions += len(rec)
        n_crops += 0 if crops is None else len(crops)
        seed += 1
    gpu.close()
    print('interseg fuzz campaign: seeds %d..%d, %d cases, %d regions, %d crops, %d failing case(s), %.0f s'
          % (a.seed0, seed - 1, n_cases, n_regions, n_crops, fails, time.time() - t0), flush=True)
    sys.exit(1 if fails else 0)


if __name__ == '__main__':
    main()
