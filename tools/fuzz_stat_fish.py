#!/usr/bin/env python3
"""Randomised parity campaign of ecseg_fish_spots (csrc/fishspot_kernels.hip) against the vectorised CPU oracle
tests/stat_fish_ref.py ``records`` - records, cleaned masks and boundaries, exactly - beyond the fixed seeds of
tests/test_gpu_stat_fish.py: cases come from that module's ``case_mismatches(seed)`` (blobby nuclei with gaps in the labels,
painted and filter-decided spots, 1 / 2 / 3 probes, K in {1, 3, 7, 15, 23}, line thickness 1..3, random sizes).  A case that
holds a pixel inside the derived 2 B band of the float64 decision is ambiguous: it is skipped and counted, and the count
is printed.  Runs for --seconds, prints one line per failure and a summary; exit code 1 on any mismatch.  A failing seed
becomes a fixed case in the test module.  --asymmetric replaces every scene's projected Gaussian by K x K standard-normal weights
without any symmetry, with the threshold between the two middle coefficients of the deciding pixels
(tests/test_gpu_peak_filter.py ``case_mismatches``): a mirrored or transposed tap index shows there, and both outcomes are common.

    python tools/fuzz_stat_fish.py --seconds 300 [--seed0 1000] [--seeds 3,17] [--asymmetric]
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
    ap.add_argument('--seed0', type=int, default=1000)
    ap.add_argument('--seeds', default=None, help='comma-separated list: run exactly these seeds')
    ap.add_argument('--asymmetric', action='store_true', help='asymmetric standard-normal kernels in place of the projected Gaussian')
    a = ap.parse_args()
    if a.asymmetric:
        import test_gpu_peak_filter as T
    else:
        import test_gpu_stat_fish as T
    from ecseg_amd._lib import Handle
    gpu = Handle(0)
    t0 = time.time()
    seed = a.seed0
    todo = [int(x) for x in a.seeds.split(',')] if a.seeds else None
    n_cases = n_ambiguous = fails = 0
    while time.time() - t0 < a.seconds:
        if todo is not None:
            if not todo:
                break
            seed = todo.pop(0)
        bad, ambiguous = T.case_mismatches(gpu, seed)
        if ambiguous:
            n_ambiguous += 1
        else:
            for b in bad:
                print('FAIL seed %d: %s' % (seed, b), flush=True)
            fails += len(bad) > 0
            n_cases += 1
        seed += 1
    gpu.close()
    print('stat_fish fuzz campaign%s: seeds %d..%d, %d cases compared, %d ambiguous case(s) skipped, %d failing case(s), %.0f s'
          % (' (asymmetric kernels)' if a.asymmetric else '', a.seed0, seed - 1, n_cases, n_ambiguous, fails, time.time() - t0), flush=True)
    sys.exit(1 if fails else 0)


if __name__ == '__main__':
    main()
