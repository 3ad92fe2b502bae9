#!/usr/bin/env python3
"""Randomised parity campaign of ecseg_min_cut (csrc/mincut_kernels.hip) against the CPU oracle tests/min_cut_ref.py
``solve_scipy`` - side and max-flow value, exactly - beyond the fixed seeds of tests/test_gpu_min_cut.py: batches of seeded tasks from
tests/min_cut_cases.py ``random_task`` (overlapping discs, dense noise, windows with holes; windows up to --max-side, distances 1 ..
32), every batch once with the state in LDS and once forced into the global scratch region.  Runs for --seconds, prints one
line per failure and a summary; exit code 1 on any mismatch.  A failing seed becomes a fixed case in the test module.

    python tools/fuzz_min_cut.py --seconds 300 [--seed0 1000] [--batch 16] [--max-side 96]

    python tools/fuzz_min_cut.py --regions --seconds 300 [--seed0 5000]

is the seeded campaign of ecseg_min_cut_regions (csrc/mincut_centers_kernels.hip) instead: the scenes of
tests/min_cut_region_cases.py ``seeded_case`` from --seed0 on, every one with the per-crop state in LDS and in global memory, every
output against ``expected`` (tests/min_cut_ref.py).  It stops at the first difference (exit code 1).
"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))


def regions_campaign(seconds, seed0):
    import min_cut_region_cases as rc
    import test_gpu_min_cut_regions as T
    from ecseg_amd._lib import Handle
    gpu = Handle(0)
    t0, seed = time.time(), seed0
    try:
        while time.time() - t0 < seconds:
            case = rc.seeded_case(seed)
            want = rc.expected(*case)
            for lds in (T.LDS_PIXELS, 0):
                gpu.set_option('min_cut_centers_lds_pixels', lds)
                bad = T.mismatches(gpu, case, want)
                if bad:
                    print('seed %d (%s, coeff %s, min_rad %d, lds_pixels %d): %s' % (seed, case[0].shape, case[1], case[2], lds, '; '.join(bad)), flush=True)
                    return 1
            seed += 1
    finally:
        gpu.set_option('min_cut_centers_lds_pixels', T.LDS_PIXELS)
        gpu.close()
    print('min_cut_regions: %d scenes from seed %d, no difference' % (seed - seed0, seed0), flush=True)
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--regions', action='store_true')
    ap.add_argument('--seconds', type=float, default=300)
    ap.add_argument('--seed0', type=int, default=1000)
    ap.add_argument('--batch', type=int, default=16)
    ap.add_argument('--max-side', type=int, default=96)
    a = ap.parse_args()
    if a.regions:
        sys.exit(regions_campaign(a.seconds, a.seed0))
    import min_cut_cases as cases
    import min_cut_ref as ref
    import test_gpu_min_cut as T
    from ecseg_amd._lib import Handle
    gpu = Handle(0)
    t0 = time.time()
    seed = a.seed0
    n_cases = fails = 0
    while time.time() - t0 < a.seconds:
        groups = {}
        for k in range(a.batch):
            M, s, t, d = cases.random_task(seed + k, a.max_side)
            groups.setdefault(d, []).append((seed + k, (M, s, t)))
        for d, members in sorted(groups.items()):
            tasks = [m[1] for m in members]
            want = [ref.solve_scipy(M, s, t, d) for M, s, t in tasks]
            for lds in (T.LDS_PIXELS, 0):
                gpu.set_option('min_cut_lds_pixels', lds)
                for b in T.task_mismatches(gpu, tasks, d, want):
                    print('FAIL seeds %s, d %d, %s: %s' % ([m[0] for m in members], d, 'LDS' if lds else 'global', b), flush=True)
                    fails += 1
                n_cases += len(tasks)
        seed += a.batch
    gpu.close()
    print('min_cut fuzz campaign: seeds %d..%d, %d task solutions compared (each task in LDS and in global memory), %d failing, %.0f s'
          % (a.seed0, seed - 1, n_cases, fails, time.time() - t0), flush=True)
    sys.exit(1 if fails else 0)


if __name__ == '__main__':
    main()
