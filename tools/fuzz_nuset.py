#!/usr/bin/env python3
"""Randomised parity campaign of the proposal layer (ecseg_rpn_proposals, csrc/nuset_kernels.hip: decode, bitonic sort, IoU bit matrix,
greedy sweep) against its float32 restatement tests/nuset_ref.py - selected candidates and scores exactly, coordinates within 4
float32 spacings of the image extent - beyond the fixed seeds of tests/test_gpu_nuset.py: the cases of tests/nuset_cases.py
``random_case(seed, --max-positions)`` (1 .. 21 anchors on up to --max-positions squared positions; 64 reaches 86 016 candidates and a sort of
131 072 keys), all on ONE handle, so that calls of every size follow each other on the same buffers.  A seed whose case the float32
and float64 restatements decide differently (``nuset_ref.undecided``) is skipped and counted.  Runs for --seconds, prints one line
per failing seed and a summary; exit code 1 on any mismatch.  A failing seed becomes a fixed case in CAMPAIGN_REGRESSIONS of the
test module.

    python tools/fuzz_nuset.py --seconds 300 [--seed0 1000] [--max-positions 64]
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
    ap.add_argument('--max-positions', type=int, default=24)
    a = ap.parse_args()
    import nuset_cases as cases
    import nuset_ref as ref
    from ecseg_amd._lib import Handle
    gpu = Handle(0)
    t0 = time.time()
    seed = a.seed0
    n_cases = n_props = skipped = fails = unequal = largest = 0
    worst = 0.0
    while time.time() - t0 < a.seconds:
        c = cases.random_case(seed, a.max_positions)
        reason, want = ref.judge(c)
        if reason is not None:
            skipped += 1
        else:
            bad, err, ne = ref.case_mismatches(gpu, c, want)
            if bad:
                print('FAIL seed %d, max_positions %d (%s, %d x %d x %d, pre %d, post %d): %s'
                      % (seed, a.max_positions, c['mode'], c['cls'].shape[0], c['cls'].shape[1], c['A'], c['pre'], c['post'], '; '.join(bad)), flush=True)
                fails += 1
            n_cases += 1
            n_props += len(want['indices'])
            worst, unequal, largest = max(worst, err), unequal + ne, max(largest, c['cls'].size // 2)
        seed += 1
    gpu.close()
    print('nuset fuzz campaign: seeds %d..%d at up to %d positions a side, %d cases (%d proposals) compared, the largest of %d candidates, '
          '%d undecided seeds skipped, %d failing, max coordinate error %g, %d coordinates not bit-equal, %.0f s'
          % (a.seed0, seed - 1, a.max_positions, n_cases, n_props, largest, skipped, fails, worst, unequal, time.time() - t0), flush=True)
    sys.exit(1 if fails else 0)


if __name__ == '__main__':
    main()
