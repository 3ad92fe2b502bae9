#!/usr/bin/env python3
"""Randomised parity campaign of ecseg_overlay (run_overlay in csrc/overlay_kernels.hip) against the CPU oracle
(oracle/overlay.py with oracle/postproc.py) - the nine cells of the ``meta_overlay`` row, exactly - beyond the fixed seeds of
tests/test_gpu_overlay.py: cases come from that module's ``case_mismatches(gpu, seed)`` (label maps of seven kinds, bytes
above 3 and whole tiles of one class among them; fish blobs around the size threshold on, beside and diagonal to the
components; sensitivities, thresholds and channel counts of tests/overlay_cases.py; the committed extents and random ones up
to 200 x 260).  Prints one line per failing seed and a summary; exit code 1 on any mismatch.  A failing seed becomes a fixed
case in the test module.

    python tools/fuzz_overlay.py --seeds 1000:4000
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
    ap.add_argument('--seeds', default='1000:2000', help='A:B runs seeds A .. B - 1; a comma-separated list runs exactly those')
    a = ap.parse_args()
    if ':' in a.seeds:
        first, last = (int(x) for x in a.seeds.split(':'))
        todo = range(first, last)
    else:
        todo = [int(x) for x in a.seeds.split(',')]
    import test_gpu_overlay as T
    from ecseg_amd._lib import Handle
    gpu = Handle(0)
    t0 = time.time()
    failing = []
    for seed in todo:
        bad = T.case_mismatches(gpu, seed)
        for b in bad:
            print('FAIL seed %d: %s' % (seed, b), flush=True)
        if bad:
            failing.append(seed)
    gpu.close()
    print('overlay fuzz campaign: seeds %s, %d cases compared, %d failing case(s)%s, %.0f s'
          % (a.seeds, len(todo), len(failing), ': ' + ','.join(str(s) for s in failing) if failing else '', time.time() - t0), flush=True)
    sys.exit(1 if failing else 0)


if __name__ == '__main__':
    main()
