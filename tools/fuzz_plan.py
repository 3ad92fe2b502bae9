#!/usr/bin/env python3
"""Randomised campaign of ``keras_plan.build_plan`` + ``load_plan`` on the device against the float64 interpreter of the Keras graph
(tests/plan_ref.py), beyond the N_SEEDS fixed seeds of tests/test_gpu_plan.py: cases come from ``plan_cases.random_graph(seed)`` (a DAG
of 6 to 20 layers over the vocabulary of the hand cases, random skip connections, weights redrawn until A stays within 1e3 of
|y|.max()), run with ``fuse=True`` and ``fuse=False`` and held to |device - y| <= C_BOUND * 2^-24 * A on every output element.  Prints
one line per failing seed and a summary; exit code 1 on any mismatch.  A failing seed becomes a committed case in tests/plan_cases.py.

    python tools/fuzz_plan.py --seeds 1000:4000
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
    ap.add_argument('--seeds', default='1000:1200', help='A:B runs seeds A .. B - 1; a comma-separated list runs exactly those')
    a = ap.parse_args()
    if ':' in a.seeds:
        first, last = (int(x) for x in a.seeds.split(':'))
        todo = range(first, last)
    else:
        todo = [int(x) for x in a.seeds.split(',')]
    import plan_cases
    import test_gpu_plan as T
    from ecseg_amd._lib import Handle
    gpu = Handle(0)
    t0 = time.time()
    failing, worst = [], 0.0
    for seed in todo:
        bad, ratio = T.case_mismatches(gpu, plan_cases.random_graph(seed))
        worst = max(worst, ratio)
        for b in bad:
            print('FAIL seed %d: %s' % (seed, b), flush=True)
        if bad:
            failing.append(seed)
    gpu.close()
    print('plan fuzz campaign: seeds %s, %d graphs compared, worst ratio %.4f of the bound, %d failing seed(s)%s, %.0f s'
          % (a.seeds, len(todo), worst, len(failing), ': ' + ','.join(str(s) for s in failing) if failing else '', time.time() - t0), flush=True)
    sys.exit(1 if failing else 0)


if __name__ == '__main__':
    main()
