#!/usr/bin/env python3
"""Seeded device-vs-restatement campaign of NuSeT's two rescale calls (ecseg_rescale_down, ecseg_rescale_mask_up against
tests/rescale_ref.py) on one handle: ``random_down(seed)`` and ``random_up(seed)`` of tests/rescale_cases.py for ``--seconds`` or
``--cases``, the filtered bytes, the float64 image bit for bit and the final masks byte for byte; exit code 1 at the first difference.

    timeout -k 10 200 python tools/fuzz_rescale.py --seconds 120 [--first-seed 300000] [--max-extent 160]

Run it under a time limit of its own, as above, and start nothing more on the device after a failure."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..')
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import rescale_cases as rc                   # noqa: E402
import rescale_ref as rr                     # noqa: E402

from ecseg_amd import _lib                   # noqa: E402


def check(handle, seed, max_extent):
    """-> the first stage that differs, or None."""
    c = rc.random_down(seed, max_extent)
    out, filtered = handle.rescale_down(c['image'], c['scale'])
    want, want_f = rr.rescale_down(c['image'], c['scale'])
    if not np.array_equal(filtered, want_f):
        return 'rescale_down: filtered (%d bytes)' % int((filtered != want_f).sum())
    if out.shape != want.shape or out.tobytes() != want.tobytes():
        return 'rescale_down: float64 image'
    c = rc.random_up(seed, max(2, max_extent * 3 // 5))
    for t in c['sizes']:
        if not np.array_equal(handle.rescale_mask_up(c['mask'], c['scale'], t), rr.rescale_mask_up(c['mask'], c['scale'], t)):
            return 'rescale_mask_up at %d' % t
    return None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--seconds', type=float, default=120.0)
    ap.add_argument('--cases', type=int, default=0)
    ap.add_argument('--first-seed', type=int, default=300000)
    ap.add_argument('--max-extent', type=int, default=160)
    a = ap.parse_args()
    handle = _lib.Handle(0)
    t0, n, seed = time.time(), 0, a.first_seed
    try:
        while (n < a.cases) if a.cases else (time.time() - t0 < a.seconds):
            bad = check(handle, seed, a.max_extent)
            if bad:
                print('seed %d: %s differs' % (seed, bad))
                return 1
            n, seed = n + 1, seed + 1
    finally:
        handle.close()
    print('fuzz_rescale: seeds %d..%d, %d down and %d up cases in %.0f s, 0 failures' % (a.first_seed, seed - 1, n, n, time.time() - t0))
    return 0


if __name__ == '__main__':
    sys.exit(main())
