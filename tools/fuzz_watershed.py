#!/usr/bin/env python3
"""Seeded device-vs-restatement campaign of NuSeT's marker watershed and clean-up (ecseg_marker_watershed, ecseg_clean_nuclei against
tests/watershed_ref.py) on one handle: ``random_case(seed)`` of tests/watershed_cases.py for ``--seconds`` or ``--cases``, byte
for byte, exit code 1 at the first difference (its seed belongs into ``REGRESSION_SEEDS``).

    python tools/fuzz_watershed.py --seconds 120 [--first-seed 300000] [--max-extent 128]"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..')
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import watershed_cases as wc                 # noqa: E402
import watershed_ref as wr                   # noqa: E402

from ecseg_amd import _lib, nuset            # noqa: E402


def check(handle, case):
    """-> the first stage that differs, or None."""
    mk = nuset.watershed_markers(case['scores'], case['proposals'], case['mask'], case['min_score'], handle)
    want_mk = wr.marker_list(case['scores'], case['proposals'], case['mask'], case['min_score'])
    if (mk is None) != (want_mk is None) or (mk is not None and not all(np.array_equal(a, b) for a, b in zip(mk, want_mk))):
        return 'markers'
    ws = case['mask'] if mk is None else handle.marker_watershed(case['mask'], *mk)
    want = wr.watershed(case['scores'], case['proposals'], case['mask'], case['min_score'])
    if not np.array_equal(ws, want):
        return 'marker_watershed (%d pixels)' % int((ws != want).sum())
    cl, mean = wr.clean_image(want)
    for t in case['sizes']:
        out, got_mean, got_cl = handle.clean_nuclei(ws, t, want_cleaned=True)
        if not np.array_equal(got_cl, cl) or not (got_mean == mean or (np.isnan(got_mean) and np.isnan(mean))):
            return 'clean_image'
        if not np.array_equal(out, wr.final_mask(cl, t)):
            return 'final mask at %d' % t
    return None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--seconds', type=float, default=120.0)
    ap.add_argument('--cases', type=int, default=0)
    ap.add_argument('--first-seed', type=int, default=300000)
    ap.add_argument('--max-extent', type=int, default=128)
    a = ap.parse_args()
    handle = _lib.Handle(0)
    t0, n, seed = time.time(), 0, a.first_seed
    try:
        while (n < a.cases) if a.cases else (time.time() - t0 < a.seconds):
            bad = check(handle, wc.random_case(seed, a.max_extent))
            if bad:
                print('seed %d: %s differs' % (seed, bad))
                return 1
            n, seed = n + 1, seed + 1
    finally:
        handle.close()
    print('fuzz_watershed: seeds %d..%d, %d cases in %.0f s, 0 failures' % (a.first_seed, seed - 1, n, time.time() - t0))
    return 0


if __name__ == '__main__':
    sys.exit(main())
