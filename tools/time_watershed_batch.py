#!/usr/bin/env python3
"""One batched marker watershed (ecseg_marker_watershed_batch: one flood wave per image) against the same images through N
sequential ecseg_marker_watershed calls, on the same handle in the same process: N different seeds of tools/time_watershed.py's
1040 x 1392 scene of 300 nuclei, N = 1, 4, 16 and 64.  One warm-up of both, then ``--passes`` passes of each, reported as median
[min, max] of the device time (ECSEG_T_COUNT, summed over the sequential calls) and of the wall time, with the factor between
the medians and the images per second of the batched call.  The batched results are compared with the sequential ones, byte for
byte.  Sets no target.

Every N runs in a child process of its own under a time limit sized to it; when one fails or runs out of time, the later ones are
not started.

    python tools/time_watershed_batch.py [--sizes 1,4,16,64] [--passes 5]"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..')
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from time_watershed import scene             # noqa: E402

H, W = 1040, 1392
SECONDS_PER_IMAGE = 6.0                      # a generous bound on one serial flood of this scene, for the time limits only


def spread(v):
    return '%9.1f [%9.1f, %9.1f]' % (np.median(v), min(v), max(v))


def one(n, passes):
    """-> the dict of one N (device and wall milliseconds of every pass)."""
    from ecseg_amd import _lib
    handle = _lib.Handle(0)
    scenes = [scene(H, W, seed=3 + k) for k in range(n)]
    masks, markers = [s[0] for s in scenes], [s[1:] for s in scenes]
    out = dict(n=n, passes=passes, foreground=[int(m.sum()) for m in masks], batch_dev=[], batch_wall=[], seq_dev=[], seq_wall=[])
    for p in range(passes + 1):                              # pass 0 is the warm-up (allocations, code objects)
        t0 = time.perf_counter()
        got = handle.marker_watershed_batch(masks, markers)
        wall = 1e3 * (time.perf_counter() - t0)
        dev = handle.timings()['count']
        t0 = time.perf_counter()
        sdev, want = 0.0, []
        for m, mk in zip(masks, markers):
            want.append(handle.marker_watershed(m, *mk))
            sdev += handle.timings()['count']
        swall = 1e3 * (time.perf_counter() - t0)
        if not all(np.array_equal(g, w) for g, w in zip(got, want)):
            raise SystemExit('N = %d: the batched call and the sequential calls differ' % n)
        print('  N = %d pass %d of %d: batched %.0f ms, sequential %.0f ms (wall)' % (n, p, passes, wall, swall), file=sys.stderr, flush=True)
        if p:
            out['batch_dev'].append(dev); out['batch_wall'].append(wall); out['seq_dev'].append(sdev); out['seq_wall'].append(swall)
    handle.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--sizes', default='1,4,16,64')
    ap.add_argument('--passes', type=int, default=5)
    ap.add_argument('--one', type=int, default=0, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.one:
        print('RESULT ' + json.dumps(one(a.one, a.passes)), flush=True)
        return
    print('%d x %d, 300 nuclei, one warm-up and %d passes; milliseconds as median [min, max]' % (H, W, a.passes))
    for n in (int(v) for v in a.sizes.split(',')):
        limit = 120 + (a.passes + 1) * (n + 1) * SECONDS_PER_IMAGE
        try:
            run = subprocess.run([sys.executable, os.path.abspath(__file__), '--one', str(n), '--passes', str(a.passes)], stdout=subprocess.PIPE,
                                 text=True, timeout=limit)                 # (the child's progress lines go straight to stderr)
        except subprocess.TimeoutExpired:
            print('N = %d did not finish within %d s: stopping here' % (n, limit))
            sys.exit(1)
        lines = [ln for ln in run.stdout.splitlines() if ln.startswith('RESULT ')]
        if run.returncode != 0 or not lines:
            print('N = %d failed (exit code %d): stopping here\n%s' % (n, run.returncode, run.stdout[-2000:]))
            sys.exit(1)
        r = json.loads(lines[-1][7:])
        print('N = %d (foreground %d .. %d pixels per image)' % (n, min(r['foreground']), max(r['foreground'])))
        for what, b, s in (('device', r['batch_dev'], r['seq_dev']), ('wall  ', r['batch_wall'], r['seq_wall'])):
            print('  %s  batched %s   sequential %s   factor %.2f   batched max %s sequential min' %
                  (what, spread(b), spread(s), np.median(s) / np.median(b), '<' if max(b) < min(s) else '>='))
        print('  batched: %.2f images/s by device time, %.2f by wall time; sequential: %.2f by wall time' %
              (1e3 * n / np.median(r['batch_dev']), 1e3 * n / np.median(r['batch_wall']), 1e3 * n / np.median(r['seq_wall'])), flush=True)


if __name__ == '__main__':
    main()
