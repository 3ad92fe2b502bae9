#!/usr/bin/env python3
"""Device time of NuSeT's marker watershed and clean-up (ECSEG_T_COUNT of ecseg_marker_watershed and ecseg_clean_nuclei) at 304 x 416
and 1040 x 1392 on synthetic scenes of 300 nuclei, against the scipy parts of the restatement (fill holes + distance transform;
the labellings of clean_image) on one core of the same box.  Prints medians with minimum and maximum; sets no target.

    python tools/time_watershed.py [--repeats 5]"""
import argparse
import os
import sys
import time

import numpy as np
from scipy import ndimage as ndi

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..')
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import watershed_ref as wr                   # noqa: E402

from ecseg_amd import _lib                   # noqa: E402


def scene(h, w, n=300, seed=3):
    """n discs sized so that they cover about a quarter of the image, one marker per disc centre plus a few strays."""
    rng = np.random.default_rng(seed)
    m = np.zeros((h, w), np.uint8)
    r = max(2, int(np.sqrt(h * w / (4 * n * np.pi))))
    yy, xx = np.ogrid[:h, :w]
    rows, cols = [], []
    for _ in range(n):
        cy, cx = int(rng.integers(r, h - r)), int(rng.integers(r, w - r))
        m[(yy - cy) ** 2 + (xx - cx) ** 2 <= r * r] = 1
        rows.append(cy); cols.append(cx)
    return m, np.asarray(rows, np.int32), np.asarray(cols, np.int32), np.arange(1, n + 1, dtype=np.int32)


def stats(v):
    return 'median %.2f ms (min %.2f, max %.2f)' % (1e3 * np.median(v), 1e3 * min(v), 1e3 * max(v))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--repeats', type=int, default=5)
    a = ap.parse_args()
    handle = _lib.Handle(0)
    for h, w in ((304, 416), (1040, 1392)):
        m, rows, cols, labels = scene(h, w)
        ws = handle.marker_watershed(m, rows, cols, labels)            # warm-up (allocations)
        handle.clean_nuclei(ws, 20)
        t_ws, t_cl, c_edt, c_cl = [], [], [], []
        for _ in range(a.repeats):
            handle.marker_watershed(m, rows, cols, labels)
            t_ws.append(list(handle.timings().values())[4] / 1e3)
            handle.clean_nuclei(ws, 20)
            t_cl.append(list(handle.timings().values())[4] / 1e3)
            t0 = time.perf_counter(); wr.squared_distance(m); c_edt.append(time.perf_counter() - t0)
            t0 = time.perf_counter(); wr.final_mask(wr.clean_image(ws)[0], 20); c_cl.append(time.perf_counter() - t0)
        print('%d x %d, %d foreground pixels, %d repeats' % (h, w, int(m.sum()), a.repeats))
        print('  device marker_watershed   %s   (serial flood)' % stats(t_ws))
        print('  device clean_nuclei       %s' % stats(t_cl))
        print('  scipy fill_holes + edt    %s   (one core; the flood itself is not timed on the host)' % stats(c_edt))
        print('  scipy clean + threshold   %s   (one core)' % stats(c_cl))
    handle.close()


if __name__ == '__main__':
    main()
