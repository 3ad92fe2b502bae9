#!/usr/bin/env python3
"""Randomised parity campaign of ecseg_fish_distances (csrc/fishdist_kernels.hip) against the vectorised CPU oracle
tests/fish_distance_ref.py ``records``, field by field, beyond the fixed seeds of tests/test_gpu_fish_distance.py: cases
come from that module's seeded generator ``_case(seed)`` (overlapping elliptical nuclei of random size with gaps in the
labels, spots spilling over cell borders, 2 / 3 / 4 channels, all colour assignments).  Runs for --seconds, prints one
line per failure and a summary; exit code 1 on any mismatch.  A failing seed becomes a fixed case in the test module.

    python tools/fuzz_fish_distance.py --seconds 300 [--seed0 1000] [--seeds 3,17] [--batch]

``--batch`` sends random chunks of 1 to 9 of those scenes through ecseg_fish_distances_batch (``Handle.fish_distances_many``) and
compares every image of a chunk with ``records``; a failure names the chunk's seed and the image.
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
    ap.add_argument('--batch', action='store_true', help='chunks of 1 to 9 scenes through the batched call')
    a = ap.parse_args()
    import numpy as np
    import test_gpu_fish_distance as T
    import test_gpu_fish_distance_batch as B
    from ecseg_amd._lib import Handle
    gpu = Handle(0)
    t0 = time.time()
    seed = a.seed0
    todo = [int(x) for x in a.seeds.split(',')] if a.seeds else None
    n_cases = n_cells = fails = 0
    while time.time() - t0 < a.seconds:
        if todo is not None:
            if not todo:
                break
            seed = todo.pop(0)
        if a.batch:
            rng = np.random.default_rng(seed)
            images = [T._case(int(rng.integers(0, 2 ** 31)))[:2] for _ in range(int(rng.integers(1, 10)))]
            fi, ci = [(0, 1), (1, 0), (0, 0), (1, 1)][int(rng.integers(0, 4))]
            bad, got = B.chunk_mismatches(gpu, images, fi, ci)
            for b in bad:
                print('FAIL chunk seed %d (%d images) fish=%d centromere=%d: %s' % (seed, len(images), fi, ci, b), flush=True)
            n_cells += sum(len(g) for g in got if not isinstance(g, Exception))
        else:
            lsq, seg, fi, ci = T._case(seed)
            bad, got = T._mismatches(gpu, lsq, seg, fi, ci)
            for b in bad:
                print('FAIL seed %d %dx%d C=%d fish=%d centromere=%d: %s' % ((seed,) + seg.shape + (lsq.shape[2], fi, ci, b)), flush=True)
            n_cells += len(got)
        fails += len(bad) > 0
        n_cases += 1
        seed += 1
    gpu.close()
    print('fish_distance fuzz campaign: seeds %d..%d, %d cases, %d cells, %d failing case(s), %.0f s'
          % (a.seed0, seed - 1, n_cases, n_cells, fails, time.time() - t0), flush=True)
    sys.exit(1 if fails else 0)


if __name__ == '__main__':
    main()
