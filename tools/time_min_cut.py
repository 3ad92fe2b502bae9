"""Timing of the min-cut nucleus splitter on a synthetic full-size scene.

    python tools/time_min_cut.py [--reps 7] [--cpu-workers 16] [--scenes 16]

On 1040 x 1392 scenes of about 300 nuclei with about 10 % clumps (tests/min_cut_cases.py ``big_scene``) it reports, as median with min
and max over --reps passes after a warm-up pass,
  * the kernel time of the ecseg_min_cut calls of one image (ECSEG_T_COUNT, summed over the recursion levels),
  * the whole ``binary_seg_to_instance_min_cut`` of one image (labelling, centre search, device calls, relabelling, colours),
  * the centre search on the host alone,
and, as the baseline, the scipy restatement tests/min_cut_ref.py ``instance_min_cut`` of the same scenes on one core and on a pool
of --cpu-workers processes (seconds per image = wall time / scenes).  The labels of the device path are compared with the
restatement's on every scene.  Prints one JSON line.
"""
import argparse
import json
import os
import statistics
import sys
import time
from concurrent.futures import ProcessPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))


def _cpu_scene(seed):
    """-> (seconds of the restatement alone, its labels)."""
    import min_cut_cases as cases
    import min_cut_ref as ref
    mask = cases.big_scene(seed)
    t0 = time.perf_counter()
    labels, _ = ref.instance_min_cut(mask, 60, 1.25)
    return time.perf_counter() - t0, labels


def _mmm(values):
    return {'median': statistics.median(values), 'min': min(values), 'max': max(values)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--cpu-workers', type=int, default=16)
    ap.add_argument('--scenes', type=int, default=16)
    a = ap.parse_args()
    import min_cut_cases as cases
    from ecseg_amd import min_cut as mc
    from ecseg_amd._lib import Handle
    gpu = Handle(0)
    out = {'device': gpu.device_name, 'scenes': a.scenes, 'reps': a.reps}
    mask = cases.big_scene(0)
    whole, kernel, centers, stats = [], [], [], {}
    for rep in range(a.reps + 1):
        stats = {}
        t0 = time.perf_counter()
        labels, _ = mc.binary_seg_to_instance_min_cut(mask, 60, 1.25, handle=gpu, stats=stats)
        if rep:
            whole.append((time.perf_counter() - t0) * 1e3)
            kernel.append(stats.get('kernel_ms', 0.0))
            centers.append(stats['centers'] * 1e3)
    out.update(regions_before=int(np.unique(gpu.ccl_labels(mask, 4)).size - 1), cells_after=int(labels.max()), regions_cut=stats.get('regions', 0),
               tasks=stats.get('tasks', 0), device_calls=stats.get('calls', 0), kernel_ms=_mmm(kernel), whole_function_ms=_mmm(whole),
               centre_search_ms=_mmm(centers))
    one = [_cpu_scene(k) for k in range(min(a.scenes, 3))]
    out['cpu_one_core_s_per_image'] = _mmm([t for t, _ in one])
    out['labels_equal_to_the_restatement'] = bool(np.array_equal(one[0][1], labels))
    t0 = time.perf_counter()
    with ProcessPoolExecutor(a.cpu_workers) as pool:
        got = list(pool.map(_cpu_scene, range(a.scenes)))
    out['cpu_%d_workers_s_per_image' % a.cpu_workers] = (time.perf_counter() - t0) / a.scenes
    mism = 0
    for k in range(a.scenes):
        dev, _ = mc.binary_seg_to_instance_min_cut(cases.big_scene(k), 60, 1.25, handle=gpu)
        mism += not np.array_equal(dev, got[k][1])
    out['scenes_with_other_labels'] = mism
    gpu.close()
    print(json.dumps(out), flush=True)


if __name__ == '__main__':
    main()
