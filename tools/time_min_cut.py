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

    python tools/time_min_cut.py --regions-on-device off|on|alternate [--passes 3] [--leg-timeout 300]

times the whole ``binary_seg_to_instance_min_cut`` on the same scene with ``regions_on_device`` off, on, or - ``alternate`` - in the
legs off, on, off, on of one session: every leg is a child process under its own time limit, does one warm-up pass and then
--passes passes, and reports median (min - max) of the whole function, the 'centers' share (with the key on: the one device call
plus the record walk) and ECSEG_T_COUNT of ecseg_min_cut_regions.  The project's rule: the key is a gain only where the slowest
pass with it on is faster than the fastest pass with it off; the line says so in ``gain``.
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


def _leg(on, passes):
    """One leg in this process -> dict for the parent."""
    import min_cut_cases as cases
    from ecseg_amd import min_cut as mc
    from ecseg_amd._lib import Handle
    gpu = Handle(0)
    mask = cases.big_scene(0)
    whole, centers, call_ms = [], [], []
    for rep in range(passes + 1):
        stats = {}
        t0 = time.perf_counter()
        labels, _ = mc.binary_seg_to_instance_min_cut(mask, 60, 1.25, handle=gpu, stats=stats, regions_on_device=on)
        if rep:
            whole.append((time.perf_counter() - t0) * 1e3)
            centers.append(stats['centers'] * 1e3)
    if on:
        for _ in range(passes):
            gpu.min_cut_regions((mask != 0).astype(np.uint8), 1.25)
            call_ms.append(float(gpu.timings()['count']))
    out = {'on': on, 'whole_function_ms': _mmm(whole), 'centers_ms': _mmm(centers), 'cells': int(labels.max()),
           'labels_sha': __import__('hashlib').sha256(np.ascontiguousarray(labels).tobytes()).hexdigest()}
    if call_ms:
        out['min_cut_regions_kernel_ms'] = _mmm(call_ms)
    gpu.close()
    return out


def _legs(mode, passes, limit):
    import subprocess
    order = {'off': [False], 'on': [True], 'alternate': [False, True, False, True]}[mode]
    legs = []
    for on in order:                                         # a fresh child per leg, each under its own time limit
        cmd = [sys.executable, os.path.abspath(__file__), '--leg', 'on' if on else 'off', '--passes', str(passes)]
        try:
            got = subprocess.run(cmd, capture_output=True, text=True, timeout=limit)
        except subprocess.TimeoutExpired:
            print(json.dumps({'error': 'leg %s ran into its time limit of %d s' % ('on' if on else 'off', limit), 'legs': legs}), flush=True)
            return 1
        if got.returncode != 0:
            print(json.dumps({'error': 'leg failed', 'stderr': got.stderr[-2000:], 'legs': legs}), flush=True)
            return 1
        legs.append(json.loads(got.stdout.strip().splitlines()[-1]))
    out = {'mode': mode, 'passes': passes, 'legs': legs, 'labels_equal': len({leg['labels_sha'] for leg in legs}) == 1}
    offs = [leg['whole_function_ms'] for leg in legs if not leg['on']]
    ons = [leg['whole_function_ms'] for leg in legs if leg['on']]
    if offs and ons:
        out['fastest_off_ms'], out['slowest_on_ms'] = min(v['min'] for v in offs), max(v['max'] for v in ons)
        out['gain'] = out['slowest_on_ms'] < out['fastest_off_ms']
    print(json.dumps(out), flush=True)
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--cpu-workers', type=int, default=16)
    ap.add_argument('--scenes', type=int, default=16)
    ap.add_argument('--regions-on-device', choices=['off', 'on', 'alternate'])
    ap.add_argument('--passes', type=int, default=3)
    ap.add_argument('--leg-timeout', type=int, default=300)
    ap.add_argument('--leg', choices=['off', 'on'], help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.leg:
        print(json.dumps(_leg(a.leg == 'on', a.passes)), flush=True)
        return
    if a.regions_on_device:
        sys.exit(_legs(a.regions_on_device, a.passes, a.leg_timeout))
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
