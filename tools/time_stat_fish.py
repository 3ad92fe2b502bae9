"""Timing of ``make stat_fish`` on synthetic full-size scenes.

    python tools/time_stat_fish.py [--images 16] [--reps 5] [--cpu-workers 16] [--channels 4] [--main-passes 3]

Per 1040 x 1392 scene with 300 nuclei (tests/stat_fish_cases.py ``full_size_scene``) it reports
  * device milliseconds per image of ecseg_fish_spots (ECSEG_T_COUNT: the kernels alone), of the nucleus labelling in front of
    it, and the wall time of the whole call (copies included), median and spread over --reps passes after a warm-up pass;
  * the time to read that image's two input files (the LZW RGB image and the mask TIFF);
  * device milliseconds and wall time of ecseg_fish_render, the call that composes the three colour files;
  * the files-in / files-out rate of ``main()`` on the folder: one warm-up pass, then the median with min and max of --main-passes
    passes;
  * the same scenes through the vectorised numpy / scipy restatement tests/stat_fish_ref.py ``records`` on one core and on a
    pool of --cpu-workers processes, as the baseline.
With ``--channels 4`` the scenes are four-channel ``.npy`` images (blue, green, red and an aqua channel made of the green one shifted
by 40 columns) and ``color_sensitivity`` has three entries: the third probe end to end.  Prints one JSON line.
"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time
from concurrent.futures import ProcessPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))


def _cpu_records(seed):
    """-> seconds of the restatement alone (the scene's synthesis is not part of the baseline)."""
    import stat_fish_cases as cases
    import stat_fish_ref as ref
    img, mask = cases.full_size_scene(seed)
    t0 = time.perf_counter()
    ref.records(img, ref.nuclei(mask), (1, 0), cases.proj_kernel(7, 3.0), 15.0, (70.0, 70.0), 7, 2)     # two probes, whatever --channels
    return time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--images', type=int, default=16)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--cpu-workers', type=int, default=16)
    ap.add_argument('--channels', type=int, default=3, choices=(3, 4))
    ap.add_argument('--main-passes', type=int, default=3)
    a = ap.parse_args()
    import yaml
    import stat_fish_cases as cases
    from ecseg_amd import image_io, stat_fish
    from ecseg_amd._lib import Handle
    gpu = Handle(0)
    out = {'images': a.images, 'channels': a.channels, 'device': gpu.device_name}
    probes, order = ((1, 0), (2, 1, 0)) if a.channels == 3 else ((1, 2, 3), (0, 1, 2, 3))
    with tempfile.TemporaryDirectory() as tmp:
        inp = os.path.join(tmp, 'in')
        os.makedirs(os.path.join(inp, 'nuclei_masks'))
        scenes = []
        for k in range(a.images):
            img, mask = cases.full_size_scene(100 + k)
            if a.channels == 4:                              # BGRA, as the reference indexes a .npy
                img = np.ascontiguousarray(np.dstack([img[..., 2], img[..., 1], img[..., 0], np.roll(img[..., 1], 40, axis=1)]))
                np.save(os.path.join(inp, 'img%03d.npy' % k), img)
            else:
                image_io.write_tiff_rgb8(os.path.join(inp, 'img%03d.tif' % k), img)
            scenes.append((img, mask))
            image_io.write_tiff_gray8(os.path.join(inp, 'nuclei_masks', 'img%03d.tif' % k), mask)
        w = stat_fish.gaussian_proj_kernel([7, 7], 3.0)
        kern, label, wall, nuclei, render_kern, render_wall = [], [], [], 0, [], []
        for rep in range(a.reps + 1):
            for img, mask in scenes:
                t0 = time.perf_counter()
                lab = gpu.ccl_labels(mask, 8)
                t_label = gpu.timings()['count']
                rec, thr, bnd = gpu.fish_spots(lab, img, probes, w, 15, (70,) * len(probes), 7, 2)
                t1 = time.perf_counter()
                t_spots = gpu.timings()['count']
                gpu.fish_render(img, order, thr, bnd)
                t2 = time.perf_counter()
                if rep:
                    kern.append(t_spots); label.append(t_label); wall.append((t1 - t0) * 1e3)
                    render_kern.append(gpu.timings()['count']); render_wall.append((t2 - t1) * 1e3)
                else:
                    nuclei += len(rec)
        out.update(nuclei_per_image=nuclei / a.images, kernel_ms_median=statistics.median(kern), kernel_ms_min=min(kern), kernel_ms_max=max(kern),
                   labelling_ms_median=statistics.median(label), call_wall_ms_median=statistics.median(wall),
                   render_kernel_ms_median=statistics.median(render_kern), render_kernel_ms_min=min(render_kern),
                   render_kernel_ms_max=max(render_kern), render_call_wall_ms_median=statistics.median(render_wall))
        reads = []
        for rep in range(a.reps):
            for k in range(a.images):
                t0 = time.perf_counter()
                image_io.imread(os.path.join(inp, 'img%03d.%s' % (k, 'tif' if a.channels == 3 else 'npy')))
                image_io.imread(os.path.join(inp, 'nuclei_masks', 'img%03d.tif' % k))
                reads.append((time.perf_counter() - t0) * 1e3)
        out['read_ms_median'] = statistics.median(reads)
        cfg = {'stat_fish': {'inpath': inp, 'scale': 1, 'use_min_cut': False, 'nuclei_size_T': 5000}}
        with open(os.path.join(tmp, 'config.yaml'), 'w') as f:
            yaml.safe_dump(cfg, f)
        if a.channels == 4:
            os.makedirs(os.path.join(tmp, 'src'))
            with open(os.path.join(tmp, 'src', 'stat_fish_params.yaml'), 'w') as f:
                f.write('color_sensitivity: [70, 70, 70]\n')
        cwd = os.getcwd()
        os.chdir(tmp)
        try:
            rates = []
            for rep in range(a.main_passes + 1):
                t0 = time.perf_counter()
                stat_fish.main([], handle=gpu)
                if rep:                                      # the first pass warms the arenas and the page cache
                    rates.append(a.images / (time.perf_counter() - t0))
        finally:
            os.chdir(cwd)
        out.update(main_images_per_s=statistics.median(rates), main_images_per_s_min=min(rates), main_images_per_s_max=max(rates))
    gpu.close()
    n_cpu = min(a.images, 4)
    one = [_cpu_records(100 + k) for k in range(n_cpu)]
    out['cpu_records_s_per_image_one_core'] = statistics.median(one)
    t0 = time.perf_counter()
    with ProcessPoolExecutor(a.cpu_workers) as pool:
        list(pool.map(_cpu_records, [100 + k for k in range(a.images)]))
    out['cpu_records_images_per_s_%d_workers' % a.cpu_workers] = a.images / (time.perf_counter() - t0)     # synthesis included in the wall time
    print(json.dumps(out))


if __name__ == '__main__':
    main()
