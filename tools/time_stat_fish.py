"""Timing of ``make stat_fish`` on synthetic full-size scenes.

    python tools/time_stat_fish.py [--images 16] [--reps 5] [--cpu-workers 16] [--channels 4] [--main-passes 3]
                                   [--tiff-on-device off|on|alternate] [--tiff-read-on-device off|on|alternate] [--tiff-read-batch K] [--tiff-write-batch K] [--batch K] [--no-cpu-baseline]

Per 1040 x 1392 scene with 300 nuclei (tests/stat_fish_cases.py ``full_size_scene``) it reports
  * device milliseconds per image of ecseg_fish_spots (ECSEG_T_COUNT: the kernels alone), of the nucleus labelling in front of
    it, and the wall time of the whole call (copies included), median and spread over --reps passes after a warm-up pass;
  * the time to read that image's two input files (the LZW RGB image and the mask TIFF);
  * device milliseconds and wall time of ecseg_fish_render, the call that composes the three colour files;
  * the files-in / files-out rate of ``main()`` on the folder: one warm-up pass, then the median with min and max of --main-passes
    passes, and the write stage of ``process_image`` per image over those passes;
  * with ``--tiff-on-device on`` the same under the config key ``tiff_on_device: true`` (every TIFF LZW-encoded on the device), with
    ``alternate`` key off and key on in turn, twice, each with its own warm-up pass (``main_by_key``); either way the device
    milliseconds (render + encode for the first) and the wall time of ecseg_fish_render_tiff and of ecseg_tiff_encode of the mask;
  * with ``--tiff-read-on-device on`` ``main()`` runs under ``tiff_read_on_device: true`` (the input TIFFs decoded on the device), with
    ``alternate`` that key off and on in turn, twice (``main_by_read_key``; ``--tiff-on-device on`` then holds in all four), and the read
    stage of ``process_image`` per image is reported beside the write stage;
  * with ``--tiff-read-batch K`` (K above 1) ``tiff_read_on_device: true`` holds throughout and ``tiff_read_batch`` 1 and K alternate,
    twice (``main_by_read_batch``); the read stage then includes the chunks that ``main()`` reads ahead;
  * with ``--batch K`` (K above 1) ``tiff_on_device: true`` holds throughout - and the read keys as given - and ``stat_fish.batch`` 1 and K
    alternate, twice (``main_by_batch``): images/s, the read / device / write stage per image and ``encode_kernel_ms_per_image``, which
    then is ECSEG_T_COUNT of every encoding or chunk call (``stat_fish_many`` holds labelling, spots, render and encode) per image;
  * with ``--tiff-write-batch K`` (K above 1) ``tiff_on_device: true`` holds throughout - and the read keys as given, ``--tiff-read-batch``
    as a fixed value - and ``tiff_write_batch`` 1 and K alternate, twice (``main_by_write_batch``); the write stage then includes the
    chunks that ``main()`` writes, and ``encode_kernel_ms_per_image`` is ECSEG_T_COUNT of the encoding calls (``fish_render_tiff`` and
    ``tiff_encode``, or ``fish_render_tiff_many``) per image;
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
    ap.add_argument('--tiff-on-device', choices=('off', 'on', 'alternate'), default='off')
    ap.add_argument('--tiff-read-on-device', choices=('off', 'on', 'alternate'), default='off')
    ap.add_argument('--tiff-read-batch', type=int, default=1, help='with --tiff-read-on-device on: tiff_read_batch 1 and this value alternate, twice')
    ap.add_argument('--tiff-write-batch', type=int, default=1, help='with tiff_on_device on: tiff_write_batch 1 and this value alternate, twice')
    ap.add_argument('--batch', type=int, default=1, help='with tiff_on_device on: stat_fish.batch 1 and this value alternate, twice')
    ap.add_argument('--no-cpu-baseline', action='store_true')
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
        tiff = {k: [] for k in ('render_tiff_kernel_ms', 'render_tiff_wall_ms', 'mask_tiff_kernel_ms', 'mask_tiff_wall_ms')}
        with_tiff = a.tiff_on_device != 'off'
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
                t_render = gpu.timings()['count']
                if with_tiff:
                    gpu.fish_render_tiff(img, order, thr, bnd)
                    t3 = time.perf_counter()
                    t_files = gpu.timings()['count']
                    gpu.tiff_encode(mask)
                    t4 = time.perf_counter()
                    if rep:
                        tiff['render_tiff_kernel_ms'].append(t_files); tiff['render_tiff_wall_ms'].append((t3 - t2) * 1e3)
                        tiff['mask_tiff_kernel_ms'].append(gpu.timings()['count']); tiff['mask_tiff_wall_ms'].append((t4 - t3) * 1e3)
                if rep:
                    kern.append(t_spots); label.append(t_label); wall.append((t1 - t0) * 1e3)
                    render_kern.append(t_render); render_wall.append((t2 - t1) * 1e3)
                else:
                    nuclei += len(rec)
        out.update(nuclei_per_image=nuclei / a.images, kernel_ms_median=statistics.median(kern), kernel_ms_min=min(kern), kernel_ms_max=max(kern),
                   labelling_ms_median=statistics.median(label), call_wall_ms_median=statistics.median(wall),
                   render_kernel_ms_median=statistics.median(render_kern), render_kernel_ms_min=min(render_kern),
                   render_kernel_ms_max=max(render_kern), render_call_wall_ms_median=statistics.median(render_wall))
        for k, v in tiff.items():
            if v:
                out.update({k + '_median': statistics.median(v), k + '_min': min(v), k + '_max': max(v)})
        reads = []
        for rep in range(a.reps):
            for k in range(a.images):
                t0 = time.perf_counter()
                image_io.imread(os.path.join(inp, 'img%03d.%s' % (k, 'tif' if a.channels == 3 else 'npy')))
                image_io.imread(os.path.join(inp, 'nuclei_masks', 'img%03d.tif' % k))
                reads.append((time.perf_counter() - t0) * 1e3)
        out['read_ms_median'] = statistics.median(reads)
        if a.channels == 4:
            os.makedirs(os.path.join(tmp, 'src'))
            with open(os.path.join(tmp, 'src', 'stat_fish_params.yaml'), 'w') as f:
                f.write('color_sensitivity: [70, 70, 70]\n')
        seen = {}
        process_image = stat_fish.process_image

        def spy(*args, **kw):                                # main()'s stage times: it hands every image the same dict, and adds its flushes to it
            seen['stats'] = kw['stats']
            return process_image(*args, **kw)

        prepare_image = stat_fish.prepare_image

        def spy_prepare(*args, **kw):
            seen['stats'] = kw['stats']
            return prepare_image(*args, **kw)

        encode_ms = []
        for name in ('fish_render_tiff', 'tiff_encode', 'fish_render_tiff_many', 'stat_fish_many'):     # ECSEG_T_COUNT of every encoding call of main()
            def timed(*args, _call=getattr(gpu, name), **kw):
                r = _call(*args, **kw)
                encode_ms.append(gpu.timings()['count'])
                return r
            setattr(gpu, name, timed)

        def passes(key, read_key=False, read_batch=1, write_batch=1, fish_batch=1):
            """One warm-up pass (arenas, page cache) and --main-passes timed ones -> images/s of each, write stage ms per image."""
            cfg = {'stat_fish': {'inpath': inp, 'scale': 1, 'use_min_cut': False, 'nuclei_size_T': 5000}}
            if key:
                cfg['stat_fish']['tiff_on_device'] = True
            if read_key:
                cfg['stat_fish']['tiff_read_on_device'] = True
            if read_batch > 1:
                cfg['stat_fish']['tiff_read_batch'] = read_batch
            if write_batch > 1:
                cfg['stat_fish']['tiff_write_batch'] = write_batch
            if fish_batch > 1:
                cfg['stat_fish']['batch'] = fish_batch
            with open(os.path.join(tmp, 'config.yaml'), 'w') as f:
                yaml.safe_dump(cfg, f)
            rates, writes, stage_reads, encodes, devices = [], [], [], [], []
            for rep in range(a.main_passes + 1):
                t0 = time.perf_counter()
                del encode_ms[:]
                stat_fish.main([], handle=gpu)
                if rep:
                    rates.append(a.images / (time.perf_counter() - t0))
                    writes.append(seen['stats']['write'] * 1e3 / a.images)
                    stage_reads.append(seen['stats']['read'] * 1e3 / a.images)
                    encodes.append(sum(encode_ms) / a.images)
                    devices.append(seen['stats'].get('device', 0.0) * 1e3 / a.images)
                seen.clear()
            return rates, writes, stage_reads, encodes, devices

        def summary(rates, writes, stage_reads, encodes, devices):
            return dict(main_images_per_s=statistics.median(rates), main_images_per_s_min=min(rates), main_images_per_s_max=max(rates),
                        write_stage_ms_per_image=statistics.median(writes), read_stage_ms_per_image=statistics.median(stage_reads),
                        encode_kernel_ms_per_image=statistics.median(encodes), encode_kernel_ms_per_image_min=min(encodes),
                        encode_kernel_ms_per_image_max=max(encodes), device_stage_ms_per_image=statistics.median(devices))
        cwd = os.getcwd()
        os.chdir(tmp)
        stat_fish.process_image = spy
        stat_fish.prepare_image = spy_prepare
        try:
            if a.batch > 1:                                       # tiff_on_device on throughout, stat_fish.batch 1 and K alternating, twice
                r_on = a.tiff_read_on_device == 'on'
                rb = a.tiff_read_batch if r_on else 1
                out['main_by_batch'] = [dict(tiff_on_device=True, tiff_read_on_device=r_on, tiff_read_batch=rb, batch=k, **summary(*passes(True, r_on, rb, 1, k)))
                                        for k in (1, a.batch, 1, a.batch)]
                ones = [r for r in out['main_by_batch'] if r['batch'] == 1]
                many = [r for r in out['main_by_batch'] if r['batch'] > 1]
                out['max_1_below_min_k'] = max(r['main_images_per_s_max'] for r in ones) < min(r['main_images_per_s_min'] for r in many)
                out['max_k_below_min_1'] = max(r['main_images_per_s_max'] for r in many) < min(r['main_images_per_s_min'] for r in ones)
                out.update(ones[0])
            elif a.tiff_write_batch > 1:                            # tiff_on_device on throughout, tiff_write_batch 1 and K alternating, twice
                r_on = a.tiff_read_on_device == 'on'
                out['main_by_write_batch'] = [dict(tiff_on_device=True, tiff_read_on_device=r_on, tiff_read_batch=a.tiff_read_batch if r_on else 1,
                                                   tiff_write_batch=k, **summary(*passes(True, r_on, a.tiff_read_batch if r_on else 1, k)))
                                              for k in (1, a.tiff_write_batch, 1, a.tiff_write_batch)]
                ones = [r for r in out['main_by_write_batch'] if r['tiff_write_batch'] == 1]
                many = [r for r in out['main_by_write_batch'] if r['tiff_write_batch'] > 1]
                out['max_1_below_min_k'] = max(r['main_images_per_s_max'] for r in ones) < min(r['main_images_per_s_min'] for r in many)
                out['max_k_below_min_1'] = max(r['main_images_per_s_max'] for r in many) < min(r['main_images_per_s_min'] for r in ones)
                out.update(ones[0])
            elif a.tiff_read_batch > 1:                           # the read key on throughout, tiff_read_batch 1 and K alternating, twice
                w = a.tiff_on_device == 'on'
                out['main_by_read_batch'] = [dict(tiff_on_device=w, tiff_read_on_device=True, tiff_read_batch=k, **summary(*passes(w, True, k)))
                                             for k in (1, a.tiff_read_batch, 1, a.tiff_read_batch)]
                ones = [r for r in out['main_by_read_batch'] if r['tiff_read_batch'] == 1]
                many = [r for r in out['main_by_read_batch'] if r['tiff_read_batch'] > 1]
                out['max_1_below_min_k'] = max(r['main_images_per_s_max'] for r in ones) < min(r['main_images_per_s_min'] for r in many)
                out['max_k_below_min_1'] = max(r['main_images_per_s_max'] for r in many) < min(r['main_images_per_s_min'] for r in ones)
                out.update(ones[0])
            elif a.tiff_read_on_device == 'alternate':
                w = a.tiff_on_device == 'on'
                out['main_by_read_key'] = [dict(tiff_on_device=w, tiff_read_on_device=key, **summary(*passes(w, key))) for key in (False, True, False, True)]
                offs = [r for r in out['main_by_read_key'] if not r['tiff_read_on_device']]
                ons = [r for r in out['main_by_read_key'] if r['tiff_read_on_device']]
                out['max_off_below_min_on'] = max(r['main_images_per_s_max'] for r in offs) < min(r['main_images_per_s_min'] for r in ons)
                out.update(offs[0])
            elif a.tiff_on_device == 'alternate':
                out['main_by_key'] = [dict(tiff_on_device=key, **summary(*passes(key))) for key in (False, True, False, True)]
                offs = [r for r in out['main_by_key'] if not r['tiff_on_device']]
                ons = [r for r in out['main_by_key'] if r['tiff_on_device']]
                out['max_off_below_min_on'] = max(r['main_images_per_s_max'] for r in offs) < min(r['main_images_per_s_min'] for r in ons)
                out.update(offs[0])
            else:
                out.update(tiff_on_device=a.tiff_on_device == 'on', tiff_read_on_device=a.tiff_read_on_device == 'on',
                           **summary(*passes(a.tiff_on_device == 'on', a.tiff_read_on_device == 'on')))
        finally:
            stat_fish.process_image = process_image
            stat_fish.prepare_image = prepare_image
            os.chdir(cwd)
    gpu.close()
    if a.no_cpu_baseline:
        print(json.dumps(out))
        return
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
