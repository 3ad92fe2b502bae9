"""Timing of ``make fish_distance_calculation`` on synthetic stat_fish output.

    python tools/time_fish_distance.py [--images 16] [--nuclei 300] [--height 1040] [--width 1392] [--reps 5] [--cpu-workers 16]

Per 1040 x 1392 scene with a few hundred nuclei it reports
  * device milliseconds per image of ecseg_fish_distances (ECSEG_T_COUNT: the kernels alone) and the wall time of the
    whole call (copies included), median and spread over --reps passes after one warm-up pass;
  * the time to read that image's two input files (np.load of the int64 label map + image_io.imread of the LZW RGB
    lsq TIFF), the relation the target has to hold: the kernels take less time than the reads;
  * the files-in / CSV-out rate of ``main()`` on the folder;
  * the same scenes through the CPU baselines tests/fish_distance_ref.py ``loop`` (the reference's per-pixel loop) and
    ``records`` (vectorised numpy) on a pool of --cpu-workers processes.
Prints one JSON line.

    python tools/time_fish_distance.py --batch 8 alternate [--images 32] [--io-threads N]

``alternate`` runs ``main()`` over one such folder with ``batch`` 1, k, 1, k: per leg one warm-up pass and three timed passes, and
prints one JSON line with, per leg, the images per second of every pass (median, min, max) and the seconds each pass spent reading
(at ``batch`` above 1: waiting for the reader threads), in the device call with what prepares it, and on the rows.  By the project's
rule ``batch: k`` is a gain only where the minimum of its legs lies above the maximum of the ``batch: 1`` legs.
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


def synth_scene(seed, H, W, n_nuclei):
    """Instance-label map of elliptical nuclei (radius 15-40) and an lsq image with 1-3 red and 1-2 green spots of a few
    dozen pixels per nucleus, channel 2 the nucleus boundaries."""
    rng = np.random.default_rng(seed)
    yy, xx = np.ogrid[:H, :W]
    seg = np.zeros((H, W), np.int64)
    lsq = np.zeros((H, W, 3), np.uint8)
    for k in range(n_nuclei):
        ry, rx = int(rng.integers(15, 40)), int(rng.integers(15, 40))
        cy, cx = int(rng.integers(ry, H - ry)), int(rng.integers(rx, W - rx))
        seg[((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2 <= 1.0] = k + 1
        for ch, n in ((0, int(rng.integers(1, 4))), (1, int(rng.integers(1, 3)))):
            for _ in range(n):
                r = int(rng.integers(2, 5))
                sy, sx = cy + int(rng.integers(-ry // 2, ry // 2 + 1)), cx + int(rng.integers(-rx // 2, rx // 2 + 1))
                lsq[max(sy - r, 0):sy + r + 1, max(sx - r, 0):sx + r + 1, ch][
                    np.hypot(*np.ogrid[max(sy - r, 0) - sy:min(sy + r + 1, H) - sy, max(sx - r, 0) - sx:min(sx + r + 1, W) - sx]) <= r] = 255
    edge = np.zeros((H, W), bool)
    edge[:, 1:] |= seg[:, 1:] != seg[:, :-1]
    edge[1:, :] |= seg[1:, :] != seg[:-1, :]
    lsq[..., 2] = edge * 255
    return lsq, seg


def _cpu_loop(job):
    """-> (values, seconds of the loop alone: the scene's synthesis is not part of the baseline)."""
    import fish_distance_ref as ref
    lsq, seg = synth_scene(*job)
    t0 = time.perf_counter()
    n = len(ref.loop(lsq, seg, (1, 0, 3)))
    return n, time.perf_counter() - t0


def _cpu_records(job):
    import fish_distance_ref as ref
    lsq, seg = synth_scene(*job)
    t0 = time.perf_counter()
    n = len(ref.records(lsq, seg, 0, 1))
    return n, time.perf_counter() - t0


def _stats(xs):
    return {'median': round(statistics.median(xs), 4), 'min': round(min(xs), 4), 'max': round(max(xs), 4)}


def write_folder(inp, data):
    """the scenes as stat_fish leaves them under ``inp``"""
    from PIL import Image

    from ecseg_amd import image_io
    for k, (lsq, seg) in enumerate(data):
        name = 'img_%03d' % k
        d = os.path.join(inp, 'annotated', name)
        os.makedirs(d)
        image_io.write_tiff_gray8(os.path.join(inp, name + '.tif'), np.zeros((4, 4), np.uint8))
        np.save(os.path.join(d, name + '__segmentation_min_cut.npy'), seg)
        Image.fromarray(lsq).save(os.path.join(d, name + '_lsq_t.tif'), compression='tiff_lzw')


def alternate(a):
    """``main()`` with batch 1, k, 1, k over one folder -> the JSON line of the module docstring"""
    import yaml

    from ecseg_amd import fish_distance_calculation as fdc
    from ecseg_amd._lib import Handle
    data = [synth_scene(2000 + k, a.height, a.width, a.nuclei) for k in range(a.images)]
    out = {'images': a.images, 'shape': [a.height, a.width], 'batch': a.batch, 'passes_per_leg': 3, 'legs': []}
    h = Handle(0)
    with tempfile.TemporaryDirectory() as tmp:
        inp = os.path.join(tmp, 'in')
        write_folder(inp, data)
        cwd = os.getcwd()
        os.chdir(tmp)
        devnull = open(os.devnull, 'w')
        try:
            csvs = []
            for k in (1, a.batch, 1, a.batch):
                var = {'inpath': inp, 'centromere_probe_color': 'green', 'fish_probe_color': 'red', 'max_centromeric_spots': 3, 'batch': k}
                if a.io_threads:
                    var['io_threads'] = a.io_threads
                with open('config.yaml', 'w') as f:
                    yaml.safe_dump({'fish_distance_calculation': var}, f)
                rates, parts = [], []
                for rep in range(4):                           # one warm-up pass, three timed
                    stats = {}
                    stdout, sys.stdout = sys.stdout, devnull
                    try:
                        t0 = time.perf_counter()
                        fdc.main([], handle=h, stats=stats)
                        dt = time.perf_counter() - t0
                    finally:
                        sys.stdout = stdout
                    if rep:
                        rates.append(a.images / dt)
                        parts.append({key: round(stats.get(key, 0.0), 4) for key in ('read_s', 'device_s', 'rows_s')})
                csvs.append(open(os.path.join(inp, 'centromere_distances.csv')).read())
                out['legs'].append({'batch': k, 'images_per_s': _stats(rates), 'passes': parts})
            out['csv_rows'] = csvs[0].count('\n') - 1
            out['same_csv'] = all(c == csvs[0] for c in csvs)
        finally:
            os.chdir(cwd)
    h.close()
    one = [leg['images_per_s'] for leg in out['legs'] if leg['batch'] == 1]
    many = [leg['images_per_s'] for leg in out['legs'] if leg['batch'] != 1]
    out['gain'] = bool(many) and min(m['min'] for m in many) > max(o['max'] for o in one)
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('mode', nargs='?', choices=['alternate'], help='alternate: main() with batch 1, k, 1, k (needs --batch k)')
    ap.add_argument('--batch', type=int, default=0)
    ap.add_argument('--io-threads', type=int, default=0)
    ap.add_argument('--images', type=int, default=16)
    ap.add_argument('--nuclei', type=int, default=300)
    ap.add_argument('--height', type=int, default=1040)
    ap.add_argument('--width', type=int, default=1392)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--cpu-workers', type=int, default=16)
    ap.add_argument('--no-cpu', action='store_true')
    a = ap.parse_args()
    if a.mode == 'alternate':
        if a.batch < 2:
            ap.error('alternate needs --batch k with k above 1')
        return alternate(a)
    import yaml

    from ecseg_amd import fish_distance_calculation as fdc
    from ecseg_amd._lib import Handle
    jobs = [(2000 + k, a.height, a.width, a.nuclei) for k in range(a.images)]
    data = [synth_scene(*j) for j in jobs]
    maps = [np.ascontiguousarray(seg, np.int32) for _, seg in data]
    h = Handle(0)
    n_cells = n_values = 0
    for (lsq, _), lab in zip(data, maps):                      # warm-up pass: buffers, code objects
        rec = h.fish_distances(lab, lsq, 0, 1)
        n_cells += len(rec)
        n_values += len(fdc.distances_from_records(rec, 3))
    dev, wall = [], []
    for _ in range(a.reps):
        d = w = 0.0
        for (lsq, _), lab in zip(data, maps):
            t0 = time.perf_counter()
            h.fish_distances(lab, lsq, 0, 1)
            w += time.perf_counter() - t0
            d += h.timings()['count']
        dev.append(d / a.images)
        wall.append(1e3 * w / a.images)
    out = {'images': a.images, 'shape': [a.height, a.width], 'cells': n_cells, 'values': n_values, 'reps': a.reps,
           'device_ms_per_image': _stats(dev), 'call_ms_per_image': _stats(wall)}
    with tempfile.TemporaryDirectory() as tmp:
        inp = os.path.join(tmp, 'in')
        write_folder(inp, data)
        reads = []
        for rep in range(a.reps + 1):
            t0 = time.perf_counter()
            for k in range(a.images):
                fdc.load_image(inp, os.path.join(inp, 'img_%03d.tif' % k))
            if rep:
                reads.append(1e3 * (time.perf_counter() - t0) / a.images)
        out['read_ms_per_image'] = _stats(reads)
        out['read_over_device'] = round(out['read_ms_per_image']['min'] / out['device_ms_per_image']['max'], 1)
        with open(os.path.join(tmp, 'config.yaml'), 'w') as f:
            yaml.safe_dump({'fish_distance_calculation': {'inpath': inp, 'centromere_probe_color': 'green', 'fish_probe_color': 'red',
                                                          'max_centromeric_spots': 3}}, f)
        cwd = os.getcwd()
        os.chdir(tmp)
        try:
            rates = []
            devnull = open(os.devnull, 'w')
            for rep in range(a.reps + 1):
                stdout, sys.stdout = sys.stdout, devnull
                try:
                    t0 = time.perf_counter()
                    fdc.main([], handle=h)
                    dt = time.perf_counter() - t0
                finally:
                    sys.stdout = stdout
                if rep:
                    rates.append(a.images / dt)
            out['main_images_per_s'] = _stats(rates)
            out['csv_rows'] = open(os.path.join(inp, 'centromere_distances.csv')).read().count('\n') - 1
        finally:
            os.chdir(cwd)
    h.close()
    if not a.no_cpu:
        for key, fn in (('cpu_loop', _cpu_loop), ('cpu_records', _cpu_records)):
            with ProcessPoolExecutor(a.cpu_workers) as ex:
                res = list(ex.map(fn, jobs))
            secs = [s for _, s in res]                         # per image on one core, with the other workers busy
            out[key] = {'workers': a.cpu_workers, 'ms_per_image_one_core': _stats([1e3 * s for s in secs]),
                        'images_per_s_all_workers': round(a.cpu_workers / statistics.mean(secs), 2), 'n': sum(n for n, _ in res)}
    print(json.dumps(out))


if __name__ == '__main__':
    main()
