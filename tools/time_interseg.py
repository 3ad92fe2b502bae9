"""Throughput of the interSeg file-level driver (``make interseg``) on synthetic FISH images.

    python tools/time_interseg.py [--images 16] [--nuclei 40] [--height 1040] [--width 1392] [--cpu-workers 16]
    python tools/time_interseg.py --classify-on-device off|on|alternate     # the classifier stage with interseg.classify_on_device
                                                                            # off / on (alternate: off, on, off, on in one process)
    python tools/time_interseg.py --classify-on-device on --batch 8 alternate   # `make interseg` end to end over a folder of files, file
                                                                            # reads included, interseg.batch 1, 8, 1, 8: a child process per visit

Without --batch nothing is read from a file: the images are arrays in memory, so the read stage is in none of those figures.

Device side: per image ``Handle.nuclei_regions`` + ``Handle.nucleus_crops`` (regions + crops), the two classifiers
(tests/golden/interseg_synth.h5 and ecseg_c_synth.h5, batched) and the host work around them (region rows, decisions).
For comparison it restates the reference's per-nucleus loop (src/interseg.py:121-152) in numpy - a full-image mask and a
full-image multiply per nucleus, then the crop and a bilinear resize - over the same images on a pool of CPU processes;
the classifiers are not part of that restatement.  Prints one JSON line.
"""
import argparse
import json
import os
import sys
import time
from concurrent.futures import ProcessPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def synth_image(seed, H, W, n_nuclei):
    rng = np.random.default_rng(seed)
    yy, xx = np.ogrid[:H, :W]
    seg = np.zeros((H, W), np.uint8)
    for k in range(n_nuclei):
        ry, rx = (int(rng.integers(140, 200)),) * 2 if k == 0 else (int(rng.integers(15, 60)), int(rng.integers(15, 60)))
        cy, cx = int(rng.integers(ry, H - ry)), int(rng.integers(rx, W - rx))
        seg[((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2 <= 1.0] = 255
    img = rng.integers(0, 60, (H, W, 3), dtype=np.uint8)
    img[seg != 0] += rng.integers(0, 120, (int((seg != 0).sum()), 3), dtype=np.uint8)
    return seg, img


def _resize_bilinear(win):
    """skimage's order-1 'reflect' resize to 256 x 256 restated in numpy float64 (exact affine parameters)."""
    h, w = win.shape[:2]
    i = np.arange(256)

    def taps(n):
        r = (i + 0.5) * n / 256.0 - 0.5
        a = np.floor(r).astype(int)
        f = r - a
        refl = (lambda c: np.zeros_like(c)) if n == 1 else (lambda c: np.where(c < 0, -c, np.where(c >= n, 2 * (n - 1) - c, c)))
        return refl(a), refl(a + 1), f
    r0, r1, fr = taps(h)
    c0, c1, fc = taps(w)
    a = win.astype(np.float64)
    top = a[r0][:, c0] * (1 - fc)[None, :, None] + a[r0][:, c1] * fc[None, :, None]
    bot = a[r1][:, c0] * (1 - fc)[None, :, None] + a[r1][:, c1] * fc[None, :, None]
    return (top * (1 - fr)[:, None, None] + bot * fr[:, None, None]).astype(np.uint8)


def cpu_reference_loop(args):
    """src/interseg.py:121-152,190-194 per image, numpy: the reference's O(nuclei x H x W) mask-and-multiply per nucleus."""
    from scipy import ndimage as ndi

    from ecseg_amd.interseg import crop_windows
    seg, img = synth_image(*args)
    lab, n = ndi.label(seg != 0, structure=np.ones((3, 3), int))
    crops = 0
    for r in range(1, n + 1):
        mask = lab == r
        temp = img * mask[..., None]
        if temp[..., 0].sum() / mask.sum() < 12.75:
            continue
        ys, xs = np.nonzero(mask)
        y0, x0, y1, x1 = ys.min(), xs.min(), ys.max() + 1, xs.max() + 1
        for dy, dx, th, tw in crop_windows(y1 - y0, x1 - x0):
            _resize_bilinear(temp[y0 + dy:y0 + dy + th, x0 + dx:x0 + dx + tw])
            crops += 1
    return crops


def classify_pass(data, h, mi, mc, on, split=False):
    """One pass over the images as process_image runs them (regions, crops, classifiers, rows) with the key off or on.  Returns
    (seconds of the pass, per-stage seconds, device milliseconds: crop kernels, input kernel, each plan).  ``split`` (key off): the
    classifier stage again, piece by piece - crop slicing, ecSeg-i predict, preprocess_ecseg_c, ecSeg-c predict, rows."""
    from ecseg_amd import interseg
    st = {'regions': 0.0, 'crops': 0.0, 'classifiers': 0.0, 'rows': 0.0}
    dev = {'crop_kernels': 0.0, 'input_kernel': 0.0, 'plan_i': 0.0, 'plan_c': 0.0}
    parts = {'slice_u8': 0.0, 'predict_i': 0.0, 'preprocess_numpy': 0.0, 'predict_c': 0.0}
    t_all = time.perf_counter()
    for seg, img in data:
        t0 = time.perf_counter()
        rec = h.nuclei_regions(seg, img, 0)
        centers, low, desc, tiled, owner = interseg.region_rows(rec)
        t1 = time.perf_counter()
        if on:
            _, pi, ri, pc, rc = h.classify_nucleus_crops(desc, (0, 1, 2), tiled, True, mi, mc)
            t2 = t3 = time.perf_counter()
            rows = interseg.rows_from_predictions(True, True, ri, pi, rc, pc)
            t4 = time.perf_counter()
            tm = h.timings()
            dev['crop_kernels'] += tm['count']
            dev['input_kernel'] += tm['tile']
            dev['plan_i'] += mi.handle.timings()['unet']
            dev['plan_c'] += mc.handle.timings()['unet']
            st['classifiers'] += t2 - t1
            st['rows'] += t4 - t3
        else:
            crops, cmax = h.nucleus_crops(desc, (0, 1, 2))
            t2 = time.perf_counter()
            dev['crop_kernels'] += h.timings()['count']
            rows = []
            for b0 in range(0, len(desc), interseg.CROP_BATCH):
                sl = slice(b0, b0 + interseg.CROP_BATCH)
                rows += interseg.classify_crops(mi, crops[sl], mc, True, from_patches=tiled[sl], channel_max=cmax[sl])
            t3 = time.perf_counter()
            st['crops'] += t2 - t1
            st['classifiers'] += t3 - t2
            if split:
                for b0 in range(0, len(desc), interseg.CROP_BATCH):
                    c, m, tl = crops[b0:b0 + interseg.CROP_BATCH], cmax[b0:b0 + interseg.CROP_BATCH], tiled[b0:b0 + interseg.CROP_BATCH]
                    live = np.flatnonzero(~(tl & (m.max(axis=1) == 0)))
                    q0 = time.perf_counter()
                    x = c[live][..., 0]
                    q1 = time.perf_counter()
                    mi.predict(x)
                    q2 = time.perf_counter()
                    xc = [interseg.preprocess_ecseg_c(c[k]) for k in live if m[k, 1] > 10]
                    xc = np.stack(xc) if xc else np.zeros((0, 256, 256, 3), np.float32)
                    q3 = time.perf_counter()
                    mc.predict(xc)
                    q4 = time.perf_counter()
                    for key, v in zip(parts, (q1 - q0, q2 - q1, q3 - q2, q4 - q3)):
                        parts[key] += v
        st['regions'] += t1 - t0
    return time.perf_counter() - t_all, st, dev, parts


def classify_report(a):
    """--classify-on-device: images/s as median (min - max) of 3 passes after a warm-up pass, per mode visit; per-stage seconds and device
    milliseconds per image; for the key off, the split of the classifier stage into plan calls (upload + network + download), crop slicing
    and numpy."""
    from ecseg_amd import hdf5_min
    from ecseg_amd.model import MetasegModel
    g = os.path.join(ROOT, 'tests', 'golden')
    mi = MetasegModel(*hdf5_min.load_keras_h5(os.path.join(g, 'interseg_synth.h5')))
    mc = MetasegModel(*hdf5_min.load_keras_h5(os.path.join(g, 'ecseg_c_synth.h5')))
    h = mi.handle
    data = [synth_image(1000 + k, a.height, a.width, a.nuclei) for k in range(a.images)]
    visits = {'off': [False], 'on': [True], 'alternate': [False, True, False, True]}[a.classify_on_device]
    n = len(data)
    out = {'images': n, 'shape': [a.height, a.width], 'visits': []}
    for on in visits:
        classify_pass(data, h, mi, mc, on)                                   # warm-up: buffers of this mode
        rates, last = [], None
        for _ in range(3):
            wall, st, dev, _ = last = classify_pass(data, h, mi, mc, on)
            rates.append(n / wall)
        rec = {'classify_on_device': on, 'images_per_s': {'median': round(float(np.median(rates)), 3), 'min': round(min(rates), 3), 'max': round(max(rates), 3)},
               'stage_ms_per_image': {k: round(1e3 * v / n, 3) for k, v in last[1].items()},
               'device_ms_per_image': {k: round(v / n, 4) for k, v in last[2].items()}}
        if not on:
            _, _, _, parts = classify_pass(data, h, mi, mc, False, split=True)
            # predict_* = upload + plan + download as the host path pays them; the plans' own device time is plan_i / plan_c of an `on` visit
            rec['classifier_stage_split_ms_per_image'] = {k: round(1e3 * v / n, 3) for k, v in parts.items()}
        out['visits'].append(rec)
    print(json.dumps(out))


def batch_visit(a):
    """One mode visit of --batch, in a process of its own: ``interseg.main``'s loop (files read from the folder, device calls, rows)
    over the folder with ``classify_on_device`` on and ``batch`` = a.batch_visit; a warm-up pass, then 3 timed passes.  One JSON line."""
    from concurrent.futures import ThreadPoolExecutor

    from ecseg_amd import hdf5_min, interseg, utils
    from ecseg_amd.model import MetasegModel
    g = os.path.join(ROOT, 'tests', 'golden')
    mi = MetasegModel(*hdf5_min.load_keras_h5(os.path.join(g, 'interseg_synth.h5')))
    mc = MetasegModel(*hdf5_min.load_keras_h5(os.path.join(g, 'ecseg_c_synth.h5')))
    h, k = mi.handle, a.batch_visit
    paths = utils.get_imgs(a.folder)

    def one_pass(pool):
        st, rows = {}, 0
        t0 = time.perf_counter()
        if k == 1:
            for p in paths:
                rows += len(interseg.process_image(p, h, mi, mc, 0, True, stats=st, classify_on_device=True))
            st['device'] = st.pop('device_crops') + st.pop('classifiers')
        else:
            for c0 in range(0, len(paths), k):
                for r in interseg.process_chunk(paths[c0:c0 + k], [True] * len(paths[c0:c0 + k]), h, mi, mc, 0, pool, stats=st):
                    rows += len(r)
        return time.perf_counter() - t0, st, rows
    with ThreadPoolExecutor(utils.default_io_threads()) as pool:
        one_pass(pool)
        runs = [one_pass(pool) for _ in range(3)]
    rates = [len(paths) / r[0] for r in runs]
    print(json.dumps({'batch': k, 'images': len(paths), 'rows': runs[-1][2], 'io_threads': utils.default_io_threads(),
                      'images_per_s': {'median': round(float(np.median(rates)), 3), 'min': round(min(rates), 3), 'max': round(max(rates), 3)},
                      'stage_s_per_pass': {key: round(float(np.median([r[1][key] for r in runs])), 4) for key in ('read', 'device', 'rows')}}))


def batch_report(a):
    """--batch K [alternate]: the synthetic images written once as the files ``make interseg`` reads (RGB TIFFs and their
    annotated/<name>/<name>_segmentation.tif), then ``batch`` 1, K, 1, K (alternate) or K alone, every visit a child process under its
    own time limit.  Prints one JSON line with the visits in order."""
    import subprocess
    import tempfile

    from ecseg_amd import image_io
    with tempfile.TemporaryDirectory() as folder:
        for j in range(a.images):
            seg, img = synth_image(1000 + j, a.height, a.width, a.nuclei)
            name = 'img%03d' % j
            os.makedirs(os.path.join(folder, 'annotated', name))
            image_io.write_tiff_rgb8(os.path.join(folder, name + '.tif'), img)
            image_io.write_tiff_gray8(os.path.join(folder, 'annotated', name, name + '_segmentation.tif'), seg)
        visits = [1, a.batch, 1, a.batch] if a.mode == 'alternate' else [a.batch]
        out = {'images': a.images, 'shape': [a.height, a.width], 'visits': []}
        for k in visits:
            cmd = [sys.executable, os.path.abspath(__file__), '--batch-visit', str(k), '--folder', folder]
            try:
                res = subprocess.run(cmd, capture_output=True, text=True, timeout=a.visit_timeout)
            except subprocess.TimeoutExpired:
                out['visits'].append({'batch': k, 'error': 'no result within %d s' % a.visit_timeout})
                break                                                       # nothing more is started behind a visit that hung
            if res.returncode != 0:
                out['visits'].append({'batch': k, 'error': 'exit %d: %s' % (res.returncode, res.stderr[-500:])})
                break
            out['visits'].append(json.loads(res.stdout.strip().splitlines()[-1]))
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=None, help='time `make interseg` end to end (file reads included) with interseg.batch 1 and this value')
    ap.add_argument('mode', nargs='?', choices=['alternate'], default=None, help='with --batch: batch 1, K, 1, K instead of K alone')
    ap.add_argument('--visit-timeout', type=int, default=240, help='with --batch: seconds a mode visit may take')
    ap.add_argument('--batch-visit', type=int, default=None, help=argparse.SUPPRESS)
    ap.add_argument('--folder', default=None, help=argparse.SUPPRESS)
    ap.add_argument('--images', type=int, default=16)
    ap.add_argument('--nuclei', type=int, default=40)
    ap.add_argument('--height', type=int, default=1040)
    ap.add_argument('--width', type=int, default=1392)
    ap.add_argument('--cpu-workers', type=int, default=16)
    ap.add_argument('--no-cpu', action='store_true')
    ap.add_argument('--classify-on-device', choices=['off', 'on', 'alternate'], default=None,
                    help='time the classifier stage of `make interseg` with interseg.classify_on_device off, on, or off, on, off, on over the same images')
    a = ap.parse_args()
    if a.batch_visit:
        return batch_visit(a)
    if a.batch:
        return batch_report(a)
    if a.classify_on_device:
        return classify_report(a)
    from ecseg_amd import hdf5_min, interseg
    from ecseg_amd.model import MetasegModel
    g = os.path.join(ROOT, 'tests', 'golden')
    mi = MetasegModel(*hdf5_min.load_keras_h5(os.path.join(g, 'interseg_synth.h5')))
    mc = MetasegModel(*hdf5_min.load_keras_h5(os.path.join(g, 'ecseg_c_synth.h5')))
    h = mi.handle
    jobs = [(1000 + k, a.height, a.width, a.nuclei) for k in range(a.images)]
    data = [synth_image(*j) for j in jobs]
    # warm-up: buffers, plans
    seg, img = data[0]
    rec = h.nuclei_regions(seg, img, 0)
    _, _, desc, tiled, _ = interseg.region_rows(rec)
    crops, cmax = h.nucleus_crops(desc)
    interseg.classify_crops(mi, crops[:8], mc, True, from_patches=tiled[:8], channel_max=cmax[:8])
    t = {'regions_crops': 0.0, 'classifiers': 0.0, 'host': 0.0}
    n_crops = n_nuclei = 0
    t_all = time.perf_counter()
    for seg, img in data:
        t0 = time.perf_counter()
        rec = h.nuclei_regions(seg, img, 0)
        t1 = time.perf_counter()
        centers, low, desc, tiled, owner = interseg.region_rows(rec)
        t2 = time.perf_counter()
        crops, cmax = h.nucleus_crops(desc, (0, 1, 2))
        t3 = time.perf_counter()
        rows = []
        for b0 in range(0, len(desc), interseg.CROP_BATCH):
            sl = slice(b0, b0 + interseg.CROP_BATCH)
            rows += interseg.classify_crops(mi, crops[sl], mc, True, from_patches=tiled[sl], channel_max=cmax[sl])
        t4 = time.perf_counter()
        t['regions_crops'] += (t1 - t0) + (t3 - t2)
        t['host'] += t2 - t1
        t['classifiers'] += t4 - t3
        n_crops += len(desc)
        n_nuclei += len(rec)
    wall = time.perf_counter() - t_all
    out = {'images': a.images, 'shape': [a.height, a.width], 'nuclei': n_nuclei, 'crops': n_crops,
           'images_per_s': a.images / wall, 'seconds': {k: round(v, 4) for k, v in t.items()},
           'ms_per_image': {k: round(1e3 * v / a.images, 3) for k, v in t.items()}}
    if not a.no_cpu:
        t0 = time.perf_counter()
        with ProcessPoolExecutor(a.cpu_workers) as ex:
            cpu_crops = sum(ex.map(cpu_reference_loop, jobs))
        cw = time.perf_counter() - t0
        out['cpu_restatement'] = {'workers': a.cpu_workers, 'images_per_s': a.images / cw, 'crops': cpu_crops,
                                  'ms_per_nucleus_single_core': round(1e3 * cw * a.cpu_workers / max(n_nuclei, 1), 3)}
    print(json.dumps(out))


if __name__ == '__main__':
    main()
