"""Timing of the device TIFF reader (ecseg_tiff_decode) against the host reader (ecseg_tiff_read) on one core.

    python tools/time_tiff_decode.py [--passes 5] [--limit 120]
    python tools/time_tiff_decode.py --batch [--passes 5] [--limit 300] [--ks 1,2,4,8,16,32]
    python tools/time_tiff_decode.py --deflate [--batch] ...
    python tools/time_tiff_decode.py --tiled [--batch] [--deflate] ...
    python tools/time_tiff_decode.py --packbits [--batch] ...

A 1040 x 1392 RGB scene of the stat_fish generator (tests/stat_fish_cases.py ``full_size_scene``) is written with LZW and the
horizontal predictor at 1, 5, 15, 64 and 1040 rows per strip, and once uncompressed.  Per file: the host reader from the page
cache, the whole device call (parse, upload, kernels, download) and the kernels alone from the handle's timers - median, minimum
and maximum of --passes passes after a warm-up pass.  Every file's device run is a child process of its own under --limit
seconds, so that a file that keeps a wave too long ends that run and no other.  Handle.tiff_decode decodes every
file it is given; the routing rule that image_io.imread asks (csrc/tiff_parse.h, TIFF_DEVICE_MIN_STRIPS) takes its threshold from
this table.  Prints one JSON line per file and a last line
with the smallest strip count at which the device call is faster than the host reader.

--batch: the batched reader (ecseg_tiff_decode_batch through image_io.imread_many) on k = 1, 2, 4, 8, 16, 32 such scenes of
different seeds at 1, 5 and 15 rows per strip, and on the stat_fish pair (the RGB file at 1 row per strip with its 208-strip mask,
k images of them).  Every (plan, k) cell is a child process of its own under --limit seconds: it writes its files, reads them one
after another with ecseg_tiff_read on one host thread (the yardstick), then through imread_many as it is - reading the files, both
questions of the routing rule, one Handle.tiff_decode_many - with only the rule's verdict replaced, so that every set is sent (the
verdict is reported beside the times) - one warm-up and --passes passes each, median, minimum
and maximum.  A cell counts as a win only when the batch's maximum is below the host's minimum; the last line lists the cells that
win, and nothing is claimed between cells.

--deflate: the same two tables for Deflate strips (compression 8, zlib level 6, horizontal predictor; the device decodes them with
the handle option tiff_deflate_on_device, ``Handle.tiff_decode(data, deflate=True)`` / ``imread_many(..., deflate=True)``): single
files at 1, 5 and 15 rows per strip - 15 rows are 62640 decoded bytes, the strip plan of about 64 KiB that tifffile writes - and
batches of them and of the stat_fish pair (the mask a Deflate file of 208 strips).  The host side is ecseg_tiff_read, which inflates
with zlib on one thread.  A single file wins, too, only where the device call's maximum is below the host's minimum; the Deflate
thresholds of csrc/tiff_parse.h are the smallest strip counts that win (none: the rules never send a Deflate file on their own).

--tiled: the table for tiled files (handle option tiff_tiled_on_device; tiffb_untile_kernel): the same scene written by the tests' tile
writer (tests/tiff_tiles_cases.py) with square tiles of 16, 64, 256 and 512 pixels, LZW with the horizontal predictor, and with --deflate
zlib level 6 instead.  The yardstick is what reads such a file today, ``image_io.imread(path)`` without a handle (the pure-Python
reader, tile after tile); the device side is ``Handle.tiff_decode`` with the option on - with --batch ``imread_many`` over k = --ks such
scenes with only the rule's verdict replaced.  Every cell is a child process of its own under --limit seconds; median (min - max); a
cell wins only where the device's maximum is below the host's minimum, and the thresholds of csrc/tiff_parse.h
(TIFF_TILED_DEVICE_MIN_TILES, TIFF_TILED_BATCH_DEVICE_MIN_TILES) are the smallest measured tile counts that win - a tile size that was
not measured is never counted.

--packbits: the table for PackBits strips (compression 32773; handle option tiff_packbits_on_device; tiffb_packbits_kernel): the same
scene written by the tests' PackBits writer (tests/tiff_packbits_cases.py) at 1, 5 and 15 rows per strip with the horizontal
predictor, the same shape of table as --deflate: ``image_io.imread(path)`` without a handle (the Python reader, the only host reader of
PackBits) against ``Handle.tiff_decode`` with the option on - with --batch ``imread_many`` over k = --ks such scenes with only the
rule's verdict replaced.  No rule of csrc/tiff_parse.h counts a PackBits file until this table is measured.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
ROWS = (1, 5, 15, 64, 1040)


def write_files(folder, deflate=False):
    import stat_fish_cases as cases
    import ctypes as C
    import tiff_decode_cases as dc
    from ecseg_amd._lib import load_library
    img, _ = cases.full_size_scene(100)
    H, W = img.shape[:2]
    flat = np.ascontiguousarray(img).reshape(H, W * 3)
    pred = flat.copy()
    pred[:, 3:] = flat[:, 3:] - flat[:, :-3]
    names = {}
    lib = load_library()

    def encode(rows):                                        # the host encoder: the stream of dc.pack(dc.lzw_codes(...)), faster
        src = np.ascontiguousarray(rows).reshape(-1)
        dst = np.empty(2 * src.size + 64, np.uint8)
        m = lib.ecseg_lzw_encode(src.ctypes.data_as(C.c_void_p), src.size, dst.ctypes.data_as(C.c_void_p), dst.size)
        assert m > 0
        return dst[:m].tobytes()
    for rps in ROWS:
        if deflate:
            if rps <= 15:
                strips = [zlib.compress(pred[r:r + rps].tobytes(), 6) for r in range(0, H, rps)]
                names['zip_rps%d' % rps] = dc.tiff_file(strips, H, W, rps, spp=3, predictor=2, compression=8)
            continue
        strips = [encode(pred[r:r + rps]) for r in range(0, H, rps)]
        names['lzw_rps%d' % rps] = dc.tiff_file(strips, H, W, rps, spp=3, predictor=2)
    if deflate:
        for name, data in names.items():
            with open(os.path.join(folder, name + '.tif'), 'wb') as f:
                f.write(data)
        np.save(os.path.join(folder, 'pixels.npy'), img)
        return list(names)
    names['raw'] = dc.tiff_file([flat.tobytes()], H, W, H, spp=3, compression=1)
    for name, data in names.items():
        with open(os.path.join(folder, name + '.tif'), 'wb') as f:
            f.write(data)
    np.save(os.path.join(folder, 'pixels.npy'), img)
    return list(names)


def stats(ms):
    return dict(median=statistics.median(ms), min=min(ms), max=max(ms))


def one(path, passes, deflate=False):
    """The child: one file on the host reader and on the device -> one JSON line."""
    from ecseg_amd import image_io
    from ecseg_amd._lib import Handle
    want = np.load(os.path.join(os.path.dirname(path), 'pixels.npy'))
    data = open(path, 'rb').read()
    host = []
    for rep in range(passes + 1):
        t0 = time.perf_counter()
        a = image_io._native_tiff(path)
        if rep:
            host.append((time.perf_counter() - t0) * 1e3)
    assert np.array_equal(a, want)
    out = dict(file=os.path.basename(path), bytes=len(data), host_read_ms=stats(host))
    gpu = Handle(0)
    call, kern = [], []
    for rep in range(passes + 1):
        t0 = time.perf_counter()
        a = gpu.tiff_decode(data, deflate=True) if deflate else gpu.tiff_decode(data)
        if a is None:
            out['device'] = 'a layout the device reader leaves to the host'
            break
        if rep:
            call.append((time.perf_counter() - t0) * 1e3)
            kern.append(gpu.timings()['count'])
    else:
        assert np.array_equal(a, want)
        out.update(device_call_ms=stats(call), device_kernel_ms=stats(kern))
        out['wins'] = out['device_call_ms']['max'] < out['host_read_ms']['min']
    gpu.close()
    print(json.dumps(out), flush=True)


BATCH_PLANS = ('rps1', 'rps5', 'rps15', 'pair')


def write_batch(folder, plan, k, deflate=False):
    """k scenes of seeds 100 .. 100 + k - 1 at the plan's rows per strip ('pair': 1, each with its mask as write_tiff_gray8 writes
    it) -> the paths."""
    import ctypes as C
    import stat_fish_cases as cases
    import tiff_decode_cases as dc
    from ecseg_amd import image_io
    from ecseg_amd._lib import load_library
    lib = load_library()
    rps = 1 if plan == 'pair' else int(plan[3:])
    paths = []
    for j in range(k):
        img, seg = cases.full_size_scene(100 + j)
        H, W = img.shape[:2]
        flat = np.ascontiguousarray(img).reshape(H, W * 3)
        pred = flat.copy()
        pred[:, 3:] = flat[:, 3:] - flat[:, :-3]
        strips = []
        for r in range(0, H, rps):
            if deflate:
                strips.append(zlib.compress(pred[r:r + rps].tobytes(), 6))
                continue
            src = np.ascontiguousarray(pred[r:r + rps]).reshape(-1)
            dst = np.empty(2 * src.size + 64, np.uint8)
            m = lib.ecseg_lzw_encode(src.ctypes.data_as(C.c_void_p), src.size, dst.ctypes.data_as(C.c_void_p), dst.size)
            assert m > 0
            strips.append(dst[:m].tobytes())
        paths.append(os.path.join(folder, 'scene_%02d.tif' % j))
        with open(paths[-1], 'wb') as f:
            f.write(dc.tiff_file(strips, H, W, rps, spp=3, predictor=2, compression=8 if deflate else 5))
        if plan == 'pair':
            paths.append(os.path.join(folder, 'mask_%02d.tif' % j))
            if deflate:                                      # the mask at write_tiff_gray8's 5 rows per strip: 208 Deflate strips
                m = (np.asarray(seg) > 0).astype(np.uint8) * np.uint8(255)
                with open(paths[-1], 'wb') as f:
                    f.write(dc.tiff_file([zlib.compress(m[r:r + 5].tobytes(), 6) for r in range(0, H, 5)], H, W, 5, compression=8))
                continue
            image_io.write_tiff_gray8(paths[-1], (np.asarray(seg) > 0).astype(np.uint8) * np.uint8(255))
    return paths


def batch_one(plan, k, passes, deflate=False):
    """The child: one (plan, k) cell on the host reader and through imread_many -> one JSON line."""
    from ecseg_amd import image_io
    from ecseg_amd._lib import Handle
    with tempfile.TemporaryDirectory() as tmp:
        paths = write_batch(tmp, plan, k, deflate)
        datas = [open(p, 'rb').read() for p in paths]
        goes, counts = image_io.tiff_batch_goes_to_device(datas, deflate=deflate)
        host = []
        for rep in range(passes + 1):
            t0 = time.perf_counter()
            want = [image_io._native_tiff(p) for p in paths]
            if rep:
                host.append((time.perf_counter() - t0) * 1e3)
        out = dict(plan=plan, k=k, files=len(paths), bytes=sum(len(d) for d in datas), rule_sends_the_set=bool(goes), host_read_ms=stats(host))
        rule = image_io.tiff_batch_goes_to_device                # the measurement sends every set: the rule's questions are asked and
        image_io.tiff_batch_goes_to_device = lambda datas: (True, rule(datas)[1])       # timed as ever, only the verdict is replaced
        if deflate:                                              # (Deflate files: every file counts too, where the rule counts none)
            image_io.tiff_batch_goes_to_device = lambda datas, deflate=False: (rule(datas, deflate=deflate) and True, [True] * len(datas))
        gpu = Handle(0)
        call = []
        for rep in range(passes + 1):
            t0 = time.perf_counter()
            got = image_io.imread_many(paths, handle=gpu, deflate=True) if deflate else image_io.imread_many(paths, handle=gpu)
            if rep:
                call.append((time.perf_counter() - t0) * 1e3)
        assert all(isinstance(g, np.ndarray) and g.dtype == w.dtype and np.array_equal(g, w) for g, w in zip(got, want))
        out.update(imread_many_ms=stats(call), device_kernel_ms_last_call=gpu.timings()['count'])
        out['wins'] = out['imread_many_ms']['max'] < out['host_read_ms']['min']
        gpu.close()
    print(json.dumps(out), flush=True)


TILE_SIZES = (16, 64, 256, 512)


def write_tiled(folder, tile, seed, deflate):
    import stat_fish_cases as cases
    import tiff_tiles_cases as tc
    img, _ = cases.full_size_scene(seed)
    path = os.path.join(folder, 'tile%d_%s_%d.tif' % (tile, 'zip' if deflate else 'lzw', seed))
    with open(path, 'wb') as f:
        f.write(tc.tiled_tiff(np.ascontiguousarray(img), tile, tile, 8 if deflate else 5, 2))
    return path, -(-img.shape[0] // tile) * -(-img.shape[1] // tile)


def tiled_one(tile, k, passes, deflate, batch):
    """The child: k scenes at one tile size, read by image_io.imread without a handle and on the device -> one JSON line."""
    from ecseg_amd import image_io
    from ecseg_amd._lib import Handle
    with tempfile.TemporaryDirectory() as tmp:
        written = [write_tiled(tmp, tile, 100 + j, deflate) for j in range(k)]
        paths, tiles = [p for p, _ in written], sum(n for _, n in written)
        datas = [open(p, 'rb').read() for p in paths]
        host = []
        for rep in range(passes + 1):
            t0 = time.perf_counter()
            want = [image_io.imread(p) for p in paths]
            if rep:
                host.append((time.perf_counter() - t0) * 1e3)
        gpu = Handle(0)
        gpu.set_option('tiff_tiled_on_device', 1)
        gpu.set_option('tiff_deflate_on_device', int(deflate))
        if batch:
            goes, _ = image_io.tiff_batch_goes_to_device(datas, deflate=deflate, tiled=True)
            rule = image_io.tiff_batch_goes_to_device            # the rule's questions are asked and timed, only the verdict is replaced
            image_io.tiff_batch_goes_to_device = lambda datas, deflate=False, tiled=False: (rule(datas, deflate=deflate, tiled=tiled) and True, [True] * len(datas))
        else:
            goes = image_io.tiff_goes_to_device(datas[0], deflate=deflate, tiled=True)
        call, kern = [], []
        for rep in range(passes + 1):
            t0 = time.perf_counter()
            got = image_io.imread_many(paths, handle=gpu, deflate=deflate) if batch else [gpu.tiff_decode(datas[0])]
            if rep:
                call.append((time.perf_counter() - t0) * 1e3)
                kern.append(gpu.timings()['count'])
        assert all(isinstance(g, np.ndarray) and g.dtype == w.dtype and np.array_equal(g, w) for g, w in zip(got, want))
        out = dict(tile=tile, k=k, tiles=tiles, codec='zip' if deflate else 'lzw', bytes=sum(len(d) for d in datas), rule_sends_it=bool(goes),
                   host_imread_ms=stats(host), device_call_ms=stats(call), device_kernel_ms=stats(kern))
        out['wins'] = out['device_call_ms']['max'] < out['host_imread_ms']['min']
        gpu.close()
    print(json.dumps(out), flush=True)


def tiled_main(a):
    rows = []
    for tile in TILE_SIZES:
        for k in (a.ks if a.batch else [1]):
            cell = dict(tile=tile, k=k)
            try:
                r = subprocess.run([sys.executable, os.path.abspath(__file__), '--tiled-one', '%d:%d' % (tile, k), '--passes', str(a.passes)] +
                                   (['--deflate'] if a.deflate else []) + (['--batch'] if a.batch else []), capture_output=True, text=True, timeout=a.limit)
            except subprocess.TimeoutExpired:
                print(json.dumps(dict(cell, device='ended at the time limit of %g s' % a.limit)), flush=True)
                return                                       # a hung device run: nothing more is started on the device
            if r.returncode != 0:
                print(json.dumps(dict(cell, failed=r.returncode, stderr=r.stderr[-2000:])), flush=True)
                return
            line = r.stdout.strip().splitlines()[-1]
            print(line, flush=True)
            rows.append(json.loads(line))
    print(json.dumps(dict(cells_where_the_device_maximum_is_below_the_host_minimum=[[r['tile'], r['k'], r['tiles']] for r in rows if r['wins']])))


PACKBITS_ROWS = (1, 5, 15)                                   # rows per strip: the plans of the LZW tables


def packbits_one(rps, k, passes, batch):
    """The child: k scenes as PackBits strips at one plan (horizontal predictor), read by image_io.imread without a handle - the Python
    reader, the only host reader of PackBits - and on the device (handle option tiff_packbits_on_device) -> one JSON line."""
    import stat_fish_cases as cases
    import tiff_packbits_cases as pc
    from ecseg_amd import image_io
    from ecseg_amd._lib import Handle
    with tempfile.TemporaryDirectory() as tmp:
        paths = []
        for j in range(k):
            img, _ = cases.full_size_scene(100 + j)
            paths.append(os.path.join(tmp, 'packbits%d_%d.tif' % (rps, j)))
            with open(paths[-1], 'wb') as f:
                f.write(pc.strip_file(np.ascontiguousarray(img), rps, predictor=2))
        datas = [open(p, 'rb').read() for p in paths]
        strips = k * -(-img.shape[0] // rps)
        host = []
        for rep in range(passes + 1):
            t0 = time.perf_counter()
            want = [image_io.imread(p) for p in paths]
            if rep:
                host.append((time.perf_counter() - t0) * 1e3)
        gpu = Handle(0)
        gpu.set_option('tiff_packbits_on_device', 1)
        if batch:
            goes, _ = image_io.tiff_batch_goes_to_device(datas, packbits=True)
            rule = image_io.tiff_batch_goes_to_device            # the rule's questions are asked and timed, only the verdict is replaced
            image_io.tiff_batch_goes_to_device = lambda datas, **kw: (rule(datas, **kw) and True, [True] * len(datas))
        else:
            goes = image_io.tiff_goes_to_device(datas[0], packbits=True)
        call, kern = [], []
        for rep in range(passes + 1):
            t0 = time.perf_counter()
            got = image_io.imread_many(paths, handle=gpu) if batch else [gpu.tiff_decode(datas[0])]
            if rep:
                call.append((time.perf_counter() - t0) * 1e3)
                kern.append(gpu.timings()['count'])
        assert all(isinstance(g, np.ndarray) and g.dtype == w.dtype and np.array_equal(g, w) for g, w in zip(got, want))
        out = dict(rows_per_strip=rps, k=k, strips=strips, codec='packbits', bytes=sum(len(d) for d in datas), rule_sends_it=bool(goes),
                   host_imread_ms=stats(host), device_call_ms=stats(call), device_kernel_ms=stats(kern))
        out['wins'] = out['device_call_ms']['max'] < out['host_imread_ms']['min']
        gpu.close()
    print(json.dumps(out), flush=True)


def packbits_main(a):
    rows = []
    for rps in PACKBITS_ROWS:
        for k in (a.ks if a.batch else [1]):
            cell = dict(rows_per_strip=rps, k=k)
            try:
                r = subprocess.run([sys.executable, os.path.abspath(__file__), '--packbits-one', '%d:%d' % (rps, k), '--passes', str(a.passes)] +
                                   (['--batch'] if a.batch else []), capture_output=True, text=True, timeout=a.limit)
            except subprocess.TimeoutExpired:
                print(json.dumps(dict(cell, device='ended at the time limit of %g s' % a.limit)), flush=True)
                return                                       # a hung device run: nothing more is started on the device
            if r.returncode != 0:
                print(json.dumps(dict(cell, failed=r.returncode, stderr=r.stderr[-2000:])), flush=True)
                return
            line = r.stdout.strip().splitlines()[-1]
            print(line, flush=True)
            rows.append(json.loads(line))
    print(json.dumps(dict(cells_where_the_device_maximum_is_below_the_host_minimum=[[r['rows_per_strip'], r['k'], r['strips']] for r in rows if r['wins']])))


def batch_main(a):
    rows = []
    for plan in BATCH_PLANS:
        for k in a.ks:
            cell = dict(plan=plan, k=k)
            try:
                r = subprocess.run([sys.executable, os.path.abspath(__file__), '--batch-one', '%s:%d' % (plan, k), '--passes', str(a.passes)] +
                                   (['--deflate'] if a.deflate else []),
                                   capture_output=True, text=True, timeout=a.limit)
            except subprocess.TimeoutExpired:
                print(json.dumps(dict(cell, device='ended at the time limit of %g s' % a.limit)), flush=True)
                return                                       # a hung device run: nothing more is started on the device
            if r.returncode != 0:
                print(json.dumps(dict(cell, failed=r.returncode, stderr=r.stderr[-2000:])), flush=True)
                return
            line = r.stdout.strip().splitlines()[-1]
            print(line, flush=True)
            rows.append(json.loads(line))
    print(json.dumps(dict(cells_where_the_batch_maximum_is_below_the_host_minimum=[[r['plan'], r['k']] for r in rows if r['wins']])))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--passes', type=int, default=5)
    ap.add_argument('--limit', type=float, default=120.0)
    ap.add_argument('--one')
    ap.add_argument('--batch', action='store_true')
    ap.add_argument('--deflate', action='store_true')
    ap.add_argument('--batch-one')
    ap.add_argument('--tiled', action='store_true')
    ap.add_argument('--tiled-one')
    ap.add_argument('--packbits', action='store_true')
    ap.add_argument('--packbits-one')
    ap.add_argument('--ks', type=lambda v: [int(x) for x in v.split(',')], default=[1, 2, 4, 8, 16, 32])
    a = ap.parse_args()
    if a.tiled_one:
        tile, k = a.tiled_one.split(':')
        return tiled_one(int(tile), int(k), a.passes, a.deflate, a.batch)
    if a.tiled:
        return tiled_main(a)
    if a.packbits_one:
        rps, k = a.packbits_one.split(':')
        return packbits_one(int(rps), int(k), a.passes, a.batch)
    if a.packbits:
        return packbits_main(a)
    if a.one:
        return one(a.one, a.passes, a.deflate)
    if a.batch_one:
        plan, k = a.batch_one.split(':')
        return batch_one(plan, int(k), a.passes, a.deflate)
    if a.batch:
        return batch_main(a)
    rows = []
    with tempfile.TemporaryDirectory() as tmp:
        for name in write_files(tmp, a.deflate):
            try:
                r = subprocess.run([sys.executable, os.path.abspath(__file__), '--one', os.path.join(tmp, name + '.tif'), '--passes', str(a.passes)] +
                                   (['--deflate'] if a.deflate else []),
                                   capture_output=True, text=True, timeout=a.limit)
            except subprocess.TimeoutExpired:
                print(json.dumps(dict(file=name + '.tif', device='ended at the time limit of %g s' % a.limit)), flush=True)
                break                                        # a hung device run: nothing more is started on the device
            if r.returncode != 0:
                print(json.dumps(dict(file=name + '.tif', failed=r.returncode, stderr=r.stderr[-2000:])), flush=True)
                break
            line = r.stdout.strip().splitlines()[-1]
            print(line, flush=True)
            rows.append(json.loads(line))
    if a.deflate:
        print(json.dumps(dict(strip_counts_where_the_device_maximum_is_below_the_host_minimum=sorted(-(-1040 // int(r['file'][7:-4])) for r in rows if r.get('wins')))))
        return
    faster = [(-(-1040 // int(r['file'][7:-4])), r) for r in rows if r['file'].startswith('lzw_') and 'device_call_ms' in r and
              r['device_call_ms']['median'] < r['host_read_ms']['median']]
    print(json.dumps(dict(smallest_strip_count_with_the_device_call_faster=min((n for n, _ in faster), default=None))))


if __name__ == '__main__':
    main()
