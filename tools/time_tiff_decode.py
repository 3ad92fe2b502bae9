"""Timing of the device TIFF reader (ecseg_tiff_decode) against the host reader (ecseg_tiff_read) on one core.

    python tools/time_tiff_decode.py [--passes 5] [--limit 120]

A 1040 x 1392 RGB scene of the stat_fish generator (tests/stat_fish_cases.py ``full_size_scene``) is written with LZW and the
horizontal predictor at 1, 5, 15, 64 and 1040 rows per strip, and once uncompressed.  Per file: the host reader from the page
cache, the whole device call (parse, upload, kernels, download) and the kernels alone from the handle's timers - median, minimum
and maximum of --passes passes after a warm-up pass.  Every file's device run is a child process of its own under --limit
seconds, so that a file that keeps a wave too long ends that run and no other.  Handle.tiff_decode decodes every
file it is given; the routing rule that image_io.imread asks (csrc/tiff_parse.h, TIFF_DEVICE_MIN_STRIPS) takes its threshold from
this table.  Prints one JSON line per file and a last line
with the smallest strip count at which the device call is faster than the host reader.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
ROWS = (1, 5, 15, 64, 1040)


def write_files(folder):
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
        strips = [encode(pred[r:r + rps]) for r in range(0, H, rps)]
        names['lzw_rps%d' % rps] = dc.tiff_file(strips, H, W, rps, spp=3, predictor=2)
    names['raw'] = dc.tiff_file([flat.tobytes()], H, W, H, spp=3, compression=1)
    for name, data in names.items():
        with open(os.path.join(folder, name + '.tif'), 'wb') as f:
            f.write(data)
    np.save(os.path.join(folder, 'pixels.npy'), img)
    return list(names)


def stats(ms):
    return dict(median=statistics.median(ms), min=min(ms), max=max(ms))


def one(path, passes):
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
        a = gpu.tiff_decode(data)
        if a is None:
            out['device'] = 'a layout the device reader leaves to the host'
            break
        if rep:
            call.append((time.perf_counter() - t0) * 1e3)
            kern.append(gpu.timings()['count'])
    else:
        assert np.array_equal(a, want)
        out.update(device_call_ms=stats(call), device_kernel_ms=stats(kern))
    gpu.close()
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--passes', type=int, default=5)
    ap.add_argument('--limit', type=float, default=120.0)
    ap.add_argument('--one')
    a = ap.parse_args()
    if a.one:
        return one(a.one, a.passes)
    rows = []
    with tempfile.TemporaryDirectory() as tmp:
        for name in write_files(tmp):
            try:
                r = subprocess.run([sys.executable, os.path.abspath(__file__), '--one', os.path.join(tmp, name + '.tif'), '--passes', str(a.passes)],
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
    faster = [(-(-1040 // int(r['file'][7:-4])), r) for r in rows if r['file'].startswith('lzw_') and 'device_call_ms' in r and
              r['device_call_ms']['median'] < r['host_read_ms']['median']]
    print(json.dumps(dict(smallest_strip_count_with_the_device_call_faster=min((n for n, _ in faster), default=None))))


if __name__ == '__main__':
    main()
