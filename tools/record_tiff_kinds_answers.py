"""One-off recorder of tests/golden/tiff_kinds_answers.json: what the handle-free TIFF routing functions answered BEFORE the kinds
word replaced the `_ex`, `_ex2` and `_ex3` families (ECSEG_ABI_VERSION 5, commit 7dd6ba2).  To regenerate the recording, check that
commit out, build it (`make build`), and run this script from a later checkout against that library:

    python tools/record_tiff_kinds_answers.py --lib /path/to/parent/ecseg_amd/libecseg_hip.so

It needs no GPU (the four functions do no device work) and calls only the `_ex3` exports, with the word's bits as their three
switches: bit 0 deflate, bit 1 tiled, bit 2 PackBits.  Per file of tests/tiff_kinds_cases.py and per word 0..7 it records
[routes, counts, set routes of the file taken twice, arena bytes of the file alone].  A library of ABI 6 has no such exports and is
refused: the recording is the parent's, never that of the code the test holds to it."""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'tests')]
import tiff_kinds_cases as kc                # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--lib', required=True, help='libecseg_hip.so built from the parent commit (ABI 5)')
    ap.add_argument('--out', default=kc.ANSWERS)
    args = ap.parse_args()
    lib = C.CDLL(args.lib)
    if lib.ecseg_abi_version() != 5:
        sys.exit('this library has ABI %d: the recording is made with the parent commit\'s (5)' % lib.ecseg_abi_version())
    vp, ll, i32 = C.c_void_p, C.c_longlong, C.c_int
    lib.ecseg_tiff_decode_routes_ex3.argtypes = [vp, ll, i32, i32, i32]
    lib.ecseg_tiff_decode_batch_counts_ex3.argtypes = [vp, ll, i32, i32, i32]
    lib.ecseg_tiff_decode_batch_routes_ex3.argtypes = [vp, ll, vp, i32, i32, i32, i32]
    lib.ecseg_tiff_decode_batch_bytes_ex3.argtypes = [vp, ll, vp, i32, i32, i32, i32]
    lib.ecseg_tiff_decode_batch_bytes_ex3.restype = ll
    ptr = lambda a: a.ctypes.data_as(vp)
    answers = {}
    for name, data in kc.all_files():
        one = np.frombuffer(data, np.uint8)
        two = np.concatenate([one, one])
        r1, r2 = np.array([[0, one.size]], np.int64), np.array([[0, one.size], [one.size, one.size]], np.int64)
        rows = []
        for word in kc.WORDS:
            d, t, p = word & 1, word >> 1 & 1, word >> 2 & 1
            rows.append([int(lib.ecseg_tiff_decode_routes_ex3(ptr(one), one.size, d, t, p)),
                         int(lib.ecseg_tiff_decode_batch_counts_ex3(ptr(one), one.size, d, t, p)),
                         int(lib.ecseg_tiff_decode_batch_routes_ex3(ptr(two), two.size, ptr(r2), 2, d, t, p)),
                         int(lib.ecseg_tiff_decode_batch_bytes_ex3(ptr(one), one.size, ptr(r1), 1, d, t, p))])
        answers[name] = rows
    with open(args.out, 'w') as f:
        f.write('{\n' + ',\n'.join('%s: %s' % (json.dumps(k), json.dumps(v, separators=(',', ':'))) for k, v in sorted(answers.items())) + '\n}\n')
    print('%d files, %d bytes -> %s' % (len(answers), os.path.getsize(args.out), args.out))


if __name__ == '__main__':
    main()
