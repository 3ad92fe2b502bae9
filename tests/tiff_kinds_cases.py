"""The files whose handle-free answers (routes, counts, set routes, arena bytes) are recorded in tests/golden/tiff_kinds_answers.json:
every file of the tiles, inflate and PackBits case sets, files of strips on both sides of each routing threshold, and the files of
tests/golden/io_tiff_files.json.  One list for tools/record_tiff_kinds_answers.py, which wrote the recording, and for
tests/test_tiff_kinds.py, which holds the library to it."""
import base64
import json
import os
import zlib

import tiff_decode_cases as dc
import tiff_inflate_cases as ic
import tiff_packbits_cases as pc
import tiff_tiles_cases as tc

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
ANSWERS = os.path.join(GOLDEN, 'tiff_kinds_answers.json')
WORDS = tuple(range(8))                # every combination of deflate (1), tiled (2) and PackBits (4)


def file_of_strips(n, compression):
    """n one-row strips of 8 bytes: what the routing thresholds count"""
    strip = zlib.compress(bytes(8)) if compression in (8, 32946) else dc.pack(dc.lzw_codes(bytes(8))) if compression == 5 else bytes(8)
    return dc.tiff_file([strip] * n, n, 8, 1, compression=compression)


def all_files():
    """[(case name, file bytes)], the names unique"""
    out = [('tiles/' + name, data) for name, _, data in tc.all_cases()]
    out += [('tiles_refused/' + name, data) for name, data in tc.refused_cases().items()]
    out += [('tiles_damaged/' + name, data) for name, (_, data, _) in tc.damaged_cases().items()]
    for k, (name, stream, want, _, _) in enumerate(ic.hand_cases() + ic.zlib_streams()):   # a one-strip file around each stream, both Deflate codes
        out.append(('inflate/' + name, dc.tiff_file([stream], 1, want, 1, compression=32946 if k % 2 else 8)))
    out += [('inflate/' + name, dc.tiff_file([stream], 1, want, 1, compression=8)) for name, stream, want in ic.mutations()]
    out += [('packbits/' + name, data) for name, _, data, _ in pc.plan_cases()]
    out += [('packbits/' + name, data) for name, _, data in pc.hand_cases()]
    for comp in (1, 5, 8, 32946, pc.PACKBITS):
        out += [('strips/c%d_n%d' % (comp, n), file_of_strips(n, comp)) for n in (1, 139, 140, 208, 519, 520, 1039, 1040, 3000)]
    with open(os.path.join(GOLDEN, 'io_tiff_files.json')) as f:
        out += [('io/' + name, base64.b64decode(b64)) for name, b64 in json.load(f)['files'].items()]
    assert len({name for name, _ in out}) == len(out)
    return out
