#!/usr/bin/env python3
"""tests/golden/dapi_example.tif: the pixels of the reference's example image (tests/golden/dapi_example.npz) written by
libtiff (through Pillow, which needs `strip_size`: Pillow >= 10) in the layout OpenCV's imwrite gave example_ecSeg/dapi.jpeg:
8-bit gray, LZW, horizontal predictor, 5 rows per strip (208 strips at 1040 rows).  The I/O test decodes it with the native
reader and compares against the stored pixels, so the test needs nothing outside the repository.

    python tools/make_example_tiff.py
"""
import os

import numpy as np
from PIL import Image

GOLDEN = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'tests', 'golden')


def main():
    px = np.load(os.path.join(GOLDEN, 'dapi_example.npz'))['dapi']
    path = os.path.join(GOLDEN, 'dapi_example.tif')
    Image.fromarray(px).save(path, compression='tiff_lzw', tiffinfo={317: 2}, strip_size=5 * px.shape[1])
    im = Image.open(path)
    tags = im.tag_v2
    assert tags[259] == 5 and tags[317] == 2 and tags[278] == 5 and tags[258] == (8,), dict(tags)
    assert np.array_equal(np.array(im), px)
    print('%s: %d bytes, %d strips' % (path, os.path.getsize(path), len(tags[273])))


if __name__ == '__main__':
    main()
