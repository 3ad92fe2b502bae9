#!/opt/conda/bin/python3.9
"""Golden vectors of NuSeT's ``_anchor_size``, taken from the reference's own function on the libraries it runs on.

Run (build container only, never on the GPU box):

    /opt/conda/bin/python3.9 tools/make_golden_nuset.py

It imports ``/root/reference/src/model_layers/anchor_size.py`` with a stub ``tensorflow`` module (the file imports it for the
``py_func`` wrapper only; ``_anchor_size`` itself is numpy + scikit-image 0.18.3: ``morphology.label`` with its default full
connectivity, ``regionprops`` bounding boxes, the median of max(height, width)), runs it on a dozen small masks and stores

  tests/golden/nuset_anchor_size.npz   mask_<k> (uint8), names (one per mask), sizes (float64; NaN: no region)

Only data is stored.
"""
import os
import sys
import types
import warnings

import numpy as np

warnings.filterwarnings('ignore')
sys.modules['tensorflow'] = types.ModuleType('tensorflow')
sys.path.insert(0, '/root/reference/src')
from model_layers.anchor_size import _anchor_size          # noqa: E402

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', 'tests', 'golden')


def masks():
    rng = np.random.default_rng(5)
    out = []

    def add(name, m):
        out.append((name, np.ascontiguousarray(m, np.uint8)))

    add('empty', np.zeros((16, 16)))
    m = np.zeros((16, 16)); m[5, 9] = 1
    add('one_pixel', m)
    m = np.zeros((16, 16)); m[2:5, 2:6] = 1; m[5:9, 6:8] = 1           # two rectangles touching at a corner: ONE 8-connected region
    add('touching_diagonally', m)
    m = np.zeros((20, 24)); m[3:15, 4:20] = 1; m[5:13, 6:18] = 0
    add('ring', m)
    m = np.zeros((20, 24)); m[3:15, 4:20] = 1; m[5:13, 6:18] = 0; m[8:10, 10:13] = 1       # a blob inside the ring: two regions
    add('ring_with_core', m)
    m = np.zeros((16, 32)); m[1:4, 1:30] = 1; m[8:15, 3:5] = 1
    add('wide_and_tall', m)
    m = np.zeros((16, 16)); m[0:3, 0:3] = 1; m[13:16, 12:16] = 1; m[6:8, 0:2] = 1; m[0:5, 14:16] = 1
    add('at_the_borders', m)
    m = np.zeros((12, 12)); m[1:3, 1:3] = 1; m[5:9, 5:8] = 1                        # even count: the median is a half
    add('two_regions_half_median', m)
    add('full', np.ones((16, 16)))
    m = np.zeros((16, 16)); m[::2, ::2] = 1                                          # isolated pixels, no two touching
    add('checker_sparse', m)
    m = np.zeros((9, 9)); m[np.arange(9), np.arange(9)] = 1                          # a diagonal line: one region, 9 x 9 box
    add('diagonal_line', m)
    add('random_blobs', rng.random((32, 48)) < 0.3)
    return out


def main():
    ms = masks()
    data = {'mask_%d' % k: m for k, (_, m) in enumerate(ms)}
    data['names'] = np.array([n for n, _ in ms])
    data['sizes'] = np.array([float(_anchor_size(m)) for _, m in ms], np.float64)
    np.savez_compressed(os.path.join(OUT, 'nuset_anchor_size.npz'), **data)
    for (n, _), s in zip(ms, data['sizes']):
        print('%-26s %s' % (n, s))


if __name__ == '__main__':
    main()
