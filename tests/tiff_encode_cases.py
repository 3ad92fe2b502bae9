"""The case list of the device TIFF encoder (csrc/tiff_kernels.hip): seeded uint8 images at the smallest shapes at which it can go
wrong.  tests/test_tiff_encode.py holds the list to its coverage (restarts, width steps at EOI, odd and even strips) with the
restatement tests/lzw_ref.py; tests/test_gpu_tiff_encode.py runs every case on the device."""
from collections import namedtuple

import numpy as np

import lzw_ref

Case = namedtuple('Case', 'name img invert')
SEED = 20240


def _noise(seed, *shape):
    return np.random.default_rng(seed).integers(0, 256, shape, dtype=np.uint8)


def _row_with_predicted_bytes(want):
    """A one-row gray image whose predicted bytes (what the encoder sees) are ``want``: the running sum modulo 256."""
    return np.cumsum(np.frombuffer(want, np.uint8), dtype=np.uint64).astype(np.uint8)[None, :]


def _build():
    cases = []

    def add(name, img, invert=False):
        cases.append(Case(name, np.ascontiguousarray(img, np.uint8), invert))

    # extents and strips
    add('gray_1x1', _noise(1, 1, 1))
    add('gray_3x1', _noise(2, 3, 1))
    add('gray_3x4096_two_rows_per_strip_short_last', _noise(3, 3, 4096))
    add('gray_2x8192_one_row_per_strip', _noise(4, 2, 8192))
    add('gray_2x8193_strip_longer_than_8192', _noise(5, 2, 8193))
    add('rgb_2x2731_line_8193', _noise(6, 2, 2731, 3))
    add('rgb_5x7', _noise(7, 5, 7, 3))
    ramp300 = (np.arange(300)[:, None] * 3 + np.arange(4097)[None, :] // 5).astype(np.uint8)
    ramp300[::7, ::11] ^= _noise(8, 300, 4097)[::7, ::11]
    add('gray_300x4097_more_strips_than_cus', ramp300)
    add('gray_2x100_one_strip_offset_inline', _noise(9, 2, 100))
    add('gray_5x333_invert', _noise(10, 5, 333), True)
    add('rgb_3x1392_three_strips', _noise(11, 3, 1392, 3))
    # data
    add('gray_40x200_constant', np.full((40, 200), 77))
    add('gray_1x9000_constant_row', np.full((1, 9000), 200))
    add('gray_20x300_ramp', np.arange(6000).reshape(20, 300) // 3)
    add('rgb_9x500_ramp', (np.arange(13500).reshape(9, 500, 3) * 7) // 5)
    add('gray_31x257_noise', _noise(12, 31, 257))
    add('gray_128x64_noise_one_strip_with_a_restart', _noise(13, 128, 64))
    add('gray_2x12000_noise_several_restarts_in_a_strip', _noise(14, 2, 12000))
    # boundary lengths: one-row strips of predicted noise, their lengths found by the restatement
    stream = _noise(SEED, 6000).tobytes()
    for what, n in sorted(lzw_ref.boundary_lengths(stream).items()):
        add('gray_1x%d_%s' % (n, what), _row_with_predicted_bytes(stream[:n]))
    return cases


CASES = _build()


def spp(case):
    return 1 if case.img.ndim == 2 else 3
