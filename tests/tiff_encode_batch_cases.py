"""The case list of the batched device TIFF encoder (the tiffb_* kernels of csrc/tiff_kernels.hip, csrc/tiff_encode_batch.h): tiny
seeded rasters, each chosen for a branch of the strip routine or of the layout, and the batches made of them.
tests/test_tiff_encode_batch.py holds the list to the branches it is named for with the restatement tests/lzw_ref.py;
tests/test_gpu_tiff_encode_batch.py runs every case and every batch on the device."""
import numpy as np

import lzw_ref
from tiff_encode_cases import Case, _noise, _row_with_predicted_bytes, spp      # noqa: F401

CHUNK = 1024                                     # TL_IN: the bytes of a strip that are staged at once


def restart_byte(data):
    """Index of the byte at which the strip's first table restart happens (the byte that creates entry 4093), or None."""
    states = []
    lzw_ref.encode(data, states)
    return next((i + 1 for i, s in enumerate(states) if s[2]), None)


def _restart_on_a_chunk_border(seed):
    """Predicted bytes of one strip (at most 8192) whose first restart falls on the last byte of a staged chunk: zeros in front of
    seeded noise - a zero more moves the restart one byte on, or not at all where it adds a table entry."""
    noise = _noise(seed, 6000).tobytes()
    p = 0
    for _ in range(40):
        k = restart_byte(bytes(p) + noise)
        if k % CHUNK == CHUNK - 1:
            return (bytes(p) + noise)[:k + 1 + 700]
        p += (CHUNK - 1 - k) % CHUNK
    raise AssertionError('no prefix puts the restart on a chunk border')


def _build():
    cases = []

    def add(name, img, invert=False):
        cases.append(Case(name, np.ascontiguousarray(img, np.uint8), invert))

    add('gray_1x1', _noise(31, 1, 1))
    add('rgb_1x1', _noise(32, 1, 1, 3))
    add('gray_7x1392_five_rows_per_strip_short_last', _noise(33, 7, 1392) // 32)
    add('gray_5x333_invert', _noise(34, 5, 333), True)
    add('gray_1x1023_below_a_chunk', _noise(35, 1, 1023))
    add('gray_8x128_exactly_a_chunk', _noise(36, 8, 128))
    add('gray_1x1025_a_chunk_and_a_byte', _noise(37, 1, 1025))
    add('rgb_2x2731_line_8193', _noise(38, 2, 2731, 3) // 64)
    add('gray_1x8192_noise_restart_inside', _noise(39, 1, 8192))
    add('gray_restart_on_a_chunk_border', _row_with_predicted_bytes(_restart_on_a_chunk_border(40)))
    add('gray_4x2048_constant_strip', np.full((4, 2048), 9))
    add('rgb_5x7_invert_off', _noise(41, 5, 7, 3))
    add('gray_3x50_ramp', np.arange(150).reshape(3, 50) // 4)
    add('rgb_9x500_ramp', (np.arange(13500).reshape(9, 500, 3) * 7) // 5)
    return cases


CASES = _build()


def _order(n, seed=None):
    """n case indices: the list cycled, or a seeded shuffle of that."""
    idx = [k % len(CASES) for k in range(n)] if n >= len(CASES) else list(range(0, len(CASES), max(1, len(CASES) // n)))[:n]
    if seed is not None:
        mixed = [idx[k] for k in np.random.default_rng(seed).permutation(len(idx))]
        idx = mixed if mixed != idx else idx[::-1]
    return idx


# every composition in two orders; the 17-file ones hold every case, both sample counts, invert on and off
BATCHES = {}
for _n in (1, 2, 3, 8, 17):
    BATCHES['%d_files' % _n] = _order(_n)
    BATCHES['%d_files_shuffled' % _n] = _order(_n, seed=50 + _n)
BATCHES['1_files_shuffled'] = [CASES.index(next(c for c in CASES if c.name.startswith('rgb_2x2731')))]      # (one file has one order: another file)


def pack(cases, gaps=None):
    """-> (1-D uint8 buffer, (n, 5) int64 table: byte offset, H, W, spp, invert) with ``gaps[k]`` bytes of 0xEE in front of raster k."""
    gaps = [0] * len(cases) if gaps is None else gaps
    parts, rows, at = [], [], 0
    for c, g in zip(cases, gaps):
        parts.append(np.full(g, 0xEE, np.uint8))
        at += g
        rows.append([at, c.img.shape[0], c.img.shape[1], spp(c), int(c.invert)])
        parts.append(c.img.reshape(-1))
        at += c.img.size
    return (np.concatenate(parts) if parts else np.zeros(0, np.uint8)), np.array(rows, np.int64).reshape(-1, 5)
