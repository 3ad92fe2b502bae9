"""The label images the PNG coders are held to (tests/test_png_labels_host.py on the CPU, tests/test_gpu_png_encode.py on the
device): small extents around the 64-pixel blocks the run search works in, and contents that reach every branch of the stream -
no match at all, runs whose k - 1 is a multiple of 64 (no remainder match), runs longer than 64 pixels (whole 256-byte matches),
runs across a block border, labels above 3, and one image large enough that Adler-32 has to be reduced on the way."""
from collections import namedtuple

import numpy as np

Case = namedtuple('Case', 'name labels')
PALETTE = np.array([[0x38, 0x6c, 0xb0, 255], [0xff, 0xff, 0x99, 255], [0x7f, 0xc9, 0x7f, 255], [0xf0, 0x02, 0x7f, 255]], np.uint8)
WIDTHS = (1, 2, 63, 64, 65, 66, 128, 129, 257, 300)
HEIGHTS = (1, 2, 37)


def speckle(rng, H, W):
    return rng.integers(0, 4, (H, W), dtype=np.uint8)


def mixed(rng, H, W):
    """Rows of runs with lengths from 1 to beyond the row: short ones, ones around 64 and ones around 128."""
    out = np.empty((H, W), np.uint8)
    for y in range(H):
        x = 0
        c = int(rng.integers(0, 4))
        while x < W:
            k = int(rng.choice((1, 2, 3, int(rng.integers(1, 20)), int(rng.integers(60, 70)), int(rng.integers(120, 135)), W)))
            out[y, x:x + k] = c
            x += k
            c = (c + 1 + int(rng.integers(0, 3))) % 4
    return out


def blobs(rng, H, W, n=40):
    yy, xx = np.mgrid[:H, :W]
    out = np.zeros((H, W), np.uint8)
    for _ in range(n):
        cy, cx, r = rng.integers(0, H), rng.integers(0, W), rng.integers(3, 30)
        out[(yy - cy) ** 2 + (xx - cx) ** 2 <= r * r] = rng.integers(1, 4)
    return out


def runs_of(k, W, H=2):
    """Runs of exactly k pixels from pixel 0 on, colours in turn; the second row starts one pixel late."""
    row = (np.arange(W) // k % 4).astype(np.uint8)
    out = np.stack([np.roll(row, y) for y in range(H)])
    out[1:, 0] = 3
    return out


def expected_rows(labels):
    """The bytes a decoder must give back: per scan line the filter byte 0 and palette[min(label, 3)] of every pixel."""
    H, W = labels.shape
    rows = np.zeros((H, 1 + 4 * W), np.uint8)
    rows[:, 1:] = PALETTE[np.minimum(labels, 3)].reshape(H, 4 * W)
    return rows.tobytes()


def _cases():
    rng = np.random.default_rng(20261019)
    out = []
    for H in HEIGHTS:
        for W in WIDTHS:
            out.append(Case('mixed_%dx%d' % (H, W), mixed(rng, H, W)))
    for W in WIDTHS:
        out.append(Case('one_colour_2x%d' % W, np.full((2, W), 2, np.uint8)))
        out.append(Case('alternating_2x%d' % W, ((np.arange(W)[None, :] + np.arange(2)[:, None]) % 2 * 3).astype(np.uint8)))
        out.append(Case('speckle_37x%d' % W, speckle(rng, 37, W)))
    out.append(Case('one_colour_1x1', np.zeros((1, 1), np.uint8)))
    for k in (64, 65, 128, 129, 257):
        out.append(Case('runs_of_%d_2x300' % k, runs_of(k, 300)))
        out.append(Case('runs_of_%d_2x%d' % (k, 2 * k), runs_of(k, 2 * k)))
    border = np.zeros((3, 129), np.uint8)
    border[0, 60:70] = 1                                      # across the border of blocks 0 and 1
    border[1, 63:65] = 2                                      # its two pixels on either side of the border
    border[2, 1:128] = 3                                      # over a whole block, borders on both sides
    out.append(Case('block_border_3x129', border))
    clamp = rng.integers(0, 256, (37, 66)).astype(np.uint8)
    clamp[5] = 4
    clamp[6] = 255
    out.append(Case('clamped_37x66', clamp))
    out.append(Case('speckle_300x270', speckle(rng, 300, 270)))
    out.append(Case('blobs_300x270', blobs(rng, 300, 270)))
    out.append(Case('speckle_520x696', speckle(rng, 520, 696)))
    for c in out:
        c.labels.setflags(write=False)
    return out


CASES = _cases()
BATCH_EXTENT = (37, 129)


def batch(n):
    """n different images of one extent: the cases of that extent and seeded ones behind them."""
    rng = np.random.default_rng(77)
    H, W = BATCH_EXTENT
    imgs = [c.labels for c in CASES if c.labels.shape == BATCH_EXTENT]
    while len(imgs) < n:
        imgs.append(mixed(rng, H, W) if len(imgs) % 2 else blobs(rng, H, W, 6))
    return np.ascontiguousarray(np.stack(imgs[:n]))
