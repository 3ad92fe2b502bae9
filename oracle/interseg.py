"""CPU restatement of interSeg's region records and nucleus crops (src/interseg.py:121-152,193-194), exact in integers: what
ecseg_nuclei_regions / ecseg_nucleus_crops (ecseg_amd/csrc/interseg_kernels.hip) return, bit for bit.

* ``region_records``: measure.label(seg, connectivity=None) + regionprops' area, bbox and centroid sums, and the sum of one
  image channel over each region.  Labels are 8-connected and numbered in raster order of each region's first pixel
  (scipy's order is skimage's); aggregation is one ``np.bincount`` per field and ``ndi.find_objects``, so a speckle map
  of 10^5 regions costs as much as one region.
* ``nucleus_crop``: the masked window resized to 256 x 256 as skimage.transform.resize(order=1, mode='reflect',
  preserve_range=True).astype(uint8) does, in exact integers (``exact_resize``).  skimage itself holds k - 1 at pixels
  whose exact value is an integer k (tests/test_interseg_driver.py pins that rule against its fixtures).
"""
import numpy as np
from scipy import ndimage as ndi


def region_records(seg, img, channel0):
    """(H, W) mask, (>= H, >= W, C) uint8 image -> (int64 (n, 8) records, int32 (H, W) label map, 1 + region index or 0).
    Record: area, min row, min col, max row + 1, max col + 1, sum of rows, sum of columns, sum of img[..., channel0]."""
    H, W = seg.shape
    lab, n = ndi.label(np.asarray(seg) != 0, structure=np.ones((3, 3), int))
    rec = np.zeros((n, 8), np.int64)
    if n == 0:
        return rec, lab
    flat = lab.ravel()
    rows = np.repeat(np.arange(H, dtype=np.int64), W)
    cols = np.tile(np.arange(W, dtype=np.int64), H)
    vals = np.ascontiguousarray(img[:H, :W, channel0]).ravel().astype(np.int64)
    # bincount sums its weights in float64: exact while every partial sum is an integer below 2^53
    assert H * W * max(H, W, 256) < 2 ** 53
    rec[:, 0] = np.bincount(flat, minlength=n + 1)[1:]
    for f, wgt in ((5, rows), (6, cols), (7, vals)):
        rec[:, f] = np.bincount(flat, weights=wgt, minlength=n + 1)[1:].astype(np.int64)
    box = ndi.find_objects(lab)
    rec[:, 1:5] = [(r.start, c.start, r.stop, c.stop) for r, c in box]
    return rec, lab


def exact_resize(win):
    """(h, w, C) uint8 window, h, w <= 256 -> the 256 x 256 bilinear of the exact affine map in integers, and the mask of
    the pixels whose value is an exact integer (value * 2^18 divisible by 2^18).  Output row i samples window row
    (h (2i + 1) - 256) / 512; the taps -1 and h reflect to 1 and h - 2 (h = 1: row 0)."""
    h, w = win.shape[:2]
    i = np.arange(256)

    def taps(n):
        q = n * (2 * i + 1) - 256
        a = (q + 512) // 512 - 1
        f = q - a * 512
        refl = (lambda c: np.zeros_like(c)) if n == 1 else (lambda c: np.where(c < 0, -c, np.where(c >= n, 2 * (n - 1) - c, c)))
        return refl(a), refl(a + 1), f
    r0, r1, fr = taps(h)
    c0, c1, fc = taps(w)
    assert win.dtype == np.uint8
    a = win.astype(np.int32)                                 # the 4 weights sum to 2^18: every value < 2^26
    fr, fc = fr.astype(np.int32), fc.astype(np.int32)
    t = (512 - fr)[:, None, None] * a[r0] + fr[:, None, None] * a[r1]              # rows first: the same integer sum
    v = (512 - fc)[None, :, None] * t[:, c0] + fc[None, :, None] * t[:, c1]
    return (v >> 18).astype(np.uint8), (v & (2 ** 18 - 1)) == 0


def nucleus_crop(img, lab, region, y0, x0, h, w, order=(0, 1, 2)):
    """The 256 x 256 x 3 uint8 crop of window (y0, x0, h, w) of ``img`` with every pixel outside region ``region`` (0-based,
    ``lab`` == region + 1) zeroed, channels img[..., order[0]], img[..., order[1]], img[..., order[2]]."""
    win = img[y0:y0 + h, x0:x0 + w][..., list(order)]
    assert win.shape[:2] == (h, w) and 1 <= h <= 256 and 1 <= w <= 256
    keep = lab[y0:y0 + h, x0:x0 + w] == region + 1
    return exact_resize(win * keep[..., None].astype(win.dtype))[0]
