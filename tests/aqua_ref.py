"""Restatement of what the reference does with a fourth (aqua) channel when it composes its three colour files
(src/stat_fish.py:110-115 ``merge_channels``, :295-300), for tests/test_stat_fish_aqua.py and tests/test_gpu_stat_fish_aqua.py.
Not a test module, and never the product's Python.

``merge_channels`` evaluates the reference's expression as the reference evaluates it, on whatever dtype comes in: that is the
point.  On the uint8 image of :295 ``coeff * img[..., -1]`` is a Python int times a uint8 array, which stays uint8 and wraps
modulo 256 before the division; on the int array of :297-299 (boundaries are int, so the ``dstack`` is) nothing wraps.  The closed
forms of both (``merged_closed_form``, ``lsq_closed_form``) are what ecseg_fish_render documents; tests/test_stat_fish_aqua.py
asserts on exhaustive inputs that they equal the expression under the numpy in use, so a numpy that changes the wrap is noticed.

Everything here is BGR(A), the reference's order; ``files`` returns the three rasters as the files hold them, RGB
(``cv2.imwrite`` stores a BGR array so)."""
import numpy as np

AQUA_RGB = [233, 137, 54]
K_BGR = (54, 137, 233)                           # AQUA_RGB reversed: the coefficient of blue, green, red


def merge_channels(img, aqua_rgb=AQUA_RGB):
    """:110-115.  (H, W, 3) passes; (H, W, 4) -> uint8 (H, W, 3)."""
    if img.shape[-1] == 3:
        return img
    assert img.shape[-1] == 4
    added = np.dstack([coeff * img[..., -1] / 255 for coeff in aqua_rgb[::-1]])
    return np.minimum(img[..., :-1] + added, 255).astype(np.uint8)


def files(I, thresholded, boundaries):
    """:293-300 from the uint8 BGR(A) image ``I``, the cleaned uint8 (H, W, C - 1) masks and the (H, W) 0 / 255 boundaries ->
    (_original, _original_with_segmentation, _lsq_) as written, RGB."""
    I = np.asarray(I)
    assert I.dtype == np.uint8
    b = np.asarray(boundaries).astype(np.int64)              # get_boundaries returns int arrays
    b3 = np.dstack([b, -b, b])
    merged = merge_channels(I).astype(np.uint8)
    with_segmentation = np.minimum(merged + b3, 255).astype(np.uint8)
    blob = np.dstack([b3[:, :, 0], np.asarray(thresholded)])
    assert blob.dtype == np.int64
    if blob.shape[-1] > 3:
        blob = merge_channels(blob)
    blob = blob.astype(np.uint8)
    return tuple(np.ascontiguousarray(a[..., ::-1]) for a in (merged, with_segmentation, blob))


def merged_closed_form(I):
    """out_c = min(255, a_c + [((k_c * q) & 255) == 255]) on a uint8 BGRA image."""
    I = np.asarray(I).astype(np.int64)
    q = I[..., 3]
    return np.dstack([np.minimum(I[..., c] + (((k * q) & 255) == 255), 255) for c, k in enumerate(K_BGR)]).astype(np.uint8)


def lsq_closed_form(blob):
    """out_c = min(255, x_c + k_c * m // 255) on the int (boundaries, mask 0, mask 1, mask 2) array."""
    blob = np.asarray(blob).astype(np.int64)
    m = blob[..., 3]
    return np.dstack([np.minimum(blob[..., c] + k * m // 255, 255) for c, k in enumerate(K_BGR)]).astype(np.uint8)


def exhaustive_image():
    """(256, 256, 4) uint8: the three colour channels hold the row number, aqua the column number: every (a, q) pair under every
    coefficient."""
    a, q = np.meshgrid(np.arange(256, dtype=np.uint8), np.arange(256, dtype=np.uint8), indexing='ij')
    return np.ascontiguousarray(np.dstack([a, a, a, q]))


def lsq_combinations():
    """The sixteen 0 / 255 combinations -> (boundaries (4, 4), thresholded (4, 4, 3)), both uint8."""
    bits = np.arange(16).reshape(4, 4)
    planes = [(((bits >> j) & 1) * 255).astype(np.uint8) for j in range(4)]
    return planes[0], np.ascontiguousarray(np.dstack(planes[1:]))
