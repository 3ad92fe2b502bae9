"""CPU oracle of fish_distance_calculation for the tests and tools: what the reference's ``get_distances_img``
(src/fish_distance_calculation.py:16-46) computes, written from its contract.  Not a test module.

It is a restatement, not a capture of the reference's output: scikit-image is not a dependency of this suite, so
``scipy.ndimage.label(structure=ones((3, 3)))`` counts the 8-connected FISH spots where the reference calls
``skimage.measure.label`` (same components for a 2-D mask; only their number is read), and cells are the labels > 0 that
occur, ascending, as ``regionprops`` walks them.  ``loop`` keeps the one piece of float arithmetic that decides the bits of
a value: ``np.linalg.norm(c - f, axis=1).min() / np.sqrt(area)`` per FISH pixel ``f``, then the minimum over ``f``.

``records`` is an independent, vectorised producer of the eight integer fields ecseg_fish_distances returns.
"""
import numpy as np
from scipy import ndimage

EIGHT = np.ones((3, 3), int)


def loop(lsq, segmentation, presets):
    """One value per accepted nucleus, ascending labels; presets = (centromere channel, FISH channel, spot limit).
    A nucleus counts when channels 0 and 1 are both non-zero somewhere inside it and its FISH pixels form at most
    ``spot limit`` 8-connected spots; its value is inf without FISH pixels.  FISH pixels without a centromere pixel raise
    ValueError (the minimum of nothing), where the reference stops too."""
    cen_channel, fish_channel, spot_limit = presets
    seg = np.asarray(segmentation)
    lsq = np.asarray(lsq)
    values = []
    for label in np.unique(seg[seg > 0]).tolist():
        inside = seg == label
        if not (lsq[..., 0][inside].any() and lsq[..., 1][inside].any()):
            continue
        fish_mask = inside & (lsq[..., fish_channel] != 0)
        if ndimage.label(fish_mask, structure=EIGHT)[1] > spot_limit:
            continue
        root_area = np.sqrt(inside.sum())
        fish_yx = np.argwhere(fish_mask)
        cen_yx = np.argwhere(inside & (lsq[..., cen_channel] != 0))
        value = float('inf')
        for f in fish_yx:
            value = min(value, np.linalg.norm(cen_yx - f, axis=1).min() / root_area)
        values.append(value)
    return values


def records(lsq, segmentation, fish_index, centromere_index):
    """int64 (n_cells, 8) records of ecseg_fish_distances: label, area, gate bits, FISH pixels, centromere pixels, FISH
    components (8-connected inside the cell), min squared FISH - centromere distance (-1: a set is empty), 0."""
    seg = np.asarray(segmentation).astype(np.int64)
    lsq = np.asarray(lsq)
    labels = np.unique(seg[seg > 0])
    out = np.zeros((len(labels), 8), np.int64)
    if not len(labels):
        return out
    n = len(labels)
    inside = seg > 0
    idx = np.searchsorted(labels, np.where(inside, seg, labels[0]))

    def per_cell(mask):
        return np.bincount(idx[mask & inside], minlength=n)
    fish = (lsq[..., fish_index] != 0) & inside
    cen = (lsq[..., centromere_index] != 0) & inside
    out[:, 0] = labels
    out[:, 1] = per_cell(np.ones(seg.shape, bool))
    out[:, 2] = (per_cell(lsq[..., 0] != 0) > 0) + 2 * (per_cell(lsq[..., 1] != 0) > 0)
    out[:, 3] = per_cell(fish)
    out[:, 4] = per_cell(cen)
    out[:, 6] = -1
    # the pixels of every cell, grouped: one stable sort instead of a full-image mask per cell
    fy, fx = np.nonzero(fish)
    cy, cx = np.nonzero(cen)
    f_cell, c_cell = idx[fy, fx], idx[cy, cx]
    f_order, c_order = np.argsort(f_cell, kind='stable'), np.argsort(c_cell, kind='stable')
    f_start = np.searchsorted(f_cell[f_order], np.arange(n + 1))
    c_start = np.searchsorted(c_cell[c_order], np.arange(n + 1))
    for k in np.flatnonzero(out[:, 3] > 0):
        f = f_order[f_start[k]:f_start[k + 1]]
        y, x = fy[f].astype(np.int64), fx[f].astype(np.int64)
        y0, x0 = y.min(), x.min()
        box = np.zeros((y.max() - y0 + 1, x.max() - x0 + 1), bool)
        box[y - y0, x - x0] = True                           # FISH pixels of THIS cell only
        out[k, 5] = ndimage.label(box, structure=EIGHT)[1]
        c = c_order[c_start[k]:c_start[k + 1]]
        if not len(c):
            continue
        yy, xx = cy[c].astype(np.int64), cx[c].astype(np.int64)
        best = None
        for j0 in range(0, len(c), 2048):                    # bounded memory for dense masks
            for i0 in range(0, len(f), 2048):
                d = (y[i0:i0 + 2048, None] - yy[None, j0:j0 + 2048]) ** 2 + (x[i0:i0 + 2048, None] - xx[None, j0:j0 + 2048]) ** 2
                m = int(d.min())
                best = m if best is None else min(best, m)
            if best == 0:
                break
        out[k, 6] = best
    return out
