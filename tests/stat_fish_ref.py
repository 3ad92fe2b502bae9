"""CPU oracle of stat_fish behind nuclei_segment for the tests and tools: what the reference's ``get_thresholded``, the loop over
``regionprops`` with ``count_blobs`` / ``intensity_metrics`` and ``get_boundaries`` compute (src/stat_fish.py:73-107,134-142,
226-300), written from the contract of ecseg_fish_spots.  Not a test module, and never the product's Python.

It is a restatement, not a capture of the reference's output (TensorFlow, scikit-image and OpenCV are not dependencies of this
suite): ``scipy.ndimage.label`` with its default structure labels the spots - the very function the reference calls -, cells
are the labels > 0 that occur, ascending, as ``regionprops`` walks them, the correlation is an explicit float64 sum over the
taps of the zero-padded channel, and the boundary sums are integers.

``loop`` walks cell by cell as the reference does; ``records`` is an independent, vectorised producer of the same fields
(connected components of the pixel graph whose edges join 4-neighbours of one cell).

The float64 decision ``coefficient > normal_threshold`` is the one place where two correct evaluations may differ: any summation
order, with or without FMA, lies within ``B = g * sum(|w| * |x|)`` of the exact value, ``g = n u / (1 - n u)``, ``n = K * K``,
``u = 2 ** -53`` (derived, not measured; it also covers TensorFlow's unknown order).  ``ambiguous`` counts the pixels whose
decision matters and whose coefficient is within ``2 B`` of the threshold.
"""
import numpy as np
from scipy import ndimage
from scipy.sparse import coo_matrix
from scipy.sparse.csgraph import connected_components

N_FIELDS = 24
EIGHT = np.ones((3, 3), int)


def nuclei(mask):
    """measure.label(mask, connectivity=None) of a 2-D mask: 8-connected, numbered in raster order of the first pixel."""
    return ndimage.label(np.asarray(mask) != 0, structure=EIGHT)[0]


def ranks(seg):
    seg = np.asarray(seg).astype(np.int64)
    values = np.unique(seg[seg > 0])
    return np.where(seg > 0, np.searchsorted(values, seg) + 1, 0), values


def correlate(channel, weights):
    """Zero-padded "SAME" correlation, float64, one explicit sum per tap (row-major tap order)."""
    x = np.asarray(channel, np.float64)
    w = np.asarray(weights, np.float64)
    K = w.shape[0]
    r = K // 2
    H, W = x.shape
    pad = np.zeros((H + 2 * r, W + 2 * r), np.float64)
    pad[r:r + H, r:r + W] = x
    out = np.zeros((H, W), np.float64)
    with np.errstate(invalid='ignore'):
        for ky in range(K):
            for kx in range(K):
                out = out + w[ky, kx] * pad[ky:ky + H, kx:kx + W]
    return out


def error_bound(channel, weights):
    w = np.abs(np.asarray(weights, np.float64))
    n = w.size
    u = 2.0 ** -53
    g = n * u / (1 - n * u)
    with np.errstate(invalid='ignore'):
        return g * correlate(np.abs(np.asarray(channel, np.float64)), w)


def thresholded(img, probes, seg, weights, normal_threshold, intensity_thresholds):
    """get_thresholded (:73-88) -> (uint8 (H, W, n_probe) 0 / 255 before the small spots go, number of ambiguous pixels)."""
    img = np.asarray(img)
    seg = np.asarray(seg)
    out = np.zeros(seg.shape + (len(probes),), np.uint8)
    ambiguous = 0
    for j, (c, it) in enumerate(zip(probes, intensity_thresholds)):
        channel = img[..., c]
        coefficient = correlate(channel, weights)
        with np.errstate(invalid='ignore'):
            normal = coefficient > normal_threshold
        top = int(channel.max()) if channel.size else 0
        is_max = (channel == top) & bool(top)
        matters = (channel.astype(np.float64) > it) & (seg > 0) & ~is_max
        with np.errstate(invalid='ignore'):
            near = np.abs(coefficient - normal_threshold) <= 2 * error_bound(channel, weights)
        ambiguous += int((matters & near).sum())
        out[..., j] = ((normal | is_max) & (channel.astype(np.float64) > it) & (seg > 0)) * np.uint8(255)
    return out, ambiguous


def boundaries(rank, t):
    """get_boundaries (:91-107) on the rank map: integer sums of the 2 t taps, padding t - 1 before and t after."""
    R = np.asarray(rank).astype(np.int64)
    H, W = R.shape
    ph = np.pad(R, ((0, 0), (t - 1, t)))
    pv = np.pad(R, ((t - 1, t), (0, 0)))
    h = np.zeros((H, W), np.int64)
    v = np.zeros((H, W), np.int64)
    for j in range(2 * t):
        sign = 1 if j < t else -1
        h += sign * ph[:, j:j + W]
        v += sign * pv[j:j + H, :]
    return ((h != 0) | (v != 0)).astype(np.uint8) * np.uint8(255)


def _count_blobs(fish_splice, cell_seg, min_cc):
    """count_blobs (:134-142): clears the small blobs of this cell from fish_splice in place."""
    labeled, count = ndimage.label(fish_splice * cell_seg)
    for blob in range(1, count + 1):
        component = labeled == blob
        if component.sum() < min_cc:
            fish_splice[component] = 0
            count -= 1
    return count


def loop(img, seg, probes, weights, normal_threshold, intensity_thresholds, min_cc, line_thickness):
    """-> (records int64 (n, 24), cleaned thresholded, boundaries, ambiguous pixel count), cell by cell as :249-275."""
    img = np.asarray(img)
    rank, values = ranks(seg)
    thr, ambiguous = thresholded(img, probes, rank, weights, normal_threshold, intensity_thresholds)
    thr = thr.astype(np.int64)
    rec = np.zeros((len(values), N_FIELDS), np.int64)
    for k, sl in enumerate(ndimage.find_objects(rank)):
        cell_seg = (rank[sl] == k + 1).astype(np.int64)
        ys, xs = np.nonzero(rank == k + 1)
        rec[k, :4] = values[k], len(ys), ys.sum(), xs.sum()
        fish = [thr[sl + (j,)] for j in range(len(probes))]                 # views: clearing shows in thr
        for j, c in enumerate(probes):
            raw = img[sl + (c,)].astype(np.int64) * cell_seg
            foci = _count_blobs(fish[j], cell_seg, min_cc)
            rec[k, 4 + 5 * j:9 + 5 * j] = (fish[j] * cell_seg).sum() // 255, foci, raw.sum(), np.count_nonzero(raw), raw.max()
        if len(probes) >= 2:
            pair = fish[0] * (fish[1] // 255)
            rec[k, 20] = _count_blobs(pair, cell_seg, min_cc)
            rec[k, 19] = (pair * cell_seg).sum() // 255
    return rec, thr.astype(np.uint8), boundaries(rank, line_thickness), ambiguous


def _components(mask, rank):
    """4-connected components of mask joined only inside one cell -> (component id per pixel, -1 outside; sizes)."""
    H, W = mask.shape
    idx = np.arange(H * W).reshape(H, W)
    a = mask[:, 1:] & mask[:, :-1] & (rank[:, 1:] == rank[:, :-1])
    b = mask[1:, :] & mask[:-1, :] & (rank[1:, :] == rank[:-1, :])
    src = np.concatenate([idx[:, 1:][a], idx[1:, :][b]])
    dst = np.concatenate([idx[:, :-1][a], idx[:-1, :][b]])
    graph = coo_matrix((np.ones(len(src), np.int8), (src, dst)), shape=(H * W, H * W))
    _, comp = connected_components(graph, directed=False)
    comp = comp.reshape(H, W)
    sizes = np.bincount(comp[mask], minlength=H * W)
    return np.where(mask, comp, -1), sizes


def records(img, seg, probes, weights, normal_threshold, intensity_thresholds, min_cc, line_thickness):
    """The vectorised second producer: same return value as ``loop``."""
    img = np.asarray(img)
    rank, values = ranks(seg)
    n = len(values)
    thr, ambiguous = thresholded(img, probes, rank, weights, normal_threshold, intensity_thresholds)
    rec = np.zeros((n, N_FIELDS), np.int64)
    inside = rank > 0
    cell = rank[inside] - 1
    yy, xx = np.nonzero(inside)
    rec[:, 0] = values
    rec[:, 1] = np.bincount(cell, minlength=n)
    rec[:, 2] = np.bincount(cell, weights=yy, minlength=n).astype(np.int64)
    rec[:, 3] = np.bincount(cell, weights=xx, minlength=n).astype(np.int64)

    def kept(mask):
        comp, sizes = _components(mask, rank)
        keep = mask & (sizes[np.where(mask, comp, 0)] >= min_cc)
        roots = np.unique(comp[keep])
        first = ndimage.minimum(np.arange(mask.size).reshape(mask.shape), comp, roots) if len(roots) else np.zeros(0)
        owner = rank.ravel()[np.asarray(first, np.int64)] - 1
        return keep, np.bincount(rank[keep] - 1, minlength=n), np.bincount(owner, minlength=n)

    clean = []
    for j, c in enumerate(probes):
        keep, pixels, foci = kept(thr[..., j] != 0)
        clean.append(keep)
        raw = img[..., c][inside].astype(np.int64)
        rec[:, 4 + 5 * j] = pixels
        rec[:, 5 + 5 * j] = foci
        rec[:, 6 + 5 * j] = np.bincount(cell, weights=raw, minlength=n).astype(np.int64)
        rec[:, 7 + 5 * j] = np.bincount(cell[raw != 0], minlength=n)
        if n:
            rec[:, 8 + 5 * j] = ndimage.maximum(img[..., c].astype(np.int64), rank, np.arange(1, n + 1))
    if len(probes) >= 2:
        _, rec[:, 19], rec[:, 20] = kept(clean[0] & clean[1])
    out = np.stack(clean, axis=-1).astype(np.uint8) * np.uint8(255) if clean else thr
    return rec, out, boundaries(rank, line_thickness), ambiguous
