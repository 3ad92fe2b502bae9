"""The min-cut nucleus splitter of ``make stat_fish`` (reference src/max_flow_binary_mask.py, reached through ``use_min_cut: True``).

The reference labels the nucleus mask, takes every region that is large against the median, finds "centres" in its distance
transform and cuts the region between the first two centres with a maximum flow, recursively.  The maximum flows - the whole cost of
the reference, pure-Python Edmonds-Karp - are device work here: ``Handle.min_cut`` (ecseg_min_cut, csrc/mincut_kernels.hip) takes a
batch of independent tasks, and ``segment_min_cut``'s recursion is driven from the host so that all tasks of one recursion depth over
all regions of an image go in one call.  What the reference takes from the flow is the set reachable from the source in the
residual network, which is the same for every maximum flow: the device may augment in any order and the partition is the
reference's.  Everything else is small integer work on bounding-box crops and stays on the host (numpy / scipy).

``cv2.distanceTransform(.., DIST_L1, 3)`` is taken, from OpenCV's documentation, to be the exact city-block distance to the nearest
zero pixel of the crop; OpenCV is not a dependency and this stage is not pinned against it.
"""
import hashlib

import numpy as np

MIN_SIZE = 100                  # segment_min_cut's min_size (src/max_flow_binary_mask.py:119)
FAR = 1 << 30                   # the distance transform of a crop without a zero pixel ("very large")
EIGHT = np.ones((3, 3), int)


def flow_distance(flow_limit):
    """src/max_flow_binary_mask.py:207-208; the reference asserts ``distance > 0``."""
    distance = (-1 + int(np.sqrt(1 + (2 * flow_limit)))) // 2
    if distance < 1:
        raise ValueError('flow_limit = %s gives distance %d: it must be at least 1 (flow_limit >= 4)' % (flow_limit, distance))
    return distance


def city_block_distance(mask):
    """cv2.distanceTransform(mask, cv2.DIST_L1, 3) (src/max_flow_binary_mask.py:161): per pixel the L1 distance to the nearest zero
    pixel of ``mask`` itself, 0 on zero pixels; ``FAR`` everywhere when there is none."""
    from scipy import ndimage
    on = np.asarray(mask) != 0
    if on.all():
        return np.full(on.shape, FAR, np.int64)
    return ndimage.distance_transform_cdt(on, metric='taxicab').astype(np.int64)


def binary_img_to_centers(mask, center_conv, rng):
    """src/max_flow_binary_mask.py:143-156: one centre per 8-connected component (``connectivity=2``, :145) of ``center_conv``, in
    raster order of the components' first pixels (regionprops' order, :146).  The centre is the component's centroid under
    ``np.round`` (:147), i.e. half to even, decided in integers: with sum S over n pixels the mean is exactly k + 1/2 iff
    2 S == n (2 k + 1).  A rounded centroid off the mask (:148) is replaced by ``alternatives[rng.randint(len(alternatives))]``
    (:149-150), the component's pixels in raster order; ``rng`` stands for the global generator the reference seeds once per image
    (:203), so the draws come in the reference's order."""
    from scipy import ndimage
    lab, n = ndimage.label(np.asarray(center_conv) != 0, structure=EIGHT)
    if n == 0:
        return []
    ys, xs = np.nonzero(lab)                                 # raster order
    comp = lab[ys, xs]
    area = np.bincount(comp, minlength=n + 1)
    centers = []
    for k in range(1, n + 1):
        c = []
        for tot in (int(ys[comp == k].sum()), int(xs[comp == k].sum())):
            q, r = divmod(2 * tot + int(area[k]), 2 * int(area[k]))       # floor(mean + 1/2) and whether the mean is k + 1/2
            c.append(q - 1 if (r == 0 and q % 2) else q)
        if not mask[c[0], c[1]]:
            sel = np.flatnonzero(comp == k)
            pick = sel[rng.randint(len(sel))]
            c = [int(ys[pick]), int(xs[pick])]
        centers.append((int(c[0]), int(c[1])))
    return centers


def get_centers(segmented_cells, min_rad=10, percentile=0, rng=None):
    """src/max_flow_binary_mask.py:159-199 on one bounding-box crop (0 / 1) -> list of (row, column) centres.
    Candidates (:163-191): interior pixels of the crop that are on the mask, whose distance is > ``min_rad`` and that pass the four
    non-strict directional tests - not smaller than the neighbour above and below (:169), left and right (:171), on the main
    diagonal (:181) and on the anti-diagonal (:189).  Centre pixels (:196-198): interior pixels with distance >=
    max(percentile of the candidates' distances, min_rad), padded back to the crop (:199).  A crop with h < 3 or w < 3 has no
    interior, hence no centre (:193-195)."""
    mask = np.asarray(segmented_cells)
    if rng is None:
        rng = np.random.RandomState(1)
    if mask.ndim != 2 or mask.shape[0] < 3 or mask.shape[1] < 3:
        return []
    d = city_block_distance(mask)
    c = d[1:-1, 1:-1]
    cand = mask[1:-1, 1:-1] != 0
    cand &= (c >= d[2:, 1:-1]) & (d[:-2, 1:-1] <= c)
    cand &= (c >= d[1:-1, 2:]) & (d[1:-1, :-2] <= c)
    cand &= (c >= d[2:, 2:]) & (d[:-2, :-2] <= c)
    cand &= (c >= d[2:, :-2]) & (d[:-2, 2:] <= c)
    cand &= c > min_rad
    if not cand.any():
        return []
    floor = max(np.percentile(c[cand], percentile), min_rad)
    return binary_img_to_centers(mask, np.pad(c >= floor, 1), rng)


class _Node:
    __slots__ = ('mask', 'centers', 'kids')

    def __init__(self, mask, centers):
        self.mask, self.centers, self.kids = mask, centers, None


def _cells(node):
    if node.kids is not None:
        return _cells(node.kids[0]) + _cells(node.kids[1])   # groups_1 + groups_2 (:140)
    return [node.mask] if node.centers else []               # (:120-123)


def segment_many(items, dist, handle, min_size=MIN_SIZE, stats=None):
    """``segment_min_cut`` (src/max_flow_binary_mask.py:119-140) for many (mask, centers) pairs at once -> per pair the list of
    cell masks in the reference's order.  The recursion tree is grown level by level: every node with two or more centres is one
    task - source ``centers[0]``, sink ``centers[1]`` (:124) - of ONE ``handle.min_cut`` call per level."""
    roots = [_Node((np.asarray(m) != 0).astype(np.uint8), [tuple(int(v) for v in c) for c in cs]) for m, cs in items]
    level = roots
    while True:
        todo = [n for n in level if len(n.centers) > 1]
        if not todo:
            break
        sides, _ = handle.min_cut([(n.mask, n.centers[0], n.centers[1]) for n in todo], dist)
        if stats is not None:
            stats['calls'] = stats.get('calls', 0) + 1
            stats['tasks'] = stats.get('tasks', 0) + len(todo)
            if hasattr(handle, 'timings'):
                stats['kernel_ms'] = stats.get('kernel_ms', 0.0) + handle.timings()['count']
        level = []
        for n, side in zip(todo, sides):
            c1, c2 = n.centers[:2]
            g1 = (np.asarray(side) != 0).astype(np.uint8)
            g2 = n.mask - g1
            centers = list(n.centers)
            if int(g1.sum()) < min_size:                     # (:127-130) the source's side is merged back and its centre dropped
                g1, g2 = np.zeros_like(n.mask), n.mask
                centers.remove(c1)
            elif int(g2.sum()) < min_size:                   # (:131-134)
                g1, g2 = n.mask, np.zeros_like(n.mask)
                centers.remove(c2)
            n.kids = (_Node(g1, [c for c in centers if g1[c]]), _Node(g2, [c for c in centers if g2[c]]))    # (:136-137)
            level += n.kids
    return [_cells(r) for r in roots]


def segment_min_cut(mask, centers, dist, min_size=MIN_SIZE, handle=None):
    """src/max_flow_binary_mask.py:119-140 for one mask: always split on ``centers[:2]``; a side below ``min_size`` pixels is merged
    back and loses its centre; the other centres go to the side whose pixel they sit on; the result is groups_1 + groups_2."""
    return segment_many([(mask, centers)], dist, handle, min_size)[0]


def label_colors(labels, mask, seed=1):
    """The visualisation of src/max_flow_binary_mask.py:228-231: r and g are one byte of blake2b(str(label)) salted with
    "<seed>_r" / "<seed>_g" (0 for label 0), computed once per label; b = clip(384 - r - g, 0, 255) inside ``mask``."""
    labels = np.asarray(labels)
    lut = np.zeros((int(labels.max()) + 1 if labels.size else 1, 2), np.int64)
    for v in np.unique(labels[labels > 0]).tolist():
        for j, salt in enumerate('rg'):
            lut[v, j] = int(hashlib.blake2b(str(v).encode(), digest_size=1, salt=('%s_%s' % (seed, salt)).encode()).hexdigest(), 16)
    r, g = lut[labels, 0], lut[labels, 1]
    b = np.clip(384 - r - g, 0, 255) * (np.asarray(mask) != 0)
    return np.dstack([r, g, b]).astype(np.uint8)


def device_regions(handle, seg, coeff, rng, min_rad=10):
    """The labelling, the selection and ``get_centers`` of every selected region from ONE ``handle.min_cut_regions`` call ->
    (labels, [(label, box, mask, centers)] for the regions with two or more centres).  The host walks the records in region order
    and component order; a component whose rounded centroid is off the mask ([3] == 0) takes ``rng.randint(area)`` and that entry
    of the component's pixels in raster order (:148-150), so the draws come in the reference's order."""
    labels, regions, centers, windows, comps = handle.min_cut_regions((np.asarray(seg) != 0).astype(np.uint8), coeff, min_rad)
    out = []
    for i, reg in enumerate(np.asarray(regions).tolist()):
        k, r0, c0, h, w, _, first, count = reg
        cs = []
        for j, rec in enumerate(np.asarray(centers[first:first + count]).tolist()):
            row, col = rec[1], rec[2]
            if not rec[3]:
                pick = np.flatnonzero(np.asarray(comps[i]).reshape(-1) == j + 1)[rng.randint(rec[4])]
                row, col = divmod(int(pick), w)
            cs.append((int(row), int(col)))
        if len(cs) > 1:
            out.append((k, (slice(r0, r0 + h), slice(c0, c0 + w)), np.asarray(windows[i]), cs))
    return np.asarray(labels), out


def binary_seg_to_instance_min_cut(segmented_cells, flow_limit, cell_size_threshold_coeff, seed=1, handle=None, stats=None,
                                   regions_on_device=False):
    """src/max_flow_binary_mask.py:202-233 -> (labels int32 (H, W), visualization uint8 (H, W, 3)).
    Base labelling (:204): 4-connected (``connectivity=1``), numbered 1..n in raster order of the first pixel -
    ``handle.ccl_labels(mask, 4)`` renumbered by rank.  Regions with area > coeff * median(area) (:205-206,214) are cut where
    ``get_centers`` on their bounding-box crop (:212,215) finds more than one centre (:216), with distance
    ``(-1 + int(sqrt(1 + 2 * flow_limit))) // 2`` (:207).  The first cell of a region keeps its label, the others get
    ``num_cells + 1``, ``+ 2``, ... in region order, then cell order (:220-225).  One ``RandomState(seed)`` per call stands for
    ``np.random.seed(seed)`` (:203).  ``handle``: anything with ``ccl_labels`` and ``min_cut`` (a ``_lib.Handle``); ``stats``: a dict
    that receives the time of the centre finding ('centers', seconds), the device calls ('calls', 'tasks') and their kernel time
    ('kernel_ms').  ``regions_on_device``: everything before the first ``min_cut`` call comes from one
    ``handle.min_cut_regions`` call (``device_regions``); 'centers' is then the wall time of that call plus the record walk."""
    import time
    from scipy import ndimage
    if handle is None:
        raise ValueError('binary_seg_to_instance_min_cut needs a handle with ccl_labels and min_cut')
    seg = np.asarray(segmented_cells)
    if seg.ndim != 2:
        raise ValueError('binary_seg_to_instance_min_cut takes a 2-D mask')
    distance = flow_distance(flow_limit)
    rng = np.random.RandomState(seed)
    if regions_on_device:
        t0 = time.perf_counter()
        labels, found = device_regions(handle, seg, cell_size_threshold_coeff, rng)
        num_cells = int(labels.max()) if labels.size else 0
        if num_cells == 0:
            return labels, label_colors(labels, seg, seed)
        boxes = {k: box for k, box, _, _ in found}
        items = [(mask, centers) for _, _, mask, centers in found]
        owners = [k for k, _, _, _ in found]
    else:
        raw = np.asarray(handle.ccl_labels((seg != 0).astype(np.uint8) * np.uint8(255), 4))
        values = np.unique(raw[raw > 0])
        labels = np.where(raw > 0, np.searchsorted(values, raw) + 1, 0).astype(np.int32)
        num_cells = len(values)
        if num_cells == 0:
            return labels, label_colors(labels, seg, seed)
        areas = np.bincount(labels.reshape(-1), minlength=num_cells + 1)[1:]
        expected = np.median(areas)
        boxes = dict(enumerate(ndimage.find_objects(labels), start=1))
        t0 = time.perf_counter()
        items, owners = [], []
        for k in range(1, num_cells + 1):
            if areas[k - 1] > cell_size_threshold_coeff * expected:
                mask = (labels[boxes[k]] == k).astype(np.uint8)
                centers = get_centers(mask, rng=rng)
                if len(centers) > 1:
                    items.append((mask, centers))
                    owners.append(k)
    if stats is not None:
        stats['centers'] = stats.get('centers', 0.0) + time.perf_counter() - t0
        stats['regions'] = stats.get('regions', 0) + len(items)
    out = labels.copy()
    for k, cells in zip(owners, segment_many(items, distance, handle, stats=stats)):
        view = out[boxes[k]]
        view[labels[boxes[k]] == k] = 0
        for i, cell in enumerate(cells):
            if i:
                num_cells += 1
            view[cell != 0] = k if i == 0 else num_cells
    return out, label_colors(out, seg, seed)
