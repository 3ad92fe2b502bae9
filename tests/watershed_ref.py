"""numpy / scipy restatement of the ``py_func`` half of NuSeT's ``nuclei_segment`` (reference src/utils.py:153-162):
``_watershed`` (src/model_layers/marker_watershed.py:9-96), ``clean_image`` (src/nuset_utils/normalization.py:25-37) and the final
threshold with ``remove_small_objects``.  Python 3, modern numpy, no scikit-image; the reference's quirks are kept, not fixed.

tests/test_watershed.py requires it to equal tests/golden/nuset_watershed.npz (made by tools/make_golden_watershed.py from the
reference's own functions) byte for byte; the GPU tests and tools/fuzz_watershed.py compare the device against it.

The flood is scikit-image 0.18's ``watershed(-distance, markers_rw, mask=mask, watershed_line=True)`` with ``connectivity=1``.  Its
queue is a binary heap ordered by (value, age); the value is restated as the integer -d^2 (sqrt is strictly monotone on integers
below 2^52).  Every marker pixel carries age 0, so marker pixels of equal d^2 have EQUAL keys and leave the heap in an order that
only the heap's own sift rules decide - and that order shows in the result (the ages of what they push depend on it).  ``flood``
therefore restates the heap itself (``_Heap``); the campaign of tools/make_golden_watershed.py found no difference with it.
One FIFO per value with markers in raster order is identical wherever no two marker pixels tie and differs from scikit-image on
about 4 random scenes in 1000 (``flood_fifo`` in the golden tool keeps measuring that)."""
import numpy as np
from scipy import ndimage as ndi

EDGE = 20                                                # marker_watershed.py:16
MIN_REGION_AREA = 10                                     # :65
DISK3 = [(dy, dx) for dy in range(-3, 4) for dx in range(-3, 4) if dy * dy + dx * dx <= 9]   # morphology.disk(3): 29 offsets
NEIGHBOURS = ((-1, 0), (0, -1), (0, 1), (1, 0))          # _offsets_to_raveled_neighbors at connectivity 1: raveled order
FULL8 = np.ones((3, 3), int)


def _round(v):
    """Python's ``round``: half to even."""
    return int(round(float(v)))


def marker_list(scores, proposals, mask, min_score):
    """Lines 22-80: the ordered markers as (rows, cols, labels) int32 arrays, later entries overwriting earlier ones, or None for
    the two all-ones-contour branches (no score, or none above ``min_score``)."""
    scores = np.asarray(scores, np.float32).reshape(-1)
    proposals = np.asarray(proposals, np.float32).reshape(-1, 4)
    m = np.asarray(mask) != 0
    H, W = m.shape
    if scores.size == 0 or not scores.max() > min_score:
        return None
    top = scores > min_score
    scores, proposals = scores[top], proposals[top]
    order = scores.argsort()                             # ascending, numpy's default quicksort as in the reference
    proposals = proposals[order]
    markers = np.zeros((H, W), np.int64)
    rows, cols = [], []
    for b in proposals:
        r = _round((b[3] + b[1]) / np.float32(2))        # "x_pos" is the row: bbox[1], bbox[3]
        c = _round((b[2] + b[0]) / np.float32(2))
        if r >= H or c >= W or r < -H or c < -W:
            raise IndexError('marker (%d, %d) outside the %d x %d image: the reference raises here' % (r, c, H, W))
        r, c = r % H, c % W                              # numpy's negative indices wrap
        if EDGE <= r < H - EDGE and EDGE <= c < W - EDGE:
            rows.append(r); cols.append(c)
            markers[r, c] = len(rows)
    lab, n = ndi.label(m, structure=FULL8)               # morphology.label's default: full connectivity
    areas = np.bincount(lab.ravel(), minlength=n + 1)
    for k, sl in enumerate(ndi.find_objects(lab)):
        if areas[k + 1] < MIN_REGION_AREA:
            continue
        r0, r1 = min(sl[0].start, H - 1), min(sl[0].stop, H - 1)
        c0, c1 = min(sl[1].start, W - 1), min(sl[1].stop, W - 1)
        if markers[r0:r1, c0:c1].sum() == 0:
            r, c = _round((r0 + r1) / 2), _round((c0 + c1) / 2)
            rows.append(r); cols.append(c)
            markers[r, c] = len(rows)
    return np.asarray(rows, np.int32), np.asarray(cols, np.int32), np.arange(1, len(rows) + 1, dtype=np.int32)


def marker_image(shape, rows, cols, labels):
    m = np.zeros(shape, np.int64)
    for r, c, l in zip(rows, cols, labels):
        m[r, c] = l
    return m


def dilate_disk3(markers):
    H, W = markers.shape
    pad = np.zeros((H + 6, W + 6), markers.dtype)
    pad[3:-3, 3:-3] = markers
    out = np.zeros_like(markers)
    for dy, dx in DISK3:
        np.maximum(out, pad[3 + dy:3 + dy + H, 3 + dx:3 + dx + W], out=out)
    return out


def fill_holes(mask):
    """``binary_fill_holes`` with its default structure: the background components that do not reach the border, 4-connected, are set."""
    return ndi.binary_fill_holes(np.asarray(mask) != 0)


def squared_edt(filled):
    """d^2 of ``distance_transform_edt`` as int64.  An image without a zero pixel gets scipy's answer, the distance to (-1, 0)."""
    d = ndi.distance_transform_edt(np.asarray(filled) != 0)
    return np.rint(d * d).astype(np.int64)


def squared_distance(mask):
    """d^2 of ``distance_transform_edt(binary_fill_holes(mask))`` as int64."""
    return squared_edt(fill_holes(mask))


def squared_edt_brute(filled):
    """``squared_edt`` a second time with nothing shared: per pixel the minimum of dy^2 + dx^2 over every zero pixel, in integers, no
    scipy.  O(pixels x zeros): for small images.  Without a zero, (row + 1)^2 + column^2: scipy's documented distance to (-1, 0)."""
    f = np.asarray(filled) != 0
    H, W = f.shape
    yy, xx = np.mgrid[:H, :W].astype(np.int64)
    zy, zx = (v.astype(np.int64) for v in np.nonzero(~f))
    if zy.size == 0:
        return (yy + 1) ** 2 + xx ** 2
    out = np.empty((H, W), np.int64)
    for y in range(H):                                       # a row at a time: (W, zeros) values
        out[y] = ((y - zy[None, :]) ** 2 + (xx[y][:, None] - zx[None, :]) ** 2).min(axis=1)
    return out


class _Heap:
    """A binary heap on (value, age) with the classic push (swim up while strictly smaller) and pop (last to the root, sink towards
    the smaller child, left on ties): the order of equal keys depends on it."""

    def __init__(self):
        self.a = []

    def push(self, e):
        a = self.a
        a.append(e)
        c = len(a) - 1
        while c > 0:
            p = (c + 1) // 2 - 1
            if a[c][:2] < a[p][:2]:
                a[c], a[p] = a[p], a[c]
                c = p
            else:
                break

    def pop(self):
        a = self.a
        top = a[0]
        last = a.pop()
        if a:
            a[0] = last
            i, n = 0, len(a)
            while True:
                l, r, s = 2 * i + 1, 2 * i + 2, i
                if l >= n:
                    break
                if a[l][:2] < a[i][:2]:
                    s = l
                if r < n and a[r][:2] < a[s][:2]:
                    s = r
                if s == i:
                    break
                a[i], a[s] = a[s], a[i]
                i = s
        return top


def flood(mask, markers_rw, d2, heap=_Heap, neighbours=NEIGHBOURS, lines=None):
    """The watershed with lines on one binary heap over the whole image: int64 labels, 0 on lines (a marker pixel that becomes a line
    keeps its label), outside the mask and where no marker reaches.  ``lines``: a list that receives the (row, column) of every line
    pixel in the order they are found.  ``heap`` and ``neighbours`` are what tests/test_watershed_stages.py swaps for wrong ones."""
    m = (np.asarray(mask) != 0).copy()
    H, W = m.shape
    out = (markers_rw * m).astype(np.int64)
    hp = heap()
    for r, c in zip(*np.nonzero(out)):
        hp.push((-int(d2[r, c]), 0, int(r), int(c), int(r), int(c)))
    age = 0
    while hp.a:
        _, _, r, c, sr, sc = hp.pop()
        if out[r, c] and (r, c) != (sr, sc):
            continue
        labs = set(int(out[r + dy, c + dx]) for dy, dx in neighbours
                   if 0 <= r + dy < H and 0 <= c + dx < W and m[r + dy, c + dx] and out[r + dy, c + dx])
        if len(labs) > 1:
            m[r, c] = False
            if lines is not None:
                lines.append((r, c))
            continue
        out[r, c] = out[sr, sc]
        for dy, dx in neighbours:
            y, x = r + dy, c + dx
            if 0 <= y < H and 0 <= x < W and m[y, x] and not out[y, x]:
                age += 1
                hp.push((-int(d2[y, x]), age, y, x, sr, sc))
    return out


def watershed_from_markers(mask, rows, cols, labels, flood_fn=flood):
    """Lines 82-91 from the ordered marker list: ``pred_mask * contour`` as int32."""
    mask = np.asarray(mask)
    rw = dilate_disk3(marker_image(mask.shape, rows, cols, labels))
    lab = flood_fn(mask, rw, squared_distance(mask))
    return (mask.astype(np.int64) * (lab != 0)).astype(np.int32)


def stages(mask, rows, cols, labels, marker_fn=marker_image, dilate_fn=dilate_disk3, mask_rw=True, fill_fn=fill_holes, edt_fn=squared_edt,
           flood_fn=flood):
    """``watershed_from_markers`` with everything on the way, as the device keeps it (ecseg_marker_watershed_stages_debug):
    rw int32 = markers_rw * mask; filled uint8 0 / 1; d2 int32 = the squared distance on the mask's pixels and 0 off the mask (the flood
    reads it nowhere else; ``squared_edt_brute(filled)`` says what the filled holes would hold); lab int32 = the flood's labels; out
    int32 = ``pred_mask * contour``.  The keyword arguments are the stages themselves: tests/test_watershed_stages.py swaps one for a
    wrong one and asks who notices."""
    mask = np.asarray(mask)
    m = mask != 0
    rw = dilate_fn(marker_fn(mask.shape, rows, cols, labels))
    if mask_rw:
        rw = rw * m
    filled = fill_fn(mask)
    d2 = edt_fn(filled) * m
    lab = flood_fn(mask, rw, d2)
    out = (mask.astype(np.int64) * (lab != 0)).astype(np.int32)
    return dict(rw=rw.astype(np.int32), filled=filled.astype(np.uint8), d2=d2.astype(np.int32), lab=lab.astype(np.int32), out=out)


STAGE_ORDER = ('rw', 'filled', 'd2', 'lab', 'out')


def watershed(scores, proposals, mask, min_score, flood_fn=flood):
    """``_watershed``: int32 (H, W)."""
    mk = marker_list(scores, proposals, mask, min_score)
    if mk is None:
        return np.asarray(mask).astype(np.int32)
    return watershed_from_markers(mask, *mk, flood_fn=flood_fn)


def _remove_small(img, min_size, structure):
    """morphology.remove_small_objects on a bool image: components with fewer than ``min_size`` pixels go."""
    if min_size == 0:
        return img.copy()
    lab, _ = ndi.label(img, structure=structure)
    sizes = np.bincount(lab.ravel())
    with np.errstate(invalid='ignore'):
        small = sizes < min_size
    out = img.copy()
    out[small[lab]] = False
    return out


def clean_image(image):
    """``clean_image``: -> (uint8 0 / 1 image, mean_area float64; NaN without a cell)."""
    img = np.asarray(image) != 0
    _, n = ndi.label(img)                                # connectivity 1
    with np.errstate(divide='ignore', invalid='ignore'):
        mean_area = np.float64(np.float32(img.sum())) / np.float64(n)
    thr = mean_area / 5
    img = _remove_small(img, thr, FULL8)
    img = ~_remove_small(~img, thr, FULL8)               # remove_small_holes: small background components, at the border too
    return img.astype(np.uint8), float(mean_area)


def final_mask(cleaned, nuclei_size_t):
    """src/utils.py:159-162 on ``clean_image``'s output: uint8 0 / 255.  An image of one value divides 0 by 0: NaN -> 0."""
    c = np.asarray(cleaned, np.uint8)
    if c.min() == c.max():
        return np.zeros(c.shape, np.uint8)
    img = _remove_small(c > c.min(), nuclei_size_t, None)
    return (img * 255).astype(np.uint8)


def segment_tail(scores, proposals, mask, min_score, nuclei_size_t):
    """Everything behind the network at ``resize_scale == 1``: -> uint8 0 / 255."""
    return final_mask(clean_image(watershed(scores, proposals, mask, min_score))[0], nuclei_size_t)
