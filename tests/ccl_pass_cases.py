"""Inputs and pass descriptions for the tests of one labelling pass (test_ccl_pass.py on the host, test_gpu_ccl_pass.py on the
device).  The images are small - every path of the labelling kernels exists at 2 x 2 tiles of 64 x 32 pixels - and chosen for the
tile geometry; every pattern is built for the label alphabet 0 .. 3 and, through ``as_mask``, as a mask whose non-zero bytes are
4, 8, 252, 1 and 255 (three of them with value & 3 == 0, which only LUT_NONZERO keys)."""
import collections
import functools

import numpy as np

import ccl_pass_ref as ref
from ccl_pass_ref import (AUX_BORDER, AUX_IMAGE, AUX_NONE, AUX_VALUE_EQ, LUT_MULTI, LUT_NONZERO, NEED_LAST, NEED_LISTS, NEED_NCOMP,
                          NEED_NPX, STAT_AREA, STAT_SUMS, TILE_H, TILE_W)

# (1, 1), (1, 130): degenerate; (32, 64): exactly one tile; (33, 65): one pixel into three more tiles; (64, 128): 2 x 2 tiles, all
# of them eligible for the 8-byte pre-passes; (70, 136): W % 8 == 0 with partial tiles right and below; (96, 200): W % 8 == 0 and
# 3 x 4 tiles, one of them interior; (70, 131): W % 8 != 0, no pre-pass anywhere
SHAPES = [(1, 1), (1, 130), (32, 64), (33, 65), (64, 128), (70, 136), (96, 200), (70, 131)]
BATCH_SHAPE = (70, 136)
BATCHES = (1, 3, 8, 9, 17)      # no complete group of 8 images, exactly one, one + 1, two + 1


def _tiles(H, W):
    return -(-H // TILE_H), -(-W // TILE_W)


# ---- patterns: (H, W, seed) -> uint8 labels 0 .. 3 -------------------------------------------------------------------------
def p_empty(H, W, seed):
    return np.zeros((H, W), np.uint8)


def _full(value):
    def make(H, W, seed):
        return np.full((H, W), value, np.uint8)
    return make


def _hole(which, value):
    def make(H, W, seed):
        """All 3 except one pixel of `value`, in the interior / right-edge / bottom-edge / corner tile."""
        ny, nx = _tiles(H, W)
        ty, tx = {'interior': (min(1, ny - 1), min(1, nx - 1)), 'right': (min(1, ny - 1), nx - 1), 'bottom': (ny - 1, min(1, nx - 1)),
                  'corner': (ny - 1, nx - 1)}[which]
        a = np.full((H, W), 3, np.uint8)
        a[min(H - 1, ty * TILE_H + 5 + seed % 3), min(W - 1, tx * TILE_W + 9 + seed % 5)] = value
        return a
    return make


def p_rows(H, W, seed):
    """Runs of exactly 64 lanes: full rows (runs that continue across the chunk border), runs from lane 0, runs up to lane 63,
    and one class per chunk (a run of 64 between two other keys)."""
    a = np.zeros((H, W), np.uint8)
    x = np.arange(W)
    for y in range(H):
        k = (y + seed) % 8
        if k == 0:
            a[y] = 1
        elif k == 2:
            a[y, x % 64 < 40] = 2
        elif k == 4:
            a[y, x % 64 >= 20] = 3
        elif k == 6:
            a[y] = 1 + (x // 64) % 3
    return a


def p_checker(H, W, seed):
    yy, xx = np.indices((H, W))
    return (((yy + xx + seed) % 2) * 2).astype(np.uint8)


def _comb(vertical, spine):
    def make(H, W, seed):
        """Teeth one pixel wide that meet only on the spine: a row (31 | 32) for vertical teeth, a column (63 | 64) for horizontal."""
        a = np.zeros((H, W), np.uint8)
        if vertical:
            a[:, seed % 2::2] = 1
            a[min(spine, H - 1), :] = 1
        else:
            a[seed % 2::2, :] = 1
            a[:, min(spine, W - 1)] = 1
        return a
    return make


def p_spiral(H, W, seed):
    a = np.zeros((H, W), np.uint8)
    pitch = 3
    y0, x0, y1, x1 = 0, 0, H - 1, W - 1
    while y0 <= y1 and x0 <= x1:
        a[y0, x0:x1 + 1] = 1
        a[y0:y1 + 1, x1] = 1
        if y1 - y0 < pitch or x1 - x0 < pitch:
            break
        a[y1, x0 + pitch:x1 + 1] = 1
        a[y0 + pitch:y1 + 1, x0 + pitch] = 1
        y0, x0, y1, x1 = y0 + pitch, x0 + pitch, y1 - pitch, x1 - pitch
    return a * np.uint8(1 + seed % 3)


def _diag(period, sign):
    def make(H, W, seed):
        yy, xx = np.indices((H, W))
        d = yy + sign * xx + seed + W
        return np.where(d % period == 0, 1 + (d // period) % 3, 0).astype(np.uint8)
    return make


def p_rings(H, W, seed):
    """Square rings of classes 1, 2, 3 around the tile corner (31.5, 63.5), two pixels thick with one-pixel holes between them.
    The inner holes are closed; the rings from the fourth on are cut on row 31, so the holes between them reach the outside
    through one-pixel gaps; the second ring is cut on its diagonal corner only (open at 8-connectivity, closed at 4)."""
    yy, xx = np.indices((H, W))
    d = np.maximum(np.abs(2 * yy - 63), np.abs(2 * xx - 127)) // 2
    k = d // 3
    a = np.where((d % 3 != 0) & (d <= 28), 1 + k % 3, 0).astype(np.uint8)
    a[(yy == 31) & (xx < 63) & (k >= 3)] = 0
    a[(31 - yy == d) & (63 - xx == d) & (k == 1)] = 0
    return a


def p_ring_gap(H, W, seed):
    """A class-1 outline whose top edge runs along row 32 with a one-pixel gap at the tile corner pixel (32, 64): its hole is open
    to the border; inside it a closed class-2 outline."""
    a = np.zeros((H, W), np.uint8)

    def outline(y0, y1, x0, x1, v):
        y1, x1 = min(y1, H - 2), min(x1, W - 2)
        if y0 < y1 and x0 < x1:
            a[y0, x0:x1 + 1] = v
            a[y1, x0:x1 + 1] = v
            a[y0:y1 + 1, x0] = v
            a[y0:y1 + 1, x1] = v
    outline(32, 60, 10, 120, 1)
    outline(40, 50, 30, 100, 2)
    if H > 32 and W > 64:
        a[32, 64] = 0
    return a


def p_moat(H, W, seed):
    """A class-1 ring two pixels thick around the rows 30 .. 65 and columns 60 .. 130: the background inside it is an enclosed hole
    that holds the whole tile (1, 1) where the image has one."""
    a = np.zeros((H, W), np.uint8)
    y0, y1, x0, x1 = 28, min(67, H - 2), 58, min(132, W - 2)
    if y1 - y0 > 4 and x1 - x0 > 4:
        a[y0:y1 + 1, x0:x1 + 1] = 1
        a[y0 + 2:y1 - 1, x0 + 2:x1 - 1] = 0
    return a


def p_corner(H, W, seed):
    """A class-3 component whose only border pixel is (H - 1, W - 1), reached over a diagonal step (8-connectivity), and a class-2
    blob away from the border."""
    a = np.zeros((H, W), np.uint8)
    a[H - 1, W - 1] = 3
    if H >= 8 and W >= 8:
        a[H - 2, W - 2] = 3
        a[H - 5:H - 2, W - 5:W - 2] = 3
        a[2:5, 2:6] = 2
    return a


def _noise(density):
    def make(H, W, seed):
        r = np.random.RandomState(1000 + seed)
        return np.where(r.random_sample((H, W)) < density, r.randint(1, 4, (H, W)), 0).astype(np.uint8)
    return make


def p_dirichlet(H, W, seed):
    r = np.random.RandomState(2000 + seed)
    return r.choice(4, size=(H, W), p=r.dirichlet(np.ones(4))).astype(np.uint8)


def p_bytes(H, W, seed):
    """Any byte: the LUTs key on value & 3, LUT_NONZERO on the whole byte."""
    r = np.random.RandomState(3000 + seed)
    return np.where(r.random_sample((H, W)) < 0.5, r.randint(0, 256, (H, W)), 0).astype(np.uint8)


PATTERNS = collections.OrderedDict([('empty', p_empty), ('full_1', _full(1)), ('full_2', _full(2))] +
                                   [('hole_%s_%d' % (w, v), _hole(w, v)) for w, other in (('interior', 1), ('right', 2), ('bottom', 2), ('corner', 1)) for v in (0, other)] +
                                   [('rows', p_rows), ('checker', p_checker), ('comb_v31', _comb(True, 31)), ('comb_v32', _comb(True, 32)),
                                    ('comb_h63', _comb(False, 63)), ('comb_h64', _comb(False, 64)), ('spiral', p_spiral),
                                    ('diag2', _diag(2, 1)), ('diag3', _diag(3, -1)), ('diag4', _diag(4, 1)), ('rings', p_rings),
                                    ('ring_gap', p_ring_gap), ('moat', p_moat), ('corner', p_corner), ('noise02', _noise(0.02)),
                                    ('noise30', _noise(0.3)), ('noise55', _noise(0.55)), ('noise90', _noise(0.9)), ('dirichlet', p_dirichlet), ('bytes', p_bytes)])

_MASK_BYTES = np.array([4, 8, 252, 1, 255], np.uint8)


def as_mask(labels):
    """The same pixels keyed, as a mask: non-zero bytes from 4, 8, 252, 1, 255 by position."""
    yy, xx = np.indices(labels.shape[-2:])
    return np.where(labels != 0, _MASK_BYTES[(3 * yy + 5 * xx + labels) % 5], 0).astype(np.uint8)


Case = collections.namedtuple('Case', 'name names labels mask aux')     # stacks (n, H, W); names: the pattern of every image


@functools.lru_cache(maxsize=None)
def cases():
    """Every pattern at every shape: one batch per shape (31 images: three groups of 8 and 7 more), except that BATCH_SHAPE is dealt
    over batches of 1, 3, 8, 9 and 17 images, the last slots filled with further seeds of the random patterns.  The images of a
    batch all differ.  aux: seeded bytes 0 .. 31 for AUX_IMAGE."""
    out = []
    names = list(PATTERNS)

    def batch(tag, shape, picks):
        H, W = shape
        labels = np.stack([PATTERNS[n](H, W, seed) for n, seed in picks])
        aux = np.random.RandomState(len(out)).randint(0, 32, labels.shape).astype(np.uint8)
        for a in (labels, aux):
            a.setflags(write=False)
        mask = as_mask(labels)
        mask.setflags(write=False)
        out.append(Case('%s_%dx%d_n%d' % (tag, H, W, len(picks)), [n for n, _ in picks], labels, mask, aux))
    for shape in SHAPES:
        if shape == BATCH_SHAPE:
            extra = ['noise30', 'dirichlet', 'noise55', 'noise02', 'dirichlet', 'noise90', 'noise30']
            picks = [(n, k) for k, n in enumerate(names)] + [(n, 100 + k) for k, n in enumerate(extra)]
            assert len(picks) == sum(BATCHES)
            at = 0
            for nb in BATCHES:
                batch('batch', shape, picks[at:at + nb])
                at += nb
        else:
            batch('all', shape, [(n, k) for k, n in enumerate(names)])
    return tuple(out)


def single_bit_aux(comp):
    """An aux image with one bit (of 0 .. 4, by component) set on a single pixel per component: its last pixel in raster order."""
    flat = comp.ravel()
    aux = np.zeros(flat.size, np.uint8)
    ids, last = np.unique(flat[::-1], return_index=True)
    for c, k in zip(ids, last):
        if c > 0:
            aux[flat.size - 1 - k] = 1 << (int(c) % 5)
    return aux.reshape(comp.shape)


# ---- passes ---------------------------------------------------------------------------------------------------------------
Mode = collections.namedtuple('Mode', 'name src lut conn stat aux_mode aux_c need count_only sparse allow_full')


def _mode(name, src, lut, conn, stat=0, aux_mode=AUX_NONE, aux_c=0, need=0, count_only=False, sparse=False, allow_full=False):
    return Mode(name, src, lut, conn, stat, aux_mode, aux_c, need, count_only, sparse, allow_full)


# every CclPass a driver of csrc/meta_inference_kernels.hip, ccl_kernels.hip or overlay_kernels.hip builds, verbatim (src: the label images or their mask variant)
DRIVER_MODES = [
    _mode('fill_holes_1', 'labels', ref.lut_ne(1), 4, 0, AUX_BORDER, sparse=True, allow_full=True),
    _mode('fill_holes_2', 'labels', ref.lut_ne(2), 4, 0, AUX_BORDER, sparse=True, allow_full=True),
    _mode('size_thresh', 'labels', LUT_MULTI, 8, STAT_AREA, need=NEED_NCOMP | NEED_NPX, sparse=True),
    _mode('nucleus_lists', 'labels', LUT_MULTI, 8, STAT_AREA | STAT_SUMS, need=NEED_LISTS, sparse=True),
    _mode('merge_comp_1', 'labels', ref.lut_nonzero_except(2), 8, 0, AUX_VALUE_EQ, 1, need=NEED_LAST, sparse=True),
    _mode('merge_comp_2', 'labels', ref.lut_nonzero_except(1), 8, 0, AUX_VALUE_EQ, 2, need=NEED_LAST, sparse=True),
    _mode('count_ec', 'labels', ref.lut_eq(3), 8, need=NEED_NCOMP | NEED_NPX, count_only=True, sparse=True),
    _mode('count_cc', 'mask', LUT_NONZERO, 8, need=NEED_NCOMP | NEED_NPX, count_only=True, sparse=True),
    _mode('ccl_labels_4', 'mask', LUT_NONZERO, 4),
    _mode('ccl_labels_8', 'mask', LUT_NONZERO, 8),
    _mode('coloc__hsr_chrom', 'mask', LUT_NONZERO, 8, 0, AUX_IMAGE, need=NEED_NPX),            # run_count_coloc; run_count_hsr's second pass
    _mode('hsr_size__overlay_hsr', 'mask', LUT_NONZERO, 4, STAT_AREA),                           # run_count_hsr's first pass; run_overlay's two
    _mode('overlay_chrom_ec', 'labels', 0x03020000, 8, 0, AUX_IMAGE, need=NEED_NCOMP | NEED_NPX),
    _mode('overlay_a', 'mask', LUT_NONZERO, 8, 0, AUX_IMAGE, need=NEED_NCOMP | NEED_NPX),
    _mode('overlay_b', 'mask', LUT_NONZERO, 8, need=NEED_NCOMP | NEED_NPX),
]
# the drivers the list above stands for
DRIVER_PASSES = ('fill_holes_1', 'fill_holes_2', 'size_thresh', 'nucleus_lists', 'merge_comp_1', 'merge_comp_2', 'count_ec', 'count_cc',
                 'ccl_labels_4', 'ccl_labels_8', 'coloc', 'hsr_size', 'hsr_chrom', 'overlay_hsr', 'overlay_chrom_ec', 'overlay_a', 'overlay_b')

CROSS_MODES = [_mode('x_c%d_s%d_a%d_%s' % (conn, stat, aux_mode, 'sparse' if sparse else 'dense'), 'labels', LUT_MULTI, conn, stat,
                     aux_mode, 2, NEED_NCOMP | NEED_NPX | NEED_LAST, sparse=bool(sparse))
               for conn in (4, 8) for stat in (0, STAT_AREA, STAT_AREA | STAT_SUMS)
               for aux_mode in (AUX_NONE, AUX_BORDER, AUX_VALUE_EQ, AUX_IMAGE) for sparse in (0, 1)]
MODES = DRIVER_MODES + CROSS_MODES


def queries_of(mode):
    """The flag queries asked after a pass (none after a count_only pass, which writes no flag words): bit 0 on any key, every key
    with no bit, bits 2 and 4 together, and bit 5, which no pixel can set.  In groups of at most 5, the most one launch answers."""
    if mode.count_only:
        return []
    q = [(0, 1)] + [(k, 0) for k in ref.lut_keys(mode.lut)] + [(0, 0b10100), (0, 0b100000)]
    return [q[i:i + 5] for i in range(0, len(q), 5)]
