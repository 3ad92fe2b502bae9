"""References for the six clean-up stages of meta_inference, one at a time (what ``Handle.meta_inference_stages`` runs on the
device), and a table of MUTANTS per stage: small wrong variants of the oracle that the case list of meta_stage_cases.py has to be
able to tell from it (test_meta_stages.py).

``stage(k, img)`` calls the functions of oracle/postproc.py and restates nothing.  The mutants need the oracle's text with one
thing changed, so each stage has one restated variant below whose switches are all off by default; test_meta_stages.py holds the
switched-off variant to ``stage`` on every case, so that a mutant differs from the oracle by its switch alone.

  stage 1, 2   fill_holes(img, 1 | 2)
  stage 3      size_thresh, then ec_band_removal (fused on the device)
  stage 4      nucleus_in_metaphase
  stage 5      merge_comp(img, 1)
  stage 6      merge_comp(img, 2), then img[dilate(img == 3)] = 3
"""
import functools

import numpy as np
from scipy import ndimage as ndi

from oracle import postproc as P

STAGES = (1, 2, 3, 4, 5, 6)


def stage(k, img):
    """Stage k of oracle.postproc.meta_inference on a copy of ``img`` -> uint8."""
    a = np.array(img, dtype=np.int64, copy=True)
    if k in (1, 2):
        P.fill_holes(a, k)
    elif k == 3:
        P.size_thresh(a)
        P.ec_band_removal(a)
    elif k == 4:
        P.nucleus_in_metaphase(a)
    elif k == 5:
        P.merge_comp(a, 1)
    elif k == 6:
        P.merge_comp(a, 2)
        a[ndi.binary_dilation(a == 3, structure=P._CROSS)] = 3
    else:
        raise ValueError('stages are 1..6')
    return a.astype(np.uint8)


def chain(first, last, img):
    """Stages first..last, one after the other."""
    out = np.asarray(img, np.uint8)
    for k in range(first, last + 1):
        out = stage(k, out)
    return out


def kill_mask(img):
    """The oracle's ``kill[nuc]`` of nucleus_in_metaphase: the stage changes nothing but the pixels of the nuclei it erases."""
    return ((np.asarray(img) == 1) & (stage(4, img) == 0)).astype(np.uint8)


# ---- the oracle's intermediates, for the hand cases to assert the branch they are named for --------------------------------
def areas(img, c):
    """Areas of the 8-connected components of class c, in label order."""
    lab, n = P.label8(np.asarray(img) == c)
    return P._areas(lab, n)


def mean_area(img, c):
    return P._mean(areas(img, c))


def centroids(img, c):
    lab, n = P.label8(np.asarray(img) == c)
    return P._centroids(lab, n) if n else (np.zeros(0), np.zeros(0))


def side_counts(img, v=70.0):
    """Per nucleus (label order): the chromosome centroids in the (left, right, bottom, top) half bands, in the oracle's words."""
    cy, cx = centroids(img, 2)
    ny, nx = centroids(img, 1)
    return [(int(np.count_nonzero((cx > x) & (cx < x + v))), int(np.count_nonzero((cx < x) & (cx > x - v))),
             int(np.count_nonzero((cy < y) & (cy > y - v))), int(np.count_nonzero((cy > y) & (cy < y + v)))) for y, x in zip(ny, nx)]


# ---- restated variants with switches ----------------------------------------------------------------------------------------
def _fill_holes(img, c, conn8=False, skip_edge=None):
    bg = img != c
    lab, n = (P.label8 if conn8 else P.label4)(bg)
    edges = dict(top=lab[0, :], bottom=lab[-1, :], left=lab[:, 0], right=lab[:, -1])
    open_ids = np.unique(np.concatenate([v for k, v in edges.items() if k != skip_edge]))
    is_open = np.zeros(n + 1, bool)
    is_open[open_ids] = True
    is_open[0] = False
    img[~is_open[lab]] = c
    return img


def _thresh_band(img, nuc_le=False, chrom_le=False, ec_le=False, relabel_ec=False, band_first=False, erode_border=1):
    def band(img):
        ec = img == 3
        img[ndi.binary_dilation(ec, structure=P._CROSS) ^ ndi.binary_erosion(ec, structure=P._CROSS, border_value=erode_border)] = 0

    if band_first:
        band(img)
    nuc, n_n = P.label8(img == 1)
    chrom, n_c = P.label8(img == 2)
    avg_chrom = P._mean(P._areas(chrom, n_c))
    a_n = P._areas(nuc, n_n)
    kill = np.zeros(n_n + 1, bool)
    kill[1:] = (a_n <= avg_chrom) if nuc_le else (a_n < avg_chrom)
    img[kill[nuc]] = 0
    chrom, n_c = P.label8(img == 2)
    ec, n_e = P.label8(img == 3)
    a_e = P._areas(ec, n_e)
    avg_ec = P._mean(a_e)
    a_c = P._areas(chrom, n_c)
    to_ec = np.zeros(n_c + 1, bool)
    to_ec[1:] = (a_c <= avg_ec) if chrom_le else (a_c < avg_ec)
    img[to_ec[chrom]] = 3
    if relabel_ec:
        ec, n_e = P.label8(img == 3)
        a_e = P._areas(ec, n_e)
    small = np.zeros(n_e + 1, bool)
    small[1:] = (a_e <= P.EC_SIZE_THRESHOLD) if ec_le else (a_e < P.EC_SIZE_THRESHOLD)
    img[small[ec]] = 0
    if not band_first:
        band(img)
    return img


def _nucleus(img, count_ge=False, bound_le=False, v=70.0, min_chrom_count=5):
    chrom, n_c = P.label8(img == 2)
    nuc, n_n = P.label8(img == 1)
    cy, cx = P._centroids(chrom, n_c) if n_c else (np.zeros(0), np.zeros(0))
    ny, nx = P._centroids(nuc, n_n) if n_n else (np.zeros(0), np.zeros(0))
    lt, gt = (np.less_equal, np.greater_equal) if bound_le else (np.less, np.greater)
    over = (lambda n: n >= min_chrom_count) if count_ge else (lambda n: n > min_chrom_count)
    kill = np.zeros(n_n + 1, bool)
    for k in range(n_n):
        left = over(np.count_nonzero((cx > nx[k]) & lt(cx, nx[k] + v)))
        right = over(np.count_nonzero((cx < nx[k]) & gt(cx, nx[k] - v)))
        bottom = over(np.count_nonzero((cy < ny[k]) & gt(cy, ny[k] - v)))
        top = over(np.count_nonzero((cy > ny[k]) & lt(cy, ny[k] + v)))
        kill[k + 1] = left and right and bottom and top
    img[kill[nuc]] = 0
    return img


def _merge(img, c, visit_last=False, constant_border=False, restore=True):
    m = 2 if c == 1 else 1
    lifted = img == m
    img[lifted] = 0
    lab, n = ndi.label(img, structure=P._FULL)
    has_c = np.zeros(n + 1, bool)
    has_c[np.unique(lab[img == c])] = True
    has_c[0] = False
    if n >= 1 and not visit_last:
        has_c[n] = False
    img[has_c[lab]] = c
    kw = dict(mode='constant', cval=0) if constant_border else {}
    opened = ndi.grey_dilation(ndi.grey_erosion(img, footprint=P._CROSS, **kw), footprint=P._CROSS, **kw)
    img[opened == c] = c
    if restore:
        img[lifted] = m
    return img


def _merge2_dilate(img, final='cross', **kw):
    _merge(img, 2, **kw)
    if final != 'none':
        img[ndi.binary_dilation(img == 3, structure=P._CROSS if final == 'cross' else P._FULL)] = 3
    return img


def _variant(fn, *args, **kw):
    def run(img):
        return fn(np.array(img, dtype=np.int64, copy=True), *args, **kw).astype(np.uint8)
    return run


# the restated variant of every stage with every switch off: equal to stage(k, .) (test_meta_stages.py)
UNMUTATED = {1: _variant(_fill_holes, 1), 2: _variant(_fill_holes, 2), 3: _variant(_thresh_band), 4: _variant(_nucleus),
             5: _variant(_merge, 1), 6: _variant(_merge2_dilate)}


def _fill_mutants(c):
    out = {'background_8_connected': _variant(_fill_holes, c, conn8=True)}
    for edge in ('top', 'bottom', 'left', 'right'):
        out['ignores_%s_edge' % edge] = _variant(_fill_holes, c, skip_edge=edge)
    return out


def _merge_mutants(fn, *args):
    return {'last_component_visited': _variant(fn, *args, visit_last=True),
            'opening_constant_border': _variant(fn, *args, constant_border=True),
            'lifted_class_not_restored': _variant(fn, *args, restore=False)}


MUTANTS = {
    1: _fill_mutants(1),
    2: _fill_mutants(2),
    3: {'erosion_border_0': _variant(_thresh_band, erode_border=0),
        'nucleus_area_le_mean': _variant(_thresh_band, nuc_le=True),
        'chromosome_area_le_mean': _variant(_thresh_band, chrom_le=True),
        'ec_area_le_15': _variant(_thresh_band, ec_le=True),
        'ec_relabelled_after_reassignment': _variant(_thresh_band, relabel_ec=True),
        'band_before_size_thresh': _variant(_thresh_band, band_first=True)},
    4: {'count_ge': _variant(_nucleus, count_ge=True),
        'bound_70_le': _variant(_nucleus, bound_le=True)},
    5: _merge_mutants(_merge, 1),
    6: dict(_merge_mutants(_merge2_dilate),
            final_dilation_dropped=_variant(_merge2_dilate, final='none'),
            final_dilation_8_connected=_variant(_merge2_dilate, final='full')),
}


@functools.lru_cache(maxsize=None)
def mutant_names():
    return [(k, name) for k in STAGES for name in MUTANTS[k]]
