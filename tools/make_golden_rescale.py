#!/opt/conda/bin/python3.9
"""Golden vectors of the two ``rescale`` calls of NuSeT's ``nuclei_segment`` (reference src/utils.py:136 and :157-162), taken from
scikit-image 0.18.3 / scipy 1.7.1, the libraries the watershed contract is pinned on.  Build container only, never on the GPU box:

    tools/make_golden_rescale.py                        writes tests/golden/nuset_rescale.npz
    tools/make_golden_rescale.py --campaign 400         compares seeded random cases, stores nothing

``nuclei_segment`` itself cannot be imported (it needs TensorFlow sessions), so the calls are made with its arguments:
``rescale(image, s, anti_aliasing=True)`` (:136), ``rescale(cleaned, 1 / s)`` (:157), the min-max scaling, threshold and
``morphology.remove_small_objects(bool, NUCLEI_SIZE_T)`` (:159-162); ``scipy.ndimage.gaussian_filter`` is called once more on its
own, with the arguments ``resize`` gives it, for the filtered uint8 image.  Per down case k the file holds down_image_k,
down_scale_k, down_filtered_k and down_out_k (float64); per up case k up_mask_k, up_scale_k, up_sizes_k and up_final_k_<T>;
``down_maxdiff`` is the largest |tests/rescale_ref.py - skimage| over all down cases (skimage fits its affine map by SVD, so its
coordinates differ from the exact ones in the last bits).  Only data is stored.

A case with an UNDECIDED pixel is refused: no test may leave a pixel out.  Up: |((v - vmin) / (vmax - vmin)) * 255 - 1| < 1e-9, where
those last bits could decide the mask.  Down: a byte of the filtered image that changes when the weights take libm's ``exp`` in place
of numpy's - on a flat or exactly linear stretch a pass lands on an integer give or take the last bit of a weight, numpy's ``exp``
is not correctly rounded and differs between releases (1.26.4 and 2.2.6 do), so such a byte would pin one interpreter, not the
method (constants and ramps at 0.3 are such cases)."""
import argparse
import math
import os
import sys
import time
import warnings

import numpy as np

warnings.filterwarnings('ignore')
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, '..', 'tests'))
import rescale_cases as rc                                         # noqa: E402
import rescale_ref as rr                                           # noqa: E402

from scipy import ndimage as ndi                                   # noqa: E402
from skimage import morphology                                     # noqa: E402
from skimage.transform import rescale                              # noqa: E402

UNDECIDED = 1e-9


def reference_down(case):
    img, s = case['image'], case['scale']
    out = rescale(img, s, anti_aliasing=True)                                       # :136
    factors = np.asarray(img.shape, dtype=float) / np.asarray(out.shape, dtype=float)
    filtered = ndi.gaussian_filter(img, np.maximum(0, (factors - 1) / 2), cval=0, mode='mirror')      # as resize calls it
    return out, filtered


def libm_weights(f):
    """``rescale_ref.gaussian_weights`` with ``math.exp``."""
    sigma = max(0.0, (float(f) - 1) / 2)
    if not sigma > 1e-15:
        return np.ones(1, np.float64)
    radius = int(4.0 * sigma + 0.5)
    x = np.arange(-radius, radius + 1)
    phi = np.array([math.exp(float(v)) for v in -0.5 / (sigma * sigma) * x ** 2])
    return phi / phi.sum()


def undecided_down(case):
    """Bytes of the filtered image that the last bit of ``exp`` decides."""
    img = case['image']
    oh, ow = rr.out_extent(img.shape, case['scale'])
    other = rr.filter_axis(rr.filter_axis(img, libm_weights(img.shape[0] / oh), 0), libm_weights(img.shape[1] / ow), 1)
    return int((other != rr.rescale_down(img, case['scale'])[1]).sum())


def reference_up(case):
    mw = rescale(case['mask'], case['scale'])                                       # :157
    with np.errstate(all='ignore'):
        t = ((mw - mw.min()) / (mw.max() - mw.min())) * 255                         # :159
        i8 = t.astype(np.uint8)
    i8[i8 > 0] = 255
    fin = {}
    for size in case['sizes']:
        fin[size] = (morphology.remove_small_objects(i8.astype('bool'), size).astype('int') * 255).astype('uint8')
    return fin, int((np.abs(t - 1) < UNDECIDED).sum())


def compare_down(case):
    out, filtered = reference_down(case)
    mine, mine_f = rr.rescale_down(case['image'], case['scale'])
    bad = []
    if mine.shape != out.shape:
        return ['extent %s != %s' % (mine.shape, out.shape)], float('inf'), out, filtered
    if not np.array_equal(mine_f, filtered):
        bad.append('filtered (%d px)' % int((mine_f != filtered).sum()))
    return bad, float(np.abs(mine - out).max()), out, filtered


def compare_up(case):
    fin, undecided = reference_up(case)
    bad = []
    for size, f in fin.items():
        m = rr.rescale_mask_up(case['mask'], case['scale'], size)
        if m.shape != f.shape or not np.array_equal(m, f):
            bad.append('final_%d' % size)
    return bad, undecided, fin


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--campaign', type=int, default=0)
    ap.add_argument('--first-seed', type=int, default=100000)
    a = ap.parse_args()
    if a.campaign:
        t0, failures, skipped, skipped_down, worst = time.time(), [], 0, 0, 0.0
        for seed in range(a.first_seed, a.first_seed + a.campaign):
            down = rc.random_down(seed)
            bad, diff, _, _ = compare_down(down)
            if undecided_down(down):
                skipped_down += 1
            else:
                worst = max(worst, diff)
                if diff > 1e-12:
                    bad.append('down differs by %.3g' % diff)
            up = rc.random_up(seed)
            up_bad, undecided, _ = compare_up(up)
            if undecided:
                skipped += 1                                       # the last bits of skimage's coordinates may decide: not a finding
            else:
                bad += up_bad
            if bad:
                failures.append(seed)
                print('seed %d: %s' % (seed, ', '.join(bad)), flush=True)
        print('campaign: %d down + %d up cases, %d with a difference (the filtered bytes of every down case are compared); left out for an '
              'undecided pixel: %d up cases, and the float64 image of %d down cases; largest down difference %.3g, %.0f s'
              % (a.campaign, a.campaign, len(failures), skipped, skipped_down, worst, time.time() - t0))
        return 1 if failures else 0
    data, maxdiff = {}, 0.0
    downs, ups = rc.down_cases(), rc.up_cases()
    for k, case in enumerate(downs):
        bad, diff, out, filtered = compare_down(case)
        maxdiff = max(maxdiff, diff)
        data['down_image_%d' % k] = case['image']
        data['down_scale_%d' % k] = np.float64(case['scale'])
        data['down_filtered_%d' % k] = filtered
        data['down_out_%d' % k] = out
        print('%-24s %3d x %3d -> %3d x %3d  |restatement - skimage| %.3g  %s' % ((case['name'],) + case['image'].shape + out.shape +
                                                                                  (diff, ', '.join(bad) or 'filtered equal')))
        if bad:
            return 1
        if undecided_down(case):
            print('%s: %d filtered byte(s) decided by the last bit of exp: the case is refused' % (case['name'], undecided_down(case)))
            return 1
    for k, case in enumerate(ups):
        bad, undecided, fin = compare_up(case)
        if undecided:
            print('%s: %d undecided pixel(s): the case is refused' % (case['name'], undecided))
            return 1
        data['up_mask_%d' % k] = case['mask']
        data['up_scale_%d' % k] = np.float64(case['scale'])
        data['up_sizes_%d' % k] = np.asarray(case['sizes'], np.int64)
        for size, f in fin.items():
            data['up_final_%d_%d' % (k, size)] = f
        shape = fin[case['sizes'][0]].shape
        print('%-24s %3d x %3d -> %4d x %4d  foreground %s  %s' % ((case['name'],) + case['mask'].shape + shape +
              (' '.join('%d:%d' % (s, int((f != 0).sum())) for s, f in fin.items()), ', '.join(bad) or 'restatement equal')))
        if bad:
            return 1
    if not maxdiff < 1e-12:
        print('down_maxdiff %.3g is not below 1e-12: the restatement is wrong' % maxdiff)
        return 1
    data['down_names'] = np.array([c['name'] for c in downs])
    data['up_names'] = np.array([c['name'] for c in ups])
    data['down_maxdiff'] = np.float64(maxdiff)
    out = os.path.join(HERE, '..', 'tests', 'golden', 'nuset_rescale.npz')
    np.savez_compressed(out, **data)
    print('%s: %d down and %d up cases, down_maxdiff %.3g, %d bytes' % (os.path.normpath(out), len(downs), len(ups), maxdiff,
                                                                          os.path.getsize(out)))
    return 0


if __name__ == '__main__':
    sys.exit(main())
