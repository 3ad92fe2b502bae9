"""The peak filter of stat_fish on the device - fs_threshold_body (csrc/fishspot_kernels.hip) behind ecseg_fish_spots and, as
fsb_threshold_kernel, behind ecseg_stat_fish_batch - on the cases of tests/peak_filter_cases.py: tap orientation (one-tap and
asymmetric kernels, halo up to K = 63 across tile seams), float64 accumulation (integer weights whose sums are exact, thresholds 3 B
from a Gaussian coefficient), the IEEE rules of non-finite taps on zero pixels and zero padding, and one image of a chunk against
its neighbours' weights and thresholds.  Every comparison is exact and covers records, masks and boundaries.  The expectations
come from slicing, from Python integers, from the IEEE rule or from the oracle tests/stat_fish_ref.py with ``ambiguous == 0``
asserted; tests/test_peak_filter.py (CPU) holds the oracle to the first three and shows what each case excludes."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import peak_filter_cases as pf               # noqa: E402
import stat_fish_cases as cases              # noqa: E402
import stat_fish_ref as ref                  # noqa: E402
from test_gpu_stat_fish import _run, mismatches              # noqa: E402

pytestmark = pytest.mark.gpu


def differences(got, want):
    """(records, masks, boundaries) against the same three -> list of differences"""
    bad = []
    if got[0].shape != want[0].shape or not np.array_equal(got[0], want[0]):
        bad.append('records differ: %s, expected %s' % (got[0].tolist()[:1], want[0].tolist()[:1]))
    if got[1].shape != want[1].shape or not np.array_equal(got[1], want[1]):
        n = [int((got[1][..., j] != want[1][..., j]).sum()) for j in range(want[1].shape[2])] if got[1].shape == want[1].shape else -1
        bad.append('masks differ in %s pixel(s) per probe' % n)
    if not np.array_equal(got[2], want[2]):
        bad.append('boundaries differ in %d pixel(s)' % int((got[2] != want[2]).sum()))
    return bad


def check_masks(gpu, case, masks, what):
    """A direct case against the masks expected for it (records and boundaries follow from them)."""
    bad = differences(_run(gpu, case), pf.expected_outputs(case, masks))
    assert not bad, '%s: %s' % (what, '; '.join(bad))


def check_oracle(gpu, case, what):
    bad, ambiguous = mismatches(gpu, case)
    assert ambiguous == 0, '%s holds %d pixel(s) inside the 2 B band: not a committed case' % (what, ambiguous)
    assert not bad, '%s: %s' % (what, '; '.join(bad))


def case_mismatches(gpu, seed):
    """tools/fuzz_stat_fish.py --asymmetric: the scene test_gpu_stat_fish.case_mismatches builds for the seed, with its kernel
    replaced by the asymmetric one and the threshold between its two middle coefficients -> (differences, ambiguous pixels)."""
    rng = np.random.default_rng(seed + 31337)
    size = None if seed % 3 else (int(rng.integers(1, 260)), int(rng.integers(1, 260)))
    case = cases.scene(seed, size=size, n_probe=int(rng.choice([1, 2, 2, 2, 3])))
    return mismatches(gpu, pf.asymmetric(case, seed))


# ---- 1. one-tap kernels: a shift by hand ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('size', pf.SIZES, ids=lambda s: '%dx%d' % s)
@pytest.mark.parametrize('K', pf.ONE_TAP_K)
def test_one_tap_kernel_is_a_shift(gpu, K, size):
    for tap in pf.taps(K):
        case, masks = pf.one_tap(K, tap, size)
        check_masks(gpu, case, masks, 'K = %d, tap %s, %d x %d' % ((K, tap) + size))


# ---- 2. a general asymmetric kernel ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('k', range(pf.N_ASYM))
def test_asymmetric_kernel(gpu, k):
    case = pf.asymmetric_cases()[0][k]
    check_oracle(gpu, case, 'asymmetric case %d (K = %d)' % (k, case['weights'].shape[0]))


# ---- 3. exact-integer weights: float64 or nothing ------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', ['K3', 'K5', 'cancellation'])
def test_integer_weights_decide_on_the_last_bit(gpu, name):
    calls = pf.cancellation_calls() if name == 'cancellation' else pf.integer_calls(int(name[1:]))
    for case, masks, (j, y, x), on in calls:
        assert (masks[y, x, j] == 255) == on
        check_masks(gpu, case, masks, '%s, probe %d pixel (%d, %d), threshold %r (the pixel is %s)' % (name, j, y, x, case['normal'], 'on' if on else 'off'))


# ---- 4. thresholds one error band from a Gaussian coefficient ----------------------------------------------------------------------------
@pytest.mark.parametrize('which', range(len(pf.BAND_KERNELS)))
def test_thresholds_three_bounds_from_a_coefficient(gpu, which):
    want = {}
    for case, (j, y, x), on in pf.band_calls(which)[0]:
        what = 'kernel %s, probe %d pixel (%d, %d), threshold %r' % (pf.BAND_KERNELS[which], j, y, x, case['normal'])
        check_oracle(gpu, case, what)
        thr = _run(gpu, case)[1]
        assert (thr[y, x, j] == 255) == on, what
        want.setdefault((j, y, x), []).append(thr)
    assert all(len(v) == 2 and not np.array_equal(*v) for v in want.values())


# ---- 5. non-finite taps ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('size', [(33, 130), (17, 65), (1, 200)], ids=lambda s: '%dx%d' % s)
@pytest.mark.parametrize('K', [3, 7])
def test_infinite_taps(gpu, K, size):
    for tap in pf.taps(K):
        for value in (np.inf, -np.inf):
            case, masks = pf.one_tap(K, tap, size, value)
            check_masks(gpu, case, masks, 'K = %d, tap %s = %r, %d x %d' % ((K, tap, value) + size))


@pytest.mark.parametrize('K', [3, 7])
def test_nan_corner_tap(gpu, K):
    case, masks = pf.nan_corner(K)
    check_masks(gpu, case, masks, 'K = %d' % K)
    check_oracle(gpu, case, 'K = %d' % K)


def test_signed_zero_and_subnormal_taps(gpu):
    for case in pf.odd_tap_cases():
        check_oracle(gpu, case, 'K = %d' % case['weights'].shape[0])


# ---- 6. the batch path ---------------------------------------------------------------------------------------------------------------------
def _item(case):
    assert case['img'].shape[2] == 3 and len(case['probes']) == 2
    blue = [c for c in range(3) if c not in case['probes']][0]
    return dict(img=case['img'], channels=[blue] + list(case['probes']), labels=case['seg'], weights=case['weights'],
                normal_threshold=case['normal'], intensity_thresholds=list(case['ithr']), min_cc_size=case['min_cc'])


def _packed(gpu, chunk, line):
    """one ecseg_stat_fish_batch call over the cases -> per case (records, masks, boundaries)"""
    prepared = [gpu._stat_fish_item(_item(c)) for c in chunk]
    res = gpu.stat_fish_packed(prepared, line, 4096, want_masks=True, poison=0x5a)
    out, p0, r0, t0 = [], 0, 0, 0
    for case, n in zip(chunk, res['n_cells'].tolist()):
        H, W = case['seg'].shape
        out.append((res['records'][r0:r0 + n].copy(), res['thresholded'][t0:t0 + 2 * H * W].reshape(H, W, 2).copy(),
                    res['boundaries'][p0:p0 + H * W].reshape(H, W).copy()))
        p0 += H * W; r0 += n; t0 += 2 * H * W
    return out


def _batch_chunk():
    """-> (cases, expected masks or None where the oracle is the expectation, index of the integer-weight image, its second call).
    Three images of K = 7, two of K = 3, one of K = 63, no two with the same matrix; image 1's tap is image 0's transposed."""
    asym7 = dict([c for c in pf.asymmetric_cases()[0] if c['weights'].shape[0] == 7][1], line=1)    # (it keeps the scene's cells)
    integer = pf.integer_calls(3)
    chunk = [pf.one_tap(7, (0, 6), (16, 64)), pf.one_tap(7, (6, 0), (17, 65)), (asym7, None), pf.one_tap(3, (2, 1), (1, 200)),
             integer[0][:2], pf.one_tap(63, (0, 62), (33, 130))]
    return [c for c, _ in chunk], [m for _, m in chunk], 4, integer[1][:2]


def test_batch_images_keep_their_own_weights_and_thresholds(gpu):
    chunk, masks, at, (second, second_masks) = _batch_chunk()
    line = 1
    assert sorted(c['weights'].shape[0] for c in chunk) == [3, 3, 7, 7, 7, 63]
    assert all(not np.array_equal(a['weights'], b['weights']) for i, a in enumerate(chunk) for b in chunk[:i])
    assert all(c['line'] == line for c in chunk)
    got = _packed(gpu, chunk, line)
    again = _packed(gpu, chunk[::-1], line)[::-1]
    for k, (case, m) in enumerate(zip(chunk, masks)):
        what = 'image %d' % k
        alone = _run(gpu, case)
        bad = differences(got[k], alone)
        assert not bad, '%s against the image alone: %s' % (what, '; '.join(bad))
        bad = differences(again[k], alone)
        assert not bad, '%s in the reversed chunk: %s' % (what, '; '.join(bad))
        if m is None:
            rec, thr, bnd, ambiguous = ref.records(*cases.args(case))
            assert ambiguous == 0
            want = (rec, thr, bnd)
        else:
            want = pf.expected_outputs(case, m)
        bad = differences(got[k], want)
        assert not bad, '%s against its expectation: %s' % (what, '; '.join(bad))
    # the threshold pair of the integer weights: on the coefficient (off) above, one float64 below it (on) here
    j, y, x = pf.integer_calls(3)[0][2]
    assert got[at][1][y, x, j] == 0 and second['normal'] < chunk[at]['normal'] and np.float32(second['normal']) == np.float32(chunk[at]['normal'])
    chunk2 = list(chunk)
    chunk2[at] = second
    got2 = _packed(gpu, chunk2, line)
    bad = differences(got2[at], pf.expected_outputs(second, second_masks))
    assert not bad and got2[at][1][y, x, j] == 255, '; '.join(bad)
    for k in range(len(chunk)):
        if k != at:
            assert not differences(got2[k], got[k]), 'image %d changed with its neighbour\'s threshold' % k
