"""The cases of tests/peak_filter_cases.py without a GPU: the oracle (tests/stat_fish_ref.py) is held to expectations that do not come
from its ``correlate`` - slicing for the one-tap kernels, Python integers for the integer weights, the IEEE rules for the non-finite
taps -, and every case is shown to tell the contract from the mistakes it is there for: a mirrored or transposed tap index, a
float32 accumulator, float32 weights, skipped zero pixels.  tests/test_gpu_peak_filter.py runs the same cases on the device.

The oracle's band is not defined for infinite weights (B is infinite there, so it counts every pixel); those two cases are held to
the IEEE rule alone, on every pixel.  The integer cases put the threshold ON a coefficient, inside the band on purpose: their
expectation is the integer arithmetic, where nothing is ambiguous.  Everywhere else ``ambiguous == 0`` is asserted."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import peak_filter_cases as pf               # noqa: E402
import stat_fish_cases as cases              # noqa: E402
import stat_fish_ref as ref                  # noqa: E402


def oracle_masks(case, weights=None):
    """The oracle's thresholded masks (min_cc_size = 1 in every direct case: nothing is cleaned) and its ambiguous count."""
    w = case['weights'] if weights is None else weights
    return ref.thresholded(case['img'], case['probes'], ref.ranks(case['seg'])[0], w, case['normal'], case['ithr'])


def masks_from(case, coefficient):
    """The masks of a direct case from the coefficients of a restatement under test (one (H, W) array per probe)."""
    on = []
    for c, co in zip(case['probes'], coefficient):
        ch = case['img'][..., c]
        with np.errstate(invalid='ignore'):
            on.append((co > case['normal']) | (ch == ch.max()))
    return np.stack(on, -1).astype(np.uint8) * np.uint8(255)


def correlate_with(channel, weights, accumulator=np.float64, skip_zero_pixels=False):
    """ref.correlate's sum with the mistakes a rewrite of the kernel could make: a narrower accumulator (the product is formed in
    float64 and the running sum rounded, as ``float sum`` would), taps skipped where the pixel is 0."""
    x = np.asarray(channel, np.float64)
    K = weights.shape[0]
    r = K // 2
    H, W = x.shape
    pad = np.zeros((H + 2 * r, W + 2 * r))
    pad[r:r + H, r:r + W] = x
    out = np.zeros((H, W), accumulator)
    with np.errstate(invalid='ignore', over='ignore'):
        for ky in range(K):
            for kx in range(K):
                px = pad[ky:ky + H, kx:kx + W]
                term = weights[ky, kx] * px
                if skip_zero_pixels:
                    term = np.where(px == 0, 0.0, term)
                out = (out.astype(np.float64) + term).astype(accumulator)
    return out.astype(np.float64)


# ---- the helpers of the case file ----------------------------------------------------------------------------------------------------
def test_shift_by_slicing_on_a_hand_case():
    ch = np.arange(1, 13, dtype=np.uint8).reshape(3, 4)
    assert pf.shifted(ch, 0, 0).tolist() == ch.tolist()
    assert pf.shifted(ch, 1, 0).tolist() == [[5, 6, 7, 8], [9, 10, 11, 12], [0, 0, 0, 0]]
    assert pf.shifted(ch, 0, -1).tolist() == [[0, 1, 2, 3], [0, 5, 6, 7], [0, 9, 10, 11]]
    assert pf.shifted(ch, -2, 3).tolist() == [[0, 0, 0, 0], [0, 0, 0, 0], [4, 0, 0, 0]]
    assert not pf.shifted(ch, 3, 0).any() and not pf.shifted(ch, 0, -4).any()


def test_expected_outputs_are_the_oracles_on_direct_cases():
    """records and boundaries written from the masks alone (one cell, nothing cleaned) = both producers of the oracle"""
    for K, tap, size in ((3, (0, 2), (17, 65)), (7, (6, 3), (33, 130)), (7, (3, 3), (1, 200)), (3, (2, 0), (5, 7))):
        case, masks = pf.one_tap(K, tap, size)
        for producer in (ref.records, ref.loop):
            rec, thr, bnd, amb = producer(*cases.args(case))
            assert amb == 0
            want = pf.expected_outputs(case, masks)
            assert np.array_equal(rec, want[0]) and np.array_equal(thr, want[1]) and np.array_equal(bnd, want[2])
            assert rec[0, 5] > 1 and rec[0, 20] > 1


# ---- 1. one-tap kernels ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('K', pf.ONE_TAP_K)
def test_one_tap_oracle_equals_the_shift_by_slicing(K):
    for size in pf.SIZES:
        for tap in pf.taps(K):
            case, masks = pf.one_tap(K, tap, size)
            assert int(case['weights'].sum()) == 1 and case['weights'][tap] == 1
            for j, c in enumerate(case['probes']):
                assert (case['img'][..., c] == 255).sum() == 1 and masks[..., j][case['img'][..., c] == 255] == 255
            got, amb = oracle_masks(case)
            assert amb == 0
            assert np.array_equal(got, masks), (K, tap, size)


@pytest.mark.parametrize('K', pf.ONE_TAP_K)
def test_one_tap_cases_see_a_mirrored_or_transposed_index(K):
    r = K // 2
    for tap in pf.taps(K):
        a, b = tap
        case, masks = pf.one_tap(K, tap, (33, 130))
        assert 0.3 < (masks != 0).mean() < 0.7 or K == 63     # both outcomes are common (K = 63 leaves 2 of 33 rows for a corner tap)
        moves = {'rows': a != r, 'columns': b != r, 'transpose': a != b, 'convolution': (a, b) != (r, r)}
        for name, w in pf.flips(case['weights']).items():
            (a2,), (b2,) = np.nonzero(w)                     # a one-tap kernel again: the oracle was held to its shift above
            other = pf.with_peaks([pf.shifted(case['img'][..., c], a2 - r, b2 - r) > case['normal'] for c in case['probes']],
                                  [tuple(int(v[0]) for v in np.nonzero(case['img'][..., c] == 255)) for c in case['probes']])
            if K < 63:
                assert np.array_equal(other, oracle_masks(case, w)[0])
            for j in range(2):                               # on either probe
                assert np.array_equal(other[..., j], masks[..., j]) == (not moves[name]), (K, tap, name)
    # the whole window is padding: only the maxima are on
    case, masks = pf.one_tap(63, (0, 0), (5, 7))
    assert (masks != 0).sum() == 2


# ---- 2. a general asymmetric kernel ----------------------------------------------------------------------------------------------------
def test_asymmetric_cases_accept_at_least_three_seeds_in_four():
    accepted, tried = pf.asymmetric_cases()
    assert len(accepted) == pf.N_ASYM and 4 * (tried - len(accepted)) <= tried, tried
    assert sorted(c['weights'].shape[0] for c in accepted) == sorted(pf.ASYM_K * 3)
    assert sum((c['seg'] == 1).all() for c in accepted) == 8


def test_asymmetric_cases_agree_on_both_producers_and_see_every_flip():
    for k, case in enumerate(pf.asymmetric_cases()[0]):
        a = ref.records(*cases.args(case))
        assert a[3] == 0
        if k % 3 == 0:
            b = ref.loop(*cases.args(case))
            assert b[3] == 0 and all(np.array_equal(x, y) for x, y in zip(a[:3], b[:3]))
        got = oracle_masks(case)[0]
        dec = np.stack(pf.deciding(case), -1)
        assert dec.sum() > 200 and 0.3 < (got[dec] != 0).mean() < 0.7, k      # both outcomes are common
        w = case['weights']
        for name, other in pf.flips(w).items():
            assert not np.array_equal(other, w)
            diff = (oracle_masks(case, other)[0] != got).sum()
            assert diff > 20, (k, name, diff)


# ---- 3. exact-integer weights ----------------------------------------------------------------------------------------------------------
def _integer_sets():
    return [pf.integer_calls(K) for K in pf.INT_K] + [pf.cancellation_calls()]


def test_integer_weights_oracle_equals_python_integers():
    for calls in _integer_sets():
        case = calls[0][0]
        w = case['weights']
        assert np.abs(w).max() <= 2 ** 40 and (w == np.rint(w)).all()
        assert w.size * 255 * 2 ** 40 < 2 ** 53             # every partial sum of every order is an integer below 2^53
        for j, c in enumerate(case['probes']):
            exact = pf.exact_coefficients(case['img'][..., c], w)
            got = ref.correlate(case['img'][..., c], w)
            assert all(float(e) == g for e, g in zip(exact.flat, got.flat))
            # another order (columns first, last tap first), also exact
            again = ref.correlate(case['img'][..., c][::-1, ::-1].T, w[::-1, ::-1].T)[::-1, ::-1].T
            assert np.array_equal(again, got)


def test_integer_thresholds_sit_on_the_coefficient_and_one_step_below():
    for k, calls in enumerate(_integer_sets()):
        assert len(calls) == (16, 16, 8)[k]
        for (off, m_off, target, on0), (on, m_on, target1, on1) in zip(calls[0::2], calls[1::2]):
            j, y, x = target
            assert target == target1 and (on0, on1) == (False, True)
            c = pf.exact_coefficients(off['img'][..., off['probes'][j]], off['weights'])[y, x]
            assert off['normal'] == c and on['normal'] < c and (on['normal'] == c - 1 or np.nextafter(on['normal'], np.inf) == c)
            assert m_off[y, x, j] == 0 and m_on[y, x, j] == 255
            assert pf.deciding(off)[j][y, x]
            # the oracle's own float64 sum gives the same masks: exact arithmetic, no band needed
            assert np.array_equal(oracle_masks(off)[0], m_off) and np.array_equal(oracle_masks(on)[0], m_on)
            assert (m_off != m_on).sum() >= 1 and ((m_off != m_on).sum() == 1 or k == 2)


def test_integer_cases_see_a_float32_accumulator_and_float32_weights():
    for k, calls in enumerate(_integer_sets()):
        seen32 = seenw = 0
        case = calls[0][0]
        chans = [case['img'][..., c] for c in case['probes']]
        acc32 = [correlate_with(ch, case['weights'], np.float32) for ch in chans]
        w32 = [ref.correlate(ch, case['weights'].astype(np.float32).astype(np.float64)) for ch in chans]
        for case, masks, _, _ in calls:
            seen32 += not np.array_equal(masks_from(case, acc32), masks)
            seenw += not np.array_equal(masks_from(case, w32), masks)
        assert seen32 >= len(calls) // 2, seen32
        if k != 2:                  # (the cancellation weights differ from float32 values too, but by chance)
            assert seenw >= len(calls) // 2, seenw


def test_cancellation_terms_are_near_2_to_45_and_the_coefficient_is_one_digit():
    calls = pf.cancellation_calls()
    w = calls[0][0]['weights']
    ring = np.delete(w.ravel(), 4)
    assert w[1, 1] == 1 and ring.sum() == 0 and (np.abs(ring) >= 2 ** 39).all() and (np.abs(ring) <= 2 ** 40).all()
    assert 2 ** 44 < np.abs(ring * 37).min() and np.abs(ring * 37).max() < 2 ** 46
    for case, masks, (j, y, x), on in calls:
        ch = case['img'][..., case['probes'][j]]
        assert 1 <= ch[y, x] <= 9 and (np.delete(ch[y - 1:y + 2, x - 1:x + 2].ravel(), 4) == 37).all()
        assert case['normal'] == ch[y, x] - on


# ---- 4. thresholds one error band from a Gaussian coefficient ----------------------------------------------------------------------------
@pytest.mark.parametrize('which', range(len(pf.BAND_KERNELS)))
def test_band_targets(which):
    calls, tried = pf.band_calls(which)
    assert len(calls) == 2 * pf.N_BAND and 4 * (tried - pf.N_BAND) <= tried, tried
    targets = [t for _, t, _ in calls[0::2]]
    assert len(set(targets)) == pf.N_BAND and {t[0] for t in targets} == {0, 1}
    seam = [x in (63, 64) or y in (15, 16, 31, 32) for _, y, x in targets]
    assert sum(seam) == pf.N_BAND // 2
    base = calls[0][0]
    coef = pf.coefficients(base)
    cs = np.array([coef[j][y, x] for j, y, x in targets])
    lo, hi = np.percentile(np.concatenate([c.ravel() for c in coef]), [20, 80])
    assert cs.min() < lo and cs.max() > hi                   # spread over the coefficient range
    acc32 = [correlate_with(base['img'][..., c], base['weights'], np.float32) for c in base['probes']]
    w32 = [ref.correlate(base['img'][..., c], base['weights'].astype(np.float32).astype(np.float64)) for c in base['probes']]
    seen32 = seenw = 0
    for case, (j, y, x), on in calls:
        c = coef[j][y, x]
        B = ref.error_bound(case['img'][..., case['probes'][j]], case['weights'])[y, x]
        assert B > 0 and case['normal'] == (c - 3 * B if on else c + 3 * B) and case['normal'] != c
        got, amb = oracle_masks(case)
        assert amb == 0 and (got[y, x, j] == 255) == on
        assert pf.deciding(case)[j][y, x]
        seen32 += not np.array_equal(masks_from(case, acc32), got)
        seenw += not np.array_equal(masks_from(case, w32), got)
    assert seen32 >= 1 and seenw >= 1, (seen32, seenw)
    print('kernel %d: a float32 accumulator is seen by %d of %d calls, float32 weights by %d' % (which, seen32, len(calls), seenw))


# ---- 5. non-finite and odd taps ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('K', [3, 7])
def test_infinite_taps_follow_the_ieee_rule(K):
    for size in ((33, 130), (17, 65), (1, 200)):
        for tap in pf.taps(K):
            case, masks = pf.one_tap(K, tap, size, np.inf)
            assert np.array_equal(oracle_masks(case)[0], masks)
            ch = case['img'][..., 1]
            assert 0.2 < (ch == 0).mean() < 0.5                # a third of the channel is zero
            if size[0] > 1:
                assert 0.3 < (masks != 0).mean() < 0.8       # both outcomes
            # a sum that skips zero pixels, padding included, turns the NaNs into +inf
            skipped = [correlate_with(case['img'][..., c], case['weights'], skip_zero_pixels=True) for c in case['probes']]
            assert not np.array_equal(masks_from(case, skipped), masks)
            case, masks = pf.one_tap(K, tap, size, -np.inf)
            assert np.array_equal(oracle_masks(case)[0], masks) and (masks != 0).sum() == 2
            skipped = [correlate_with(case['img'][..., c], case['weights'], skip_zero_pixels=True) for c in case['probes']]
            assert not np.array_equal(masks_from(case, skipped), masks)


@pytest.mark.parametrize('K', [3, 7])
def test_nan_corner_tap_leaves_the_maxima_alone(K):
    case, masks = pf.nan_corner(K)
    got, amb = oracle_masks(case)
    assert amb == 0 and np.array_equal(got, masks) and (masks != 0).sum() == 2
    # without the NaN the threshold of -1e300 lets everything through; skipping zero pixels lets some through
    w = np.nan_to_num(case['weights'])
    assert (oracle_masks(case, w)[0] != 0).all()
    skipped = [correlate_with(case['img'][..., c], case['weights'], skip_zero_pixels=True) for c in case['probes']]
    assert (masks_from(case, skipped) != 0).sum() > 100


def test_signed_zero_and_subnormal_taps():
    out = pf.odd_tap_cases()
    assert [c['weights'].shape[0] for c in out] == [3, 7]
    for case in out:
        w = case['weights']
        K = w.shape[0]
        assert w[0, K - 1] == 0 and np.signbit(w[0, K - 1]) and w[K - 1, 1] == 5e-324 and w[K - 1, 1] > 0
        a = ref.records(*cases.args(case))
        assert a[3] == 0
        dec = np.stack(pf.deciding(case), -1)
        assert 0.3 < (oracle_masks(case)[0][dec] != 0).mean() < 0.7
