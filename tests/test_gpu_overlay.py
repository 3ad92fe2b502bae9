"""ecseg_overlay (run_overlay in csrc/overlay_kernels.hip) on the device: the nine counts of a ``meta_overlay`` row against the hand
rows and the oracle of tests/overlay_cases.py (oracle/overlay.py with oracle/postproc.py), never against the product's own
Python.  The 12 int64 fields go through ``csvio.overlay_cells`` and every comparison is exact.  ``case_mismatches(gpu, seed)``
is also the check of tools/fuzz_overlay.py; a failing seed of that campaign becomes a case here.

The Python binding takes uint8 images only (``_lib._u8`` refuses every other type; ``make meta_overlay`` converts 16-bit
files with ecseg_u16_to_u8 before the call), so there is no 16-bit case in this module."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import overlay_cases as cases                # noqa: E402
from ecseg_amd import csvio                  # noqa: E402
from oracle import postproc                  # noqa: E402

pytestmark = pytest.mark.gpu
HAND = cases.hand_cases()


def _rows(gpu, labels, rgb, sens, thr):
    """The device's rows of a stack of images (or of one image) as lists of nine cells."""
    out = np.asarray(gpu.overlay(labels, rgb, sens, thr))
    return [csvio.overlay_cells(r) for r in out.reshape(-1, 12)]


def _run(gpu, case):
    return _rows(gpu, case['labels'], case['rgb'], case['sens'], case['thr'])[0]


def mismatches(gpu, case, want=None):
    """-> list of differences between the device's row and ``want`` (the oracle's row when None)."""
    want = cases.oracle_row(case) if want is None else want
    got = _run(gpu, case)
    if cases.same_row(got, want):
        return []
    H, W, C = case['rgb'].shape
    return ['%d x %d x %d, sensitivity %d, threshold %d: device %s, expected %s' % (H, W, C, case['sens'], case['thr'], got, want)]


def case_mismatches(gpu, seed):
    """The fuzz campaign's check of one generated scene: the committed extents on two seeds of three, a random one otherwise."""
    rng = np.random.default_rng(seed + 424243)
    size = None if seed % 3 else (int(rng.integers(1, 201)), int(rng.integers(1, 261)))
    return mismatches(gpu, cases.scene(seed, size=size))


def _check(gpu, case, want=None):
    bad = mismatches(gpu, case, want)
    assert not bad, '; '.join(bad)


# ---- hand cases and seeds -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', sorted(HAND))
def test_hand_written_rows(gpu, name):
    case, want = HAND[name]
    _check(gpu, case, want)
    _check(gpu, case)


def test_committed_seeds(gpu):
    bad = []
    for seed in range(cases.N_SEEDS):
        bad += ['seed %d: %s' % (seed, b) for b in mismatches(gpu, cases.scene(seed))]
    assert not bad, '\n'.join(bad)


@pytest.mark.parametrize('size', cases.EXTENTS)
def test_odd_sizes(gpu, size):
    for seed in range(3):
        _check(gpu, cases.scene(200 + 3 * cases.EXTENTS.index(size) + seed, size=size))


@pytest.mark.parametrize('C', cases.CHANNELS)
def test_sensitivity_threshold_and_channels(gpu, C):
    base = cases.scene(306, size=(96, 160), C=C, sens=85, thr=20)          # mode 5: discs, rings and bytes above 3
    assert (base['labels'] == 2).any() and (base['labels'] == 3).any() and (base['labels'] > 3).any()
    for sens in cases.SENSITIVITIES:
        for thr in cases.THRESHOLDS:
            # the same label map and blob layout; the channel values move with the sensitivity
            _check(gpu, cases.scene(306, size=(96, 160), C=C, sens=sens, thr=thr))


# ---- batches ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n', [1, 3, 8, 9, 19, 70])           # 70: more images than one internal chunk of 64
def test_batches_match_the_oracle_and_the_single_runs(gpu, n):
    labels, rgb, sens, thr = cases.batch(n, (65, 129), thr=5)
    rows = _rows(gpu, labels, rgb, sens, thr)
    assert len(rows) == n
    for i in range(n):
        want = cases.oracle_row(cases._case(labels[i], rgb[i], sens, thr))
        assert cases.same_row(rows[i], want), (i, rows[i], want)
        alone = _rows(gpu, labels[i], rgb[i], sens, thr)[0]
        assert cases.same_row(alone, rows[i]), (i, alone, rows[i])


@pytest.mark.parametrize('order', [(0, 1, 2), (2, 1, 0), (1, 2, 0), (2, 0, 1, 2, 1, 0, 0, 2, 1)])
def test_a_quirk_does_not_leak_into_the_neighbouring_image(gpu, order):
    labels, rgb, sens, thr, want = cases.quirk_batch()
    idx = list(order)
    rows = _rows(gpu, labels[idx], rgb[idx], sens, thr)
    for k, i in enumerate(idx):
        assert cases.same_row(rows[k], want[i]), (k, i, rows[k], want[i])


def test_quirk_images_among_ordinary_scenes(gpu):
    """An all-chromosome, an all-ecDNA and an all-green image between generated scenes of a multi-tile extent."""
    labels, rgb, sens, thr = cases.batch(9, (65, 129), seed0=7100, thr=5)
    labels[2] = 2
    labels[4] = 3
    labels[7] = 0; rgb[7, ..., 1] = 255
    rows = _rows(gpu, labels, rgb, sens, thr)
    wants = [cases.oracle_row(cases._case(labels[i], rgb[i], sens, thr)) for i in range(9)]
    assert wants[2][7] == 0 and wants[4][0] == (1, 0.0) and wants[7][1] == (1, 0.0) and wants[3][7] + wants[3][8] > 0
    for i in range(9):
        assert cases.same_row(rows[i], wants[i]), (i, rows[i], wants[i])


# ---- repeats: the handle's scratch is shared ---------------------------------------------------------------------------------------
def test_two_calls_give_identical_bytes(gpu):
    case = cases.scene(12)
    a = np.asarray(gpu.overlay(case['labels'], case['rgb'], case['sens'], case['thr']))
    b = np.asarray(gpu.overlay(case['labels'], case['rgb'], case['sens'], case['thr']))
    assert a.dtype == np.int64 and a.shape == (12,) and a.tobytes() == b.tobytes()


def test_large_then_one_pixel_then_large(gpu):
    large, tiny = cases.scene(38), cases.scene(13)
    assert large['labels'].shape == (200, 260) and tiny['labels'].shape == (1, 1)
    first = _run(gpu, large)
    _check(gpu, tiny)
    _check(gpu, large)
    assert cases.same_row(_run(gpu, large), first)


def test_overlay_after_count_hsr_and_after_meta_inference(gpu):
    """count_hsr, meta_inference and the overlay use the same scratch images and per-image counters."""
    case = cases.scene(23)                                     # 96 x 160
    other = cases.scene(24)                                    # 150 x 333
    want = cases.oracle_row(case)
    chrom, fish2 = other['labels'] == 2, (other['rgb'][..., 0] > other['sens']) & (other['labels'] != 1)
    assert gpu.count_hsr(chrom, fish2, 3) == postproc.count_HSR(chrom, fish2, 3)
    _check(gpu, case, want)
    post, _ = gpu.meta_inference(np.minimum(other['labels'], 3))
    assert np.array_equal(post, postproc.meta_inference(np.minimum(other['labels'], 3)))
    _check(gpu, case, want)
    chrom = case['labels'] == 2
    assert gpu.count_hsr(chrom, fish2[:96, :160], 1) == postproc.count_HSR(chrom, fish2[:96, :160], 1)
    _check(gpu, case, want)


# ---- refusals ------------------------------------------------------------------------------------------------------------------------
def test_bad_arguments_are_refused_and_leave_the_handle_usable(gpu):
    from ecseg_amd._lib import _ptr
    case, want = HAND['ec_with_red_and_green_on_one_pixel']
    labels, rgb = case['labels'], case['rgb']
    H, W, C = rgb.shape
    out = np.full(12, -7, np.int64)
    one = np.ascontiguousarray(rgb[..., :1])
    for args in ((_ptr(labels), _ptr(one), 1, H, W, 1),                   # C = 1
                 (_ptr(labels), _ptr(rgb), 1, 0, W, C),                   # H = 0
                 (_ptr(labels), _ptr(rgb), 1, H, 0, C),                   # W = 0
                 (_ptr(labels), _ptr(rgb), -1, H, W, C),                  # negative n
                 (None, _ptr(rgb), 1, H, W, C),                           # null pointers with n > 0
                 (_ptr(labels), None, 1, H, W, C)):
        rc = gpu.lib.ecseg_overlay(gpu.h, args[0], args[1], args[2], args[3], args[4], args[5], case['sens'], case['thr'], _ptr(out))
        assert rc == -1 and b'overlay' in gpu.lib.ecseg_last_error(gpu.h), args[2:]
        assert (out == -7).all()
        _check(gpu, case, want)
    rc = gpu.lib.ecseg_overlay(gpu.h, _ptr(labels), _ptr(rgb), 1, H, W, C, case['sens'], case['thr'], None)
    assert rc == -1
    _check(gpu, case, want)
    assert gpu.lib.ecseg_overlay(gpu.h, None, None, 0, H, W, C, case['sens'], case['thr'], None) == 0      # nothing to do
    _check(gpu, case, want)
