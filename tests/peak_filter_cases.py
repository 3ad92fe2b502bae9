"""Inputs of tests/test_peak_filter.py, tests/test_gpu_peak_filter.py and tools/fuzz_stat_fish.py --asymmetric: cases that read the
one floating-point decision of stat_fish, ``coefficient > normal_threshold`` (fs_threshold_body, csrc/fishspot_kernels.hip), bit by
bit.  Generators only, not a test module.

A "direct" case has ``min_cc_size = 1`` (the cleaned mask is the thresholded mask), a label map that is 1 everywhere and intensity
thresholds of -1 (every pixel passes the gate), so the mask that comes back IS the filter's bit - except on the channel's maximum,
which is a centre whatever the filter says (src/stat_fish.py:82): every generator here puts the one 255 of a channel on a known
pixel, and every expectation sets that pixel on.

  1. one_tap: w zero but w[a, b] = 1; the coefficient is the channel shifted by (a - r, b - r) with zero fill: expected by slicing.
  2. asymmetric: K x K standard-normal weights on the scenes of tests/stat_fish_cases.py, threshold between the two middle
     coefficients of the deciding pixels; a seed is taken only when the oracle counts no pixel inside its 2 B band.
  3. integer: integer weights up to 2^40 on uint8 pixels: every partial sum of every order is an integer below 2^53, so every
     correct float64 evaluation is exact; expected from Python integers; thresholds ON a coefficient and one ulp below it.
  4. band: thresholds 3 B below and above a Gaussian coefficient (B: the oracle's derived bound at that pixel).
  5. non-finite taps: +inf, -inf, NaN; -0.0 and the smallest subnormal inside an asymmetric kernel.
"""
import functools

import numpy as np
from scipy import ndimage

import stat_fish_cases as cases
import stat_fish_ref as ref

PROBES = (1, 0)                                              # probe 0 reads img[..., 1], probe 1 reads img[..., 0]
SIZES = ((33, 130), (16, 64), (17, 65), (5, 7), (1, 200), (200, 1))      # around the 64 x 16 tile of the kernel
ONE_TAP_K = (3, 7, 63)
ONE_TAP_T = 127.5
INF_TAP_T = -1.0
ASYM_K = (3, 7, 15, 23)
ASYM_SIZES = ((65, 63), (33, 130), (40, 70), (17, 65), (50, 129))
ASYM_SEED0 = 7000
N_ASYM = 12
INT_K = (3, 5)
INT_SIZE = (20, 70)                                          # crosses a tile column (64) and a tile row (16)
BAND_KERNELS = ((7, 3.0), (23, 0.9))
BAND_SIZE = (40, 70)
BAND_SEED = 7100
N_BAND = 16


# ---- building blocks --------------------------------------------------------------------------------------------------------------
def channel(rng, H, W, zeros=0.0):
    """Uniform 0..254 with one 255 on a known pixel -> (uint8 (H, W), (y, x) of the maximum).  ``zeros``: the share of pixels set to 0."""
    ch = rng.integers(0, 255, (H, W)).astype(np.uint8)
    if zeros:
        ch[rng.random((H, W)) < zeros] = 0
    peak = (int(rng.integers(0, H)), int(rng.integers(0, W)))
    ch[peak] = 255
    return ch, peak


def direct(channels, weights, normal, rng=None):
    """The case that shows the filter's bit of two probe channels (see the module's text)."""
    H, W = channels[0].shape
    img = np.zeros((H, W, 3), np.uint8)
    if rng is not None:
        img[..., 2] = rng.integers(0, 256, (H, W))           # the channel no probe reads
    for c, ch in zip(PROBES, channels):
        img[..., c] = ch
    return cases._case(img, np.ones((H, W), np.int32), PROBES, weights, normal, (-1.0, -1.0), 1, 1)


def made_direct(case):
    """A scene of stat_fish_cases with the direct settings: its image (three channels of it), kernel and threshold."""
    img = np.ascontiguousarray(case['img'][..., :3])
    return cases._case(img, np.ones(img.shape[:2], np.int32), case['probes'], case['weights'], case['normal'],
                       (-1.0,) * len(case['probes']), 1, 1)


def shifted(ch, dy, dx):
    """out[y, x] = ch[y + dy, x + dx], 0 where that lies outside: by slicing alone."""
    H, W = ch.shape
    out = np.zeros_like(ch)
    y0, y1 = max(0, -dy), min(H, H - dy)
    x0, x1 = max(0, -dx), min(W, W - dx)
    if y0 < y1 and x0 < x1:
        out[y0:y1, x0:x1] = ch[y0 + dy:y1 + dy, x0 + dx:x1 + dx]
    return out


def with_peaks(on, peaks):
    """list of bool (H, W) per probe + the maxima -> uint8 (H, W, n_probe) 0 / 255 with every maximum on."""
    out = np.stack(on, axis=-1).copy()
    for j, p in enumerate(peaks):
        out[p + (j,)] = True
    return out.astype(np.uint8) * np.uint8(255)


def expected_outputs(case, masks):
    """(records, masks, boundaries) of a direct case from its masks alone: one cell that is the whole image, nothing cleaned."""
    img = case['img']
    H, W = img.shape[:2]
    assert (case['seg'] == 1).all() and case['min_cc'] == 1
    rec = np.zeros((1, ref.N_FIELDS), np.int64)
    rec[0, :4] = 1, H * W, W * (H * (H - 1) // 2), H * (W * (W - 1) // 2)
    on = [masks[..., j] != 0 for j in range(masks.shape[2])]
    for j, c in enumerate(case['probes']):
        raw = img[..., c].astype(np.int64)
        rec[0, 4 + 5 * j:9 + 5 * j] = on[j].sum(), ndimage.label(on[j])[1], raw.sum(), np.count_nonzero(raw), raw.max()
    if len(on) >= 2:
        rec[0, 19:21] = (on[0] & on[1]).sum(), ndimage.label(on[0] & on[1])[1]
    return rec, masks, ref.boundaries(case['seg'], case['line'])


def deciding(case):
    """Per probe the pixels whose bit the filter decides: inside a cell, above the intensity threshold, not the maximum."""
    out = []
    for c, it in zip(case['probes'], case['ithr']):
        ch = case['img'][..., c]
        top = int(ch.max())
        out.append((ch.astype(np.float64) > it) & (case['seg'] > 0) & ~((ch == top) & bool(top)))
    return out


def coefficients(case):
    return [ref.correlate(case['img'][..., c], case['weights']) for c in case['probes']]


def ambiguous(case):
    return ref.thresholded(case['img'], case['probes'], ref.ranks(case['seg'])[0], case['weights'], case['normal'], case['ithr'])[1]


def flips(w):
    """The three mistakes of a tap index: rows mirrored, columns mirrored, transposed (both mirrors = a convolution)."""
    return {'rows': np.ascontiguousarray(w[::-1]), 'columns': np.ascontiguousarray(w[:, ::-1]), 'transpose': np.ascontiguousarray(w.T),
            'convolution': np.ascontiguousarray(w[::-1, ::-1])}


# ---- 1. one-tap kernels (and 5: the same tap at +inf / -inf) ------------------------------------------------------------------------
def taps(K):
    r = K // 2
    return ((0, 0), (0, K - 1), (K - 1, 0), (K - 1, K - 1), (0, r), (r, 0), (r, K - 1), (K - 1, r), (r, r))


def one_tap(K, tap, size, value=1.0):
    """-> (case, expected masks).  value: 1 (a shift, threshold 127.5), +inf (on where the shifted pixel is non-zero: inf * 0 = NaN is
    not above any threshold, so the zero padding is off) or -inf (nothing but the maxima).  The infinite taps take the threshold
    INF_TAP_T = -1: a sum that left out the taps on zero pixels would give 0 there, which is above it."""
    a, b = tap
    r = K // 2
    rng = np.random.default_rng([K, a, b, size[0], size[1]])
    zeros = 1 / 3 if np.isinf(value) else 0.0
    chans, peaks = zip(*(channel(rng, size[0], size[1], zeros) for _ in PROBES))       # two different channels: a stale tile shows
    w = np.zeros((K, K))
    w[a, b] = value
    moved = [shifted(ch, a - r, b - r) for ch in chans]
    if value == 1.0:
        on = [m > ONE_TAP_T for m in moved]
    elif value > 0:
        on = [m != 0 for m in moved]
    else:
        on = [np.zeros(size, bool) for _ in moved]
    return direct(chans, w, ONE_TAP_T if value == 1.0 else INF_TAP_T, rng), with_peaks(on, peaks)


# ---- 2. a general asymmetric kernel ----------------------------------------------------------------------------------------------------
def asymmetric_kernel(K, seed):
    return np.random.default_rng([K, seed, 2]).standard_normal((K, K))


def middle_threshold(case):
    """The median coefficient of the deciding pixels, taken between two neighbouring coefficients so that none sits on it."""
    dec = deciding(case)
    c = np.sort(np.concatenate([co[d] for co, d in zip(coefficients(case), dec)]))
    c = c[np.isfinite(c)]
    if len(c) < 2:
        return 0.0
    return float((c[len(c) // 2 - 1] + c[len(c) // 2]) / 2)


def asymmetric(case, seed, K=None):
    """``case`` with its kernel replaced by the asymmetric one of ``seed`` (K: the case's own unless given) and the middle threshold."""
    new = dict(case)
    new['weights'] = asymmetric_kernel(case['weights'].shape[0] if K is None else K, seed)
    new['normal'] = middle_threshold(new)
    return new


@functools.lru_cache(maxsize=None)
def asymmetric_cases():
    """-> (the N_ASYM accepted cases, three per K, seeds tried).  Seeds are walked from ASYM_SEED0; the scene modes with a saturated or
    an all-zero channel or without nuclei (seed % 9 in 5, 6, 8: nothing for the filter to decide) are passed over and not counted; a
    seed is refused when the oracle counts a pixel inside the 2 B band.  Cases 0-3 and 8-11 are direct, 4-7 keep the scene's own
    cells, intensity thresholds and min_cc_size."""
    accepted, tried, seed = [], 0, ASYM_SEED0
    while len(accepted) < N_ASYM:
        seed += 1
        if seed % 9 in (5, 6, 8):
            continue
        K = ASYM_K[len(accepted) % len(ASYM_K)]
        case = cases.scene(seed, size=ASYM_SIZES[seed % len(ASYM_SIZES)], K=K, n_probe=2)
        case = cases._case(case['img'][..., :3], case['seg'], case['probes'], case['weights'], case['normal'], case['ithr'],
                           case['min_cc'], case['line'])
        if len(accepted) // len(ASYM_K) != 1:
            case = made_direct(case)
        case = asymmetric(case, seed)
        tried += 1
        if ambiguous(case) == 0:
            accepted.append(case)
    return tuple(accepted), tried


# ---- 3. exact-integer weights ----------------------------------------------------------------------------------------------------------
def exact_coefficients(ch, w):
    """The correlation in Python integers -> object array (H, W) of int."""
    K = w.shape[0]
    r = K // 2
    H, W = ch.shape
    pad = np.zeros((H + 2 * r, W + 2 * r), object)
    pad[r:r + H, r:r + W] = ch.astype(object)
    out = np.zeros((H, W), object)
    for ky in range(K):
        for kx in range(K):
            assert float(w[ky, kx]).is_integer()
            out = out + int(w[ky, kx]) * pad[ky:ky + H, kx:kx + W]
    assert all(type(v) is int for v in out.flat)
    return out


def _exact_masks(exact, peaks, t):
    """Python's int > float comparison is exact."""
    return with_peaks([np.array([[v > t for v in row] for row in e], bool) for e in exact], peaks)


def _integer_calls(chans, peaks, w, targets, below, rng=None):
    """For each target (probe, y, x) with exact coefficient c: the case at threshold c (the target is off: the comparison is strict)
    and at ``below(c)`` (on) -> list of (case, expected masks, (probe, y, x), whether the target is on)."""
    exact = [exact_coefficients(ch, w) for ch in chans]
    base = direct(chans, w, 0.0, rng)
    calls = []
    for j, y, x in targets:
        c = exact[j][y, x]
        assert float(c) == c
        for t, on in ((float(c), False), (float(below(c)), True)):
            case = dict(base)
            case['normal'] = t
            calls.append((case, _exact_masks(exact, peaks, t), (j, y, x), on))
    return calls, exact


@functools.lru_cache(maxsize=None)
def integer_calls(K):
    """Weights uniform in [-2^40, 2^40]: 8 deciding pixels with distinct coefficients, columns 63 and 64 among them; thresholds at the
    coefficient and at the float64 just below it."""
    rng = np.random.default_rng([K, 3])
    w = rng.integers(-2 ** 40, 2 ** 40, (K, K), endpoint=True).astype(np.float64)
    chans, peaks = zip(*(channel(rng, *INT_SIZE) for _ in PROBES))
    spots = [(0, 3, 63), (1, 3, 64), (0, 15, 64), (1, 16, 63), (0, 0, 0), (1, 19, 69), (0, 10, 30), (1, 16, 5)]
    targets = [(j, y, x + (1 if (y, x) == peaks[j] else 0)) for j, y, x in spots]
    calls, exact = _integer_calls(chans, peaks, w, targets, lambda c: np.nextafter(float(c), -np.inf), rng)
    assert len({exact[j][y, x] for j, y, x in targets}) == len(targets)
    return tuple(calls)


@functools.lru_cache(maxsize=None)
def cancellation_calls():
    """K = 3: the eight outer weights are integers of 2^39 .. 2^40 in size that sum to 0, the centre weight is 1.  On a patch whose
    pixels are all 37 but a centre of 1 .. 9, eight terms near 2^45 cancel and the coefficient is the centre's own value.  Thresholds at
    that value c and at c - 1."""
    rng = np.random.default_rng(45)
    while True:
        ring = rng.integers(2 ** 39, 2 ** 40, 7) * rng.choice([-1, 1], 7)
        if 2 ** 39 <= abs(int(ring.sum())) <= 2 ** 40:
            break
    ring = [int(v) for v in ring] + [-int(ring.sum())]
    w = np.array(ring[:4] + [1] + ring[4:], np.float64).reshape(3, 3)
    H, W = INT_SIZE
    chans, peaks = [], []
    for j in range(2):
        ch = rng.integers(0, 255, (H, W)).astype(np.uint8)
        ch[:, :44] = 37
        for y in range(2, H - 2, 4):
            for x in range(2 + j, 40, 4):
                ch[y, x] = 1 + (y // 4 + x // 4 + j) % 9
        peak = (int(rng.integers(0, H)), int(rng.integers(50, W)))
        ch[peak] = 255
        chans.append(ch); peaks.append(peak)
    targets = [(0, 6, 2), (1, 10, 15), (0, 14, 38), (1, 2, 27)]
    calls, exact = _integer_calls(chans, peaks, w, targets, lambda c: c - 1)
    assert all(1 <= exact[j][y, x] <= 9 and exact[j][y, x] == chans[j][y, x] for j, y, x in targets)
    return tuple(calls)


# ---- 4. thresholds one error band from a Gaussian coefficient --------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def band_calls(which):
    """-> (calls, targets tried).  calls: 2 * N_BAND of (case, (probe, y, x), whether the target is on): per target with oracle
    coefficient c and bound B the thresholds c - 3 B (on) and c + 3 B (off).  Any float64 evaluation lies within B of the exact value,
    as does the oracle, so the two are within 2 B of each other; 3 B also keeps the target outside the oracle's own 2 B band.  Half of
    the targets lie on a tile seam (columns 63 / 64, rows 15 / 16 and 31 / 32), and each half is spread over the coefficient range;
    a target is refused, and its neighbour in coefficient order tried, unless no pixel is ambiguous at either threshold."""
    K, sigma = BAND_KERNELS[which]
    base = made_direct(cases.scene(BAND_SEED, size=BAND_SIZE, K=K, n_probe=2))
    base['weights'] = cases.proj_kernel(K, sigma)
    coef, dec = coefficients(base), deciding(base)
    bound = [ref.error_bound(base['img'][..., c], base['weights']) for c in base['probes']]
    yy, xx = np.indices(BAND_SIZE)
    seam = np.isin(xx, (63, 64)) | np.isin(yy, (15, 16, 31, 32))
    calls, used, tried = [], set(), 0
    for k in range(N_BAND):
        j, on_seam = k % 2, (k // 2) % 2 == 0
        ys, xs = np.nonzero(dec[j] & (seam == on_seam) & (bound[j] > 0))
        order = np.argsort(coef[j][ys, xs], kind='stable')
        at = (2 * (k // 4) + 1) * len(order) // (2 * (N_BAND // 4))
        while True:
            y, x = int(ys[order[at]]), int(xs[order[at]])
            at += 1
            if (j, y, x) in used:
                continue
            tried += 1
            c, B = float(coef[j][y, x]), float(bound[j][y, x])
            pair = []
            for t, on in ((c - 3 * B, True), (c + 3 * B, False)):
                case = dict(base)
                case['normal'] = t
                pair.append((case, (j, y, x), on))
            if all(ambiguous(p[0]) == 0 for p in pair):
                used.add((j, y, x))
                calls += pair
                break
    return tuple(calls), tried


# ---- 5. non-finite and odd taps ----------------------------------------------------------------------------------------------------------
def nan_corner(K, size=(33, 130)):
    """An asymmetric kernel with NaN in one corner: every sum holds that tap (times a pixel or times the padding's 0), so nothing is on
    but the maxima."""
    rng = np.random.default_rng([K, 5])
    chans, peaks = zip(*(channel(rng, *size, 1 / 3) for _ in PROBES))
    w = asymmetric_kernel(K, 5)
    w[K - 1, 0] = np.nan
    return direct(chans, w, -1e300, rng), with_peaks([np.zeros(size, bool) for _ in PROBES], peaks)


@functools.lru_cache(maxsize=None)
def odd_tap_cases():
    """The first accepted asymmetric case of K = 3 and of K = 7 with one tap replaced by -0.0 and another by 5e-324 (the threshold is
    taken again; refused and the next case tried if a pixel is ambiguous) -> tuple of cases, exact against the oracle."""
    out = []
    for K in (3, 7):
        for case in asymmetric_cases()[0]:
            if case['weights'].shape[0] != K:
                continue
            new = dict(case)
            w = case['weights'].copy()
            w[0, K - 1] = -0.0
            w[K - 1, 1] = 5e-324
            new['weights'] = w
            new['normal'] = middle_threshold(new)
            if ambiguous(new) == 0:
                out.append(new)
                break
    assert len(out) == 2
    return tuple(out)
