"""Named cases for the two ends of the post-processing (tests/stitch_pre_ref.py; the device: ecseg_stitch_stages_debug,
ecseg_preprocess_stages_debug, ecseg_otsu_debug).  Everything is a function of constants and seeds; nothing is drawn at import.

* ``STITCH_NAMES`` / ``make_stitch(name)``: every stitch size with its image count, the tie-risk count of image k built to be ``tie_count(k)`` - a known
  number, different for every image of a batch - and the per-pixel rows (``pixel_rows``) in the core of the 256 x 256 case, with
  channel strides 4 and 8.  ``big_stitch_case()``: 64 images of 257 x 257, past the 16384-workgroup cap and not a multiple of 256.
* ``preprocess_cases()``: extents, channel counts, both sample widths, every 16-bit value once, constants, the two sides of "half of
  the pixels", alternating batches.
* ``otsu_histograms()``: the seeded adversarial set with the hand-made ones in front."""
import itertools
import os

import numpy as np

import stitch_pre_ref as ref                 # (the stitch map: which patch pixel lies behind a canvas pixel)

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
UNUSED = np.float32(7.0)                                     # what the channels from 4 on hold: a winner in any argmax, if it were read

# ---- stitch ---------------------------------------------------------------------------------------------------------------------
# (H, W, images): one window; two starts one pixel apart and an odd px; the square whose right strip :242 drops; the smoke size; cropped
# 255 and 256; cropped 412 = 2 x 206 without a remainder window; an odd px with a remainder window on both axes
STITCH_SIZES = ((256, 256, 2), (257, 257, 3), (300, 300, 2), (300, 462, 3), (305, 306, 2), (462, 256, 2), (463, 300, 2))
STITCH_BATCHES = ((256, 256, 65), (256, 256, 129))           # a thread visits 2 and 3 images; every workgroup lies in one image
BIG_STITCH = (257, 257, 64)                                  # 4 227 136 pixels: past the cap, workgroups across image boundaries
# The 16384 workgroups of that launch take 4 194 304 pixels at a time, so workgroups 0 .. 127 and threads 0 .. 63 of workgroup 128 go on
# from image 0 into image 63.  Zones (lo, hi, n) of image 0 that get near-ties: those workgroups' pixels (flushed inside the loop), and
# both parts of workgroup 128, whose threads 64 .. 255 end in image 0 while its thread 0 ends in image 63
BIG_ZONES = ((0, 32768, 4), (32768, 32832, 2), (32832, 33024, 3))


def _starts(dim):
    q, r = divmod(dim - 50, 206)
    return q + (1 if r else 0)


def n_patches(H, W):
    return _starts(H) * _starts(W)


def tie_count(k):
    """The tie-risk count image k of any batch is built to have: different for every k below 256."""
    return 20 + 5 * k


def _base_patches(H, W, seed):
    """(n_pos, 256, 256, 4) float32 in [0, 1]: quantised values k / 255 with a clear winner everywhere (the two largest 3 or more
    apart), the winner's channel and the values drawn per pixel."""
    rng = np.random.default_rng(seed)
    shape = (n_patches(H, W), 256, 256)
    win = rng.integers(0, 4, shape)
    top = rng.integers(40, 256, shape)
    q = rng.integers(0, 35, shape + (4,))                    # the losers: below 35, the winner 40 or more
    np.put_along_axis(q, win[..., None], top[..., None], axis=-1)
    return (q / 255.0).astype(np.float32)


def _tie_pixels(k, H, W, written, zones=()):
    """The ``tie_count(k)`` flat canvas pixels of image k that become near-ties: 1 to 5 among its first 256 pixels and 1 to 3 among its
    last 256 - where a workgroup of 256 threads that lies across an image boundary sees them, in the image on either side -, ``n`` evenly
    spaced in every zone (lo, hi, n) of flat pixels, the rest drawn from the whole image by seed k.  ``written``: the flat pixels the stitch
    writes, ascending; only those can count."""
    px = H * W
    first, last = written[written < 256], written[written >= px - 256]
    picks = [first[(13 * k + j) % len(first)] for j in range(1 + k % 5)] + [last[(7 * k + j) % len(last)] for j in range(1 + k % 3)]
    for lo, hi, n in zones:
        z = written[(written >= lo) & (written < hi)]
        picks += z[np.arange(n) * (len(z) // n)].tolist()
    picks = np.unique(picks)
    rest = np.random.default_rng(k).choice(np.setdiff1d(written, picks), tie_count(k) - len(picks), replace=False)
    return np.sort(np.concatenate([picks, rest]))


def _with_ties(patches, k, H, W, zones=()):
    """Image k: the base with a block that names the image in the core of the last patch (which every stitch map reads whole: the cores
    are written last, in patch order) and with the patch pixels behind ``_tie_pixels`` turned into near-ties, gap 0 and gap 1 in turns."""
    p = patches.copy()
    p[-1, 100:108, 100:108] = np.float32([0.1, 0.2, 0.3, 0.4])[np.arange(k, k + 4) % 4]      # winner (3 - k) % 4
    m = ref.stitch_map(H, W).reshape(-1)
    c = _tie_pixels(k, H, W, np.flatnonzero(m >= 0), zones)
    a, j = 50 + (c + k) % 200, np.arange(len(c))
    rows = np.stack([a, a - j % 2, np.zeros_like(a), np.full_like(a, 7)], axis=1)
    rows = np.take_along_axis(rows, (np.arange(4)[None, :] + (c % 4)[:, None]) % 4, axis=1)
    p[m[c] >> 16, (m[c] >> 8) & 255, m[c] & 255] = (rows / 255.0).astype(np.float32)
    return p


def _widen(p, stride):
    if stride == 4:
        return p
    out = np.full(p.shape[:-1] + (stride,), UNUSED, np.float32)
    out[..., :4] = p
    return out


def stitch_case(H, W, n_img, stride=4, name=None):
    base = _base_patches(H, W, seed=H * 1000 + W)
    probs = np.concatenate([_with_ties(base, k, H, W) for k in range(n_img)])
    return dict(name=name or 'stitch_%dx%d_n%d_cs%d' % (H, W, n_img, stride), H=H, W=W, n_img=n_img, probs=_widen(probs, stride),
                ties=[tie_count(k) for k in range(n_img)])


def big_stitch_case():
    """64 images of 257 x 257 (256 MiB of probabilities): the base tiled, then the per-image change written into the tiled array."""
    H, W, n = BIG_STITCH
    base = _base_patches(H, W, seed=H * 1000 + W)
    n_pos = len(base)
    probs = np.tile(base, (n, 1, 1, 1))
    for k in range(n):
        probs[k * n_pos:(k + 1) * n_pos] = _with_ties(base, k, H, W, BIG_ZONES if k == 0 else ())
    return dict(name='stitch_257x257_n64_over_the_cap', H=H, W=W, n_img=n, probs=probs, ties=[tie_count(k) for k in range(n)])


def pixel_rows():
    """-> list of (name, (n, 4) float32 rows within [-1, 1])."""
    out = []
    u = lambda q: np.float32(q / 255.0)
    for label, second in (('q_and_q_minus_1', 1), ('q_and_q', 0), ('q_and_q_minus_2', 2)):
        rows = [perm for q in (2, 3, 100, 128, 255) for perm in itertools.permutations((u(q), u(q - second), u(0), u(1) if q > 3 else u(0)))]
        out.append((label, np.array(rows, np.float32)))
    out.append(('all_four_equal', np.array([[v] * 4 for v in (0.0, 0.25, 0.5, 1.0, u(77))], np.float32)))
    out.append(('negative_clip_to_zero', np.array([[-1.0, -0.5, -0.002, 0.0], [-0.3, 0.001, -1.0, -0.0], [-0.5, -0.5, 0.004, 0.002],
                                                   [-1.0, -1.0, -1.0, -1.0], [0.002, -0.9, 0.0, 0.003]], np.float32)))
    out.append(('zero_and_one', np.array(list(itertools.product((0.0, 1.0), repeat=4)), np.float32)))
    out.append(('half_is_the_one_exact_tie_of_rint', np.array([[0.5, u(128), 0, 0], [u(127), 0.5, 0, 0], [u(128), 0, 0.5, 0], [0, 0.5, u(129), 0.5]], np.float32)))
    g = np.load(os.path.join(GOLDEN, 'quant_argmax.npz'), allow_pickle=False)
    out.append(('golden_quant_argmax', g['probs'].astype(np.float32)))
    return out


def pixel_rows_case(stride):
    """One 256 x 256 image whose patch core holds every row of ``pixel_rows`` (206 to a line), zeros elsewhere (zeros: all equal, a tie)."""
    rows = np.concatenate([r for _, r in pixel_rows()])
    assert len(rows) <= 206 * 206 and np.abs(rows).max() <= 1.0
    p = np.zeros((1, 256, 256, 4), np.float32)
    ys, xs = np.divmod(np.arange(len(rows)), 206)
    p[0, 25 + ys, 25 + xs] = rows
    return dict(name='pixel_rows_cs%d' % stride, H=256, W=256, n_img=1, probs=_widen(p, stride), ties=None, rows=rows, at=(25 + ys, 25 + xs))


def _stitch_makers():
    specs = [(H, W, n, 4) for H, W, n in STITCH_SIZES] + [(257, 257, 3, 8), (300, 462, 1, 8), (256, 256, 1, 4)]
    specs += [(H, W, n, 4) for H, W, n in STITCH_BATCHES]
    makers = {'stitch_%dx%d_n%d_cs%d' % s: (lambda s=s: stitch_case(*s)) for s in specs}
    makers.update({'pixel_rows_cs%d' % cs: (lambda cs=cs: pixel_rows_case(cs)) for cs in (4, 8)})
    return makers


STITCH_MAKERS = _stitch_makers()
STITCH_NAMES = list(STITCH_MAKERS)                           # every case but the big one; the arrays are made when a test asks
SMALL_STITCH_NAMES = [n for n in STITCH_NAMES if '_n65_' not in n and '_n129_' not in n]


def make_stitch(name):
    return STITCH_MAKERS[name]()


# ---- meta_preprocess ------------------------------------------------------------------------------------------------------------
PRE_EXTENTS = ((1, 1), (1, 255), (16, 16), (17, 15), (256, 256))


def _channels(gray, C, dtype):
    """(H, W) -> (H, W, C) with the picked content in channel 2 (channel 0 when C == 1) and other content elsewhere."""
    if C == 1:
        return gray[..., None].astype(dtype)
    top = np.iinfo(dtype).max
    out = np.empty(gray.shape + (C,), dtype)
    out[..., 2] = gray
    out[..., 0] = top - gray                                 # the opposite decision
    out[..., 1] = (gray.astype(np.int64) * 3 + 1) % (top + 1)
    if C == 4:
        out[..., 3] = top
    return out


def _blob(H, W, seed, dtype, bright):
    """A few bright (or, for the inverted kind, dark) pixels on a noisy ground: two clear classes at any extent."""
    rng = np.random.default_rng(seed)
    top = np.iinfo(dtype).max
    lo = rng.integers(0, top // 8 + 1, (H, W))
    hi = rng.integers(top - top // 8, top + 1, (H, W))
    fg = rng.random((H, W)) < 0.25
    if H * W > 1:
        fg.flat[0], fg.flat[-1] = True, False                # both classes at every extent above one pixel
    g = np.where(fg, hi, lo)
    return (g if bright else top - g).astype(dtype)


def two_valued(H, W, upper, lo=40, hi=200):
    """(H, W) uint8 with exactly ``upper`` pixels of ``hi``, spread over the image, the rest ``lo``."""
    g = np.full(H * W, lo, np.uint8)
    g[(np.arange(upper) * 7919) % (H * W) if np.gcd(7919, H * W) == 1 else np.arange(upper)] = hi
    assert int((g == hi).sum()) == upper
    return g.reshape(H, W)


def all_u16_values():
    """256 x 256 uint16 holding every value once, in an order that is no ramp."""
    return ((np.arange(65536, dtype=np.int64) * 40503 + 12345) % 65536).astype(np.uint16).reshape(256, 256)


def preprocess_cases():
    """-> list of dict(name, imgs (n, H, W, C) uint8 / uint16)."""
    cs = []
    add = lambda name, imgs: cs.append(dict(name=name, imgs=np.ascontiguousarray(imgs)))
    for (H, W), C, dt in itertools.product(PRE_EXTENTS, (1, 3, 4), (np.uint8, np.uint16)):
        imgs = [_channels(_blob(H, W, 100 * H + W + k, dt, bright=k % 2 == 0), C, dt) for k in range(2)]
        add('extent_%dx%d_c%d_%s' % (H, W, C, np.dtype(dt).name), np.stack(imgs))
    v = all_u16_values()
    add('every_u16_value_c1', v[None, ..., None])
    add('every_u16_value_c3', _channels(v, 3, np.uint16)[None])
    for value in (0, 1, 255):
        add('constant_%d' % value, np.full((1, 16, 16, 1), value, np.uint8))
        add('constant_%d_u16_c3' % value, _channels(np.full((17, 15), value * 257, np.uint16), 3, np.uint16)[None])
    for H, W in ((16, 16), (17, 15), (256, 256)):
        px = H * W
        for label, upper in (('half', px // 2), ('half_plus_1', px // 2 + 1), ('half_rounded_up', (px + 1) // 2)):
            add('two_valued_%dx%d_%s' % (H, W, label), _channels(two_valued(H, W, upper), 3, np.uint8)[None])
    for n in (1, 64, 65, 129):
        imgs = [_channels(_blob(17, 15, 7000 + k, np.uint8, bright=k % 2 == 0), 3, np.uint8) for k in range(n)]
        add('alternating_batch_of_%d' % n, np.stack(imgs))
    return cs


# ---- histograms for Otsu alone --------------------------------------------------------------------------------------------------
HIST_SEED, HIST_DRAWS = 20240611, 3000
INT32_MAX = 2 ** 31 - 1


def _hist(pairs):
    h = np.zeros(256, np.int64)
    for b, v in pairs:
        h[b] += v
    return h


def hand_histograms():
    """-> list of (name, (256) int64): one populated bin; one pixel against many, on both sides of the FLT_EPSILON class-weight skip and
    on it (a class of weight 2^-23 exactly is kept, 10^-6 is kept, 1 / (2^23 + 1) and everything lighter is skipped); everything in
    bins 0 and 255."""
    out = [('single_bin_0', _hist([(0, 4096)])), ('single_bin_255', _hist([(255, 4096)])), ('single_bin_0_one_pixel', _hist([(0, 1)]))]
    for label, many in (('1e6', 10 ** 6), ('2p23_minus_1', 2 ** 23 - 1), ('2p23', 2 ** 23), ('1e7', 10 ** 7), ('1e8', 10 ** 8), ('int32_max_minus_1', INT32_MAX - 1)):
        out.append(('one_pixel_below_%s' % label, _hist([(3, 1), (200, many)])))
        out.append(('one_pixel_above_%s' % label, _hist([(3, many), (200, 1)])))
    out.append(('two_pixels_above_int32_max_minus_2', _hist([(0, INT32_MAX - 2), (255, 2)])))
    for a, b in ((1, 1), (5, 5), (5, 6), (6, 5), (INT32_MAX // 2, INT32_MAX // 2), (INT32_MAX // 2, INT32_MAX // 2 + 1), (INT32_MAX // 2 + 1, INT32_MAX // 2)):
        out.append(('bins_0_and_255_%d_%d' % (a, b), _hist([(0, a), (255, b)])))
    return out


def drawn_histograms(seed=HIST_SEED, draws=HIST_DRAWS):
    """The three families in which two thresholds have (nearly) the same class variance, so that the last bit of sigma picks the winner:
    mirror-symmetric with three peaks, symmetric and sparse, and 2 to 5 populated bins."""
    rng = np.random.default_rng(seed)
    out = []
    for k in range(draws):
        kind = k % 3
        if kind == 0:
            c, d = int(rng.integers(24, 232)), int(rng.integers(2, 20))
            a, b, w = int(rng.integers(1, 5000)), int(rng.integers(1, 5000)), int(rng.integers(0, 3))
            pairs = []
            for j in range(-w, w + 1):
                s = a // (1 + abs(j)) + 1
                pairs += [(c - d + j, s), (c + d - j, s), (c + j, b // (1 + abs(j)) + 1)]
            out.append(('three_peaks_%04d' % k, _hist(pairs)))
        elif kind == 1:
            n, c2 = int(rng.integers(2, 9)), int(rng.integers(60, 451))      # twice the centre: bins b and c2 - b
            lo, hi = max(0, c2 - 255), min(255, c2)
            bins = rng.integers(lo, hi + 1, n)
            vals = rng.integers(1, 2000, n)
            out.append(('symmetric_sparse_%04d' % k, _hist([(int(b), int(v)) for b, v in zip(bins, vals)] +
                                                           [(c2 - int(b), int(v)) for b, v in zip(bins, vals)])))
        elif k % 9 == 2:                                     # 2 to 5 populated bins: anywhere, any counts
            n = int(rng.integers(2, 6))
            bins = rng.choice(256, n, replace=False)
            vals = rng.integers(1, int(rng.choice([4, 50, 100000])), n)
            out.append(('few_bins_%04d' % k, _hist([(int(b), int(v)) for b, v in zip(bins, vals)])))
        elif k % 9 == 5:                                     # 3 to 5 equally spaced bins of one count
            n, step, v = int(rng.integers(3, 6)), int(rng.integers(1, 50)), int(rng.integers(1, 1000))
            b0 = int(rng.integers(0, 256 - step * (n - 1)))
            out.append(('few_bins_%04d' % k, _hist([(b0 + step * i, v) for i in range(n)])))
        else:                                                # 2 to 5 bins mirrored about a centre
            n, c2 = int(rng.integers(2, 6)), int(rng.integers(60, 451))
            lo, hi = max(0, c2 - 255), min(255, c2)
            bins, vals = rng.integers(lo, hi + 1, n // 2), rng.integers(1, 2000, n // 2)
            pairs = [(int(b), int(v)) for b, v in zip(bins, vals)] + [(c2 - int(b), int(v)) for b, v in zip(bins, vals)]
            if n % 2 and c2 % 2 == 0:
                pairs.append((c2 // 2, int(rng.integers(1, 2000))))
            out.append(('few_bins_%04d' % k, _hist(pairs)))
    return out


def otsu_histograms():
    """-> (names, (n, 256) uint32, (n) int64 pixel counts)."""
    both = hand_histograms() + drawn_histograms()
    hs = np.stack([h for _, h in both])
    assert hs.max() <= 2 ** 32 - 1 and hs.sum(axis=1).max() <= INT32_MAX
    return [n for n, _ in both], hs.astype(np.uint32), hs.sum(axis=1).astype(np.int64)
