"""Seeded inputs of the proposal layer for tests/test_nuset.py (restatement against restatement, no GPU) and tests/test_gpu_nuset.py
(device against restatement).  Not a test module.

Every case is chosen so that no decision of a float32 run hangs on a rounding: scores that differ in float64 differ in float32 in
the same order, and every pair decision of the NMS stays clear of the threshold by more than ``nuset_ref.iou_bound``
(tests/test_nuset.py checks both for every case here, so a case that is edited must pass there first).  The seeds of the random
cases were picked by that check.

Beyond the seven hand-made cases of ``ALL``: ``BOUNDARY``, named cases at the sort lengths, NMS extents and filtered fractions at
which the device code takes another path, and ``random_case(seed)`` over ``RANDOM_SEEDS``, the seeded generator that
tools/fuzz_nuset.py walks further."""
import numpy as np

RATIOS = (0.125, 0.25, 0.5, 1.0, 2.0, 4.0, 8.0)
SCALES = (0.5, 1.0, 2.0)
SEED_TOP_K = 1            # (seed 0 leaves one IoU within 1e-5 of the threshold)
BASE_SIZES = (37.5, 11.5, 81.0, 23.25)     # the anchor base sizes of the hand-made cases
MAX_PRE = 8192            # ECSEG_RPN_MAX_PRE_NMS


def ref_anchors(A, base_size):
    """The first ``A`` of the 21 reference anchors of generate_anchors_reference for ``base_size`` (float64, ratio-major)."""
    s, r = np.meshgrid(np.asarray(SCALES), np.asarray(RATIOS))
    s, q = s.reshape(-1)[:A], np.sqrt(r.reshape(-1)[:A])
    h, w = s * q * base_size, s / q * base_size
    return np.stack([-(w - 1) / 2, -(h - 1) / 2, (w - 1) / 2, (h - 1) / 2], axis=-1)


def _case(name, cls, bbox, ref, thr, pre, post, stride=16, im=None):
    fh, fw = cls.shape[:2]
    im_h, im_w = im if im is not None else (fh * stride, fw * stride)
    return dict(name=name, cls=np.ascontiguousarray(cls, np.float32), bbox=np.ascontiguousarray(bbox, np.float32), ref=ref, stride=stride,
                im_h=im_h, im_w=im_w, thr=thr, pre=pre, post=post)


def _random(rng, fh, fw, A, shift, grow):
    """Logits N(0, 2); centres moved by up to ``shift`` anchor extents, log-sizes by up to ``grow``."""
    cls = rng.normal(0.0, 2.0, (fh, fw, 2 * A))
    bbox = rng.uniform(-1.0, 1.0, (fh, fw, A, 4)) * np.array([shift, shift, grow, grow])
    return cls, bbox.reshape(fh, fw, 4 * A)


def small():
    """1. 2 x 3 positions, fewer candidates than pre_nms_top_n; boxes overlap a lot, the NMS removes most."""
    rng = np.random.default_rng(11)
    cls, bbox = _random(rng, 2, 3, 4, 0.3, 0.4)
    return _case('small', cls, bbox, ref_anchors(4, 37.5), 0.3, 100, 20)


def top_k_cut():
    """2. 17 x 17 positions x 21 anchors = 6069 candidates > pre_nms_top_n = 6000: the cut of the top-k."""
    rng = np.random.default_rng(SEED_TOP_K)
    cls, bbox = _random(rng, 17, 17, 21, 1.5, 0.5)
    # 6069 random float32 scores would tie or swap places with their float64 values somewhere: spread them evenly instead,
    # 1 / 6070 apart, in random order
    n = 17 * 17 * 21
    target = (rng.permutation(n) + 0.5) / (n + 1)
    cls = cls.reshape(n, 2)
    cls[:, 1] = cls[:, 0] + np.log(target / (1.0 - target))
    cls = cls.reshape(17, 17, 42)
    return _case('top_k_cut', cls, bbox, ref_anchors(21, 11.5), 0.5, 6000, 800)


def cap():
    """3. 20 x 20 positions x 3 anchors with dw = dh near -3: 1200 boxes of ~3 pixels that overlap nowhere, so the NMS removes
    nothing and stops at post_nms_top_n = 800."""
    rng = np.random.default_rng(13)
    fh = fw = 20
    cls = rng.normal(0.0, 2.0, (fh, fw, 6))
    bbox = np.zeros((fh, fw, 3, 4))
    bbox[..., 0] = (np.arange(3) - 1) * 0.08 + rng.uniform(-0.01, 0.01, (fh, fw, 3))     # 5 pixels apart at 64 pixels of anchor
    bbox[..., 1] = rng.uniform(-0.01, 0.01, (fh, fw, 3))
    bbox[..., 2:] = -3.0 + rng.uniform(-0.05, 0.05, (fh, fw, 3, 2))
    ref = np.tile(np.array([[-31.5, -31.5, 31.5, 31.5]]), (3, 1))
    return _case('cap', cls, bbox.reshape(fh, fw, 12), ref, 0.1, 6000, 800)


def equal_scores():
    """4. Equal scores: every position repeats the same three logit pairs, so scores tie across positions and the lower candidate
    index goes first; the tied boxes of neighbouring positions overlap, so the order decides who survives."""
    fh, fw, A = 3, 4, 3
    cls = np.tile(np.array([0.25, 1.5, -0.5, 0.75, 2.0, 2.0]), (fh, fw, 1))
    bbox = np.zeros((fh, fw, A, 4))
    bbox[..., 2] = np.array([0.0, 0.25, -0.25])
    bbox[..., 3] = np.array([0.0, -0.25, 0.25])
    return _case('equal_scores', cls, bbox.reshape(fh, fw, 4 * A), ref_anchors(3, 81.0), 0.3, 30, 20)


def bad_values():
    """5. One NaN score and one box with dw = -inf (width 0): both dropped, the rest as usual."""
    c = small()
    cls, bbox = c['cls'].copy(), c['bbox'].copy()
    cls[0, 1, 2] = np.nan                                    # candidate (0 * 3 + 1) * 4 + 1
    bbox[1, 0, 4 * 2 + 2] = -np.inf                          # candidate (1 * 3 + 0) * 4 + 2
    return dict(c, name='bad_values', cls=cls, bbox=bbox)


def all_filtered():
    """6. Every candidate fails the filter (dh = -inf, or a NaN score): n_out = 0."""
    c = small()
    cls, bbox = c['cls'].copy(), c['bbox'].copy()
    bbox[..., 3::4] = -np.inf
    cls[0, 0, :] = np.nan
    return dict(c, name='all_filtered', cls=cls, bbox=bbox)


def outside():
    """7. Boxes far outside the image on every side, clipped to its border after the NMS."""
    rng = np.random.default_rng(17)
    cls, bbox = _random(rng, 4, 5, 3, 0.2, 0.3)
    b = bbox.reshape(4, 5, 3, 4)
    b[..., 0] += np.array([-40.0, 0.0, 40.0])                # left of the image, inside, right of it
    b[..., 1] += np.where(np.arange(4) % 2 == 0, -30.0, 30.0)[:, None, None]   # above / below
    b[1, 2, 1, :2] = 0.0                                     # one box stays inside
    return _case('outside', cls, b.reshape(4, 5, 12), ref_anchors(3, 23.25), 0.4, 50, 40)


ALL = (small, top_k_cut, cap, equal_scores, bad_values, all_filtered, outside)


# ---- boundary cases: sort lengths, NMS extents, filtered fractions --------------------------------------------------------------
def _spread(rng, cls, n):
    """Scores spread evenly, 1 / (n + 1) apart, in random order (as ``top_k_cut``): float32 cannot tie or swap them."""
    target = (rng.permutation(n) + 0.5) / (n + 1)
    cls = cls.reshape(n, 2)
    cls[:, 1] = cls[:, 0] + np.log(target / (1.0 - target))
    return cls


PALETTE = np.array([[0.25, 1.5], [-0.5, 0.25], [2.0, 2.0], [1.0, -1.0], [0.0, 3.0]])      # five logit pairs, five distinct scores


def _palette(rng, cls, n):
    """Every candidate draws one of five logit pairs: ties everywhere, broken by the candidate index."""
    cls = cls.reshape(n, 2)
    cls[:] = PALETTE[rng.integers(0, len(PALETTE), n)]
    return cls


def _filter(rng, cls, bbox, n, p_box, p_nan):
    """About ``p_box`` of the candidates get dw or dh = -inf (an empty box), about ``p_nan`` a NaN score: both fail the keep test."""
    cls, bbox = cls.reshape(n, 2), bbox.reshape(n, 4)
    gone = np.flatnonzero(rng.random(n) < p_box)
    bbox[gone, 2 + rng.integers(0, 2, len(gone))] = -np.inf
    cls[rng.random(n) < p_nan, 1] = np.nan
    return cls, bbox


def _sized(name, seed, fh, fw, A, pre, post, scores='spread', p_box=0.0, p_nan=0.0, thr=0.5, base=11.5, shift=1.5, grow=0.5):
    rng = np.random.default_rng(seed)
    n = fh * fw * A
    cls, bbox = _random(rng, fh, fw, A, shift, grow)
    cls = (_spread if scores == 'spread' else _palette)(rng, cls, n)
    if p_box or p_nan:
        cls, bbox = _filter(rng, cls, bbox, n, p_box, p_nan)
    return _case(name, cls.reshape(fh, fw, 2 * A), bbox.reshape(fh, fw, 4 * A), ref_anchors(A, base), thr, pre, post)


# the first seed that nuset_ref.undecided accepts: seed 0 of n4096 leaves an IoU 1.2e-3 inside its bound of the threshold, seed 0
# of ties6069 one 9e-6 inside
SEED_N2047, SEED_N2048, SEED_N2050, SEED_N4096, SEED_N4097, SEED_N21504 = 0, 0, 0, 1, 0, 0
SEED_TIES, SEED_PRE100, SEED_POST5, SEED_FILTERED, SEED_WHOLE = 1, 0, 0, 0, 0


def n2047():
    """23 x 89 x 1 = 2047 candidates: one padding key in the only 2048-key block."""
    return _sized('n2047', SEED_N2047, 23, 89, 1, 6000, 800)


def n2048():
    """32 x 16 x 4 = 2048: no padding key at all, and K = 2048 is a multiple of 64 (no ragged last word of the bit matrix)."""
    return _sized('n2048', SEED_N2048, 32, 16, 4, 6000, 800)


def n2050():
    """25 x 41 x 2 = 2050: sort length 4096 with 2046 padding keys; the one global stride 2048, then the block kernel."""
    return _sized('n2050', SEED_N2050, 25, 41, 2, 6000, 800)


def n4096():
    """32 x 32 x 4 = 4096: sort length 4096, full."""
    return _sized('n4096', SEED_N4096, 32, 32, 4, 6000, 800)


def n4097():
    """17 x 241 x 1 = 4097: sort length 8192, half of it padding."""
    return _sized('n4097', SEED_N4097, 17, 241, 1, 4097, 800)


def n21504():
    """32 x 32 x 21 = 21504: sort length 32768 (global strides 16384 .. 2048), K = 8192 = the largest pre_nms_top_n, 128 words a row:
    the second trip of the sweep's 64-word loop over a full row."""
    return _sized('n21504', SEED_N21504, 32, 32, 21, MAX_PRE, 800)


def ties6069():
    """17 x 17 x 21 with the five-pair palette: runs of ~1200 equal scores across 2048-key blocks and global strides."""
    return _sized('ties6069', SEED_TIES, 17, 17, 21, 6000, 800, scores='palette')


def pre100():
    """17 x 17 x 21, pre_nms_top_n = 100: the cut falls far below ``kept``, in the middle of a sorted block; K = 100."""
    return _sized('pre100', SEED_PRE100, 17, 17, 21, 100, 800)


def post5():
    """17 x 17 x 21, post_nms_top_n = 5: the cap ends the sweep after a handful of picks."""
    return _sized('post5', SEED_POST5, 17, 17, 21, 6000, 5)


def filtered6069():
    """17 x 17 x 21 with about a third of the candidates filtered: 0 < kept < K, so thousands of all-ones keys lie inside [kept, K)."""
    return _sized('filtered6069', SEED_FILTERED, 17, 17, 21, 6000, 800, p_box=0.32, p_nan=0.02)


def whole_order():
    """64 x 64 x 2 = 8192 boxes of ~3 pixels, two per 16-pixel cell and 8 pixels apart, that touch nowhere (built like ``cap``): the
    NMS removes nothing, post_nms_top_n = 8192 caps nothing, and the 8192 returned indices are the device's ENTIRE sorted order."""
    rng = np.random.default_rng(SEED_WHOLE)
    fh = fw = 64
    n = fh * fw * 2
    cls = _spread(rng, rng.normal(0.0, 2.0, (fh, fw, 4)), n)
    bbox = np.zeros((fh, fw, 2, 4))
    bbox[..., 0] = (np.arange(2) - 0.5) * 0.125 + rng.uniform(-0.01, 0.01, (fh, fw, 2))     # +-4 pixels at 64 pixels of anchor
    bbox[..., 1] = rng.uniform(-0.01, 0.01, (fh, fw, 2))
    bbox[..., 2:] = -3.0 + rng.uniform(-0.05, 0.05, (fh, fw, 2, 2))
    ref = np.tile(np.array([[-31.5, -31.5, 31.5, 31.5]]), (2, 1))
    return _case('whole_order', cls.reshape(fh, fw, 4), bbox.reshape(fh, fw, 8), ref, 0.5, MAX_PRE, MAX_PRE)


BOUNDARY = (n2047, n2048, n2050, n4096, n4097, n21504, ties6069, pre100, post5, filtered6069, whole_order)


# ---- the seeded generator ---------------------------------------------------------------------------------------------------
ANCHOR_COUNTS = (1, 3, 4, 9, 21)
SCORE_MODES = ('spread', 'palette', 'spread_filtered')
RANDOM_SEEDS = range(48)
RANDOM_UNDECIDED = ()     # the seeds of RANDOM_SEEDS that nuset_ref.undecided rejects (tests/test_nuset.py keeps this list true)


def random_case(seed, max_positions=24):
    """The case of ``seed``: A of ANCHOR_COUNTS, fh and fw of 1 .. ``max_positions``, centres moved by up to ``shift`` anchor extents
    and log-sizes by up to ``grow``, a base size of BASE_SIZES, a threshold, pre_nms_top_n of {N // 3, N, 100, 6000} (within
    1 .. MAX_PRE), post_nms_top_n of {800, 20, 5} and one of SCORE_MODES.  The dict carries ``mode`` and ``A`` besides the usual."""
    rng = np.random.default_rng([int(seed), 0x4E75])
    A = int(rng.choice(ANCHOR_COUNTS))
    fh, fw = (int(v) for v in rng.integers(1, max_positions + 1, 2))
    shift, grow = float(rng.choice((0.3, 0.8, 1.5))), float(rng.choice((0.3, 0.5)))
    base = float(rng.choice(BASE_SIZES))
    thr = float(rng.choice((0.1, 0.3, 0.5, 0.7)))
    n = fh * fw * A
    pre = min(max(int(rng.choice((n // 3, n, 100, 6000))), 1), MAX_PRE)
    post = int(rng.choice((800, 20, 5)))
    mode = SCORE_MODES[int(rng.integers(0, 3))]
    cls, bbox = _random(rng, fh, fw, A, shift, grow)
    cls = (_palette if mode == 'palette' else _spread)(rng, cls, n)
    if mode == 'spread_filtered':
        cls, bbox = _filter(rng, cls, bbox, n, 0.2, 0.02)
    c = _case('random_%d' % seed, cls.reshape(fh, fw, 2 * A), bbox.reshape(fh, fw, 4 * A), ref_anchors(A, base), thr, pre, post)
    return dict(c, mode=mode, A=A)
