"""Seeded inputs of the proposal layer for tests/test_nuset.py (restatement against restatement, no GPU) and tests/test_gpu_nuset.py
(device against restatement).  Not a test module.

Every case is chosen so that no decision of a float32 run hangs on a rounding: scores that differ in float64 differ in float32 in
the same order, and every pair decision of the NMS stays clear of the threshold by more than ``nuset_ref.iou_bound``
(tests/test_nuset.py checks both for every case here, so a case that is edited must pass there first).  The seeds of the random
cases were picked by that check."""
import numpy as np

RATIOS = (0.125, 0.25, 0.5, 1.0, 2.0, 4.0, 8.0)
SCALES = (0.5, 1.0, 2.0)
SEED_TOP_K = 1            # (seed 0 leaves one IoU within 1e-5 of the threshold)


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
