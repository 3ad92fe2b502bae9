"""The two ends of the post-processing (csrc/stitch_preprocess_kernels.hip) restated in numpy, int64 and float64, for
tests/test_stitch_pre.py and tests/test_gpu_stitch_pre.py.  Written from the reference's lines and from OpenCV's published behaviour,
not from ``oracle/`` (tests/test_stitch_pre.py holds the two against each other), and without the product's Python.

Stitch side (src/image_tools.py:148-252, src/utils.py:117-118): ``window_starts``, ``positions``, ``stitch_map`` (the slice assignments
of patches2im_overlap carried out on index patches), ``quantise``, ``argmax_first``, ``tie_risk``, ``stitch_probs``, and ``stitch``
that puts them together.  Preprocess side (src/image_tools.py:86-101): ``u16_to_u8``, ``pick_channel``, ``histogram``, ``otsu``,
``white_decision``, ``preprocess``.  ``otsu_fused`` and the keyword arguments are the mutants of tests/test_stitch_pre.py: each a slip a
kernel could make."""
import numpy as np

SCW, OV = 256, 25                                            # the window and its overlap
SPW = SCW - 2 * OV                                           # 206: the prediction window
FLT_EPSILON = 2.0 ** -23


# ---- stitch ---------------------------------------------------------------------------------------------------------------------
def window_starts(dim):
    """:163-174 along one axis: multiples of 206 over the cropped extent, and one more window flush with the far edge for a remainder."""
    q, r = divmod(dim - 2 * OV, SPW)
    return [SPW * e for e in range(q)] + ([dim - 2 * OV - SPW] if r else [])


def positions(H, W):
    """:176-178: (n, 2) (row, column) starts; meshgrid(L_h, L_w) ravelled walks the columns outside, the rows inside."""
    Lh, Lw = window_starts(H), window_starts(W)
    return np.array([(h, w) for w in Lw for h in Lh], np.int64).reshape(-1, 2)


def stitch_map(H, W):
    """(H, W) int64: (patch << 16) | (y << 8) | x of the patch pixel that patches2im_overlap leaves at each canvas pixel, -1 where it
    writes nothing.  The assignments of :206-250 in their order, on patches that hold their own indices; numpy resolves the negative
    slice ends as it does there."""
    pos = positions(H, W)
    h_l, w_l = (int(v) for v in pos.max(axis=0))
    canvas = np.full((h_l + SCW, w_l + SCW), -1, np.int64)
    assert canvas.shape == (H, W)
    yy, xx = np.mgrid[:SCW, :SCW]
    lead, core, trail = slice(0, OV), slice(OV, -OV), slice(-OV, None)
    for i, (ph, pw) in enumerate(pos.tolist()):
        e = (i << 16) | (yy << 8) | xx
        rows, cols = slice(ph + OV, ph + SCW - OV), slice(pw + OV, pw + SCW - OV)
        if ph == 0:
            if pw == 0:
                canvas[lead, lead] = e[lead, lead]
                canvas[OV:SCW - OV, lead] = e[core, lead]
                canvas[lead, OV:SCW - OV] = e[lead, core]
            else:
                if pw == w_l:
                    canvas[lead, trail] = e[lead, trail]
                canvas[lead, cols] = e[lead, core]
        if pw == 0 and ph != 0:
            canvas[rows, lead] = e[core, lead]
        if ph == h_l:
            if pw == w_l:
                canvas[trail, trail] = e[trail, trail]
                canvas[h_l + OV:-OV, trail] = e[core, trail]
                canvas[trail, w_l + OV:-OV] = e[trail, core]
            else:
                if pw == 0:
                    canvas[trail, lead] = e[trail, lead]
                canvas[trail, cols] = e[trail, core]
        if pw == w_l and pw != h_l:                          # :242 compares the column start with the last ROW start
            canvas[rows, trail] = e[core, trail]
    for i, (ph, pw) in enumerate(pos.tolist()):              # :247-250: every core, in patch order
        canvas[ph + OV:ph + OV + SPW, pw + OV:pw + OV + SPW] = ((i << 16) | (yy << 8) | xx)[core, core]
    return canvas


def quantise(p):
    """img_as_ubyte of float values in [-1, 1]: rint(float64(p) * 255), half to even, clipped to 0 .. 255 -> int64."""
    return np.clip(np.rint(np.asarray(p, np.float32).astype(np.float64) * 255.0), 0, 255).astype(np.int64)


def argmax_first(q, last=False):
    """np.argmax over the last axis: the FIRST index of the maximum (``last``: the mutant that keeps the last one)."""
    q = np.asarray(q)
    if last:
        return q.shape[-1] - 1 - np.argmax(q[..., ::-1], axis=-1)
    return np.argmax(q, axis=-1)


def tie_pixels(q, written, gap=1):
    """Where a last-bit difference in one probability can change the label: written pixels whose two largest quantised values differ by
    at most ``gap`` (mutant: 0, the test ``< 1``)."""
    top2 = np.sort(np.asarray(q), axis=-1)[..., -2:]
    return written & (top2[..., 1] - top2[..., 0] <= gap)


def launch_model(tie, n_img, px, end_of_other_image='own'):
    """How the counting launch walks a batch, for the cases that are named after its paths: workgroups of 256 threads, one per 256 pixels
    but 16384 at the most, thread t of the grid taking the flat pixels t, t + grid, t + 2 grid, ...  A thread counts the tie pixels of the
    image it is in; when its walk enters another image it adds what it has to the image it leaves (the FLUSH INSIDE THE LOOP); at the end
    the threads whose last image is that of the workgroup's thread 0 go through one shared sum, and a thread whose last image is ANOTHER
    one adds its count to that image itself (the MIXED WORKGROUP END).  ``tie``: (n_img * px) bool.  -> dict ``loop_flushes`` and
    ``mixed_ends`` (the number of such additions with a count above 0) and ``tie_risk`` (n_img) int64 - the plain per-image counts,
    unless ``end_of_other_image`` names a slip: 'thread0' adds the mixed-end counts to thread 0's image, 'dropped' loses them."""
    total = n_img * px
    grid = min(-(-total // 256), 256 * 64) * 256             # threads in the launch
    t = np.flatnonzero(np.asarray(tie).reshape(-1))
    pairs, cnt = np.unique(np.stack([t % grid, t // px]), axis=1, return_counts=True)
    tid, im = pairs
    last_image = lambda thread: (thread + (total - 1 - thread) // grid * grid) // px      # of the last pixel a thread visits
    at_end = im == last_image(tid)
    mixed = at_end & (last_image(tid) != last_image(tid // 256 * 256))
    counts = np.zeros(n_img, np.int64)
    np.add.at(counts, im[~mixed], cnt[~mixed])
    if end_of_other_image == 'own':
        np.add.at(counts, im[mixed], cnt[mixed])
    elif end_of_other_image == 'thread0':
        np.add.at(counts, last_image(tid[mixed] // 256 * 256), cnt[mixed])
    else:
        assert end_of_other_image == 'dropped'
    return dict(loop_flushes=int((~at_end).sum()), mixed_ends=int(mixed.sum()), tie_risk=counts)


def stitch(probs, n_img, H, W, last=False, gap=1, count_modulo=None, end_of_other_image='own'):
    """(n_img * n_pos, 256, 256, cs >= 4) float32 -> dict ``labels`` (n, H, W) uint8, ``tie_risk`` (n) int32, ``probs`` (n, H, W, 4)
    float32.  Channels from 4 on are not read.  Mutants: ``count_modulo``, counters indexed by image % count_modulo;
    ``end_of_other_image``, see ``launch_model``."""
    probs = np.asarray(probs)
    m = stitch_map(H, W)
    n_pos = len(positions(H, W))
    assert probs.dtype == np.float32 and probs.shape[0] == n_img * n_pos and probs.shape[1:3] == (SCW, SCW) and probs.shape[3] >= 4
    written = m >= 0
    src = np.where(written, m, 0)
    patch, y, x = src >> 16, (src >> 8) & 255, src & 255
    out = np.zeros((n_img, H, W, 4), np.float32)
    for k in range(n_img):
        out[k][written] = probs[k * n_pos + patch[written], y[written], x[written], :4]
    q = quantise(out)
    ties = tie_pixels(q, written[None], gap)
    tie = ties.reshape(n_img, -1).sum(axis=1)
    if end_of_other_image != 'own':
        tie = launch_model(ties, n_img, H * W, end_of_other_image)['tie_risk']
    if count_modulo:
        folded = np.zeros(n_img, np.int64)
        np.add.at(folded, np.arange(n_img) % count_modulo, tie)
        tie = folded
    return dict(labels=argmax_first(q, last).astype(np.uint8), tie_risk=tie.astype(np.int32), probs=out, ties=ties)


STITCH_ORDER = ('probs', 'labels', 'tie_risk')               # the order a difference is reported in: the gather first


# ---- meta_preprocess ------------------------------------------------------------------------------------------------------------
def u16_to_u8(img, half_up=False, truncate=False):
    """cv2.convertScaleAbs(alpha = 255 / 65535) on uint16: the product in float32, cvRound (half to even), saturated.  uint8 passes.
    Mutants: ``half_up`` floor(x + 0.5) on the same float32 product; ``truncate``."""
    img = np.asarray(img)
    if img.dtype != np.uint16:
        assert img.dtype == np.uint8
        return img
    f = np.abs(img.astype(np.float32) * np.float32(255.0 / 65535.0))
    assert f.dtype == np.float32
    r = np.floor(f.astype(np.float64) + 0.5) if half_up else (np.floor(f) if truncate else np.rint(f))
    return np.minimum(r, 255).astype(np.uint8)


def pick_channel(img, channel=2):
    """(H, W) passes; (H, W, C): C == 1 its only channel, else channel 2 (mutant: another)."""
    img = np.asarray(img)
    if img.ndim == 2:
        return img
    return img[..., 0] if img.shape[-1] == 1 else img[..., channel]


def histogram(gray):
    return np.bincount(np.asarray(gray, np.uint8).reshape(-1), minlength=256).astype(np.int64)


def _fma(a, b, c):
    """a * b + c rounded once.  Floats are ratios of integers with a power of two below, and Python's int / int is correctly rounded."""
    (an, ad), (bn, bd), (cn, cd) = a.as_integer_ratio(), b.as_integer_ratio(), c.as_integer_ratio()
    return (an * bn * cd + cn * ad * bd) / (ad * bd * cd)


try:
    from math import fma as _math_fma                        # Python 3.13

    def _fma(a, b, c):                                       # noqa: F811
        return _math_fma(a, b, c)
except ImportError:
    pass


def otsu(hist, px, fused=False):
    """OpenCV's getThreshVal_Otsu_8u in plain float64, operation by operation: the first strict maximum of the between-class variance,
    classes lighter than FLT_EPSILON skipped.  ``px`` is the histogram's sum.  ``fused``: see ``otsu_fused``."""
    h = [int(v) for v in hist]
    assert len(h) == 256 and sum(h) == px > 0
    scale = 1.0 / float(px)
    mu = float(sum(i * v for i, v in enumerate(h))) * scale  # (the sum is an integer below 2^53: exact in any order)
    mu1 = q1 = max_sigma = 0.0
    max_val = 0
    for i in range(256):
        p_i = float(h[i]) * scale
        mu1 *= q1
        q1 += p_i
        q2 = 1.0 - q1
        if min(q1, q2) < FLT_EPSILON or max(q1, q2) > 1.0 - FLT_EPSILON:
            continue
        if fused:
            mu1 = _fma(float(i), p_i, mu1) / q1
            mu2 = _fma(-q1, mu1, mu) / q2
        else:
            mu1 = (mu1 + float(i) * p_i) / q1
            mu2 = (mu - q1 * mu1) / q2
        sigma = q1 * q2 * (mu1 - mu2) * (mu1 - mu2)
        if sigma > max_sigma:
            max_sigma, max_val = sigma, i
    return max_val


def otsu_fused(hist, px):
    """A MUTANT: the same loop with ``mu1 + i * p_i`` and ``mu - q1 * mu1`` each rounded once, as a compiler that contracts a * b + c
    into a fused multiply-add evaluates them."""
    return otsu(hist, px, fused=True)


def white_decision(hist, px, threshold, or_equal=False):
    """:94: more than half of the pixels lie above the threshold, strictly (mutant: ``>=``).  px * 0.5 is exact in float64."""
    white = int(sum(int(v) for v in hist[threshold + 1:]))
    return int(white >= px * 0.5) if or_equal else int(white > px * 0.5)


def otsu_decide(hist, px, otsu_fn=otsu, or_equal=False):
    """-> (threshold, inverted) of one histogram."""
    t = otsu_fn(hist, px)
    return t, white_decision(hist, px, t, or_equal)


def preprocess(img, otsu_fn=otsu, or_equal=False, channel=2, half_up=False, truncate=False):
    """meta_preprocess of one image (H, W[, C]) uint8 / uint16 -> dict ``hist`` (256) uint32 of the 8-bit channel before the inversion,
    ``threshold``, ``inverted``, ``gray`` (H, W) uint8."""
    g = np.ascontiguousarray(pick_channel(u16_to_u8(img, half_up, truncate), channel))
    h = histogram(g)
    t, inv = otsu_decide(h, g.size, otsu_fn, or_equal)
    return dict(hist=h.astype(np.uint32), threshold=t, inverted=inv, gray=(255 - g).astype(np.uint8) if inv else g)


PRE_ORDER = ('hist', 'threshold', 'inverted', 'gray')        # the order the stages run in
