"""The two ends of the post-processing on the device (csrc/stitch_preprocess_kernels.hip through ecseg_stitch_stages_debug,
ecseg_preprocess_stages_debug and ecseg_otsu_debug) against tests/stitch_pre_ref.py, with no tolerance anywhere: the stitched
probabilities, the labels and the tie-risk counts byte for byte; the histogram, Otsu's threshold, the inversion flag and the gray
image of meta_preprocess; threshold and flag of a few thousand histograms on which the last bit of the class variance decides.  The
first stage that differs is named, in the order the stages run.  Cases: tests/stitch_pre_cases.py; tests/test_stitch_pre.py ties the
restatement to the oracle and shows which case catches which slip."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import stitch_pre_cases as cases             # noqa: E402
import stitch_pre_ref as ref                 # noqa: E402

from ecseg_amd import _lib                   # noqa: E402

pytestmark = pytest.mark.gpu
INVALID = -1                                 # ECSEG_E_INVALID
PRE_CASES = cases.preprocess_cases()
PRE_NAMES = [c['name'] for c in PRE_CASES]
_STITCH = {}


def first_difference(got, exp, order):
    """None, or 'stage: n of N values differ, the first at index: got / expected' for the first differing stage in running order."""
    for key in order:
        g, e = np.asarray(got[key]), np.asarray(exp[key])
        if g.shape != e.shape:
            return '%s: shape %s, expected %s' % (key, g.shape, e.shape)
        assert np.array_equal(e.astype(g.dtype), e), key     # (the expected values fit the device's type)
        e = e.astype(g.dtype)
        if g.tobytes() != e.tobytes():                       # bytes: -0.0 is not 0.0 in a gather
            bits = lambda a: a.view(np.uint32) if a.dtype == np.float32 else a
            bad = np.argwhere(bits(g) != bits(e))
            at = tuple(int(v) for v in bad[0])
            return '%s: %d of %d values differ, the first at %s: %r, expected %r' % (key, len(bad), g.size, at, g[at], e[at])
    return None


def stitch_case(name):
    """A stitch case with its restatement, made once for all the tests of this file (the two large batches are not kept)."""
    if name in _STITCH:
        return _STITCH[name]
    c = cases.make_stitch(name)
    c['want'] = ref.stitch(c['probs'], c['n_img'], c['H'], c['W'])
    if name in cases.SMALL_STITCH_NAMES:
        _STITCH[name] = c
    return c


def check_stitch(got, c, what='the restatement', want=None):
    assert got['labels'].dtype == np.uint8 and got['tie_risk'].dtype == np.int32 and got['probs'].dtype == np.float32
    diff = first_difference(got, want or c['want'], ref.STITCH_ORDER)
    assert diff is None, '%s against %s - %s' % (c['name'], what, diff)


# ---- stitch -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', cases.STITCH_NAMES)
def test_stitch_equals_the_restatement_and_repeats(gpu, name):
    c = stitch_case(name)
    got = gpu.stitch_stages(c['probs'], c['n_img'], c['H'], c['W'])
    check_stitch(got, c)
    if c['ties'] is not None:
        assert got['tie_risk'].tolist() == c['ties']
    again = gpu.stitch_stages(c['probs'], c['n_img'], c['H'], c['W'])
    for key in ref.STITCH_ORDER:
        assert again[key].tobytes() == got[key].tobytes(), (name, key)


def test_stitch_batch_over_the_launch_cap(gpu):
    """64 images of 257 x 257 in one launch: 16384 workgroups walk 4 227 136 pixels, so workgroups 0 .. 128 go on from image 0 into
    image 63 (the flush inside the pixel loop) and workgroups lie across image boundaries (the workgroup-end path for a thread of
    another image).  Near-ties lie where both paths carry a count: tests/test_stitch_pre.py counts 12 and 198 such additions."""
    c = cases.big_stitch_case()
    got = gpu.stitch_stages(c['probs'], c['n_img'], c['H'], c['W'])
    assert got['tie_risk'].tolist() == c['ties'], 'tie-risk counts of the images: %s' % got['tie_risk'].tolist()
    check_stitch(got, c, want=ref.stitch(c['probs'], c['n_img'], c['H'], c['W']))


@pytest.mark.parametrize('name', ['stitch_257x257_n3_cs4', 'stitch_300x462_n3_cs4', 'stitch_257x257_n3_cs8', 'stitch_300x300_n2_cs4'])
def test_stitch_batch_equals_the_single_image_calls(gpu, name):
    c = stitch_case(name)
    n_pos = len(c['probs']) // c['n_img']
    for k in range(c['n_img']):
        alone = gpu.stitch_stages(c['probs'][k * n_pos:(k + 1) * n_pos], 1, c['H'], c['W'])
        check_stitch(alone, c, 'image %d of the batch' % k, want={key: c['want'][key][k:k + 1] for key in ref.STITCH_ORDER})


@pytest.mark.parametrize('name', [n for n in cases.SMALL_STITCH_NAMES if n.endswith('cs4')])
def test_stitch_argmax_equals_the_debug_labels(gpu, name):
    c = stitch_case(name)
    lab = gpu.stitch_argmax(c['probs'], c['n_img'], c['H'], c['W'])
    assert lab.dtype == np.uint8 and lab.tobytes() == c['want']['labels'].tobytes(), name
    assert lab.tobytes() == gpu.stitch_stages(c['probs'], c['n_img'], c['H'], c['W'])['labels'].tobytes()


def test_stitch_null_outputs_and_bad_arguments(gpu):
    c = stitch_case('stitch_257x257_n3_cs8')
    p, n, H, W, want = c['probs'], c['n_img'], c['H'], c['W'], c['want']
    ptr = _lib._ptr
    call = lambda *a: gpu.lib.ecseg_stitch_stages_debug(gpu.h, *a)
    lab, tie, out = np.full((n, H, W), 9, np.uint8), np.full(n, -5, np.int32), np.full((n, H, W, 4), 2, np.float32)
    assert call(ptr(p), 8, n, H, W, ptr(lab), None, None) == 0 and np.array_equal(lab, want['labels'])
    assert call(ptr(p), 8, n, H, W, None, ptr(tie), None) == 0 and np.array_equal(tie, want['tie_risk'])
    assert call(ptr(p), 8, n, H, W, None, None, ptr(out)) == 0 and out.tobytes() == want['probs'].tobytes()
    assert call(ptr(p), 8, n, H, W, None, None, None) == 0
    assert call(ptr(p), 8, 0, H, W, None, None, None) == 0
    lab[:] = 9
    for bad in ((None, 8, n, H, W), (ptr(p), 3, n, H, W), (ptr(p), 0, n, H, W), (ptr(p), 8, -1, H, W), (ptr(p), 8, n, 255, W), (ptr(p), 8, n, H, 0)):
        assert call(*bad, ptr(lab), ptr(tie), ptr(out)) == INVALID and gpu.lib.ecseg_last_error(gpu.h)
    assert (lab == 9).all()
    assert gpu.lib.ecseg_stitch_stages_debug(None, ptr(p), 8, n, H, W, None, None, None) == INVALID
    with pytest.raises(ValueError):
        gpu.stitch_stages(p[:-1], n, H, W)
    check_stitch(gpu.stitch_stages(p, n, H, W), c)           # the handle still works


# ---- meta_preprocess --------------------------------------------------------------------------------------------------------------
def _want_pre(imgs):
    each = [ref.preprocess(im) for im in imgs]
    return dict(hist=np.stack([e['hist'] for e in each]), threshold=np.array([e['threshold'] for e in each], np.int32),
                inverted=np.array([e['inverted'] for e in each], np.int32), gray=np.stack([e['gray'] for e in each]))


@pytest.mark.parametrize('k', range(len(PRE_CASES)), ids=PRE_NAMES)
def test_preprocess_equals_the_restatement_and_the_plain_call(gpu, k):
    imgs = PRE_CASES[k]['imgs']
    got = gpu.preprocess_stages(imgs)
    assert [got[key].dtype for key in ref.PRE_ORDER] == [np.uint32, np.int32, np.int32, np.uint8]
    diff = first_difference(got, _want_pre(imgs), ref.PRE_ORDER)
    assert diff is None, '%s - %s' % (PRE_NAMES[k], diff)
    gray, inv = gpu.preprocess(imgs)
    assert gray.tobytes() == got['gray'].tobytes() and inv.tobytes() == got['inverted'].tobytes()
    again = gpu.preprocess_stages(imgs)
    for key in ref.PRE_ORDER:
        assert again[key].tobytes() == got[key].tobytes(), key


def test_every_u16_value_through_u16_to_u8(gpu):
    v = cases.all_u16_values()
    assert np.array_equal(gpu.u16_to_u8(v), ref.u16_to_u8(v))
    ramp = np.arange(65536, dtype=np.uint16)
    assert np.array_equal(gpu.u16_to_u8(ramp), ref.u16_to_u8(ramp))


def test_preprocess_null_outputs_and_bad_arguments(gpu):
    imgs = PRE_CASES[PRE_NAMES.index('extent_17x15_c3_uint16')]['imgs']
    n, H, W, C = imgs.shape
    want = _want_pre(imgs)
    ptr = _lib._ptr
    call = lambda *a: gpu.lib.ecseg_preprocess_stages_debug(gpu.h, *a)
    hist, thr, inv, gray = np.empty((n, 256), np.uint32), np.empty(n, np.int32), np.empty(n, np.int32), np.full((n, H, W), 9, np.uint8)
    assert call(ptr(imgs), n, H, W, C, 2, None, None, None, ptr(gray)) == 0 and np.array_equal(gray, want['gray'])
    assert call(ptr(imgs), n, H, W, C, 2, ptr(hist), None, None, None) == 0 and np.array_equal(hist, want['hist'])
    assert call(ptr(imgs), n, H, W, C, 2, None, ptr(thr), ptr(inv), None) == 0
    assert np.array_equal(thr, want['threshold']) and np.array_equal(inv, want['inverted'])
    assert call(ptr(imgs), n, H, W, C, 2, None, None, None, None) == 0
    gray[:] = 9
    for bad in ((None, n, H, W, C, 2), (ptr(imgs), -1, H, W, C, 2), (ptr(imgs), n, 0, W, C, 2), (ptr(imgs), n, H, -3, C, 2),
                (ptr(imgs), n, H, W, 2, 2), (ptr(imgs), n, H, W, 5, 2), (ptr(imgs), n, H, W, C, 3), (ptr(imgs), n, H, W, C, 0)):
        assert call(*bad, ptr(hist), ptr(thr), ptr(inv), ptr(gray)) == INVALID and gpu.lib.ecseg_last_error(gpu.h)
    assert (gray == 9).all()
    with pytest.raises(TypeError):
        gpu.preprocess_stages(imgs.astype(np.int16))
    assert first_difference(gpu.preprocess_stages(imgs), want, ref.PRE_ORDER) is None      # the handle still works


# ---- Otsu alone -------------------------------------------------------------------------------------------------------------------
def test_otsu_on_every_histogram(gpu):
    """Threshold and flag of every histogram of the set in one call.  The kernel compiled with floating-point contraction (``q1 + h *
    scale``, ``mu1 + i * p_i`` and ``mu - q1 * mu1`` as fused multiply-adds) returned another threshold on 451 of these 3023 histograms
    (the fused model of tests/stitch_pre_ref.py: on 274), and on each of them the other inversion flag; with contraction off in the kernel, on none."""
    names, hs, px = cases.otsu_histograms()
    want = np.array([ref.otsu_decide(h, int(p)) for h, p in zip(hs, px)], np.int32)
    thr, inv = gpu.otsu(hs, px)
    bad_t, bad_f = np.nonzero(thr != want[:, 0])[0], np.nonzero(inv != want[:, 1])[0]
    fused = np.array([ref.otsu_decide(hs[i], int(px[i]), ref.otsu_fused) for i in bad_t], np.int32).reshape(-1, 2)
    print('\n%d histograms: the device differs from plain float64 on the threshold of %d and on the flag of %d; on %d of those it returns '
          'what fused multiply-adds give' % (len(names), len(bad_t), len(bad_f), int((fused[:, 0] == thr[bad_t]).sum())))
    assert len(bad_t) == 0, 'threshold: %d of %d histograms differ, the first %s: %d, expected %d' % (
        len(bad_t), len(names), names[bad_t[0]], thr[bad_t[0]], want[bad_t[0], 0])
    assert len(bad_f) == 0, 'flag: %d of %d histograms differ, the first %s' % (len(bad_f), len(names), names[bad_f[0]])
    again = gpu.otsu(hs[::-1], px[::-1])                     # another order, another thread for each: the same values
    assert np.array_equal(again[0][::-1], thr) and np.array_equal(again[1][::-1], inv)
    one = gpu.otsu(hs[-1:], px[-1:])
    assert (int(one[0][0]), int(one[1][0])) == tuple(want[-1])


def test_otsu_null_outputs_and_bad_arguments(gpu):
    names, hs, px = cases.otsu_histograms()
    hs, px = np.ascontiguousarray(hs[:70]), np.ascontiguousarray(px[:70])
    want = np.array([ref.otsu_decide(h, int(p)) for h, p in zip(hs, px)], np.int32)
    ptr = _lib._ptr
    call = lambda *a: gpu.lib.ecseg_otsu_debug(gpu.h, *a)
    thr, inv = np.full(70, -7, np.int32), np.full(70, -7, np.int32)
    assert call(ptr(hs), 70, ptr(px), ptr(thr), None) == 0 and np.array_equal(thr, want[:, 0])
    assert call(ptr(hs), 70, ptr(px), None, ptr(inv)) == 0 and np.array_equal(inv, want[:, 1])
    assert call(ptr(hs), 70, ptr(px), None, None) == 0 and call(ptr(hs), 0, ptr(px), None, None) == 0
    thr[:] = -7
    off = px.copy(); off[69] += 1
    zero_h, zero_p = np.zeros((1, 256), np.uint32), np.zeros(1, np.int64)
    over_h = np.zeros((1, 256), np.uint32); over_h[0, 0] = over_h[0, 9] = 2 ** 30
    for bad in ((None, 70, ptr(px)), (ptr(hs), 70, None), (ptr(hs), -1, ptr(px)), (ptr(hs), 70, ptr(off)), (ptr(zero_h), 1, ptr(zero_p)),
                (ptr(over_h), 1, ptr(np.array([2 ** 31], np.int64)))):
        assert call(*bad, ptr(thr), ptr(inv)) == INVALID and gpu.lib.ecseg_last_error(gpu.h)
    assert (thr == -7).all()
    with pytest.raises(ValueError):
        gpu.otsu(hs, px[:-1])
    with pytest.raises(_lib.EcsegError):
        gpu.otsu(hs, off)
    got = gpu.otsu(hs, px)                                   # the handle still works
    assert np.array_equal(got[0], want[:, 0]) and np.array_equal(got[1], want[:, 1])
