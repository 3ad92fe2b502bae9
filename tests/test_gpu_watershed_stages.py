"""Every stage of the marker watershed on the device (csrc/watershed_kernels.hip through ecseg_marker_watershed_stages_debug and
ecseg_marker_watershed_batch_stages_debug) against ``watershed_ref.stages``, with no tolerance and in the order the stages run: the
dilated marker image ``rw``, the hole-filled mask ``filled``, the squared distance ``d2``, the flood's labels ``lab`` and the final
``out``.  The first stage that differs is named, so that a wrong distance is reported as a wrong distance and not as a line that
moved.  tests/test_watershed_stages.py ties the restatement to a second distance and shows, with mutants, what comparing ``out``
alone lets through.  Cases: tests/watershed_stage_cases.py (extents from 1 x 1, both sides of 64 columns and 256 pixels, zeros and
holes placed for every branch, labels against list order, a seeded range) and every case of tests/watershed_cases.py."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import watershed_cases as old_cases          # noqa: E402
import watershed_ref as ref                  # noqa: E402
import watershed_stage_cases as cases        # noqa: E402

from ecseg_amd import _lib                   # noqa: E402

pytestmark = pytest.mark.gpu
INVALID = -1                                 # ECSEG_E_INVALID
DTYPES = dict(rw=np.int32, filled=np.uint8, d2=np.int32, lab=np.int32, out=np.uint8)


def _from_old(c):
    mk = ref.marker_list(c['scores'], c['proposals'], c['mask'], c['min_score'])
    return None if mk is None else dict(name=c['name'], mask=c['mask'], rows=mk[0], cols=mk[1], labels=mk[2])


CASES = cases.all_cases()
NAMES = [c['name'] for c in CASES]
OLD = [c for c in map(_from_old, old_cases.all_cases()) if c is not None]        # the cases that reach the watershed
_WANT = {}


def _args(c):
    return c['mask'], c['rows'], c['cols'], c['labels']


def want(c):
    """``stages`` of a case, computed once for all the tests of this file."""
    if c['name'] not in _WANT:
        _WANT[c['name']] = ref.stages(*_args(c))
    return _WANT[c['name']]


def first_difference(got, exp):
    """None, or 'stage: n of N pixels differ, the first at (row, column): got / expected' for the first differing stage in running order."""
    for key in ref.STAGE_ORDER:
        g, e = got[key], exp[key]
        if g.shape != e.shape:
            return '%s: shape %s, expected %s' % (key, g.shape, e.shape)
        if not np.array_equal(g, e):
            bad = np.argwhere(g != e)
            y, x = (int(v) for v in bad[0])
            return '%s: %d of %d pixels differ, the first at (%d, %d): %d, expected %d' % (key, len(bad), g.size, y, x, g[y, x], e[y, x])
    return None


def check(got, c, what='the restatement'):
    assert all(got[key].dtype == DTYPES[key] for key in DTYPES)
    diff = first_difference(got, want(c))
    assert diff is None, '%s against %s - %s' % (c['name'], what, diff)


@pytest.mark.parametrize('k', range(len(CASES)), ids=NAMES)
def test_every_stage_equals_the_restatement(gpu, k):
    check(gpu.marker_watershed_stages(*_args(CASES[k])), CASES[k])


@pytest.mark.parametrize('k', range(len(OLD)), ids=[c['name'] for c in OLD])
def test_every_stage_equals_the_restatement_on_the_committed_cases(gpu, k):
    check(gpu.marker_watershed_stages(*_args(OLD[k])), OLD[k])


# ---- the batch ------------------------------------------------------------------------------------------------------------------
def _pack(cs, gaps):
    """-> (buffer, table, rows, cols, labels): image k starts ``gaps[k]`` bytes behind the end of the one in front; the gaps hold 1."""
    tab = np.zeros((len(cs), 5), np.int64)
    off = first = 0
    for k, c in enumerate(cs):
        off += gaps[k]
        tab[k] = (off, c['mask'].shape[0], c['mask'].shape[1], first, len(c['rows']))
        off += c['mask'].size
        first += len(c['rows'])
    buf = np.ones(off + 3, np.uint8)
    for row, c in zip(tab, cs):
        buf[row[0]:row[0] + c['mask'].size] = c['mask'].reshape(-1)
    cat = lambda key: np.concatenate([c[key] for c in cs] + [np.zeros(0, np.int32)])
    return buf, tab, cat('rows'), cat('cols'), cat('labels')


GAPS = (1, 0, 3, 2, 5, 7, 6)                                 # between the images: mostly no multiple of 4, so the int32 slices start anywhere


def _batch(gpu, cs):
    buf, tab, r, c, l = _pack(cs, [GAPS[k % len(GAPS)] for k in range(len(cs))])
    assert any(o % 4 for o in tab[:, 0].tolist())
    return gpu.marker_watershed_batch_stages(buf, tab, r, c, l)


@pytest.fixture(scope='module')
def everything(gpu):
    """Every new case in ONE call."""
    return _batch(gpu, CASES)


def test_the_batch_equals_the_restatement_and_the_single_call(gpu, everything):
    assert len(everything) == len(CASES)
    for c, got in zip(CASES, everything):
        check(got, c)
        alone = gpu.marker_watershed_stages(*_args(c))
        diff = first_difference(got, alone)
        assert diff is None, '%s, the batch against the single call - %s' % (c['name'], diff)


def test_the_reversed_batch_gives_the_same_bytes(gpu, everything):
    got = _batch(gpu, CASES[::-1])[::-1]
    for c, a, b in zip(CASES, got, everything):
        for key in ref.STAGE_ORDER:
            assert a[key].tobytes() == b[key].tobytes(), (c['name'], key)


@pytest.mark.parametrize('order', [('extent_1x1', 'large_160'), ('large_160', 'extent_1x1'), ('large_160', 'one_pixel_no_marker', 'extent_2x2')])
def test_one_pixel_beside_the_largest(gpu, order):
    """The grid is the large image's: every block of the small image but the first returns at once."""
    cs = [CASES[NAMES.index(n)] for n in order]
    for c, got in zip(cs, _batch(gpu, cs)):
        check(got, c)


def test_the_committed_cases_in_one_batch(gpu):
    for c, got in zip(OLD, _batch(gpu, OLD)):
        check(got, c)


# ---- the handle and the arguments --------------------------------------------------------------------------------------------------
def test_one_handle_over_a_large_a_one_pixel_and_the_large_case_again(gpu):
    big, tiny = CASES[NAMES.index('large_160')], CASES[NAMES.index('extent_1x1')]
    first = gpu.marker_watershed_stages(*_args(big))
    small = gpu.marker_watershed_stages(*_args(tiny))
    again = gpu.marker_watershed_stages(*_args(big))
    check(first, big)
    check(small, tiny)
    for key in ref.STAGE_ORDER:
        assert first[key].tobytes() == again[key].tobytes(), key


def test_null_stage_pointers_give_the_plain_call(gpu):
    ptr = _lib._ptr
    for c in (CASES[NAMES.index('marker_pixels_become_lines')], CASES[NAMES.index('extent_64x65')], CASES[NAMES.index('no_marker')]):
        m, r, cc, l = _args(c)
        out = np.full(m.shape, 7, np.uint8)
        rc = gpu.lib.ecseg_marker_watershed_stages_debug(gpu.h, ptr(m), m.shape[0], m.shape[1], ptr(r), ptr(cc), ptr(l), len(r), ptr(out),
                                                         None, None, None, None)
        assert rc == 0 and np.array_equal(out, gpu.marker_watershed(m, r, cc, l)) and np.array_equal(out, want(c)['out'])
        d2 = np.empty(m.shape, np.int32)                     # one pointer alone
        rc = gpu.lib.ecseg_marker_watershed_stages_debug(gpu.h, ptr(m), m.shape[0], m.shape[1], ptr(r), ptr(cc), ptr(l), len(r), ptr(out),
                                                         None, None, ptr(d2), None)
        assert rc == 0 and np.array_equal(d2, want(c)['d2'])
    cs = [CASES[NAMES.index('extent_3x65')], CASES[NAMES.index('hole_closed')]]
    buf, tab, r, cc, l = _pack(cs, [1, 2])
    out = np.full(buf.size, 7, np.uint8)
    rc = gpu.lib.ecseg_marker_watershed_batch_stages_debug(gpu.h, ptr(buf), buf.size, ptr(tab), len(tab), ptr(r), ptr(cc), ptr(l), len(r), ptr(out),
                                                           None, None, None, None)
    assert rc == 0 and np.array_equal(out, gpu.marker_watershed_packed(buf, tab, r, cc, l))
    for c, (o, H, W, _, _) in zip(cs, tab.tolist()):
        assert np.array_equal(out[o:o + H * W].reshape(H, W), want(c)['out'])


def test_bad_arguments_are_refused_and_the_handle_still_works(gpu):
    c = CASES[NAMES.index('hole_closed')]
    m, r, cc, l = _args(c)
    H, W = m.shape
    ptr = _lib._ptr
    out = np.empty_like(m)
    st = [np.empty(m.shape, np.int32), np.empty(m.shape, np.uint8), np.empty(m.shape, np.int32), np.empty(m.shape, np.int32)]
    sp = [ptr(a) for a in st]
    call = lambda mask, h, w, rr, n, o: gpu.lib.ecseg_marker_watershed_stages_debug(gpu.h, mask, h, w, rr, ptr(cc), ptr(l), n, o, *sp)
    assert call(ptr(m), H, W, ptr(r), len(r), ptr(out)) == 0
    assert call(None, H, W, ptr(r), len(r), ptr(out)) == INVALID
    assert call(ptr(m), H, W, ptr(r), len(r), None) == INVALID
    assert call(ptr(m), 0, W, ptr(r), len(r), ptr(out)) == INVALID
    assert call(ptr(m), H, 16385, ptr(r), len(r), ptr(out)) == INVALID
    assert call(ptr(m), H, W, ptr(r), -1, ptr(out)) == INVALID
    assert call(ptr(m), H, W, None, len(r), ptr(out)) == INVALID
    bad = r.copy(); bad[1] = H
    assert call(ptr(m), H, W, ptr(bad), len(r), ptr(out)) == INVALID and b'marker 1' in gpu.lib.ecseg_last_error(gpu.h)
    zero = np.zeros_like(l)
    assert gpu.lib.ecseg_marker_watershed_stages_debug(gpu.h, ptr(m), H, W, ptr(r), ptr(cc), ptr(zero), len(r), ptr(out), *sp) == INVALID
    with pytest.raises(_lib.EcsegError):
        gpu.marker_watershed_stages(m, [H], [0], [1])
    with pytest.raises(ValueError):
        gpu.marker_watershed_stages(m, [1, 2], [1], [1])

    buf, tab, br, bc, bl = _pack([c, c], [1, 3])
    big = [np.empty(buf.size, np.int32), np.empty(buf.size, np.uint8), np.empty(buf.size, np.int32), np.empty(buf.size, np.int32)]
    bout = np.empty_like(buf)
    bcall = lambda t, nbytes=buf.size, o=ptr(bout): gpu.lib.ecseg_marker_watershed_batch_stages_debug(
        gpu.h, ptr(buf), nbytes, ptr(np.ascontiguousarray(t, np.int64)), len(t), ptr(br), ptr(bc), ptr(bl), len(br), o, *[ptr(a) for a in big])
    assert bcall(tab) == 0
    over = tab.copy(); over[1, 0] = tab[0, 0] + m.size - 1
    assert bcall(over) == INVALID and b'overlap' in gpu.lib.ecseg_last_error(gpu.h)
    assert bcall(tab, nbytes=int(tab[1, 0]) + m.size - 1) == INVALID
    assert bcall(tab, o=None) == INVALID
    wide = tab.copy(); wide[0, 2] = 16385
    assert bcall(wide) == INVALID
    more = tab.copy(); more[1, 4] += 1
    assert bcall(more) == INVALID and b'lists' in gpu.lib.ecseg_last_error(gpu.h)
    with pytest.raises(_lib.EcsegError):
        gpu.marker_watershed_batch_stages(buf, over, br, bc, bl)

    check(gpu.marker_watershed_stages(m, r, cc, l), c)       # the handle still works, in both calls
    for got in gpu.marker_watershed_batch_stages(buf, tab, br, bc, bl):
        check(got, c)
