"""One connected-component labelling pass on the device (``Handle.ccl_pass``: run_ccl_pass of csrc/ccl_kernels.hip alone, every
product exported) against the reference of ccl_pass_ref.py, bit for bit: roots, areas, coordinate sums, flag words, counters, root
lists, flag queries and the tile votes, for every pass a driver builds and the cross of connectivity x statistics x aux mode x
sparse, on every image of ccl_pass_cases.py (test_ccl_pass.py holds the reference and the case list themselves on the host)."""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ccl_pass_cases as cc          # noqa: E402
import ccl_pass_ref as ref           # noqa: E402

from ecseg_amd._lib import EcsegError    # noqa: E402

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _labelling(ci, i, src, lut, conn):
    """The reference labelling of image i of case ci, shared by every mode with this key image, LUT and connectivity."""
    return ref.Labelling(getattr(cc.cases()[ci], src)[i], lut, conn)


@functools.lru_cache(maxsize=None)
def _single_bit_aux(ci, src, lut, conn):
    n = getattr(cc.cases()[ci], src).shape[0]
    return np.stack([cc.single_bit_aux(_labelling(ci, i, src, lut, conn).comp) for i in range(n)])


def _run(gpu, imgs, aux, mode, queries=()):
    return gpu.ccl_pass(imgs, aux if mode.aux_mode == ref.AUX_IMAGE else None, lut=mode.lut, conn=mode.conn, stat=mode.stat,
                        aux_mode=mode.aux_mode, aux_c=mode.aux_c, need=mode.need, count_only=mode.count_only, sparse=mode.sparse,
                        allow_full=mode.allow_full, queries=queries)


_check_queries, _check = ref.check_queries, ref.check_pass     # (shared with tests/test_gpu_scratch.py)


def _hold(gpu, mode, ci):
    case = cc.cases()[ci]
    imgs = getattr(case, mode.src)
    labs = [_labelling(ci, i, mode.src, mode.lut, mode.conn) for i in range(imgs.shape[0])]
    auxes = [('', None)]
    if mode.aux_mode == ref.AUX_IMAGE:
        auxes = [('seeded', case.aux), ('one-bit', _single_bit_aux(ci, mode.src, mode.lut, mode.conn))]
    groups = cc.queries_of(mode) or [[]]
    for tag, aux in auxes:
        what = (mode.name, case.name, tag)
        _check(_run(gpu, imgs, aux, mode, groups[0]), imgs, aux, mode, labs, groups[0], what)
        for q in groups[1:]:
            _check_queries(_run(gpu, imgs, aux, mode, q), labs, aux, mode, q, what)


@pytest.mark.parametrize('mode', cc.MODES, ids=[m.name for m in cc.MODES])
def test_pass_equals_reference(gpu, mode):
    """Every image of the case list under this pass: no case is left out for any mode."""
    for ci in range(len(cc.cases())):
        _hold(gpu, mode, ci)


def _stale_images():
    H, W = 96, 200
    a = cc.PATTERNS['noise90'](H, W, 7)
    b = cc.PATTERNS['noise30'](H, W, 8).copy()
    b[0:32, 64:128] = 1          # no key under lut_ne(1), lut_nonzero_except(1)
    b[32:64, 64:128] = 2         # none under lut_ne(2), lut_nonzero_except(2), lut_eq(3)
    b[64:96, 128:192] = 0        # none under LUT_MULTI, LUT_NONZERO, lut_eq(3), the overlay LUT
    b[32:64, 0:64] = 0
    return a, b


def test_nothing_of_an_earlier_pass_leaks_into_a_later_one(gpu):
    """A dense pass with every statistic and all five flag bits on image A leaves parents, slots, owner bits and tile votes
    everywhere; then each sparse pass on an image whose keyed tiles are a strict subset of A's, and the full-tile fill passes on
    an image whose full tiles were busy tiles of A - each equal to the reference."""
    a, b = _stale_images()
    dense = cc._mode('dense', 'labels', ref.LUT_MULTI, 8, ref.STAT_AREA | ref.STAT_SUMS, ref.AUX_IMAGE, need=ref.NEED_NCOMP | ref.NEED_NPX)
    aux_a = np.full(a.shape, 31, np.uint8)
    lab_a = ref.Labelling(a, dense.lut, dense.conn)
    assert ref.tile_model(ref.keys_of(a, dense.lut), False).all()
    aux_b = np.random.RandomState(3).randint(0, 32, b.shape).astype(np.uint8)

    def dirty():
        _check(_run(gpu, a[None], aux_a[None], dense), a[None], aux_a[None], dense, [lab_a], [], 'dense A')

    for mode in [m for m in cc.MODES if m.sparse]:
        img = b if mode.src == 'labels' else cc.as_mask(b)
        tiles = ref.tile_model(ref.keys_of(img, mode.lut), False)
        assert not tiles.all() and tiles.any(), mode.name            # a strict subset of A's keyed tiles
        dirty()
        q = (cc.queries_of(mode) or [[]])[0]
        _check(_run(gpu, img[None], aux_b[None], mode, q), img[None], aux_b[None], mode, [ref.Labelling(img, mode.lut, mode.conn)], q,
               ('after dense A', mode.name))
    for c, mode in ((1, cc.DRIVER_MODES[0]), (2, cc.DRIVER_MODES[1])):
        assert mode.allow_full and mode.lut == ref.lut_ne(c)
        img = cc.PATTERNS['moat'](*a.shape, 0) * np.uint8(c)
        assert (ref.tile_model(ref.keys_of(img, mode.lut), True) == 2).any()
        dirty()
        q = cc.queries_of(mode)[0]
        _check(_run(gpu, img[None], None, mode, q), img[None], None, mode, [ref.Labelling(img, mode.lut, mode.conn)], q,
               ('full tiles after dense A', mode.name))


@pytest.mark.parametrize('mode', cc.DRIVER_MODES, ids=[m.name for m in cc.DRIVER_MODES])
def test_pass_is_deterministic(gpu, mode):
    """Twice on the densest case (every pattern at 96 x 200): identical exports, the lists as sorted arrays."""
    ci = next(k for k, c in enumerate(cc.cases()) if c.labels.shape[1:] == (96, 200))
    case = cc.cases()[ci]
    imgs = getattr(case, mode.src)
    q = (cc.queries_of(mode) or [[]])[0]
    one, two = _run(gpu, imgs, case.aux, mode, q), _run(gpu, imgs, case.aux, mode, q)
    assert sorted(one) == sorted(two)
    for k in one:
        if k in ('list1', 'list2'):
            assert all(np.array_equal(np.sort(x), np.sort(y)) for x, y in zip(one[k], two[k])), k
        else:
            assert one[k].tobytes() == two[k].tobytes(), k


def test_unsupported_passes_are_rejected(gpu):
    """ECSEG_E_INVALID: a connectivity other than 4 / 8, AUX_IMAGE without an image, root lists at 4-connectivity (their capacity
    bounds 8-connected components only), flag queries after a count_only pass (it writes no flag words)."""
    img = cc.PATTERNS['noise30'](33, 65, 1)
    for kw in (dict(conn=6), dict(conn=0), dict(aux_mode=ref.AUX_IMAGE), dict(conn=4, need=ref.NEED_LISTS, lut=ref.LUT_MULTI),
               dict(count_only=True, need=ref.NEED_NCOMP, queries=[(0, 1)])):
        with pytest.raises(EcsegError) as e:
            gpu.ccl_pass(img, **kw)
        assert e.value.code == -1, kw
    got = gpu.ccl_pass(img, conn=8, need=ref.NEED_LISTS, lut=ref.LUT_MULTI, stat=ref.STAT_AREA)     # the same at 8: accepted
    assert got['nlist1'][0] == len(ref.Labelling(img, ref.LUT_MULTI, 8).list1)
