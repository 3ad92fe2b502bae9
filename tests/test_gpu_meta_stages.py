"""The clean-up stages of meta_inference on the device one at a time (``Handle.meta_inference_stages``: run_meta_inference of
csrc/meta_inference_kernels.hip with a range of stages) against the stage references of meta_stage_ref.py, byte for byte, on every image of
meta_stage_cases.py fed DIRECTLY to the stage: the final image of the whole chain, which test_gpu_post.py and test_gpu_fuzz.py
compare, can hide a stage's error behind the stages after it (test_meta_stages.py shows that it does)."""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import meta_stage_cases as mc        # noqa: E402
import meta_stage_ref as ref         # noqa: E402

from ecseg_amd._lib import EcsegError    # noqa: E402

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _want(k, ci, first, last):
    """Stages first..last of the reference on the batch of case ci of stage k's list: computed once, shared, read-only."""
    if first < last:
        out = np.stack([ref.stage(last, a) for a in _want(k, ci, first, last - 1)])
    else:
        out = np.stack([ref.stage(first, a) for a in mc.cases(k)[ci].x])
    out.setflags(write=False)
    return out


def _same(got, want, what):
    assert got.dtype == np.uint8 and got.shape == want.shape, what
    if not np.array_equal(got, want):
        bad = np.argwhere(got != want)
        raise AssertionError('%s: %d pixels differ, first at (image, y, x) = %s: got %d, want %d'
                             % (what, len(bad), tuple(bad[0]), got[tuple(bad[0])], want[tuple(bad[0])]))


@pytest.mark.parametrize('k', ref.STAGES)
def test_single_stage_equals_reference(gpu, k):
    """Every case of the stage's list, no tolerance; stage 4 also the per-pixel decision of the nucleus test."""
    for ci, case in enumerate(mc.cases(k)):
        if k == 4:
            got, kill = gpu.meta_inference_stages(case.x, 4, 4, want_kill=True)
            _same(kill, np.stack([ref.kill_mask(a) for a in case.x]), ('kill', case.name))
        else:
            got = gpu.meta_inference_stages(case.x, k, k)
        _same(got, _want(k, ci, k, k), (k, case.name))


@pytest.mark.parametrize('k', ref.STAGES)
def test_prefixes_and_suffixes_equal_the_chained_reference(gpu, k):
    """Ranges 1..k and k..6 on stage k's list; 1..6 is the production call."""
    for ci, case in enumerate(mc.cases(k)):
        _same(gpu.meta_inference_stages(case.x, 1, k), _want(k, ci, 1, k), ('1..%d' % k, case.name))
        _same(gpu.meta_inference_stages(case.x, k, 6), _want(k, ci, k, 6), ('%d..6' % k, case.name))
        if k == 6:
            prod, nec = gpu.meta_inference(case.x)
            _same(prod, _want(k, ci, 1, 6), ('production', case.name))
            for i, a in enumerate(case.x):
                assert np.array_equal(_want(k, ci, 1, 6)[i], ref.P.meta_inference(a)), (case.name, i)
                assert int(nec[i]) == ref.P.count_cc(prod[i] == 3)[0], (case.name, i)


def test_single_images_equal_the_batch(gpu):
    """A 2-D image goes as a batch of one: image 1 of each extent's batch alone, through every stage."""
    for k in ref.STAGES:
        for ci, case in enumerate(mc.cases(k)):
            if case.name.startswith('extent_'):
                _same(gpu.meta_inference_stages(case.x[1], k, k), _want(k, ci, k, k)[1], (k, case.name, 'alone'))


@pytest.mark.parametrize('k', ref.STAGES)
def test_v4_pair_agrees_away_from_the_cut(gpu, k):
    """(66, 132) runs the 32-bit-load twins of the fused kernels and the 4-pixel nucleus kill, (66, 131) - the same images without
    their empty last column - the bytewise ones.  Both equal the reference in full; restricted to the columns further than
    PAIR_FOOTPRINT[k] from the cut (the reach of the stage's stencils: 1 for the band's erosion, 2 for the opening, 3 with the final
    dilation, 0 where a stage has no stencil) they equal each other."""
    wide, narrow = mc.extent_batch(*mc.V4_PAIR[0]), mc.extent_batch(*mc.V4_PAIR[1])
    gw, gn = gpu.meta_inference_stages(wide, k, k), gpu.meta_inference_stages(narrow, k, k)
    _same(gw, np.stack([ref.stage(k, a) for a in wide]), (k, 'wide'))
    _same(gn, np.stack([ref.stage(k, a) for a in narrow]), (k, 'narrow'))
    keep = narrow.shape[2] - mc.PAIR_FOOTPRINT[k]
    _same(np.ascontiguousarray(gw[:, :, :keep]), np.ascontiguousarray(gn[:, :, :keep]), (k, 'pair'))


def test_stale_workspace_is_not_read(gpu):
    """A dense whole-chain call leaves parents, slots, flag words, lists and both scratch images full; then every single stage on a
    sparser image of the same extent equals the reference."""
    H, W = 96, 200
    rng = np.random.default_rng(99)
    dense = rng.integers(1, 4, (2, H, W)).astype(np.uint8)
    sparse = mc.extent_batch(H, W)[:2].copy()
    sparse[:, 32:64, 64:128] = 0
    sparse[:, 0:32, 128:192] = 0
    want_dense = np.stack([ref.chain(1, 6, a) for a in dense])
    for k in ref.STAGES:
        _same(gpu.meta_inference_stages(dense, 1, 6), want_dense, ('dense', k))
        got, kill = gpu.meta_inference_stages(sparse, k, k, want_kill=True)
        _same(got, np.stack([ref.stage(k, a) for a in sparse]), ('sparse after dense', k))
        _same(kill, np.stack([ref.kill_mask(a) for a in sparse]) if k == 4 else np.zeros_like(sparse), ('kill after dense', k))


def test_two_calls_return_identical_bytes(gpu):
    ci = next(i for i, c in enumerate(mc.cases(1)) if c.x.shape[1:] == (96, 200))
    x = mc.cases(1)[ci].x
    for first, last in [(k, k) for k in ref.STAGES] + [(1, 6), (2, 5)]:
        one = gpu.meta_inference_stages(x, first, last, want_kill=True)
        two = gpu.meta_inference_stages(x, first, last, want_kill=True)
        assert one[0].tobytes() == two[0].tobytes() and one[1].tobytes() == two[1].tobytes(), (first, last)


def test_bad_ranges_are_refused(gpu):
    x = mc.extent_batch(33, 65)
    for first, last in ((0, 3), (1, 7), (4, 3), (7, 7), (-1, -1), (0, 0), (6, 1)):
        with pytest.raises(EcsegError) as e:
            gpu.meta_inference_stages(x, first, last)
        assert e.value.code == -1, (first, last)
    _same(gpu.meta_inference_stages(x, 3, 3), np.stack([ref.stage(3, a) for a in x]), 'after the refusals')   # the handle still works
    _same(gpu.meta_inference(x)[0], np.stack([ref.chain(1, 6, a) for a in x]), 'production after the refusals')
