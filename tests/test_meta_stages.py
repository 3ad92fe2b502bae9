"""Host tests for the tests of the clean-up stages one at a time: the stage references (meta_stage_ref.py) chain to the oracle's
meta_inference, the case list (meta_stage_cases.py) tells every mutant of a stage from the oracle, every hand case takes the
branch it is named for - and, on record, some stage errors that these cases catch at the stage are repaired by the stages behind
it, so that the final image of the chain cannot show them."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import meta_stage_cases as mc        # noqa: E402
import meta_stage_ref as ref         # noqa: E402

from oracle import postproc          # noqa: E402


def test_entry_point_is_registered_as_an_addition_to_abi_5():
    from ecseg_amd import _lib
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'ecseg_hip.h')).read()
    assert 'still 5 - additive: ecseg_meta_inference_stages_debug' in hdr and '#define ECSEG_ABI_VERSION 6' in hdr and _lib.ABI_VERSION == 6
    assert 'ecseg_meta_inference_stages_debug' in _lib.EXPORTS and hasattr(_lib.Handle, 'meta_inference_stages')


def _images(k):
    for case in mc.cases(k):
        for i in range(case.x.shape[0]):
            yield case, i, case.x[i]


@pytest.mark.parametrize('k', ref.STAGES)
def test_chained_stages_equal_meta_inference_on_every_case(k):
    """Every image of every stage's list, taken as a raw label image: stage(1..6) in a row is the oracle's meta_inference."""
    for case, i, img in _images(k):
        assert np.array_equal(ref.chain(1, 6, img), postproc.meta_inference(img)), (case.name, i)


@pytest.mark.parametrize('k', ref.STAGES)
def test_restated_variant_with_every_switch_off_equals_the_stage(k):
    """A mutant differs from the oracle by its switch alone."""
    for case, i, img in _images(k):
        assert np.array_equal(ref.UNMUTATED[k](img), ref.stage(k, img)), (case.name, i)
        assert img.dtype == np.uint8 and img.max() <= 3


def test_case_list_has_the_extents_batches_and_the_pair():
    for k in ref.STAGES:
        cs = mc.cases(k)
        assert len({c.name for c in cs}) == len(cs)
        shapes = {c.x.shape[1:] for c in cs}
        assert set(mc.EXTENTS) <= shapes and all(c.x.flags.c_contiguous for c in cs)
        # batches of different images (a wrong image index cannot hide behind equal images) at more than two sizes
        multi = [c for c in cs if c.x.shape[0] >= 3 and c.x.shape[1:] != (1, 1)]
        assert len({c.x.shape[1:] for c in multi}) >= 2
        for c in multi:
            assert len({c.x[i].tobytes() for i in range(c.x.shape[0])}) == c.x.shape[0], c.name
        # every image at most 96 x 200, but the strips of stage 4
        big = [c.name for c in cs if c.x.shape[1] * c.x.shape[2] > 96 * 200]
        assert big == (['strip_pair_test'] if k == 4 else []), big
        assert len(mc.hand_cases(k)) >= 5
    assert {c.x.shape[1:] for c in mc.cases(4)} >= {mc.PAIR_STRIP, mc.BINNED_STRIP}
    wide, narrow = mc.extent_batch(*mc.V4_PAIR[0]), mc.extent_batch(*mc.V4_PAIR[1])
    assert wide.shape[2] % 4 == 0 and narrow.shape[2] % 4 != 0 and np.array_equal(wide[:, :, :-1], narrow) and not wide[:, :, -1].any()
    for hw in mc.FUZZ_EXTENTS:                               # the generator of test_gpu_fuzz.py itself, not a copy
        rng = np.random.default_rng(8000 + 1000 * hw[0] + hw[1])
        import test_gpu_fuzz
        assert np.array_equal(mc.fuzz_batch(*hw)[0], test_gpu_fuzz._random_labels(rng, *hw))


@pytest.mark.parametrize('k', ref.STAGES)
def test_v4_pair_agrees_away_from_the_cut_on_the_oracle(k):
    """What test_gpu_meta_stages.py asks of the device holds for the reference: with the wide image's last column empty, stage k
    on the wide and on the cropped image agree at every column further than PAIR_FOOTPRINT[k] from the cut."""
    wide, narrow = mc.extent_batch(*mc.V4_PAIR[0]), mc.extent_batch(*mc.V4_PAIR[1])
    keep = narrow.shape[2] - mc.PAIR_FOOTPRINT[k]
    for i in range(wide.shape[0]):
        assert np.array_equal(ref.stage(k, wide[i])[:, :keep], ref.stage(k, narrow[i])[:, :keep]), i


@pytest.mark.parametrize('k', ref.STAGES)
def test_every_hand_case_takes_the_branch_it_is_named_for(k):
    for case in mc.hand_cases(k):
        assert case.check(case.x), case.name


def _mutant_table():
    """Per mutant: the images of its stage's list on which the stage output differs from the oracle's (killed at the stage), and
    those of them on which the final image of the chain differs too (visible at the end)."""
    rows = []
    for k, name in ref.mutant_names():
        fn = ref.MUTANTS[k][name]
        n = killed = visible = 0
        for case, i, img in _images(k):
            n += 1
            good, bad = ref.stage(k, img), fn(img)
            if not np.array_equal(good, bad):
                killed += 1
                visible += int(not np.array_equal(ref.chain(k + 1, 6, good), ref.chain(k + 1, 6, bad)))
        rows.append((k, name, n, killed, visible))
    return rows


@pytest.fixture(scope='module')
def mutant_table():
    rows = _mutant_table()
    print('\nstage  mutant                              images  killed at the stage  visible at the end of the chain  masked')
    for k, name, n, killed, visible in rows:
        print('%5d  %-34s  %6d  %19d  %31d  %6d' % (k, name, n, killed, visible, killed - visible))
    return rows


def test_every_mutant_is_killed_by_a_case_of_its_stage(mutant_table):
    unkilled = [(k, name) for k, name, _, killed, _ in mutant_table if killed == 0]
    assert not unkilled, 'no case tells these from the oracle: %s' % unkilled


def test_later_stages_mask_stage_errors_on_these_cases(mutant_table):
    """The reason for testing stage by stage, on record: for some stage-3 / stage-5 mutant there are committed cases on which the
    stage output is wrong and the final image of the chain is not."""
    masked = {(k, name): killed - visible for k, name, _, killed, visible in mutant_table if k in (3, 5)}
    assert len(masked) == len(ref.MUTANTS[3]) + len(ref.MUTANTS[5])
    assert max(masked.values()) > 0, masked
