"""The ``meta_overlay`` row without a GPU: the oracle (oracle/overlay.py with oracle/postproc.py) pinned on the hand-written
rows of tests/overlay_cases.py, and the conditions that make the committed seeds of its generator worth running - every one
computed with the oracle alone.  The device is held to the same cases in tests/test_gpu_overlay.py."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import overlay_cases as cases                # noqa: E402
from oracle import postproc                  # noqa: E402

HAND = cases.hand_cases()


@pytest.fixture(scope='module')
def seeds():
    """seed -> (case, oracle row), computed once."""
    out = {}
    for seed in range(cases.N_SEEDS):
        case = cases.scene(seed)
        out[seed] = (case, cases.oracle_row(case))
    return out


@pytest.mark.parametrize('name', sorted(HAND))
def test_oracle_gives_the_hand_written_row(name):
    case, want = HAND[name]
    got = cases.oracle_row(case)
    assert cases.same_row(got, want), (got, want)


def test_quirk_batch_rows():
    labels, rgb, sens, thr, rows = cases.quirk_batch()
    for i, want in enumerate(rows):
        got = cases.oracle_row(cases._case(labels[i], rgb[i], sens, thr))
        assert cases.same_row(got, want), (i, got, want)


def test_same_row_tells_the_float_zero_from_the_integer():
    row = cases._row(ec=(1, 0.0))
    assert cases.same_row(row, cases._row(ec=(1, 0.0)))
    assert not cases.same_row(row, cases._row(ec=(1, 0)))
    assert not cases.same_row(row, cases._row(ec=(1, 0.0), hsr_g=1))


def test_hand_cases_cover_the_parameters_the_golden_rows_never_pass():
    thr = {c['thr'] for c, _ in HAND.values()}
    sens = {c['sens'] for c, _ in HAND.values()}
    chans = {c['rgb'].shape[2] for c, _ in HAND.values()}
    assert {0, 1, 2, 20, 73} <= thr and {0, 254, 255} <= sens and chans == {2, 3, 4}
    assert max(int(c['labels'].max()) for c, _ in HAND.values()) == 255


def test_generator_is_seeded_and_cycles_the_extents(seeds):
    for seed in (0, 5, 17):
        again = cases.scene(seed)
        assert all(np.array_equal(again[k], seeds[seed][0][k]) for k in ('labels', 'rgb'))
    assert {seeds[s][0]['labels'].shape for s in seeds} == set(cases.EXTENTS)
    assert {seeds[s][0]['sens'] for s in seeds} == set(cases.SENSITIVITIES)
    assert {seeds[s][0]['thr'] for s in seeds} == set(cases.THRESHOLDS)
    assert {seeds[s][0]['rgb'].shape[2] for s in seeds} == set(cases.CHANNELS)
    over = cases.scene(3, size=(7, 9), C=4, sens=30, thr=5)
    assert over['labels'].shape == (7, 9) and over['rgb'].shape == (7, 9, 4) and (over['sens'], over['thr']) == (30, 5)


def test_every_column_is_non_zero_in_five_seeds(seeds):
    hits = [0] * 9
    for _, row in seeds.values():
        for j, cell in enumerate(row):
            hits[j] += (cell[0] if j < 3 else cell) != 0
    assert min(hits) >= 5, hits


def _masks(case):
    labels, rgb, sens = case['labels'], case['rgb'], case['sens']
    red, green = rgb[..., 0] > sens, rgb[..., 1] > sens
    fish, fish2 = green & (labels != 1), red & (labels != 1)
    return labels == 2, labels == 3, fish, fish2


def test_each_quirk_occurs_in_a_seed_where_it_changes_the_row(seeds):
    ec_quirk = chrom_quirk = a_quirk = 0
    for case, _ in seeds.values():
        chrom, ec, fish, fish2 = _masks(case)
        kept = postproc.remove_small_objects4(fish2, case['thr']).any() or postproc.remove_small_objects4(fish, case['thr']).any()
        ec_quirk += bool(ec.all() and (fish.any() or fish2.any()))
        chrom_quirk += bool(chrom.all() and kept)
        a = fish & ~chrom
        a_quirk += bool(a.all() and (fish2 & ~chrom).any())
    assert ec_quirk >= 1 and chrom_quirk >= 1 and a_quirk >= 1, (ec_quirk, chrom_quirk, a_quirk)


def test_a_seed_has_fish_components_on_both_sides_of_its_threshold(seeds):
    """One below (area thr - 1: dropped) and one at or one above it (area thr or thr + 1: kept), under 4-connectivity, after
    the nucleus pixels have left."""
    both = 0
    for case, _ in seeds.values():
        thr = case['thr']
        if thr < 2:
            continue
        _, _, fish, fish2 = _masks(case)
        areas = set()
        for m in (fish, fish2):
            lab, n = postproc.label4(m)
            areas |= set(np.bincount(lab.ravel(), minlength=n + 1)[1:].tolist())
        both += (thr - 1) in areas and (thr in areas or thr + 1 in areas)
    assert both >= 1


def test_three_seeds_hold_label_bytes_above_3(seeds):
    assert sum(bool((case['labels'] > 3).any()) for case, _ in seeds.values()) >= 3


def test_three_seeds_hold_a_full_tile_of_chromosome_or_ec(seeds):
    def has_full_tile(labels):
        H, W = labels.shape
        for ty in range(H // cases.TILE_H):
            for tx in range(W // cases.TILE_W):
                t = labels[cases.TILE_H * ty:cases.TILE_H * (ty + 1), cases.TILE_W * tx:cases.TILE_W * (tx + 1)]
                if (t == 2).all() or (t == 3).all():
                    return True
        return False
    assert sum(has_full_tile(case['labels']) for case, _ in seeds.values()) >= 3


def test_batch_stacks_different_scenes_of_one_extent():
    labels, rgb, sens, thr = cases.batch(4, (65, 129))
    assert labels.shape == (4, 65, 129) and rgb.shape == (4, 65, 129, 3) and (sens, thr) == (85, 20)
    assert len({labels[i].tobytes() for i in range(4)}) == 4
