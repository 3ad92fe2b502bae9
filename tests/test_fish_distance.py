"""fish_distance_calculation without a GPU: the CPU oracle tests/fish_distance_ref.py on hand-computed cases, the host
arithmetic of ecseg_amd/fish_distance_calculation.py against that oracle bit for bit, the CSV text against pandas, and
``main()`` with a stub handle that answers from the oracle's records."""
import math
import os
import re
import sys

import numpy as np
import pytest
import yaml

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fish_distance_cases as cases          # noqa: E402
import fish_distance_ref as ref              # noqa: E402
from ecseg_amd import csvio, image_io        # noqa: E402
from ecseg_amd import fish_distance_calculation as fdc   # noqa: E402
from ecseg_amd.interseg import ImageError    # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HAND = cases.hand_cases()


class StubHandle:
    """Answers Handle.fish_distances from the vectorised oracle; remembers what it was asked."""
    def __init__(self):
        self.calls = []

    def fish_distances(self, labels, lsq, fish_channel, centromere_channel, capacity=4096):
        assert labels.dtype == np.int32 and labels.flags.c_contiguous and lsq.dtype == np.uint8
        assert labels.size == 0 or int(labels.max()) <= labels.size, 'labels above H * W must be remapped on the host'
        self.calls.append((labels.copy(), fish_channel, centromere_channel))
        return ref.records(lsq, labels, fish_channel, centromere_channel)


def _hex(values):
    return [float(v).hex() for v in values]


# ---- the oracle itself -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', sorted(HAND))
def test_loop_on_hand_computed_cases(name):
    lsq, seg, presets, want = HAND[name]
    got = ref.loop(lsq, seg, presets)
    assert _hex(got) == _hex(want), (got, want)


def test_hand_cases_reach_every_rule():
    """Every rule has a case that yields a value and one that yields none, named by what it checks."""
    names = set(HAND)
    assert HAND['triangle_3_4_5'][3] == [0.625]
    for rule in ('triangle_3_4_5', 'pixel_of_both_colours', 'same_colour_red', 'gate_fails_on_channel_0', 'gate_fails_on_channel_1',
                 'exactly_max_spots', 'max_plus_one_spots', 'diagonal_touch_is_one_spot', 'two_spots_over_a_limit_of_one',
                 'nearer_centromere_of_the_neighbour_is_ignored', 'spot_across_the_border_counts_once_per_cell',
                 'blue_fish_probe_is_empty', 'label_of_two_blobs_and_gaps_and_negatives'):
        assert rule in names, rule
    outcomes = {name: len(c[3]) for name, c in HAND.items()}
    assert any(v == 0 for v in outcomes.values()) and any(v == 2 for v in outcomes.values())
    assert any(c[3] == [float('inf')] for c in HAND.values()) and any(c[3] == [0.0] for c in HAND.values())


def test_loop_raises_where_the_reference_dies():
    lsq, seg, _, _ = HAND['triangle_3_4_5']
    with pytest.raises(ValueError):
        ref.loop(lsq, seg, (2, 0, 3))                        # blue centromere probe, empty: .min() of an empty array


@pytest.mark.parametrize('name', sorted(HAND))
def test_records_on_hand_computed_cases(name):
    lsq, seg, (ci, fi, mx), want = HAND[name]
    assert _hex(fdc.distances_from_records(ref.records(lsq, seg, fi, ci), mx)) == _hex(want)


def test_record_fields_of_a_known_cell():
    lsq, seg, _, _ = HAND['label_of_two_blobs_and_gaps_and_negatives']
    assert ref.records(lsq, seg, 0, 1).tolist() == [[2, 1, 3, 1, 1, 1, 0, 0], [7, 18, 3, 1, 1, 1, 128, 0]]
    lsq, seg, _, _ = HAND['spot_across_the_border_counts_once_per_cell']
    assert ref.records(lsq, seg, 0, 1).tolist() == [[1, 36, 3, 3, 1, 2, 2, 0], [2, 36, 3, 3, 1, 2, 25, 0]]
    assert ref.records(lsq, seg, 2, 1).tolist() == [[1, 36, 3, 0, 1, 0, -1, 0], [2, 36, 3, 0, 1, 0, -1, 0]]


# ---- host arithmetic against the reference's float arithmetic --------------------------------------------------------
def test_distances_from_records_equal_the_loop_bit_for_bit_on_random_scenes():
    """The square root of the exact integer minimum over sqrt(area) against np.linalg.norm(...).min() / np.sqrt(area)."""
    n_values = 0
    tally = np.zeros(5, int)
    for seed in range(220):
        lsq, seg = cases.scene(seed, size=cases.SCENE_SIZES[seed % len(cases.SCENE_SIZES)] if seed % 3 else (48, 60))
        ci, fi = (1, 0) if seed % 2 else (0, 1)
        want = ref.loop(lsq, seg, (ci, fi, cases.MAX_SPOTS))
        got = fdc.distances_from_records(ref.records(lsq, seg, fi, ci), cases.MAX_SPOTS)
        assert _hex(got) == _hex(want), seed
        n_values += len(want)
        tally += cases.outcomes(lsq, seg, fi, ci, cases.MAX_SPOTS, ref.records)
    assert n_values >= 400 and (tally[:4] >= 20).all(), (n_values, tally)


def test_distances_from_records_rules():
    rec = [[1, 4, 3, 0, 0, 0, -1, 0],       # no FISH pixel: inf
           [2, 4, 1, 5, 5, 1, 0, 0],        # gate
           [3, 4, 2, 5, 5, 1, 0, 0],
           [4, 4, 3, 5, 5, 4, 9, 0],        # spots > 3
           [5, 4, 3, 5, 5, 3, 9, 0],
           [6, 16, 3, 1, 1, 1, 0, 0]]
    assert fdc.distances_from_records(rec, 3) == [float('inf'), 1.5, 0.0]
    assert fdc.distances_from_records(rec, 4) == [float('inf'), 1.5, 1.5, 0.0]
    assert fdc.distances_from_records(np.zeros((0, 8), np.int64), 3) == []
    with pytest.raises(ImageError, match='no centromere pixel'):
        fdc.distances_from_records([[9, 4, 3, 2, 0, 1, -1, 0]], 3)
    assert fdc.distances_from_records([[9, 4, 3, 2, 0, 4, -1, 0]], 3) == []        # skipped before the reference reaches .min()


def test_csv_text_equals_pandas():
    import pandas as pd
    values = [float('inf'), 0.0, 1e-05, 0.625, math.sqrt(2) / math.sqrt(36), math.sqrt(5) / math.sqrt(4103), 1 / 3, 123456.789e3]
    for seed in range(20):
        lsq, seg = cases.scene(seed)
        values += ref.loop(lsq, seg, (1, 0, cases.MAX_SPOTS))
    for vals in (values, []):
        want = pd.DataFrame({'normalized_distance': vals}).to_csv(index=False)
        assert csvio.csv_text(fdc.CSV_COLUMNS, [[v] for v in vals]) == want
    assert csvio.csv_text(fdc.CSV_COLUMNS, []) == 'normalized_distance\n'


# ---- get_distances_img --------------------------------------------------------------------------------------------------
def test_get_distances_img_remaps_labels_above_the_pixel_count():
    lsq, seg, presets, want = HAND['label_of_two_blobs_and_gaps_and_negatives']
    mid = np.where(seg == 7, 5000, np.where(seg == 2, 900, seg))                    # above H * W = 81, small enough for the loop
    big = np.where(seg == 7, 10 ** 12, np.where(seg == 2, 10 ** 6, seg))            # labels far above what fits int32
    h = StubHandle()
    assert _hex(fdc.get_distances_img(lsq, mid, presets, h)) == _hex(want) == _hex(ref.loop(lsq, mid, presets))
    assert _hex(fdc.get_distances_img(lsq, big, presets, StubHandle())) == _hex(want)
    assert sorted(np.unique(h.calls[0][0]).tolist()) == [0, 1, 2] and h.calls[0][1:] == (0, 1)
    assert _hex(fdc.get_distances_img(lsq, seg, presets, h)) == _hex(want)
    assert sorted(np.unique(h.calls[1][0]).tolist()) == [0, 2, 7]                   # labels that fit are sent as they are
    assert _hex(fdc.get_distances_img(lsq, big.astype(np.uint64) * (big > 0), presets, h)) == _hex(want)


@pytest.mark.parametrize('what', ['float_map', 'map_3d', 'lsq_gray', 'lsq_u16', 'two_channels_blue', 'shape'])
def test_get_distances_img_refuses(what):
    lsq, seg, presets, _ = HAND['triangle_3_4_5']
    if what == 'float_map':
        seg = seg.astype(float)
    elif what == 'map_3d':
        seg = seg[None]
    elif what == 'lsq_gray':
        lsq = lsq[..., 0]
    elif what == 'lsq_u16':
        lsq = lsq.astype(np.uint16)
    elif what == 'two_channels_blue':
        lsq, presets = lsq[..., :2], (2, 0, 3)
    else:
        seg = seg[:-1]
    with pytest.raises(ImageError):
        fdc.get_distances_img(lsq, seg, presets, StubHandle())


def test_get_distances_img_two_channels_suffice_for_red_and_green():
    lsq, seg, presets, want = HAND['triangle_3_4_5']
    assert _hex(fdc.get_distances_img(np.ascontiguousarray(lsq[..., :2]), seg, presets, StubHandle())) == _hex(want)


# ---- main() -----------------------------------------------------------------------------------------------------------
def _rgb_tiff(path, img):
    from PIL import Image
    Image.fromarray(img).save(str(path), compression='tiff_lzw')


def _add(inp, name, lsq, seg, dtype=np.int64, lsq_suffix='_lsq_thresh'):
    image_io.write_tiff_gray8(str(inp / (name + '.tif')), np.zeros((4, 4), np.uint8))     # never opened
    d = inp / 'annotated' / name
    d.mkdir(parents=True)
    if seg is not None:
        np.save(str(d / (name + '__segmentation_min_cut.npy')), seg.astype(dtype))
    if lsq is not None:
        _rgb_tiff(d / (name + lsq_suffix + '.tif'), lsq)


def _config(tmp_path, monkeypatch, **over):
    var = {'inpath': str(tmp_path / 'in'), 'centromere_probe_color': 'green', 'fish_probe_color': 'red', 'max_centromeric_spots': 3}
    var.update(over)
    yaml.safe_dump({'fish_distance_calculation': var, 'metaseg': {'inpath': 'x'}}, open(tmp_path / 'config.yaml', 'w'))
    monkeypatch.chdir(tmp_path)


def _run(expect_code=None):
    if expect_code is None:
        fdc.main([], handle=StubHandle())
        return
    with pytest.raises(SystemExit) as e:
        fdc.main([], handle=StubHandle())
    assert e.value.code == expect_code


def _csv(tmp_path):
    return open(tmp_path / 'in' / 'centromere_distances.csv').read()


def _expected_csv(scenes, presets):
    vals = []
    for lsq, seg in scenes:
        vals += ref.loop(lsq, seg, presets)
    return csvio.csv_text(['normalized_distance'], [[v] for v in vals])


def test_main_writes_the_csv_in_sorted_image_order(tmp_path, monkeypatch, capsys):
    inp = tmp_path / 'in'
    (inp / 'annotated').mkdir(parents=True)
    scenes = {name: cases.scene(k, size=(60, 80)) for k, name in enumerate(['b_img', 'a_img', 'c.img'])}
    for name, (lsq, seg) in scenes.items():
        _add(inp, name, lsq, seg, dtype=np.int32 if name == 'a_img' else np.int64)
    _rgb_tiff(inp / 'annotated' / 'a_img' / 'a_img_lsq_zzz.tif', scenes['b_img'][0])         # a second match: the first in sorted order is read
    (inp / 'notes.txt').write_text('ignored')
    np.save(str(inp / 'ignored.npy'), np.zeros((3, 3)))
    _config(tmp_path, monkeypatch)
    _run()
    want = _expected_csv([scenes['a_img'], scenes['b_img'], scenes['c.img']], (1, 0, 3))
    assert _csv(tmp_path) == want and want.count('\n') > 10
    _config(tmp_path, monkeypatch, centromere_probe_color='Red', fish_probe_color='GREEN', max_centromeric_spots=1)
    _run()
    assert _csv(tmp_path) == _expected_csv([scenes['a_img'], scenes['b_img'], scenes['c.img']], (0, 1, 1))


def test_main_header_only_csv_for_a_folder_without_tif(tmp_path, monkeypatch):
    (tmp_path / 'in' / 'annotated').mkdir(parents=True)
    _config(tmp_path, monkeypatch)
    _run()
    assert _csv(tmp_path) == 'normalized_distance\n'


@pytest.mark.parametrize('what', ['no_inpath', 'no_annotated', 'colour', 'colour_fish', 'spots_float', 'spots_text', 'spots_bool'])
def test_main_exit_code_2(tmp_path, monkeypatch, capsys, what):
    if what != 'no_inpath':
        (tmp_path / 'in').mkdir()
    if what not in ('no_inpath', 'no_annotated'):
        (tmp_path / 'in' / 'annotated').mkdir()
    over = {'colour': {'centromere_probe_color': 'yellow'}, 'colour_fish': {'fish_probe_color': 3},
            'spots_float': {'max_centromeric_spots': 2.5}, 'spots_text': {'max_centromeric_spots': 'three'},
            'spots_bool': {'max_centromeric_spots': True}}.get(what, {})
    _config(tmp_path, monkeypatch, **over)
    _run(2)
    assert capsys.readouterr().out.strip() and not os.path.exists(tmp_path / 'in' / 'centromere_distances.csv')


@pytest.mark.parametrize('what', ['no_folder', 'no_npy', 'float_npy', 'npy_3d', 'pickled_npy', 'no_lsq', 'broken_lsq', 'gray_lsq', 'two_channel_lsq', 'shape',
                                  'empty_centromere'])
def test_main_per_image_failure_keeps_the_other_rows(tmp_path, monkeypatch, capsys, what):
    inp = tmp_path / 'in'
    (inp / 'annotated').mkdir(parents=True)
    good_a, good_z = cases.scene(3, size=(50, 70)), cases.scene(4, size=(40, 40))
    _add(inp, 'a_good', *good_a)
    _add(inp, 'z_good', *good_z)
    lsq, seg = cases.scene(5, size=(30, 30))
    over = {}
    if what == 'no_folder':
        image_io.write_tiff_gray8(str(inp / 'm_bad.tif'), np.zeros((4, 4), np.uint8))
    elif what == 'no_npy':
        _add(inp, 'm_bad', lsq, None)
    elif what == 'float_npy':
        _add(inp, 'm_bad', lsq, seg, dtype=np.float64)
    elif what == 'npy_3d':
        _add(inp, 'm_bad', lsq, seg[None])
    elif what == 'pickled_npy':
        _add(inp, 'm_bad', lsq, None)
        np.save(str(inp / 'annotated' / 'm_bad' / 'm_bad__segmentation_min_cut.npy'), np.array([{'a': 1}], dtype=object), allow_pickle=True)
    elif what == 'no_lsq':
        _add(inp, 'm_bad', None, seg)
    elif what == 'broken_lsq':
        _add(inp, 'm_bad', None, seg)
        (inp / 'annotated' / 'm_bad' / 'm_bad_lsq.tif').write_bytes(b'II*\0 not a tiff')
    elif what == 'gray_lsq':
        _add(inp, 'm_bad', None, seg)
        image_io.write_tiff_gray8(str(inp / 'annotated' / 'm_bad' / 'm_bad_lsq.tif'), lsq[..., 0])
    elif what == 'two_channel_lsq':                         # a blue probe needs channel 2; the other images have three channels
        _add(inp, 'm_bad', None, seg)
        from PIL import Image
        Image.fromarray(np.ascontiguousarray(lsq[..., :2]), 'LA').save(str(inp / 'annotated' / 'm_bad' / 'm_bad_lsq.tif'), compression='tiff_lzw')
        assert image_io.imread(str(inp / 'annotated' / 'm_bad' / 'm_bad_lsq.tif')).shape == lsq.shape[:2] + (2,)
        over = {'fish_probe_color': 'blue'}
    elif what == 'shape':
        _add(inp, 'm_bad', lsq[:-1], seg)
    else:                                                    # blue centromere probe: FISH pixels, no centromere pixel, gate passes
        l2, s2, _, _ = HAND['triangle_3_4_5']
        _add(inp, 'm_bad', l2, s2)
        over = {'centromere_probe_color': 'blue'}
        for l, _ in (good_a, good_z):
            l[..., 2] = 255
        for name, (l, s) in (('a_good', good_a), ('z_good', good_z)):
            _rgb_tiff(inp / 'annotated' / name / (name + '_lsq_thresh.tif'), l)
    _config(tmp_path, monkeypatch, **over)
    _run(1)
    out = capsys.readouterr().out
    assert 'm_bad.tif' in out and '1 image(s) were NOT processed' in out
    presets = (2, 0, 3) if what == 'empty_centromere' else (1, 2, 3) if what == 'two_channel_lsq' else (1, 0, 3)
    if what == 'two_channel_lsq':
        assert 'channel' in out
    want = _expected_csv([good_a, good_z], presets)
    assert _csv(tmp_path) == want and want.count('\n') > 3


# ---- the surface of the target ------------------------------------------------------------------------------------------
def test_config_has_the_reference_fish_distance_section():
    var = yaml.safe_load(open(os.path.join(ROOT, 'config.yaml')))['fish_distance_calculation']
    assert var == {'inpath': '../images', 'centromere_probe_color': 'green', 'fish_probe_color': 'red', 'max_centromeric_spots': 3}
    assert re.search(r'^fish_distance_calculation: build\n\tpython src/fish_distance_calculation.py$',
                     open(os.path.join(ROOT, 'Makefile')).read(), re.M)
    assert os.path.exists(os.path.join(ROOT, 'src', 'fish_distance_calculation.py'))


def test_entry_point_is_declared_and_exported():
    import ctypes
    from ecseg_amd._lib import ABI_VERSION, EXPORTS, LIB_PATH
    header = open(os.path.join(ROOT, 'include', 'ecseg_hip.h')).read()
    assert re.search(r'\becseg_fish_distances\s*\(', header) and 'ecseg_fish_distances' in EXPORTS
    assert ABI_VERSION == 6 and '#define ECSEG_ABI_VERSION 6' in header
    from ecseg_amd import build
    assert 'fishdist_kernels.hip' in build.SOURCES
    if os.path.exists(LIB_PATH):
        assert ctypes.CDLL(LIB_PATH).ecseg_fish_distances


def test_the_new_kernels_are_in_the_shipped_library():
    """The unchanged spill test of test_host_cpu.py covers every kernel of the library; this pins that the new ones are among them."""
    from ecseg_amd._lib import LIB_PATH
    blob = open(LIB_PATH, 'rb').read()
    for name in (b'fd_mark_kernel', b'fd_cell_stats_kernel', b'fd_fill_unite_kernel', b'fd_distance_kernel', b'scan_chunk_sum_kernel',
                 b'scan_blocks_kernel', b'scan_chunk_excl_kernel'):
        assert name in blob, name
