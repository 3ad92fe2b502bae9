"""The third FISH probe (aqua) of ``make stat_fish`` without a GPU: the restatement tests/aqua_ref.py pinned on exhaustive inputs
against the closed forms ecseg_fish_render documents, ``main()`` on a folder that mixes four-channel ``.npy`` images with a
three-channel TIFF (CSV text with the aqua columns and the empty fields, the three colour files, the ``aq`` file name), the numpy
path against a handle that offers ``fish_render``, and ``make fish_distance_calculation`` on what the run leaves behind."""
import os
import sys

import numpy as np
import pytest
import yaml

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import aqua_ref                              # noqa: E402
import fish_distance_ref as fd_ref           # noqa: E402
import stat_fish_cases as cases              # noqa: E402
import stat_fish_ref as ref                  # noqa: E402
from ecseg_amd import _lib, csvio, image_io  # noqa: E402
from ecseg_amd import fish_distance_calculation as fdc   # noqa: E402
from ecseg_amd import stat_fish as sf        # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COLUMNS_3 = ['image_name', 'nucleus_center',
             '#_FISH_pixels (green)', '#_FISH_foci (green)', 'Avg fish intensity (green)', 'Max fish intensity (green)',
             '#_FISH_pixels (red)', '#_FISH_foci (red)', 'Avg fish intensity (red)', 'Max fish intensity (red)',
             '#_FISH_pixels (aqua)', '#_FISH_foci (aqua)', 'Avg fish intensity (aqua)', 'Max fish intensity (aqua)',
             '#_DAPI_pixels', '#_FISH_pixels (green and red)', '#_FISH_foci (green and red)']
TAG = 'n15_std3.00_s7_g70.0_r70.0_aq70.0'
# the aqua values at which the uint8 wrap of merge_channels adds 1 to green / to red: (k * q) & 255 == 255 (none exists for blue's 54)
Q_GREEN = next(q for q in range(256) if (137 * q) & 255 == 255)
Q_RED = next(q for q in range(256) if (233 * q) & 255 == 255)
SEEDS = (12, 19, 40)                             # scenes of tests/stat_fish_cases.py with nuclei and no ambiguous pixel at 70 x 90
ORDER = ('b_tif', 'a_u16', 'c_u8')               # get_imgs: the TIFFs, then the .npy files, each sorted


class OracleHandle:
    """What ``main`` needs of a ``_lib.Handle``, computed by the oracle tests/stat_fish_ref.py; it has no ``fish_render``."""

    def __init__(self):
        self.calls = []

    def ccl_labels(self, mask, connectivity=8):
        assert connectivity == 8
        return ref.nuclei(mask).astype(np.int32)

    def u16_to_u8(self, a):
        return np.floor(np.asarray(a, np.float64) * (255.0 / 65535.0) + 0.5).astype(np.uint8)

    def fish_spots(self, labels, img, probes, weights, normal, ithr, min_cc, line, capacity=4096):
        self.calls.append(dict(probes=tuple(probes), ithr=tuple(ithr), channels=img.shape[2]))
        rec, thr, bnd, _ = ref.loop(img, labels, probes, np.asarray(weights, np.float64), normal, ithr, min_cc, line)
        return rec, thr, bnd


class RenderingOracleHandle(OracleHandle):
    """The same with a ``fish_render``, answered by the restatement tests/aqua_ref.py."""

    def fish_render(self, img, channels, thresholded, boundaries):
        self.calls.append(dict(render=tuple(channels)))
        return aqua_ref.files(np.ascontiguousarray(img[..., list(channels)]), thresholded, boundaries)


def four_channel_scene(seed, size=(70, 90)):
    """-> ((H, W, 4) uint8 BGRA image, 0 / 255 mask): a three-probe scene of tests/stat_fish_cases.py with blue in channel 0 and
    the probes in 1, 2, 3; a few aqua pixels hold the two values at which the reference's uint8 wrap shows, beside a saturated and
    an ordinary colour value."""
    case = cases.scene(seed, size=size, K=7, n_probe=3)
    rng = np.random.default_rng(seed)
    img = np.empty(size + (4,), np.uint8)
    img[..., 0] = rng.integers(0, 200, size)
    for j, c in enumerate(case['probes']):
        img[..., 1 + j] = case['img'][..., c]
    img[0, :4, 3] = (Q_GREEN, Q_RED, Q_GREEN, Q_RED)
    img[0, :4, :3] = ((7, 255, 8), (9, 10, 255), (0, 11, 12), (13, 14, 15))
    return img, (case['seg'] > 0).astype(np.uint8) * np.uint8(255)


def make_folder(tmp_path, kinds=(('c_u8', 'npy8'), ('a_u16', 'npy16'), ('b_tif', 'tif')), size=(70, 90), color_sensitivity=(70, 70, 70)):
    """A stat_fish input folder under tmp_path / 'in' with config.yaml and src/stat_fish_params.yaml beside it -> (folder, {name:
    (uint8 image as the reference indexes it: BGR(A), mask)})."""
    inp = tmp_path / 'in'
    (inp / 'nuclei_masks').mkdir(parents=True, exist_ok=True)
    scenes = {}
    for k, (name, kind) in enumerate(kinds):
        img, mask = four_channel_scene(SEEDS[k], size)
        if kind == 'npy8':
            np.save(inp / (name + '.npy'), img)
        elif kind == 'npy16':
            np.save(inp / (name + '.npy'), img.astype(np.uint16) * 257)       # u16_to_u8 gives the 8-bit values back
        else:
            img = np.ascontiguousarray(img[..., :3])
            image_io.write_tiff_rgb8(str(inp / (name + '.tif')), np.ascontiguousarray(img[..., ::-1]))
        image_io.write_tiff_gray8(str(inp / 'nuclei_masks' / (name + '.tif')), mask)
        scenes[name] = (img, mask)
    yaml.safe_dump({'stat_fish': dict(inpath=str(inp), scale=1, use_min_cut=False, nuclei_size_T=5000),
                    'fish_distance_calculation': dict(inpath=str(inp), centromere_probe_color='green', fish_probe_color='red',
                                                      max_centromeric_spots=3)}, open(tmp_path / 'config.yaml', 'w'))
    os.makedirs(tmp_path / 'src', exist_ok=True)
    (tmp_path / 'src' / 'stat_fish_params.yaml').write_text('color_sensitivity: [%s]\n' % ', '.join(str(v) for v in color_sensitivity))
    return inp, scenes


def expected(name, img, mask):
    """Rows (laid out as COLUMNS_3) and the three colour files of one image from the oracle and the restatement alone."""
    lab = ref.nuclei(mask)
    probes = tuple(range(1, img.shape[2]))
    rec, thr, bnd, amb = ref.loop(img, lab, probes, sf.gaussian_proj_kernel([7, 7], 3.0), 15, (70,) * len(probes), 7, 2)
    assert amb == 0, 'ambiguous float64 decision: pick another seed'
    rows = []
    for r in rec.tolist():
        row = [name, '%d_%d' % (r[2] // r[1], r[3] // r[1])]
        for j in range(3):
            row += [r[4 + 5 * j], r[5 + 5 * j], r[6 + 5 * j] / r[7 + 5 * j] if r[7 + 5 * j] else 0.0, r[8 + 5 * j]] if j < len(probes) else [''] * 4
        rows.append(row + [r[1], r[19], r[20]])
    return rows, lab, aqua_ref.files(img, thr, bnd), rec


def read_outputs(ann, name):
    d = ann / name
    assert sorted(os.listdir(d)) == sorted([name + '__segmentation_min_cut.npy', name + '_segmentation.tif', name + '_original.tif',
                                            name + '_original_with_segmentation.tif', '%s_lsq_%s.tif' % (name, TAG)])
    return tuple(image_io.imread(str(d / (name + tail))) for tail in ('_original.tif', '_original_with_segmentation.tif', '_lsq_%s.tif' % TAG))


def folder_bytes(ann):
    """{relative path: bytes} of every file a run wrote, the copied config (named after the commit) aside."""
    out = {}
    for dirpath, _, names in os.walk(ann):
        for n in names:
            if not n.startswith('config_'):
                p = os.path.join(dirpath, n)
                out[os.path.relpath(p, ann)] = open(p, 'rb').read()
    return out


# ---- the restatement ----------------------------------------------------------------------------------------------------------
def test_the_uint8_merge_wraps_and_equals_its_closed_form_on_every_pair():
    I = aqua_ref.exhaustive_image()
    got = aqua_ref.merge_channels(I)
    assert got.dtype == np.uint8 and got.shape == (256, 256, 3)
    assert np.array_equal(got, aqua_ref.merged_closed_form(I))
    changed = got != I[..., :3]
    assert not changed[..., 0].any()                         # 54 is even: 54 q is never 255 modulo 256
    for c, q in ((1, Q_GREEN), (2, Q_RED)):                  # one aqua value per odd coefficient, every row but the saturated one
        assert np.array_equal(np.argwhere(changed[..., c]), [[a, q] for a in range(255)])
        assert (got[:255, q, c] == np.arange(1, 256)).all() and got[255, q, c] == 255
    # the wrap is the uint8 product's: aqua 255 leaves blue 3 alone, and an int64 copy of the same pixel would gain 54 * 255 / 255
    px = np.array([[[3, 3, 3, 255]]], np.uint8)
    assert aqua_ref.merge_channels(px)[0, 0].tolist() == [3, 3, 3]
    assert aqua_ref.merge_channels(px.astype(np.int64))[0, 0].tolist() == [57, 140, 236]


def test_the_int_merge_of_the_lsq_file_does_not_wrap():
    bnd, thr = aqua_ref.lsq_combinations()
    blob = np.dstack([bnd.astype(np.int64), thr])
    assert len({tuple(v) for v in blob.reshape(-1, 4).tolist()}) == 16
    got = aqua_ref.merge_channels(blob)
    assert np.array_equal(got, aqua_ref.lsq_closed_form(blob))
    for x, out in zip(blob.reshape(-1, 4).tolist(), got.reshape(-1, 3).tolist()):
        want = [min(255, x[c] + (k if x[3] else 0)) for c, k in enumerate(aqua_ref.K_BGR)]
        assert out == want, (x, out)                         # an aqua spot lights all three channels
    # mask values other than 0 / 255 (the entry point takes any byte): the floor of the quotient
    rng = np.random.default_rng(5)
    blob = rng.integers(0, 256, (64, 64, 4)).astype(np.int64)
    assert np.array_equal(aqua_ref.merge_channels(blob), aqua_ref.lsq_closed_form(blob))


def test_files_of_a_three_channel_image_are_the_present_ones():
    rng = np.random.default_rng(2)
    I = rng.integers(0, 256, (9, 11, 3), dtype=np.uint8)
    thr = (rng.random((9, 11, 2)) < 0.3).astype(np.uint8) * 255
    bnd = (rng.random((9, 11)) < 0.4).astype(np.uint8) * 255
    original, seg, lsq = aqua_ref.files(I, thr, bnd)
    assert np.array_equal(original, I[..., ::-1])
    assert np.array_equal(seg, sf.with_segmentation(I[..., ::-1], bnd, 1))
    assert np.array_equal(lsq, np.dstack([thr[..., 1], thr[..., 0], bnd]))


# ---- the product's numpy path ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('channels', [(0, 1, 2, 3), (3, 1, 0, 2), (0, 1, 2), (2, 1, 0)])
def test_render_equals_the_restatement(channels):
    C = len(channels)
    I = aqua_ref.exhaustive_image()[..., :C]
    rng = np.random.default_rng(C)
    thr = (rng.random((256, 256, C - 1)) < 0.5).astype(np.uint8) * 255
    bnd = (rng.random((256, 256)) < 0.5).astype(np.uint8) * 255
    img = np.empty_like(I)
    img[..., list(channels)] = I                             # channel channels[k] of img holds the reference's channel k
    for got, want in zip(sf.render(img, channels, thr, bnd), aqua_ref.files(I, thr, bnd)):
        assert got.dtype == np.uint8 and np.array_equal(got, want)
    bnd16, thr16 = aqua_ref.lsq_combinations()
    if C == 4:
        assert np.array_equal(sf.render(np.zeros((4, 4, 4), np.uint8), (0, 1, 2, 3), thr16, bnd16)[2],
                              aqua_ref.files(np.zeros((4, 4, 4), np.uint8), thr16, bnd16)[2])


def test_columns_and_rows_with_three_probes():
    assert sf.csv_columns(3) == COLUMNS_3
    assert sf.csv_columns() == sf.csv_columns(2) == COLUMNS_3[:10] + COLUMNS_3[14:]
    rec = np.zeros((1, 24), np.int64)
    rec[0, :4] = 1, 10, 35, 47
    rec[0, 4:9] = 12, 2, 280, 3, 200
    rec[0, 14:19] = 5, 1, 90, 4, 77
    rec[0, 19:21] = 4, 1
    assert sf.rows_from_records('n', rec, 3) == [['n', '3_4', 12, 2, 280 / 3, 200, 0, 0, 0.0, 0, 5, 1, 22.5, 77, 10, 4, 1]]
    assert sf.rows_from_records('n', rec) == [['n', '3_4', 12, 2, 280 / 3, 200, 0, 0, 0.0, 0, 10, 4, 1]]
    wide = sf.widen_rows(sf.rows_from_records('n', rec) + sf.rows_from_records('n', rec, 3))
    assert wide[0] == ['n', '3_4', 12, 2, 280 / 3, 200, 0, 0, 0.0, 0, '', '', '', '', 10, 4, 1] and wide[1][10:14] == [5, 1, 22.5, 77]
    assert csvio.csv_text(COLUMNS_3, wide).splitlines()[1] == 'n,3_4,12,2,93.33333333333333,200,0,0,0.0,0,,,,,10,4,1'


# ---- main -----------------------------------------------------------------------------------------------------------------------
def test_main_on_a_folder_that_mixes_four_and_three_channel_images(tmp_path, monkeypatch):
    inp, scenes = make_folder(tmp_path)
    monkeypatch.chdir(tmp_path)
    h = OracleHandle()
    assert sf.main([], handle=h) is None                     # exit code 0: no SystemExit
    ann = inp / 'annotated'
    all_rows, aqua_foci = [], 0
    assert sorted(scenes) == sorted(ORDER)
    for name in ORDER:
        img, mask = scenes[name]
        rows, lab, want_files, rec = expected(name, img, mask)
        all_rows += rows
        for got, want, what in zip(read_outputs(ann, name), want_files, ('original', 'with_segmentation', 'lsq')):
            assert np.array_equal(got, want), (name, what)
        assert np.array_equal(np.load(ann / name / (name + '__segmentation_min_cut.npy')), lab)
        if img.shape[2] == 4:
            aqua_foci += int(rec[:, 15].sum())
            # the pair columns come from green and red alone
            pair = ref.loop(img, lab, (1, 2), sf.gaussian_proj_kernel([7, 7], 3.0), 15, (70, 70), 7, 2)[0]
            assert np.array_equal(rec[:, 19:21], pair[:, 19:21]) and [r[-2:] for r in rows] == pair[:, 19:21].tolist()
            # the wrap shows in _original: green + 1 at Q_GREEN (saturating), red + 1 at Q_RED (saturating), as RGB
            assert want_files[0][0, :4].tolist() == [[8, 255, 7], [255, 10, 9], [12, 12, 0], [16, 14, 13]]
            assert rec[:, 14].any() and (want_files[2][..., 2] == 54).any()  # an aqua spot off the boundaries: blue = 54
    assert aqua_foci > 3 and len(all_rows) > 6                # not vacuous
    assert sum(r[10] == '' for r in all_rows) == len(expected('b_tif', *scenes['b_tif'])[0]) > 0
    assert open(ann / 'stat_fish_lsq.csv').read() == csvio.csv_text(COLUMNS_3, all_rows)
    assert [c['probes'] for c in h.calls] == [(1, 0), (1, 2, 3), (1, 2, 3)] and [c['ithr'] for c in h.calls] == [(70, 70), (70, 70, 70), (70, 70, 70)]


def test_a_folder_of_three_channel_images_keeps_its_thirteen_columns(tmp_path, monkeypatch):
    inp, scenes = make_folder(tmp_path, kinds=(('t', 'tif'),))
    monkeypatch.chdir(tmp_path)
    sf.main([], handle=OracleHandle())
    rows = [r[:10] + r[14:] for r in expected('t', *scenes['t'])[0]]
    assert open(inp / 'annotated' / 'stat_fish_lsq.csv').read() == csvio.csv_text(sf.csv_columns(), rows) and len(rows) > 1


def test_a_four_channel_image_without_nuclei_still_brings_the_aqua_columns(tmp_path, monkeypatch):
    inp, scenes = make_folder(tmp_path, kinds=(('e', 'npy8'),))
    image_io.write_tiff_gray8(str(inp / 'nuclei_masks' / 'e.tif'), np.zeros((70, 90), np.uint8))
    monkeypatch.chdir(tmp_path)
    sf.main([], handle=OracleHandle())
    assert open(inp / 'annotated' / 'stat_fish_lsq.csv').read() == csvio.csv_text(COLUMNS_3, [])
    original, seg, lsq = read_outputs(inp / 'annotated', 'e')
    assert np.array_equal(original, seg) and not lsq.any()
    assert np.array_equal(original, aqua_ref.merge_channels(scenes['e'][0])[..., ::-1])


def test_two_color_sensitivity_entries_still_refuse_a_fourth_channel(tmp_path, monkeypatch, capsys):
    inp, _ = make_folder(tmp_path, kinds=(('f', 'npy8'), ('t', 'tif')), color_sensitivity=(70, 70))
    monkeypatch.chdir(tmp_path)
    with pytest.raises(SystemExit) as e:
        sf.main([], handle=OracleHandle())
    assert e.value.code == 1 and 'a fourth channel needs a third color_sensitivity entry' in capsys.readouterr().out
    assert sorted(d for d in os.listdir(inp / 'annotated') if os.path.isdir(inp / 'annotated' / d)) == ['t']


def test_the_numpy_path_and_a_rendering_handle_write_identical_files(tmp_path, monkeypatch):
    inp, _ = make_folder(tmp_path)
    monkeypatch.chdir(tmp_path)
    sf.main([], handle=OracleHandle())
    first = folder_bytes(inp / 'annotated')
    h = RenderingOracleHandle()
    sf.main([], handle=h)
    assert [c['render'] for c in h.calls if 'render' in c] == [(2, 1, 0), (0, 1, 2, 3), (0, 1, 2, 3)]     # every image, the TIFF too
    second = folder_bytes(inp / 'annotated')
    assert sorted(first) == sorted(second) and len(first) == 3 * 5 + 2
    for name in first:
        assert first[name] == second[name], name


def test_fish_distance_calculation_reads_what_the_run_leaves(tmp_path, monkeypatch):
    """The chain stays intact.  ``fish_distance_calculation.main`` walks ``<inpath>/*.tif`` as the reference does, so of this folder
    it reaches the three-channel TIFF alone; the four-channel images are ``.npy`` files, and their ``annotated/`` folders go through
    the same reader and the same per-image function (``load_image``, ``get_distances_img``) called directly.  An aqua spot lights
    all three channels of the _lsq_ file, so it is read as green and red FISH: the reference's behaviour, pinned here."""
    from test_fish_distance import StubHandle
    inp, scenes = make_folder(tmp_path)
    monkeypatch.chdir(tmp_path)
    sf.main([], handle=OracleHandle())
    code = 0
    try:
        fdc.main([], handle=StubHandle())                    # walks <inpath>/*.tif: the three-channel image
    except SystemExit as e:
        code = e.code
    _, lab, want_files, _ = expected('b_tif', *scenes['b_tif'])
    try:
        want, want_code = fd_ref.loop(want_files[2], lab, (1, 0, 3)), 0
    except ValueError:                                       # a nucleus with FISH but no centromere pixels: the reference stops there
        want, want_code = [], 1
    assert code == want_code
    assert open(inp / 'centromere_distances.csv').read() == csvio.csv_text(['normalized_distance'], [[v] for v in want])
    read = 0
    for name in ('a_u16', 'c_u8'):                           # the four-channel images' folders, through the same reader
        lsq, seg = fdc.load_image(str(inp), str(inp / (name + '.tif')))
        _, lab, want_files, _ = expected(name, *scenes[name])
        assert np.array_equal(lsq, want_files[2]) and np.array_equal(seg, lab)
        try:
            want = fd_ref.loop(lsq, lab, (1, 0, 3))
        except ValueError:
            continue
        assert fdc.get_distances_img(lsq, seg, (1, 0, 3), StubHandle()) == want
        read += 1
    assert read > 0


# ---- header, export, documents ---------------------------------------------------------------------------------------------------
def test_header_binding_and_documents_of_the_new_symbol():
    hdr = open(os.path.join(ROOT, 'include', 'ecseg_hip.h')).read()
    assert 'int ecseg_fish_render(ecseg_ctx* h, const uint8_t* img, int H, int W, int C, const int32_t* channels' in hdr
    assert 'still 5 - additive: ecseg_fish_render' in hdr and '#define ECSEG_ABI_VERSION 6' in hdr
    assert 'ecseg_fish_render' in _lib.EXPORTS and hasattr(_lib.Handle, 'fish_render') and _lib.ABI_VERSION == 6
    assert hasattr(_lib.load_library(), 'ecseg_fish_render')
    assert 'fs_render_kernel' in open(os.path.join(ROOT, 'ecseg_amd', 'csrc', 'fishspot_kernels.hip')).read()
    for doc in ('README.md', 'DESIGN.md'):
        text = open(os.path.join(ROOT, doc)).read()
        assert 'ecseg_fish_render' in text and 'aqua' in text, doc
    assert 'aqua' in sf.__doc__ and 'order of first appearance' in sf.__doc__


def test_main_keeps_freed_memory_unless_told_otherwise(tmp_path, monkeypatch):
    called = []
    monkeypatch.setattr(sf, 'keep_freed_memory', lambda: called.append(1))
    inp, _ = make_folder(tmp_path, kinds=(('t', 'tif'),))
    monkeypatch.chdir(tmp_path)
    sf.main([], handle=OracleHandle())
    assert called == [1]
    monkeypatch.undo()
    monkeypatch.setenv('ECSEG_MALLOC_DEFAULT', '1')
    assert sf.keep_freed_memory() is False
    monkeypatch.setenv('ECSEG_MALLOC_DEFAULT', '0')
    assert sf.keep_freed_memory() in (True, False)           # True on glibc
    assert 'ECSEG_MALLOC_DEFAULT' in open(os.path.join(ROOT, 'DESIGN.md')).read()
