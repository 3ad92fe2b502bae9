"""``make stat_fish`` without a GPU: the oracle (tests/stat_fish_ref.py) pinned on hand-computed answers, its two producers
against each other on every committed case (and none of them ambiguous in the float64 decision), the host side of
ecseg_amd/stat_fish.py (projected kernel, derived parameters, file names, the BGR wrap rule, CSV text, folder protocol and
exit codes) with an oracle-backed fake handle, the colour TIFF writer, and the new symbol's header and export."""
import os
import sys

import numpy as np
import pytest
import yaml

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import stat_fish_cases as cases              # noqa: E402
import stat_fish_ref as ref                  # noqa: E402
from ecseg_amd import _lib, csvio, image_io  # noqa: E402
from ecseg_amd import stat_fish as sf        # noqa: E402

HAND = cases.hand_cases()
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class OracleHandle:
    """What ``main`` needs of a ``_lib.Handle``, computed by the oracle."""

    def __init__(self):
        self.calls = []

    def ccl_labels(self, mask, connectivity=8):
        assert connectivity == 8
        return ref.nuclei(mask).astype(np.int32)

    def u16_to_u8(self, a):
        return np.floor(np.asarray(a, np.float64) * (255.0 / 65535.0) + 0.5).astype(np.uint8)

    def fish_spots(self, labels, img, probes, weights, normal, ithr, min_cc, line, capacity=4096):
        self.calls.append(dict(probes=tuple(probes), K=np.asarray(weights).shape[0], normal=normal, ithr=tuple(ithr), min_cc=min_cc, line=line))
        rec, thr, bnd, _ = ref.loop(img, labels, probes, np.asarray(weights, np.float64), normal, ithr, min_cc, line)
        return rec, thr, bnd


# ---- the oracle itself ----------------------------------------------------------------------------------------------------
def test_boundaries_of_a_tiny_map_by_hand():
    R = np.array([[0, 0, 0, 0, 0], [0, 1, 1, 1, 0], [0, 1, 1, 1, 0], [0, 1, 1, 1, 0]])
    t1 = np.array([[0, 1, 1, 1, 0], [1, 0, 0, 1, 0], [1, 0, 0, 1, 0], [1, 1, 1, 1, 0]])
    t2 = np.array([[0, 1, 1, 1, 0], [1, 1, 1, 1, 1], [1, 1, 1, 1, 1], [1, 1, 1, 1, 1]])
    assert np.array_equal(ref.boundaries(R, 1), t1 * 255)
    assert np.array_equal(ref.boundaries(R, 2), t2 * 255)
    # the sums are over label VALUES: 0 + 3 against 1 + 2 cancels for t = 2 although three labels meet there (why the driver
    # hands over the ranks 1..n, which is what the reference summed, and not the raster-index labels of the device labelling)
    assert ref.boundaries(np.tile([[0, 3, 1, 2]], (4, 1)), 2)[1].tolist() == [255, 0, 255, 255]
    assert ref.boundaries(np.tile([[0, 1, 2, 3]], (4, 1)), 2)[1].tolist() == [255, 255, 0, 255]      # 1 + 2 against 3 + nothing


def test_correlation_by_hand_and_its_bound():
    x = np.array([[1, 2], [3, 4]], np.uint8)
    w = np.arange(9, dtype=np.float64).reshape(3, 3)
    # out[0, 0] = w[1,1]*1 + w[1,2]*2 + w[2,1]*3 + w[2,2]*4
    assert ref.correlate(x, w).tolist() == [[4 + 10 + 21 + 32, 3 + 8 + 18 + 28], [1 + 4 + 12 + 20, 0 + 2 + 9 + 16]]
    assert (ref.error_bound(x, w) < 1e-12).all() and (ref.error_bound(x, w) > 0).all()
    assert np.isnan(ref.correlate(x, cases.NAN1)).all()


@pytest.mark.parametrize('name', sorted(HAND))
def test_hand_cases_on_both_producers(name):
    case, expected = HAND[name]
    a = ref.loop(*cases.args(case))
    b = ref.records(*cases.args(case))
    assert a[3] == 0 and b[3] == 0, 'ambiguous float64 decision in a committed case'
    for x, y in zip(a[:3], b[:3]):
        assert np.array_equal(x, y)
    if not expected:
        assert a[0].shape == (0, 24)
    for col, values in expected.items():
        assert a[0][:, col].tolist() == values, (col, a[0][:, col].tolist())


def test_committed_seeds_agree_and_none_is_ambiguous():
    foci = np.zeros(3, int)
    for seed in range(cases.N_SEEDS):
        case = cases.scene(seed)
        a = ref.loop(*cases.args(case))
        b = ref.records(*cases.args(case))
        assert a[3] == 0, 'seed %d has %d ambiguous pixel(s): pick another seed' % (seed, a[3])
        for x, y in zip(a[:3], b[:3]):
            assert np.array_equal(x, y), seed
        foci += a[0][:, [5, 10, 20]].sum(axis=0)
    assert (foci > 500).all(), foci                          # not vacuous


def test_an_ambiguous_case_is_counted():
    img = np.zeros((3, 3, 3), np.uint8); img[..., 1] = 10; img[1, 1, 1] = 100; img[0, 0, 0] = 1
    seg = np.ones((3, 3), np.int32)
    lap = -np.ones((3, 3)); lap[1, 1] = 8
    img[2, 2, 1] = 200                                       # the maximum is elsewhere, so the filter decides at the centre
    coefficient = ref.correlate(img[..., 1], lap)[1, 1]
    _, ambiguous = ref.thresholded(img, (1, 0), seg, lap, coefficient, (5.0, 5.0))
    assert ambiguous == 1


# ---- host side of the driver ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('K,sigma', [(7, 3.0), (15, 6.0), (23, 10.0), (3, 1.5)])
def test_projected_kernel(K, sigma):
    w = sf.gaussian_proj_kernel([K, K], sigma)
    assert w.shape == (K, K) and w.dtype == np.float64
    assert abs(w.sum()) < 1e-12                              # orthogonal to the constant kernel
    assert abs(np.linalg.norm(w) - 1) < 1e-12
    assert np.allclose(w, cases.proj_kernel(K, sigma), rtol=0, atol=1e-12)
    assert np.array_equal(w, w.T) and np.array_equal(w, w[::-1])


def test_k1_kernel_is_nan_and_gives_no_normal_centre():
    w = sf.gaussian_proj_kernel([1, 1], 3.0)
    assert w.shape == (1, 1) and np.isnan(w[0, 0])
    case, _ = HAND['k1_only_the_maximum']
    rec = ref.loop(case['img'], case['seg'], case['probes'], w, -1e300, case['ithr'], 1, 1)[0]
    assert rec[0, 4] == 1                                    # even with a threshold everything would exceed


def test_derived_parameters():
    p = sf.DEFAULT_PARAMS
    assert sf.derived_parameters(1, p) == (3.0, 7, [7, 7])
    assert sf.derived_parameters(0.5, p) == (6.0, 28, [15, 15])
    stdev, min_cc, shape = sf.derived_parameters(0.3, p)
    assert (stdev, min_cc, shape) == (3 / 0.3, 77, [23, 23])
    assert all(isinstance(v, float) and np.isnan(v) for v in sf.derived_parameters(float('nan'), p))
    assert sf.get_scale(np.array([2500, 100, 90000]), 2500) == 1.0
    assert sf.get_scale(np.array([400, 100]), 2500) == float(np.sqrt(2500 / 250.0))
    assert np.isnan(sf.get_scale(np.array([]), 2500))


def test_lsq_file_name():
    p = sf.DEFAULT_PARAMS
    assert sf.lsq_name('img', p, 3.0, 7) == 'img_lsq_n15_std3.00_s7_g70.0_r70.0.tif'
    assert sf.lsq_name('a b', p, 3 / 0.3, 77) == 'a b_lsq_n15_std10.00_s77_g70.0_r70.0.tif'
    assert sf.lsq_name('x', p, float('nan'), float('nan')) == 'x_lsq_n15_stdnan_snan_g70.0_r70.0.tif'


def test_bgr_wrap_rule():
    rng = np.random.default_rng(3)
    rgb = rng.integers(0, 256, (6, 7, 3), dtype=np.uint8)
    rgb[0, 0] = (0, 255, 7)
    b = (rng.random((6, 7)) < 0.5).astype(np.uint8) * 255
    b[0, 0] = 255
    bgr = rgb[..., ::-1].astype(np.int64)                    # the reference's arithmetic, in its channel order
    want = np.minimum(bgr + np.dstack([b, -b.astype(np.int64), b]), 255).astype(np.uint8)[..., ::-1]
    got = sf.with_segmentation(rgb, b, 1)
    assert np.array_equal(got, want) and got[0, 0].tolist() == [255, 0, 255]
    assert np.array_equal(got[b == 0], rgb[b == 0])


def test_csv_text_and_rows():
    rec = np.zeros((2, 24), np.int64)
    rec[0, :4] = 1, 10, 35, 47
    rec[0, 4:9] = 12, 2, 280, 3, 200
    rec[0, 9:14] = 0, 0, 0, 0, 0
    rec[0, 19:21] = 4, 1
    rec[1, :4] = 2, 3, 3, 299
    rec[1, 9:14] = 7, 1, 100, 4, 60
    rows = sf.rows_from_records('im,1', rec)
    text = csvio.csv_text(sf.csv_columns(), rows)
    assert text == ('image_name,nucleus_center,#_FISH_pixels (green),#_FISH_foci (green),Avg fish intensity (green),Max fish intensity (green),'
                    '#_FISH_pixels (red),#_FISH_foci (red),Avg fish intensity (red),Max fish intensity (red),#_DAPI_pixels,'
                    '#_FISH_pixels (green and red),#_FISH_foci (green and red)\n'
                    '"im,1",3_4,12,2,93.33333333333333,200,0,0,0.0,0,10,4,1\n'
                    '"im,1",1_99,0,0,0.0,0,7,1,25.0,60,3,0,0\n')


# ---- main with the oracle-backed handle ---------------------------------------------------------------------------------------
def _folder(tmp_path, names=('b_img', 'a_img'), scale=1, size=(70, 90), **section):
    from PIL import Image
    inp = tmp_path / 'in'
    (inp / 'nuclei_masks').mkdir(parents=True, exist_ok=True)
    scenes = {}
    for k, name in enumerate(names):
        case = cases.scene(12 + 7 * k, size=size, K=7)
        img = np.ascontiguousarray(case['img'][..., :3])
        mask = (case['seg'] > 0).astype(np.uint8) * 255
        Image.fromarray(img).save(str(inp / (name + '.tif')), compression='tiff_lzw')
        image_io.write_tiff_gray8(str(inp / 'nuclei_masks' / (name + '.tif')), mask)
        scenes[name] = (img, mask)
    cfg = dict(inpath=str(inp), scale=scale, use_min_cut=False, nuclei_size_T=5000)
    cfg.update(section)
    yaml.safe_dump({'stat_fish': cfg, 'metaseg': {'inpath': 'x'}}, open(tmp_path / 'config.yaml', 'w'))
    return inp, scenes


def _expected(name, img, mask, scale=1, params=sf.DEFAULT_PARAMS):
    """Files and rows of one TIFF image from the oracle alone (RGB file: green = 1, red = 0)."""
    lab = ref.nuclei(mask)
    if scale == 'auto':
        areas = np.bincount(lab[lab > 0])[1:]
        scale = float(np.sqrt(2500 / np.median(areas))) if len(areas) else float('nan')
    stdev = 3 / scale
    min_cc = int(7 // (scale * scale))
    K = int(7 // scale) if 7 // scale % 2 else int(7 // scale) + 1
    rec, thr, bnd, amb = ref.loop(img, lab, (1, 0), sf.gaussian_proj_kernel([K, K], stdev), 15, (70, 70), min_cc, 2)
    assert amb == 0
    rows = []
    for r in rec.tolist():
        rows.append([name, '%d_%d' % (r[2] // r[1], r[3] // r[1]), r[4], r[5], r[6] / r[7] if r[7] else 0.0, r[8],
                     r[9], r[10], r[11] / r[12] if r[12] else 0.0, r[13], r[1], r[19], r[20]])
    return rows, lab, np.dstack([thr[..., 1], thr[..., 0], bnd]), bnd, 'n15_std%.2f_s%d_g70.0_r70.0' % (stdev, min_cc)


def test_main_writes_the_annotated_folder(tmp_path, monkeypatch, capsys):
    inp, scenes = _folder(tmp_path)
    monkeypatch.chdir(tmp_path)
    (inp / 'annotated').mkdir()
    (inp / 'annotated' / 'old.txt').write_text('previous run')
    sf.main([], handle=OracleHandle())
    ann = inp / 'annotated'
    moved = [d for d in os.listdir(inp) if d.startswith('annotated_')]
    assert len(moved) == 1 and os.listdir(inp / moved[0]) == ['old.txt']
    assert not [d for d in os.listdir(inp) if d.startswith('tmp_')]
    configs = [f for f in os.listdir(ann) if f.startswith('config_') and f.endswith('.yaml')]
    assert len(configs) == 1 and open(ann / configs[0]).read() == open(tmp_path / 'config.yaml').read()
    assert yaml.safe_load(open(ann / 'stat_fish_params.yaml')) == sf.DEFAULT_PARAMS
    all_rows = []
    for name in sorted(scenes):                               # sorted image order
        img, mask = scenes[name]
        rows, lab, lsq, bnd, tag = _expected(name, img, mask)
        all_rows += rows
        d = ann / name
        assert sorted(os.listdir(d)) == sorted([name + '__segmentation_min_cut.npy', name + '_segmentation.tif', name + '_original.tif',
                                                name + '_original_with_segmentation.tif', '%s_lsq_%s.tif' % (name, tag)])
        saved = np.load(d / (name + '__segmentation_min_cut.npy'))
        assert saved.dtype == np.int64 and np.array_equal(saved, lab)
        assert np.array_equal(image_io.imread(str(d / (name + '_segmentation.tif'))), mask)
        assert np.array_equal(image_io.imread(str(d / (name + '_original.tif'))), img)
        assert np.array_equal(image_io.imread(str(d / ('%s_lsq_%s.tif' % (name, tag)))), lsq)
        want = img.copy()
        want[bnd != 0] = np.stack([np.full(img.shape[:2], 255, np.uint8), img[..., 1] + np.uint8(1), np.full(img.shape[:2], 255, np.uint8)], -1)[bnd != 0]
        assert np.array_equal(image_io.imread(str(d / (name + '_original_with_segmentation.tif'))), want)
    assert len(all_rows) > 4
    assert open(ann / 'stat_fish_lsq.csv').read() == csvio.csv_text(sf.csv_columns(), all_rows)


def test_main_scale_auto_half_and_params_file(tmp_path, monkeypatch):
    inp, scenes = _folder(tmp_path, names=('only',), scale='auto', masks=None)
    monkeypatch.chdir(tmp_path)
    h = OracleHandle()
    sf.main([], handle=h)
    rows, _, _, _, tag = _expected('only', *scenes['only'], scale='auto')
    assert h.calls[0]['K'] == 1 and h.calls[0]['ithr'] == (float('inf'), float('inf'))       # the call for the areas alone
    assert os.path.exists(inp / 'annotated' / 'only' / ('only_lsq_%s.tif' % tag))
    assert open(inp / 'annotated' / 'stat_fish_lsq.csv').read() == csvio.csv_text(sf.csv_columns(), rows)
    # a params file overrides the defaults and is copied
    os.makedirs(tmp_path / 'src')
    (tmp_path / 'src' / 'stat_fish_params.yaml').write_text('normal_threshold: 20\nline_thickness: 3\nmin_score: 0.95\n')
    h = OracleHandle()
    sf.main([], handle=h)
    assert h.calls[-1]['normal'] == 20 and h.calls[-1]['line'] == 3
    assert open(inp / 'annotated' / 'stat_fish_params.yaml').read() == 'normal_threshold: 20\nline_thickness: 3\nmin_score: 0.95\n'


def test_main_scale_auto_without_nuclei_takes_the_nan_branch(tmp_path, monkeypatch):
    inp, scenes = _folder(tmp_path, names=('empty',), scale='auto')
    image_io.write_tiff_gray8(str(inp / 'nuclei_masks' / 'empty.tif'), np.zeros((70, 90), np.uint8))
    monkeypatch.chdir(tmp_path)
    sf.main([], handle=OracleHandle())
    d = inp / 'annotated' / 'empty'
    lsq = image_io.imread(str(d / 'empty_lsq_n15_stdnan_snan_g70.0_r70.0.tif'))
    assert lsq.shape == (70, 90, 3) and not lsq.any()
    assert open(inp / 'annotated' / 'stat_fish_lsq.csv').read() == csvio.csv_text(sf.csv_columns(), [])


def test_npy_images_are_indexed_as_the_reference_indexes_them(tmp_path, monkeypatch):
    inp, scenes = _folder(tmp_path, names=('t',))
    img, mask = scenes['t']
    os.remove(inp / 't.tif')
    np.save(inp / 't.npy', (img[..., ::-1].astype(np.uint16) * 257))      # BGR, 16-bit: u16_to_u8 gives the 8-bit values back
    monkeypatch.chdir(tmp_path)
    sf.main([], handle=OracleHandle())
    rows, _, lsq, _, tag = _expected('t', img, mask)
    assert open(inp / 'annotated' / 'stat_fish_lsq.csv').read() == csvio.csv_text(sf.csv_columns(), rows)
    assert np.array_equal(image_io.imread(str(inp / 'annotated' / 't' / ('t_lsq_%s.tif' % tag))), lsq)
    assert np.array_equal(image_io.imread(str(inp / 'annotated' / 't' / 't_original.tif')), img)


def test_mask_and_image_are_cropped_to_their_common_extent(tmp_path, monkeypatch):
    inp, scenes = _folder(tmp_path, names=('c',))
    img, mask = scenes['c']
    image_io.write_tiff_gray8(str(inp / 'nuclei_masks' / 'c.tif'), np.pad(mask, ((0, 5), (0, 0)))[:, :80])    # taller, narrower
    monkeypatch.chdir(tmp_path)
    sf.main([], handle=OracleHandle())
    rows, _, _, _, _ = _expected('c', img[:, :80], mask[:, :80])
    assert open(inp / 'annotated' / 'stat_fish_lsq.csv').read() == csvio.csv_text(sf.csv_columns(), rows)
    assert image_io.imread(str(inp / 'annotated' / 'c' / 'c_original.tif')).shape == (70, 80, 3)


def test_per_image_failures_exit_1_and_keep_the_rest(tmp_path, monkeypatch, capsys):
    from PIL import Image
    inp, scenes = _folder(tmp_path, names=('good', 'nomask', 'sixteen', 'four', 'broken'))
    os.remove(inp / 'nuclei_masks' / 'nomask.tif')
    Image.fromarray(np.zeros((70, 90), np.uint16)).save(str(inp / 'sixteen.tif'))
    os.remove(inp / 'four.tif')
    np.save(inp / 'four.npy', np.zeros((70, 90, 4), np.uint8))
    image_io.write_tiff_gray8(str(inp / 'nuclei_masks' / 'four.tif'), scenes['four'][1])
    (inp / 'broken.tif').write_bytes(b'II*\0garbage')
    monkeypatch.chdir(tmp_path)
    with pytest.raises(SystemExit) as e:
        sf.main([], handle=OracleHandle())
    assert e.value.code == 1
    out = capsys.readouterr().out
    assert '4 image(s) were NOT processed' in out and 'has no nucleus mask' in out and '8-bit' in out
    rows, _, _, _, _ = _expected('good', *scenes['good'])
    assert open(inp / 'annotated' / 'stat_fish_lsq.csv').read() == csvio.csv_text(sf.csv_columns(), rows)
    assert sorted(d for d in os.listdir(inp / 'annotated') if os.path.isdir(inp / 'annotated' / d)) == ['good']


@pytest.mark.parametrize('change,text', [
    (dict(inpath='/nonexistent/folder'), 'Input folder does not exist'),
    (dict(use_min_cut=True), 'use_min_cut: False'),
    (dict(scale='big'), 'scale must be'),
    (dict(scale=0), 'scale must be'),
    (dict(masks='/nonexistent/masks'), 'nucleus masks'),
])
def test_configuration_errors_exit_2(tmp_path, monkeypatch, capsys, change, text):
    inp, _ = _folder(tmp_path, names=('a',), **change)
    monkeypatch.chdir(tmp_path)
    with pytest.raises(SystemExit) as e:
        sf.main([], handle=OracleHandle())
    assert e.value.code == 2 and text in capsys.readouterr().out
    assert 'max_flow_binary_mask' in sf.main.__globals__['__doc__']
    if 'inpath' not in change:
        assert not [d for d in os.listdir(inp) if d.startswith(('tmp_', 'annotated'))]


def test_more_configuration_errors(tmp_path, monkeypatch, capsys):
    inp, _ = _folder(tmp_path, names=('a',))
    monkeypatch.chdir(tmp_path)
    os.remove(inp / 'a.tif')
    with pytest.raises(SystemExit) as e:                     # no images
        sf.main([], handle=OracleHandle())
    assert e.value.code == 2
    yaml.safe_dump({'metaseg': {'inpath': 'x'}}, open(tmp_path / 'config.yaml', 'w'))
    with pytest.raises(SystemExit) as e:                     # no section
        sf.main([], handle=OracleHandle())
    assert e.value.code == 2
    _folder(tmp_path, names=('a',))
    os.makedirs(tmp_path / 'src', exist_ok=True)
    (tmp_path / 'src' / 'stat_fish_params.yaml').write_text('line_thickness: 99\n')
    with pytest.raises(SystemExit) as e:
        sf.main([], handle=OracleHandle())
    assert e.value.code == 2 and 'line_thickness' in capsys.readouterr().out


def test_shipped_config_and_makefile():
    cfg = yaml.safe_load(open(os.path.join(ROOT, 'config.yaml')))['stat_fish']
    assert cfg['use_min_cut'] is False and {'inpath', 'scale', 'use_min_cut', 'nuclei_size_T'} <= set(cfg)
    mk = open(os.path.join(ROOT, 'Makefile')).read()
    assert 'stat_fish: build\n\tpython src/stat_fish.py' in mk
    assert os.path.exists(os.path.join(ROOT, 'src', 'stat_fish.py'))
    assert not os.path.exists(os.path.join(ROOT, 'src', 'stat_fish_params.yaml'))


# ---- colour TIFF writer, header, export ---------------------------------------------------------------------------------------
@pytest.mark.parametrize('shape', [(1, 1), (5, 7), (300, 401), (40, 3000), (1040, 1392)])
def test_colour_tiff_round_trip(tmp_path, shape):
    from PIL import Image
    rng = np.random.default_rng(shape[0])
    a = rng.integers(0, 256, shape + (3,), dtype=np.uint8)
    a[: shape[0] // 2] = a[0, 0]                              # long runs too
    p = str(tmp_path / 'c.tif')
    image_io.write_tiff_rgb8(p, a)
    assert np.array_equal(image_io.imread(p), a)
    assert np.array_equal(image_io.read_tiff(p, native=False), a)
    with Image.open(p) as im:
        assert im.mode == 'RGB' and np.array_equal(np.array(im), a)
        assert im.tag_v2[259] == 5 and im.tag_v2[317] == 2 and im.tag_v2[278] == max(1, min(shape[0], 8192 // (3 * shape[1])))
    with pytest.raises(ValueError):
        image_io.write_tiff_rgb8(p, a[..., 0])


def test_int32_labels_are_saved_as_numpy_saves_int64(tmp_path):
    lab = np.random.default_rng(1).integers(0, 2 ** 31 - 1, (33, 47)).astype(np.int32)
    image_io.write_npy_int64(str(tmp_path / 'a.npy'), lab)
    np.save(str(tmp_path / 'b.npy'), lab.astype(np.int64))
    assert open(tmp_path / 'a.npy', 'rb').read() == open(tmp_path / 'b.npy', 'rb').read()


def test_header_and_export_of_the_new_symbol():
    hdr = open(os.path.join(ROOT, 'include', 'ecseg_hip.h')).read()
    assert 'int ecseg_fish_spots(ecseg_ctx* h, const int32_t* labels, int H, int W, const uint8_t* img, int C' in hdr
    for word in ('ECSEG_FISH_SPOT_INT64      24', 'ECSEG_FISH_SPOT_MAX_KERNEL', 'ECSEG_FISH_SPOT_MAX_LINE', 'src/stat_fish.py:73-107', '64-bit',
                 'ecseg_tiff_write_rgb8', 'ecseg_npy_write_i32_as_i64'):
        assert word in hdr, word
    assert sf.MAX_KERNEL == 63 and sf.MAX_LINE == 16 and _lib.Handle.FISH_SPOT_INT64 == 24
    assert 'ecseg_fish_spots' in _lib.EXPORTS
    lib = _lib.load_library()
    for name in ('ecseg_fish_spots', 'ecseg_tiff_write_rgb8', 'ecseg_npy_write_i32_as_i64'):
        assert hasattr(lib, name)
    from ecseg_amd import build
    assert 'fishspot_kernels.hip' in build.SOURCES
