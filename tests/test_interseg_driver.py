"""`make interseg` without a GPU: the host half of the file-level driver (src/interseg.py:48-258) against fixtures written by
skimage 0.18.3 / scipy / pandas (tools/make_golden_interseg.py) - crop windows and tiling, centroid strings and the
brightness gate from region records, the centromeric quality score, the config and exit-code paths - and the CPU
reference of the region and crop kernels (oracle/interseg.py, csrc/interseg_kernels.hip) against skimage's regionprops and
resize."""
import json
import os
import re

import numpy as np
import pytest
import yaml
from scipy import ndimage as ndi

from ecseg_amd import interseg
from oracle import interseg as oracle_interseg
from oracle.interseg import exact_resize

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCENES = ['interseg_scene_small.npz', 'interseg_scene_large.npz']


def region_records(seg, img, channel0):
    """What ecseg_nuclei_regions returns, restated with scipy: int64 (n, 8) area, bbox, sum of rows / columns, channel sum."""
    H, W = seg.shape
    lab, n = ndi.label(seg != 0, structure=np.ones((3, 3), int))   # 8-connected, numbered in raster order of the first pixel
    out = np.zeros((n, 8), np.int64)
    yy, xx = np.mgrid[:H, :W]
    for k in range(n):
        m = lab == k + 1
        ys, xs = yy[m], xx[m]
        out[k] = [m.sum(), ys.min(), xs.min(), ys.max() + 1, xs.max() + 1, ys.sum(), xs.sum(), int(img[:H, :W, channel0][m].sum())]
    return out, lab


@pytest.mark.parametrize('shape,want', [
    ((1, 1), [(0, 0, 1, 1)]),
    ((1, 256), [(0, 0, 1, 256)]),
    ((256, 256), [(0, 0, 256, 256)]),
    ((257, 100), [(0, 0, 256, 100)]),
    ((100, 257), [(0, 0, 100, 256)]),
    ((255, 600), [(0, 0, 255, 256), (0, 256, 255, 256)]),
    ((256, 300), [(0, 0, 256, 256)]),
    ((511, 511), [(0, 0, 256, 256)]),
    ((530, 540), [(0, 0, 256, 256), (0, 256, 256, 256), (256, 0, 256, 256), (256, 256, 256, 256)]),
    ((512, 40), [(0, 0, 256, 40), (256, 0, 256, 40)]),
])
def test_crop_windows(shape, want):
    assert interseg.crop_windows(*shape) == want


@pytest.mark.parametrize('scene', SCENES)
def test_region_rows_match_the_skimage_fixture(golden_dir, scene):
    z = np.load(os.path.join(golden_dir, scene))
    rec, _ = region_records(z['seg'], z['image'], 0)
    want = z['records']
    assert np.array_equal(rec[:, :5], want[:, :5])                             # area, bbox (regionprops order)
    assert np.array_equal(rec[:, 7], want[:, 5])
    centers, low, desc, tiled, owner = interseg.region_rows(rec)
    assert centers == [str(c) for c in z['centers']]
    assert np.array_equal(low, want[:, 7].astype(bool))
    win = z['windows'][~low[z['windows'][:, 0]]]                              # the fixture crops every region; gated ones get none
    assert np.array_equal(desc, win[:, :5]) and np.array_equal(tiled, win[:, 5].astype(bool)) and np.array_equal(owner, win[:, 0])


def test_brightness_gate_is_exact_at_12_75():
    # area 4: channel sums 51 (mean 12.75, predicted) and 50 (below: Low_TRGT)
    rec = np.array([[4, 0, 0, 2, 2, 2, 2, 51], [4, 5, 0, 7, 2, 22, 2, 50]], np.int64)
    _, low, desc, _, _ = interseg.region_rows(rec)
    assert low.tolist() == [False, True] and desc.tolist() == [[0, 0, 0, 2, 2]]


@pytest.mark.parametrize('scene', SCENES)
def test_integer_bilinear_equals_skimage_resize_but_for_exact_integers(golden_dir, scene):
    z = np.load(os.path.join(golden_dir, scene))
    seg, img = z['seg'], z['image']
    _, lab = region_records(seg, img, 0)
    km1 = 0
    for k, (r, y0, x0, h, w, _) in enumerate(z['windows']):
        win = img[y0:y0 + h, x0:x0 + w] * (lab[y0:y0 + h, x0:x0 + w] == r + 1)[..., None]
        got, exact = exact_resize(win)
        d = got.astype(int) - z['crops'][k]
        assert np.all((d == 0) | ((d == 1) & exact)), (scene, k)
        km1 += int(((d == 1) & exact).sum())
    print('%s: %d pixels where skimage holds k - 1 for an exact integer k' % (scene, km1))


@pytest.mark.parametrize('scene', SCENES)
def test_oracle_matches_the_skimage_fixture(golden_dir, scene):
    # oracle/interseg.py is the reference of the GPU kernel tests (tests/test_gpu_interseg_kernels.py): pin it to skimage
    z = np.load(os.path.join(golden_dir, scene))
    seg, img, want = z['seg'], z['image'], z['records']
    for ch in (0, 1):
        rec, lab = oracle_interseg.region_records(seg, img, ch)
        assert rec.dtype == np.int64 and rec.shape == (len(want), 8)
        assert np.array_equal(rec[:, :5], want[:, :5]) and np.array_equal(rec[:, 7], want[:, 5 + ch])
        assert np.array_equal(rec, region_records(seg, img, ch)[0]) and np.array_equal(lab, region_records(seg, img, ch)[1])
    assert interseg.region_rows(rec)[0] == [str(c) for c in z['centers']]    # centroids: the sums of rows and columns
    for order in ((0, 1, 2), (1, 0, 2)):
        for k, (r, y0, x0, h, w, _) in enumerate(z['windows']):
            got = oracle_interseg.nucleus_crop(img, lab, r, y0, x0, h, w, order)
            exact = exact_resize(img[y0:y0 + h, x0:x0 + w] * (lab[y0:y0 + h, x0:x0 + w] == r + 1)[..., None])[1][..., list(order)]
            d = got.astype(int) - z['crops'][k][..., list(order)]
            assert got.shape == (256, 256, 3) and np.all((d == 0) | ((d == 1) & exact)), (scene, order, k)


@pytest.mark.parametrize('seed', range(20))
def test_oracle_region_records_equal_the_loop_restatement(seed):
    rng = np.random.default_rng(7000 + seed)
    H, W = int(rng.integers(1, 70)), int(rng.integers(1, 90))
    seg = (rng.random((H, W)) < rng.choice([0.05, 0.3, 0.5, 0.8])).astype(np.uint8) * int(rng.integers(1, 256))
    C = int(rng.integers(1, 5))
    img = rng.integers(0, 256, (H + int(rng.integers(0, 3)), W + int(rng.integers(0, 3)), C), dtype=np.uint8)
    ch = int(rng.integers(0, C))
    rec, lab = oracle_interseg.region_records(seg, img, ch)
    want, want_lab = region_records(seg, img, ch)
    assert np.array_equal(rec, want) and np.array_equal(lab, want_lab)
    if len(rec):                                                                 # crops: any window, any channel order
        r = int(rng.integers(0, len(rec)))
        h, w = int(rng.integers(1, H + 1)), int(rng.integers(1, W + 1))
        y0, x0 = int(rng.integers(0, H - h + 1)), int(rng.integers(0, W - w + 1))
        order = [int(c) for c in rng.integers(0, C, 3)]
        got = oracle_interseg.nucleus_crop(img, lab, r, y0, x0, h, w, order)
        win = np.stack([img[y0:y0 + h, x0:x0 + w, c] for c in order], -1) * (lab[y0:y0 + h, x0:x0 + w] == r + 1)[..., None]
        assert np.array_equal(got, exact_resize(win)[0])


def _score_cases(golden_dir):
    return json.load(open(os.path.join(golden_dir, 'interseg_kurtosis.json')))


def test_quality_score_matches_scipy_and_pandas(golden_dir, tmp_path):
    cases = _score_cases(golden_dir)
    assert any(c['score'] is None for c in cases) and any(c['score'] == -3.0 for c in cases) and any(not c['pass'] for c in cases)
    for c in cases:
        p = tmp_path / 'stat_fish_lsq.csv'
        p.write_text(c['csv'])
        s = interseg.quality_score(interseg.read_stat_fish(str(p)), c['image'], c['column'])
        if c['score'] is None:
            assert np.isnan(s), c
        else:
            assert s == pytest.approx(c['score'], rel=1e-12, abs=1e-12), c
        assert bool(s <= 3) == c['pass'], c


def test_kurtosis_edge_cases():
    assert np.isnan(interseg.kurtosis([]))
    assert np.isnan(interseg.kurtosis([1.0, float('nan')]))
    assert interseg.kurtosis([5.0] * 7) == -3.0
    assert interseg.kurtosis([1.0, 2.0]) == pytest.approx(-2.0)


def _config(tmp_path, monkeypatch, **kw):
    cfg = {'inpath': str(tmp_path / 'in'), 'FISH_color': 'red', 'has_centromeric_probe': False}
    cfg.update(kw)
    (tmp_path / 'config.yaml').write_text(yaml.safe_dump({'interseg': cfg}))
    monkeypatch.chdir(tmp_path)


def test_missing_input_folder_exits_2(tmp_path, monkeypatch, capsys):
    _config(tmp_path, monkeypatch)
    with pytest.raises(SystemExit) as e:
        interseg.main([])
    assert e.value.code == 2 and 'Input folder does not exist. Exiting...' in capsys.readouterr().out


@pytest.mark.parametrize('color', ['blue', 'DAPI'])
def test_bad_fish_color_exits_2(tmp_path, monkeypatch, capsys, color):
    os.makedirs(tmp_path / 'in')
    _config(tmp_path, monkeypatch, FISH_color=color)
    with pytest.raises(SystemExit) as e:
        interseg.main([])
    assert e.value.code == 2 and 'FISH_color can only be "green" or "red".' in capsys.readouterr().out
    assert not os.path.exists(tmp_path / 'in' / 'annotated')


def test_empty_folder_exits_2_after_creating_annotated(tmp_path, monkeypatch, capsys):
    # the reference crashes on an empty folder (pd.concat of nothing); here: a message and exit code 2, no CSV
    os.makedirs(tmp_path / 'in')
    _config(tmp_path, monkeypatch, FISH_color='Green')
    with pytest.raises(SystemExit) as e:
        interseg.main([])
    assert e.value.code == 2 and 'No .tif / .npy images' in capsys.readouterr().out
    assert os.path.isdir(tmp_path / 'in' / 'annotated')
    assert not os.path.exists(tmp_path / 'in' / 'interphase_prediction_green.csv')


def test_config_has_the_reference_interseg_section():
    var = yaml.safe_load(open(os.path.join(ROOT, 'config.yaml')))['interseg']
    assert var == {'inpath': './example_interSeg', 'FISH_color': 'red', 'has_centromeric_probe': False}
    assert re.search(r'^interseg: build\n\tpython src/interseg.py$', open(os.path.join(ROOT, 'Makefile')).read(), re.M)


def test_new_entry_points_are_declared_and_exported():
    from ecseg_amd._lib import ABI_VERSION, EXPORTS
    header = open(os.path.join(ROOT, 'include', 'ecseg_hip.h')).read()
    for name in ('ecseg_nuclei_regions', 'ecseg_nucleus_crops'):
        assert re.search(r'\b%s\s*\(' % name, header) and name in EXPORTS
    assert ABI_VERSION == 6


def test_csv_columns_and_text():
    from ecseg_amd import csvio
    cols = interseg.csv_columns(True)
    assert cols == ['image_name', 'nucleus_center', 'interSeg_label', 'ecSeg-c_label', 'ecSeg-i_label']
    assert interseg.csv_columns(False) == ['image_name', 'nucleus_center', 'interSeg_label', 'ecSeg-i_label']
    txt = csvio.csv_text(interseg.csv_columns(False), [['a', '1_2', interseg.LOW_TRGT, interseg.LOW_TRGT]])
    assert txt == ('image_name,nucleus_center,interSeg_label,ecSeg-i_label\n'
                   'a,1_2,No_Prediction (Low_TRGT_brightness),No_Prediction (Low_TRGT_brightness)\n')
