"""`make interseg` on the GPU: region records and crops of ecseg_nuclei_regions / ecseg_nucleus_crops against the skimage
0.18.3 fixtures (tools/make_golden_interseg.py), and `python src/interseg.py` end to end on a folder of FISH images with
the synthetic classifiers, against rows built from the fixtures' crops through the CPU oracle."""
import csv
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest
import yaml
from PIL import Image

from ecseg_amd import hdf5_min, image_io, interseg
from oracle import unet as oracle_unet
from oracle.interseg import exact_resize

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCENES = ['interseg_scene_small.npz', 'interseg_scene_large.npz']
MARGIN = 1e-3


@pytest.mark.parametrize('scene', SCENES)
@pytest.mark.parametrize('fish_index', [0, 1])
def test_region_records_match_skimage(gpu, golden_dir, scene, fish_index):
    z = np.load(os.path.join(golden_dir, scene))
    rec = gpu.nuclei_regions(z['seg'], z['image'], fish_index)
    want = z['records']
    assert rec.shape == (len(want), 8)
    assert np.array_equal(rec[:, :5], want[:, :5])                 # order, area, bbox
    assert np.array_equal(rec[:, 7], want[:, 5 + fish_index])      # channel-0 sum of the reordered image
    centers, low, _, _, _ = interseg.region_rows(rec)
    assert centers == [str(c) for c in z['centers']]
    if fish_index == 0:
        assert np.array_equal(low, want[:, 7].astype(bool))


def test_region_capacity_is_reported_and_retried(gpu, golden_dir):
    z = np.load(os.path.join(golden_dir, SCENES[0]))
    full = gpu.nuclei_regions(z['seg'], z['image'], 0)
    assert np.array_equal(gpu.nuclei_regions(z['seg'], z['image'], 0, capacity=3), full)
    assert np.array_equal(gpu.nuclei_regions(z['seg'], z['image'], 0, capacity=0), full)


def test_instance_id_maps_are_refused(gpu):
    from ecseg_amd._lib import EcsegError
    seg = np.zeros((40, 50), np.uint8)
    seg[2:8, 2:8] = 1
    seg[20:30, 20:30] = 2
    with pytest.raises(EcsegError) as e:
        gpu.nuclei_regions(seg, np.zeros((40, 50, 3), np.uint8), 0)
    assert e.value.code == -1 and 'instance' in str(e.value)
    with pytest.raises(EcsegError):                                # no region map left on the handle
        gpu.nucleus_crops(np.array([[0, 2, 2, 6, 6]], np.int32))


@pytest.mark.parametrize('scene', SCENES)
def test_crops_match_skimage_resize(gpu, golden_dir, scene):
    z = np.load(os.path.join(golden_dir, scene))
    seg, img, win = z['seg'], z['image'], z['windows']
    gpu.nuclei_regions(seg, img, 0)
    from scipy import ndimage as ndi
    lab, _ = ndi.label(seg != 0, structure=np.ones((3, 3), int))
    for order in ((0, 1, 2), (1, 0, 2)):
        crops, cmax = gpu.nucleus_crops(win[:, :5], order)
        assert crops.shape == (len(win), 256, 256, 3)
        km1 = 0
        for k, (r, y0, x0, h, w, _) in enumerate(win):
            exact = exact_resize(img[y0:y0 + h, x0:x0 + w] * (lab[y0:y0 + h, x0:x0 + w] == r + 1)[..., None])[1][..., list(order)]
            d = crops[k].astype(int) - z['crops'][k][..., list(order)]
            assert np.all((d == 0) | ((d == 1) & exact)), (scene, k, int((d != 0).sum()))
            km1 += int((d == 1).sum())
        assert np.array_equal(cmax, crops.max(axis=(1, 2)))
        print('%s order %s: identical but for %d exact-integer pixels where skimage holds k - 1' % (scene, order, km1))
    if scene == 'interseg_scene_large.npz':
        assert any(not c.any() for c, t in zip(crops, win[:, 5]) if t), 'the large scene has an all-zero tile'


def test_crops_refuse_windows_outside_the_map(gpu):
    from ecseg_amd._lib import EcsegError
    seg = np.zeros((20, 30), np.uint8)
    seg[3:9, 4:12] = 255
    gpu.nuclei_regions(seg, np.full((20, 30, 3), 9, np.uint8), 0)
    for bad in ([1, 3, 4, 6, 8], [0, 15, 4, 6, 8], [0, 0, 0, 257, 1], [0, 0, 0, 0, 4], [0, -1, 0, 2, 2]):
        with pytest.raises(EcsegError):
            gpu.nucleus_crops(np.array([bad], np.int32))
    crops, cmax = gpu.nucleus_crops(np.array([[0, 3, 4, 6, 8]], np.int32))
    assert (crops == 9).all() and cmax.tolist() == [[9, 9, 9]]


# ---- `python src/interseg.py` end to end --------------------------------------------------------------------------------
def _expected_rows(z, name, cfg_i, w_i, cfg_c, w_c, fish_index, has_c, quality_pass):
    """Rows of one image from the fixture: region records and crops (skimage) through the CPU oracle of the classifiers;
    None in place of a label whose decision is within MARGIN of a tie."""
    order = [fish_index, 1 - fish_index, 2]
    rec = z['records']
    low = (4 * rec[:, 5 + fish_index] < 51 * rec[:, 0])
    win = z['windows']
    crops = z['crops'][..., order]
    live = [k for k in range(len(win)) if not low[win[k, 0]] and not (win[k, 5] and not crops[k].any())]
    pi = oracle_unet.forward(cfg_i, w_i, crops[live][..., 0]) if live else np.zeros((0, 3))
    pi = dict(zip(live, pi))
    rows = []
    for r in range(len(rec)):
        c = str(z['centers'][r])
        if low[r]:
            rows.append([name, c, interseg.LOW_TRGT] + ([interseg.LOW_TRGT] if has_c else []) + [interseg.LOW_TRGT])
            continue
        for k in np.flatnonzero(win[:, 0] == r):
            if k not in pi:
                rows.append([name, c] + [interseg.EMPTY] * (3 if has_c else 2))
                continue
            p = np.sort(pi[k])
            i_label = interseg.ECSEG_I_LABEL_MAP[int(np.argmax(pi[k]))] if p[-1] - p[-2] >= MARGIN else None
            if not has_c:
                rows.append([name, c, i_label, i_label])
                continue
            if not quality_pass:
                rows.append([name, c, i_label, interseg.FAILED_QUALITY, i_label])
            elif crops[k][..., 1].max() <= 10:
                rows.append([name, c, i_label, interseg.LOW_CENT, i_label])
            else:
                v = float(oracle_unet.forward(cfg_c, w_c, interseg.preprocess_ecseg_c(crops[k])[None]).reshape(-1)[0])
                c_label = interseg.ECSEG_C_LABEL_MAP[int(v > 0.5)] if abs(v - 0.5) >= MARGIN else None
                merged = interseg.INTERSEG_LABEL_MAP[(c_label, i_label)] if c_label and i_label else None
                rows.append([name, c, merged, c_label, i_label])
    return rows


@pytest.fixture(scope='module')
def classifiers(golden_dir):
    return (hdf5_min.load_keras_h5(os.path.join(golden_dir, 'interseg_synth.h5')),
            hdf5_min.load_keras_h5(os.path.join(golden_dir, 'ecseg_c_synth.h5')))


def _folder(tmp_path, golden_dir, has_c, color, extra=()):
    os.makedirs(tmp_path / 'interseg_models')
    shutil.copy(os.path.join(golden_dir, 'interseg_synth.h5'), tmp_path / 'interseg_models' / 'interseg.h5')
    shutil.copy(os.path.join(golden_dir, 'ecseg_c_synth.h5'), tmp_path / 'interseg_models' / 'ecseg_c.h5')
    inp = tmp_path / 'images'
    os.makedirs(inp)
    for scene in SCENES:
        z = np.load(os.path.join(golden_dir, scene))
        stem = scene[:-4]
        Image.fromarray(z['image']).save(str(inp / (stem + '.tif')))
        os.makedirs(inp / 'annotated' / stem)
        image_io.write_tiff_gray8(str(inp / 'annotated' / stem / (stem + '_segmentation.tif')), z['seg'])
    for name in extra:
        image_io.write_tiff_gray8(str(inp / name), np.full((30, 30), 100, np.uint8))      # grayscale: fails per image
    other = ['red', 'green'][1 - (color == 'green')]
    lines = ['image_name,Avg fish intensity (red),Avg fish intensity (green)']
    for v in (3.1, 4.2, 5.0, 4.4, 3.9):
        lines.append('interseg_scene_small,%s,%s' % ((v, 1.0) if other == 'red' else (1.0, v)))
    for v in (1, 1, 1, 1, 1, 1, 1, 1, 1, 90):                       # kurtosis > 3: Failed Centromeric Quality Score
        lines.append('interseg_scene_large,%s,%s' % ((v, 1.0) if other == 'red' else (1.0, v)))
    (inp / 'annotated' / 'stat_fish_lsq.csv').write_text('\n'.join(lines) + '\n')
    with open(tmp_path / 'config.yaml', 'w') as f:
        yaml.safe_dump({'interseg': {'inpath': str(inp), 'FISH_color': color, 'has_centromeric_probe': has_c}}, f)
    return inp


@pytest.mark.parametrize('has_c,color', [(False, 'red'), (True, 'green')])
def test_interseg_cli(tmp_path, golden_dir, classifiers, has_c, color):
    inp = _folder(tmp_path, golden_dir, has_c, color, extra=('zz_gray.tif',) if has_c else ())
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'src', 'interseg.py')], cwd=str(tmp_path), capture_output=True, text=True,
                       timeout=600)
    print(r.stdout[-3000:], r.stderr[-3000:])
    assert r.returncode == (1 if has_c else 0), r.stderr
    if has_c:
        assert "zz_gray.tif - isn't an RGB image" in r.stdout and '1 image(s) were NOT processed' in r.stdout
    with open(inp / ('interphase_prediction_%s.csv' % color), newline='') as f:
        got = list(csv.reader(f))
    assert got[0] == interseg.csv_columns(has_c)
    fish_index = 1 if color == 'green' else 0
    (cfg_i, w_i), (cfg_c, w_c) = classifiers
    want = []
    for scene in sorted(SCENES):                                   # the driver takes the images in sorted order
        z = np.load(os.path.join(golden_dir, scene))
        want += _expected_rows(z, scene[:-4], cfg_i, w_i, cfg_c, w_c, fish_index, has_c, quality_pass=scene == SCENES[0])
    assert len(got) - 1 == len(want)
    skipped = 0
    for g, w in zip(got[1:], want):
        for a, b in zip(g, w):
            if b is None:
                skipped += 1
            else:
                assert a == b, (g, w)
    print('%d rows compared, %d labels within %g of a tie skipped' % (len(want), skipped, MARGIN))
    assert any(interseg.EMPTY in row for row in got) and any(interseg.LOW_TRGT in row for row in got)
    if has_c:
        assert any(interseg.FAILED_QUALITY in row for row in got)


def test_interseg_cli_reports_missing_inputs_per_image(tmp_path, golden_dir):
    inp = _folder(tmp_path, golden_dir, True, 'red')
    os.remove(inp / 'annotated' / 'stat_fish_lsq.csv')
    os.remove(inp / 'annotated' / 'interseg_scene_large' / 'interseg_scene_large_segmentation.tif')
    big = np.zeros((600, 100), np.uint8)
    big[5:20, 5:20] = 255
    image_io.write_tiff_gray8(str(inp / 'annotated' / 'interseg_scene_small' / 'interseg_scene_small_segmentation.tif'), big)
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'src', 'interseg.py')], cwd=str(tmp_path), capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 1, r.stderr
    assert 'stat_fish_lsq.csv cannot be read' in r.stdout and '2 image(s) were NOT processed' in r.stdout
    # without a centromeric probe the table is not needed; the segmentation problems remain
    yaml.safe_dump({'interseg': {'inpath': str(inp), 'FISH_color': 'red', 'has_centromeric_probe': False}},
                   open(tmp_path / 'config.yaml', 'w'))
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'src', 'interseg.py')], cwd=str(tmp_path), capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 1, r.stderr
    assert 'is larger than the image' in r.stdout and 'has no segmentation' in r.stdout
    assert open(inp / 'interphase_prediction_red.csv').read() == 'image_name,nucleus_center,interSeg_label,ecSeg-i_label\n'
