"""interSeg's classifiers on the device, the parts that need no GPU: the per-element function of the ecSeg-c input and the selection
and chunk planning of ecseg_classify_nucleus_crops (csrc/iseg_classify.h) compiled for the host under ASan + UBSan
(tools/asan/iseg_classify_check.cpp, ``make asan_iseg_classify``) and held to numpy and to the rules of ``classify_crops``;
``rows_from_predictions`` against ``classify_crops``; the config key ``interseg.classify_on_device``."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import yaml

from ecseg_amd import image_io, interseg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def check_program(tmp_path_factory):
    """The program `make asan_iseg_classify` builds, built into a directory of this run; the target's own run must be clean."""
    if not shutil.which('g++') or not shutil.which('make'):
        pytest.skip('no host toolchain')
    exe = str(tmp_path_factory.mktemp('iseg') / 'iseg_classify_check')
    out = subprocess.run(['make', '-C', ROOT, 'asan_iseg_classify', 'ISEG_CHECK=' + exe], capture_output=True, text=True, timeout=900)
    if 'cannot find' in out.stderr and 'asan' in out.stderr:
        pytest.skip('libasan not installed')
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-3000:]
    assert 'iseg_classify_check: ok' in out.stdout
    return exe


def test_make_asan_iseg_classify_builds_and_runs_clean(check_program):
    assert os.path.exists(check_program)
    mk = open(os.path.join(ROOT, 'Makefile')).read()
    assert 'asan_iseg_classify:' in mk and '-fsanitize=address,undefined' in mk.split('asan_iseg_classify:')[1]


def test_per_element_function_is_numpys_float32_arithmetic_for_every_pair(check_program, tmp_path):
    path = str(tmp_path / 'values.bin')
    out = subprocess.run([check_program, 'values', path], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-3000:]
    got = np.fromfile(path, np.uint32).reshape(256, 256)                      # [max, x]
    x = np.arange(256, dtype=np.float32)[None, :]
    m = np.arange(256, dtype=np.float32)[:, None]
    with np.errstate(divide='ignore', invalid='ignore'):
        want = (np.rint((x / m) * np.float32(255)) / np.float32(255)).astype(np.float32)
    assert want.dtype == np.float32 and np.isnan(want[0, 0]) and np.isinf(want[0, 1:]).all()
    gf = got.view(np.float32)
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(gf), nan)                                  # NaN is matched as NaN
    assert np.array_equal(got[~nan], want.view(np.uint32)[~nan])
    # and it is preprocess_ecseg_c on a crop: every byte value in channel 0 (max 255), a channel of maximum 1, an all-zero channel
    crop = np.zeros((256, 256, 3), np.uint8)
    crop[..., 0] = np.arange(65536).reshape(256, 256) % 256
    crop[0, :2, 1] = (1, 0)
    pre = interseg.preprocess_ecseg_c(crop)
    for c in range(3):
        mx = int(crop[..., c].max())
        assert np.array_equal(pre[..., c].view(np.uint32), got[mx][crop[..., c]])


def _case_crop(pattern, j):
    """(maxima, from_patches) of crop j: tools/asan/iseg_classify_check.cpp, case_crop."""
    if pattern == 0:
        return (20, 20 + j % 200, 7), j % 3 == 0
    if pattern == 1:
        return (0, 0, 0), True
    if pattern == 2:
        return ((5, 11, 0) if j % 2 == 0 else (0, 0, 0)), True
    return (0, (10, 11, 0, 0)[j % 4], 0), False


def test_selection_and_chunks_are_classify_crops_rules(check_program):
    out = subprocess.run([check_program, 'plan'], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-3000:]
    got = {}
    for line in out.stdout.splitlines():
        head, crops, runs = line.split('|')
        n, g, pattern, cent, chunk, model = head.split()
        got[(int(n), int(g), int(pattern), int(cent), int(chunk), model)] = ([int(v) for v in crops.split()], [int(v) for v in runs.split()])
    want = {}
    for n in (0, 1, 255, 256, 257, 600):
        for g in (1, 7, 64):
            for pattern in range(4):
                for cent in (0, 1):
                    cases = [_case_crop(pattern, j) for j in range(n)]
                    # classify_crops: ecSeg-i but for all-zero tiles; ecSeg-c for those, with the image's flag, when the probe is above 10
                    run_i = [not (fp and max(m) == 0) for m, fp in cases]
                    run_c = [bool(ri and cent and m[1] > 10) for ri, (m, fp) in zip(run_i, cases)]
                    for chunk in range((n + 255) // 256):
                        for model, run in (('i', run_i), ('c', run_c)):
                            sel = [j for j in range(256 * chunk, min(n, 256 * chunk + 256)) if run[j]]
                            want[(n, g, pattern, cent, chunk, model)] = (sel, [len(sel[a:a + g]) for a in range(0, len(sel), g)])
    assert got == want
    assert len(want) == 2 * 4 * 2 * 3 * (1 + 1 + 1 + 2 + 3)
    assert want[(257, 7, 0, 1, 1, 'i')] == ([256], [1]) and want[(600, 64, 1, 1, 0, 'i')] == ([], [])
    assert want[(600, 7, 2, 1, 2, 'c')][1] == [7] * 6 + [2]                    # every other one of the last 88 crops: 44


class _Model:
    """predict() from a table: row k of the call's input is recognised by the value the test put into its first sample."""
    def __init__(self, table):
        self.table, self.calls = np.asarray(table, np.float32), []

    def predict(self, x):
        x = np.asarray(x)
        self.calls.append(x.shape)
        return self.table[[int(round(float(v.reshape(-1)[0]) * (255 if x.dtype.kind == 'f' else 1))) for v in x]]


def _hand_predictions():
    # crop k carries k + 1 in sample (0, 0) of every channel, 255 in the rows below in channels 0 and 2 (so that the ecSeg-c input
    # holds (k + 1) / 255 there); channel 1: bright but for crops 3 and 5
    n = 7
    crops = np.zeros((n, 256, 256, 3), np.uint8)
    crops[:, 1:, :, 0] = 255
    crops[:, 1:, :, 2] = 255
    crops[:, 0, 0, :] = np.arange(1, n + 1)[:, None]
    crops[:, 5, 5, 1] = 255
    crops[3, 5, 5, 1] = 10                                                    # the gate: 10 is too dim
    crops[5, 5, 5, 1] = 11                                                    # 11 is not
    crops[2] = 0                                                              # an empty tile
    tiled = np.array([0, 1, 1, 0, 1, 0, 0], bool)
    ti = np.zeros((256, 3), np.float32)
    ti[1:8] = [[0.3, 0.6, 0.1], [0.1, 0.2, 0.7], [9, 9, 9], [0.5, 0.25, 0.25], [0.2, 0.2, 0.6], [0.1, 0.8, 0.1], [0.7, 0.2, 0.1]]
    tc = np.zeros((256, 1), np.float32)
    tc[1:8, 0] = [0.3, 0.9, 9, 9, 0.50000006, 0.5, np.float32(1) / np.float32(3)]
    return crops, tiled, ti, tc


@pytest.mark.parametrize('has_c,quality', [(True, True), (True, False), (False, True)])
def test_rows_from_predictions_reproduces_classify_crops_row_for_row(has_c, quality):
    crops, tiled, ti, tc = _hand_predictions()
    n = len(crops)
    mi, mc = _Model(ti), (_Model(tc) if has_c else None)
    want = interseg.classify_crops(mi, crops, mc, quality, from_patches=tiled, channel_max=crops.max(axis=(1, 2)).astype(np.int32))
    # the same predictions as the device call hands them over: full-length arrays, rows of crops a model did not see untouched
    ran_i = ~(tiled & (crops.max(axis=(1, 2, 3)) == 0))
    ran_c = ran_i & (has_c and quality) & (crops[..., 1].max(axis=(1, 2)) > 10)
    assert ran_i.tolist() == [True, True, False, True, True, True, True]
    assert ran_c.tolist() == ([True, True, False, False, True, True, True] if has_c and quality else [False] * n)
    pred_i = np.full((n, 3), -7, np.float32)
    pred_c = np.full(n, -7, np.float32)
    pred_i[ran_i] = ti[1:8][ran_i]
    pred_c[ran_c] = tc[1:8, 0][ran_c]
    got = interseg.rows_from_predictions(has_c, quality, ran_i, pred_i, ran_c, pred_c)
    assert len(got) == len(want) == n
    for g, w in zip(got, want):
        assert list(g.items()) == list(w.items())                              # keys, order and values
        assert [type(v) for v in g.values()] == [type(v) for v in w.values()]
    assert got[2]['pred_ec'] == interseg.EMPTY and got[2]['interSeg_label'] == interseg.EMPTY
    if has_c and quality:
        assert got[3]['ecSeg-c_label'] == interseg.LOW_CENT and got[3]['pred_focal_amp'] == interseg.LOW_CENT
        assert got[2]['ecSeg-c_label'] == interseg.EMPTY
        v = np.float32(1) / np.float32(3)
        assert got[6]['pred_no_focal_amp'] == np.float32(1) - v and isinstance(got[6]['pred_no_focal_amp'], np.float32)
        assert np.float64(got[6]['pred_no_focal_amp']) != np.float64(1) - np.float64(v)       # the float32 complement, not the float64 one
        assert got[4]['ecSeg-c_label'] == 'Focal-amp' and got[5]['ecSeg-c_label'] == 'No-amp'       # 0.50000006 > 0.5, 0.5 is not
        assert got[1]['interSeg_label'] == 'HSR-amp' and got[0]['interSeg_label'] == 'No-amp'
    elif has_c:
        assert all(r['ecSeg-c_label'] == interseg.FAILED_QUALITY for k, r in enumerate(got) if k != 2)
    else:
        assert all('ecSeg-c_label' not in r for r in got)


# ---- the configuration key ------------------------------------------------------------------------------------------------------
class PlainHandle:
    """A handle of before the feature: regions and crops only."""
    def __init__(self):
        self.calls = []

    def nuclei_regions(self, seg, img, channel0, capacity=4096):
        self.calls.append(('nuclei_regions', seg.shape, img.shape, channel0))
        return np.array([[36, 2, 2, 8, 8, 36 * 5, 36 * 5, 36 * 100], [16, 10, 10, 14, 14, 16 * 12, 16 * 12, 16 * 3]], np.int64)

    def nucleus_crops(self, desc, order=(0, 1, 2)):
        self.calls.append(('nucleus_crops', np.asarray(desc).tolist(), tuple(order)))
        crops = np.zeros((len(desc), 256, 256, 3), np.uint8)
        crops[:, 0, 0, :] = 1
        return crops, crops.max(axis=(1, 2)).astype(np.int32)


class DeviceHandle(PlainHandle):
    def classify_nucleus_crops(self, desc, order, from_patches, centromeric, model_i, model_c=None, want_crops=False):
        self.calls.append(('classify_nucleus_crops', np.asarray(desc).tolist(), tuple(order), np.asarray(from_patches).tolist(), bool(centromeric),
                           model_c is not None))
        n = len(desc)
        return (np.ones((n, 3), np.int32), np.tile(model_i.table[1], (n, 1)), np.ones(n, bool), np.zeros(n, np.float32), np.zeros(n, bool))


def _interseg_folder(root):
    os.makedirs(root / 'annotated' / 'a')
    image_io.write_tiff_rgb8(str(root / 'a.tif'), np.full((20, 24, 3), 100, np.uint8))
    seg = np.zeros((20, 24), np.uint8)
    seg[2:8, 2:8] = 255
    seg[10:14, 10:14] = 255
    image_io.write_tiff_gray8(str(root / 'annotated' / 'a' / 'a_segmentation.tif'), seg)
    return str(root)


def _run_main(tmp_path, monkeypatch, handle, **cfg):
    from ecseg_amd import utils
    inp = _interseg_folder(tmp_path / 'images')
    monkeypatch.chdir(tmp_path)
    table = np.zeros((256, 3), np.float32)
    table[1] = (0.2, 0.7, 0.1)
    model = _Model(table)
    model.handle = handle
    monkeypatch.setattr(utils, 'load_model', lambda name, device=None: model)
    yaml.safe_dump({'interseg': dict(inpath=inp, FISH_color='red', has_centromeric_probe=False, **cfg)}, open(tmp_path / 'config.yaml', 'w'))
    interseg.main([])
    return model, open(os.path.join(inp, 'interphase_prediction_red.csv')).read()


@pytest.mark.parametrize('value', [1, 'yes', 'true', [True], 0])
def test_classify_on_device_must_be_a_boolean(tmp_path, monkeypatch, capsys, value):
    with pytest.raises(SystemExit) as e:
        _run_main(tmp_path, monkeypatch, DeviceHandle(), classify_on_device=value)
    assert e.value.code == 2 and 'interseg.classify_on_device must be true or false' in capsys.readouterr().out
    assert not os.path.exists(tmp_path / 'images' / 'interphase_prediction_red.csv')


def test_classify_on_device_needs_a_handle_with_the_call(tmp_path, monkeypatch, capsys):
    with pytest.raises(SystemExit) as e:
        _run_main(tmp_path, monkeypatch, PlainHandle(), classify_on_device=True)
    assert e.value.code == 2 and 'classify_on_device: true needs the device classifier path' in capsys.readouterr().out
    assert not os.path.exists(tmp_path / 'images' / 'interphase_prediction_red.csv')


def test_the_key_absent_or_false_runs_todays_path_and_true_makes_one_call_per_image(tmp_path, monkeypatch, capsys):
    runs = {}
    for name, handle, cfg in (('absent', DeviceHandle(), {}), ('off', DeviceHandle(), {'classify_on_device': False}), ('plain', PlainHandle(), {}),
                              ('on', DeviceHandle(), {'classify_on_device': True})):
        os.makedirs(tmp_path / name)
        model, text = _run_main(tmp_path / name, monkeypatch, handle, **cfg)
        runs[name] = (handle.calls, model.calls, text, capsys.readouterr().out.replace(str(tmp_path / name), ''))
    desc = [[0, 2, 2, 6, 6]]                                                   # region 1 is below the brightness gate: no crop
    assert runs['plain'][0] == [('nuclei_regions', (20, 24), (20, 24, 3), 0), ('nucleus_crops', desc, (0, 1, 2))]
    assert runs['plain'][1] == [(1, 256, 256)]
    assert runs['absent'] == runs['off'] == runs['plain']
    assert runs['on'][0] == [('nuclei_regions', (20, 24), (20, 24, 3), 0), ('classify_nucleus_crops', desc, (0, 1, 2), [False], False, False)]
    assert runs['on'][1] == []                                                 # no crop came to the host
    assert runs['on'][2:] == runs['off'][2:]                                   # the CSV text and the messages
    assert runs['on'][2] == ('image_name,nucleus_center,interSeg_label,ecSeg-i_label\na,5_5,EC-amp,EC-amp\n'
                             'a,12_12,%s,%s\n' % (interseg.LOW_TRGT, interseg.LOW_TRGT))


def test_the_documents_the_header_and_the_binding_name_the_feature():
    from ecseg_amd._lib import ABI_VERSION, EXPORTS, Handle
    header = open(os.path.join(ROOT, 'include', 'ecseg_hip.h')).read()
    for name in ('ecseg_classify_nucleus_crops', 'ecseg_iseg_classifier_inputs_debug'):
        assert re.search(r'\b%s\s*\(' % name, header) and name in EXPORTS
    assert ABI_VERSION == 6 and hasattr(Handle, 'classify_nucleus_crops')
    assert re.search(r'^  # classify_on_device: true', open(os.path.join(ROOT, 'config.yaml')).read(), re.M)
    assert yaml.safe_load(open(os.path.join(ROOT, 'config.yaml')))['interseg'].get('classify_on_device', False) is False
    for doc in ('README.md', 'DESIGN.md', 'INTEGRATION.md'):
        assert 'classify_on_device' in open(os.path.join(ROOT, doc)).read(), doc
    from ecseg_amd import build
    assert build.EXTRA_FLAGS['iseg_classify_kernels.hip'] == ['-ffp-contract=off'] and 'iseg_classify_kernels.hip' in build.SOURCES
