"""``interseg.batch: k`` without a GPU: ``interseg.main`` at ``batch: 1`` and ``batch: k`` on the same folders, through a handle whose
device calls are the CPU oracle's (oracle/interseg.py) and whose ``interseg_many`` is built from those per-image calls - the CSV bytes,
the stdout lines and the exit code must not differ; the validation of the key; and the planning header of ecseg_interseg_batch
(csrc/iseg_batch.h) compiled for the host under ASan + UBSan (tools/asan/iseg_batch_check.cpp, ``make asan_iseg_batch``)."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import yaml

from ecseg_amd import image_io, interseg
from ecseg_amd._lib import EcsegError
from oracle import interseg as oracle_interseg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class TableModel:
    """A classifier whose prediction is a function of the crop's content: ecSeg-i from the target channel's sum, ecSeg-c from the
    probe channel's."""
    def __init__(self, n_out):
        self.n_out = n_out

    def predict(self, x):
        x = np.asarray(x, np.float32)
        s = x.reshape(len(x), -1).sum(axis=1)
        if self.n_out == 3:
            p = np.stack([np.float32(1) + s % 3, np.float32(1) + s % 5, np.float32(1) + s % 7], axis=1).astype(np.float32)
            return p / p.sum(axis=1, keepdims=True)
        return (np.float32(0.25) + (np.nan_to_num(s) % 2) * np.float32(0.5)).astype(np.float32).reshape(-1, 1)


class PerImageHandle:
    """The device calls of ``process_image`` restated by the CPU oracle: a handle of before the feature."""
    def __init__(self):
        self.calls = []

    def nuclei_regions(self, seg, img, channel0, capacity=4096):
        self.calls.append('nuclei_regions')
        vals = np.unique(seg[seg != 0])
        if len(vals) > 1:
            e = EcsegError('ecseg_nuclei_regions failed (-1): segmentation holds the non-zero values %d .. %d: only 0 / non-zero nucleus '
                           'masks are supported, not instance-id maps' % (vals.min(), vals.max()))
            e.code = -1
            raise e
        rec, self.lab = oracle_interseg.region_records(seg, img, channel0)
        self.img = img
        return rec

    def _crops(self, desc, order):
        crops = np.stack([oracle_interseg.nucleus_crop(self.img, self.lab, *[int(v) for v in d], order=order) for d in desc])
        return crops, crops.reshape(len(crops), -1, 3).max(axis=1).astype(np.int32)

    def classify_nucleus_crops(self, desc, order, from_patches, centromeric, model_i, model_c=None, want_crops=False):
        self.calls.append('classify_nucleus_crops')
        crops, mx = self._crops(desc, order)
        n = len(desc)
        ran_i = ~(np.broadcast_to(np.asarray(from_patches, bool), (n,)) & (mx.max(axis=1) == 0))
        ran_c = ran_i & bool(centromeric and model_c is not None) & (mx[:, 1] > 10)
        pred_i, pred_c = np.zeros((n, 3), np.float32), np.zeros(n, np.float32)
        if ran_i.any():
            pred_i[ran_i] = model_i.predict(crops[ran_i][..., 0])
        if ran_c.any():
            pred_c[ran_c] = model_c.predict(np.stack([interseg.preprocess_ecseg_c(c) for c in crops[ran_c]])).reshape(-1)
        return mx, pred_i, ran_i, pred_c, ran_c


class OracleHandle(PerImageHandle):
    """... and ``interseg_many`` made of exactly those calls, per image."""
    def interseg_many(self, images, segs, fish_index, quality_pass, model_i, model_c=None):
        self.calls.append(('interseg_many', len(images)))
        out = []
        for img, seg, q in zip(images, segs, quality_pass):
            assert img.dtype == np.uint8 and seg.dtype == np.uint8 and img.flags.c_contiguous and seg.flags.c_contiguous
            try:
                rec = OracleHandle.nuclei_regions(self, seg, img, fish_index)
            except EcsegError as e:
                out.append(e)
                continue
            _, _, desc, tiled, owner = interseg.region_rows(rec)
            if len(desc):
                _, pi, ri, pc, rc = OracleHandle.classify_nucleus_crops(self, desc, (fish_index, 1 - fish_index, 2), tiled,
                                                                        model_c is not None and q, model_i, model_c)
            else:
                pi, ri, pc, rc = np.zeros((0, 3), np.float32), np.zeros(0, bool), np.zeros(0, np.float32), np.zeros(0, bool)
            out.append((rec, (owner, pi, ri, pc, rc)))
        self.calls = [c for c in self.calls if isinstance(c, tuple)]       # (the oracle calls above are interseg_many's own)
        return out


def _scene(rng, k, empty=False):
    H, W = 40 + 3 * k, 52 + 5 * k
    seg = np.zeros((H, W), np.uint8)
    if not empty:
        seg[2:12 + k, 3:14] = 255
        seg[20:33, 20 + k:41] = 255
        seg[H - 4:H - 1, 1:9] = 255                            # dim below: fails the brightness gate
    img = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    img[..., :2][seg != 0] |= 32
    img[H - 4:H - 1, 1:9, :2] = 3
    return img, seg


def _folder(root, n, broken=None, empty=None):
    """n images a0.tif ..; ``broken``: (index, kind) with kind 'missing' (no segmentation), 'gray' (a single-channel image) or 'ids' (an
    instance-id map); ``empty``: the index of an image without nuclei."""
    rng = np.random.default_rng(n)
    os.makedirs(root / 'annotated', exist_ok=True)
    for k in range(n):
        img, seg = _scene(rng, k, empty=(k == empty))
        kind = broken[1] if broken and broken[0] == k else None
        name = 'a%d' % k
        if kind == 'gray':
            image_io.write_tiff_gray8(str(root / (name + '.tif')), img[..., 0])
        else:
            image_io.write_tiff_rgb8(str(root / (name + '.tif')), img)
        if kind == 'ids':
            seg[20:33] = np.where(seg[20:33] != 0, 9, 0).astype(np.uint8)
        if kind != 'missing':
            os.makedirs(root / 'annotated' / name, exist_ok=True)
            image_io.write_tiff_gray8(str(root / 'annotated' / name / (name + '_segmentation.tif')), seg)
    return str(root)


def _run(tmp_path, monkeypatch, capsys, inp, handle, probe=False, **cfg):
    from ecseg_amd import utils
    monkeypatch.chdir(tmp_path)
    models = {interseg.ECSEG_I_MODEL: TableModel(3), interseg.ECSEG_C_MODEL: TableModel(1)}
    for m in models.values():
        m.handle = handle
    monkeypatch.setattr(utils, 'load_model', lambda name, device=None: models[name])
    yaml.safe_dump({'interseg': dict(inpath=inp, FISH_color='red', has_centromeric_probe=probe, **cfg)}, open(tmp_path / 'config.yaml', 'w'))
    csv_path = os.path.join(inp, 'interphase_prediction_red.csv')
    if os.path.exists(csv_path):
        os.remove(csv_path)
    code = 0
    try:
        interseg.main([])
    except SystemExit as e:
        code = e.code
    return code, capsys.readouterr().out, open(csv_path, 'rb').read() if os.path.exists(csv_path) else None


def _both(tmp_path, monkeypatch, capsys, inp, k, probe=False):
    one = _run(tmp_path, monkeypatch, capsys, inp, OracleHandle(), probe, classify_on_device=True, batch=1)
    h = OracleHandle()
    many = _run(tmp_path, monkeypatch, capsys, inp, h, probe, classify_on_device=True, batch=k)
    assert many[2] == one[2] and one[2] is not None           # the CSV, byte for byte
    assert many[1].splitlines() == one[1].splitlines()
    assert many[0] == one[0]
    return one, h


def test_five_images_two_at_a_time(tmp_path, monkeypatch, capsys):
    inp = _folder(tmp_path / 'images', 5)
    one, h = _both(tmp_path, monkeypatch, capsys, inp, 2)
    assert one[0] == 0 and one[2].count(b'\n') == 1 + 5 * 3
    assert h.calls == [('interseg_many', 2), ('interseg_many', 2), ('interseg_many', 1)]     # ONE call per chunk; a chunk of one at the end


@pytest.mark.parametrize('kind', ['missing', 'gray', 'ids'])
def test_the_middle_image_of_a_chunk_fails_alone(tmp_path, monkeypatch, capsys, kind):
    inp = _folder(tmp_path / 'images', 4, broken=(1, kind))
    one, h = _both(tmp_path, monkeypatch, capsys, inp, 3)
    assert one[0] == 1 and '1 image(s) were NOT processed' in one[1]
    assert one[2].count(b'\n') == 1 + 3 * 3 and b'a1,' not in one[2] and b'a0,' in one[2] and b'a2,' in one[2] and b'a3,' in one[2]
    assert h.calls == [('interseg_many', 3 if kind == 'ids' else 2), ('interseg_many', 1)]     # what could not be read never reaches the device


def test_an_image_without_nuclei(tmp_path, monkeypatch, capsys):
    inp = _folder(tmp_path / 'images', 3, empty=1)
    one, _ = _both(tmp_path, monkeypatch, capsys, inp, 3)
    assert one[0] == 0 and b'a1,' not in one[2] and one[2].count(b'\n') == 1 + 2 * 3


def test_centromeric_probe_with_one_image_failing_the_quality_score(tmp_path, monkeypatch, capsys):
    inp = _folder(tmp_path / 'images', 3)
    rows = ['image_name,Avg fish intensity (green)']
    rows += ['a0,%d' % v for v in (1, 2, 3, 4)]
    rows += ['a1,%d' % v for v in (1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 200)]     # kurtosis far above 3
    rows += ['a2,%d' % v for v in (5, 6, 7, 9)]
    open(os.path.join(inp, 'annotated', 'stat_fish_lsq.csv'), 'w').write('\n'.join(rows) + '\n')
    one, _ = _both(tmp_path, monkeypatch, capsys, inp, 3, probe=True)
    text = one[2].decode()
    assert one[0] == 0 and text.count(interseg.FAILED_QUALITY) == 2 and all(interseg.FAILED_QUALITY in line for line in text.splitlines() if
                                                                           line.startswith('a1,') and interseg.LOW_TRGT not in line)
    assert not any(interseg.FAILED_QUALITY in line for line in text.splitlines() if not line.startswith('a1,'))
    # ... and without the table every image fails the same way in both modes
    os.remove(os.path.join(inp, 'annotated', 'stat_fish_lsq.csv'))
    one, h = _both(tmp_path, monkeypatch, capsys, inp, 2, probe=True)
    assert one[0] == 1 and h.calls == []


@pytest.mark.parametrize('value', [0, -1, 2.5, '8', True])
@pytest.mark.parametrize('on_device', [True, False])
def test_batch_must_be_a_positive_integer(tmp_path, monkeypatch, capsys, value, on_device):
    inp = _folder(tmp_path / 'images', 1)
    code, out, text = _run(tmp_path, monkeypatch, capsys, inp, OracleHandle(), classify_on_device=on_device, batch=value)
    assert code == 2 and 'interseg.batch must be a positive integer' in out and text is None


def test_batch_without_classify_on_device_is_batch_1(tmp_path, monkeypatch, capsys):
    inp = _folder(tmp_path / 'images', 3)

    class HostHandle(OracleHandle):
        def nucleus_crops(self, desc, order=(0, 1, 2)):
            return self._crops(np.asarray(desc)[:, :5], order)
    one = _run(tmp_path, monkeypatch, capsys, inp, HostHandle(), batch=1)
    h = HostHandle()
    four = _run(tmp_path, monkeypatch, capsys, inp, h, batch=4)
    assert four == one and one[0] == 0 and not any(isinstance(c, tuple) for c in h.calls)


def test_batch_needs_a_handle_with_the_call(tmp_path, monkeypatch, capsys):
    inp = _folder(tmp_path / 'images', 2)
    code, out, text = _run(tmp_path, monkeypatch, capsys, inp, PerImageHandle(), classify_on_device=True, batch=2)
    assert code == 2 and 'needs the batched device path (interseg_many)' in out and text is None


def test_the_header_the_binding_and_the_documents_name_the_feature():
    from ecseg_amd._lib import EXPORTS, Handle
    header = open(os.path.join(ROOT, 'include', 'ecseg_hip.h')).read()
    assert re.search(r'\becseg_interseg_batch\s*\(', header) and 'ecseg_interseg_batch' in EXPORTS and hasattr(Handle, 'interseg_many')
    cfg = open(os.path.join(ROOT, 'config.yaml')).read()
    assert re.search(r'^  # batch: \d+', cfg, re.M) and yaml.safe_load(cfg)['interseg'].get('batch', 1) == 1
    for doc in ('README.md', 'DESIGN.md', 'INTEGRATION.md'):
        assert 'interseg_batch' in open(os.path.join(ROOT, doc)).read() or 'interseg.batch' in open(os.path.join(ROOT, doc)).read(), doc


# ---- the planning header on the host --------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def check_program(tmp_path_factory):
    if not shutil.which('g++') or not shutil.which('make'):
        pytest.skip('no host toolchain')
    exe = str(tmp_path_factory.mktemp('isegb') / 'iseg_batch_check')
    out = subprocess.run(['make', '-C', ROOT, 'asan_iseg_batch', 'ISEG_BATCH_CHECK=' + exe], capture_output=True, text=True, timeout=900)
    if 'cannot find' in out.stderr and 'asan' in out.stderr:
        pytest.skip('libasan not installed')
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-3000:]
    assert 'iseg_batch_check: ok' in out.stdout
    return exe


def test_make_asan_iseg_batch_builds_and_runs_clean(check_program):
    assert os.path.exists(check_program)
    mk = open(os.path.join(ROOT, 'Makefile')).read()
    assert 'asan_iseg_batch:' in mk and '-fsanitize=address,undefined' in mk.split('asan_iseg_batch:')[1]


def test_the_headers_crop_windows_are_crop_windows(check_program):
    out = subprocess.run([check_program, 'windows'], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-3000:]
    lines = out.stdout.strip().splitlines()
    assert len(lines) == 144
    for line in lines:
        head, tail = line.split('|')
        h, w = (int(v) for v in head.split())
        got = [int(v) for v in tail.split()]
        assert [tuple(got[i:i + 4]) for i in range(0, len(got), 4)] == interseg.crop_windows(h, w), line
