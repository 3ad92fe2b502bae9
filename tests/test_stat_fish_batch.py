"""``stat_fish.batch`` without a GPU: the layout header of ecseg_stat_fish_batch (csrc/fish_batch.h) compiled for the host under ASan +
UBSan (tools/asan/fish_batch_check.cpp, ``make asan_fish_batch``), the configuration rules of the key, and ``main`` at ``batch`` 1, 2
and 8 on an injected handle whose ``stat_fish_many`` is composed from tests/stat_fish_ref.py and the host writers."""
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest
import yaml

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lzw_ref                               # noqa: E402
import stat_fish_ref as ref                  # noqa: E402
import test_stat_fish_aqua as cpu            # noqa: E402
import test_tiff_encode as te                # noqa: E402
from ecseg_amd import _lib, image_io         # noqa: E402
from ecseg_amd import stat_fish as sf        # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class BatchFishHandle(te.TiffOracleHandle):
    """A handle whose ``stat_fish_many`` is the oracle per item: labels, records, the restated colour files, the host TIFF writer."""
    fail_at = None                               # the index of the stat_fish_many call that is refused

    def stat_fish_many(self, items, line_thickness, record_capacity=4096, budget_bytes=8 << 30, want_masks=False):
        n_before = len([c for c in self.calls if 'stat_fish_many' in c])
        self.calls.append(dict(stat_fish_many=len(items)))
        if self.fail_at == n_before:
            e = _lib.EcsegError('ecseg_stat_fish_batch failed (-1)')
            e.code = -1
            raise e
        out = []
        for it in items:
            assert set(it) <= set(_lib.Handle.STAT_FISH_ITEM_KEYS) and (it.get('mask') is None) != (it.get('labels') is None)
            seg = ref.nuclei(it['mask']) if it.get('mask') is not None else it['labels']
            rec, thr, bnd, _ = ref.loop(it['img'], seg, list(it['channels'][1:]), np.asarray(it['weights'], np.float64), it['normal_threshold'],
                                        it['intensity_thresholds'], it['min_cc_size'], line_thickness)
            rasters = cpu.RenderingOracleHandle.fish_render(self, it['img'], it['channels'], thr, bnd)
            self.calls.pop()                                     # (the render inside is not a call of main's)
            mask_file = it['mask'] if it.get('mask_file') is True else it.get('mask_file')
            files = tuple(lzw_ref.tiff_file(r) for r in rasters) + (None if mask_file is None else lzw_ref.tiff_file(mask_file),
                                                                    None if it.get('picture') is None else lzw_ref.tiff_file(it['picture']))
            out.append((ref.ranks(seg)[0].astype(np.int32), rec, files))
        return out


def _set_key(tmp_path, **keys):
    cfg = yaml.safe_load(open(tmp_path / 'config.yaml'))
    cfg['stat_fish'].update(keys)
    yaml.safe_dump(cfg, open(tmp_path / 'config.yaml', 'w'))


def _five_images(tmp_path):
    """five small images: one file unreadable, one image without a nucleus"""
    inp, _ = cpu.make_folder(tmp_path, kinds=(('img_0', 'tif'), ('img_1', 'tif'), ('img_4', 'npy8')), size=(40, 50))
    shutil.copyfile(inp / 'img_0.tif', inp / 'img_3.tif')
    image_io.write_tiff_gray8(str(inp / 'nuclei_masks' / 'img_3.tif'), np.zeros((40, 50), np.uint8))      # no nucleus
    (inp / 'img_2.tif').write_bytes(b'II*\x00 not a TIFF')                                                # unreadable
    shutil.copyfile(inp / 'nuclei_masks' / 'img_0.tif', inp / 'nuclei_masks' / 'img_2.tif')
    return inp


def _run(tmp_path, inp, capsys, handle=None, **keys):
    _set_key(tmp_path, **keys)
    handle = handle or BatchFishHandle()
    code = 0
    try:
        sf.main([], handle=handle)
    except SystemExit as e:
        code = e.code
    got = cpu.folder_bytes(inp / 'annotated')
    shutil.rmtree(inp / 'annotated')
    return got, code, capsys.readouterr().out, handle.calls


def test_batch_1_2_and_8_write_identical_trees_and_csv(tmp_path, monkeypatch, capsys):
    inp = _five_images(tmp_path)
    monkeypatch.chdir(tmp_path)
    one = _run(tmp_path, inp, capsys, tiff_on_device=True, batch=1)
    assert one[1] == 1 and 'img_2.tif - cannot be read' in one[2] and '1 image(s) were NOT processed' in one[2]
    assert len(one[0]) == 4 * 5 + 2 and one[0]['stat_fish_lsq.csv'].count(b'\n') > 4 and not [c for c in one[3] if 'stat_fish_many' in c]
    assert not [r for r in one[0]['stat_fish_lsq.csv'].decode().split('\n') if r.startswith('img_3,')], 'the image without a nucleus has no row'
    for k, sizes in ((2, [2, 2]), (8, [4])):
        got = _run(tmp_path, inp, capsys, tiff_on_device=True, batch=k)
        assert got[1] == 1 and got[2] == one[2], 'exit code and messages at batch %d' % k
        assert [c['stat_fish_many'] for c in got[3] if 'stat_fish_many' in c] == sizes, 'the unreadable image is in no chunk'
        assert not [c for c in got[3] if 'render_tiff' in c or 'tiff' in c or 'probes' in c], 'nothing runs one image at a time'
        assert sorted(got[0]) == sorted(one[0])
        for name in one[0]:
            assert got[0][name] == one[0][name], (k, name)
    # tiff_write_batch is ignored above 1: the chunk's files are encoded in its own call
    both = _run(tmp_path, inp, capsys, tiff_on_device=True, batch=2, tiff_write_batch=3)
    assert [c['stat_fish_many'] for c in both[3] if 'stat_fish_many' in c] == [2, 2] and all(both[0][n] == one[0][n] for n in one[0])


def test_batch_is_ignored_without_tiff_on_device(tmp_path, monkeypatch, capsys):
    inp = _five_images(tmp_path)
    monkeypatch.chdir(tmp_path)
    off = _run(tmp_path, inp, capsys, tiff_on_device=False, batch=1)
    got = _run(tmp_path, inp, capsys, tiff_on_device=False, batch=8)
    assert not [c for c in got[3] if 'stat_fish_many' in c] and got[1] == off[1] == 1 and got[2] == off[2]
    assert sorted(got[0]) == sorted(off[0]) and all(got[0][n] == off[0][n] for n in off[0])


def test_scale_auto_and_a_refused_chunk(tmp_path, monkeypatch, capsys):
    inp = _five_images(tmp_path)
    monkeypatch.chdir(tmp_path)
    one = _run(tmp_path, inp, capsys, tiff_on_device=True, batch=1, scale='auto')
    two = _run(tmp_path, inp, capsys, tiff_on_device=True, batch=2, scale='auto')
    assert one[1] == two[1] == 1 and one[2] == two[2] and sorted(one[0]) == sorted(two[0]) and all(one[0][n] == two[0][n] for n in one[0])
    good = _run(tmp_path, inp, capsys, tiff_on_device=True, batch=2)
    handle = BatchFishHandle()
    handle.fail_at = 0                                           # the first chunk: img_0, img_1 (img_2 is unreadable: in no chunk)
    bad = _run(tmp_path, inp, capsys, handle=handle, tiff_on_device=True, batch=2)
    assert bad[1] == 1 and '3 image(s) were NOT processed' in bad[2]
    for k in (0, 1):
        assert ('img_%d.tif - its chunk could not be processed' % k) in bad[2] and 'its chunk could not be processed' in bad[2]
    csv = lambda run: run[0]['stat_fish_lsq.csv'].decode().split('\n')
    assert csv(bad) == [r for r in csv(good) if not r.startswith(('img_0,', 'img_1,'))] and len(csv(bad)) < len(csv(good))
    assert not [n for n in bad[0] if n.startswith(('img_0', 'img_1'))]
    assert all(bad[0][n] == good[0][n] for n in bad[0] if n.endswith('.tif'))


@pytest.mark.parametrize('value', [0, -1, True, '8', 1.5])
def test_a_batch_that_is_no_positive_integer_is_a_configuration_error(tmp_path, monkeypatch, capsys, value):
    inp, _ = cpu.make_folder(tmp_path, kinds=(('one', 'tif'),), size=(40, 50), color_sensitivity=(70, 70))
    _set_key(tmp_path, batch=value, tiff_on_device=True)
    monkeypatch.chdir(tmp_path)
    handle = BatchFishHandle()
    with pytest.raises(SystemExit) as e:
        sf.main([], handle=handle)
    assert e.value.code == 2 and 'batch must be a positive integer' in capsys.readouterr().out
    assert not os.path.exists(inp / 'annotated') and not [d for d in os.listdir(inp) if d.startswith('tmp_')] and not handle.calls


def test_a_handle_without_the_call_is_a_configuration_error_above_1(tmp_path, monkeypatch, capsys):
    inp, _ = cpu.make_folder(tmp_path, kinds=(('one', 'tif'),), size=(40, 50), color_sensitivity=(70, 70))
    monkeypatch.chdir(tmp_path)
    _set_key(tmp_path, batch=2, tiff_on_device=True)
    with pytest.raises(SystemExit) as e:
        sf.main([], handle=te.TiffOracleHandle())
    assert e.value.code == 2 and 'stat_fish_many' in capsys.readouterr().out
    _set_key(tmp_path, batch=1)
    sf.main([], handle=te.TiffOracleHandle())


def test_the_header_the_binding_and_the_documents_name_the_feature():
    header = open(os.path.join(ROOT, 'include', 'ecseg_hip.h')).read()
    for name in ('ecseg_stat_fish_batch(', 'ecseg_stat_fish_batch_bytes(', 'ECSEG_STAT_FISH_BATCH_MAX_IMAGES'):
        assert name in header
    assert '#define ECSEG_ABI_VERSION 6' in header
    assert {'ecseg_stat_fish_batch', 'ecseg_stat_fish_batch_bytes'} <= set(_lib.EXPORTS) and hasattr(_lib.Handle, 'stat_fish_many')
    assert '# batch: 8' in open(os.path.join(ROOT, 'config.yaml')).read()
    for doc in ('README.md', 'DESIGN.md'):
        text = open(os.path.join(ROOT, doc)).read()
        assert 'stat_fish.batch' in text and 'ecseg_stat_fish_batch' in text, doc


# ---- the layout header on the host --------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def check_program(tmp_path_factory):
    if not shutil.which('g++') or not shutil.which('make'):
        pytest.skip('no host toolchain')
    exe = str(tmp_path_factory.mktemp('fsb') / 'fish_batch_check')
    out = subprocess.run(['make', '-C', ROOT, 'asan_fish_batch', 'FISH_BATCH_CHECK=' + exe], capture_output=True, text=True, timeout=900)
    if 'cannot find' in out.stderr and 'asan' in out.stderr:
        pytest.skip('libasan not installed')
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-3000:]
    assert 'fish_batch_check: ok' in out.stdout
    return exe


def test_make_asan_fish_batch_builds_and_runs_clean(check_program):
    assert os.path.exists(check_program)
    mk = open(os.path.join(ROOT, 'Makefile')).read()
    assert 'asan_fish_batch:' in mk and '-fsanitize=address,undefined' in mk.split('asan_fish_batch:')[1]
