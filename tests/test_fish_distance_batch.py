"""``fish_distance_calculation.batch`` without a GPU: the configuration rules of the key, ``main`` at ``batch`` 1 and above on an
injected handle whose ``fish_distances_many`` answers from tests/fish_distance_ref.py, the names the header and the binding declare,
and the layout header of ecseg_fish_distances_batch (csrc/fishdist_batch.h) compiled for the host under ASan + UBSan
(tools/asan/fishdist_batch_check.cpp, ``make asan_fishdist_batch``)."""
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest
import yaml

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fish_distance_ref as ref              # noqa: E402
import test_fish_distance as cpu             # noqa: E402
import test_gpu_fish_distance_batch as folder   # noqa: E402
from ecseg_amd import _lib                   # noqa: E402
from ecseg_amd import fish_distance_calculation as fdc   # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class BatchStubHandle(cpu.StubHandle):
    """``fish_distances_many`` per image from the vectorised oracle; remembers the size of every chunk."""
    refuse_chunks = False

    def fish_distances_many(self, labels, lsqs, fish_channel, centromere_channel, record_capacity=4096):
        assert len(labels) == len(lsqs) and len(labels) > 0
        self.calls.append(dict(many=len(labels)))
        if self.refuse_chunks and len(labels) > 1:
            e = _lib.EcsegError('ecseg_fish_distances_batch failed (-1): refused as a whole')
            e.code = -1
            raise e
        out = []
        for lab, lsq in zip(labels, lsqs):
            assert lab.dtype == np.int32 and lab.flags.c_contiguous and lsq.dtype == np.uint8 and lsq.flags.c_contiguous
            assert int(lab.max()) <= lab.size, 'labels above H * W must be remapped on the host'
            out.append(ref.records(lsq, lab, fish_channel, centromere_channel))
        return out


def _many(handle):
    return [c['many'] for c in handle.calls if isinstance(c, dict)]


def _exit_of(tmp_path, handle, **keys):
    """the exit code and the printed text of a ``main`` that is expected to stop"""
    var = {'inpath': str(tmp_path / 'in'), 'centromere_probe_color': 'blue', 'fish_probe_color': 'red', 'max_centromeric_spots': 3}
    var.update(keys)
    yaml.safe_dump({'fish_distance_calculation': var}, open(tmp_path / 'config.yaml', 'w'))
    with pytest.raises(SystemExit) as e:
        fdc.main([], handle=handle)
    return e.value.code


# ---- the key -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('value', [0, -1, -8, True, False, '8', 1.5, 8.0, [4]])
def test_a_batch_that_is_no_positive_integer_is_a_configuration_error(tmp_path, monkeypatch, capsys, value):
    inp, _ = folder.make_folder(tmp_path)
    monkeypatch.chdir(tmp_path)
    handle = BatchStubHandle()
    assert _exit_of(tmp_path, handle, batch=value) == 2
    assert 'batch must be a positive integer' in capsys.readouterr().out
    assert not handle.calls and not os.path.exists(inp / 'centromere_distances.csv')


def test_a_handle_without_the_call_is_a_configuration_error_above_1(tmp_path, monkeypatch, capsys):
    inp, _ = folder.make_folder(tmp_path)
    monkeypatch.chdir(tmp_path)
    handle = cpu.StubHandle()
    assert _exit_of(tmp_path, handle, batch=4) == 2
    assert 'fish_distances_many' in capsys.readouterr().out and not handle.calls
    assert not os.path.exists(inp / 'centromere_distances.csv')
    csv, out, code = folder.run_main(tmp_path, capsys, handle=handle, batch=1)          # the same handle serves batch: 1
    assert code == 1 and csv.count('\n') > 30 and len(handle.calls) == 5


# ---- main() ------------------------------------------------------------------------------------------------------------------------
def test_batch_4_equals_batch_1_on_the_same_fake(tmp_path, monkeypatch, capsys):
    inp, good = folder.make_folder(tmp_path)
    monkeypatch.chdir(tmp_path)
    h1 = BatchStubHandle()
    one = folder.run_main(tmp_path, capsys, handle=h1, batch=1)
    assert not _many(h1) and len(h1.calls) == 5, 'batch: 1 is the path of one call per image'
    others, sizes = {}, {}
    for k in (4, 2, 6, 7):
        h = BatchStubHandle()
        others[k] = folder.run_main(tmp_path, capsys, handle=h, batch=k, io_threads=2 if k == 2 else None)
        sizes[k] = _many(h)
        assert len(h.calls) == len(sizes[k]), 'nothing runs one image at a time'
    assert sizes == {4: [3, 2], 2: [2, 1, 2], 6: [5], 7: [5]}, 'img_2 has no label map: it is in no chunk'
    folder.check_runs(inp, good, one, others)
    no_key = folder.run_main(tmp_path, capsys, handle=BatchStubHandle())
    assert no_key == one, 'the default is batch: 1'


def test_a_chunk_refused_as_a_whole_is_taken_apart(tmp_path, monkeypatch, capsys):
    inp, good = folder.make_folder(tmp_path)
    monkeypatch.chdir(tmp_path)
    one = folder.run_main(tmp_path, capsys, handle=BatchStubHandle(), batch=1)
    h = BatchStubHandle()
    h.refuse_chunks = True
    got = folder.run_main(tmp_path, capsys, handle=h, batch=4)
    assert got == one and _many(h) == [3, 1, 1, 1, 2, 1, 1]


def test_a_folder_without_images_and_one_of_a_single_image(tmp_path, monkeypatch, capsys):
    (tmp_path / 'in' / 'annotated').mkdir(parents=True)
    monkeypatch.chdir(tmp_path)
    csv, out, code = folder.run_main(tmp_path, capsys, handle=BatchStubHandle(), batch=4)
    assert csv == 'normalized_distance\n' and code == 0 and out == ''


# ---- the surface -------------------------------------------------------------------------------------------------------------------
def test_the_header_the_binding_and_the_documents_name_the_feature():
    header = open(os.path.join(ROOT, 'include', 'ecseg_hip.h')).read()
    assert re.search(r'\becseg_fish_distances_batch\s*\(', header) and 'ECSEG_FISH_DISTANCES_BATCH_MAX_IMAGES' in header
    assert 'still 5 - additive: ecseg_fish_distances_batch' in header and '#define ECSEG_ABI_VERSION 6' in header
    assert 'ecseg_fish_distances_batch' in _lib.EXPORTS and hasattr(_lib.Handle, 'fish_distances_many')
    assert _lib.Handle.FISH_DISTANCES_BATCH_MAX_IMAGES == int(re.search(r'#define ECSEG_FISH_DISTANCES_BATCH_MAX_IMAGES (\d+)', header).group(1))
    binding = open(os.path.join(ROOT, 'ecseg_amd', '_lib.py')).read()
    assert 'lib.ecseg_fish_distances_batch.argtypes' in binding
    n_args = len(re.search(r'lib\.ecseg_fish_distances_batch\.argtypes = \[(.*?)\]\n', binding).group(1).split(', '))
    declared = re.search(r'int ecseg_fish_distances_batch\((.*?)\);', header, re.S).group(1)
    assert n_args == len(re.sub(r'/\*.*?\*/', '', declared).split(',')) == 11
    config = open(os.path.join(ROOT, 'config.yaml')).read().split('fish_distance_calculation:')[1]
    assert '# batch: 1' in config and '# io_threads:' in config
    for doc in ('README.md', 'DESIGN.md'):
        text = open(os.path.join(ROOT, doc)).read()
        assert 'fish_distance_calculation.batch' in text and 'ecseg_fish_distances_batch' in text, doc
    if os.path.exists(_lib.LIB_PATH):
        blob = open(_lib.LIB_PATH, 'rb').read()
        for name in (b'ecseg_fish_distances_batch', b'fdb_mark_kernel', b'fdb_void_refused_kernel', b'fdb_plan_kernel', b'fdb_cell_stats_kernel',
                     b'fdb_fill_unite_kernel', b'fdb_distance_kernel'):
            assert name in blob, name


# ---- the layout header on the host ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def check_program(tmp_path_factory):
    if not shutil.which('g++') or not shutil.which('make'):
        pytest.skip('no host toolchain')
    exe = str(tmp_path_factory.mktemp('fdb') / 'fishdist_batch_check')
    out = subprocess.run(['make', '-C', ROOT, 'asan_fishdist_batch', 'FISHDIST_BATCH_CHECK=' + exe], capture_output=True, text=True, timeout=900)
    if 'cannot find' in out.stderr and 'asan' in out.stderr:
        pytest.skip('libasan not installed')
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-3000:]
    assert 'fishdist_batch_check: ok' in out.stdout
    return exe


def test_make_asan_fishdist_batch_builds_and_runs_clean(check_program):
    assert os.path.exists(check_program)
    mk = open(os.path.join(ROOT, 'Makefile')).read()
    assert 'asan_fishdist_batch:' in mk and '-fsanitize=address,undefined' in mk.split('asan_fishdist_batch:')[1]
