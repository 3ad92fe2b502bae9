"""Tiled TIFF files for the device reader, the parts that need no GPU: the tile writer of tests/tiff_tiles_cases.py against its stored,
tifffile-checked files; the pure-Python reader (the oracle of the tiled path) on every case; the parser's verdicts through the
handle-free rule functions, switch off (today's answers) and on; the config key of `make stat_fish`; and the stand-alone sanitizer
program that walks tile_place, the tile-table parse and the staging -> raster copy on the host (tools/asan/tiff_tiles_check.cpp)."""
import base64
import json
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest
import yaml

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_stat_fish_aqua as cpu            # noqa: E402
import tiff_tiles_cases as tc                # noqa: E402
from ecseg_amd import _lib, image_io         # noqa: E402
from ecseg_amd import stat_fish as sf        # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden')


def _ptr(a):
    import ctypes as C
    return a.ctypes.data_as(C.c_void_p)


def _answers(lib, data, deflate, tiled, packbits=0):
    """(routes, counts, set routes, arena bytes of the file alone) of the handle-free functions with the word of the switches."""
    one = np.frombuffer(data, np.uint8)
    buf, ranges = _lib.pack_file_images([one, one])
    r1 = np.array([[0, one.size]], np.int64)
    kinds = _lib.tiff_kinds(deflate, tiled, packbits)
    return (lib.ecseg_tiff_decode_routes(_ptr(one), one.size, kinds), lib.ecseg_tiff_decode_batch_counts(_ptr(one), one.size, kinds),
            lib.ecseg_tiff_decode_batch_routes(_ptr(buf), buf.size, _ptr(ranges), 2, kinds),
            lib.ecseg_tiff_decode_batch_bytes(_ptr(one), one.size, _ptr(r1), 1, kinds))


def test_header_binding_and_documents_name_the_option_and_the_new_symbols():
    hdr = open(os.path.join(ROOT, 'include', 'ecseg_hip.h')).read()
    for name in ('ecseg_tiff_decode_routes', 'ecseg_tiff_decode_batch_routes', 'ecseg_tiff_decode_batch_counts', 'ecseg_tiff_decode_batch_bytes'):
        assert name + '(' in hdr and name in _lib.EXPORTS, name
    assert re.findall(r'#define (ECSEG_TIFF_\w+)\s+(\d+)u', hdr) == [('ECSEG_TIFF_DEFLATE', '1'), ('ECSEG_TIFF_TILED', '2'), ('ECSEG_TIFF_PACKBITS', '4')]
    assert not [n for n in _lib.EXPORTS if n.startswith('ecseg_tiff_decode') and '_ex' in n]
    assert 'still 5 - additive: option "tiff_tiled_on_device"' in hdr and '#define ECSEG_ABI_VERSION 6' in hdr
    for doc in ('README.md', 'DESIGN.md', 'config.yaml'):
        text = open(os.path.join(ROOT, doc)).read()
        assert 'tiff_read_tiled' in text, doc
    for doc in ('README.md', 'DESIGN.md'):
        assert 'tiff_tiled_on_device' in open(os.path.join(ROOT, doc)).read(), doc


def test_the_writer_reproduces_the_files_that_were_checked_against_tifffile():
    stored = sorted(f[:-4] for f in os.listdir(tc.GOLDEN) if f.endswith('.tif'))
    cases = tc.fixture_cases()
    assert stored == sorted(cases) and len(stored) == 5
    for name, (img, data) in cases.items():
        assert open(os.path.join(tc.GOLDEN, name + '.tif'), 'rb').read() == data, name
        assert np.array_equal(np.load(os.path.join(tc.GOLDEN, name + '.npy')), img), name


def test_the_python_reader_returns_the_stored_pixels_of_every_case(tmp_path):
    cases = tc.all_cases()
    assert len(cases) == 2 * len(tc.EXTENTS) * len(tc.KINDS) * len(tc.COMPRESSIONS)
    seen = set()
    for name, img, data in cases:
        verdict, got = tc.python_verdict(data, tmp_path)
        assert verdict == 'ok' and got.dtype == img.dtype and np.array_equal(got, tc.squeeze(img)), name
        seen.add(tuple(name.split('_')[-2:]))
    assert seen == {('p1', 'le'), ('p1', 'be'), ('p2', 'le'), ('p2', 'be')}
    for name in os.listdir(tc.GOLDEN):
        if name.endswith('.tif'):
            got = image_io.read_tiff(os.path.join(tc.GOLDEN, name))
            assert np.array_equal(got, tc.squeeze(np.load(os.path.join(tc.GOLDEN, name[:-4] + '.npy')))), name


def test_the_python_reader_on_the_damaged_files_is_the_verdict_the_device_tests_hold(tmp_path):
    """What the oracle does, written down once: a corrupt LZW tile raises TiffError, a corrupt, short or empty zlib tile zlib.error; a
    tile whose offset lies behind the file or whose count leaves it is sliced to what the file has - zeros for an LZW or uncompressed
    tile - and the file is read."""
    want = dict(corrupt_lzw_tile='error', corrupt_zlib_tile='error', short_zlib_tile='error', zlib_offset_behind_file='error',
                lzw_offset_behind_file='ok', raw_offset_behind_file='ok', lzw_count_leaves_file='ok')
    cases = tc.damaged_cases()
    assert set(cases) == set(want)
    for name, (img, data, hit) in cases.items():
        verdict, got = tc.python_verdict(data, tmp_path)
        assert verdict == want[name], (name, got)
        if verdict == 'ok':
            ref = img.copy()
            if 'behind' in name:
                ref[16 * (hit // 5):16 * (hit // 5) + 16, 16 * (hit % 5):16 * (hit % 5) + 16] = 0
            assert np.array_equal(got, ref), name
    verdict, e = tc.python_verdict(tc.refused_cases()['short_tile_table'], tmp_path)
    assert verdict == 'error' and isinstance(e, IndexError)


def test_the_parser_takes_tiled_files_only_with_the_switch_and_leaves_the_rest_to_the_python_reader():
    """Through ecseg_tiff_decode_batch_bytes, which is -1 only for bad arguments and else what the accepted files need: a file the
    parser refuses needs the empty arena, an accepted one its staging slots on top."""
    lib = _lib.load_library()
    empty = None
    slot = lambda v: (v + 255) // 256 * 256 if v else 256
    for name, img, data in tc.all_cases():
        off = _answers(lib, data, 0, 0)
        one = np.frombuffer(data, np.uint8)
        r1 = np.array([[0, one.size]], np.int64)
        assert off[3] == lib.ecseg_tiff_decode_batch_bytes(_ptr(one), one.size, _ptr(r1), 1, 0) == _answers(lib, data, 1, 0)[3], name
        assert off[:3] == (0, 0, 0) and lib.ecseg_tiff_decode_routes(_ptr(one), one.size, 0) == 0, name
        empty = off[3] if empty is None else empty
        assert off[3] == empty == 6 * 256, 'a tiled file is left out without the switch: six empty slots'
        ext = [int(v) for v in name.split('_')[1].split('x') + name.split('_')[2][1:].split('x')]
        H, W, th, tw = ext
        tiles = -(-H // th) * -(-W // tw)
        px = img.shape[2] * img.dtype.itemsize
        deflate_file = '_deflate_' in name
        on = _answers(lib, data, 1, 1)
        stage = 0 if '_raw_' in name else tiles * th * tw * px
        need = slot(80) + slot(one.size) + slot(8 * tiles) + slot(H * W * px) + slot(4 * tiles) + slot(4) + slot(32) + slot(stage)
        assert on[3] == need, (name, on[3], need)
        assert _answers(lib, data, 0, 1)[3] == (empty if deflate_file else need), name
    for name, data in tc.refused_cases().items():
        for deflate, tiled in ((0, 0), (0, 1), (1, 1)):
            assert _answers(lib, data, deflate, tiled) == (0, 0, 0, 6 * 256), (name, deflate, tiled)
    for name, (img, data, hit) in tc.damaged_cases().items():         # structurally fine: taken, the verdict is the decode's
        assert _answers(lib, data, 1, 1)[3] > 6 * 256, name


def test_the_rule_functions_answer_as_before_with_the_switch_off_and_by_the_measured_table_with_it_on():
    """csrc/tiff_parse.h: a tiled file counts only from a measured tile count on; while the table of DESIGN.md 5.9 is NOT MEASURED the
    thresholds are "never" and the rules answer 0 for every tiled file and set, whatever the switch - and files of strips are not
    touched by the switch at all."""
    lib = _lib.load_library()
    text = open(os.path.join(ROOT, 'ecseg_amd', 'csrc', 'tiff_parse.h')).read()

    def threshold(name):
        value = text.split('constexpr size_t %s = ' % name)[1].split(';')[0]
        return None if value == 'TIFF_TILED_NEVER' else int(value)
    single, batch = threshold('TIFF_TILED_DEVICE_MIN_TILES'), threshold('TIFF_TILED_BATCH_DEVICE_MIN_TILES')
    files = json.load(open(os.path.join(GOLDEN, 'io_tiff_files.json')))['files']
    for name, b64 in files.items():                                    # strips, and the two tifffile-written tiled files
        data = base64.b64decode(b64)
        one = np.frombuffer(data, np.uint8)
        for deflate in (0, 1):
            old = _answers(lib, data, deflate, 0)
            if 'tiled' not in name:                                    # a file of strips: TILED in the word changes none of the four answers,
                assert _answers(lib, data, deflate, 1) == old, (name, deflate)
                part = slice(3) if 'packbits' in name else slice(4)   # nor does PACKBITS, but for the arena of a PackBits file: it then parses
                assert _answers(lib, data, deflate, 0, 1)[part] == old[part] == _answers(lib, data, deflate, 1, 1)[part], (name, deflate)
    big = tc.pixels('rgb8', 160, 1392)                                 # 870 tiles of 16 x 16
    for comp in (1, 5, 8):
        data = tc.tiled_tiff(big, 16, 16, comp, 2)
        n = 10 * 87
        want = (int(comp != 1 and single is not None and n >= single), int(comp != 1 and batch is not None),
                int(comp != 1 and batch is not None and 2 * n >= batch))
        assert _answers(lib, data, 1, 1)[:3] == want, comp
        assert image_io.tiff_goes_to_device(data, deflate=True, tiled=True) == bool(want[0])
        assert image_io.tiff_batch_goes_to_device([data, data], deflate=True, tiled=True) == (bool(want[2]), [bool(want[1])] * 2)
        assert _answers(lib, data, 1, 0)[:3] == (0, 0, 0)
    if single is None and batch is None:
        assert 'NOT MEASURED' in open(os.path.join(ROOT, 'DESIGN.md')).read().split('tiff_tiled_on_device')[1]


# ---- the sanitizer program ---------------------------------------------------------------------------------------------------------
def test_tile_place_the_table_parse_and_the_untile_walk_under_the_sanitizers(tmp_path):
    cxx = shutil.which('g++') or shutil.which('clang++')
    if not cxx:
        pytest.skip('no host C++ compiler')
    san = ['-fsanitize=address,undefined', '-fno-sanitize-recover=all']
    probe = tmp_path / 'probe.cpp'
    probe.write_text('int main() { return 0; }\n')
    if subprocess.run([cxx] + san + [str(probe), '-o', str(tmp_path / 'probe')], capture_output=True, timeout=120).returncode != 0:
        pytest.skip('the host compiler cannot link the sanitizer runtimes')
    exe = str(tmp_path / 'tiff_tiles_check')
    csrc = os.path.join(ROOT, 'ecseg_amd', 'csrc')
    cmd = [cxx, '-std=c++17', '-O1', '-g', '-fno-omit-frame-pointer', '-Wall', '-Werror'] + san + [
        os.path.join(csrc, 'host_codec.cpp'), os.path.join(csrc, 'host_io.cpp'), os.path.join(ROOT, 'tools', 'asan', 'tiff_tiles_check.cpp'), '-lz', '-o', exe]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-3000:]
    run = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert run.returncode == 0, (run.stdout + run.stderr)[-3000:]
    assert 'tiff_tiles_check ok' in run.stdout and ' 0 files,' not in run.stdout and ' 0 files refused' not in run.stdout, run.stdout
    assert 'asan_tiff_tiles' in open(os.path.join(ROOT, 'Makefile')).read()


# ---- make stat_fish: the key ---------------------------------------------------------------------------------------------------------
class OptionHandle(cpu.RenderingOracleHandle):
    """A handle with options, whose ``tiff_decode`` is answered by the Python reader; both are recorded."""

    def set_option(self, key, value):
        self.calls.append(dict(set_option=key, value=value))
        setattr(self, key, bool(value))

    def tiff_decode(self, data, deflate=None):
        self.calls.append(dict(tiff_decode=len(data), tiled=getattr(self, 'tiff_tiled_on_device', False)))
        path = os.path.join(self.tmp, 'decode_%d.tif' % len(self.calls))
        with open(path, 'wb') as f:
            f.write(data)
        return image_io.read_tiff(path)


def _set_key(tmp_path, **keys):
    cfg = yaml.safe_load(open(tmp_path / 'config.yaml'))
    cfg['stat_fish'].update(keys)
    yaml.safe_dump(cfg, open(tmp_path / 'config.yaml', 'w'))


@pytest.mark.parametrize('value', [3, 'yes', 0, [True], None])
def test_a_tiff_read_tiled_that_is_no_boolean_is_a_configuration_error(tmp_path, monkeypatch, capsys, value):
    inp, _ = cpu.make_folder(tmp_path, kinds=(('one', 'tif'),), size=(40, 50), color_sensitivity=(70, 70))
    _set_key(tmp_path, tiff_read_tiled=value)
    monkeypatch.chdir(tmp_path)
    handle = OptionHandle()
    with pytest.raises(SystemExit) as e:
        sf.main([], handle=handle)
    assert e.value.code == 2 and 'tiff_read_tiled must be true or false' in capsys.readouterr().out
    assert not os.path.exists(inp / 'annotated') and not handle.calls


def test_the_key_sets_the_handle_option_only_with_tiff_read_on_device_and_keeps_every_byte(tmp_path, monkeypatch, capsys):
    inp, _ = cpu.make_folder(tmp_path, size=(40, 50))
    monkeypatch.chdir(tmp_path)
    asked = []
    monkeypatch.setattr(image_io, 'tiff_goes_to_device', lambda data, deflate=False, tiled=False: asked.append(tiled) or True)
    runs = {}
    for name, keys in (('absent', {}), ('alone', dict(tiff_read_tiled=True)), ('read', dict(tiff_read_on_device=True, tiff_read_tiled=False)),
                       ('both', dict(tiff_read_on_device=True, tiff_read_tiled=True))):
        _set_key(tmp_path, **keys)
        handle = OptionHandle()
        handle.tmp = str(tmp_path)
        del asked[:]
        sf.main([], handle=handle)
        runs[name] = (cpu.folder_bytes(inp / 'annotated'), list(handle.calls), capsys.readouterr().out, list(asked))
    options = lambda calls: [(c['set_option'], c['value']) for c in calls if 'set_option' in c]
    decodes = lambda calls: [c['tiled'] for c in calls if 'tiff_decode' in c]
    assert not options(runs['absent'][1]) and not options(runs['alone'][1]) and not decodes(runs['alone'][1]), 'ignored without tiff_read_on_device'
    assert not options(runs['read'][1]) and decodes(runs['read'][1]) == [False] * 4 and runs['read'][3] == [False] * 4
    assert options(runs['both'][1]) == [('tiff_tiled_on_device', 1), ('tiff_tiled_on_device', 0)], 'set for the run, and the handle handed back as it came'
    assert decodes(runs['both'][1]) == [True] * 4 and runs['both'][3] == [True] * 4, 'every read asks the rule with tiled files counting'
    for name in ('alone', 'read', 'both'):
        assert runs[name][2] == runs['absent'][2], 'the messages differ'
        assert runs[name][0] == runs['absent'][0], name
