"""PackBits input TIFFs for the device reader, without a GPU: the fixtures of tiff_packbits_cases.py are valid files (the Python reader
returns their pixels), the handle-free routing functions answer as before with the new switch off and count no PackBits file with it
on, the verdicts of image_io._packbits_decode on damaged streams are written down (it raises for none), the strip routine compiled
for the host runs clean under the sanitizers, and the configuration keys of `make metaseg` and `make stat_fish` are booleans."""
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest
import yaml

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import tiff_decode_cases as dc               # noqa: E402
import tiff_packbits_cases as pc             # noqa: E402
import tiff_tiles_cases as tc                # noqa: E402
from test_host_multirank import StubModel, make_inputs     # noqa: E402
from test_metaseg_tiffs_host import TiffsHandle, _folder, _tree      # noqa: E402
from ecseg_amd import _lib, image_io, metaseg              # noqa: E402
from ecseg_amd.utils import get_imgs         # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ('ecseg_tiff_decode_routes', 'ecseg_tiff_decode_batch_routes', 'ecseg_tiff_decode_batch_counts', 'ecseg_tiff_decode_batch_bytes')


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
    lib = _lib.load_library()
    for name in NEW:
        assert name + '(' in hdr and name in _lib.EXPORTS and hasattr(lib, name), name
    assert re.findall(r'#define (ECSEG_TIFF_\w+)\s+(\d+)u', hdr) == [('ECSEG_TIFF_DEFLATE', '1'), ('ECSEG_TIFF_TILED', '2'), ('ECSEG_TIFF_PACKBITS', '4')]
    assert not [n for n in _lib.EXPORTS if n.startswith('ecseg_tiff_decode') and '_ex' in n]
    assert 'still 5 - additive: option "tiff_packbits_on_device"' in hdr and '#define ECSEG_ABI_VERSION 6' in hdr
    for doc in ('DESIGN.md', 'README.md', 'INTEGRATION.md'):
        text = open(os.path.join(ROOT, doc)).read()
        assert 'tiff_packbits_on_device' in text and 'tiff_read_packbits' in text, doc
    text = open(os.path.join(ROOT, 'config.yaml')).read()
    cfg = yaml.safe_load(text)
    meta = text[text.index('\nmetaseg:'):text.index('\nfish_distance_calculation:')]
    for key in ('tiff_read_deflate', 'tiff_read_tiled', 'tiff_read_packbits'):
        assert '# ' + key in meta and key not in cfg['metaseg'] and key not in cfg['stat_fish'], key
    assert '# tiff_read_packbits' in text[text.index('\nstat_fish:'):text.index('\nmetaseg:')]
    assert 'asan_tiff_packbits:' in open(os.path.join(ROOT, 'Makefile')).read()
    strip = open(os.path.join(ROOT, 'ecseg_amd', 'csrc', 'tiff_packbits_strip.h')).read()
    assert 'asm' not in strip, 'plain HIP C++'


# ---- the fixtures ---------------------------------------------------------------------------------------------------------------------
def test_the_python_reader_returns_the_stored_pixels_of_every_case(tmp_path):
    cases = pc.plan_cases()
    assert len(cases) == 3 * (2 + 2 + 4) + (2 + 2 + 4)
    for name, img, data, tiled in cases:
        got = pc.python_read(data, tmp_path)
        assert got.dtype == img.dtype and np.array_equal(got, img), name
        assert image_io._native_tiff(str(tmp_path / 'case.tif')) is None, 'the native reader leaves PackBits to the Python one'
    hand = pc.hand_cases()
    assert [n for n, _, _ in hand] == ['literal_run_of_128', 'repeat_run_of_128', 'run_crosses_a_row_end', 'noop_between_runs', 'one_value_all_repeats',
                                       'noise_all_literals', 'stream_one_byte_short', 'stream_cut_in_half', 'lone_repeat_header', 'trailing_bytes',
                                       'run_passes_the_strip_end']
    for name, img, data in hand:
        got = pc.python_read(data, tmp_path)                 # (raises for none of them)
        if img is not None:
            assert np.array_equal(got, img), name


def test_the_encoder_is_read_back_by_the_python_decoder():
    rng = np.random.default_rng(7)
    for k in range(200):
        n = int(rng.integers(1, 700))
        raw = rng.integers(0, 256 if k % 3 else 3, n, dtype=np.uint8).tobytes()
        for enc in (dict(), dict(min_run=2), dict(noop_every=3), dict(min_run=200)):
            s = pc.packbits(raw, **enc)
            assert image_io._packbits_decode(s, n).tobytes() == raw, (k, enc)


# ---- the verdicts of the Python decoder, which the device holds ------------------------------------------------------------------------
def _restated(data, expected):
    """_packbits_decode as a byte loop, the way csrc/tiff_packbits_strip.h and tools/asan/tiff_packbits_fuzz.cpp state it"""
    out, i, n = [], 0, len(data)
    while i < n and len(out) < expected:
        h = data[i]
        i += 1
        if h < 128:
            out += list(data[i:min(i + h + 1, n)])
            i += h + 1
        elif h > 128:
            if i < n:
                out += [data[i]] * (257 - h)
            i += 1
    out = out[:expected]
    return bytes(out + [0] * (expected - len(out)))


def test_the_python_decoder_raises_for_no_stream_and_its_leniencies_are_these():
    """The streams for which image_io._packbits_decode raises, with the reason: there are none (RAISING_STREAMS is empty).  A seeded sweep
    over valid, truncated, overlong and random streams shows it, and the byte-loop restatement above agrees on every one of them; so
    the device gives status 0 and these bytes for each, a strip one byte short included."""
    assert pc.RAISING_STREAMS == []
    rng = np.random.default_rng(11)
    dec = image_io._packbits_decode
    for k in range(400):
        n = int(rng.integers(1, 500))
        raw = rng.integers(0, 256 if k % 2 else 4, n, dtype=np.uint8).tobytes()
        ok = pc.packbits(raw, noop_every=4 if k % 5 == 0 else 0)
        streams = [ok, ok[:-1], ok[:int(rng.integers(0, len(ok) + 1))], ok + rng.integers(0, 256, 9, dtype=np.uint8).tobytes(),
                   rng.integers(0, 256, int(rng.integers(0, 300)), dtype=np.uint8).tobytes(), b'', b'\x81', b'\x80', b'\x05\x01']
        for s in streams:
            for expected in (n, max(1, n - 3), n + 5):
                assert dec(s, expected).tobytes() == _restated(s, expected), (k, len(s), expected)
    # by hand, what "lenient" means
    assert dec(b'\x02\x01\x02', 3).tolist() == [1, 2, 0], 'a literal run the stream ends in: what there is, zeros behind'
    assert dec(b'\x00\x07\xfe', 4).tolist() == [7, 0, 0, 0], 'a repeat header that is the last byte: nothing'
    assert dec(b'\xfd\x09', 2).tolist() == [9, 9], 'a run that would pass expected is cut there'
    assert dec(b'\x00\x07\x55\x66\x77', 1).tolist() == [7], 'bytes left over are not looked at'
    assert dec(b'\x80\x00\x07\x80', 1).tolist() == [7], 'header 128 is a no-op'


# ---- the handle-free functions ----------------------------------------------------------------------------------------------------------
def _other_files():
    """LZW and Deflate strips at counts on both sides of their thresholds, uncompressed strips, tiled files: name -> bytes"""
    import zlib
    img = tc.pixels('rgb8', 1100, 16)
    rows = img.reshape(1100, -1)
    out = {'lzw_1100_strips': dc.file_of(img, 1), 'lzw_5_rows': dc.file_of(img[:60], 5), 'raw': dc.file_of(img[:60], 5, compression=1),
           'deflate_1100_strips': dc.tiff_file([zlib.compress(rows[r].tobytes()) for r in range(1100)], 1100, 16, 1, spp=3, compression=8),
           'deflate_150_strips': dc.tiff_file([zlib.compress(rows[r].tobytes()) for r in range(150)], 150, 16, 1, spp=3, compression=8)}
    for name, (im, data) in tc.fixture_cases().items():
        out['tiled_' + name] = data
    return out


def test_the_rule_functions_answer_as_before_with_the_switch_off_and_count_no_packbits_file_with_it_on():
    lib = _lib.load_library()
    empty = 6 * 256                                          # the arena of a call that takes no file: six empty slots
    packbits_files = [(n, d) for n, _, d, _ in pc.plan_cases()] + [(n, d) for n, _, d in pc.hand_cases()]
    # what an accepted file needs of the arena: table row, file image, strip tables, raster, strip words, file word - and for tiles the
    # tiled-file row and the staging slots - each rounded up to 256 bytes (an LZW file of the same tags needs the same)
    slot = lambda v: (v + 255) // 256 * 256 if v else 256
    need, parsed = {}, 0
    for name, data in packbits_files:
        H, W, spp, bits = image_io.tiff_shape(data)
        px = spp * bits // 8
        if '_t16x16_' in name:
            tiles = -(-H // 16) * -(-W // 16)
            need[name] = slot(80) + slot(len(data)) + slot(8 * tiles) + slot(H * W * px) + slot(4 * tiles) + slot(4) + slot(32) + slot(tiles * 256 * px)
        else:
            rps = int(name.split('_rps')[1].split('_')[0]) if '_rps' in name else {1: 1, 2: 2, 7: 3, 9: 4, 6: 2}[H]
            strips = -(-H // rps)
            need[name] = slot(80) + slot(len(data)) + slot(8 * strips) + slot(H * W * px) + slot(4 * strips) + slot(4)
    for name, data in packbits_files:
        tiled_file = '_t16x16_' in name
        for deflate in (0, 1):
            for tiled in (0, 1):
                assert _answers(lib, data, deflate, tiled, 0) == (0, 0, 0, empty), (name, deflate, tiled)
                on = _answers(lib, data, deflate, tiled, 1)
                assert on[:3] == (0, 0, 0), 'a PackBits file counts in no rule: %s' % name
                taken = tiled == 1 or not tiled_file
                assert on[3] == (need[name] if taken else empty), 'and parses with the switch: %s' % name
                parsed += taken and on[3] > empty
        one = np.frombuffer(data, np.uint8)
        assert not image_io.tiff_goes_to_device(data) and not image_io.tiff_goes_to_device(data, deflate=True, tiled=True, packbits=True), name
        assert not image_io.tiff_batch_counts(one) and not image_io.tiff_batch_counts(one, True, True, True), name
    assert parsed >= 4 * len(pc.plan_cases()) - 16
    assert image_io.tiff_batch_goes_to_device([d for _, d in packbits_files[:4]], deflate=True, tiled=True, packbits=True) == (False, [False] * 4)
    seen = set()
    for name, data in _other_files().items():                # every other kind of file: the switch changes nothing
        for deflate in (0, 1):
            for tiled in (0, 1):
                old = _answers(lib, data, deflate, tiled, 0)
                assert old == _answers(lib, data, deflate, tiled, 1), (name, deflate, tiled)
                seen.add((name.split('_')[0], old[:3]))
    assert ('lzw', (1, 1, 1)) in seen and ('deflate', (1, 1, 1)) in seen and ('deflate', (0, 1, 1)) in seen and ('deflate', (0, 0, 0)) in seen
    datas = [_other_files()['lzw_1100_strips'], packbits_files[0][1]]
    assert image_io.tiff_batch_goes_to_device(datas, packbits=True) == (True, [True, False]) == image_io.tiff_batch_goes_to_device(datas)


# ---- the sanitizer program ------------------------------------------------------------------------------------------------------------
def test_the_strip_routine_runs_clean_under_the_sanitizers(tmp_path):
    """`make asan_tiff_packbits`: the same sources and flags, built in the test's own folder."""
    cxx = shutil.which('g++') or shutil.which('clang++')
    if not cxx:
        pytest.skip('no host C++ compiler')
    san = ['-fsanitize=address,undefined', '-fno-sanitize-recover=all']
    probe = tmp_path / 'probe.cpp'
    probe.write_text('int main() { return 0; }\n')
    if subprocess.run([cxx] + san + [str(probe), '-o', str(tmp_path / 'probe')], capture_output=True, timeout=120).returncode != 0:
        pytest.skip('the host compiler cannot link the sanitizer runtimes')
    exe = str(tmp_path / 'tiff_packbits_fuzz')
    cmd = [cxx, '-std=c++17', '-O1', '-g', '-fno-omit-frame-pointer', '-Wall', '-Werror'] + san + [
        os.path.join(ROOT, 'tools', 'asan', 'tiff_packbits_fuzz.cpp'), '-o', exe]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-3000:]
    run = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert run.returncode == 0, (run.stdout + run.stderr)[-3000:]
    assert 'tiff_packbits_fuzz ok' in run.stdout, run.stdout
    for cls in ('valid', 'truncated', 'truncated by one byte', "overlong: a run passes the strip's end", 'overlong: bytes left over', 'random bytes'):
        assert any(line.split(None, 1)[1:] == [cls] and int(line.split()[0]) > 0 for line in run.stdout.splitlines() if line.strip()), cls


# ---- make metaseg: the keys -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('key', ['tiff_read_deflate', 'tiff_read_tiled', 'tiff_read_packbits'])
def test_a_key_that_is_no_boolean_is_a_configuration_error_of_make_metaseg(tmp_path, monkeypatch, capsys, key):
    inp = tmp_path / 'images'
    make_inputs(str(inp), 1)
    monkeypatch.chdir(tmp_path)
    for value in ('yes', 1, [True]):
        for read in (True, False):                           # (also without tiff_read_on_device: the type is checked, the value ignored)
            yaml.safe_dump({'metaseg': {'inpath': str(inp), 'tiff_read_on_device': read, key: value}}, open(tmp_path / 'config.yaml', 'w'))
            with pytest.raises(SystemExit) as e:
                metaseg.main([])
            assert e.value.code == 2 and key + ' must be true or false' in capsys.readouterr().out


class OptionTiffsHandle(TiffsHandle):
    """The injected handle of test_metaseg_tiffs_host.py with options, which it records."""

    def __init__(self, tmp, **kw):
        super().__init__(tmp, **kw)
        self.options = []

    def set_option(self, key, value):
        self.options.append((key, value))
        setattr(self, key, bool(value))


def test_the_keys_set_the_handle_options_only_with_tiff_read_on_device_and_keep_every_byte(tmp_path):
    quiet = lambda *a: None
    trees, seen = {}, {}
    for name, keys in (('absent', {}), ('alone', dict(tiff_read_deflate=True, tiff_read_tiled=True, tiff_read_packbits=True)),
                       ('read', dict(tiff_read_on_device=True)),
                       ('all', dict(tiff_read_on_device=True, tiff_read_deflate=True, tiff_read_tiled=True, tiff_read_packbits=True))):
        folder = str(tmp_path / name)
        _folder(folder)
        model = StubModel()
        model.handle = OptionTiffsHandle(tmp_path)
        rec = metaseg.run(folder, model, get_imgs(folder), 0, 1, batch_images=12, io_threads=2, log=quiet, **keys)
        trees[name], seen[name] = (_tree(folder), rec.tolist()), model.handle
    assert not seen['absent'].options and not seen['alone'].options and not seen['alone'].tiffs, 'ignored without tiff_read_on_device'
    assert not seen['read'].options and seen['read'].tiffs == [12]
    on = [(k, 1) for k in ('tiff_deflate_on_device', 'tiff_tiled_on_device', 'tiff_packbits_on_device')]
    assert seen['all'].options == on + [(k, 0) for k, _ in on], 'set for the run, and the handle handed back as it came'
    assert seen['all'].tiffs == [12], 'one Deflate file of 96 strips is below the measured 280: it stays with the host reader'
    for name in ('alone', 'read', 'all'):
        assert trees[name] == trees['absent'], name
    with pytest.raises(ValueError, match='set_option'):    # a handle without options cannot take the keys
        metaseg.run(str(tmp_path / 'all'), model_with(TiffsHandle(tmp_path)), get_imgs(str(tmp_path / 'all')), 0, 1, batch_images=12, io_threads=2, log=quiet,
                    tiff_read_on_device=True, tiff_read_packbits=True)


def model_with(handle):
    m = StubModel()
    m.handle = handle
    return m
