"""Deflate strips on the device, without a GPU: the new symbols and the option's documents, the ``tiff_read_deflate`` key of
``make stat_fish`` on injected handles, the flagged routing functions beside the old ones, the host reader's verdict for every
class of tests/tiff_inflate_cases.py, and the per-strip routine of tiffb_inflate_kernel (ti_inflate_strip) compiled for the host
under ASan + UBSan against the host rule on that corpus."""
import os
import re
import shutil
import struct
import subprocess
import sys
import zlib

import numpy as np
import pytest
import yaml

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_stat_fish_aqua as cpu            # noqa: E402
import tiff_decode_cases as dc               # noqa: E402
import tiff_inflate_cases as ic              # noqa: E402
from ecseg_amd import _lib, image_io         # noqa: E402
from ecseg_amd import stat_fish as sf        # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ('ecseg_tiff_decode_routes', 'ecseg_tiff_decode_batch_routes', 'ecseg_tiff_decode_batch_counts', 'ecseg_tiff_decode_batch_bytes')
DEFINES = [('ECSEG_TIFF_DEFLATE', '1'), ('ECSEG_TIFF_TILED', '2'), ('ECSEG_TIFF_PACKBITS', '4')]      # re.findall(r'#define (ECSEG_TIFF_\w+)\s+(\d+)u', header)


def test_header_binding_and_documents_name_the_option_and_the_new_symbols():
    hdr = open(os.path.join(ROOT, 'include', 'ecseg_hip.h')).read()
    lib = _lib.load_library()
    for name in NEW:
        assert name + '(' in hdr and name in _lib.EXPORTS and hasattr(lib, name), name
    assert re.findall(r'#define (ECSEG_TIFF_\w+)\s+(\d+)u', hdr) == DEFINES and not [n for n in _lib.EXPORTS if n.startswith('ecseg_tiff_decode') and '_ex' in n]
    assert 'still 5 - additive: option "tiff_deflate_on_device"' in hdr and '#define ECSEG_ABI_VERSION 6' in hdr
    for doc in ('DESIGN.md', 'README.md', 'INTEGRATION.md'):
        text = open(os.path.join(ROOT, doc)).read()
        assert 'tiff_deflate_on_device' in text and 'tiff_read_deflate' in text, doc
    gaps = open(os.path.join(ROOT, 'DESIGN.md')).read().split('## 9. Known gaps')[1].split('## 10.')[0]
    assert 'tiff_deflate_on_device' in gaps and 'ecseg_meta_segment_tiffs' in gaps, 'what is out of scope is said where the gaps are'
    assert '# tiff_read_deflate' in open(os.path.join(ROOT, 'config.yaml')).read()
    assert 'tiff_read_deflate' not in yaml.safe_load(open(os.path.join(ROOT, 'config.yaml')))['stat_fish']
    assert 'asan_tiff_inflate:' in open(os.path.join(ROOT, 'Makefile')).read()
    strip = open(os.path.join(ROOT, 'ecseg_amd', 'csrc', 'tiff_inflate_strip.h')).read()
    assert 'asm' not in strip, 'plain HIP C++'


# ---- the corpus ---------------------------------------------------------------------------------------------------------------------
def test_the_bit_writer_is_read_back_by_zlib():
    """The hand-built OK streams decode, with Python's zlib, to the bytes the cases state."""
    n = 0
    for name, stream, want, cls, out in ic.hand_cases() + ic.zlib_streams():
        if cls in (ic.OK_EXACT, ic.OK_SHORT):
            assert zlib.decompress(stream) == out, name
            n += 1
        elif cls == ic.OK_FULL:
            assert zlib.decompressobj().decompress(stream, want) == out, name
            n += 1
    assert n >= 30
    names = [c[0] for c in ic.hand_cases()]
    for needed in ('stored_block_of_length_0', 'fixed_match_258_at_distance_1', 'distance_32768_in_a_strip_above_32k', 'distance_one_byte_too_far',
                   'run_crossing_from_lengths_into_distances', 'one_code_distance_alphabet', 'zero_code_distance_alphabet_literals_only'):
        assert needed in names
    assert {c[3] for c in ic.hand_cases()} == set(ic.ALL_CLASSES), 'the hand cases hold every class'


def _strip_file(stream, want, compression=8):
    return dc.tiff_file([stream], 1, want, 1, compression=compression)


def test_the_host_reader_puts_every_case_in_its_class(tmp_path):
    """ecseg_tiff_read on a one-strip file around each stream: the samples of an OK case (zero-filled, cut at the strip), an error
    for a corrupt one.  The class that depends on the zlib version follows that version here; the device follows 1.2.9."""
    new_rule = tuple(int(v) for v in zlib.ZLIB_RUNTIME_VERSION.split('.')[:3] if v.isdigit()) >= (1, 2, 9)
    path = str(tmp_path / 'case.tif')
    seen = set()
    for name, stream, want, cls, out in ic.hand_cases() + ic.zlib_streams():
        with open(path, 'wb') as f:
            f.write(_strip_file(stream, want, 8 if len(seen) % 2 else 32946))
        ok = cls.startswith('ok') or (cls == ic.TRUNCATED and not new_rule)
        if ok:
            got = image_io._native_tiff(path)
            if out is not None:
                assert got.tobytes() == (out + bytes(want))[:want], name
        else:
            with pytest.raises(image_io.TiffError):
                image_io._native_tiff(path)
        seen.add(cls)
    assert seen == set(ic.ALL_CLASSES)


def _san_build(tmp_path):
    cxx = shutil.which('g++') or shutil.which('clang++')
    if not cxx:
        pytest.skip('no host C++ compiler')
    san = ['-fsanitize=address,undefined', '-fno-sanitize-recover=all']
    probe = tmp_path / 'probe.cpp'
    probe.write_text('int main() { return 0; }\n')
    if subprocess.run([cxx] + san + [str(probe), '-o', str(tmp_path / 'probe')], capture_output=True, timeout=120).returncode != 0:
        pytest.skip('the host compiler cannot link the sanitizer runtimes')
    exe = str(tmp_path / 'tiff_inflate_fuzz')
    cmd = [cxx, '-std=c++17', '-O1', '-g', '-fno-omit-frame-pointer', '-Wall', '-Werror'] + san + [
        os.path.join(ROOT, 'tools', 'asan', 'tiff_inflate_fuzz.cpp'), '-lz', '-o', exe]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-3000:]
    return exe


def test_the_strip_routine_equals_the_host_rule_under_the_sanitizers(tmp_path):
    """The stand-alone program (its own main, no preloaded runtime): built-in streams, then the corpus the device tests decode - the
    hand cases in the class they are built for, zlib's streams, the seeded mutations - and every class reached."""
    exe = _san_build(tmp_path)
    cases = ic.hand_cases() + ic.zlib_streams()
    records = [(s, w) for _, s, w, _, _ in cases] + [(s, w) for _, s, w in ic.mutations()]
    with open(tmp_path / 'corpus.bin', 'wb') as f:
        for stream, want in records:
            f.write(struct.pack('<II', len(stream), want) + stream)
    run = subprocess.run([exe, str(tmp_path / 'corpus.bin'), 'list'], capture_output=True, text=True, timeout=900)
    assert run.returncode == 0, (run.stdout + run.stderr)[-3000:]
    assert 'tiff_inflate_fuzz ok' in run.stdout and '%d corpus records' % len(records) in run.stdout, run.stdout[-2000:]
    listed = dict(line.split(' ', 2)[1:] for line in run.stdout.split('\n') if line.startswith('record '))
    for k, (name, _, _, cls, _) in enumerate(cases):
        assert listed[str(k)] == cls, (name, listed[str(k)], cls)
    by_class = {}
    for k in range(len(records)):
        by_class[listed[str(k)]] = by_class.get(listed[str(k)], 0) + 1
    assert set(by_class) >= set(ic.ALL_CLASSES), set(ic.ALL_CLASSES) - set(by_class)
    mutated = {listed[str(k)] for k in range(len(cases), len(records))}
    assert any(c.startswith('ok') for c in mutated) and len([c for c in mutated if c.startswith('corrupt')]) >= 6, mutated
    totals = dict((line.split(' ', 2)[2], int(line.split(' ', 2)[1])) for line in run.stdout.split('\n') if line.startswith('class '))
    assert all(totals.get(c, 0) >= 1 for c in ic.ALL_CLASSES), totals


# ---- the routing functions --------------------------------------------------------------------------------------------------------
def _file_of_strips(n, compression):
    strip = zlib.compress(bytes(8)) if compression in (8, 32946) else dc.pack(dc.lzw_codes(bytes(8))) if compression == 5 else bytes(8)
    return dc.tiff_file([strip] * n, n, 8, 1, compression=compression)


def _ptr(a):
    import ctypes as C
    return a.ctypes.data_as(C.c_void_p)


def test_the_flagged_routing_functions_answer_as_the_old_ones_with_the_flag_off_and_by_the_thresholds_with_it_on():
    """csrc/tiff_parse.h: the Deflate thresholds are measured; where no measured cell wins they are "never", and the
    flagged functions then send no Deflate file on their own - only an explicit decode call takes one to the device."""
    lib = _lib.load_library()
    text = open(os.path.join(ROOT, 'ecseg_amd', 'csrc', 'tiff_parse.h')).read()

    def threshold(name):
        value = text.split('constexpr size_t %s = ' % name)[1].split(';')[0]
        return None if value == 'TIFF_DEFLATE_NEVER' else int(value)
    single, batch = threshold('TIFF_DEFLATE_DEVICE_MIN_STRIPS'), threshold('TIFF_DEFLATE_BATCH_DEVICE_MIN_STRIPS')
    for comp in (1, 5, 8, 32946):
        for n in (1, 208, 1040, 3000):
            one = np.frombuffer(_file_of_strips(n, comp), np.uint8)
            buf, ranges = _lib.pack_file_images([one, one])
            answers = lambda kinds: (lib.ecseg_tiff_decode_routes(_ptr(one), one.size, kinds), lib.ecseg_tiff_decode_batch_counts(_ptr(one), one.size, kinds),
                                     lib.ecseg_tiff_decode_batch_routes(_ptr(buf), buf.size, _ptr(ranges), 2, kinds))
            old, on = answers(0), answers(_lib.TIFF_DEFLATE)
            for more in (_lib.TIFF_TILED, _lib.TIFF_PACKBITS, _lib.TIFF_TILED | _lib.TIFF_PACKBITS):     # a file of strips: the other two kinds change nothing
                assert answers(more) == old and answers(_lib.TIFF_DEFLATE | more) == on, (comp, n, more)
            assert image_io.tiff_goes_to_device(one.tobytes()) == bool(old[0]) and image_io.tiff_goes_to_device(one.tobytes(), deflate=True) == bool(on[0])
            if comp in (1, 5):
                assert on == old, (comp, n)
                continue
            assert old == (0, 0, 0), 'a Deflate file never counts without the flag'
            want = (int(single is not None and n >= single), int(batch is not None), int(batch is not None and 2 * n >= batch))
            assert on == want, (comp, n, on, want)
            # the arena: nothing for a Deflate file without the flag (it is left out), with it what an LZW file of the same tags needs
            lzw = np.frombuffer(_file_of_strips(n, 5), np.uint8)
            r1 = np.array([[0, one.size]], np.int64)
            assert lib.ecseg_tiff_decode_batch_bytes(_ptr(one), one.size, _ptr(r1), 1, _lib.TIFF_TILED | _lib.TIFF_PACKBITS) == lib.ecseg_tiff_decode_batch_bytes(_ptr(one), one.size, _ptr(r1), 1, 0) == 6 * 256
            need = lib.ecseg_tiff_decode_batch_bytes(_ptr(one), one.size, _ptr(r1), 1, _lib.TIFF_DEFLATE)
            assert need == lib.ecseg_tiff_decode_batch_bytes(_ptr(one), one.size, _ptr(r1), 1, 7)
            slot = lambda v: (v + 255) // 256 * 256
            r2 = np.array([[0, lzw.size]], np.int64)
            assert need - slot(one.size) == lib.ecseg_tiff_decode_batch_bytes(_ptr(lzw), lzw.size, _ptr(r2), 1, 0) - slot(lzw.size) > 0


# ---- make stat_fish: the key ---------------------------------------------------------------------------------------------------------
class ReadingHandle(cpu.RenderingOracleHandle):
    """A handle whose ``tiff_decode`` is answered by the host reader and recorded, with the switch it was given."""

    def tiff_decode(self, data, deflate=None):
        self.calls.append(dict(tiff_decode=len(data), deflate=deflate))
        path = os.path.join(self.tmp, 'decode_%d.tif' % len(self.calls))
        with open(path, 'wb') as f:
            f.write(data)
        return image_io.read_tiff(path)


def _set_key(tmp_path, **keys):
    cfg = yaml.safe_load(open(tmp_path / 'config.yaml'))
    cfg['stat_fish'].update(keys)
    yaml.safe_dump(cfg, open(tmp_path / 'config.yaml', 'w'))


@pytest.mark.parametrize('value', [3, 'yes', 0, [True], None])
def test_a_tiff_read_deflate_that_is_no_boolean_is_a_configuration_error(tmp_path, monkeypatch, capsys, value):
    inp, _ = cpu.make_folder(tmp_path, kinds=(('one', 'tif'),), size=(40, 50), color_sensitivity=(70, 70))
    _set_key(tmp_path, tiff_read_deflate=value)
    monkeypatch.chdir(tmp_path)
    handle = ReadingHandle()
    with pytest.raises(SystemExit) as e:
        sf.main([], handle=handle)
    assert e.value.code == 2 and 'tiff_read_deflate must be true or false' in capsys.readouterr().out
    assert not os.path.exists(inp / 'annotated') and not handle.calls


def test_the_key_hands_the_switch_to_imread_only_with_tiff_read_on_device_and_keeps_every_byte(tmp_path, monkeypatch, capsys):
    inp, _ = cpu.make_folder(tmp_path, size=(40, 50))
    monkeypatch.chdir(tmp_path)
    handed = []
    imread = image_io.imread

    def spy(path, handle=None, **kw):
        handed.append((handle is not None, kw))
        return imread(path, handle=handle, **kw)
    monkeypatch.setattr(image_io, 'imread', spy)
    monkeypatch.setattr(image_io, 'tiff_goes_to_device', lambda data, deflate=False: True)
    runs = {}
    for name, keys in (('absent', {}), ('alone', dict(tiff_read_deflate=True)), ('read', dict(tiff_read_on_device=True, tiff_read_deflate=False)),
                       ('both', dict(tiff_read_on_device=True, tiff_read_deflate=True))):
        _set_key(tmp_path, **keys)
        handle = ReadingHandle()
        handle.tmp = str(tmp_path)
        del handed[:]
        sf.main([], handle=handle)
        runs[name] = (cpu.folder_bytes(inp / 'annotated'), [c for c in handle.calls if 'tiff_decode' in c], capsys.readouterr().out, list(handed))
    assert not runs['absent'][1] and not runs['alone'][1] and not any(h or kw for h, kw in runs['absent'][3] + runs['alone'][3]), 'ignored without tiff_read_on_device'
    assert len(runs['read'][1]) == 4 and all(c['deflate'] is None for c in runs['read'][1]) and all(h and not kw for h, kw in runs['read'][3])
    assert len(runs['both'][1]) == 4 and all(c['deflate'] is True for c in runs['both'][1]) and all(h and kw == dict(deflate=True) for h, kw in runs['both'][3])
    for name in ('alone', 'read', 'both'):
        assert runs[name][2] == runs['absent'][2], 'the messages differ'
        assert runs[name][0] == runs['absent'][0], name


def test_imread_many_hands_the_switch_to_the_rule_and_to_the_handle(tmp_path, monkeypatch):
    paths = []
    for k in range(3):
        p = str(tmp_path / ('z_%d.tif' % k))
        open(p, 'wb').write(_file_of_strips(4 + k, 8))
        paths.append(p)
    asked = []

    def rule(datas, deflate=False):
        asked.append(deflate)
        return True, [True] * len(datas)
    monkeypatch.setattr(image_io, 'tiff_batch_goes_to_device', rule)

    class Device:
        def __init__(self):
            self.seen = []

        def tiff_decode_many(self, datas, **kw):
            self.seen.append((len(datas), kw))
            return [np.full((2, 2), 7, np.uint8)] * len(datas)
    dev = Device()
    got = image_io.imread_many(paths, handle=dev, deflate=True)
    assert asked == [True] and dev.seen == [(3, dict(deflate=True))] and all(np.array_equal(a, np.full((2, 2), 7, np.uint8)) for a in got)
    dev = Device()
    image_io.imread_many(paths, handle=dev)
    assert asked == [True, False] and dev.seen == [(3, {})]
    # the real rule: Deflate files are not counted without the switch
    monkeypatch.undo()
    goes, counts = image_io.tiff_batch_goes_to_device([open(p, 'rb').read() for p in paths])
    assert not goes and counts == [False] * 3
