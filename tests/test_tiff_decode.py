"""The device TIFF reader without a GPU: the new symbols, the ``tiff_read_on_device`` key of ``make stat_fish`` on injected handles,
``image_io.imread(path, handle=...)``, the routing rule on hand-made strip tables, and the per-strip LZW routine of
tiffb_unstrip_kernel (td_lzw_strip) compiled for the host under ASan + UBSan on the tolerated and the corrupt streams of
tests/tiff_decode_cases.py."""
import os
import shutil
import struct
import subprocess
import sys

import numpy as np
import pytest
import yaml

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lzw_ref                               # noqa: E402
import test_stat_fish_aqua as cpu            # noqa: E402
import tiff_decode_cases as dc               # noqa: E402
from ecseg_amd import _lib, build, image_io  # noqa: E402
from ecseg_amd import stat_fish as sf        # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_binding_and_documents_name_the_new_symbol():
    hdr = open(os.path.join(ROOT, 'include', 'ecseg_hip.h')).read()
    assert 'int ecseg_tiff_decode(ecseg_ctx* h, const uint8_t* file, long long n_bytes, void* dst, long long dst_bytes,' in hdr
    assert 'int* H, int* W, int* samples_per_pixel, int* bits_per_sample);' in hdr and 'int ecseg_tiff_decode_routes(const uint8_t* file, long long n_bytes, unsigned kinds);' in hdr
    assert 'still 5 - additive: ecseg_tiff_decode' in hdr and '#define ECSEG_ABI_VERSION 6' in hdr and _lib.ABI_VERSION == 6
    assert 'still 5 - additive: ecseg_tiff_encode_bound' in hdr                 # the earlier lines stay
    assert 'skimage.io.imread' in hdr.split('int ecseg_tiff_decode(')[0][-2500:] and 'src/utils.py:110' in hdr.split('int ecseg_tiff_decode(')[0][-2500:]
    lib = _lib.load_library()
    for name in ('ecseg_tiff_decode', 'ecseg_tiff_decode_routes'):
        assert name in _lib.EXPORTS and hasattr(lib, name), name
    assert hasattr(_lib.Handle, 'tiff_decode') and 'tiff_decode_kernels.hip' in build.SOURCES
    for doc in ('DESIGN.md', 'README.md', 'INTEGRATION.md'):
        text = open(os.path.join(ROOT, doc)).read()
        assert 'tiff_read_on_device' in text and 'ecseg_tiff_decode' in text, doc
    assert '# tiff_read_on_device' in open(os.path.join(ROOT, 'config.yaml')).read()
    assert 'tiff_read_on_device' not in (yaml.safe_load(open(os.path.join(ROOT, 'config.yaml')))['stat_fish'])


def test_the_code_list_packer_writes_the_host_encoders_bytes():
    """tests/tiff_decode_cases.py builds its streams from code lists: on a whole strip the list, packed, is the encoder's stream."""
    for data in (b'', b'a', bytes(200), dc._noise(1, 9000), dc._noise(2, 30000, 5)):
        assert dc.pack(dc.lzw_codes(data)) == lzw_ref.encode(data).data, len(data)


class ReadingHandle(cpu.RenderingOracleHandle):
    """A handle whose ``tiff_decode`` is answered by the host reader and recorded."""

    def tiff_decode(self, data):
        self.calls.append(dict(tiff_decode=len(data)))
        path = os.path.join(self.tmp, 'decode_%d.tif' % len(self.calls))
        with open(path, 'wb') as f:
            f.write(data)
        return image_io.read_tiff(path)


def _set_key(tmp_path, **keys):
    cfg = yaml.safe_load(open(tmp_path / 'config.yaml'))
    cfg['stat_fish'].update(keys)
    yaml.safe_dump(cfg, open(tmp_path / 'config.yaml', 'w'))


@pytest.mark.parametrize('value', [3, 'yes', 0, [True], None])
def test_a_value_that_is_no_boolean_is_a_configuration_error(tmp_path, monkeypatch, capsys, value):
    inp, _ = cpu.make_folder(tmp_path, kinds=(('one', 'tif'),), size=(40, 50), color_sensitivity=(70, 70))
    _set_key(tmp_path, tiff_read_on_device=value)
    monkeypatch.chdir(tmp_path)
    handle = ReadingHandle()
    with pytest.raises(SystemExit) as e:
        sf.main([], handle=handle)
    assert e.value.code == 2 and 'tiff_read_on_device must be true or false' in capsys.readouterr().out
    assert not os.path.exists(inp / 'annotated') and not [d for d in os.listdir(inp) if d.startswith('tmp_')] and not handle.calls


def test_a_handle_without_tiff_decode_is_a_configuration_error(tmp_path, monkeypatch, capsys):
    inp, _ = cpu.make_folder(tmp_path, kinds=(('one', 'tif'),), size=(40, 50), color_sensitivity=(70, 70))
    _set_key(tmp_path, tiff_read_on_device=True)
    monkeypatch.chdir(tmp_path)
    handle = cpu.RenderingOracleHandle()
    with pytest.raises(SystemExit) as e:
        sf.main([], handle=handle)
    out = capsys.readouterr().out
    assert e.value.code == 2 and 'tiff_read_on_device: true needs the device TIFF reader (tiff_decode), which the handle in use' in out
    assert 'only tiff_read_on_device: false works on it' in out
    assert not os.path.exists(inp / 'annotated') and not handle.calls
    _set_key(tmp_path, tiff_read_on_device=False)             # the same handle runs with the key off
    sf.main([], handle=cpu.RenderingOracleHandle())
    assert os.path.isdir(inp / 'annotated')


def test_the_key_off_or_absent_never_calls_tiff_decode_and_on_keeps_every_byte(tmp_path, monkeypatch, capsys):
    """With the key on the image read and the mask read hand the handle to ``imread`` (which asks the routing rule: here every file
    is sent, to see the calls); off or absent they never do."""
    inp, _ = cpu.make_folder(tmp_path, size=(40, 50))
    monkeypatch.chdir(tmp_path)
    handed = []
    imread = image_io.imread

    def spy(path, handle=None):
        handed.append((os.path.basename(str(path)), handle is not None))
        return imread(path, handle=handle)
    monkeypatch.setattr(image_io, 'imread', spy)
    monkeypatch.setattr(image_io, 'tiff_goes_to_device', lambda data: True)
    runs = {}
    for name, keys in (('absent', {}), ('on', dict(tiff_read_on_device=True)), ('off', dict(tiff_read_on_device=False))):
        _set_key(tmp_path, **keys)
        handle = ReadingHandle()
        handle.tmp = str(tmp_path)
        del handed[:]
        sf.main([], handle=handle)
        runs[name] = (cpu.folder_bytes(inp / 'annotated'), [c for c in handle.calls if 'tiff_decode' in c], capsys.readouterr().out, list(handed))
    assert not runs['absent'][1] and not runs['off'][1] and not any(h for _, h in runs['absent'][3] + runs['off'][3])
    assert len(runs['on'][1]) == 1 + 3, 'the one TIFF image and the three masks go through tiff_decode'
    assert len(runs['on'][3]) == 6 and all(h for _, h in runs['on'][3]), runs['on'][3]
    assert runs['on'][2] == runs['absent'][2] == runs['off'][2], 'the messages differ'
    want = runs['absent'][0]
    for name in ('on', 'off'):
        got = runs[name][0]
        assert sorted(got) == sorted(want)
        for f in want:
            assert got[f] == want[f], (name, f)


def test_imread_with_a_handle_falls_back_on_none_on_corrupt_files_and_without_the_method(tmp_path):
    img = (np.arange(1040 * 8200) % 251).astype(np.uint8).reshape(1040, 8200)      # one row per strip: the rule sends it to the device
    path = str(tmp_path / 'a.tif')
    image_io.write_tiff_gray8(path, img)
    small = str(tmp_path / 'small.tif')
    image_io.write_tiff_gray8(small, img[:5, :7])

    class Device:
        def __init__(self, answer):
            self.answer, self.seen = answer, []

        def tiff_decode(self, data):
            self.seen.append(bytes(data))
            if isinstance(self.answer, Exception):
                raise self.answer
            return self.answer

    taken = Device(img + 1)
    assert np.array_equal(image_io.imread(path, handle=taken), img + 1) and taken.seen == [open(path, 'rb').read()]
    unasked = Device(img + 1)
    assert np.array_equal(image_io.imread(small, handle=unasked), img[:5, :7]) and not unasked.seen, 'a file the rule keeps on the host'
    left = Device(None)
    assert np.array_equal(image_io.imread(path, handle=left), img) and len(left.seen) == 1
    corrupt = _lib.EcsegError('ecseg_tiff_decode failed (-1)')
    corrupt.code = -1
    assert np.array_equal(image_io.imread(path, handle=Device(corrupt)), img)      # the host reader states the error, or reads the file
    broken = _lib.EcsegError('ecseg_tiff_decode failed (-3)')
    broken.code = -3
    with pytest.raises(_lib.EcsegError):
        image_io.imread(path, handle=Device(broken))
    assert np.array_equal(image_io.imread(path, handle=object()), img) and np.array_equal(image_io.imread(path), img)
    npy = str(tmp_path / 'a.npy')
    np.save(npy, img)
    never = Device(img + 1)
    assert np.array_equal(image_io.imread(npy, handle=never), img) and not never.seen
    with pytest.raises(Exception) as e:
        image_io.imread(str(tmp_path / 'missing.tif'), handle=Device(None))
    with pytest.raises(Exception) as e0:
        image_io.imread(str(tmp_path / 'missing.tif'))
    assert type(e.value) is type(e0.value) and str(e.value) == str(e0.value)


def _file_of_strips(n, compression=5, table=None):
    """A gray n x 8 file of n one-row strips (their bytes are never read by the rule)."""
    strip = dc.pack(dc.lzw_codes(bytes(8)))
    kw = {} if table is None else dict(counts=[len(strip)] * table)
    return dc.tiff_file([strip] * n, n, 8, 1, compression=compression, **kw)


def test_the_routing_rule_on_hand_made_strip_tables():
    """One rule (csrc/tiff_parse.h, asked through ecseg_tiff_decode_routes by image_io.imread): LZW and at least 1040 strips, the
    smallest count at which the device call was measured faster than the host reader."""
    goes = image_io.tiff_goes_to_device
    assert goes(_file_of_strips(1040)) and goes(_file_of_strips(3000)) and not goes(_file_of_strips(1039)) and not goes(_file_of_strips(208))
    assert not goes(_file_of_strips(1)) and not goes(_file_of_strips(70))
    assert not goes(_file_of_strips(1040, compression=1)) and not goes(_file_of_strips(1040, compression=8)), 'raw and Deflate stay on the host'
    assert not goes(_file_of_strips(1040, table=1039)), 'a table shorter than the image'
    assert not goes(dc.tiff_file([bytes(8)] * 2, 2080, 8, 1040)), 'two strips of 1040 rows'
    assert not goes(b'') and not goes(b'II*\0') and not goes(_file_of_strips(1040)[:-20]), 'what cannot be parsed stays with the host readers'
    # the full-size inputs of make stat_fish from this library's writers: the RGB image goes, the mask (208 strips) does not
    import tempfile
    with tempfile.TemporaryDirectory() as tmp:
        rgb, gray = os.path.join(tmp, 'rgb.tif'), os.path.join(tmp, 'gray.tif')
        image_io.write_tiff_rgb8(rgb, np.zeros((1040, 1392, 3), np.uint8))
        image_io.write_tiff_gray8(gray, np.zeros((1040, 1392), np.uint8))
        assert goes(open(rgb, 'rb').read()) and not goes(open(gray, 'rb').read())


def _san_build(tmp_path):
    cxx = shutil.which('g++') or shutil.which('clang++')
    if not cxx:
        pytest.skip('no host C++ compiler')
    san = ['-fsanitize=address,undefined', '-fno-sanitize-recover=all']
    probe = tmp_path / 'probe.cpp'
    probe.write_text('int main() { return 0; }\n')
    if subprocess.run([cxx] + san + [str(probe), '-o', str(tmp_path / 'probe')], capture_output=True, timeout=120).returncode != 0:
        pytest.skip('the host compiler cannot link the sanitizer runtimes')
    exe = str(tmp_path / 'tiff_decode_fuzz')
    cmd = [cxx, '-std=c++17', '-O1', '-g', '-fno-omit-frame-pointer', '-Wall', '-Werror'] + san + [
        os.path.join(ROOT, 'ecseg_amd', 'csrc', 'host_codec.cpp'), os.path.join(ROOT, 'tools', 'asan', 'tiff_decode_fuzz.cpp'), '-o', exe]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-3000:]
    return exe


def test_the_strip_routine_equals_the_host_decoder_under_the_sanitizers(tmp_path):
    """The stand-alone program (its own main, no preloaded runtime): built-in streams, then every strip of the tolerated files and
    of the corrupt corpus - the corpus tests/test_gpu_tiff_decode.py decodes on the device."""
    exe = _san_build(tmp_path)
    files = dc.tolerated_files() + dc.corrupt_corpus()
    assert len(dc.corrupt_corpus()) == 200 and len({name for name, _ in files}) == len(files)
    records = 0
    with open(tmp_path / 'corpus.bin', 'wb') as f:
        for _, data in files:
            for stream, want in dc.strips_of(data):
                f.write(struct.pack('<II', len(stream), want) + stream)
                records += 1
    assert records >= len(files)
    run = subprocess.run([exe, str(tmp_path / 'corpus.bin')], capture_output=True, text=True, timeout=600)
    assert run.returncode == 0, (run.stdout + run.stderr)[-3000:]
    assert 'tiff_decode_fuzz ok' in run.stdout and '%d corpus records' % records in run.stdout, run.stdout
    assert 'asan_tiff_decode:' in open(os.path.join(ROOT, 'Makefile')).read()


def test_the_corpora_hold_what_they_are_named_for(tmp_path):
    """The host reader on the tolerated files: all of them read, the zero fill where it is owed; the corrupt corpus holds streams of
    both outcomes."""
    def host(data, name):
        path = str(tmp_path / (name + '.tif'))
        with open(path, 'wb') as f:
            f.write(data)
        return image_io._native_tiff(path)
    got = {name: host(data, name) for name, data in dc.tolerated_files()}
    whole = got['well_formed']
    assert whole.shape == (40, 50) and np.array_equal(whole.tobytes(), dc._noise(31, 2000, 7))
    for name in ('no_leading_clearcode', 'no_eoi', 'two_clearcodes_in_a_row'):
        assert np.array_equal(got[name], whole), name
    cut = got['byte_count_cut_short'].reshape(-1)
    assert 1000 < np.flatnonzero(cut)[-1] < 1990 and np.array_equal(cut[:1000], whole.reshape(-1)[:1000])
    assert np.array_equal(got['strip_holds_more_than_want'], whole[:31])
    assert got['table_full_without_clearcode'].tobytes() == dc._noise(32, 24000) == got['two_clearcodes_at_a_restart'].tobytes()
    short = got['table_shorter_than_the_image']
    assert np.array_equal(short[:20], whole[:20]) and not short[20:].any()
    with pytest.raises(image_io.TiffError):
        host(dc.offset_behind_the_file(), 'behind')
    outcomes = []
    for name, data in dc.corrupt_corpus():
        try:
            host(data, 'c')
            outcomes.append(True)
        except image_io.TiffError:
            outcomes.append(False)
    cuts, flips = outcomes[0::2], outcomes[1::2]
    assert all(cuts), 'a truncated stream is a stream without EOI: accepted with what it gave'
    assert any(flips) and not all(flips), 'the bit flips hold no corrupt stream, or nothing else'
