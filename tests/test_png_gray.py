"""The gray-channel PNG coder without a GPU: the new symbols; the host writer (the yardstick of the device coder) on every case of
tests/png_gray_cases.py against zlib and the input channel; a run-length analysis that holds every case to the branch it is named
for; ecseg_png_channel_bound; the ``files_on_device`` key of ``make meta_overlay`` on injected handles; and the per-block pieces of the
kernels walked on the host under ASan + UBSan (tools/asan/png_gray_fuzz.cpp, ``make asan_png_gray``)."""
import os
import shutil
import struct
import subprocess
import sys
import zlib

import numpy as np
import pytest
import yaml

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import png_gray_cases as gc                  # noqa: E402
from ecseg_amd import _lib, image_io, image_tools, meta_overlay      # noqa: E402
from ecseg_amd.utils import get_imgs         # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_HOST = {}


def host_file(name, px, channel, invert, tmp_path_factory, i=0):
    if (name, i) not in _HOST:
        path = str(tmp_path_factory.mktemp('host') / 'c.png')
        image_io.write_png_channel(path, px[i], channel, invert=bool(invert))
        _HOST[(name, i)] = open(path, 'rb').read()
    return _HOST[(name, i)]


def test_header_binding_and_documents_name_the_new_symbols():
    hdr = open(os.path.join(ROOT, 'include', 'ecseg_hip.h')).read()
    assert 'long long ecseg_png_channel_bound(int H, int W);' in hdr
    assert ('int ecseg_png_channel_encode(ecseg_ctx* h, const uint8_t* pixels /* (n_img,H,W,C) host */, int n_img, int H, int W, int C, int channel, int invert,\n'
            '                             uint8_t* const* files, long long file_cap, long long* file_bytes);') in hdr
    assert 'int ecseg_overlay_files(ecseg_ctx* h, const uint8_t* labels, const void* img, int n_img, int H, int W, int C, int bytes_per_sample /* 1 | 2 */,' in hdr
    assert 'still 5 - additive: ecseg_png_channel_encode' in hdr and '#define ECSEG_ABI_VERSION 6' in hdr and _lib.ABI_VERSION == 6
    assert 'still 5 - additive: ecseg_png_labels_encode' in hdr                               # the earlier lines stay
    lib = _lib.load_library()
    for name in ('ecseg_png_channel_bound', 'ecseg_png_channel_encode', 'ecseg_overlay_files'):
        assert name in _lib.EXPORTS and hasattr(lib, name), name
    assert hasattr(_lib.Handle, 'png_channel_encode') and hasattr(_lib.Handle, 'overlay_files')
    for doc in ('DESIGN.md', 'README.md', 'INTEGRATION.md'):
        text = open(os.path.join(ROOT, doc)).read()
        assert 'files_on_device' in text and 'ecseg_png_channel_encode' in text and 'ecseg_overlay_files' in text, doc
    assert 'asan_png_gray:' in open(os.path.join(ROOT, 'Makefile')).read()
    kernels = open(os.path.join(ROOT, 'ecseg_amd', 'csrc', 'png_gray_kernels.hip')).read()
    for k in ('pgray_count_kernel', 'pgray_bits_kernel', 'pgray_scan_kernel', 'pgray_emit_kernel'):
        assert k in kernels, k
    host = open(os.path.join(ROOT, 'ecseg_amd', 'csrc', 'host_io.cpp')).read()
    assert '#include "png_gray_code.h"' in host and 'void rle_scan' not in host                # one definition, in the header
    cfg = yaml.safe_load(open(os.path.join(ROOT, 'config.yaml')))
    assert 'files_on_device' not in cfg['meta_overlay']                                        # the shipped default: off


def _idat(file):
    n, = struct.unpack('>I', file[33:37])
    assert file[37:41] == b'IDAT' and len(file) == 41 + n + 16
    return file[41:41 + n]


@pytest.mark.parametrize('case', gc.CASES, ids=gc.IDS)
def test_the_host_file_inflates_and_unfilters_to_the_channel(case, tmp_path_factory):
    name, px, channel, invert = case
    n, H, W, _ = px.shape
    for i in range(n):
        file = host_file(name, px, channel, invert, tmp_path_factory, i)
        assert file[:8] == b'\x89PNG\r\n\x1a\n' and struct.unpack('>II', file[16:24]) == (W, H) and file[24:29] == bytes([8, 0, 0, 0, 0])
        z = _idat(file)
        rows = np.frombuffer(zlib.decompress(z), np.uint8).reshape(H, W + 1)
        assert np.array_equal(rows, gc.stream_of(px[i, ..., channel], invert))
        assert np.array_equal(np.cumsum(rows[:, 1:].astype(np.uint64), axis=1).astype(np.uint8), px[i, ..., channel] ^ np.uint8(255 if invert else 0))
        assert struct.unpack('>I', z[-4:])[0] == zlib.adler32(rows.tobytes())
        assert len(file) <= _lib.load_library().ecseg_png_channel_bound(H, W)


def test_the_bound_holds_full_range_noise_and_refuses_empty_extents(tmp_path_factory):
    lib = _lib.load_library()
    px = np.random.default_rng(11).integers(0, 256, (1, 33, 200, 3), dtype=np.uint8)
    size = len(host_file('full_range_noise', px, 2, 0, tmp_path_factory))
    bound = lib.ecseg_png_channel_bound(33, 200)
    assert 33 * 201 < size <= bound <= 57 + 2 * 33 * 201 + 4096
    assert lib.ecseg_png_channel_bound(0, 5) == -1 and lib.ecseg_png_channel_bound(5, 0) == -1 and lib.ecseg_png_channel_bound(-1, -1) == -1
    assert lib.ecseg_png_channel_bound(1, 1) >= 57 + 2 + 6


def _code_lengths(z):
    """the 286 literal / length code lengths and the distance code's length from the block header of a stream of this coder"""
    bits = np.unpackbits(np.frombuffer(z[2:2 + 200], np.uint8), bitorder='little')
    assert list(bits[:3]) == [1, 0, 1]                                                         # BFINAL, BTYPE = 2
    val = lambda a: int(sum(int(b) << k for k, b in enumerate(a)))
    assert (val(bits[3:8]), val(bits[8:13]), val(bits[13:17])) == (286 - 257, 0, 19 - 4)
    order = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]
    cl = dict(zip(order, (val(bits[17 + 3 * k:20 + 3 * k]) for k in range(19))))
    assert all(cl[k] == (4 if k < 13 else 5) for k in range(19))
    pos, out = 17 + 57, []
    for _ in range(287):                                                                       # canonical: 0..12 in 4 bits, 13..18 as 26..31 in 5
        v = int(bits[pos]) * 8 + int(bits[pos + 1]) * 4 + int(bits[pos + 2]) * 2 + int(bits[pos + 3])
        pos += 4
        if v >= 13:
            v = 13 + (2 * v + int(bits[pos])) - 26
            pos += 1
        out.append(v)
    return out[:286], out[286]


def test_every_case_takes_the_branch_it_is_named_for(tmp_path_factory):
    seen = set()
    by_name = {c[0]: c for c in gc.CASES}
    for name, px, channel, invert in gc.CASES:
        n, H, W, _ = px.shape
        for i in range(n):
            flat = gc.stream_of(px[i, ..., channel], invert).ravel()
            starts, lens = gc.runs_of(flat)
            branches = {gc.split_branch(int(R) - 1) for R in lens if R >= 4}
            crossing = bool(((starts % (W + 1) != 0) & (starts // (W + 1) != (starts + lens - 1) // (W + 1)) & (lens >= 4)).any())
            z = _idat(host_file(name, px, channel, invert, tmp_path_factory, i))
            llen, dlen = _code_lengths(z)
            assert dlen == (1 if branches else 0), name                                       # any_match picks the distance code
            if name.startswith('ramp'):
                assert len(lens) == 1 and lens[0] == H * (W + 1), name
                seen |= {('ramp', b) for b in branches}
            if name.startswith('noise'):
                assert not branches and lens.max() < 4, name
                seen.add('no_match')
            if name.startswith('run'):
                _, border, placement = name.split('_')[:3]
                R = int(name[3:name.index('_')])
                at, byte = gc.placed_run(R, border, placement)
                b = gc.PLACED_BORDERS[border]
                k = int(np.searchsorted(starts, at))
                assert starts[k] == at and lens[k] == R and flat[at] == byte, name             # the run itself, at its exact length
                assert (np.delete(lens, k) == 1).all(), name                                   # and no other run
                assert {'start': at == b, 'end': at + R == b, 'straddle': at < b < at + R}[placement], name
                assert b % {'block': 64, 'span': 1024, 'line': W + 1}[border] == 0 and (border == 'span' or b % 1024 != 0), name
                assert (R < 4) == (not branches), name
                seen.add(('run', R, border, placement))
                seen |= {('run', b) for b in branches}
                if border == 'line' and placement == 'straddle' and R >= 4:
                    assert crossing and byte == 1, name
            if crossing:
                seen.add('crossing')
            if max(llen) == 15:
                seen.add('15_bits')
            if name.startswith('fibonacci'):
                assert max(llen) == 15, max(llen)
            seen |= {('any', b) for b in branches}
    ramp_n = {H * (W + 1) - 1 for H, W in gc.RAMP_EXTENTS}
    assert ramp_n == {258, 259, 260, 261, 516, 517}
    assert {('ramp', b) for b in ('one', 'whole', 'tail', 'short_tail_1', 'short_tail_2')} <= seen
    assert {gc.split_branch(r) for r in sorted(ramp_n)} == {'one', 'short_tail_1', 'short_tail_2', 'tail', 'whole'}
    assert {('run', R, border, p) for R in gc.PLACED_LENGTHS for border in ('block', 'span', 'line') for p in gc.PLACEMENTS
            if (R, p) != (1, 'straddle')} <= seen
    assert {'no_match', 'crossing', '15_bits'} <= seen
    assert len(by_name) == len(gc.CASES)
    assert {px.shape[3] for _, px, _, _ in gc.CASES} == {2, 3, 4} and {px.shape[0] for _, px, _, _ in gc.CASES} == {1, 3}
    assert {(c, i) for _, _, c, i in gc.CASES} == {(0, 0), (0, 1), (1, 0), (1, 1)}
    for name, px, _, _ in gc.CASES:
        assert px.shape[0] == 1 or len({im.tobytes() for im in px}) == px.shape[0] or name.startswith(('ramp', 'zeros', 'run')), name


def test_the_token_rule_restated_is_the_streams_token_sequence(tmp_path_factory):
    """inflate's view of the host file: the literal / match sequence zlib's own inflate reproduces the rows from is not observable, so
    the rule is held through sizes - the bits of the restated tokens under the header's code give the stream's length exactly."""
    ebits = [0] * 8 + [1] * 4 + [2] * 4 + [3] * 4 + [4] * 4 + [5] * 4 + [0]
    base = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
    for name, px, channel, invert in gc.CASES:
        flat = gc.stream_of(px[0, ..., channel], invert).ravel()
        z = _idat(host_file(name, px, channel, invert, tmp_path_factory))
        llen, _ = _code_lengths(z)
        bits = 16 + 17 + 57 + sum(4 if v < 13 else 5 for v in llen) + 4 + llen[256]            # (the distance code's length is 0 or 1: 4 bits)
        for t in gc.tokens_of(flat):
            if t >= 0:
                bits += llen[t]
            else:
                k = max(j for j in range(29) if base[j] <= -t)
                bits += llen[257 + k] + ebits[k] + 1
        assert (bits + 7) // 8 + 4 == len(z), name


# ---- the files_on_device key of `make meta_overlay` on injected handles --------------------------------------------------------------
class PlainHandle:
    """What ``run`` needs of a handle today, with every call written down."""

    def __init__(self):
        self.calls = []

    def u16_to_u8(self, a):
        self.calls.append(('u16_to_u8', a.shape, a.dtype.str))
        return (a >> 8).astype(np.uint8)

    def overlay(self, labels, rgb, sensitivity, hsr_size_threshold=20):
        self.calls.append(('overlay', labels.shape, rgb.shape, rgb.dtype.str, sensitivity, hsr_size_threshold))
        return np.arange(labels.shape[0] * 12, dtype=np.int64).reshape(-1, 12) + int(rgb.sum() % 1000)


class FilesHandle(PlainHandle):
    def overlay_files(self, labels, img, sensitivity, hsr_size_threshold=20):
        self.calls.append(('overlay_files', labels.shape, img.shape, img.dtype.str, sensitivity, hsr_size_threshold))
        I8 = self.u16_to_u8(img) if img.dtype == np.uint16 else img
        rec = PlainHandle.overlay(self, labels, I8, sensitivity, hsr_size_threshold)
        self.calls = self.calls[:-2] if img.dtype == np.uint16 else self.calls[:-1]
        return rec, [b'red %d' % int(im[..., 0].sum()) for im in I8], [b'green %d' % int(im[..., 1].sum()) for im in I8]


def _folder(root, n=3):
    for sub in ('labels', 'dapi'):
        os.makedirs(root / sub)
    rng = np.random.default_rng(3)
    for i in range(n):
        image_io.write_tiff_rgb8(str(root / ('img%d.tif' % i)), rng.integers(0, 256, (24, 40, 3), dtype=np.uint8))
        np.save(str(root / 'labels' / ('img%d.npy' % i)), rng.integers(0, 4, (24, 40)).astype(np.int64))
    return str(root)


def _tree(root):
    return {sub + '/' + f: open(os.path.join(root, sub, f), 'rb').read() for sub in ('red', 'green') for f in sorted(os.listdir(os.path.join(root, sub)))}


def test_files_on_device_must_be_a_boolean_and_needs_a_handle_with_the_call(tmp_path, monkeypatch, capsys):
    inp = _folder(tmp_path / 'images')
    monkeypatch.chdir(tmp_path)
    monkeypatch.setattr(image_tools, 'default_handle', lambda: PlainHandle())
    for value in ('yes', 1, 'true', [True]):
        yaml.safe_dump({'meta_overlay': {'inpath': inp, 'color_sensitivity': 85, 'files_on_device': value}}, open(tmp_path / 'config.yaml', 'w'))
        with pytest.raises(SystemExit) as e:
            meta_overlay.main([])
        assert e.value.code == 2 and 'meta_overlay.files_on_device must be true or false' in capsys.readouterr().out
    yaml.safe_dump({'meta_overlay': {'inpath': inp, 'color_sensitivity': 85, 'files_on_device': True}}, open(tmp_path / 'config.yaml', 'w'))
    with pytest.raises(SystemExit) as e:
        meta_overlay.main([])
    assert e.value.code == 2 and 'files_on_device: true needs the device PNG coder' in capsys.readouterr().out
    assert not os.path.exists(os.path.join(inp, 'fish_quantification.csv'))
    with pytest.raises(ValueError, match='files_on_device'):
        meta_overlay.run(inp, PlainHandle(), get_imgs(inp), 85, files_on_device=True)


def test_the_key_off_takes_todays_path_call_for_call_and_on_writes_the_devices_bytes(tmp_path, monkeypatch, capsys):
    runs = {}
    for name, handle, cfg in (('absent', FilesHandle(), {}), ('off', FilesHandle(), {'files_on_device': False}), ('plain', PlainHandle(), {}),
                              ('on', FilesHandle(), {'files_on_device': True})):
        inp = _folder(tmp_path / name / 'images')
        monkeypatch.chdir(tmp_path / name)
        monkeypatch.setattr(image_tools, 'default_handle', lambda handle=handle: handle)
        yaml.safe_dump({'meta_overlay': dict(inpath=inp, color_sensitivity=85, batch_images=2, io_threads=2, **cfg)}, open('config.yaml', 'w'))
        meta_overlay.main([])
        runs[name] = (handle.calls, _tree(inp), open(os.path.join(inp, 'fish_quantification.csv')).read(), capsys.readouterr().out.replace(str(tmp_path / name), ''))
    want = [('overlay', (2, 24, 40), (2, 24, 40, 3), '|u1', 85, 20), ('overlay', (1, 24, 40), (1, 24, 40, 3), '|u1', 85, 20)]
    assert runs['plain'][0] == want
    assert runs['absent'] == runs['off'] == runs['plain']                                      # the key off: today's calls, files, rows and messages
    assert runs['on'][0] == [('overlay_files',) + c[1:] for c in want]
    assert runs['on'][2:] == runs['off'][2:] and sorted(runs['on'][1]) == sorted(runs['off'][1])
    assert all(v.startswith((b'red ', b'green ')) for v in runs['on'][1].values())
    assert all(v.startswith(b'\x89PNG') for v in runs['off'][1].values())


# ---- the sanitizer program ------------------------------------------------------------------------------------------------------------
def test_make_asan_png_gray_builds_and_runs_clean():
    """`make asan_png_gray`: ASan + UBSan build of tools/asan/png_gray_fuzz.cpp with the host writer (csrc/host_io.cpp)."""
    if not shutil.which('g++') or not shutil.which('make'):
        pytest.skip('no host toolchain')
    out = subprocess.run(['make', '-C', ROOT, 'asan_png_gray'], capture_output=True, text=True, timeout=900)
    if 'cannot find' in out.stderr and 'asan' in out.stderr:
        pytest.skip('libasan not installed')
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-3000:]
    assert 'png_gray_fuzz:' in out.stdout and 'ok' in out.stdout
