"""The device TIFF encoder without a GPU: the restatement tests/lzw_ref.py against the host encoder on every strip of the case
list, the coverage that list owes, the host writers' bytes after the split of tiff_write_u8, the three new symbols and the
``tiff_on_device`` key of ``make stat_fish`` on injected handles."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import yaml

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lzw_ref                               # noqa: E402
import test_stat_fish_aqua as cpu            # noqa: E402
import tiff_encode_cases as tc               # noqa: E402
from ecseg_amd import _lib, build, image_io  # noqa: E402
from ecseg_amd import stat_fish as sf        # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_ENCODED = {}


def encoded(case):
    """The restatement's strips of a case, computed once for the tests that need them."""
    if case.name not in _ENCODED:
        _ENCODED[case.name] = [lzw_ref.encode(s) for s in lzw_ref.strips(case.img, case.invert)]
    return _ENCODED[case.name]


def _host_encode(data):
    lib = _lib.load_library()
    src = np.frombuffer(data, np.uint8)
    dst = np.empty(2 * len(data) + 64, np.uint8)
    m = lib.ecseg_lzw_encode(src.ctypes.data_as(C.c_void_p), len(data), dst.ctypes.data_as(C.c_void_p), dst.size)
    assert m > 0
    return dst[:m].tobytes()


@pytest.mark.parametrize('case', tc.CASES, ids=[c.name for c in tc.CASES])
def test_the_restatement_equals_the_host_encoder_on_every_strip(case):
    raw = lzw_ref.strips(case.img, case.invert)
    H, line = case.img.shape[0], case.img.shape[1] * tc.spp(case)
    assert len(raw) == -(-H // lzw_ref.rows_per_strip(H, line)) and sum(len(s) for s in raw) == case.img.size
    for k, (s, e) in enumerate(zip(raw, encoded(case))):
        assert e.data == _host_encode(s), 'strip %d' % k


def test_the_case_list_covers_what_the_encoder_can_do():
    every = [e for case in tc.CASES for e in encoded(case)]
    restarts = {e.restarts for e in every}
    assert 0 in restarts and 1 in restarts and max(restarts) >= 2, restarts
    stepped = {e.eoi_width for e in every if e.last_stepped}
    assert stepped == {10, 11, 12}, 'last() steps the width to %s only' % sorted(stepped)
    assert any(e.restart_on_last_byte for e in every), 'no strip restarts its table on the last byte'
    assert any(e.odd for e in every) and any(not e.odd for e in every)
    assert {e.eoi_width for e in every} == {9, 10, 11, 12}
    # the named extents: one strip (offset inline in the IFD), a strip longer than 8192, more strips than the device has CUs
    counts = {case.name: len(encoded(case)) for case in tc.CASES}
    assert 1 in counts.values() and max(counts.values()) > 256
    assert any(len(s) > 8192 for case in tc.CASES for s in lzw_ref.strips(case.img, case.invert))
    assert any(case.invert for case in tc.CASES) and {tc.spp(case) for case in tc.CASES} == {1, 3}
    names = ' '.join(counts)
    for what in ('last_9_10', 'last_10_11', 'last_11_12', 'restart_last'):
        assert what in names, what


@pytest.mark.parametrize('case', tc.CASES, ids=[c.name for c in tc.CASES])
def test_the_file_writers_still_produce_their_bytes_after_the_split(case, tmp_path):
    """tiff_write_u8 now ends in the frame function it shares with the device path: the file is still the restatement's, and the
    gray one still that of the independent Python writer."""
    want = lzw_ref.tiff_file(case.img, case.invert, encoded(case))
    path = str(tmp_path / 'a.tif')
    if tc.spp(case) == 1:
        image_io.write_tiff_gray8(path, case.img, invert=case.invert)
        other = str(tmp_path / 'b.tif')
        image_io.write_tiff_gray8(other, case.img, invert=case.invert, native=False)
        assert open(other, 'rb').read() == want
    else:
        image_io.write_tiff_rgb8(path, case.img)
    assert open(path, 'rb').read() == want
    assert np.array_equal(image_io.imread(path), ~case.img if case.invert else case.img)


def test_header_binding_and_documents_of_the_new_symbols():
    hdr = open(os.path.join(ROOT, 'include', 'ecseg_hip.h')).read()
    assert 'long long ecseg_tiff_encode_bound(int H, int W, int spp);' in hdr
    assert 'int ecseg_tiff_encode(ecseg_ctx* h, const uint8_t* img, int H, int W, int spp, int invert, uint8_t* out' in hdr
    assert 'int ecseg_fish_render_tiff(ecseg_ctx* h, const uint8_t* img, int H, int W, int C, const int32_t* channels' in hdr
    assert 'still 5 - additive: ecseg_tiff_encode_bound' in hdr and '#define ECSEG_ABI_VERSION 6' in hdr and _lib.ABI_VERSION == 6
    lib = _lib.load_library()
    for name in ('ecseg_tiff_encode_bound', 'ecseg_tiff_encode', 'ecseg_fish_render_tiff'):
        assert name in _lib.EXPORTS and hasattr(lib, name), name
    assert hasattr(_lib.Handle, 'tiff_encode') and hasattr(_lib.Handle, 'fish_render_tiff') and hasattr(image_io, 'write_file_image')
    assert 'tiff_kernels.hip' in build.SOURCES
    for doc in ('DESIGN.md', 'README.md', 'INTEGRATION.md', 'EXPERIMENTS.md'):
        text = open(os.path.join(ROOT, doc)).read()
        assert 'tiff_on_device' in text and 'ecseg_tiff_encode' in text, doc
    assert '# tiff_on_device' in open(os.path.join(ROOT, 'config.yaml')).read()
    assert 'tiff_on_device' not in (yaml.safe_load(open(os.path.join(ROOT, 'config.yaml')))['stat_fish'])


def test_the_bound_holds_every_case_and_refuses_what_the_writers_refuse():
    lib = _lib.load_library()
    for case in tc.CASES:
        H, W = case.img.shape[:2]
        assert lib.ecseg_tiff_encode_bound(H, W, tc.spp(case)) >= len(lzw_ref.tiff_file(case.img, case.invert, encoded(case))), case.name
    for args in ((0, 5, 1), (5, 0, 1), (5, 5, 2), (5, 5, 4), (1, 1 << 30, 1), (1, (1 << 30) // 3 + 1, 3)):
        assert lib.ecseg_tiff_encode_bound(*args) == -1, args
    assert lib.ecseg_tiff_encode_bound(1, (1 << 30) - 1, 1) > 0


class TiffOracleHandle(cpu.RenderingOracleHandle):
    """A handle whose device TIFF calls are answered by the restatements tests/aqua_ref.py and tests/lzw_ref.py."""

    def tiff_encode(self, img, invert=False):
        self.calls.append(dict(tiff=np.asarray(img).shape))
        return lzw_ref.tiff_file(img, invert)

    def fish_render_tiff(self, img, channels, thresholded, boundaries):
        self.calls.append(dict(render_tiff=tuple(channels)))
        return tuple(lzw_ref.tiff_file(r) for r in self.fish_render(img, channels, thresholded, boundaries))


def _set_key(tmp_path, **keys):
    cfg = yaml.safe_load(open(tmp_path / 'config.yaml'))
    cfg['stat_fish'].update(keys)
    yaml.safe_dump(cfg, open(tmp_path / 'config.yaml', 'w'))


@pytest.mark.parametrize('value', ['yes', 1, 0, 'true', [True], None])
def test_a_value_that_is_no_boolean_is_a_configuration_error(tmp_path, monkeypatch, capsys, value):
    inp, _ = cpu.make_folder(tmp_path, kinds=(('one', 'tif'),), size=(40, 50), color_sensitivity=(70, 70))
    _set_key(tmp_path, tiff_on_device=value)
    monkeypatch.chdir(tmp_path)
    with pytest.raises(SystemExit) as e:
        sf.main([], handle=TiffOracleHandle())
    assert e.value.code == 2 and 'tiff_on_device must be true or false' in capsys.readouterr().out
    assert not os.path.exists(inp / 'annotated') and not [d for d in os.listdir(inp) if d.startswith('tmp_')]


def test_a_handle_without_the_two_calls_is_a_configuration_error(tmp_path, monkeypatch, capsys):
    inp, _ = cpu.make_folder(tmp_path, kinds=(('one', 'tif'),), size=(40, 50), color_sensitivity=(70, 70))
    _set_key(tmp_path, tiff_on_device=True)
    monkeypatch.chdir(tmp_path)
    for handle in (cpu.OracleHandle(), cpu.RenderingOracleHandle()):
        with pytest.raises(SystemExit) as e:
            sf.main([], handle=handle)
        assert e.value.code == 2 and 'tiff_encode, fish_render_tiff' in capsys.readouterr().out
        assert not os.path.exists(inp / 'annotated') and not handle.calls
    _set_key(tmp_path, tiff_on_device=False)                 # the same handles run with the key off
    sf.main([], handle=cpu.OracleHandle())
    assert os.path.isdir(inp / 'annotated')


def test_the_key_routes_every_tiff_through_the_two_calls_and_keeps_the_bytes(tmp_path, monkeypatch):
    inp, _ = cpu.make_folder(tmp_path, size=(40, 50))
    monkeypatch.chdir(tmp_path)
    off = TiffOracleHandle()
    sf.main([], handle=off)
    want = cpu.folder_bytes(inp / 'annotated')
    assert not [c for c in off.calls if 'tiff' in c or 'render_tiff' in c] and len([c for c in off.calls if 'render' in c]) == 3
    _set_key(tmp_path, tiff_on_device=True)
    on = TiffOracleHandle()
    sf.main([], handle=on)
    got = cpu.folder_bytes(inp / 'annotated')
    assert len([c for c in on.calls if 'render_tiff' in c]) == 3 and [c['tiff'] for c in on.calls if 'tiff' in c] == [(40, 50)] * 3
    assert sorted(got) == sorted(want) and len(want) == 3 * 5 + 2
    for name in want:
        assert got[name] == want[name], name
