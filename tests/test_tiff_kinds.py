"""The kinds word of the device TIFF reader, without a GPU: the four handle-free routing functions against the answers that the
`_ex3` family gave on the commit before the word (tests/golden/tiff_kinds_answers.json, written there by
tools/record_tiff_kinds_answers.py) on every file of tests/tiff_kinds_cases.py and all 8 words; stray bits; the Python names of the
bits against the header's; and the one context manager that sets the three handle options for a while."""
import json
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import tiff_kinds_cases as kc                # noqa: E402
from ecseg_amd import _lib                   # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _ptr(a):
    import ctypes as C
    return a.ctypes.data_as(C.c_void_p)


def _answers(lib, data, kinds):
    """[routes, counts, set routes of the file taken twice, arena bytes of the file alone]: the row the recording keeps per word"""
    one = np.frombuffer(data, np.uint8)
    two = np.concatenate([one, one])
    r1, r2 = np.array([[0, one.size]], np.int64), np.array([[0, one.size], [one.size, one.size]], np.int64)
    return [lib.ecseg_tiff_decode_routes(_ptr(one), one.size, kinds), lib.ecseg_tiff_decode_batch_counts(_ptr(one), one.size, kinds),
            lib.ecseg_tiff_decode_batch_routes(_ptr(two), two.size, _ptr(r2), 2, kinds), lib.ecseg_tiff_decode_batch_bytes(_ptr(one), one.size, _ptr(r1), 1, kinds)]


@pytest.fixture(scope='module')
def files():
    return kc.all_files()


def test_the_four_functions_answer_every_word_as_the_suffixed_functions_did(files):
    lib = _lib.load_library()
    with open(kc.ANSWERS) as f:
        recorded = json.load(f)
    assert sorted(recorded) == sorted(name for name, _ in files) and len(files) > 700
    assert all(len(rows) == 8 and all(len(r) == 4 and all(type(v) is int for v in r) for r in rows) for rows in recorded.values())
    seen = set()
    for name, data in files:
        for kinds in kc.WORDS:
            got = _answers(lib, data, kinds)
            assert got == recorded[name][kinds], (name, kinds, got, recorded[name][kinds])
            seen.add((kinds, tuple(got[:3])))
    # the recording is no row of zeros: each rule says yes somewhere, with and without Deflate, and every word takes some file another leaves
    assert {(0, (1, 1, 1)), (1, (1, 1, 1)), (1, (0, 1, 1)), (1, (0, 1, 0))} <= seen
    arenas = {kinds: [recorded[name][kinds][3] for name, _ in files] for kinds in kc.WORDS}
    assert len({tuple(v) for v in arenas.values()}) == 8


def test_a_word_with_a_stray_bit_is_a_bad_argument(files):
    lib = _lib.load_library()
    picks = [data for name, data in files if name in ('strips/c5_n3000', 'strips/c8_n3000', 'io/rgb8_tiled16', 'packbits/literal_run_of_128')]
    assert len(picks) == 4
    for data in picks:
        assert _answers(lib, data, 0)[3] > 0
        for kinds in (8, 0x80000000, 8 | 1, 0x80000000 | 7, 0xfffffff8):
            assert _answers(lib, data, kinds) == [0, 0, 0, -1], kinds
    none = np.zeros((0, 2), np.int64)                        # also where no file is asked about: the word is judged first
    assert lib.ecseg_tiff_decode_batch_bytes(None, 0, _ptr(none), 0, 8) == -1
    assert lib.ecseg_tiff_decode_batch_bytes(None, 0, _ptr(none), 0, 7) == 0


def test_the_python_names_of_the_bits_are_the_headers():
    hdr = open(os.path.join(ROOT, 'include', 'ecseg_hip.h')).read()
    defines = {name: int(value) for name, value in re.findall(r'#define (ECSEG_TIFF_\w+)\s+(\d+)u', hdr)}
    assert sorted(defines) == ['ECSEG_TIFF_DEFLATE', 'ECSEG_TIFF_PACKBITS', 'ECSEG_TIFF_TILED']
    assert (_lib.TIFF_DEFLATE, _lib.TIFF_TILED, _lib.TIFF_PACKBITS) == (defines['ECSEG_TIFF_DEFLATE'], defines['ECSEG_TIFF_TILED'], defines['ECSEG_TIFF_PACKBITS'])
    assert _lib.tiff_kinds() == 0
    for d in (False, True):
        for t in (False, True):
            for p in (False, True):
                want = d * defines['ECSEG_TIFF_DEFLATE'] | t * defines['ECSEG_TIFF_TILED'] | p * defines['ECSEG_TIFF_PACKBITS']
                assert _lib.tiff_kinds(deflate=d, tiled=t, packbits=p) == _lib.tiff_kinds(d, t, p) == want
    assert sorted(bit for _, _, bit in _lib.TIFF_OPTIONS) == sorted(defines.values())
    assert isinstance(_lib.Handle.tiff_kinds, property) and '#define ECSEG_ABI_VERSION 6' in hdr and _lib.ABI_VERSION == 6
    bound = [n for n in _lib.EXPORTS if re.fullmatch(r'ecseg_tiff_decode_\w*(routes|counts|bytes)\w*', n)]
    assert sorted(bound) == ['ecseg_tiff_decode_batch_bytes', 'ecseg_tiff_decode_batch_counts', 'ecseg_tiff_decode_batch_routes', 'ecseg_tiff_decode_routes']


# ---- the context manager --------------------------------------------------------------------------------------------------------------
class RecordingHandle:
    """Anything with ``set_option`` and the three mirror attributes, as the fakes of the other tests have them."""

    def __init__(self, **on):
        self.calls = []
        for key, value in on.items():
            setattr(self, key, value)

    def set_option(self, key, value):
        self.calls.append((key, value))
        setattr(self, key, bool(value))


def test_an_option_that_is_already_on_is_not_touched_and_stays_on():
    h = RecordingHandle(tiff_tiled_on_device=True)
    with _lib.tiff_options(h, tiled=True):
        assert h.tiff_tiled_on_device and _lib.handle_tiff_kinds(h) == _lib.TIFF_TILED
    assert h.calls == [] and h.tiff_tiled_on_device is True
    with _lib.tiff_options(h, deflate=True, tiled=True, packbits=True):
        assert _lib.handle_tiff_kinds(h) == 7
    assert h.calls == [('tiff_deflate_on_device', 1), ('tiff_packbits_on_device', 1), ('tiff_deflate_on_device', 0), ('tiff_packbits_on_device', 0)]
    assert h.tiff_tiled_on_device is True and _lib.handle_tiff_kinds(h) == _lib.TIFF_TILED


def test_an_option_turned_on_is_turned_off_on_exit_also_when_the_body_raises():
    h = RecordingHandle()
    with _lib.tiff_options(h, packbits=True):
        assert h.calls == [('tiff_packbits_on_device', 1)] and h.tiff_packbits_on_device
    assert h.calls == [('tiff_packbits_on_device', 1), ('tiff_packbits_on_device', 0)] and not h.tiff_packbits_on_device
    del h.calls[:]
    with pytest.raises(KeyError):
        with _lib.tiff_options(h, deflate=True, tiled=True):
            assert _lib.handle_tiff_kinds(h) == _lib.TIFF_DEFLATE | _lib.TIFF_TILED
            raise KeyError('from the body')
    assert h.calls == [('tiff_deflate_on_device', 1), ('tiff_tiled_on_device', 1), ('tiff_deflate_on_device', 0), ('tiff_tiled_on_device', 0)]
    assert _lib.handle_tiff_kinds(h) == 0
    del h.calls[:]
    h.set_option('tiff_deflate_on_device', 1)                # and one turned off for the body comes back on
    with _lib.tiff_options(h, deflate=False):
        assert not h.tiff_deflate_on_device
    assert h.calls == [('tiff_deflate_on_device', 1), ('tiff_deflate_on_device', 0), ('tiff_deflate_on_device', 1)] and h.tiff_deflate_on_device


def test_none_touches_nothing_and_needs_no_set_option():
    h = RecordingHandle(tiff_deflate_on_device=True)
    with _lib.tiff_options(h):
        pass
    with _lib.tiff_options(h, deflate=None, tiled=None, packbits=None):
        pass
    assert h.calls == [] and h.tiff_deflate_on_device is True
    with _lib.tiff_options(object()):                        # a handle without options, when no kind is asked for
        pass
    assert _lib.Handle.tiff_options is _lib.tiff_options, 'one context manager: the method is the function'
    assert not hasattr(_lib.Handle, '_deflate_option')
