"""The device TIFF reader (csrc/tiff_decode_kernels.hip) on the device.  Every expected value is the host reader's
(ecseg_tiff_info + ecseg_tiff_read on the same bytes) or a committed fixture, never the device's: the case list of the encoder's
tests written by the host writers, the golden files of tifffile / libtiff, the OpenCV-written example, the tolerated streams and
the corrupt corpus of tests/tiff_decode_cases.py (the corpus tests/test_tiff_decode.py runs through the sanitizer program on the
CPU), and ``make stat_fish`` with and without ``tiff_read_on_device``."""
import base64
import ctypes as C
import json
import os
import sys

import numpy as np
import pytest
import yaml

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_stat_fish_aqua as cpu            # noqa: E402
import tiff_decode_cases as dc               # noqa: E402
import tiff_encode_cases as tc               # noqa: E402
from ecseg_amd import image_io               # noqa: E402
from ecseg_amd import stat_fish as sf        # noqa: E402
from ecseg_amd._lib import EcsegError, load_library   # noqa: E402

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
LEFT_TO_THE_HOST = ('rgb8_deflate', 'rgb16_deflate_pred', 'gray8_strips5_deflate_pred', 'rgb8_tiled16', 'gray16_tiled32_pred', 'gray8_packbits',
                    'rgb8_bigtiff')
_HOST = {}


def host_read(data, tmp_path):
    """What the host's native reader makes of the bytes: the array, or 'invalid'."""
    path = str(tmp_path / 'host.tif')
    image_io.write_file_image(path, data)
    try:
        a = image_io._native_tiff(path)
    except image_io.TiffError:
        return 'invalid'
    assert a is not None
    return a


def device_read(gpu, data):
    try:
        return gpu.tiff_decode(data)
    except EcsegError as e:
        assert e.code == -1, e
        return 'invalid'


def same(a, b):
    if isinstance(a, str) or isinstance(b, str):
        return isinstance(a, str) and isinstance(b, str) and a == b
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b)


def case_file(case, tmp_path_factory):
    """(file bytes, host reader's samples) of a case of the encoder's list, written by the host writer, once."""
    if case.name not in _HOST:
        path = str(tmp_path_factory.mktemp('case') / 'h.tif')
        if tc.spp(case) == 1:
            image_io.write_tiff_gray8(path, case.img, invert=case.invert)
        else:
            image_io.write_tiff_rgb8(path, case.img)
        _HOST[case.name] = (open(path, 'rb').read(), image_io._native_tiff(path))
    return _HOST[case.name]


def _case(name):
    return next(c for c in tc.CASES if name in c.name)


@pytest.mark.parametrize('case', tc.CASES, ids=[c.name for c in tc.CASES])
def test_every_case_of_the_encoders_list_decodes_to_the_host_readers_samples(gpu, case, tmp_path_factory):
    data, want = case_file(case, tmp_path_factory)
    got = gpu.tiff_decode(data)
    assert got is not None and same(got, want)
    assert np.array_equal(want, ~case.img if case.invert else case.img)
    assert 0 < gpu.timings()['count'] < 10000
    assert same(gpu.tiff_decode(data), want), 'a second call gives other samples'


def test_the_golden_files_by_layout(gpu, tmp_path):
    files = json.load(open(os.path.join(GOLDEN, 'io_tiff_files.json')))['files']
    pixels = np.load(os.path.join(GOLDEN, 'io_tiff_pixels.npz'))
    assert set(LEFT_TO_THE_HOST) < set(files)
    on_device = 0
    for name, b64 in sorted(files.items()):
        data = base64.b64decode(b64)
        got = gpu.tiff_decode(data)
        if name in LEFT_TO_THE_HOST:
            assert got is None, name
        else:
            assert got is not None and same(got, pixels[name]), name
            on_device += 1
        path = str(tmp_path / (name + '.tif'))
        image_io.write_file_image(path, data)
        assert same(image_io.imread(path, handle=gpu), pixels[name]), name
    assert on_device == len(files) - len(LEFT_TO_THE_HOST) == 7       # raw, big-endian 16-bit, libtiff's LZW with and without predictor


def test_the_opencv_written_example_of_208_strips(gpu):
    path = os.path.join(GOLDEN, 'dapi_example.tif')
    want = image_io._native_tiff(path)
    assert want.shape == (1040, 1392)
    assert same(gpu.tiff_decode(open(path, 'rb').read()), want) and same(image_io.imread(path, handle=gpu), want)


def test_imread_sends_a_file_of_1040_strips_to_the_device_and_keeps_one_of_1039(gpu, tmp_path):
    class Counting:
        def __init__(self):
            self.calls = 0

        def tiff_decode(self, data):
            self.calls += 1
            return gpu.tiff_decode(data)

    rows = np.random.default_rng(5).integers(0, 4, (1040, 8), dtype=np.uint8)
    for n, sent in ((1040, 1), (1039, 0)):
        data = dc.tiff_file([dc.pack(dc.lzw_codes(r.tobytes())) for r in rows[:n]], n, 8, 1)
        path = str(tmp_path / ('%d.tif' % n))
        image_io.write_file_image(path, data)
        handle = Counting()
        assert same(image_io.imread(path, handle=handle), rows[:n]) and handle.calls == sent, n
        assert same(gpu.tiff_decode(data), image_io._native_tiff(path))


@pytest.mark.parametrize('name', [name for name, _ in dc.tolerated_files()])
def test_tolerated_streams_give_what_the_host_decoder_gives(gpu, tmp_path, name):
    data = dict(dc.tolerated_files())[name]
    want = host_read(data, tmp_path)
    assert not isinstance(want, str), 'the host refuses a stream this list calls tolerated'
    assert same(device_read(gpu, data), want)


def test_a_strip_offset_behind_the_file_is_invalid(gpu, tmp_path):
    data = dc.offset_behind_the_file()
    assert host_read(data, tmp_path) == 'invalid'
    with pytest.raises(EcsegError) as e:
        gpu.tiff_decode(data)
    assert e.value.code == -1 and 'behind the end of the file' in str(e.value)


def test_the_corrupt_corpus_has_the_hosts_status_and_bytes(gpu, tmp_path, tmp_path_factory):
    """200 seeded truncations and single-bit flips; the same files pass the sanitizer program in tests/test_tiff_decode.py."""
    corpus = dc.corrupt_corpus()
    assert len(corpus) == 200
    invalid = 0
    for name, data in corpus:
        want = host_read(data, tmp_path)
        assert same(device_read(gpu, data), want), name
        invalid += isinstance(want, str)
    assert 0 < invalid < 200
    whole, want = case_file(_case('gray_31x257'), tmp_path_factory)
    assert same(gpu.tiff_decode(whole), want), 'the handle is of no use after corrupt files'


def test_one_handle_a_large_file_a_small_one_and_the_large_one_again(gpu, tmp_path_factory):
    for case in (_case('gray_300x4097'), _case('gray_3x1'), _case('gray_300x4097'), _case('rgb_5x7'), _case('gray_300x4097')):
        data, want = case_file(case, tmp_path_factory)
        assert same(gpu.tiff_decode(data), want), case.name


def test_the_c_entry_point_reports_the_shape_and_refuses_a_short_destination(gpu, tmp_path_factory):
    lib = load_library()
    for case in (_case('gray_31x257'), _case('rgb_5x7')):
        data, want = case_file(case, tmp_path_factory)
        buf = np.frombuffer(data, np.uint8)
        H, W, spp, bits = C.c_int(), C.c_int(), C.c_int(), C.c_int()
        shape = (C.byref(H), C.byref(W), C.byref(spp), C.byref(bits))
        vp = lambda a: a.ctypes.data_as(C.c_void_p)
        assert lib.ecseg_tiff_decode(gpu.h, vp(buf), buf.size, None, 0, *shape) == 0
        assert (H.value, W.value, spp.value, bits.value) == (want.shape[0], want.shape[1], tc.spp(case), 8)
        out = np.full(want.size + 16, 0xa5, np.uint8)
        assert lib.ecseg_tiff_decode(gpu.h, vp(buf), buf.size, vp(out), want.size - 1, *shape) == -1
        assert 'fewer bytes' in lib.ecseg_last_error(gpu.h).decode() and (out == 0xa5).all(), 'a destination one byte short was written'
        assert lib.ecseg_tiff_decode(gpu.h, vp(buf), buf.size, vp(out), want.size, *shape) == 0
        assert np.array_equal(out[:want.size], want.reshape(-1)) and (out[want.size:] == 0xa5).all()
        assert lib.ecseg_tiff_decode(gpu.h, None, buf.size, vp(out), want.size, *shape) == -1
        assert lib.ecseg_tiff_decode(gpu.h, vp(buf), 7, vp(out), want.size, *shape) == -1       # not a TIFF


def _three_strips_one_flipped(k, at=9):
    """An 8-pixel-wide LZW file of three one-row strips, bit ``at`` of strip k flipped as the corrupt corpus flips one: bit 9 is the
    top bit of the first code behind the ClearCode, which then names an entry the fresh table does not have."""
    rows = np.random.default_rng(9).integers(0, 256, (3, 8), dtype=np.uint8)
    strips = [bytearray(dc.pack(dc.lzw_codes(r.tobytes()))) for r in rows]
    strips[k][at >> 3] ^= 0x80 >> (at & 7)
    return dc.tiff_file([bytes(s) for s in strips], 3, 8, 1)


@pytest.mark.parametrize('k', (1, 2))
def test_a_corrupt_strip_is_named_and_the_destination_is_not_written(gpu, tmp_path, k):
    data = _three_strips_one_flipped(k)
    assert host_read(data, tmp_path) == 'invalid'
    with pytest.raises(EcsegError) as e:
        gpu.tiff_decode(data)
    assert e.value.code == -1 and 'strip %d holds a corrupt LZW stream' % k in str(e.value)
    lib = load_library()
    buf = np.frombuffer(data, np.uint8)
    H, W, spp, bits = C.c_int(), C.c_int(), C.c_int(), C.c_int()
    out = np.full(24 + 16, 0xa5, np.uint8)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    assert lib.ecseg_tiff_decode(gpu.h, vp(buf), buf.size, vp(out), 24, C.byref(H), C.byref(W), C.byref(spp), C.byref(bits)) == -1
    assert 'tiff_decode: strip %d holds a corrupt LZW stream' % k in lib.ecseg_last_error(gpu.h).decode()
    assert (H.value, W.value, spp.value, bits.value) == (3, 8, 1, 8) and (out == 0xa5).all(), 'a corrupt file reached the destination'


def test_a_call_that_only_measures_or_refuses_leaves_every_stage_timer_at_zero(gpu, tmp_path_factory):
    lib = load_library()
    data, want = case_file(_case('gray_3x1'), tmp_path_factory)
    buf = np.frombuffer(data, np.uint8)
    H, W, spp, bits = C.c_int(), C.c_int(), C.c_int(), C.c_int()
    shape = (C.byref(H), C.byref(W), C.byref(spp), C.byref(bits))
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    out = np.zeros(want.size, np.uint8)
    for refusing in (False, True):
        assert same(gpu.tiff_decode(data), want) and gpu.timings()['count'] > 0
        if refusing:
            assert lib.ecseg_tiff_decode(gpu.h, vp(buf), 7, vp(out), out.size, *shape) == -1       # not a TIFF
        else:
            assert lib.ecseg_tiff_decode(gpu.h, vp(buf), buf.size, None, 0, *shape) == 0
            assert (H.value, W.value, spp.value, bits.value) == (want.shape[0], want.shape[1], 1, 8)
        assert all(v == 0 for v in gpu.timings().values()), (refusing, gpu.timings())


def test_make_stat_fish_writes_the_same_bytes_with_the_key_absent_on_and_off(gpu, tmp_path, monkeypatch, capsys):
    """Three- and four-channel images, the min-cut picture included: every file and the CSV; then both device keys at once."""
    inp, _ = cpu.make_folder(tmp_path, size=(67, 93))

    def run(**keys):
        cfg = yaml.safe_load(open(tmp_path / 'config.yaml'))
        cfg['stat_fish'].update(use_min_cut=True, **keys)
        cfg['stat_fish'] = {k: v for k, v in cfg['stat_fish'].items() if v is not None}
        yaml.safe_dump(cfg, open(tmp_path / 'config.yaml', 'w'))
        sf.main([], handle=gpu)
        return cpu.folder_bytes(inp / 'annotated'), capsys.readouterr().out

    monkeypatch.chdir(tmp_path)
    want, said = run()
    runs = dict(on=run(tiff_read_on_device=True), off=run(tiff_read_on_device=False), both=run(tiff_read_on_device=True, tiff_on_device=True))
    assert len(want) == 3 * 6 + 2 and 'stat_fish_lsq.csv' in want         # the count of tests/test_gpu_tiff_encode.py
    for name, (got, out) in runs.items():
        assert sorted(got) == sorted(want), name
        for f in want:
            assert got[f] == want[f], (name, f)
        assert out == said, name
