"""The device gray-channel PNG coder (csrc/png_gray_kernels.hip) on the device: every case of tests/png_gray_cases.py against the file
the host writer puts on disk, byte for byte, and - independently of the host writer - against zlib and the input channel; repeats;
the capacity protocol; bad arguments."""
import ctypes as C
import os
import struct
import sys
import zlib

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import png_gray_cases as gc                  # noqa: E402
from ecseg_amd import image_io               # noqa: E402
from ecseg_amd._lib import EcsegError, load_library   # noqa: E402

pytestmark = pytest.mark.gpu
_HOST = {}


def host_files(name, px, channel, invert, tmp_path_factory):
    """The files the host writer puts on disk, written once per case for the tests that need them."""
    if name not in _HOST:
        d = tmp_path_factory.mktemp('host')
        out = []
        for i in range(px.shape[0]):
            image_io.write_png_channel(str(d / ('%d.png' % i)), px[i], channel, invert=bool(invert))
            out.append(open(d / ('%d.png' % i), 'rb').read())
        _HOST[name] = out
    return _HOST[name]


def _first_difference(got, want):
    return next((i for i, (a, b) in enumerate(zip(got, want)) if a != b), min(len(got), len(want)))


def unpack(file, H, W):
    """a gray PNG of one IDAT chunk -> (the channel its stream inflates and un-SUBs to, the stream's stored Adler-32, that of its bytes)"""
    assert file[:8] == b'\x89PNG\r\n\x1a\n' and file[12:16] == b'IHDR' and struct.unpack('>II', file[16:24]) == (W, H)
    assert file[24:29] == bytes([8, 0, 0, 0, 0]) and file[37:41] == b'IDAT' and file[-12:] == b'\0\0\0\0IEND\xaeB`\x82'
    n, = struct.unpack('>I', file[33:37])
    z = file[41:41 + n]
    assert len(file) == 41 + n + 4 + 12 and struct.unpack('>I', file[41 + n:45 + n])[0] == zlib.crc32(file[37:41 + n])
    rows = np.frombuffer(zlib.decompress(z), np.uint8).reshape(H, W + 1)
    assert (rows[:, 0] == 1).all()
    return np.cumsum(rows[:, 1:].astype(np.uint64), axis=1).astype(np.uint8), struct.unpack('>I', z[-4:])[0], zlib.adler32(rows.tobytes())


@pytest.mark.parametrize('case', gc.CASES, ids=gc.IDS)
def test_the_device_file_is_the_host_file_and_inflates_to_the_channel(gpu, case, tmp_path_factory):
    name, px, channel, invert = case
    n, H, W, _ = px.shape
    want = host_files(name, px, channel, invert, tmp_path_factory)
    got = gpu.png_channel_encode(px, channel, invert=bool(invert))
    assert isinstance(got, list) and len(got) == n
    for i in range(n):
        assert isinstance(got[i], bytes) and len(got[i]) == len(want[i]), (i, len(got[i]), len(want[i]))
        assert got[i] == want[i], 'image %d: first difference at byte %d of %d' % (i, _first_difference(got[i], want[i]), len(want[i]))
        chan, stored, computed = unpack(got[i], H, W)
        assert np.array_equal(chan, px[i, ..., channel] ^ np.uint8(255 if invert else 0)) and stored == computed
    assert gpu.last_file_bytes == [len(w) for w in want]
    assert 0 < gpu.timings()['count'] < 10000
    assert gpu.png_channel_encode(px, channel, invert=bool(invert)) == got, 'a second call gives other bytes'
    assert gpu.png_channel_encode(px[0], channel, invert=bool(invert)) == got[0]       # one image: the file itself


def test_one_handle_runs_a_large_case_a_small_one_and_the_large_one_again(gpu, tmp_path_factory):
    by_name = {c[0]: c for c in gc.CASES}
    large = next(k for k in gc.IDS if k.startswith('speckle_70x255'))
    small = next(k for k in gc.IDS if k.startswith('noise_1x1'))
    for name in (large, small, large):
        _, px, channel, invert = by_name[name]
        assert gpu.png_channel_encode(px, channel, invert=bool(invert)) == host_files(name, px, channel, invert, tmp_path_factory), name


def test_a_capacity_one_byte_short_drops_that_file_only_and_reports_its_size(gpu, tmp_path_factory):
    name = next(k for k in gc.IDS if k.startswith('fish_33x200'))
    _, px, channel, invert = {c[0]: c for c in gc.CASES}[name]
    assert px.shape[0] == 3
    # image 1 is to be the one that does not fit: full-range noise gives it the largest file
    px = px.copy()
    px[1, :, :, channel] = np.random.default_rng(5).integers(0, 256, px.shape[1:3], dtype=np.uint8)
    want = host_files(name + '_capacity', px, channel, invert, tmp_path_factory)
    assert len(want[1]) > max(len(want[0]), len(want[2]))
    cap = len(want[1]) - 1
    got = gpu.png_channel_encode(px, channel, invert=bool(invert), capacity=cap)
    assert got[1] is None and gpu.last_file_bytes[1] == -len(want[1])
    assert got[0] == want[0] and got[2] == want[2] and gpu.last_file_bytes[0] == len(want[0]) and gpu.last_file_bytes[2] == len(want[2])
    assert gpu.png_channel_encode(px, channel, invert=bool(invert), capacity=cap + 1) == want     # exactly enough is enough
    # nothing of the file that does not fit is written, and nothing lands behind a file that does
    lib = load_library()
    n, H, W, Cc = px.shape
    buf = np.full(n * cap + 64, 0xa5, np.uint8)
    ptrs = (C.c_void_p * n)(*[buf.ctypes.data + i * cap for i in range(n)])
    out = (C.c_longlong * n)()
    assert lib.ecseg_png_channel_encode(gpu.h, px.ctypes.data_as(C.c_void_p), n, H, W, Cc, channel, invert, ptrs, cap, out) == 0
    for i in range(n):
        slot = buf[i * cap:(i + 1) * cap]
        if i == 1:
            assert out[i] == -len(want[i]) and (slot == 0xa5).all(), 'bytes of a file that does not fit were written'
        else:
            assert out[i] == len(want[i]) and slot[:out[i]].tobytes() == want[i] and (slot[out[i]:] == 0xa5).all()
    assert (buf[n * cap:] == 0xa5).all()


def test_the_default_capacity_is_the_bound_and_holds_full_range_noise(gpu, tmp_path_factory):
    px = np.random.default_rng(11).integers(0, 256, (1, 33, 200, 3), dtype=np.uint8)
    want = host_files('full_range_noise', px, 2, 0, tmp_path_factory)
    assert gpu.png_channel_encode(px, 2) == want
    assert len(want[0]) <= load_library().ecseg_png_channel_bound(33, 200)


def test_bad_arguments_are_refused(gpu):
    lib = load_library()
    px = np.zeros((2, 4, 4, 3), np.uint8)
    buf = np.zeros(2 * 4096, np.uint8)
    ptrs = (C.c_void_p * 2)(buf.ctypes.data, buf.ctypes.data + 4096)
    holes = (C.c_void_p * 2)(buf.ctypes.data, None)
    out = (C.c_longlong * 2)()
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    call = lib.ecseg_png_channel_encode
    assert call(gpu.h, vp(px), 2, 4, 4, 3, 0, 0, ptrs, 4096, out) == 0 and out[0] > 0 and out[1] == out[0]
    for n, H, W, Cc, ch in ((2, 0, 4, 3, 0), (2, 4, 0, 3, 0), (-1, 4, 4, 3, 0), (65536, 4, 4, 3, 0), (2, 4, 4, 3, 3), (2, 4, 4, 3, -1), (2, 4, 4, 0, 0)):
        assert call(gpu.h, vp(px), n, H, W, Cc, ch, 0, ptrs, 4096, out) == -1, (n, H, W, Cc, ch)
        assert 'bad arguments' in lib.ecseg_last_error(gpu.h).decode()
    assert call(gpu.h, None, 2, 4, 4, 3, 0, 0, ptrs, 4096, out) == -1
    assert call(gpu.h, vp(px), 2, 4, 4, 3, 0, 0, None, 4096, out) == -1
    assert call(gpu.h, vp(px), 2, 4, 4, 3, 0, 0, ptrs, 4096, None) == -1
    assert call(gpu.h, vp(px), 2, 4, 4, 3, 0, 0, holes, 4096, out) == -1
    assert call(gpu.h, vp(px), 2, 4, 4, 3, 0, 0, ptrs, 0, out) == -1
    assert call(None, vp(px), 2, 4, 4, 3, 0, 0, ptrs, 4096, out) == -1
    assert call(gpu.h, vp(px), 0, 4, 4, 3, 0, 0, ptrs, 4096, out) == 0                 # no image: nothing to do
    with pytest.raises(ValueError):
        gpu.png_channel_encode(np.zeros((0, 4, 3), np.uint8), 0)
    with pytest.raises(EcsegError) as e:
        gpu.png_channel_encode(px, 0, capacity=0)
    assert e.value.code == -1
