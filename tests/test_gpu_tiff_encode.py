"""The device TIFF encoder (csrc/tiff_kernels.hip) on the device: every case of tests/tiff_encode_cases.py against the file the
host writers put on disk, byte for byte; ecseg_fish_render_tiff against the host-written files of ecseg_fish_render's rasters;
``make stat_fish`` with and without ``tiff_on_device``."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import yaml

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_stat_fish_aqua as cpu            # noqa: E402
import tiff_encode_cases as tc               # noqa: E402
from ecseg_amd import image_io               # noqa: E402
from ecseg_amd import stat_fish as sf        # noqa: E402
from ecseg_amd._lib import EcsegError, load_library   # noqa: E402

pytestmark = pytest.mark.gpu
_HOST = {}


def host_file(case, tmp_path_factory):
    """The file the host writer puts on disk for a case, written once for the tests that need it."""
    if case.name not in _HOST:
        path = str(tmp_path_factory.mktemp('host') / 'h.tif')
        if tc.spp(case) == 1:
            image_io.write_tiff_gray8(path, case.img, invert=case.invert)
        else:
            image_io.write_tiff_rgb8(path, case.img)
        _HOST[case.name] = open(path, 'rb').read()
    return _HOST[case.name]


def _case(name):
    return next(c for c in tc.CASES if name in c.name)


def _native_read(path, shape):
    lib = load_library()
    H, W, spp, bits = C.c_int(), C.c_int(), C.c_int(), C.c_int()
    assert lib.ecseg_tiff_info(os.fsencode(path), C.byref(H), C.byref(W), C.byref(spp), C.byref(bits)) == 0
    assert (H.value, W.value, spp.value, bits.value) == (shape[0], shape[1], shape[2] if len(shape) == 3 else 1, 8)
    out = np.empty(shape, np.uint8)
    assert lib.ecseg_tiff_read(os.fsencode(path), out.ctypes.data_as(C.c_void_p), out.size) == 0
    return out


@pytest.mark.parametrize('case', tc.CASES, ids=[c.name for c in tc.CASES])
def test_the_device_file_is_the_host_file(gpu, case, tmp_path, tmp_path_factory):
    want = host_file(case, tmp_path_factory)
    got = gpu.tiff_encode(case.img, invert=case.invert)
    assert isinstance(got, bytes) and len(got) == len(want), (len(got), len(want))
    assert got == want, 'first difference at byte %d of %d' % (next(i for i, (a, b) in enumerate(zip(got, want)) if a != b), len(want))
    assert 0 < gpu.timings()['count'] < 10000
    path = str(tmp_path / 'd.tif')
    image_io.write_file_image(path, got)
    assert np.array_equal(_native_read(path, case.img.shape), ~case.img if case.invert else case.img)
    assert gpu.tiff_encode(case.img, invert=case.invert) == got, 'a second call gives other bytes'


def test_one_handle_runs_a_large_case_a_small_one_and_the_large_one_again(gpu, tmp_path_factory):
    large, small = _case('gray_300x4097'), _case('gray_3x1')
    for case in (large, small, large, _case('rgb_5x7'), large):
        assert gpu.tiff_encode(case.img, invert=case.invert) == host_file(case, tmp_path_factory), case.name


def test_too_small_a_capacity_is_an_error_never_a_truncated_file(gpu, tmp_path_factory):
    lib = load_library()
    for case in (_case('gray_31x257'), _case('rgb_5x7'), _case('gray_1x1')):
        want = host_file(case, tmp_path_factory)
        H, W = case.img.shape[:2]
        assert lib.ecseg_tiff_encode_bound(H, W, tc.spp(case)) >= len(want)
        for cap in (len(want) - 1, 8, 0):
            out = np.full(len(want) + 16, 0xa5, np.uint8)
            n = C.c_longlong(-7)
            rc = lib.ecseg_tiff_encode(gpu.h, case.img.ctypes.data_as(C.c_void_p), H, W, tc.spp(case), 0, out.ctypes.data_as(C.c_void_p), cap, C.byref(n))
            assert rc == -1 and 'does not fit' in lib.ecseg_last_error(gpu.h).decode() and n.value == 0, (case.name, cap)
            assert (out == 0xa5).all(), 'bytes were written into a buffer that is too small'
            with pytest.raises(EcsegError) as e:
                gpu.tiff_encode(case.img, capacity=cap)
            assert e.value.code == -1
        assert gpu.tiff_encode(case.img, capacity=len(want)) == want       # exactly enough is enough
    img = np.zeros((4, 4), np.uint8)
    out = np.zeros(4096, np.uint8)
    n = C.c_longlong()
    for args in ((0, 4, 1), (4, 0, 1), (4, 4, 2), (4, 4, 4)):
        assert lib.ecseg_tiff_encode(gpu.h, img.ctypes.data_as(C.c_void_p), args[0], args[1], args[2], 0, out.ctypes.data_as(C.c_void_p), 4096, C.byref(n)) == -1
    assert lib.ecseg_tiff_encode(gpu.h, None, 4, 4, 1, 0, out.ctypes.data_as(C.c_void_p), 4096, C.byref(n)) == -1
    assert gpu.tiff_encode(img) == host_file(tc.Case('zeros_4x4', img, False), tmp_path_factory)


@pytest.mark.parametrize('C_', [3, 4])
@pytest.mark.parametrize('size', [(5, 7), (67, 93), (3, 2731)])
def test_fish_render_tiff_equals_the_host_written_files_of_fish_render(gpu, tmp_path, size, C_):
    H, W = size
    rng = np.random.default_rng(H * 1000 + W + C_)
    I = rng.integers(0, 256, (H, W, C_), dtype=np.uint8)
    I[H // 2:] //= 16                                        # a flat half: long matches beside the noise
    if C_ == 4:
        I[..., 3].flat[::3] = cpu.Q_GREEN
        I[..., 3].flat[1::3] = cpu.Q_RED
    thr = (rng.random((H, W, C_ - 1)) < 0.4).astype(np.uint8) * np.uint8(255)
    bnd = (rng.random((H, W)) < 0.3).astype(np.uint8) * np.uint8(255)
    channels = (2, 1, 0) if C_ == 3 else (2, 1, 0, 3)
    rasters = gpu.fish_render(I, channels, thr, bnd)
    files = gpu.fish_render_tiff(I, channels, thr, bnd)
    assert len(files) == 3 and 0 < gpu.timings()['count'] < 10000
    for k, (r, f) in enumerate(zip(rasters, files)):
        path = str(tmp_path / ('%d.tif' % k))
        image_io.write_tiff_rgb8(path, r)
        assert f == open(path, 'rb').read(), 'file %d' % k
    again, raw = gpu.fish_render_tiff(I, channels, thr, bnd, want_rasters=True)
    assert again == files and all(np.array_equal(a, b) for a, b in zip(raw, rasters))


def test_fish_render_tiff_refuses_what_fish_render_refuses_and_a_small_capacity(gpu):
    H, W = 6, 9
    bnd = np.zeros((H, W), np.uint8)
    with pytest.raises(EcsegError) as e:
        gpu.fish_render_tiff(np.zeros((H, W, 4), np.uint8), (0, 1, 2, 3), np.zeros((H, W, 2), np.uint8), bnd)
    assert e.value.code == -1 and 'n_probe' in str(e.value)
    with pytest.raises(EcsegError) as e:
        gpu.fish_render_tiff(np.zeros((H, W, 3), np.uint8), (0, 1, 3), np.zeros((H, W, 2), np.uint8), bnd)
    assert e.value.code == -1 and 'channel index' in str(e.value)
    lib = load_library()
    img, thr, ch = np.zeros((H, W, 3), np.uint8), np.zeros((H, W, 2), np.uint8), np.array([0, 1, 2], np.int32)
    files = [np.full(4096, 0xa5, np.uint8) for _ in range(3)]
    ptrs = (C.c_void_p * 3)(*[f.ctypes.data for f in files])
    n = (C.c_longlong * 3)()
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    assert lib.ecseg_fish_render_tiff(gpu.h, vp(img), H, W, 3, vp(ch), vp(thr), 2, vp(bnd), ptrs, 100, n, None, None, None) == -1
    assert 'does not fit' in lib.ecseg_last_error(gpu.h).decode() and all((f == 0xa5).all() for f in files)
    assert lib.ecseg_fish_render_tiff(gpu.h, vp(img), H, W, 3, vp(ch), vp(thr), 2, vp(bnd), ptrs, 4096, n, None, None, None) == 0
    assert all(0 < k < 4096 for k in n)


def test_make_stat_fish_writes_the_same_bytes_with_the_key_and_without(gpu, tmp_path, monkeypatch):
    """Three- and four-channel images, the min-cut picture included: every file and the CSV."""
    inp, _ = cpu.make_folder(tmp_path, size=(67, 93))

    def run(**keys):
        cfg = yaml.safe_load(open(tmp_path / 'config.yaml'))
        cfg['stat_fish'].update(use_min_cut=True, **keys)
        cfg['stat_fish'] = {k: v for k, v in cfg['stat_fish'].items() if v is not None}
        yaml.safe_dump(cfg, open(tmp_path / 'config.yaml', 'w'))
        sf.main([], handle=gpu)
        return cpu.folder_bytes(inp / 'annotated')

    monkeypatch.chdir(tmp_path)
    want = run()
    got = run(tiff_on_device=True)
    back = run(tiff_on_device=False)
    assert sorted(got) == sorted(want) == sorted(back) and len(want) == 3 * 6 + 2
    assert any(name.endswith('_segmentation_corrected_min_cut.tif') for name in want) and 'stat_fish_lsq.csv' in want
    for name in want:
        assert got[name] == want[name] == back[name], name
