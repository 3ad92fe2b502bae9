"""The device label-PNG coder (csrc/png_kernels.hip) on the device: every case of tests/png_label_cases.py against the file the
host writer puts on disk, byte for byte; batches; repeats; the capacity protocol; bad arguments."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import png_label_cases as pc                 # noqa: E402
from ecseg_amd import image_io               # noqa: E402
from ecseg_amd._lib import EcsegError, load_library   # noqa: E402

pytestmark = pytest.mark.gpu
_HOST = {}


def host_file(name, labels, tmp_path_factory):
    """The file the host writer puts on disk, written once per image for the tests that need it."""
    if name not in _HOST:
        path = str(tmp_path_factory.mktemp('host') / 'l.png')
        image_io.write_label_png(path, labels)
        _HOST[name] = open(path, 'rb').read()
    return _HOST[name]


def _first_difference(got, want):
    return next((i for i, (a, b) in enumerate(zip(got, want)) if a != b), min(len(got), len(want)))


@pytest.mark.parametrize('case', pc.CASES, ids=[c.name for c in pc.CASES])
def test_the_device_file_is_the_host_file(gpu, case, tmp_path_factory):
    want = host_file(case.name, case.labels, tmp_path_factory)
    got = gpu.png_labels_encode(case.labels)
    assert isinstance(got, bytes) and len(got) == len(want), (len(got), len(want))
    assert got == want, 'first difference at byte %d of %d' % (_first_difference(got, want), len(want))
    assert gpu.last_file_bytes == [len(want)]
    assert 0 < gpu.timings()['count'] < 10000
    assert gpu.png_labels_encode(case.labels) == got, 'a second call gives other bytes'


@pytest.mark.parametrize('n', [1, 3, 5])
def test_a_batch_of_different_images_gives_each_its_file(gpu, n, tmp_path_factory):
    labels = pc.batch(n)
    assert len({im.tobytes() for im in labels}) == n
    want = [host_file('batch%d' % i, labels[i], tmp_path_factory) for i in range(n)]
    got = gpu.png_labels_encode(labels)
    assert isinstance(got, list) and len(got) == n
    for i in range(n):
        assert got[i] == want[i], 'image %d: first difference at byte %d of %d' % (i, _first_difference(got[i], want[i]), len(want[i]))
    assert gpu.png_labels_encode(labels) == got


def test_one_handle_runs_a_large_case_a_small_one_and_the_large_one_again(gpu, tmp_path_factory):
    by_name = {c.name: c for c in pc.CASES}
    for name in ('speckle_520x696', 'one_colour_1x1', 'speckle_520x696', 'blobs_300x270', 'speckle_520x696'):
        assert gpu.png_labels_encode(by_name[name].labels) == host_file(name, by_name[name].labels, tmp_path_factory), name


def test_a_capacity_one_byte_short_drops_that_file_only_and_reports_its_size(gpu, tmp_path_factory):
    labels = pc.batch(3)
    want = [host_file('batch%d' % i, labels[i], tmp_path_factory) for i in range(3)]
    sizes = sorted(len(w) for w in want)
    assert sizes[1] < sizes[2], 'the largest file must stand alone for this test'
    big = max(range(3), key=lambda i: len(want[i]))
    got = gpu.png_labels_encode(labels, capacity=len(want[big]) - 1)
    assert got[big] is None and gpu.last_file_bytes[big] == -len(want[big])
    for i in range(3):
        if i != big:
            assert got[i] == want[i] and gpu.last_file_bytes[i] == len(want[i])
    assert gpu.png_labels_encode(labels, capacity=len(want[big])) == want        # exactly enough is enough
    # nothing of a file that does not fit is written, and nothing lands behind a file that does
    lib = load_library()
    n, (H, W) = 3, pc.BATCH_EXTENT
    cap = len(want[big]) - 1
    buf = np.full(n * cap + 64, 0xa5, np.uint8)
    ptrs = (C.c_void_p * n)(*[buf.ctypes.data + i * cap for i in range(n)])
    out = (C.c_longlong * n)()
    assert lib.ecseg_png_labels_encode(gpu.h, labels.ctypes.data_as(C.c_void_p), n, H, W, ptrs, cap, out) == 0
    for i in range(n):
        slot = buf[i * cap:(i + 1) * cap]
        if i == big:
            assert out[i] == -len(want[i]) and (slot == 0xa5).all(), 'bytes of a file that does not fit were written'
        else:
            assert out[i] == len(want[i]) and slot[:out[i]].tobytes() == want[i] and (slot[out[i]:] == 0xa5).all()
    assert (buf[n * cap:] == 0xa5).all()


def test_bad_arguments_are_refused(gpu):
    lib = load_library()
    lab = np.zeros((2, 4, 4), np.uint8)
    buf = np.zeros(2 * 4096, np.uint8)
    ptrs = (C.c_void_p * 2)(buf.ctypes.data, buf.ctypes.data + 4096)
    holes = (C.c_void_p * 2)(buf.ctypes.data, None)
    out = (C.c_longlong * 2)()
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    call = lib.ecseg_png_labels_encode
    assert call(gpu.h, vp(lab), 2, 4, 4, ptrs, 4096, out) == 0 and out[0] > 0 and out[1] == out[0]
    for args in ((2, 0, 4), (2, 4, 0), (-1, 4, 4), (65536, 4, 4), (2, 4, 1 << 30)):
        assert call(gpu.h, vp(lab), args[0], args[1], args[2], ptrs, 4096, out) == -1, args
        assert 'bad arguments' in lib.ecseg_last_error(gpu.h).decode()
    assert call(gpu.h, None, 2, 4, 4, ptrs, 4096, out) == -1
    assert call(gpu.h, vp(lab), 2, 4, 4, None, 4096, out) == -1
    assert call(gpu.h, vp(lab), 2, 4, 4, ptrs, 4096, None) == -1
    assert call(gpu.h, vp(lab), 2, 4, 4, holes, 4096, out) == -1
    assert call(gpu.h, vp(lab), 2, 4, 4, ptrs, 0, out) == -1
    assert call(None, vp(lab), 2, 4, 4, ptrs, 4096, out) == -1
    assert call(gpu.h, vp(lab), 0, 4, 4, ptrs, 4096, out) == 0                  # no image: nothing to do
    with pytest.raises(ValueError):
        gpu.png_labels_encode(np.zeros((0, 4), np.uint8))
    with pytest.raises(EcsegError) as e:
        gpu.png_labels_encode(lab, capacity=0)
    assert e.value.code == -1
