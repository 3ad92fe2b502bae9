"""ecseg_overlay_files on the device: the rows of ``overlay`` on the 8-bit image and the red / green files of the host writer, byte for
byte, on the committed overlay seeds and on 16-bit inputs; and ``meta_overlay.run`` over a folder with ``files_on_device`` on and off."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import overlay_cases as oc                   # noqa: E402
from ecseg_amd import csvio, image_io, meta_overlay     # noqa: E402
from ecseg_amd.utils import get_imgs         # noqa: E402

pytestmark = pytest.mark.gpu


def _host_files(I8, tmp_path):
    out = []
    for ch, sub in ((0, 'red'), (1, 'green')):
        path = str(tmp_path / (sub + '.png'))
        image_io.write_png_channel(path, I8, ch, invert=True)
        out.append(open(path, 'rb').read())
    return out


def _check(gpu, labels, img, sens, thr, tmp_path):
    """one call on (n, H, W) labels and (n, H, W, C) images against overlay(u16_to_u8) and the host writer"""
    I8 = gpu.u16_to_u8(img) if img.dtype == np.uint16 else img
    want = gpu.overlay(labels, np.ascontiguousarray(I8), sens, thr)
    rec, red, green = gpu.overlay_files(labels, img, sens, thr)
    assert rec.dtype == want.dtype and np.array_equal(rec, want)
    for i in range(labels.shape[0]):
        r, g = _host_files(I8[i], tmp_path)
        assert red[i] == r and green[i] == g, i
    t = gpu.file_timings()
    assert t['dapi'] == 0 and 0 < t['png'] <= gpu.timings()['count'] < 10000


@pytest.mark.parametrize('seed', range(oc.N_SEEDS))
def test_rows_and_files_on_the_committed_seeds(gpu, seed, tmp_path):
    c = oc.scene(seed)
    _check(gpu, c['labels'][None], c['rgb'][None], c['sens'], c['thr'], tmp_path)


def _u16_batch(seed, n=2, C=3):
    labels, rgb, sens, thr = oc.batch(n, (96, 128), seed0=seed, C=C)
    rng = np.random.default_rng(seed)
    img = rgb.astype(np.uint16) * 257                         # full-range 16-bit samples around the 8-bit scene, low bytes stirred
    img ^= rng.integers(0, 256, img.shape, dtype=np.uint16)
    return labels, img, sens, thr


@pytest.mark.parametrize('seed,C', [(8100, 3), (8200, 4)])
def test_rows_and_files_on_16_bit_images(gpu, seed, C, tmp_path):
    _check(gpu, *_u16_batch(seed, C=C), tmp_path)


def test_one_image_comes_back_as_one_row_and_two_files(gpu, tmp_path):
    labels, rgb, sens, thr = oc.batch(1, (96, 128))
    rec, red, green = gpu.overlay_files(labels[0], rgb[0], sens, thr)
    assert rec.shape == (12,) and np.array_equal(rec, gpu.overlay(labels[0], rgb[0], sens, thr))
    assert [red, green] == _host_files(rgb[0], tmp_path)


def _folder(root):
    """5 RGB images of 96 x 128 in two dtypes (so that groups split) and one grayscale file, with the labels metaseg would leave"""
    for sub in ('labels', 'dapi', 'red', 'green'):
        os.makedirs(root / sub)
    labels, rgb, _, _ = oc.batch(5, (96, 128), seed0=9100)
    for i in range(5):
        name = 'img%d.tif' % i
        img = rgb[i] if i in (0, 1, 4) else _u16_batch(9200 + i, n=1)[1][0]
        image_io.write_tiff_rgb8(str(root / name), img) if img.dtype == np.uint8 else _write_tiff16(str(root / name), img)
        np.save(str(root / 'labels' / ('img%d.npy' % i)), labels[i].astype(np.int64))
    image_io.write_tiff_gray8(str(root / 'gray.tif'), rgb[0, ..., 0])
    return str(root)


def _write_tiff16(path, img):
    """an uncompressed little-endian 16-bit RGB TIFF of one strip"""
    import struct
    H, W, C = img.shape
    data = np.ascontiguousarray(img, '<u2').tobytes()
    extra_off = 8 + len(data)
    extra = struct.pack('<3H', 16, 16, 16)
    ifd_off = extra_off + len(extra)
    tags = [(256, 4, 1, W), (257, 4, 1, H), (258, 3, 3, extra_off), (259, 3, 1, 1), (262, 3, 1, 2), (273, 4, 1, 8), (277, 3, 1, 3),
            (278, 4, 1, H), (279, 4, 1, len(data)), (284, 3, 1, 1)]
    with open(path, 'wb') as f:
        f.write(b'II' + struct.pack('<HI', 42, ifd_off) + data + extra + struct.pack('<H', len(tags)))
        for t in tags:
            f.write(struct.pack('<HHII', *t))
        f.write(struct.pack('<I', 0))


def test_a_folder_run_with_the_key_on_writes_the_files_and_rows_of_the_key_off(gpu, tmp_path):
    out = {}
    for key in (False, True):
        root = _folder(tmp_path / ('on' if key else 'off'))
        said = []
        stats = {}
        rows = meta_overlay.run(root, gpu, get_imgs(root), 85, batch_images=2, io_threads=2, log=lambda *a: said.append(a[0] if len(a) == 1 else a[1:]),
                                stats=stats, files_on_device=key)
        files = {}
        for sub in ('red', 'green'):
            for f in sorted(os.listdir(os.path.join(root, sub))):
                files[sub + '/' + f] = open(os.path.join(root, sub, f), 'rb').read()
        out[key] = (csvio.csv_text(csvio.OVERLAY_COLUMNS, rows), files, len(said), sorted(stats))
    assert out[True] == out[False]
    assert len(out[True][1]) == 10 and len(out[True][0].splitlines()) == 6
    assert image_io.imread(os.path.join(str(tmp_path / 'on'), 'img2.tif')).dtype == np.uint16


def _raw_call(gpu, labels, img, sens, thr, cap, red=None, green=None, sentinel=0xa5):
    """ecseg_overlay_files itself on buffers of `cap` bytes per file filled with a sentinel -> (status, rows, buffers, lengths)"""
    import ctypes as C
    from ecseg_amd._lib import load_library
    lib = load_library()
    n, H, W, Cc = img.shape
    bufs = [np.full(n * cap + 64, sentinel, np.uint8) for _ in range(2)]
    tabs = [(C.c_void_p * n)(*[b.ctypes.data + i * cap for i in range(n)]) for b in bufs]
    lens = [(C.c_longlong * n)(), (C.c_longlong * n)()]
    out = np.zeros((n, 12), np.int64)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    rc = lib.ecseg_overlay_files(gpu.h, vp(labels), vp(img), n, H, W, Cc, img.dtype.itemsize, sens, thr, vp(out),
                                 tabs[0] if red is None else red, tabs[1] if green is None else green, cap, lens[0], lens[1])
    return rc, out, bufs, [list(v) for v in lens]


def test_a_capacity_one_byte_short_drops_that_file_only_and_reports_its_size(gpu, tmp_path):
    labels, rgb, sens, thr = oc.batch(3, (96, 128), seed0=9300)
    rgb = rgb.copy()
    rgb[1, ..., 1] = np.random.default_rng(4).integers(0, 256, (96, 128), dtype=np.uint8)      # image 1's green file is the largest of the six
    want = [_host_files(rgb[i], tmp_path) for i in range(3)]
    sizes = sorted(len(f) for pair in want for f in pair)
    assert len(want[1][1]) == sizes[-1] > sizes[-2]
    cap = len(want[1][1]) - 1
    rc, rows, bufs, lens = _raw_call(gpu, labels, rgb, sens, thr, cap)
    assert rc == 0 and np.array_equal(rows, gpu.overlay(labels, rgb, sens, thr))
    for i in range(3):
        for c in range(2):
            slot = bufs[c][i * cap:(i + 1) * cap]
            if (i, c) == (1, 1):
                assert lens[c][i] == -len(want[i][c]) and (slot == 0xa5).all(), 'bytes of a file that does not fit were written'
            else:
                assert lens[c][i] == len(want[i][c]) and slot[:lens[c][i]].tobytes() == want[i][c] and (slot[lens[c][i]:] == 0xa5).all(), (i, c)
    assert (bufs[0][3 * cap:] == 0xa5).all() and (bufs[1][3 * cap:] == 0xa5).all()
    rc, _, bufs, lens = _raw_call(gpu, labels, rgb, sens, thr, cap + 1)                          # exactly enough is enough
    assert rc == 0 and lens[1][1] == cap + 1 and bufs[1][(cap + 1):2 * (cap + 1)].tobytes() == want[1][1]


def test_bad_arguments_are_refused(gpu):
    import ctypes as C
    from ecseg_amd._lib import load_library
    lib = load_library()
    labels = np.zeros((2, 4, 4), np.uint8)
    img = np.zeros((2, 4, 4, 3), np.uint8)
    rc, _, _, lens = _raw_call(gpu, labels, img, 85, 20, 4096)
    assert rc == 0 and lens[0][0] > 0 and lens[0] == lens[1]
    buf = np.zeros(2 * 4096, np.uint8)
    tab = (C.c_void_p * 2)(buf.ctypes.data, buf.ctypes.data + 4096)
    holes = (C.c_void_p * 2)(buf.ctypes.data, None)
    n2 = (C.c_longlong * 2)()
    out = np.zeros((2, 12), np.int64)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)

    def call(h=gpu.h, lab=vp(labels), im=vp(img), n=2, H=4, W=4, Cc=3, bps=1, o=vp(out), red=tab, green=tab, cap=4096, rb=n2, gb=n2):
        return lib.ecseg_overlay_files(h, lab, im, n, H, W, Cc, bps, 85, 20, o, red, green, cap, rb, gb)

    for kw in (dict(H=0), dict(W=0), dict(n=-1), dict(n=65536), dict(Cc=1), dict(bps=0), dict(bps=3), dict(bps=4), dict(cap=0), dict(lab=None),
               dict(im=None), dict(o=None), dict(red=None), dict(green=None), dict(rb=None), dict(gb=None), dict(red=holes), dict(green=holes)):
        assert call(**kw) == -1, kw
        assert 'overlay_files' in lib.ecseg_last_error(gpu.h).decode()
    assert call(h=None) == -1
    assert call(n=0) == 0                                     # no image: nothing to do
    with pytest.raises(TypeError):
        gpu.overlay_files(labels, img.astype(np.float32), 85)
    with pytest.raises(ValueError):
        gpu.overlay_files(labels, img[:1], 85)
