"""ecseg_meta_segment_files on the device: the results of ecseg_meta_segment plus, per image, the dapi TIFF and the label PNG as
the host writers put them on disk, byte for byte; the capacity protocol; ``make metaseg`` with ``files_on_device`` on, off and
absent."""
import ctypes as C
import os
import shutil

import numpy as np
import pytest
from PIL import Image

from ecseg_amd import image_io, metaseg, synth
from ecseg_amd._lib import load_library
from ecseg_amd.model import MetasegModel
from ecseg_amd.utils import get_imgs

pytestmark = pytest.mark.gpu
SIZES = [(256, 256), (300, 270)]


@pytest.fixture(scope='module')
def model16(gpu):
    cfg = synth.unet_config(base=16)
    return MetasegModel(cfg, synth.unet_weights(cfg, seed=0), handle=gpu)


def _images(H, W):
    imgs = np.stack([synth.dapi_image(60 + i, H, W, rgb=True) for i in range(3)])
    imgs[1, ..., 2] = 255 - imgs[1, ..., 2]                 # a bright background: the inverting branch of the pre-processing
    return imgs


def _host_files(gray, post, tmp_path):
    t, p = str(tmp_path / 'h.tif'), str(tmp_path / 'h.png')
    image_io.write_tiff_gray8(t, gray, invert=True)
    image_io.write_label_png(p, post)
    return open(t, 'rb').read(), open(p, 'rb').read()


@pytest.mark.parametrize('size', SIZES, ids=['%dx%d' % s for s in SIZES])
def test_the_files_are_the_host_writers_files_and_the_results_meta_segments(model16, size, tmp_path):
    H, W = size
    h = model16.handle
    imgs = _images(H, W)
    want = h.meta_segment(imgs)
    gray, post, nec, tie, dapi, png = h.meta_segment_files(imgs)
    assert all(np.array_equal(a, b) for a, b in zip(want, (gray, post, nec, tie)))
    host = [_host_files(gray[i], post[i], tmp_path) for i in range(3)]
    for i in range(3):
        assert isinstance(dapi[i], bytes) and dapi[i] == host[i][0], 'dapi file %d' % i
        assert isinstance(png[i], bytes) and png[i] == host[i][1], 'label PNG %d' % i
    assert h.last_file_bytes == [len(f[0]) for f in host] + [len(f[1]) for f in host]
    ms = h.file_timings()
    assert 0 < ms['dapi'] < 10000 and 0 < ms['png'] < 10000
    # one byte short for one file of each kind: that file alone is missing, its size is reported, results and other files are whole
    r = h.meta_segment_files(imgs, dapi_capacity=len(host[1][0]) - 1, png_capacity=max(len(f[1]) for f in host))
    assert all(np.array_equal(a, b) for a, b in zip(want, r[:4]))
    for i in range(3):
        fits = len(host[i][0]) <= len(host[1][0]) - 1
        assert r[4][i] == (host[i][0] if fits else None) and h.last_file_bytes[i] == (len(host[i][0]) if fits else -len(host[i][0]))
        assert r[5][i] == host[i][1]
    big = max(range(3), key=lambda i: len(host[i][1]))
    r = h.meta_segment_files(imgs, png_capacity=len(host[big][1]) - 1)
    assert r[5][big] is None and h.last_file_bytes[3 + big] == -len(host[big][1]) and r[4] == [f[0] for f in host]
    # page-locked buffers for the files: views of them, the same bytes; and again the plain call
    dcap, pcap = metaseg.file_capacities(H, W)
    bufs = [h.host_empty((3 * dcap,)), h.host_empty((3 * pcap,))]
    try:
        for b in bufs:
            b[...] = 0xa5
        r = h.meta_segment_files(imgs, file_bufs=bufs)
        for i in range(3):
            assert r[4][i].tobytes() == host[i][0] and r[5][i].tobytes() == host[i][1]
            assert (bufs[0][i * dcap + len(host[i][0]):(i + 1) * dcap] == 0xa5).all(), 'bytes behind a file'
            assert (bufs[1][i * pcap + len(host[i][1]):(i + 1) * pcap] == 0xa5).all(), 'bytes behind a file'
    finally:
        for b in bufs:
            h.host_release(b)
    assert all(np.array_equal(a, b) for a, b in zip(want, h.meta_segment(imgs)))


def test_bad_arguments_are_refused(model16):
    h, lib = model16.handle, load_library()
    imgs = _images(256, 256)[:1]
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    buf = np.zeros(2 << 20, np.uint8)
    post = np.zeros((1, 256, 256), np.uint8)
    tab, hole = (C.c_void_p * 1)(buf.ctypes.data), (C.c_void_p * 1)(None)
    n1, n2 = (C.c_longlong * 1)(), (C.c_longlong * 1)()

    def call(img=vp(imgs), n=1, H=256, W=256, Cc=3, bps=1, d=tab, dcap=1 << 20, dn=n1, p=tab, pcap=1 << 20, pn=n2, out=vp(post)):
        return lib.ecseg_meta_segment_files(h.h, img, n, H, W, Cc, bps, d, dcap, dn, p, pcap, pn, None, out, None, None)

    assert call() == 0 and n1[0] > 0 and n2[0] > 0                              # (gray_out, n_ec and tie_risk may be null)
    for kw in (dict(img=None), dict(out=None), dict(H=0), dict(W=0), dict(Cc=2), dict(bps=3), dict(n=-1), dict(d=None), dict(p=None),
               dict(dn=None), dict(pn=None), dict(dcap=0), dict(pcap=0), dict(d=hole), dict(p=hole)):
        assert call(**kw) == -1, kw
    assert call(n=0) == 0


def test_make_metaseg_writes_the_same_bytes_with_the_key_on_off_and_absent(model16, tmp_path):
    H, W = SIZES[1]
    runs = {}
    for name, kw in (('absent', {}), ('on', dict(files_on_device=True)), ('off', dict(files_on_device=False))):
        folder = tmp_path / name
        for sub in ('dapi', 'labels'):
            os.makedirs(folder / sub)
        for i, rgb in enumerate(_images(H, W)):
            Image.fromarray(rgb).save(str(folder / ('img%d.tif' % i)), compression='tiff_lzw')
        paths = get_imgs(str(folder))
        rec = metaseg.run(str(folder), model16, paths, batch_images=2, io_threads=2, log=lambda *a: None, **kw)
        assert not metaseg.finish(str(folder), paths, rec, 0, log=lambda *a: None)
        files = {}
        for root, _, names in os.walk(folder):
            for n in names:
                files[os.path.relpath(os.path.join(root, n), folder)] = open(os.path.join(root, n), 'rb').read()
        runs[name] = files
        shutil.rmtree(folder)
    assert sorted(runs['on']) == sorted(runs['off']) == sorted(runs['absent']) and len(runs['on']) == 3 + 3 * 3 + 3
    for n in runs['absent']:
        assert runs['on'][n] == runs['absent'][n] == runs['off'][n], n
    assert 'ec_quantification.csv' in runs['on'] and os.path.join('labels', 'img0.png') in runs['on']
