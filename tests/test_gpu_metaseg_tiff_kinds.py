"""ecseg_meta_segment_tiffs, ecseg_meta_segment_tiffs_files and ecseg_prefetch_tiffs read the handle options tiff_deflate_on_device,
tiff_tiled_on_device and tiff_packbits_on_device: Deflate strips, LZW and Deflate tiles, PackBits strips and tiles decode into the
U-Net's batch as LZW strips do - status[i] what ecseg_tiff_decode returns for the file alone on this handle, a failed image the
all-zero image with n_ec -1, every other image exactly ecseg_meta_segment on image_io.read_tiff's samples - in the call itself and on
the decode-ahead path, where a set decoded under other options is withdrawn.  With the options off every one of these files is -5,
as on the commit before.  One U-Net window (256 x 256), gray and RGB, the small seeded model of test_gpu_metaseg_tiffs.py."""
import contextlib
import functools
import os
import shutil
import sys
import zlib

import numpy as np
import pytest
import yaml

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import tiff_decode_cases as dc               # noqa: E402
import tiff_packbits_cases as pc             # noqa: E402
import tiff_tiles_cases as tc                # noqa: E402
from test_gpu_metaseg_tiffs import _samples, model16, same, tshape      # noqa: E402,F401  (model16: the module's fixture)
from ecseg_amd import image_io, metaseg      # noqa: E402
from ecseg_amd._lib import E_UNSUPPORTED     # noqa: E402

pytestmark = pytest.mark.gpu
SIZE = (256, 256)
OPTIONS = ('tiff_deflate_on_device', 'tiff_tiled_on_device', 'tiff_packbits_on_device')
# name -> (the options it needs, the writer)
KINDS = {
    'deflate_strips': (('deflate',), lambda img: deflate_strips(img, 8)),
    'lzw_tiles': (('tiled',), lambda img: tc.tiled_tiff(img, 64, 64, 5, 2)),
    'deflate_tiles': (('deflate', 'tiled'), lambda img: tc.tiled_tiff(img, 64, 64, 8, 1)),
    'packbits_strips': (('packbits',), lambda img: pc.strip_file(img, 8)),
    'packbits_tiles': (('packbits', 'tiled'), lambda img: pc.tile_file(img, 64, 64)),
}
CASES = [(kind, spp) for kind in KINDS for spp in (1, 3)]
IDS = ['%s_%s' % (k, 'gray' if s == 1 else 'rgb') for k, s in CASES]


def deflate_strips(img, rps):
    H, W = img.shape[:2]
    rows = img.reshape(H, -1)
    return dc.tiff_file([zlib.compress(rows[r:r + rps].tobytes(), 6) for r in range(0, H, rps)], H, W, rps, spp=1 if img.ndim == 2 else img.shape[2],
                        compression=8)


@contextlib.contextmanager
def options(h, names=()):
    try:
        h.set_option('tiff_deflate_on_device', int('deflate' in names))
        h.set_option('tiff_tiled_on_device', int('tiled' in names))
        h.set_option('tiff_packbits_on_device', int('packbits' in names))
        yield h
    finally:
        for key in OPTIONS:
            h.set_option(key, 0)


def read_tiff(data):
    import tempfile
    with tempfile.TemporaryDirectory() as tmp:
        p = os.path.join(tmp, 'f.tif')
        open(p, 'wb').write(data)
        return image_io.read_tiff(p)


@functools.lru_cache(maxsize=None)
def kind_files(kind, spp, seed0=60):
    """three files of a kind (the middle one with the bright background) -> (file bytes, image_io.read_tiff's samples)"""
    datas = [KINDS[kind][1](_samples(seed0 + i, SIZE[0], SIZE[1], spp, 8, i == 1)) for i in range(3)]
    imgs = [read_tiff(d) for d in datas]
    assert all(np.array_equal(im, _samples(seed0 + i, SIZE[0], SIZE[1], spp, 8, i == 1)) for i, im in enumerate(imgs))
    return datas, imgs


@pytest.mark.parametrize('kind,spp', CASES, ids=IDS)
def test_the_results_are_meta_segments_on_the_python_readers_samples(model16, tmp_path, kind, spp):
    h = model16.handle
    datas, imgs = kind_files(kind, spp)
    shape = tshape(imgs[0])
    want = h.meta_segment(np.stack(imgs))
    with options(h, KINDS[kind][0]):
        got = h.meta_segment_tiffs(datas, shape)
        assert got[4] == [0, 0, 0]
        assert same(want, got[:4])
        assert 0 < h.read_timings()['decode'] < 10000
        files = h.meta_segment_files(np.stack(imgs))
        tf = h.meta_segment_tiffs_files(datas, shape)
        assert tf[6] == [0, 0, 0] and same(want, tf[:4])
        assert list(tf[4]) == list(files[4]) and list(tf[5]) == list(files[5]), 'the dapi TIFFs and the label PNGs, byte for byte'
        assert all(isinstance(f, bytes) and len(f) > 100 for f in list(tf[4]) + list(tf[5]))
    with options(h):                                         # the options off: as on the commit before
        off = h.meta_segment_tiffs(datas, shape)
        assert off[4] == [E_UNSUPPORTED] * 3 and off[2].tolist() == [-1] * 3
    for name in KINDS[kind][0]:                              # and each option the kind needs is needed
        with options(h, [n for n in KINDS[kind][0] if n != name]):
            assert h.meta_segment_tiffs(datas, shape)[4] == [E_UNSUPPORTED] * 3, name


def _pinned(h, datas, keep):
    buf = h.host_empty((sum(len(d) for d in datas),))
    keep.append(buf)
    at, views = 0, []
    for d in datas:
        buf[at:at + len(d)] = np.frombuffer(d, np.uint8)
        views.append(buf[at:at + len(d)])
        at += len(d)
    return views


@pytest.mark.parametrize('kind,spp', CASES, ids=IDS)
def test_decode_ahead_changes_no_result_and_a_set_planned_under_other_options_is_withdrawn(model16, kind, spp):
    h = model16.handle
    on = KINDS[kind][0]
    (da, ia), (db, ib) = kind_files(kind, spp), kind_files(kind, spp, 80)
    shape = tshape(ia[0])
    with options(h, on):
        plain = [h.meta_segment_tiffs(d, shape) for d in (da, db)]
    assert all(r[4] == [0, 0, 0] for r in plain)
    keep = []
    try:
        A, B = _pinned(h, da, keep), _pinned(h, db, keep)
        with options(h, on):
            # prefetched, then consumed: the results of the plain calls
            h.prefetch_tiffs(B, shape)
            ra = h.meta_segment_tiffs(A, shape)
            rb = h.meta_segment_tiffs(B, shape)
            assert same(plain[0][:4], ra[:4]) and same(plain[1][:4], rb[:4]) and ra[4] == rb[4] == [0, 0, 0]
            assert h.read_timings()['decode'] > 0
            # decoded ahead with the options on, consumed after they went off: not these rasters - the files are refused, as a plain call refuses them
            h.prefetch_tiffs(B, shape)
            assert same(plain[0][:4], h.meta_segment_tiffs(A, shape)[:4])
            for key in OPTIONS:
                h.set_option(key, 0)
            off = h.meta_segment_tiffs(B, shape)
            assert off[4] == [E_UNSUPPORTED] * 3 and off[2].tolist() == [-1] * 3
        with options(h):
            # planned ahead with the options off (every file refused), consumed after they went on: decoded by the call itself
            h.prefetch_tiffs(B, shape)
            assert h.meta_segment_tiffs(A, shape)[4] == [E_UNSUPPORTED] * 3
            for key in OPTIONS:
                h.set_option(key, int(key.split('_')[1] in on))
            rb = h.meta_segment_tiffs(B, shape)
            assert rb[4] == [0, 0, 0] and same(plain[1][:4], rb[:4])
            # and the files' call on the decode-ahead path
            h.prefetch_tiffs(A, shape)
            h.meta_segment_tiffs(B, shape)
            tf = h.meta_segment_tiffs_files(A, shape)
            assert tf[6] == [0, 0, 0] and same(plain[0][:4], tf[:4])
    finally:
        h.prefetch_tiffs(None)
        for key in OPTIONS:
            h.set_option(key, 0)
        for b in keep:
            h.host_release(b)


def test_a_corrupt_deflate_file_and_one_of_another_extent_cost_their_neighbours_nothing(model16):
    h = model16.handle
    datas, imgs = kind_files('deflate_strips', 1)
    shape = tshape(imgs[0])
    img = imgs[1]
    rows = img.reshape(SIZE[0], -1)
    strips = [zlib.compress(rows[r:r + 8].tobytes(), 6) for r in range(0, SIZE[0], 8)]
    strips[5] = strips[5][:-2] + bytes([strips[5][-2] ^ 0x55, strips[5][-1]])          # a wrong Adler-32
    corrupt = dc.tiff_file(strips, SIZE[0], SIZE[1], 8, compression=8)
    other = deflate_strips(np.ascontiguousarray(img[:-3, :-5]), 8)
    with pytest.raises((zlib.error, image_io.TiffError)):
        read_tiff(corrupt)
    with options(h, ('deflate',)):
        want = h.meta_segment_tiffs(datas, shape)
        zero = h.meta_segment(np.zeros((1,) + SIZE, np.uint8))
        got = h.meta_segment_tiffs([datas[0], corrupt, other, datas[2]], shape)
        assert got[4] == [0, -1, -1, 0] and got[2].tolist()[1:3] == [-1, -1]
        for k, w in ((0, 0), (3, 2)):
            assert all(np.array_equal(a[w], b[k]) for a, b in zip(want[:4], got[:4])), k
        for k in (1, 2):
            assert np.array_equal(got[0][k], zero[0][0]) and np.array_equal(got[1][k], zero[1][0]), 'the all-zero image'
        tf = h.meta_segment_tiffs_files([datas[0], corrupt, other, datas[2]], shape)
        assert tf[6] == [0, -1, -1, 0] and tf[4][1] is None and tf[5][2] is None and tf[4][0] is not None and tf[5][3] is not None


def _cli_folder(folder):
    """256 x 256 gray images, one each of LZW strips, Deflate strips, LZW tiles, PackBits strips and .npy - and a second Deflate file, so
    that the folder holds 512 Deflate strips: with the keys on the rule (280 from the measured table) sends the LZW and the two Deflate
    files to the device in one call, and the join runs under the driver; tiled and PackBits files count in no rule and stay on the host"""
    os.makedirs(folder)
    img = lambda k: _samples(100 + k, SIZE[0], SIZE[1], 1, 8, k == 2)
    open(os.path.join(folder, 'a_deflate.tif'), 'wb').write(deflate_strips(img(1), 1))      # (the driver groups neighbours: the three files that count lie together)
    open(os.path.join(folder, 'b_deflate.tif'), 'wb').write(deflate_strips(img(5), 1))
    open(os.path.join(folder, 'c_lzw.tif'), 'wb').write(dc.file_of(img(0), 1))
    open(os.path.join(folder, 'd_tiled.tif'), 'wb').write(tc.tiled_tiff(img(2), 64, 64, 5, 2))
    open(os.path.join(folder, 'e_packbits.tif'), 'wb').write(pc.strip_file(img(3), 8))
    np.save(os.path.join(folder, 'f.npy'), img(4))


def test_make_metaseg_writes_the_same_files_with_all_keys_on_and_off(model16, tmp_path, monkeypatch, capsys):
    monkeypatch.setattr(metaseg, 'load_model', lambda name, device=None: model16)
    seen = []
    run = metaseg.run

    def spy(*a, **kw):
        seen.append(kw['stats'])
        return run(*a, **kw)
    monkeypatch.setattr(metaseg, 'run', spy)
    monkeypatch.chdir(tmp_path)
    keys = ('tiff_read_on_device', 'tiff_read_deflate', 'tiff_read_tiled', 'tiff_read_packbits')
    runs = {}
    for name, value in (('off', False), ('on', True)):
        folder = str(tmp_path / name)
        _cli_folder(folder)
        yaml.safe_dump({'metaseg': dict(inpath=folder, **{k: value for k in keys})}, open(tmp_path / 'config.yaml', 'w'))
        try:
            metaseg.main([])                                 # (returns: exit code 0)
        except SystemExit as e:
            assert e.code in (None, 0), (name, capsys.readouterr().out[-2000:])
        files = {}
        for sub in ('dapi', 'labels', ''):
            for n in sorted(os.listdir(os.path.join(folder, sub))):
                p = os.path.join(folder, sub, n)
                if os.path.isfile(p) and (sub or n == 'ec_quantification.csv'):
                    files[os.path.join(sub, n)] = open(p, 'rb').read()
        runs[name] = files
        shutil.rmtree(folder)
    assert [s['tiff_device_images'] for s in seen] == [0, 3]
    assert len(runs['off']) == 6 * 3 + 1 and 'ec_quantification.csv' in runs['off']
    assert sorted(runs['on']) == sorted(runs['off'])
    for n in runs['off']:
        assert runs['on'][n] == runs['off'][n], n
    for key in OPTIONS:
        assert not getattr(model16.handle, key, False), 'the handle goes back as it came'
