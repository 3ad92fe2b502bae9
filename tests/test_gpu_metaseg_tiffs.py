"""ecseg_meta_segment_tiffs on the device: the files of a batch decode straight into the input of the call that segments them.  Every
expected value is ``Handle.meta_segment`` on the samples the host reader (``image_io._native_tiff``) returns for the same bytes:
gray, labels, n_ec and tie_risk are equal byte for byte; a bad file costs the others nothing and leaves nothing stale; the
decode-ahead changes no result; ``make metaseg`` writes the same files with ``tiff_read_on_device`` on, off and absent."""
import ctypes as C
import functools
import os
import shutil
import sys

import numpy as np
import pytest
import yaml

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import tiff_decode_cases as tc               # noqa: E402
from ecseg_amd import image_io, metaseg, synth      # noqa: E402
from ecseg_amd._lib import E_UNSUPPORTED, load_library, pack_file_images      # noqa: E402
from ecseg_amd.model import MetasegModel     # noqa: E402

pytestmark = pytest.mark.gpu
SIZES = [(256, 256), (300, 270)]
# (name, samples per pixel, bits, rows per strip, compression, predictor, big-endian)
PLANS = [('rgb8_lzw_5rows_predictor', 3, 8, 5, 5, 2, False), ('gray8_lzw_1row', 1, 8, 1, 5, 1, False),
         ('rgb16_be_lzw_predictor', 3, 16, 7, 5, 2, True), ('rgba8_uncompressed', 4, 8, 16, 1, 1, False)]


@pytest.fixture(scope='module')
def model16(gpu):
    cfg = synth.unet_config(base=16)
    return MetasegModel(cfg, synth.unet_weights(cfg, seed=0), handle=gpu)


tiff_of = tc.file_of                         # (shared with tests/test_gpu_scratch.py)


def _samples(seed, H, W, spp, bits, bright=False):
    rgb = synth.dapi_image(seed, H, W, rgb=True)
    if bright:
        rgb[..., 2] = 255 - rgb[..., 2]                     # a bright background: the inverting branch of the pre-processing
    a = rgb[..., 2] if spp == 1 else rgb if spp == 3 else np.concatenate([rgb, np.full((H, W, 1), 255, np.uint8)], axis=2)
    return a.astype(np.uint16) * 257 if bits == 16 else np.ascontiguousarray(a)


@functools.lru_cache(maxsize=None)
def plan_files(plan, size, seed0=60):
    """three files of a plan and size (the middle one with the bright background) -> (file bytes, the host reader's samples)"""
    _, spp, bits, rps, comp, pred, be = PLANS[plan]
    H, W = size
    datas = [tiff_of(_samples(seed0 + i, H, W, spp, bits, i == 1), rps, comp, pred, be) for i in range(3)]
    return datas, [host_read(d) for d in datas]


def host_read(data):
    import tempfile
    with tempfile.TemporaryDirectory() as tmp:
        p = os.path.join(tmp, 'f.tif')
        open(p, 'wb').write(data)
        return image_io._native_tiff(p)


def tshape(a):
    return (a.shape[0], a.shape[1], 1 if a.ndim == 2 else a.shape[2], 8 * a.dtype.itemsize)


def same(want, got):
    return all(np.array_equal(a, b) for a, b in zip(want, got))


@pytest.mark.parametrize('size', SIZES, ids=['%dx%d' % s for s in SIZES])
@pytest.mark.parametrize('plan', range(len(PLANS)), ids=[p[0] for p in PLANS])
def test_the_results_are_meta_segments_on_the_host_readers_samples(model16, plan, size):
    h = model16.handle
    datas, imgs = plan_files(plan, size)
    assert all(im is not None and tshape(im) == (size[0], size[1]) + PLANS[plan][1:3] for im in imgs)
    want = h.meta_segment(np.stack(imgs))
    got = h.meta_segment_tiffs(datas, tshape(imgs[0]))
    assert got[4] == [0, 0, 0]
    assert same(want, got[:4])
    assert 0 < h.read_timings()['decode'] < 10000
    shapes, status = h.tiff_decode_packed(*pack_file_images([np.frombuffer(d, np.uint8) for d in datas]))      # (dst = NULL: no device work)
    assert status.tolist() == [0, 0, 0] and all(tuple(s) == tshape(imgs[0]) for s in shapes.tolist())


def _bad_files(size):
    H, W = size
    good = plan_files(1, size)[0][1]                          # gray, one row per strip
    img = plan_files(1, size)[1][1]
    strips = [tc.pack(tc.lzw_codes(img[r].tobytes())) for r in range(H)]
    broken = list(strips)
    broken[H // 2] = b'\xff' * len(strips[H // 2])          # a stream that does not start with a ClearCode and runs off its table
    from PIL import Image
    import io
    deflate = io.BytesIO()
    Image.fromarray(img).save(deflate, format='TIFF', compression='tiff_adobe_deflate')
    offs = [8] * H
    offs[3] = len(good) + 4096
    return [('corrupt_stream', tc.tiff_file(broken, H, W, 1), -1), ('offset_behind_the_file', tc.tiff_file(strips, H, W, 1, offsets=offs), -1),
            ('another_extent', tiff_of(np.ascontiguousarray(img[:-3, :-5]), 1), -1), ('deflate', deflate.getvalue(), E_UNSUPPORTED)]


@pytest.mark.parametrize('case', range(4), ids=['corrupt_stream', 'offset_behind_the_file', 'another_extent', 'deflate'])
def test_one_bad_file_in_the_middle_costs_the_others_nothing(model16, case):
    h, size = model16.handle, SIZES[0]
    datas, imgs = plan_files(1, size)
    name, bad, code = _bad_files(size)[case]
    want = h.meta_segment_tiffs(datas, tshape(imgs[0]))
    zero = h.meta_segment(np.zeros((1,) + size, np.uint8))
    if name == 'corrupt_stream':                             # directly behind a call on other images: nothing stale may show
        other = plan_files(1, size, 80)
        assert h.meta_segment_tiffs(other[0], tshape(imgs[0]))[4] == [0, 0, 0]
    got = h.meta_segment_tiffs([datas[0], bad, datas[2]], tshape(imgs[0]))
    assert got[4] == [0, code, 0]
    assert got[2].tolist()[1] == -1
    for k in (0, 2):
        assert all(np.array_equal(w[k], g[k]) for w, g in zip(want[:4], got[:4])), k
    assert np.array_equal(got[0][1], zero[0][0]) and np.array_equal(got[1][1], zero[1][0])     # the all-zero image's gray and labels


def test_the_files_are_the_host_writers_files(model16, tmp_path):
    h, size = model16.handle, SIZES[1]
    datas, imgs = plan_files(0, size)
    want = h.meta_segment(np.stack(imgs))
    gray, post, nec, tie, dapi, png, st = h.meta_segment_tiffs_files(datas, tshape(imgs[0]))
    assert st == [0, 0, 0] and same(want, (gray, post, nec, tie))
    for i in range(3):
        t, p = str(tmp_path / 'h.tif'), str(tmp_path / 'h.png')
        image_io.write_tiff_gray8(t, gray[i], invert=True)
        image_io.write_label_png(p, post[i])
        assert dapi[i] == open(t, 'rb').read() and png[i] == open(p, 'rb').read(), i
    r = h.meta_segment_tiffs_files([datas[0], tiff_of(np.zeros((8, 8), np.uint8), 1), datas[2]], tshape(imgs[0]))
    assert r[6] == [0, -1, 0] and r[4][1] is None and r[5][1] is None and r[4][0] == dapi[0] and r[5][2] == png[2]
    assert h.last_file_bytes[1] == 0 and h.last_file_bytes[4] == 0 and r[2].tolist()[1] == -1


def test_decode_ahead_changes_no_result(model16):
    h, size = model16.handle, SIZES[0]
    sets = [plan_files(1, size, s) for s in (60, 80, 100)]
    shape = tshape(sets[0][1][0])
    plain = [h.meta_segment_tiffs(d, shape) for d, _ in sets]
    assert all(r[4] == [0, 0, 0] for r in plain)
    # the files in page-locked memory, each batch a run of views of its own buffer (what the driver passes twice: named, then called)
    pinned, views = [], []
    try:
        for d, _ in sets:
            buf = h.host_empty((sum(len(f) for f in d),))
            pinned.append(buf)
            at, v = 0, []
            for f in d:
                buf[at:at + len(f)] = np.frombuffer(f, np.uint8)
                v.append(buf[at:at + len(f)])
                at += len(f)
            views.append(v)
        A, B, Cc = views
        # every batch names the next: the results are those without
        h.prefetch_tiffs(B, shape)
        ra = h.meta_segment_tiffs(A, shape)
        h.prefetch_tiffs(Cc, shape)
        rb = h.meta_segment_tiffs(B, shape)
        rc = h.meta_segment_tiffs(Cc, shape)
        for want, got in zip(plain, (ra, rb, rc)):
            assert same(want[:4], got[:4]) and got[4] == [0, 0, 0]
        assert h.read_timings()['decode'] > 0                # (those of the decode-ahead that served the last call)
        # B sent ahead, then C called: C's results
        h.prefetch_tiffs(B, shape)
        assert same(plain[0][:4], h.meta_segment_tiffs(A, shape)[:4])
        assert same(plain[2][:4], h.meta_segment_tiffs(Cc, shape)[:4])
        # named, then withdrawn
        h.prefetch_tiffs(B, shape)
        h.prefetch_tiffs(None)
        assert same(plain[0][:4], h.meta_segment_tiffs(A, shape)[:4])
        assert same(plain[1][:4], h.meta_segment_tiffs(B, shape)[:4])
        # sent ahead, then a plain call on images in between
        h.prefetch_tiffs(B, shape)
        assert same(plain[0][:4], h.meta_segment_tiffs(A, shape)[:4])
        imgs = np.stack(sets[2][1])
        assert same(plain[2][:4], h.meta_segment(imgs))
        assert same(plain[1][:4], h.meta_segment_tiffs(B, shape)[:4])
        # a batch with a corrupt file, decoded ahead: its status words are read by the call that takes the rasters
        bad = np.frombuffer(_bad_files(size)[0][1], np.uint8)
        mixed = [A[0], bad, A[2]]
        want = h.meta_segment_tiffs(mixed, shape)
        flat = h.host_empty((sum(m.size for m in mixed),))
        pinned.append(flat)
        at, mv = 0, []
        for m in mixed:
            flat[at:at + m.size] = m
            mv.append(flat[at:at + m.size])
            at += m.size
        h.prefetch_tiffs(mv, shape)
        h.meta_segment_tiffs(B, shape)
        got = h.meta_segment_tiffs(mv, shape)
        assert got[4] == want[4] == [0, -1, 0] and same(want[:4], got[:4])
    finally:
        h.prefetch_tiffs(None)
        for b in pinned:
            h.host_release(b)


def test_argument_errors_are_refused_and_the_handle_stays_usable(model16):
    h, lib, size = model16.handle, load_library(), SIZES[0]
    datas, imgs = plan_files(1, size)
    buf, ranges = pack_file_images([np.frombuffer(d, np.uint8) for d in datas])
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    post, st = np.zeros((3,) + size, np.uint8), np.zeros(3, np.int32)

    def call(files=vp(buf), tab=vp(ranges), Cc=1):
        return lib.ecseg_meta_segment_tiffs(h.h, files, buf.size, tab, 3, size[0], size[1], Cc, 1, vp(st), None, vp(post), None, None)

    assert call() == 0 and st.tolist() == [0, 0, 0]
    overlap = ranges.copy()
    overlap[1, 0] -= 1
    assert call(tab=None) == -1 and call(files=None) == -1 and call(tab=vp(overlap)) == -1 and call(Cc=2) == -1
    want = h.meta_segment(np.stack(imgs))
    assert same(want, h.meta_segment_tiffs(datas, tshape(imgs[0]))[:4])


def _cli_folder(folder):
    """five 256 x 256 gray LZW files at one row per strip (1280 strips: the rule sends the set), a .npy image, a Deflate TIFF, a
    corrupt TIFF in the middle of the set (with batch_images = 6 the device meets it) and a file of another extent"""
    from PIL import Image
    os.makedirs(folder)
    for i in range(5):
        open(os.path.join(folder, 'img%d.tif' % i), 'wb').write(plan_files(1, SIZES[0], 60 if i < 3 else 80)[0][i % 3])
    np.save(os.path.join(folder, 'n.npy'), plan_files(1, SIZES[0], 100)[1][0])
    Image.fromarray(plan_files(1, SIZES[0], 100)[1][2]).save(os.path.join(folder, 'deflate.tif'), compression='tiff_adobe_deflate')
    open(os.path.join(folder, 'img1x.tif'), 'wb').write(_bad_files(SIZES[0])[0][1])
    open(os.path.join(folder, 'other.tif'), 'wb').write(plan_files(1, SIZES[1])[0][0])


def test_make_metaseg_writes_the_same_files_with_the_key_on_off_and_absent(model16, tmp_path, monkeypatch, capsys):
    monkeypatch.setattr(metaseg, 'load_model', lambda name, device=None: model16)
    seen = []
    run = metaseg.run

    def spy(*a, **kw):
        seen.append(kw['stats'])
        return run(*a, **dict(kw, batch_images=6, io_threads=2))
    monkeypatch.setattr(metaseg, 'run', spy)
    monkeypatch.chdir(tmp_path)
    runs, said = {}, {}
    for name, keys in (('absent', {}), ('on', dict(tiff_read_on_device=True)), ('off', dict(tiff_read_on_device=False)),
                       ('both', dict(tiff_read_on_device=True, files_on_device=True))):
        folder = str(tmp_path / name)
        _cli_folder(folder)
        yaml.safe_dump({'metaseg': dict(inpath=folder, **keys)}, open(tmp_path / 'config.yaml', 'w'))
        with pytest.raises(SystemExit) as e:
            metaseg.main([])
        assert e.value.code == 1, name                       # (the corrupt file is missing from the CSV)
        out = capsys.readouterr().out.replace(folder, '<folder>')
        said[name] = sorted(line for line in out.splitlines() if ' image(s) in ' not in line)
        files = {}
        for sub in ('dapi', 'labels', ''):
            for n in sorted(os.listdir(os.path.join(folder, sub))):
                p = os.path.join(folder, sub, n)
                if os.path.isfile(p) and (sub or n == 'ec_quantification.csv'):
                    files[os.path.join(sub, n)] = open(p, 'rb').read()
        runs[name] = files
        shutil.rmtree(folder)
    assert [s['tiff_device_images'] for s in seen] == [0, 5, 0, 5]
    assert len(runs['absent']) == 8 * 3 + 1 and 'ec_quantification.csv' in runs['absent']
    for name in ('on', 'off', 'both'):
        assert sorted(runs[name]) == sorted(runs['absent']), name
        for n in runs['absent']:
            assert runs[name][n] == runs['absent'][n], (name, n)
        assert said[name] == said['absent'], name
    assert any(line.startswith('Skipping <folder>/img1x.tif') for line in said['on'])
