"""The batched device TIFF reader (ecseg_tiff_decode_batch; the tiffb_* kernels of csrc/tiff_decode_kernels.hip) on the device.
Every expected value is the host reader's (ecseg_tiff_info + ecseg_tiff_read on the same bytes), and every file is also decoded
alone by ``Handle.tiff_decode``: a batch must give each file what it gets by itself, sample for sample and status for status."""
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
from ecseg_amd import image_io               # noqa: E402
from ecseg_amd import stat_fish as sf        # noqa: E402
from ecseg_amd._lib import EcsegError, load_library   # noqa: E402

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
EXTENTS = ((1, 1), (1, 7), (5, 1), (3, 64), (3, 65), (41, 43))
SENTINEL = 0xA5


def make_file(seed, H, W, rps, spp, bits, big_endian, predictor, lzw):
    """A file of ``dc.tiff_file`` around seeded samples: strips of ``rps`` rows, differenced where the predictor is on, in the file's
    byte order, LZW or as they are."""
    rng = np.random.default_rng(seed)
    top = 6 if seed % 2 else (256 if bits == 8 else 65536)       # long strings or noise
    img = rng.integers(0, top, (H, W, spp), dtype=np.uint16 if bits == 16 else np.uint8)
    stored = img
    if predictor:
        stored = img.copy()
        stored[:, 1:] = img[:, 1:] - img[:, :-1]
    stored = stored.astype(('>' if big_endian else '<') + ('u2' if bits == 16 else 'u1'))
    strips = [stored[r:r + rps].tobytes() for r in range(0, H, rps)]
    if lzw:
        strips = [dc.pack(dc.lzw_codes(s)) for s in strips]
    return dc.tiff_file(strips, H, W, rps, spp=spp, bits=bits, compression=5 if lzw else 1, predictor=2 if predictor else 1, big_endian=big_endian)


def host_read(data, tmp):
    """What the host's native reader makes of the bytes: the array, 'invalid', or None (left to the Python reader)."""
    path = os.path.join(str(tmp), 'host.tif')
    image_io.write_file_image(path, data)
    try:
        return image_io._native_tiff(path)
    except image_io.TiffError:
        return 'invalid'


def same(a, b):
    if a is None or b is None:
        return a is None and b is None
    if isinstance(a, str) or isinstance(b, str):
        return isinstance(a, str) and isinstance(b, str) and a == b
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b)


def plain(got):
    """An entry of ``tiff_decode_many`` in the terms of ``host_read``."""
    if isinstance(got, EcsegError):
        assert got.code == -1, got
        return 'invalid'
    assert not isinstance(got, Exception), got
    return got


@pytest.fixture(scope='module')
def pool(tmp_path_factory):
    """[(name, file bytes, host reader's samples)]: every extent at 1, 2 and all rows per strip, 8 and 16 bit in both byte orders,
    gray / RGB / RGBA, predictor on and off, LZW and uncompressed: 6 x 3 x 48 files, computed once and never changed."""
    tmp = tmp_path_factory.mktemp('pool')
    out, seed = [], 0
    for H, W in EXTENTS:
        for rps in (1, 2, H):
            for bits in (8, 16):
                for big in (False, True):
                    for spp in (1, 3, 4):
                        for pred in (False, True):
                            for lzw in (True, False):
                                seed += 1
                                data = make_file(seed, H, W, rps, spp, bits, big, pred, lzw)
                                want = host_read(data, tmp)
                                assert isinstance(want, np.ndarray) and want.shape[:2] == (H, W) and want.dtype == (np.uint16 if bits == 16 else np.uint8)
                                out.append(('%dx%d_rps%d_%dbit_%s_spp%d_pred%d_%s' % (H, W, rps, bits, 'be' if big else 'le', spp, pred, 'lzw' if lzw else 'raw'),
                                            data, want))
    assert len(out) == 6 * 3 * 48
    return out


def test_every_file_of_the_pool_alone(gpu, pool):
    """``Handle.tiff_decode`` of each file alone: the second yardstick of the batch tests holds the first."""
    for name, data, want in pool:
        assert same(gpu.tiff_decode(data), want), name


@pytest.mark.parametrize('n', [1, 2, 3, 65, 300])
def test_batches_of_mixed_files_in_three_orders(gpu, pool, n):
    """LZW and uncompressed, 8 and 16 bit, every extent, in one call; as picked, reversed and rotated."""
    picked = [pool[(7 + 109 * k) % len(pool)] for k in range(n)]       # 109 is coprime to the pool's 864: no file twice, the 48 kinds 13 apart
    kinds = {(w.dtype.itemsize, d[:2], name[-3:]) for name, d, w in picked}
    assert len(kinds) == (1, 2, 3, 8, 8)[(1, 2, 3, 65, 300).index(n)], 'both sample sizes, both byte orders, LZW and uncompressed'
    for order in (picked, picked[::-1], picked[n // 3:] + picked[:n // 3]):
        got = gpu.tiff_decode_many([d for _, d, _ in order])
        assert len(got) == n
        for (name, _, want), g in zip(order, got):
            assert same(plain(g), want), name
    assert 0 < gpu.timings()['count'] < 10000


def _packed(files):
    buf = np.frombuffer(b''.join(files), np.uint8)
    sizes = np.array([len(f) for f in files], np.int64)
    return buf, np.stack([np.cumsum(sizes) - sizes, sizes], axis=1)


def _raster_bytes(shape):
    return int(shape[0]) * int(shape[1]) * int(shape[2]) * (int(shape[3]) // 8)


def _decode_with_gaps(gpu, files, gap=5):
    """The files through ``tiff_decode_packed`` into a sentinel-filled destination with ``gap`` bytes (one more where a 16-bit raster
    would start odd) between the rasters -> (destination, offsets, shapes, status)."""
    buf, tab = _packed(files)
    shapes, status = gpu.tiff_decode_packed(buf, tab)
    offs, end = [], 2
    for sh, st in zip(shapes, status):
        end += gap
        end += end & 1 if sh[3] == 16 else 0
        offs.append(end)
        end += _raster_bytes(sh) if st == 0 else 0
    dst = np.full(end + 9, SENTINEL, np.uint8)
    shapes2, status2 = gpu.tiff_decode_packed(buf, tab, dst, offs)
    assert np.array_equal(shapes, shapes2)
    return dst, offs, shapes, status2


def _check_gapped(dst, offs, shapes, status, wants, names):
    """Every good file's raster is the host's, every other byte of the destination is still the sentinel."""
    untouched = np.ones(dst.size, bool)
    for off, sh, st, want, name in zip(offs, shapes, status, wants, names):
        if isinstance(want, np.ndarray):
            assert st == 0, (name, st)
            n = _raster_bytes(sh)
            got = dst[off:off + n].view(want.dtype).reshape(want.shape if want.ndim == 3 else want.shape + (1,))
            assert np.array_equal(got.reshape(want.shape), want), name
            untouched[off:off + n] = False
        elif want is None:
            assert st == -5, (name, st)
        else:
            assert st == -1, (name, st)
    assert (dst[untouched] == SENTINEL).all(), 'a byte outside the rasters of the good files was written'


def test_gaps_between_the_rasters_and_a_16_bit_raster_behind_an_odd_8_bit_one(gpu, pool):
    by = {name: (data, want) for name, data, want in pool}
    names = ['1x7_rps1_8bit_le_spp1_pred1_lzw', '3x65_rps2_16bit_be_spp3_pred1_lzw', '5x1_rps5_8bit_le_spp3_pred0_raw', '41x43_rps2_16bit_le_spp1_pred0_raw',
             '1x1_rps1_8bit_be_spp1_pred0_lzw', '3x64_rps1_16bit_be_spp4_pred1_lzw']
    files, wants = [by[n][0] for n in names], [by[n][1] for n in names]
    for gap in (0, 1, 5):
        dst, offs, shapes, status = _decode_with_gaps(gpu, files, gap)
        assert gap or offs[1] == offs[0] + 7 + 1, 'the 16-bit raster follows an odd-length 8-bit one'
        _check_gapped(dst, offs, shapes, status, wants, names)


@pytest.fixture(scope='module')
def odd_files(tmp_path_factory):
    """([(name, bytes, host's answer)] tolerated, the same for corrupt files): the streams the host decoder accepts beside a
    well-formed one (no leading ClearCode, no EOI, a full table, a short strip table ...), a KwKwK stream, and files the host refuses -
    a strip offset behind the file and the first three invalid files of the seeded corpus."""
    tmp = tmp_path_factory.mktemp('odd')
    tolerated = [(name, data, host_read(data, tmp)) for name, data in dc.tolerated_files()]
    kwkwk = dc.tiff_file([dc.pack(dc.lzw_codes(b'a' * 300 + b'ab' * 200 + b'abc' * 100))], 10, 100, 10)       # runs: the code just made is used at once
    tolerated.append(('kwkwk', kwkwk, host_read(kwkwk, tmp)))
    assert all(isinstance(w, np.ndarray) for _, _, w in tolerated)
    assert {'no_leading_clearcode', 'no_eoi', 'table_full_without_clearcode', 'table_shorter_than_the_image', 'kwkwk'} <= {n for n, _, _ in tolerated}
    corrupt = [('offset_behind_the_file', dc.offset_behind_the_file(), 'invalid')]
    for name, data in dc.corrupt_corpus():
        if len(corrupt) < 4 and isinstance(host_read(data, tmp), str):
            corrupt.append((name, data, 'invalid'))
    assert len(corrupt) == 4
    return tolerated, corrupt


def test_corrupt_files_first_last_and_in_the_middle_mark_themselves_and_nothing_else(gpu, odd_files, pool):
    tolerated, corrupt = odd_files
    good = tolerated + [pool[k] for k in (5, 123, 400, 777)]
    for where in ('first', 'last', 'middle', 'all'):
        if where == 'first':
            batch = corrupt[:2] + good
        elif where == 'last':
            batch = good + corrupt[2:]
        elif where == 'middle':
            batch = good[:5] + corrupt[1:3] + good[5:]
        else:
            batch = [corrupt[0], good[0], corrupt[1], corrupt[2], good[1], corrupt[3]]
        names, files, wants = [b[0] for b in batch], [b[1] for b in batch], [b[2] for b in batch]
        dst, offs, shapes, status = _decode_with_gaps(gpu, files)
        _check_gapped(dst, offs, shapes, status, wants, names)
        for (name, data, want), g in zip(batch, gpu.tiff_decode_many(files)):
            assert same(plain(g), want), (where, name)
            try:
                alone = gpu.tiff_decode(data)
            except EcsegError as e:
                alone = 'invalid' if e.code == -1 else e
            assert same(alone, want), (where, name)


def test_files_left_to_the_host_are_unsupported_in_place(gpu, pool, tmp_path):
    files = json.load(open(os.path.join(GOLDEN, 'io_tiff_files.json')))['files']
    pixels = np.load(os.path.join(GOLDEN, 'io_tiff_pixels.npz'))
    left = ('rgb8_deflate', 'rgb8_tiled16', 'gray8_packbits', 'rgb8_bigtiff')
    names = sorted(files)
    datas = [base64.b64decode(files[n]) for n in names]
    got = gpu.tiff_decode_many(datas)
    for name, data, g in zip(names, datas, got):
        alone = gpu.tiff_decode(data)
        assert same(g, alone), name
        if g is not None:
            assert same(g, pixels[name]), name
    assert all(got[names.index(n)] is None for n in left) and sum(g is not None for g in got) == 7
    shapes, status = gpu.tiff_decode_packed(*_packed(datas))
    k = names.index('rgb8_deflate')
    assert status[k] == -5 and tuple(shapes[k][:2]) == pixels['rgb8_deflate'].shape[:2], 'a Deflate file has its shape reported'
    assert status[names.index('rgb8_tiled16')] == -5 and not shapes[names.index('rgb8_tiled16')].any()


def test_the_pass_without_a_destination_fills_shapes_and_status_only(gpu, pool, odd_files):
    tolerated, corrupt = odd_files
    batch = [pool[3], corrupt[0], pool[500], (None, b'II*\0 nothing', 'invalid'), pool[863]]
    shapes, status = gpu.tiff_decode_packed(*_packed([b[1] for b in batch]))
    assert status.tolist() == [0, 0, 0, -1, 0], 'an offset behind the file is found with the strips, as in ecseg_tiff_decode'
    for (_, _, want), sh in zip(batch, shapes):
        if isinstance(want, np.ndarray):
            assert tuple(sh) == (want.shape[0], want.shape[1], want.shape[2] if want.ndim == 3 else 1, want.dtype.itemsize * 8)
    assert not shapes[3].any()
    assert gpu.timings()['count'] == 0


def test_each_argument_error_is_refused_and_nothing_is_written(gpu, pool):
    lib = load_library()
    vp = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    by = {name: (data, want) for name, data, want in pool}
    f8, w8 = by['1x7_rps1_8bit_le_spp1_pred0_lzw']
    f16, w16 = by['3x64_rps2_16bit_le_spp1_pred0_lzw']
    buf, tab = _packed([f8, f16])
    shapes, status = np.zeros((2, 4), np.int32), np.zeros(2, np.int32)
    dst = np.full(7 + 1 + w16.nbytes + 8, SENTINEL, np.uint8)

    def call(tab=tab, n=2, dst=dst, dst_bytes=None, offs=(0, 8), files=buf, files_bytes=None, shapes=shapes, status=status):
        o = None if offs is None else np.array(offs, np.int64)
        t = np.ascontiguousarray(tab, np.int64)
        return lib.ecseg_tiff_decode_batch(gpu.h, vp(files), buf.size if files_bytes is None else files_bytes, vp(t), n, vp(dst),
                                           (dst.size if dst is not None else 0) if dst_bytes is None else dst_bytes, vp(o), vp(shapes), vp(status))
    bad = [
        ('n_files < 0', dict(n=-1)),
        ('a range outside files_bytes', dict(files_bytes=buf.size - 1)),
        ('a range outside files_bytes', dict(tab=[[0, len(f8)], [len(f8), len(f16) + 1]])),
        ('a negative range', dict(tab=[[0, -1], [len(f8), len(f16)]])),
        ('overlapping ranges', dict(tab=[[0, len(f8)], [len(f8) - 1, len(f16)]])),
        ('ranges out of order', dict(tab=[[len(f8), len(f16)], [0, len(f8)]])),
        ('too little room before dst_bytes', dict(dst_bytes=8 + w16.nbytes - 1)),
        ('a raster that starts behind dst_bytes', dict(offs=(0, dst.size + 2))),
        ('a negative offset', dict(offs=(0, -2))),
        ('overlapping rasters', dict(offs=(0, 6))),
        ('overlapping rasters, the other way round', dict(offs=(w16.nbytes - 2, 0))),
        ('a 16-bit raster at an odd offset', dict(offs=(0, 9))),
        ('no offsets', dict(offs=None)),
        ('no files', dict(files=None)),
        ('no shapes', dict(shapes=None)),
        ('no status', dict(status=None)),
        ('a negative dst_bytes', dict(dst_bytes=-1)),
    ]
    for what, kw in bad:
        assert call(**kw) == -1, what
        assert 'tiff_decode_batch' in lib.ecseg_last_error(gpu.h).decode(), what
        assert (dst == SENTINEL).all(), what
    assert call(n=0) == 0 and call(n=0, files=None, dst=None, offs=None, shapes=None, status=None) == 0 and (dst == SENTINEL).all()
    assert call() == 0 and status.tolist() == [0, 0]
    assert np.array_equal(dst[:7], w8.reshape(-1)) and dst[7] == SENTINEL and np.array_equal(dst[8:8 + w16.nbytes].view(np.uint16), w16.reshape(-1))
    assert (dst[8 + w16.nbytes:] == SENTINEL).all()
    dst[:] = SENTINEL                                            # the rasters in the other order in the destination
    assert call(offs=(w16.nbytes + 1, 0)) == 0
    assert np.array_equal(dst[:w16.nbytes].view(np.uint16), w16.reshape(-1)) and np.array_equal(dst[w16.nbytes + 1:w16.nbytes + 8], w8.reshape(-1))


def test_one_handle_two_different_batches_and_byte_identical_repeats(gpu, pool):
    """The call arena is carved anew for every batch: a large batch, a small one, the large one again, each twice."""
    large = [pool[k] for k in range(0, len(pool), 9)]
    small = [pool[k] for k in (860, 2)]
    first = {}
    for which, batch in (('large', large), ('small', small), ('large', large), ('small', small)):
        got = gpu.tiff_decode_many([d for _, d, _ in batch])
        for (name, _, want), g in zip(batch, got):
            assert same(g, want), (which, name)
        raw = [g.tobytes() for g in got]
        assert first.setdefault(which, raw) == raw, 'a repeat gives other bytes'


def test_a_lowered_budget_splits_the_batch_into_several_calls(gpu, pool, monkeypatch):
    batch = [pool[k] for k in range(3, len(pool), 29)]
    datas = [d for _, d, _ in batch]
    calls = []
    packed = gpu.tiff_decode_packed

    def counting(files, ranges, dst=None, dst_offsets=None):
        if dst is not None:
            calls.append(len(ranges))
        return packed(files, ranges, dst, dst_offsets)
    monkeypatch.setattr(gpu, 'tiff_decode_packed', counting)
    whole = gpu.tiff_decode_many(datas)
    assert calls == [len(batch)]
    del calls[:]
    buf, tab = _packed(datas)
    need = load_library().ecseg_tiff_decode_batch_bytes(buf.ctypes.data_as(C.c_void_p), buf.size, tab.ctypes.data_as(C.c_void_p), len(tab), 0)
    assert need > 6 * 256
    split = gpu.tiff_decode_many(datas, budget_bytes=need // 3)
    assert len(calls) >= 3 and sum(calls) == len(batch), calls
    del calls[:]
    alone = gpu.tiff_decode_many(datas, budget_bytes=1)          # a file that exceeds the budget alone goes alone
    assert calls == [1] * len(batch)
    for (name, _, want), a, b, c in zip(batch, whole, split, alone):
        assert same(a, want) and same(b, want) and same(c, want), name


def test_the_opencv_written_example_twice_in_one_batch(gpu):
    path = os.path.join(GOLDEN, 'dapi_example.tif')
    want = image_io._native_tiff(path)
    data = open(path, 'rb').read()
    got = gpu.tiff_decode_many([data, data])
    assert want.shape == (1040, 1392) and same(got[0], want) and same(got[1], want) and same(gpu.tiff_decode(data), want)


def test_imread_many_sends_a_set_of_1040_strips_and_keeps_one_of_1039(gpu, tmp_path):
    class Counting:
        def __init__(self):
            self.calls = []

        def tiff_decode_many(self, datas):
            self.calls.append(len(datas))
            return gpu.tiff_decode_many(datas)

    rng = np.random.default_rng(11)
    paths = []
    for k, rows in enumerate((208, 208, 208, 208, 207, 1)):
        img = rng.integers(0, 4, (rows, 8), dtype=np.uint8)
        p = str(tmp_path / ('f%d.tif' % k))
        image_io.write_file_image(p, dc.tiff_file([dc.pack(dc.lzw_codes(r.tobytes())) for r in img], rows, 8, 1))
        paths.append(p)
    raw = str(tmp_path / 'raw.tif')
    image_io.write_file_image(raw, dc.tiff_file([bytes(range(12))], 3, 4, 3, compression=1))
    for subset, sent in ((paths + [raw], [6]), (paths[:5] + [raw], [])):
        handle = Counting()
        got = image_io.imread_many(subset, handle=handle)
        assert handle.calls == sent
        for p, g in zip(subset, got):
            assert same(g, image_io.imread(p)), p


def test_make_stat_fish_writes_the_same_bytes_with_tiff_read_batch_4_and_1(gpu, tmp_path, monkeypatch, capsys):
    """The small-scene folder with both keys; every set is sent (the rule is replaced: the small files would stay on the host)."""
    import shutil
    inp, _ = cpu.make_folder(tmp_path, size=(67, 93))            # a_u16.npy, b_tif.tif, c_u8.npy
    for name in ('d_tif', 'e_tif'):                              # and the TIFF scene twice more
        shutil.copyfile(inp / 'b_tif.tif', inp / (name + '.tif'))
        shutil.copyfile(inp / 'nuclei_masks' / 'b_tif.tif', inp / 'nuclei_masks' / (name + '.tif'))
    monkeypatch.chdir(tmp_path)
    monkeypatch.setattr(image_io, 'tiff_goes_to_device', lambda data: True)
    monkeypatch.setattr(image_io, 'tiff_batch_goes_to_device', lambda datas: (True, [True] * len(datas)))
    sent = []
    many = gpu.tiff_decode_many

    def counting(datas, **kw):
        sent.append(len(datas))
        return many(datas, **kw)
    monkeypatch.setattr(gpu, 'tiff_decode_many', counting)

    def run(**keys):
        cfg = yaml.safe_load(open(tmp_path / 'config.yaml'))
        cfg['stat_fish'].update(tiff_read_on_device=True, **keys)
        yaml.safe_dump(cfg, open(tmp_path / 'config.yaml', 'w'))
        sf.main([], handle=gpu)
        return cpu.folder_bytes(inp / 'annotated'), capsys.readouterr().out

    want, said = run(tiff_read_batch=1)
    assert not sent
    got, out = run(tiff_read_batch=4)
    from ecseg_amd.utils import get_imgs
    order = get_imgs(str(inp))                                   # the images as main() takes them, four at a time
    assert len(order) == 5
    assert sent == [sum(p.endswith('.tif') for p in order[at:at + 4]) + len(order[at:at + 4]) for at in (0, 4)], \
        'the TIFF images and the masks of a chunk in one call'
    assert sorted(got) == sorted(want) and len(want) > 5 * 4 and out == said
    for f in want:
        assert got[f] == want[f], f
