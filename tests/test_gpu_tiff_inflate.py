"""Deflate strips decoded on the device (tiffb_inflate_kernel, csrc/tiff_inflate_strip.h) behind the handle option
``tiff_deflate_on_device``.  Every expected value is the host reader's (ecseg_tiff_info + ecseg_tiff_read on the same bytes); the one
class that depends on the zlib version (a stream that ends before the strip is full and before its own end) is held to the stated
rule, corrupt.  The images are tiny; the corpus is the one tests/test_tiff_inflate.py runs under the sanitizers on the host."""
import os
import shutil
import sys
import zlib

import numpy as np
import pytest
import yaml

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_stat_fish_aqua as cpu            # noqa: E402
import tiff_decode_cases as dc               # noqa: E402
import tiff_inflate_cases as ic              # noqa: E402
from ecseg_amd import image_io               # noqa: E402
from ecseg_amd import stat_fish as sf        # noqa: E402
from ecseg_amd._lib import EcsegError        # noqa: E402

pytestmark = pytest.mark.gpu


def make_file(seed, H, W, rps, spp, bits, big_endian, predictor, codec, level=6):
    """A file of ``dc.tiff_file`` around seeded samples: strips of ``rps`` rows, differenced where the predictor is on, in the file's
    byte order; codec 8 / 32946: every strip a zlib stream, 5: LZW, 1: as they are."""
    rng = np.random.default_rng(seed)
    top = 6 if seed % 2 else (256 if bits == 8 else 65536)       # long matches or noise
    img = rng.integers(0, top, (H, W, spp), dtype=np.uint16 if bits == 16 else np.uint8)
    stored = img
    if predictor:
        stored = img.copy()
        stored[:, 1:] = img[:, 1:] - img[:, :-1]
    stored = stored.astype(('>' if big_endian else '<') + ('u2' if bits == 16 else 'u1'))
    strips = [stored[r:r + rps].tobytes() for r in range(0, H, rps)]
    if codec in (8, 32946):
        strips = [zlib.compress(s, level) for s in strips]
    elif codec == 5:
        strips = [dc.pack(dc.lzw_codes(s)) for s in strips]
    return dc.tiff_file(strips, H, W, rps, spp=spp, bits=bits, compression=codec, predictor=2 if predictor else 1, big_endian=big_endian)


def host_read(data, tmp):
    path = os.path.join(str(tmp), 'host.tif')
    image_io.write_file_image(path, data)
    try:
        return image_io._native_tiff(path)
    except image_io.TiffError:
        return 'invalid'


def same(a, b):
    if isinstance(a, str) or isinstance(b, str):
        return isinstance(a, str) and isinstance(b, str) and a == b
    return a is not None and b is not None and a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b)


def plain(got):
    if isinstance(got, EcsegError):
        assert got.code == -1, got
        return 'invalid'
    assert not isinstance(got, Exception), got
    return got


def decode(gpu, data):
    try:
        return gpu.tiff_decode(data, deflate=True)
    except EcsegError as e:
        assert e.code == -1, e
        return 'invalid'


@pytest.fixture(scope='module')
def pool(tmp_path_factory):
    """[(name, file bytes, host reader's samples)]: 37 x 23 RGB and 41 x 43 gray at 1 to 5 rows per strip, both compression tags,
    predictor 1 and 2, 8 bit and 16 bit big-endian, levels 0 / 1 / 9: computed once and never changed."""
    tmp = tmp_path_factory.mktemp('pool')
    out, seed = [], 0
    for H, W, spp in ((23, 37, 3), (43, 41, 1)):
        for rps in (1, 2, 3, 4, 5):
            for bits, big in ((8, False), (16, True)):
                for pred in (False, True):
                    seed += 1
                    tag = 32946 if seed % 3 == 0 else 8
                    data = make_file(seed, H, W, rps, spp, bits, big, pred, tag, level=(0, 1, 9, 6)[seed % 4])
                    want = host_read(data, tmp)
                    assert isinstance(want, np.ndarray) and want.shape[:2] == (H, W)
                    out.append(('%dx%dx%d_rps%d_%dbit_pred%d_tag%d' % (H, W, spp, rps, bits, pred, tag), data, want))
    assert len(out) == 40 and {n.split('tag')[1] for n, _, _ in out} == {'8', '32946'}
    return out


def test_every_file_of_the_pool_alone_and_unsupported_with_the_option_off(gpu, pool):
    for name, data, want in pool:
        assert same(decode(gpu, data), want), name
    name, data, want = pool[0]
    assert gpu.tiff_decode(data) is None and gpu.tiff_decode(data, deflate=False) is None, 'with the option off a Deflate file is left to the host'
    buf = np.frombuffer(data, np.uint8)
    shapes, status = gpu.tiff_decode_packed(buf, [[0, buf.size]])
    assert status.tolist() == [-5] and shapes.tolist()[0][:2] == list(want.shape[:2])
    got = gpu.tiff_decode_many([data, pool[1][1]])
    assert got == [None, None]
    gpu.set_option('tiff_deflate_on_device', 1)
    try:
        assert same(gpu.tiff_decode(data), want)
        shapes, status = gpu.tiff_decode_packed(buf, [[0, buf.size]])
        assert status.tolist() == [0]
        assert gpu.tiff_decode(data, deflate=False) is None and same(gpu.tiff_decode(data), want), 'the argument holds for one call'
    finally:
        gpu.set_option('tiff_deflate_on_device', 0)
    assert gpu.tiff_decode(data) is None


def _one_strip(stream, want):
    return dc.tiff_file([stream], 1, want, 1, compression=8)


def test_the_corpus_of_hand_built_streams_zlib_streams_and_mutations(gpu, tmp_path):
    """Every stream as the one strip of a gray file, all of them in two calls: short and long streams, the 32 KiB-distance strip,
    every corrupt class, seeded mutations.  Each file is what the host reader makes of it, the truncated class corrupt by rule."""
    cases = ic.hand_cases() + ic.zlib_streams()
    files = [(name, _one_strip(s, w), cls) for name, s, w, cls, _ in cases] + [(name, _one_strip(s, w), None) for name, s, w in ic.mutations()]
    wants = []
    for (name, data, cls), case in zip(files, cases + [None] * len(files)):
        want = 'invalid' if cls == ic.TRUNCATED else host_read(data, tmp_path)
        if cls is not None:
            assert isinstance(want, str) == cls.startswith('corrupt'), name
            if case[4] is not None and not isinstance(want, str):
                assert want.tobytes() == (case[4] + bytes(case[2]))[:case[2]], name
        wants.append(want)
    got = gpu.tiff_decode_many([d for _, d, _ in files], deflate=True)
    old_zlib = []
    for (name, _, cls), g, want in zip(files, got, wants):
        if cls is None and not same(plain(g), want) and isinstance(plain(g), str):
            old_zlib.append(name)                                 # a mutation of the truncated class under a zlib before 1.2.9: the rule says corrupt
            continue
        assert same(plain(g), want), name
    assert not old_zlib or tuple(int(v) for v in zlib.ZLIB_RUNTIME_VERSION.split('.')[:3]) < (1, 2, 9), old_zlib
    assert sum(isinstance(w, str) for w in wants) > 60 and sum(not isinstance(w, str) for w in wants) > 60
    for k in (0, 6, len(cases) - 1):                             # and alone, through the single-file call
        assert same(decode(gpu, files[k][1]), wants[k]), files[k][0]


@pytest.fixture(scope='module')
def mixed(pool, tmp_path_factory):
    """Deflate, LZW and uncompressed files, 18 in all, with the host reader's samples."""
    tmp = tmp_path_factory.mktemp('mixed')
    out = [pool[k] for k in (0, 5, 9, 14, 21, 27, 33, 38)]
    for k, (H, W, rps, spp, bits, big, pred, codec) in enumerate((
            (23, 37, 2, 3, 8, False, True, 5), (43, 41, 5, 1, 16, True, True, 5), (7, 65, 1, 1, 8, False, False, 5), (23, 37, 4, 3, 16, False, False, 5),
            (43, 41, 3, 1, 8, False, True, 1), (5, 9, 2, 4, 16, True, False, 1), (1, 1, 1, 1, 8, False, False, 1), (23, 37, 23, 3, 8, False, False, 1),
            (1, 1, 1, 1, 8, False, False, 8), (3, 64, 3, 1, 16, True, True, 32946))):
        data = make_file(100 + k, H, W, rps, spp, bits, big, pred, codec)
        out.append(('mixed_%d_codec%d' % (k, codec), data, host_read(data, tmp)))
    assert all(isinstance(w, np.ndarray) for _, _, w in out)
    return out


def _corrupt_deflate(pool):
    """A pool file with the Adler-32 of its second strip's stream changed: the device finds it, and only there."""
    name, data, want = pool[4]
    b = bytearray(data)
    (s0, n0), (s1, n1) = [(off, cnt) for off, cnt in _strip_ranges(data)][:2]
    b[s1 + n1 - 1] ^= 0x40
    return ('corrupt_' + name, bytes(b), 'invalid')


def _strip_ranges(data):
    import struct
    ifd = struct.unpack_from('<I', data, 4)[0]
    tags = {}
    for k in range(struct.unpack_from('<H', data, ifd)[0]):
        tag, typ, count, value = struct.unpack_from('<HHII', data, ifd + 2 + 12 * k)
        tags[tag] = (typ, count, value)

    def values(tag):
        typ, count, value = tags[tag]
        if count == 1:
            return [value & 0xffff if typ == 3 else value]
        return list(struct.unpack_from('<%d%s' % (count, 'H' if typ == 3 else 'I'), data, value))
    return list(zip(values(273), values(279)))


def test_mixed_batches_in_three_orders_with_a_corrupt_deflate_file_first_last_and_in_the_middle(gpu, mixed, pool, tmp_path):
    bad = _corrupt_deflate(pool)
    assert host_read(bad[1], tmp_path) == 'invalid'
    n = len(mixed)
    for order in (mixed, mixed[::-1], mixed[n // 3:] + mixed[:n // 3]):
        for at in (0, n, n // 2):
            files = order[:at] + [bad] + order[at:]
            got = gpu.tiff_decode_many([d for _, d, _ in files], deflate=True)
            for (name, _, want), g in zip(files, got):
                assert same(plain(g), want), (name, at)
    got = gpu.tiff_decode_many([d for _, d, _ in mixed])         # the option off: the Deflate files are None, the others decoded
    for (name, data, want), g in zip(mixed, got):
        assert (g is None) if ('tag' in name or name.endswith(('codec8', 'codec32946'))) else same(g, want), name


def test_gaps_between_the_rasters_stay_untouched_and_repeats_are_byte_identical(gpu, mixed, pool):
    files = mixed + [_corrupt_deflate(pool)]
    buf, ranges = image_io.pack_file_images([np.frombuffer(d, np.uint8) for _, d, _ in files])
    sizes = [pool[4][2].nbytes if isinstance(w, str) else w.nbytes for _, _, w in files]   # (the corrupt file is found on the device: it has its room)
    offs, end = [], 3
    for k, n in enumerate(sizes):
        end += 5 + k % 3
        end += end & 1
        offs.append(end)
        end += n
    gpu.set_option('tiff_deflate_on_device', 1)
    try:
        outs = []
        for _ in range(3):
            dst = np.full(end + 9, 0xA5, np.uint8)
            shapes, status = gpu.tiff_decode_packed(buf, ranges, dst, offs)
            outs.append((dst, shapes.copy(), status.copy()))
    finally:
        gpu.set_option('tiff_deflate_on_device', 0)
    dst, shapes, status = outs[0]
    assert status.tolist() == [0] * len(mixed) + [-1]
    keep = np.ones(dst.size, bool)
    for (name, _, want), off, n, st in zip(files, offs, sizes, status.tolist()):
        if st == 0:
            assert dst[off:off + n].tobytes() == want.tobytes(), name
        keep[off:off + n] = False
    bad_off = offs[-1]
    keep[bad_off:bad_off + pool[4][2].nbytes] = False            # (the corrupt file's raster is not copied back: it holds the sentinel)
    assert (dst[bad_off:bad_off + pool[4][2].nbytes] == 0xA5).all() and (dst[keep] == 0xA5).all()
    for other, s2, st2 in outs[1:]:
        assert other.tobytes() == dst.tobytes() and np.array_equal(s2, shapes) and np.array_equal(st2, status)


def test_imread_and_imread_many_with_the_switch(gpu, pool, tmp_path, monkeypatch):
    paths = []
    for k, (name, data, _) in enumerate(pool[:6]):
        p = str(tmp_path / ('%d.tif' % k))
        image_io.write_file_image(p, data)
        paths.append(p)
    # every set is sent (the rule is replaced: these tiny files stay on the host by the measured one)
    monkeypatch.setattr(image_io, 'tiff_batch_goes_to_device', lambda datas, deflate=False: (True, [True] * len(datas)))
    monkeypatch.setattr(image_io, 'tiff_goes_to_device', lambda data, deflate=False: True)
    decoded = []
    many, one = gpu.tiff_decode_many, gpu.tiff_decode
    monkeypatch.setattr(gpu, 'tiff_decode_many', lambda datas, **kw: decoded.append(('many', len(datas), kw)) or many(datas, **kw))
    monkeypatch.setattr(gpu, 'tiff_decode', lambda data, **kw: decoded.append(('one', kw)) or one(data, **kw))
    got = image_io.imread_many(paths, handle=gpu, deflate=True)
    assert decoded == [('many', 6, dict(deflate=True))]
    for (name, _, want), g in zip(pool, got):
        assert same(g, want), name
    got = image_io.imread_many(paths, handle=gpu)               # without the switch the device answers None and the host reads them
    for (name, _, want), g in zip(pool, got):
        assert same(g, want), name
    del decoded[:]
    assert same(image_io.imread(paths[2], handle=gpu, deflate=True), pool[2][2]) and decoded == [('one', dict(deflate=True))]
    assert same(image_io.imread(paths[2], handle=gpu), pool[2][2])


def test_make_stat_fish_writes_the_same_bytes_with_tiff_read_deflate_on_and_off(gpu, tmp_path, monkeypatch, capsys):
    """A four-image folder whose TIFF image and masks are rewritten with Deflate strips; the rule is replaced so that every file is
    sent, one by one and as chunks of four."""
    inp, _ = cpu.make_folder(tmp_path, kinds=(('a_tif', 'tif'),), size=(67, 93))
    for name in ('b_tif', 'c_tif', 'd_tif'):                     # the TIFF scene three times more
        shutil.copyfile(inp / 'a_tif.tif', inp / (name + '.tif'))
        shutil.copyfile(inp / 'nuclei_masks' / 'a_tif.tif', inp / 'nuclei_masks' / (name + '.tif'))
    n_files = 0
    for folder in (inp, inp / 'nuclei_masks'):
        for f in sorted(os.listdir(folder)):
            if f.endswith('.tif'):
                a = image_io.read_tiff(str(folder / f))
                a3 = a if a.ndim == 3 else a[..., None]
                strips = [zlib.compress(a3[r:r + 5].tobytes()) for r in range(0, a3.shape[0], 5)]
                image_io.write_file_image(str(folder / f), dc.tiff_file(strips, a3.shape[0], a3.shape[1], 5, spp=a3.shape[2], compression=8))
                assert np.array_equal(image_io.read_tiff(str(folder / f)), a)
                n_files += 1
    assert n_files == 8
    monkeypatch.chdir(tmp_path)
    monkeypatch.setattr(image_io, 'tiff_goes_to_device', lambda data, deflate=False: True)
    monkeypatch.setattr(image_io, 'tiff_batch_goes_to_device', lambda datas, deflate=False: (True, [True] * len(datas)))
    arrays = []
    many, one = gpu.tiff_decode_many, gpu.tiff_decode

    def counting_many(datas, **kw):
        out = many(datas, **kw)
        arrays.append(sum(isinstance(a, np.ndarray) for a in out))
        return out

    def counting_one(data, **kw):
        out = one(data, **kw)
        arrays.append(int(isinstance(out, np.ndarray)))
        return out
    monkeypatch.setattr(gpu, 'tiff_decode_many', counting_many)
    monkeypatch.setattr(gpu, 'tiff_decode', counting_one)

    def run(**keys):
        cfg = yaml.safe_load(open(tmp_path / 'config.yaml'))
        for k in ('tiff_read_on_device', 'tiff_read_batch', 'tiff_read_deflate'):
            cfg['stat_fish'].pop(k, None)
        cfg['stat_fish'].update(keys)
        yaml.safe_dump(cfg, open(tmp_path / 'config.yaml', 'w'))
        del arrays[:]
        sf.main([], handle=gpu)
        return cpu.folder_bytes(inp / 'annotated'), capsys.readouterr().out, sum(arrays)

    want, said, n = run()
    assert n == 0 and len(want) > 4 * 4
    for keys, decoded in ((dict(tiff_read_on_device=True), 0), (dict(tiff_read_on_device=True, tiff_read_deflate=False), 0),
                          (dict(tiff_read_on_device=True, tiff_read_deflate=True), 8),
                          (dict(tiff_read_on_device=True, tiff_read_deflate=True, tiff_read_batch=4), 8), (dict(tiff_read_deflate=True), 0)):
        got, out, n = run(**keys)
        assert n == decoded, (keys, n)
        assert out == said and sorted(got) == sorted(want), keys
        for f in want:
            assert got[f] == want[f], (keys, f)
    shutil.rmtree(inp / 'annotated')
