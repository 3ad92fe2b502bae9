"""Tiled TIFF files decoded on the device (tiffb_untile_kernel, csrc/tiff_untile.h) behind the handle option ``tiff_tiled_on_device``.
Every expected value is the pure-Python reader's (image_io.read_tiff(native=False)) on the same bytes: its samples byte for byte, and
its verdict - ECSEG_E_INVALID (-1) where it raises on a tile's stream (TiffError for LZW, zlib.error for Deflate), ECSEG_E_UNSUPPORTED
(-5) for a file the parser leaves to it (a short tile table, where it raises IndexError).  The images are tiny; the cases are those of
tests/tiff_tiles_cases.py, which tests/test_tiff_tiles.py holds to the Python reader and to tifffile-checked files on the CPU."""
import base64
import json
import os
import shutil
import sys

import numpy as np
import pytest
import yaml

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_stat_fish_aqua as cpu            # noqa: E402
import tiff_tiles_cases as tc                # noqa: E402
from ecseg_amd import image_io               # noqa: E402
from ecseg_amd import stat_fish as sf        # noqa: E402
from ecseg_amd._lib import EcsegError        # noqa: E402

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')


@pytest.fixture(scope='module')
def cases(tmp_path_factory):
    """(name, file bytes, the Python reader's array) of every case, computed once."""
    tmp = tmp_path_factory.mktemp('tiles')
    out = []
    for name, img, data in tc.all_cases():
        verdict, want = tc.python_verdict(data, tmp)
        assert verdict == 'ok' and np.array_equal(want, tc.squeeze(img)), name
        out.append((name, data, want))
    files = json.load(open(os.path.join(GOLDEN, 'io_tiff_files.json')))['files']
    for name in ('rgb8_tiled16', 'gray16_tiled32_pred'):                # written by tifffile
        data = base64.b64decode(files[name])
        verdict, want = tc.python_verdict(data, tmp)
        assert verdict == 'ok'
        out.append((name, data, want))
    return out


@pytest.fixture()
def tiled(gpu):
    gpu.set_option('tiff_tiled_on_device', 1)
    gpu.set_option('tiff_deflate_on_device', 1)
    try:
        yield gpu
    finally:
        gpu.set_option('tiff_tiled_on_device', 0)
        gpu.set_option('tiff_deflate_on_device', 0)


def same(a, b):
    return isinstance(a, np.ndarray) and a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def test_every_extent_sample_kind_and_coding_alone_equals_the_python_reader(tiled, cases):
    assert len(cases) == 2 * 7 * 5 * 3 + 2
    for name, data, want in cases:
        got = tiled.tiff_decode(data)
        assert same(got, want), name


def test_with_the_option_off_tiled_files_are_left_to_the_host_without_a_shape(gpu, cases):
    gpu.set_option('tiff_deflate_on_device', 1)
    try:
        picked = cases[::7] + cases[-2:]
        for name, data, _ in picked:
            assert gpu.tiff_decode(data) is None, name
        buf, ranges = image_io.pack_file_images([np.frombuffer(d, np.uint8) for _, d, _ in picked])
        dst = np.full(1 << 20, 0xA5, np.uint8)
        shapes, status = gpu.tiff_decode_packed(buf, ranges, dst, np.arange(len(picked)) * 2)
        assert (status == -5).all() and not shapes.any() and (dst == 0xA5).all()
        assert all(a is None for a in gpu.tiff_decode_many([d for _, d, _ in picked]))
    finally:
        gpu.set_option('tiff_deflate_on_device', 0)


def _strip_files():
    """Files of strips for the mixed batches: LZW and uncompressed, written by the project's own writers."""
    import tempfile
    out = []
    with tempfile.TemporaryDirectory() as tmp:
        for k, (H, W) in enumerate(((37, 53), (5, 300))):
            img = tc.pixels('gray8', H, W, seed=9 + k)[..., 0]
            path = os.path.join(tmp, 's%d.tif' % k)
            image_io.write_tiff_gray8(path, img)
            out.append(('strips_gray8_%d' % k, open(path, 'rb').read(), img))
    return out


def _packed(handle, files, order, gap):
    """One ecseg_tiff_decode_batch over ``files`` in ``order`` with ``gap`` sentinel bytes between the rasters -> per file the array,
    or its status; asserts that nothing outside the rasters of the clean files changed."""
    files = [files[k] for k in order]
    buf, ranges = image_io.pack_file_images([np.frombuffer(d, np.uint8) for _, d, _ in files])
    shapes, status = handle.tiff_decode_packed(buf, ranges)
    sizes = [int(H) * W * spp * (bits // 8) for H, W, spp, bits in shapes.tolist()]
    offs, end = [], 3
    for k, n in enumerate(sizes):
        end += gap + k % 3
        end += end & 1
        offs.append(end)
        end += n
    dst = np.full(end + 9, 0xA5, np.uint8)
    shapes2, status = handle.tiff_decode_packed(buf, ranges, dst, offs)
    assert np.array_equal(shapes, shapes2)
    keep = np.ones(dst.size, bool)
    out = {}
    for (name, _, _), (H, W, spp, bits), off, n, st in zip(files, shapes.tolist(), offs, sizes, status.tolist()):
        if st == 0:
            a = dst[off:off + n].view(np.uint8 if bits == 8 else np.uint16).reshape(H, W, spp)
            out[name] = a[..., 0] if spp == 1 else a
            keep[off:off + n] = False
        else:
            out[name] = st
    assert (dst[keep] == 0xA5).all(), 'a byte outside the rasters of the clean files changed'
    return out


def test_one_batch_mixes_tiled_and_strip_files_forwards_and_reversed_with_gaps(tiled, cases):
    files = cases[3::11] + cases[-2:] + _strip_files()
    assert any('_raw_' in n for n, _, _ in files) and any('_lzw_' in n for n, _, _ in files) and any('_deflate_' in n for n, _, _ in files)
    n = len(files)
    for order, gap in ((list(range(n)), 0), (list(range(n))[::-1], 5), (list(range(1, n, 2)) + list(range(0, n, 2)), 33)):
        got = _packed(tiled, files, order, gap)
        for name, _, want in files:
            assert same(got[name], want), (name, gap)
    many = tiled.tiff_decode_many([d for _, d, _ in files])
    for (name, _, want), g in zip(files, many):
        assert same(g, want), name


def test_a_damaged_or_refused_file_gets_the_python_verdict_and_disturbs_no_neighbour(tiled, cases, tmp_path):
    damaged = tc.damaged_cases()
    refused = tc.refused_cases()
    neighbours = cases[5::41] + _strip_files()
    solo = {name: tiled.tiff_decode(data) for name, data, _ in neighbours}
    for (name, _, want) in neighbours:
        assert same(solo[name], want), name
    bad = [(name, data) for name, (_, data, _) in damaged.items()] + [('short_tile_table', refused['short_tile_table'])]
    files, want_status = [], {}
    for k, (name, data) in enumerate(bad):
        verdict, ref = tc.python_verdict(data, tmp_path, name)
        want_status[name] = ref if verdict == 'ok' else -5 if isinstance(ref, IndexError) else -1
        files.append((name, data, None))
        files.append(neighbours[k % len(neighbours)])       # a neighbour behind every bad file
    files = [(('%s#%d' % (n, k)) if w is not None else n, d, w) for k, (n, d, w) in enumerate(files)]
    assert sorted(v for v in want_status.values() if isinstance(v, int)) == [-5, -1, -1, -1, -1] and len(want_status) == 8
    for order in (list(range(len(files))), list(range(len(files)))[::-1]):
        got = _packed(tiled, files, order, 7)
        for name, data, want in files:
            if want is not None:
                assert same(got[name], want) and same(got[name], solo[name.split('#')[0]]), name
            elif isinstance(want_status[name], int):
                assert isinstance(got[name], int) and got[name] == want_status[name], (name, got[name])
            else:
                assert same(got[name], want_status[name]), name
    for name, data in bad:                                              # and alone
        if isinstance(want_status[name], np.ndarray):
            assert same(tiled.tiff_decode(data), want_status[name]), name
        elif want_status[name] == -5:
            assert tiled.tiff_decode(data) is None, name
        else:
            with pytest.raises(EcsegError) as e:
                tiled.tiff_decode(data)
            assert e.value.code == -1 and 'tile' in str(e.value), name
    for name, data in refused.items():
        assert tiled.tiff_decode(data) is None, name


def test_arena_reuse_poisoned_arenas_and_repeats_give_identical_bytes(tiled, cases):
    big = [c for c in cases if c[0].split('_')[1] == '130x257']
    small = _strip_files()[:1]
    assert len(big) == 60

    def run(files):
        return [a.tobytes() if isinstance(a, np.ndarray) else a for a in tiled.tiff_decode_many([d for _, d, _ in files])]
    first = run(big)
    assert all(isinstance(b, bytes) for b in first) and first == [w.tobytes() for _, _, w in big]
    assert run(small) == [small[0][2].tobytes()]
    assert run(big) == first, 'a large tiled batch behind a small one of strips on the same arena'
    tiled.scratch_fill_debug(0xFF)
    assert run(big) == first, 'on a poisoned arena'
    tiled.scratch_fill_debug(0xFF)
    assert run(small) == [small[0][2].tobytes()]
    assert run(big) == first and run(big) == first


def test_make_stat_fish_on_a_tiled_folder_is_the_same_with_the_key_on_and_off(gpu, tmp_path, monkeypatch, capsys):
    """Three images whose TIFF image and mask are rewritten as tiled files (LZW, predictor 2, 16 x 32 tiles); the rule is replaced so
    that every file is sent with the key on - by the measured rule none would be - one by one and as a chunk."""
    inp, _ = cpu.make_folder(tmp_path, kinds=(('a_tif', 'tif'),), size=(67, 93))
    for name in ('b_tif', 'c_tif'):
        shutil.copyfile(inp / 'a_tif.tif', inp / (name + '.tif'))
        shutil.copyfile(inp / 'nuclei_masks' / 'a_tif.tif', inp / 'nuclei_masks' / (name + '.tif'))
    n_files = 0
    for folder in (inp, inp / 'nuclei_masks'):
        for f in sorted(os.listdir(folder)):
            if f.endswith('.tif'):
                a = image_io.read_tiff(str(folder / f))
                image_io.write_file_image(str(folder / f), tc.tiled_tiff(a, 16, 32, 5, 2))
                assert np.array_equal(image_io.read_tiff(str(folder / f)), a)
                n_files += 1
    assert n_files == 6
    monkeypatch.chdir(tmp_path)
    monkeypatch.setattr(image_io, 'tiff_goes_to_device', lambda data, deflate=False, tiled=False: True)
    monkeypatch.setattr(image_io, 'tiff_batch_goes_to_device', lambda datas, deflate=False, tiled=False: (True, [True] * len(datas)))
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
        for k in ('tiff_read_on_device', 'tiff_read_batch', 'tiff_read_tiled'):
            cfg['stat_fish'].pop(k, None)
        cfg['stat_fish'].update(keys)
        yaml.safe_dump(cfg, open(tmp_path / 'config.yaml', 'w'))
        del arrays[:]
        try:
            sf.main([], handle=gpu)
            code = 0
        except SystemExit as e:
            code = e.code
        assert not getattr(gpu, 'tiff_tiled_on_device', False), 'the handle comes back as it went in'
        return cpu.folder_bytes(inp / 'annotated'), capsys.readouterr().out, sum(arrays), code

    want, said, n, code = run()
    assert n == 0 and len(want) > 3 * 4 and not code
    for keys, decoded in ((dict(tiff_read_on_device=True), 0), (dict(tiff_read_on_device=True, tiff_read_tiled=True), 6),
                          (dict(tiff_read_on_device=True, tiff_read_tiled=True, tiff_read_batch=3), 6), (dict(tiff_read_tiled=True), 0)):
        got, out, n, c = run(**keys)
        assert n == decoded, (keys, n)
        assert out == said and c == code and sorted(got) == sorted(want), keys
        for f in want:
            assert got[f] == want[f], (keys, f)
    shutil.rmtree(inp / 'annotated')
