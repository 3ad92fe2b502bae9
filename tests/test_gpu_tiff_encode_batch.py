"""The batched device TIFF encoder (the tiffb_* kernels of csrc/tiff_kernels.hip) on the device: every case and every batch of
tests/tiff_encode_batch_cases.py through ``Handle.tiff_encode_many`` against the host writers' files and ``Handle.tiff_encode`` of each
raster alone, byte for byte; the argument rules of ecseg_tiff_encode_batch on poisoned buffers; ``Handle.fish_render_tiff_many``
against ``fish_render_tiff`` + ``tiff_encode`` per image; ``make stat_fish`` at ``tiff_write_batch`` 1, 2 and 8."""
import ctypes as C
import os
import shutil
import sys

import numpy as np
import pytest
import yaml

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_stat_fish_aqua as cpu            # noqa: E402
import tiff_encode_batch_cases as bc         # noqa: E402
from ecseg_amd import image_io               # noqa: E402
from ecseg_amd import stat_fish as sf        # noqa: E402
from ecseg_amd._lib import EcsegError, load_library   # noqa: E402

pytestmark = pytest.mark.gpu
_HOST, _ALONE = {}, {}


def host_file(case, tmp_path_factory):
    """The file the host writer puts on disk for a case, written once for the tests that need it."""
    if case.name not in _HOST:
        path = str(tmp_path_factory.mktemp('host') / 'h.tif')
        if bc.spp(case) == 1:
            image_io.write_tiff_gray8(path, case.img, invert=case.invert)
        else:
            image_io.write_tiff_rgb8(path, case.img)
        _HOST[case.name] = open(path, 'rb').read()
    return _HOST[case.name]


def alone(gpu, case):
    """``Handle.tiff_encode`` of a case's raster alone, computed once."""
    if case.name not in _ALONE:
        _ALONE[case.name] = gpu.tiff_encode(case.img, invert=case.invert)
    return _ALONE[case.name]


def _many(gpu, cases, **kw):
    return gpu.tiff_encode_many([c.img for c in cases], [c.invert for c in cases], **kw)


def _check(gpu, cases, files, tmp_path_factory):
    assert len(files) == len(cases)
    for k, (c, f) in enumerate(zip(cases, files)):
        want = host_file(c, tmp_path_factory)
        assert isinstance(f, bytes) and len(f) == len(want), (k, c.name, len(f), len(want))
        assert f == want, '%s (file %d): first difference at byte %d of %d' % (c.name, k, next(i for i, (a, b) in enumerate(zip(f, want)) if a != b), len(want))
        assert f == alone(gpu, c), c.name


@pytest.mark.parametrize('case', bc.CASES, ids=[c.name for c in bc.CASES])
def test_a_batch_of_one_is_the_host_file_and_the_single_call(gpu, case, tmp_path_factory):
    _check(gpu, [case], _many(gpu, [case]), tmp_path_factory)
    assert 0 < gpu.timings()['count'] < 10000


@pytest.mark.parametrize('name', sorted(bc.BATCHES), ids=sorted(bc.BATCHES))
def test_every_file_of_a_batch_is_the_host_file_and_the_single_call(gpu, name, tmp_path_factory):
    cases = [bc.CASES[i] for i in bc.BATCHES[name]]
    _check(gpu, cases, _many(gpu, cases), tmp_path_factory)


def test_permuting_a_batch_permutes_the_files_and_changes_no_byte(gpu):
    a, b = bc.BATCHES['17_files'], bc.BATCHES['17_files_shuffled']
    fa = _many(gpu, [bc.CASES[i] for i in a])
    fb = _many(gpu, [bc.CASES[i] for i in b])
    by_case = {}
    for i, f in zip(a, fa):
        assert by_case.setdefault(i, f) == f
    assert [by_case[i] for i in b] == fb


def test_gaps_between_the_rasters_change_nothing(gpu, tmp_path_factory):
    cases = [bc.CASES[i] for i in bc.BATCHES['8_files_shuffled']]
    buf, tab = bc.pack(cases, gaps=[5, 0, 1, 300, 0, 7, 2, 64])
    out, ranges = gpu.tiff_encode_packed(np.concatenate([buf, np.full(9, 0xEE, np.uint8)]), tab)
    assert ranges[0, 0] == 0 and (ranges[1:, 0] == ranges[:-1, 0] + ranges[:-1, 1]).all(), 'the files lie back to back'
    _check(gpu, cases, [out[o:o + n].tobytes() for o, n in ranges.tolist()], tmp_path_factory)


def test_the_empty_batch(gpu):
    assert gpu.tiff_encode_many([]) == []
    lib = load_library()
    out, ranges = np.full(16, 0xa5, np.uint8), np.full(2, -7, np.int64)
    assert lib.ecseg_tiff_encode_batch(gpu.h, None, 0, None, 0, None, 0, None) == 0
    assert lib.ecseg_tiff_encode_batch(gpu.h, None, 0, None, 0, out.ctypes.data, 16, ranges.ctypes.data) == 0
    assert (out == 0xa5).all() and (ranges == -7).all() and gpu.timings()['count'] == 0


def test_every_argument_error_leaves_the_poisoned_output_untouched(gpu, tmp_path_factory):
    lib = load_library()
    cases = [bc.CASES[i] for i in bc.BATCHES['3_files']]
    buf, tab = bc.pack(cases)
    want = b''.join(host_file(c, tmp_path_factory) for c in cases)
    out, ranges = np.full(len(want) + 64, 0xa5, np.uint8), np.full((3, 2), -7, np.int64)
    vp = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    n_raster = buf.size

    def call(buf=buf, nbytes=None, tab=tab, n=3, dst=out, cap=None, rng=ranges):
        rc = lib.ecseg_tiff_encode_batch(gpu.h, vp(buf), n_raster if nbytes is None else nbytes, vp(tab), n, vp(dst), out.size if cap is None else cap, vp(rng))
        assert (out == 0xa5).all() and (ranges == -7).all(), 'a refused call wrote into its output'
        return rc, lib.ecseg_last_error(gpu.h).decode()

    def row(k, col, v):
        t = tab.copy()
        t[k, col] = v
        return t
    assert call(buf=None)[0] == -1 and call(tab=None)[0] == -1 and call(dst=None)[0] == -1 and call(rng=None)[0] == -1
    assert call(n=-1)[0] == -1 and call(nbytes=-1)[0] == -1 and call(cap=-1)[0] == -1
    for t in (row(1, 1, 0), row(1, 2, -3), row(2, 3, 2), row(2, 3, 4), row(0, 3, 0), row(1, 2, 1 << 30)):
        rc, why = call(tab=t)
        assert rc == -1 and 'tiff_encode_batch: file' in why, why
    rc, why = call(tab=row(1, 0, tab[1, 0] - 1))
    assert rc == -1 and 'overlaps the one in front or leaves' in why
    rc, why = call(nbytes=buf.size - 1)
    assert rc == -1 and 'overlaps the one in front or leaves' in why
    rc, why = call(tab=np.zeros((65536, 5), np.int64), n=65536)
    assert rc == -1 and '65536 files or more' in why
    for cap in (len(want) - 1, 8, 0):                             # a capacity one byte short, and less
        rc, why = call(cap=cap)
        assert rc == -1 and 'do not fit the capacity' in why, (cap, why)
    with pytest.raises(EcsegError) as e:
        gpu.tiff_encode_packed(buf, tab, capacity=len(want) - 1)
    assert e.value.code == -1
    files, got = gpu.tiff_encode_packed(buf, tab, capacity=len(want))          # exactly enough is enough
    assert files[:len(want)].tobytes() == want and got.tolist() == [[sum(len(host_file(c, tmp_path_factory)) for c in cases[:k]), len(host_file(c, tmp_path_factory))]
                                                                    for k, c in enumerate(cases)]
    with pytest.raises(ValueError):
        gpu.tiff_encode_many([np.zeros((3, 3, 2), np.uint8)])
    with pytest.raises(ValueError):
        gpu.tiff_encode_many([np.zeros((3, 3), np.uint8)], inverts=[True, False])


def test_a_budget_that_splits_the_list_into_three_calls_gives_the_same_list(gpu, monkeypatch):
    cases = [bc.CASES[i] for i in bc.BATCHES['17_files']]
    whole = _many(gpu, cases)
    lib = load_library()
    needs = [lib.ecseg_tiff_encode_batch_bytes(np.array([[0, c.img.shape[0], c.img.shape[1], bc.spp(c), 0]], np.int64).ctypes.data, 1) for c in cases]
    assert all(n > 0 for n in needs)
    budget = next(b for b in range(max(needs), sum(needs), 256) if len(gpu._split_by_budget(needs, b)) == 3)
    calls = []
    packed = gpu.tiff_encode_packed
    monkeypatch.setattr(gpu, 'tiff_encode_packed', lambda buf, tab, **kw: calls.append(len(tab)) or packed(buf, tab, **kw))
    assert _many(gpu, cases, budget_bytes=budget) == whole
    assert len(calls) == 3 and sum(calls) == 17
    del calls[:]
    assert _many(gpu, cases[:4], budget_bytes=1) == whole[:4] and calls == [1, 1, 1, 1], 'an image that exceeds the budget alone goes alone'


def test_one_handle_runs_a_large_batch_a_tiny_one_and_the_large_one_again(gpu):
    large = [bc.CASES[i] for i in bc.BATCHES['17_files_shuffled']]
    first = _many(gpu, large)
    tiny = _many(gpu, [bc.CASES[0]])
    assert _many(gpu, large) == first and _many(gpu, [bc.CASES[0]]) == tiny


# ---- fish_render_tiff_many ----------------------------------------------------------------------------------------------------------
def _scene(H, W, C_, seed):
    rng = np.random.default_rng(seed)
    I = rng.integers(0, 256, (H, W, C_), dtype=np.uint8)
    I[H // 2:] //= 16                                        # a flat half: long matches beside the noise
    if C_ == 4:
        I[..., 3].flat[::3] = cpu.Q_GREEN
        I[..., 3].flat[1::3] = cpu.Q_RED
    thr = (rng.random((H, W, C_ - 1)) < 0.4).astype(np.uint8) * np.uint8(255)
    bnd = (rng.random((H, W)) < 0.3).astype(np.uint8) * np.uint8(255)
    mask = (rng.random((H, W)) < 0.5).astype(np.uint8) * np.uint8(255)
    picture = rng.integers(0, 4, (H, W, 3), dtype=np.uint8) * np.uint8(60)
    return I, ((2, 1, 0) if C_ == 3 else (2, 1, 0, 3)), thr, bnd, mask, picture


def test_fish_render_tiff_many_equals_fish_render_tiff_and_tiff_encode_per_image(gpu):
    """Three scenes of different extents, three- and four-channel, with and without the mask and the picture, in one call."""
    a, b, c = _scene(41, 43, 3, 1), _scene(64, 96, 4, 2), _scene(33, 1392, 3, 3)
    items = [a, b[:5] + (None,), c[:4] + (None, None), a[:4] + (None, a[5]), b]
    got = gpu.fish_render_tiff_many(items)
    assert 0 < gpu.timings()['count'] < 10000 and len(got) == len(items)
    for k, (item, files) in enumerate(zip(items, got)):
        want = gpu.fish_render_tiff(*item[:4])
        assert isinstance(files, tuple) and len(files) == 5 and files[:3] == want, 'image %d' % k
        assert files[3] == (None if item[4] is None else gpu.tiff_encode(item[4])), 'mask of image %d' % k
        assert files[4] == (None if item[5] is None else gpu.tiff_encode(item[5])), 'picture of image %d' % k
    assert gpu.fish_render_tiff_many(items[::-1]) == got[::-1]
    assert gpu.fish_render_tiff_many(items, budget_bytes=1) == got, 'one call per image'
    assert gpu.fish_render_tiff_many([]) == []


def test_fish_render_tiff_batch_refuses_what_fish_render_refuses_and_a_small_capacity(gpu):
    H, W = 6, 9
    bnd = np.zeros((H, W), np.uint8)
    with pytest.raises(EcsegError) as e:
        gpu.fish_render_tiff_many([(np.zeros((H, W, 3), np.uint8), (0, 1, 3), np.zeros((H, W, 2), np.uint8), bnd, None, None)])
    assert e.value.code == -1 and 'channel index' in str(e.value)
    with pytest.raises(ValueError):
        gpu.fish_render_tiff_many([(np.zeros((H, W, 3), np.uint8), (0, 1, 2), np.zeros((H, W, 2), np.uint8), bnd, np.zeros((H, W + 1), np.uint8), None)])
    lib = load_library()
    img, thr = np.zeros((H, W, 3), np.uint8), np.zeros((H, W, 2), np.uint8)
    shapes, ch = np.array([[H, W, 3]], np.int32), np.array([[0, 1, 2, 0]], np.int32)
    one = lambda a: (C.c_void_p * 1)(a.ctypes.data)
    out, ranges = np.full(4096, 0xa5, np.uint8), np.full((1, 5, 2), -7, np.int64)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    args = lambda cap: (gpu.h, 1, one(img), vp(shapes), vp(ch), one(thr), one(bnd), None, None, vp(out), cap, vp(ranges))
    assert lib.ecseg_fish_render_tiff_batch(*args(100)) == -1
    assert 'do not fit the capacity' in lib.ecseg_last_error(gpu.h).decode() and (out == 0xa5).all() and (ranges == -7).all()
    assert lib.ecseg_fish_render_tiff_batch(*args(4096)) == 0
    assert (ranges[0, :3, 1] > 0).all() and (ranges[0, 3:] == 0).all() and ranges[0, 2].sum() < 4096


# ---- make stat_fish ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('use_min_cut', [False, True])
def test_make_stat_fish_writes_the_same_tree_at_tiff_write_batch_1_2_and_8(gpu, tmp_path, monkeypatch, use_min_cut):
    """A five-image folder, three- and four-channel images: every file and the CSV text."""
    inp, _ = cpu.make_folder(tmp_path, size=(67, 93))
    for k in (0, 1):
        shutil.copyfile(inp / 'b_tif.tif', inp / ('d_%d.tif' % k))
        shutil.copyfile(inp / 'nuclei_masks' / 'b_tif.tif', inp / 'nuclei_masks' / ('d_%d.tif' % k))

    def run(**keys):
        cfg = yaml.safe_load(open(tmp_path / 'config.yaml'))
        cfg['stat_fish'].update(use_min_cut=use_min_cut, tiff_on_device=True, **keys)
        yaml.safe_dump(cfg, open(tmp_path / 'config.yaml', 'w'))
        sf.main([], handle=gpu)
        return cpu.folder_bytes(inp / 'annotated')

    monkeypatch.chdir(tmp_path)
    want = run(tiff_write_batch=1)
    assert len(want) == 5 * (6 if use_min_cut else 5) + 2 and 'stat_fish_lsq.csv' in want
    for k in (2, 8):
        got = run(tiff_write_batch=k, tiff_read_on_device=True, tiff_read_batch=3)
        assert sorted(got) == sorted(want), k
        assert got['stat_fish_lsq.csv'].decode() == want['stat_fish_lsq.csv'].decode(), k
        for name in want:
            assert got[name] == want[name], (k, name)
