"""ecseg_fish_distances_batch (the fdb_* kernels of csrc/fishdist_kernels.hip, layout csrc/fishdist_batch.h) and ``make
fish_distance_calculation`` with ``batch`` above 1 on the device.  Every image of every chunk is compared field by field with the
vectorised oracle ``fish_distance_ref.records``, distances bit for bit (float.hex) with ``fish_distance_ref.loop``; never with the
product's own Python.  Where the issue of the feature asks for it, the whole output is also held byte for byte to n single
``fish_distances`` calls.  ``chunk_case(seed)`` is also the generator of ``tools/fuzz_fish_distance.py --batch``."""
import os
import sys

import numpy as np
import pytest
import yaml

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fish_distance_cases as cases          # noqa: E402
import fish_distance_ref as ref              # noqa: E402
import test_gpu_fish_distance as single      # noqa: E402
from ecseg_amd import image_io               # noqa: E402
from ecseg_amd import fish_distance_calculation as fdc   # noqa: E402

pytestmark = pytest.mark.gpu
HAND = cases.hand_cases()
_i32, _ranked, _hex = single._i32, single._ranked, single._hex


def _oracle(images, fi, ci):
    return [ref.records(lsq, seg, fi, ci) for lsq, seg in images]


def chunk_mismatches(gpu, images, fi, ci, want=None, capacity=4096):
    """-> (what differs from the oracle, per image and named by it; the answers)"""
    want = _oracle(images, fi, ci) if want is None else want
    got = gpu.fish_distances_many([seg for _, seg in images], [lsq for lsq, _ in images], fi, ci, capacity)
    bad = []
    if len(got) != len(images):
        return ['%d answers for %d images' % (len(got), len(images))], got
    for i, (g, w) in enumerate(zip(got, want)):
        if isinstance(g, Exception):
            bad.append('image %d: %s' % (i, g))
        elif g.shape != w.shape:
            bad.append('image %d: %d cells, the oracle has %d' % (i, len(g), len(w)))
        elif (g != w).any():
            r = np.flatnonzero((g != w).any(axis=1))[0]
            bad.append('image %d: cell %d is %s, oracle %s' % (i, r, g[r].tolist(), w[r].tolist()))
    return bad, got


def _check(gpu, images, fi=0, ci=1, want=None, capacity=4096):
    bad, got = chunk_mismatches(gpu, images, fi, ci, want, capacity)
    assert not bad, '; '.join(bad)
    return got


def _scene(seed, size, C=3):
    lsq, seg = cases.scene(seed, size=size, C=C)
    return lsq, (_i32(seg) if seg.max() <= seg.size else _ranked(seg))


def chunk_case(seed):
    """-> (images, fish index, centromere index): a seeded chunk of 1, 3, 8, 9 or 17 scenes of the single-image generator"""
    rng = np.random.default_rng(seed + 104729)
    n = (1, 3, 8, 9, 17)[seed % 5]
    images = []
    for k in range(n):
        lsq, seg, _, _ = single._case(5000 + 31 * seed + k)
        images.append((lsq, seg))
    fi, ci = [(0, 1), (1, 0), (0, 0), (1, 1)][int(rng.integers(0, 4)) if seed % 5 == 0 else seed % 2]
    return images, fi, ci


def _bytes(answers):
    return [a.tobytes() for a in answers]


# ---- 1. one image --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', sorted(HAND))
def test_a_chunk_of_one_equals_the_oracle_on_the_hand_cases(gpu, name):
    lsq, seg, (ci, fi, mx), want = HAND[name]
    got = _check(gpu, [(lsq, _i32(seg))], fi, ci)
    assert _hex(fdc.distances_from_records(got[0], mx)) == _hex(ref.loop(lsq, seg, (ci, fi, mx))) == _hex(want)


# ---- 2. mixed shapes -----------------------------------------------------------------------------------------------------------
MIXED = ((1, 300), (300, 1), (3, 64), (65, 63), (33, 70), (64, 64), (96, 130))


def test_mixed_shapes_and_channel_counts_in_one_chunk(gpu):
    images = [_scene(200 + k, size, C=(2, 3, 4)[k % 3]) for k, size in enumerate(MIXED)]
    for fi, ci in ((0, 1), (1, 0)):
        got = _check(gpu, images, fi, ci)
        alone = [gpu.fish_distances(seg, lsq, fi, ci) for lsq, seg in images]
        assert _bytes(got) == _bytes(alone), 'the chunk and n single calls differ'
        assert sum(len(g) for g in got) > 40


# ---- 3. the seam ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('x0, x1', [(5, 5), (15, 0), (0, 15), (15, 15), (0, 0), (7, 8), (8, 7)])
def test_nothing_reaches_across_the_seam_of_two_images_of_equal_width(gpu, x0, x1):
    """Image 0 ends with a FISH pixel in its last row, image 1 begins with one in its first row: on the global pixel axis the second lies
    one "row" below the first (x1 == x0), diagonally below it (|x1 - x0| == 1), or - last column against first column - right behind
    it.  Each cell keeps one component, its own area and the distance to its own centromere pixel."""
    H, W = 8, 16
    a, b = np.zeros((H, W, 3), np.uint8), np.zeros((H, W, 3), np.uint8)
    sa, sb = np.zeros((H, W), np.int32), np.zeros((H, W), np.int32)
    sa[4:, :] = 1; sb[:3, :] = 1
    a[H - 1, x0, 0] = 9; a[4, 2, 1] = 7                        # own centromere: 3 rows up
    b[0, x1, 0] = 9; b[2, 12, 1] = 7                           # own centromere: 2 rows down
    want = [np.array([[1, 4 * W, 3, 1, 1, 1, 9 + (x0 - 2) ** 2, 0]], np.int64), np.array([[1, 3 * W, 3, 1, 1, 1, 4 + (x1 - 12) ** 2, 0]], np.int64)]
    assert all(np.array_equal(w, o) for w, o in zip(want, _oracle([(a, sa), (b, sb)], 0, 1)))
    _check(gpu, [(a, sa), (b, sb)], 0, 1, want=want)
    # a spot that runs along both sides of the seam is one component per cell, and a third image of the same width changes nothing
    a[H - 1, :, 0] = 9; b[0, :, 0] = 9
    got = _check(gpu, [(a, sa), (b, sb), (a, sa)], 0, 1)
    assert got[0][0, 5] == 1 and got[1][0, 5] == 1 and got[0].tobytes() == got[2].tobytes()


# ---- 4. images that contribute nothing or are refused --------------------------------------------------------------------------------
@pytest.mark.parametrize('where', ['first', 'middle', 'last', 'all'])
def test_an_image_without_a_label_shifts_nobodys_records(gpu, where):
    images = [_scene(300 + k, (33, 70)) for k in range(3)]
    want = _oracle(images, 0, 1)
    empty = (np.full((20, 30, 3), 255, np.uint8), np.zeros((20, 30), np.int32))
    at = {'first': [0], 'middle': [1], 'last': [3], 'all': [0, 2, 4]}[where]
    for k in at:
        images.insert(k, empty)
        want.insert(k, np.zeros((0, 8), np.int64))
    got = _check(gpu, images, 0, 1, want=want)
    assert [len(g) for g in got] == [len(w) for w in want]
    only = _check(gpu, [empty, empty], 0, 1)
    assert [g.shape for g in only] == [(0, 8), (0, 8)]
    assert gpu.fish_distances_many([], [], 0, 1) == []


def test_a_label_above_the_pixel_count_fails_its_image_alone(gpu):
    from ecseg_amd._lib import EcsegError
    images = [_scene(310 + k, (65, 63)) for k in range(3)]
    want = _oracle(images, 0, 1)
    lsq, seg = images[1]
    bad = seg.copy()
    bad[2, 2] = seg.size + 1
    for chunk, k in (([images[0], (lsq, bad), images[2]], 1), ([(lsq, bad), images[0]], 0), ([images[0], (lsq, bad)], 1), ([(lsq, bad)], 0)):
        got = gpu.fish_distances_many([s for _, s in chunk], [l for l, _ in chunk], 0, 1)
        assert isinstance(got[k], EcsegError) and got[k].code == -1 and 'larger than H * W = %d' % seg.size in str(got[k])
        with pytest.raises(EcsegError) as e:
            gpu.fish_distances(bad, lsq, 0, 1)
        assert str(e.value) == str(got[k]), 'the error the image raises alone'
        for j, (l, s) in enumerate(chunk):
            if j != k:
                assert np.array_equal(got[j], ref.records(l, s, 0, 1)), 'a neighbour of the refused image'
        rec, n_cells, status = gpu.fish_distances_batch_raw([s for _, s in chunk], [l for l, _ in chunk], 0, 1, 4096)
        assert status.tolist() == [-1 if j == k else 0 for j in range(len(chunk))] and n_cells[k] == 0
    bad[2, 2] = seg.size                                       # the largest label that is accepted
    _check(gpu, [images[0], (lsq, bad), images[2]], 0, 1)
    assert np.array_equal(want[0], _check(gpu, images, 0, 1)[0])


def test_argument_errors_name_the_image_and_leave_the_handle_usable(gpu):
    from ecseg_amd._lib import EcsegError
    images = [_scene(320 + k, (33, 70)) for k in range(3)]
    two = (np.ascontiguousarray(images[1][0][..., :2]), images[1][1])
    with pytest.raises(EcsegError, match='image 1: channel out of range') as e:
        gpu.fish_distances_many([images[0][1], two[1], images[2][1]], [images[0][0], two[0], images[2][0]], 2, 1)
    assert e.value.code == -1
    one = (np.ascontiguousarray(images[2][0][..., :1]), images[2][1])
    with pytest.raises(EcsegError, match='image 2: the lsq image needs at least 2 channels'):
        gpu.fish_distances_many([images[0][1], two[1], one[1]], [images[0][0], two[0], one[0]], 0, 1)
    with pytest.raises(ValueError):
        gpu.fish_distances_many([images[0][1][:-1]], [images[0][0]], 0, 1)
    with pytest.raises(ValueError):
        gpu.fish_distances_many([images[0][1]], [], 0, 1)
    _check(gpu, images, 0, 1)


# ---- 5. capacity ---------------------------------------------------------------------------------------------------------------
def test_a_capacity_below_the_chunks_cells_writes_the_counts_alone(gpu):
    images = [_scene(330 + k, (65, 63)) for k in range(4)]
    want = _oracle(images, 0, 1)
    total = sum(len(w) for w in want)
    labs, ims = [s for _, s in images], [l for l, _ in images]
    for cap in (total - 1, 1, 0):
        rec, n_cells, status = gpu.fish_distances_batch_raw(labs, ims, 0, 1, cap)
        assert n_cells.tolist() == [len(w) for w in want] and not status.any() and not rec.any(), 'nothing but n_cells is written'
    rec, n_cells, _ = gpu.fish_distances_batch_raw(labs, ims, 0, 1, total)
    assert np.array_equal(rec, np.concatenate(want))
    for cap in (total - 1, 1, 0, total, total + 5):
        _check(gpu, images, 0, 1, want=want, capacity=cap)


# ---- 6. more than 64 cells in one statistics tile ------------------------------------------------------------------------------------
def test_more_than_64_cells_in_one_tile_of_the_second_image(gpu):
    rng = np.random.default_rng(6)
    H, W = 64, 128
    seg = np.zeros((H, W), np.int32)
    seg[:32, :64] = (np.arange(32)[:, None] // 2) * 32 + np.arange(64)[None] // 2 + 1       # 512 cells of 2 x 2 in one 64 x 32 tile
    seg[32:, :64] = ((np.arange(32)[:, None] // 8) * 4 + np.arange(64)[None] // 16) * 64 + 1000   # labels equal mod 64
    seg[:, 64:] = 3000 + 64 * (np.arange(64)[None] // 8) * (1 + np.arange(64)[:, None] // 8)
    lsq = (rng.random((H, W, 3)) < 0.3).astype(np.uint8) * 200
    first, third = _scene(340, (33, 70)), _scene(341, (3, 64))
    got = _check(gpu, [first, (lsq, seg), third], 0, 1)
    assert len(got[1]) > 512 + 16
    # the same label values in the image in front: two images, two sets of cells
    got = _check(gpu, [(lsq, seg), (lsq[::-1].copy(), seg[::-1].copy()), (lsq, seg)], 1, 0)
    assert got[0].tobytes() == got[2].tobytes() and np.array_equal(got[0][:, 0], got[1][:, 0])


# ---- 7. the 64-bit sum ---------------------------------------------------------------------------------------------------------
def test_a_long_image_takes_the_64_bit_distance_and_leaves_the_small_ones_alone(gpu):
    W = 40000
    lsq = np.zeros((1, W, 3), np.uint8)
    seg = np.ones((1, W), np.int32)
    lsq[0, 0, 0] = 1; lsq[0, W - 1, 1] = 1
    small = [_scene(350, (33, 70)), _scene(351, (65, 63))]
    want = _oracle(small, 0, 1)
    long_want = np.array([[1, W, 3, 1, 1, 1, (W - 1) ** 2, 0]], np.int64)
    assert (W - 1) ** 2 < 2 ** 32 and 2 * 32768 ** 2 >= 2 ** 31        # (above 32768 the path is chosen by the extent, not by the value)
    got = _check(gpu, [small[0], (lsq, seg), small[1]], 0, 1, want=[want[0], long_want, want[1]])
    assert got[1][0, 6] == 39999 ** 2
    assert _hex(fdc.distances_from_records(got[1], 3)) == _hex([39999 / np.sqrt(W)])
    assert _bytes(_check(gpu, small, 0, 1, want=want)) == [got[0].tobytes(), got[2].tobytes()], 'the 32-bit chunk gives the same records'
    lsq2 = np.zeros((2, 70000, 3), np.uint8)                           # a squared distance above 2^32
    seg2 = np.ones((2, 70000), np.int32)
    lsq2[0, 0, 0] = 1; lsq2[1, 69999, 1] = 1
    got = _check(gpu, [small[0], (lsq2, seg2)], 0, 1)
    assert got[1][0, 6] == 69999 ** 2 + 1 > 2 ** 32


# ---- 8. seeded scenes ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('seed', range(20))
def test_seeded_chunks_equal_the_oracle_and_repeat_their_bytes(gpu, seed):
    images, fi, ci = chunk_case(seed)
    assert len(images) == (1, 3, 8, 9, 17)[seed % 5]
    got = _check(gpu, images, fi, ci)
    again = gpu.fish_distances_many([s for _, s in images], [l for l, _ in images], fi, ci)
    assert _bytes(got) == _bytes(again)
    if seed < 5:
        assert _bytes(got) == _bytes([gpu.fish_distances(s, l, fi, ci) for l, s in images]), 'n single calls'


# ---- 9. stale scratch ----------------------------------------------------------------------------------------------------------
def test_large_small_large_on_one_handle_equals_fresh_handles(gpu):
    from ecseg_amd._lib import Handle
    big = [_scene(360 + k, (130, 257)) for k in range(3)]
    small = [_scene(370 + k, (33, 70)) for k in range(2)]
    big2 = [_scene(380 + k, (130, 257)) for k in range(3)]
    order = (big, small, big, big2, small)

    def run(h, chunk):
        return h.fish_distances_many([s for _, s in chunk], [l for l, _ in chunk], 0, 1)
    h = Handle(0)
    try:
        seq = []
        for k, chunk in enumerate(order):
            seq.append(run(h, chunk))
            if k == 2:
                h.scratch_fill_debug(0xA5)                     # and whatever the driver's own buffer held is gone
    finally:
        h.close()
    for chunk, got in zip(order, seq):
        f = Handle(0)
        try:
            fresh = run(f, chunk)
        finally:
            f.close()
        assert _bytes(got) == _bytes(fresh), 'an answer depends on what an earlier call left in the scratch buffer'
        assert all(np.array_equal(g, w) for g, w in zip(got, _oracle(chunk, 0, 1)))


def test_device_time_is_reported_and_other_drivers_keep_their_state(gpu, golden_dir):
    z = np.load(os.path.join(golden_dir, 'interseg_scene_small.npz'))
    rec = gpu.nuclei_regions(z['seg'], z['image'], 0)
    desc = np.array([[r, rec[r, 1], rec[r, 2], min(rec[r, 3] - rec[r, 1], 256), min(rec[r, 4] - rec[r, 2], 256)] for r in range(len(rec))], np.int32)
    want_crops, want_max = gpu.nucleus_crops(desc)
    gpu.nuclei_regions(z['seg'], z['image'], 0)
    _check(gpu, [_scene(390 + k, (96, 130)) for k in range(4)], 0, 1)
    assert 0 < gpu.timings()['count'] < 1000
    crops, cmax = gpu.nucleus_crops(desc)
    assert len(desc) > 0 and np.array_equal(crops, want_crops) and np.array_equal(cmax, want_max)


# ---- 10. main() on a small folder --------------------------------------------------------------------------------------------------
PRESETS = (2, 0, 3)                                            # centromere probe blue, FISH probe red, at most 3 spots


def folder_scene(k):
    """Scene k of the folder: 96 x 130, the blue channel a copy of the green one, so that every nucleus that passes the gate has
    centromere pixels; in scene 4 one nucleus that passes the gate, with FISH pixels in at most 3 spots, loses its blue pixels."""
    lsq, seg = cases.scene(400 + k, size=(96, 130))
    lsq[..., 2] = lsq[..., 1]
    if k == 4:
        rec = ref.records(lsq, seg, 0, 2)
        hit = [r for r in rec.tolist() if r[2] == 3 and r[3] > 0 and r[5] <= 3]
        assert hit, 'scene 4 has no nucleus to empty'
        lsq[..., 2][seg == hit[0][0]] = 0
    return lsq, seg


def make_folder(tmp_path):
    """Six images under tmp_path/in: img_2 has no .npy, img_4 a nucleus with FISH pixels and no centromere pixel; img_1 is saved as
    int32 and img_5 with labels above H * W.  -> (folder, the scenes that yield rows, in sorted order)"""
    from PIL import Image
    inp = tmp_path / 'in'
    good = []
    for k in range(6):
        name = 'img_%d' % k
        lsq, seg = folder_scene(k)
        if k == 5:
            seg = np.where(seg > 0, seg * 1000, seg)
        d = inp / 'annotated' / name
        d.mkdir(parents=True)
        image_io.write_tiff_gray8(str(inp / (name + '.tif')), np.zeros((4, 4), np.uint8))
        if k != 2:
            np.save(str(d / (name + '__segmentation_min_cut.npy')), seg.astype(np.int32 if k == 1 else np.int64))
        Image.fromarray(lsq).save(str(d / (name + '_lsq_t20.tif')), compression='tiff_lzw')
        if k not in (2, 4):
            good.append((lsq, seg))
    return inp, good


def run_main(tmp_path, capsys, handle=None, **keys):
    var = {'inpath': str(tmp_path / 'in'), 'centromere_probe_color': 'blue', 'fish_probe_color': 'red', 'max_centromeric_spots': 3}
    var.update(keys)
    yaml.safe_dump({'fish_distance_calculation': var}, open(tmp_path / 'config.yaml', 'w'))
    code = 0
    try:
        fdc.main([], handle=handle)
    except SystemExit as e:
        code = e.code
    csv = open(tmp_path / 'in' / 'centromere_distances.csv').read()
    os.remove(tmp_path / 'in' / 'centromere_distances.csv')
    return csv, capsys.readouterr().out, code


def check_runs(inp, good, one, others):
    """what test 10 asserts of the run at ``batch`` 1 and of the runs above it, on the device and on a handle that answers from the oracle"""
    assert one[2] == 1 and '2 image(s) were NOT processed' in one[1] and 'img_2.tif - has no segmentation' in one[1]
    assert 'img_4.tif - nucleus' in one[1] and 'no centromere pixel' in one[1]
    for k, got in others.items():
        assert got == one, 'batch %d: the CSV, the lines or the exit code differ from batch 1' % k
    vals = []
    for lsq, seg in good:
        vals += ref.loop(lsq, seg, PRESETS)
    rows = one[0].split('\n')
    assert rows[0] == 'normalized_distance' and rows[-1] == '' and len(vals) > 30 and len(set(vals)) > 10
    assert _hex(float(r) for r in rows[1:-1]) == _hex(vals), 'bit for bit the values of the reference loop'
    lines = [l for l in one[1].split('\n') if l.startswith('Processing image:')]
    assert lines == ['Processing image:  ' + str(inp / ('img_%d.tif' % k)) for k in range(6)]


def test_main_with_batch_4_equals_batch_1_and_the_reference_loop(tmp_path, monkeypatch, capsys):
    inp, good = make_folder(tmp_path)
    monkeypatch.chdir(tmp_path)
    with pytest.raises(ValueError):
        ref.loop(*folder_scene(4), PRESETS)                    # the oracle stops on img_4 as the reference does
    one = run_main(tmp_path, capsys, batch=1)
    check_runs(inp, good, one, {k: run_main(tmp_path, capsys, batch=k, io_threads=3 if k == 4 else None) for k in (4, 2, 7)})
