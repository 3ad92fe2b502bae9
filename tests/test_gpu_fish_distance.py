"""ecseg_fish_distances (csrc/fishdist_kernels.hip) and ``make fish_distance_calculation`` on the device.  Records are
compared field by field with the vectorised oracle ``fish_distance_ref.records``, distances bit for bit (float.hex) with
``fish_distance_ref.loop``, the line-by-line restatement of the reference; never with the product's own Python.
``_case(seed)`` is also the generator of tools/fuzz_fish_distance.py; a failing seed of that campaign becomes a case here."""
import os
import sys

import numpy as np
import pytest
import yaml

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fish_distance_cases as cases          # noqa: E402
import fish_distance_ref as ref              # noqa: E402
from ecseg_amd import csvio, image_io        # noqa: E402
from ecseg_amd import fish_distance_calculation as fdc   # noqa: E402

pytestmark = pytest.mark.gpu
HAND = cases.hand_cases()
N_SEEDS = 60


def _hex(values):
    return [float(v).hex() for v in values]


def _i32(seg):
    return np.ascontiguousarray(np.where(seg > 0, seg, 0), np.int32)


def _ranked(seg):
    """Labels replaced by their rank: what a caller of the C entry point does with a map whose labels exceed H * W."""
    values = np.unique(seg[seg > 0])
    return np.where(seg > 0, np.searchsorted(values, seg) + 1, 0).astype(np.int32)


def _mismatches(gpu, lsq, seg, fi, ci, capacity=4096, want=None):
    want = ref.records(lsq, seg, fi, ci) if want is None else want
    got = gpu.fish_distances(seg, lsq, fi, ci, capacity)
    if got.shape != want.shape:
        return ['%d cells, the oracle has %d' % (len(got), len(want))], got
    rows = np.flatnonzero((got != want).any(axis=1))
    if len(rows):
        r = rows[0]
        return ['%d of %d records differ, first cell %d: %s, oracle %s' % (len(rows), len(want), r, got[r].tolist(), want[r].tolist())], got
    return [], got


def _check(gpu, lsq, seg, fi=0, ci=1, capacity=4096, want=None):
    bad, got = _mismatches(gpu, lsq, seg, fi, ci, capacity, want)
    assert not bad, '; '.join(bad)
    return got


def _case(seed):
    """-> (lsq, seg int32, fish index, centromere index): a random scene of tools/fuzz_fish_distance.py."""
    rng = np.random.default_rng(seed + 7919)
    size = cases.SCENE_SIZES[seed % len(cases.SCENE_SIZES)] if seed % 4 else (int(rng.integers(1, 330)), int(rng.integers(1, 330)))
    lsq, seg = cases.scene(seed, size=size, C=int(rng.choice([2, 3, 3, 4])))
    fi, ci = [(0, 1), (1, 0), (0, 0), (lsq.shape[2] - 1, 1)][int(rng.integers(0, 4)) if seed % 5 == 0 else seed % 2]
    return lsq, (_i32(seg) if seg.max() <= seg.size else _ranked(seg)), fi, ci


def case_mismatches(gpu, seed):
    lsq, seg, fi, ci = _case(seed)
    return _mismatches(gpu, lsq, seg, fi, ci)[0]


# ---- hand cases and random scenes ------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', sorted(HAND))
def test_hand_computed_cases(gpu, name):
    lsq, seg, (ci, fi, mx), want = HAND[name]
    got = _check(gpu, lsq, _i32(seg), fi, ci)
    assert _hex(fdc.distances_from_records(got, mx)) == _hex(ref.loop(lsq, seg, (ci, fi, mx))) == _hex(want)
    assert _hex(fdc.get_distances_img(lsq, seg, (ci, fi, mx), gpu)) == _hex(want)


def test_random_scenes_both_colour_assignments(gpu):
    tally = np.zeros(5, int)
    for seed in range(N_SEEDS):
        lsq, seg = cases.scene(seed)
        for ci, fi in ((1, 0), (0, 1)):
            want = ref.loop(lsq, seg, (ci, fi, cases.MAX_SPOTS))
            tally += cases.outcomes(lsq, seg, fi, ci, cases.MAX_SPOTS, ref.records)
            got = _check(gpu, lsq, _i32(seg), fi, ci)
            assert _hex(fdc.distances_from_records(got, cases.MAX_SPOTS)) == _hex(want), (seed, ci, fi)
            assert _hex(fdc.get_distances_img(lsq, seg, (ci, fi, cases.MAX_SPOTS), gpu)) == _hex(want), (seed, ci, fi)
    # the oracle's own output: finite, 0.0, gate failure, skipped for the spot count - a vacuous pass is not possible
    assert (tally[:4] >= 20).all(), tally


def test_fuzz_generator_cases(gpu):
    for seed in range(80):
        bad = case_mismatches(gpu, seed)
        assert not bad, 'seed %d: %s' % (seed, '; '.join(bad))


@pytest.mark.parametrize('size', [(1, 1), (1, 64), (64, 1), (1, 1000), (1000, 1), (2, 2), (63, 65), (33, 1025), (1025, 3), (512, 512), (512, 514)])
def test_degenerate_sizes(gpu, size):
    for seed in range(3):
        lsq, seg = cases.scene(100 + seed, size=size)
        _check(gpu, lsq, _i32(seg) if seg.max() <= seg.size else _ranked(seg), seed % 2, 1 - seed % 2)


# ---- paths a realistic scene never reaches ------------------------------------------------------------------------------
def test_one_dense_cell_left_half_fish_right_half_centromere(gpu):
    lsq = np.zeros((300, 300, 3), np.uint8)
    seg = np.zeros((300, 300), np.int32)
    seg[20:276, 30:286] = 5
    lsq[:, :158, 0] = 200                                    # spills over the cell on purpose
    lsq[:, 158:, 1] = 100
    want = np.array([[5, 65536, 3, 256 * 128, 256 * 128, 1, 1, 0]], np.int64)
    assert np.array_equal(ref.records(lsq[20:276, 120:200], seg[20:276, 120:200], 0, 1)[:, 5:7], want[:, 5:7])   # the oracle on a strip
    got = _check(gpu, lsq, seg, 0, 1, want=want)
    assert fdc.distances_from_records(got, 3) == [1 / 256]
    lsq[:, 150:166] = 0                                       # a gap of 16 columns between the halves, all tiles of the list scanned
    want = np.array([[5, 65536, 3, 256 * 120, 256 * 120, 1, 17 * 17, 0]], np.int64)
    _check(gpu, lsq, seg, 0, 1, want=want)
    _check(gpu, lsq, seg, 1, 0, want=want)


def test_one_label_over_a_whole_image_is_searched_by_many_workgroups(gpu):
    """One cell of 1040 x 1392 with 400 columns of FISH and 400 of centromere, 593 columns apart: 1.7 x 10^11 pairs, split
    over the FISH-list slices of fd_distance_kernel.  Also one cell among few (more slices than FISH pixels)."""
    H, W = 1040, 1392
    lsq = np.zeros((H, W, 3), np.uint8)
    seg = np.full((H, W), 9, np.int32)
    lsq[:, :400, 0] = 1
    lsq[:, 992:, 1] = 1
    want = np.array([[9, H * W, 3, H * 400, H * 400, 1, 593 ** 2, 0]], np.int64)
    _check(gpu, lsq, seg, 0, 1, want=want)
    print('whole-image cell: %.1f ms of kernels' % gpu.timings()['count'])
    seg[:8, :8] = 4                                            # a second, tiny cell: FISH pixels fewer than one slice
    lsq[3, 3, 1] = 1
    want = np.array([[4, 64, 3, 64, 1, 1, 0, 0], [9, H * W - 64, 3, H * 400 - 64, H * 400, 1, 593 ** 2, 0]], np.int64)
    _check(gpu, lsq, seg, 0, 1, want=want)


def test_cell_that_is_entirely_fish(gpu):
    lsq = np.zeros((200, 260, 3), np.uint8)
    seg = np.zeros((200, 260), np.int32)
    yy, xx = np.ogrid[:200, :260]
    seg[((yy - 100) / 90) ** 2 + ((xx - 130) / 120) ** 2 <= 1] = 3
    lsq[..., 0] = 1
    lsq[100, 130, 1] = 1
    area = int((seg == 3).sum())
    _check(gpu, lsq, seg, 0, 1, want=np.array([[3, area, 3, area, 1, 1, 0, 0]], np.int64))
    _check(gpu, lsq, seg, 0, 0, want=np.array([[3, area, 3, area, area, 1, 0, 0]], np.int64))
    lsq[100, 130, 0] = 0                                      # a hole: still one component, distance 1
    _check(gpu, lsq, seg, 0, 1, want=np.array([[3, area, 3, area - 1, 1, 1, 1, 0]], np.int64))


def _spiral(n):
    m = np.zeros((n, n), bool)
    y = x = 0
    dy, dx = 0, 1
    top, left, bottom, right = 0, 0, n - 1, n - 1
    lim = [top, left, bottom, right]
    m[0, 0] = True
    for _ in range(n * n):
        ny, nx = y + dy, x + dx
        if not (lim[0] <= ny <= lim[2] and lim[1] <= nx <= lim[3]):
            if (dy, dx) == (0, 1):
                lim[0] += 2
            elif (dy, dx) == (1, 0):
                lim[3] -= 2
            elif (dy, dx) == (0, -1):
                lim[2] -= 2
            else:
                lim[1] += 2
            dy, dx = dx, -dy
            ny, nx = y + dy, x + dx
            if not (0 <= ny < n and 0 <= nx < n) or m[ny, nx] or m[min(max(ny + dy, 0), n - 1), min(max(nx + dx, 0), n - 1)]:
                break
        y, x = ny, nx
        m[y, x] = True
    return m


def test_spiral_comb_and_ring_components(gpu):
    H = W = 140
    lsq = np.zeros((H, W, 3), np.uint8)
    seg = np.zeros((H, W), np.int32)
    seg[:70, :70] = 1; seg[:70, 70:] = 2; seg[70:, :70] = 3; seg[70:, 70:] = 4
    lsq[2:67, 2:67, 0][_spiral(65)] = 9                       # one long winding component
    comb = np.zeros((60, 60), bool); comb[::2, :] = True; comb[:, 0] = True; comb[1::4, 0] = False    # teeth joined in pairs
    lsq[5:65, 75:135, 0][comb] = 9
    yy, xx = np.ogrid[:60, :60]
    for r in (28, 22, 16, 10, 4):                             # five concentric rings
        d = np.hypot(yy - 30, xx - 30)
        lsq[75:135, 5:65, 0][(d >= r - 0.5) & (d < r + 0.5)] = 9
    zig = np.zeros((60, 60), bool)                            # diagonal chains: 8-connected only
    for k in range(0, 60, 6):
        zig[np.arange(60), (np.arange(60) + k) % 60] = True
    lsq[75:135, 75:135, 0][zig] = 9
    lsq[69, 69, 1] = lsq[69, 70, 1] = lsq[70, 69, 1] = lsq[70, 70, 1] = 5
    want = ref.records(lsq, seg, 0, 1)
    assert want[0, 5] == 1 and want[1, 5] > 3 and want[2, 5] == 5 and want[3, 5] >= 10, want[:, 5]
    _check(gpu, lsq, seg, 0, 1, want=want)
    from scipy import ndimage
    assert ndimage.label(zig)[1] > ndimage.label(zig, structure=ref.EIGHT)[1]      # 4-connectivity would count more


def test_label_of_two_distant_blobs_and_labels_1_7_hw(gpu):
    H, W = 90, 70
    lsq = np.zeros((H, W, 3), np.uint8)
    seg = np.zeros((H, W), np.int32)
    seg[:10, :10] = 7; seg[80:, 60:] = 7; seg[40:50, 30:40] = 1; seg[0:5, 60:70] = H * W
    lsq[2, 2, 0] = 5; lsq[85, 65, 1] = 5                       # the FISH pixel in one blob, the centromere in the other
    lsq[41, 31, 0] = lsq[48, 38, 0] = 5; lsq[45, 35, 1] = 5
    lsq[1, 61, :2] = 5
    got = _check(gpu, lsq, seg, 0, 1)
    assert got[:, 0].tolist() == [1, 7, H * W] and got[1, 6] == 83 ** 2 + 63 ** 2
    assert _hex(fdc.distances_from_records(got, 3)) == _hex(ref.loop(lsq, seg, (1, 0, 3)))


def test_twenty_thousand_one_pixel_cells_and_the_capacity_retry(gpu):
    rng = np.random.default_rng(5)
    H, W = 100, 200
    seg = (rng.permutation(H * W) + 1).reshape(H, W).astype(np.int32)
    lsq = (rng.random((H, W, 3)) < 0.5).astype(np.uint8) * 77
    want = ref.records(lsq, seg, 0, 1)
    assert len(want) == 20000
    got = _check(gpu, lsq, seg, 0, 1, capacity=4096, want=want)          # 20 000 > 4096: the binding comes back with a larger buffer
    _check(gpu, lsq, seg, 0, 1, capacity=20000, want=want)
    _check(gpu, lsq, seg, 0, 1, capacity=0, want=want)
    vals = fdc.distances_from_records(got, 3)
    assert set(vals) == {0.0} and len(vals) == int(((lsq[..., 0] != 0) & (lsq[..., 1] != 0)).sum())


def test_more_than_64_cells_in_one_tile_and_labels_equal_mod_64(gpu):
    rng = np.random.default_rng(6)
    H, W = 64, 128
    seg = np.zeros((H, W), np.int32)
    seg[:32, :64] = (np.arange(32)[:, None] // 2) * 32 + np.arange(64)[None] // 2 + 1       # 512 cells of 2 x 2 in one 64 x 32 tile
    seg[32:, :64] = ((np.arange(32)[:, None] // 8) * 4 + np.arange(64)[None] // 16) * 64 + 1000   # 16 cells, dense indices far apart, labels equal mod 64
    seg[:, 64:] = 3000 + 64 * (np.arange(64)[None] // 8) * (1 + np.arange(64)[:, None] // 8)
    lsq = (rng.random((H, W, 3)) < 0.3).astype(np.uint8) * 200
    want = ref.records(lsq, seg, 0, 1)
    assert len(want) > 512 + 16
    _check(gpu, lsq, seg, 0, 1, want=want)
    _check(gpu, lsq, seg, 1, 0)
    # dense cell indices (not label values) are the table's key: 70 cells whose INDICES are spread over one tile
    seg2 = np.zeros((32, 64), np.int32)
    seg2[:] = (np.arange(64)[None] + 64 * (np.arange(32)[:, None] % 3)) + 1
    _check(gpu, lsq[:32, :64], seg2, 0, 1)


def test_all_background_map(gpu):
    lsq = np.full((50, 60, 3), 9, np.uint8)
    for seg in (np.zeros((50, 60), np.int32), np.full((50, 60), -4, np.int32)):
        got = gpu.fish_distances(seg, lsq, 0, 1)
        assert got.shape == (0, 8)
        assert fdc.get_distances_img(lsq, seg, (1, 0, 3), gpu) == []


def test_wide_image_takes_the_64_bit_distance(gpu):
    """An extent above 32768: dy * dy + dx * dx no longer fits 32 bits."""
    H, W = 2, 70000
    lsq = np.zeros((H, W, 3), np.uint8)
    seg = np.ones((H, W), np.int32)                           # one cell: FISH at columns 0 and 35000, centromeres at 34999 and 69999
    lsq[0, 0, 0] = 1; lsq[1, 34999, 1] = 1
    lsq[0, 35000, 0] = 1; lsq[1, 69999, 1] = 1
    got = _check(gpu, lsq, seg, 0, 1)
    assert got[0, 6] == 2
    lsq[0, 35000, 0] = 0; lsq[1, 34999, 1] = 0                 # FISH at column 0, centromere at column 69999
    got = _check(gpu, lsq, seg, 0, 1)
    assert got[0, 6] == 69999 ** 2 + 1 > 2 ** 32
    assert _hex(fdc.distances_from_records(got, 3)) == _hex(ref.loop(lsq, seg, (1, 0, 3)))


# ---- the handle ---------------------------------------------------------------------------------------------------------
def test_buffer_reuse_large_small_large():
    from ecseg_amd._lib import Handle
    big = cases.scene(11, size=(400, 520))
    small = cases.scene(12, size=(40, 50))
    big2 = cases.scene(13, size=(400, 520))
    h = Handle(0)
    try:
        seq = [h.fish_distances(_i32(s), l, 0, 1) for l, s in (big, small, big2, small, big)]
    finally:
        h.close()
    for (l, s), got in zip((big, small, big2, small, big), seq):
        f = Handle(0)
        try:
            fresh = f.fish_distances(_i32(s), l, 0, 1)
        finally:
            f.close()
        assert np.array_equal(got, fresh) and np.array_equal(got, ref.records(l, s, 0, 1))


def test_region_map_of_nuclei_regions_survives_fish_distances(gpu, golden_dir):
    z = np.load(os.path.join(golden_dir, 'interseg_scene_small.npz'))
    seg, img = z['seg'], z['image']
    rec = gpu.nuclei_regions(seg, img, 0)
    desc = np.array([[r, rec[r, 1], rec[r, 2], min(rec[r, 3] - rec[r, 1], 256), min(rec[r, 4] - rec[r, 2], 256)] for r in range(len(rec))], np.int32)
    want_crops, want_max = gpu.nucleus_crops(desc)
    gpu.nuclei_regions(seg, img, 0)
    lsq, lab = cases.scene(21, size=(500, 700))
    _check(gpu, lsq, _i32(lab), 0, 1)
    crops, cmax = gpu.nucleus_crops(desc)
    assert len(desc) > 0 and np.array_equal(crops, want_crops) and np.array_equal(cmax, want_max)


def test_bad_arguments_leave_the_handle_usable(gpu):
    from ecseg_amd._lib import EcsegError
    lsq, seg, _, _ = HAND['triangle_3_4_5']
    seg = _i32(seg)
    for kw, text in ((dict(lsq=lsq[..., :1].copy(), fi=0, ci=0), 'channels'), (dict(fi=3), 'channel'), (dict(ci=-1), 'channel'),
                     (dict(fi=0, ci=7), 'channel')):
        with pytest.raises(EcsegError) as e:
            gpu.fish_distances(seg, kw.get('lsq', lsq), kw.get('fi', 0), kw.get('ci', 1))
        assert e.value.code == -1 and text in str(e.value)
        _check(gpu, lsq, seg, 0, 1)
    too_big = seg.copy()
    too_big[2, 2] = seg.size + 1
    with pytest.raises(EcsegError, match='larger than H \\* W') as e:
        gpu.fish_distances(too_big, lsq, 0, 1)
    assert e.value.code == -1
    _check(gpu, lsq, seg, 0, 1)
    too_big[2, 2] = seg.size                                  # the largest label that is accepted
    _check(gpu, lsq, too_big, 0, 1)
    with pytest.raises(ValueError):
        gpu.fish_distances(seg[:-1], lsq, 0, 1)
    with pytest.raises(ValueError):
        gpu.fish_distances(seg.astype(float), lsq, 0, 1)


def test_device_time_is_reported(gpu):
    lsq, seg = cases.scene(31, size=(300, 400))
    gpu.fish_distances(_i32(seg), lsq, 0, 1)
    assert 0 < gpu.timings()['count'] < 1000


# ---- file level ---------------------------------------------------------------------------------------------------------
def test_main_on_the_device(tmp_path, monkeypatch, capsys):
    from PIL import Image
    inp = tmp_path / 'in'
    scenes = []
    for k, (name, dtype) in enumerate((('img_b', np.int64), ('img_a', np.int32), ('img_c', np.int64))):
        lsq, seg = cases.scene(40 + k, size=(260, 330))
        if name == 'img_c':
            seg = np.where(seg > 0, seg * 1000, seg)         # labels above H * W: remapped on the host
        scenes.append((name, lsq, seg))
        d = inp / 'annotated' / name
        d.mkdir(parents=True)
        image_io.write_tiff_gray8(str(inp / (name + '.tif')), np.zeros((4, 4), np.uint8))
        np.save(str(d / (name + '__segmentation_min_cut.npy')), seg.astype(dtype))
        Image.fromarray(lsq).save(str(d / (name + '_lsq_t20.tif')), compression='tiff_lzw')
    yaml.safe_dump({'fish_distance_calculation': {'inpath': str(inp), 'centromere_probe_color': 'green', 'fish_probe_color': 'red',
                                                  'max_centromeric_spots': 3}}, open(tmp_path / 'config.yaml', 'w'))
    monkeypatch.chdir(tmp_path)
    fdc.main([])
    vals = []
    for name, lsq, seg in sorted(scenes):
        vals += ref.loop(lsq, seg, (1, 0, 3))
    want = csvio.csv_text(['normalized_distance'], [[v] for v in vals])
    assert open(inp / 'centromere_distances.csv').read() == want and len(vals) > 30
