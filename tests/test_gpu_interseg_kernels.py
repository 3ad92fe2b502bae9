"""The interSeg region and crop kernels (ecseg_nuclei_regions / ecseg_nucleus_crops, csrc/interseg_kernels.hip) against
the exact CPU reference oracle/interseg.py, bit for bit, on masks built to reach the paths the two fixture scenes of
test_gpu_interseg_driver.py never do: more than 64 regions in one 64 x 32 stats tile (the LDS table overflows to global
atomics) and region indices equal mod 64 (linear probing), sums of rows / columns above 2^32, degenerate and
pass-boundary geometry, interlocking shapes and several runs of one region in one 64-lane row segment, every crop window
size at the map's edges, multi-launch crop calls, 1 / 3 / 4 channels and repeated channel orders, buffer reuse across
calls of different sizes on one handle, and the instance-id refusal.  ``_interseg_case(seed)`` is also the generator of
tools/fuzz_interseg.py; failing seeds of that campaign become fixed cases here."""
import numpy as np
import pytest

from oracle import interseg as oi

pytestmark = pytest.mark.gpu
SIZES = (1, 2, 31, 32, 33, 63, 64, 65, 1023, 1024, 1025)
EDGE_HW = (1, 2, 3, 255, 256)


# ---- comparison -----------------------------------------------------------------------------------------------------
def _mismatches(gpu, seg, img, channel0=0, desc=None, order=(0, 1, 2), capacity=4096):
    """Runs nuclei_regions (+ nucleus_crops of ``desc``, (n, 5) windows or a function of the oracle's records and label
    map that returns them) on the handle and compares with the oracle.  -> (list of mismatch descriptions, oracle
    records, oracle label map, device crops or None)."""
    bad = []
    want, lab = oi.region_records(seg, img, channel0)
    got = gpu.nuclei_regions(seg, img, channel0, capacity)
    if got.shape != want.shape:
        return ['%d regions, the oracle has %d' % (len(got), len(want))], want, lab, None
    rows = np.flatnonzero((got != want).any(axis=1))
    if len(rows):
        r = rows[0]
        bad.append('%d of %d records differ, first region %d: %s, oracle %s' % (len(rows), len(want), r, got[r].tolist(), want[r].tolist()))
    if callable(desc):
        desc = desc(want, lab)
    if desc is None or len(desc) == 0:
        return bad, want, lab, None
    desc = np.asarray(desc, np.int32).reshape(-1, 5)
    crops, cmax = gpu.nucleus_crops(desc, order)
    ref_max = np.zeros((len(desc), 3), np.int32)
    n_bad = 0
    for k, d in enumerate(desc):
        ref = oi.nucleus_crop(img, lab, *[int(v) for v in d], order=order)
        ref_max[k] = ref.max(axis=(0, 1))
        if not np.array_equal(crops[k], ref):
            if not n_bad:
                bad.append('crop %d %s order %s: %d values differ' % (k, d.tolist(), tuple(order), int((crops[k] != ref).sum())))
            n_bad += 1
    if n_bad > 1:
        bad.append('%d of %d crops differ' % (n_bad, len(desc)))
    if not np.array_equal(cmax, ref_max):
        k = int(np.flatnonzero((cmax != ref_max).any(axis=1))[0])
        bad.append('channel_max of crop %d: %s, oracle %s' % (k, cmax[k].tolist(), ref_max[k].tolist()))
    return bad, want, lab, crops


def _check(gpu, seg, img, channel0=0, desc=None, order=(0, 1, 2), capacity=4096):
    bad, want, lab, crops = _mismatches(gpu, seg, img, channel0, desc, order, capacity)
    assert not bad, '; '.join(bad)
    return want, lab, crops


# ---- generators -----------------------------------------------------------------------------------------------------
def _image(rng, H, W, C, extra=(0, 0)):
    """(H + extra rows, W + extra columns, C) random uint8 image: an image larger than the mask is legal."""
    return rng.integers(0, 256, (H + extra[0], W + extra[1], C), dtype=np.uint8)


def _window(rng, rec, r, H, W, h=None, w=None):
    """(region, y0, x0, h, w): an h x w window inside the map, placed to overlap region r's bbox where it can."""
    h = min(h or int(rng.integers(1, 257)), H)
    w = min(w or int(rng.integers(1, 257)), W)
    y0, x0, y1, x1 = (int(v) for v in rec[r, 1:5])
    y = int(np.clip(rng.integers(y0 - h + 1, y1), 0, H - h))
    x = int(np.clip(rng.integers(x0 - w + 1, x1), 0, W - w))
    return [r, y, x, h, w]


def _bbox_windows(rec, regions):
    """The driver's windows: each region's bbox, clipped to its first 256 x 256."""
    return [[r, int(rec[r, 1]), int(rec[r, 2]), int(min(rec[r, 3] - rec[r, 1], 256)), int(min(rec[r, 4] - rec[r, 2], 256))]
            for r in regions]


def _crop_sample(rng, rec, H, W, n):
    """Up to n windows: half the regions' bboxes, half windows of random or edge sizes around a random region."""
    if len(rec) == 0 or n == 0:
        return np.zeros((0, 5), np.int32)
    regions = rng.integers(0, len(rec), n)
    out = []
    for k, r in enumerate(regions):
        if k % 2 == 0:
            out += _bbox_windows(rec, [int(r)])
        else:
            edge = rng.random() < 0.5
            h = int(rng.choice(EDGE_HW)) if edge else None
            w = int(rng.choice(EDGE_HW)) if edge else None
            out.append(_window(rng, rec, int(r), H, W, h, w))
    return np.array(out, np.int32)


def _disks(rng, H, W, n, rmax):
    m = np.zeros((H, W), bool)
    for _ in range(n):
        r = int(rng.integers(0, rmax + 1))
        cy, cx = int(rng.integers(0, H)), int(rng.integers(0, W))
        ya, yb, xa, xb = max(cy - r, 0), min(cy + r + 1, H), max(cx - r, 0), min(cx + r + 1, W)
        yy, xx = np.ogrid[ya:yb, xa:xb]
        m[ya:yb, xa:xb] |= (yy - cy) ** 2 + (xx - cx) ** 2 <= r * r + int(rng.integers(0, r + 1))
    return m


def _spiral(n):
    """n x n square spiral of 1-pixel lines 1 pixel apart (one region), drawn clockwise from the top-left corner."""
    m = np.zeros((n, n), bool)
    y = x = 0
    m[0, 0] = True
    steps = [(0, 1), (1, 0), (0, -1), (-1, 0)]
    length, turn = n - 1, 0
    while length > 0:
        for _ in range(2):
            dy, dx = steps[turn % 4]
            for _ in range(length):
                y, x = y + dy, x + dx
                m[y, x] = True
            turn += 1
        length -= 2
    return m


def _shapes(rng, H=192, W=448):
    """Interlocking and thin regions, each where a window's masking of its neighbours does the work: two interlocking
    combs inside one 64-lane segment (15 runs of each comb per row), a ring around an island and a dot, diagonal chains
    (8- but not 4-connected) 3 columns apart, a zigzag across column 192 and row 128, a U with an island between its arms
    (both arms in one 64-lane segment), a spiral, and a few blobs."""
    m = np.zeros((H, W), bool)
    m[2, 2:62] = True                                        # comb A: base on top, teeth down at columns 2, 6, .., 58
    m[2:60, 2:62:4] = True
    m[62, 0:64] = True                                       # comb B: base below, teeth up at columns 4, 8, .., 60
    m[5:63, 4:64:4] = True
    m[10:72, 80:142] = True                                  # ring (2 pixels thick) across column 128 and rows 32 / 64
    m[12:70, 82:140] = False
    m[30:50, 100:120] = True                                 # island in the ring
    m[60, 130] = True                                        # a dot between island and ring
    k = np.arange(80)
    m[10 + k, 150 + k] = True                                # diagonal chains
    m[10 + k, 153 + k] = True
    k = np.arange(60)
    m[100 + k, 191 + k % 2] = True                           # zigzag
    m[100:141, 262:266] = True                               # U: two arms, one 64-lane segment (256..319) holds both
    m[100:141, 290:294] = True
    m[137:141, 262:294] = True
    m[100:131, 270:286] = True                               # island between the arms
    m[10:71, 360:421] |= _spiral(61)
    m[120:190, 340:440] |= _disks(rng, 70, 100, 12, 9)
    return m[:H, :W]


def _short_runs_tile(rng, H=96, W=192, ty=1, tx=1):
    """More than 64 regions in stats tile (ty, tx) that are wider and taller than one pixel: runs of 2 - 5 pixels on every
    other row, 2 x 2 / 3 x 3 blobs across the tile's four edges, a few regions in the neighbouring tiles."""
    m = np.zeros((H, W), bool)
    y0, x0 = ty * 32, tx * 64
    for y in range(y0 + 1, y0 + 31, 2):
        x = x0 + int(rng.integers(0, 3))
        while x < x0 + 62:
            n = int(rng.integers(2, 6))
            m[y, x:min(x + n, x0 + 64)] = True
            x += n + int(rng.integers(1, 3))
    for _ in range(12):                                      # blobs across the four edges of the tile
        b = int(rng.integers(2, 4))
        edge = int(rng.integers(0, 4))
        if edge < 2:
            y = (y0 if edge == 0 else y0 + 32) - b // 2
            x = x0 + int(rng.integers(0, 64 - b))
        else:
            x = (x0 if edge == 2 else x0 + 64) - b // 2
            y = y0 + int(rng.integers(0, 32 - b))
        m[y:y + b, x:x + b] = True
    m |= _disks(rng, H, W, 6, 3) & ~np.pad(np.ones((32, 64), bool), ((y0, H - y0 - 32), (x0, W - x0 - 64)))
    return m


def _lattice_in_tile(rng, n, H=96, W=192, ty=1, tx=1):
    """n isolated pixels on the 2-pixel lattice of stats tile (ty, tx) (512 sites), plus some regions around the tile."""
    m = np.zeros((H, W), bool)
    sites = rng.choice(512, n, replace=False)
    m[ty * 32 + 2 * (sites // 32), tx * 64 + 2 * (sites % 32)] = True
    m[2:6, 2:40] = True
    m[H - 5:H - 1, W - 50:W - 3] = True
    return m


def _mask(rng, H, W):
    kind = int(rng.integers(0, 6))
    if kind == 0:                                            # blobs
        return _disks(rng, H, W, int(rng.integers(1, 60)), int(rng.integers(1, max(2, min(H, W) // 4))))
    if kind == 1:                                            # speckle
        return rng.random((H, W)) < rng.choice([0.03, 0.2, 0.45, 0.6, 0.9])
    if kind == 2:                                            # isolated pixels on a lattice, some missing
        s = int(rng.integers(2, 4))
        m = np.zeros((H, W), bool)
        m[int(rng.integers(0, s))::s, int(rng.integers(0, s))::s] = True
        return m & (rng.random((H, W)) < rng.choice([0.5, 1.0]))
    if kind == 3:                                            # thin lines: rows, columns, diagonals
        m = np.zeros((H, W), bool)
        for _ in range(int(rng.integers(1, 30))):
            t = int(rng.integers(0, 3))
            if t == 0:
                m[int(rng.integers(0, H)), int(rng.integers(0, W)):int(rng.integers(0, W + 1))] = True
            elif t == 1:
                m[int(rng.integers(0, H)):int(rng.integers(0, H + 1)), int(rng.integers(0, W))] = True
            else:
                y, x, n = int(rng.integers(0, H)), int(rng.integers(0, W)), int(rng.integers(1, 300))
                k = np.arange(min(n, H - y, W - x))
                m[y + k, x + k] = True
        return m
    if kind == 4:                                            # shapes, tiled or cut to the map
        s = _shapes(rng)
        reps = (-(-H // s.shape[0]), -(-W // s.shape[1]))
        return np.tile(s, reps)[:H, :W]
    m = np.ones((H, W), bool)                                # one big component with holes
    m[rng.random((H, W)) < rng.choice([0.1, 0.3])] = False
    return m


def _interseg_case(seed):
    """Seeded random case -> (seg, img, channel0, desc(records, labels), order): random blob / speckle / lattice / thin / shape masks of
    random size (small, tile-boundary, up to 1100 x 1400), 1 / 3 / 4 channels, a random channel order (repeats allowed),
    an image up to 5 pixels larger than the mask, and at most a few hundred crop windows."""
    rng = np.random.default_rng(90000 + seed)
    size = int(rng.integers(0, 4))
    if size == 0:
        H, W = (int(v) for v in rng.integers(1, 100, 2))
    elif size == 1:
        H, W = (int(rng.choice(SIZES)) for _ in range(2))
    elif size == 2:
        H, W = int(rng.integers(1, 600)), int(rng.integers(1, 700))
    else:
        H, W = int(rng.integers(600, 1100)), int(rng.integers(700, 1400))
    seg = _mask(rng, H, W).astype(np.uint8) * int(rng.integers(1, 256))
    C = int(rng.choice([1, 3, 4]))
    img = _image(rng, H, W, C, (int(rng.integers(0, 6)), int(rng.integers(0, 6))))
    channel0 = int(rng.integers(0, C))
    order = tuple(int(c) for c in rng.integers(0, C, 3))
    n = int(rng.integers(0, 300))
    return seg, img, channel0, lambda rec, lab: _crop_sample(rng, rec, H, W, n), order


# ---- stats tile: LDS table overflow and hash collisions --------------------------------------------------------------
@pytest.mark.parametrize('n', [63, 64, 65, 512])
def test_isolated_pixels_in_one_tile(gpu, n):
    rng = np.random.default_rng(n)
    seg = _lattice_in_tile(rng, n).astype(np.uint8) * 255
    img = _image(rng, *seg.shape, 3)
    want, _, _ = _check(gpu, seg, img, 1)
    assert len(want) == n + 2
    rng2 = np.random.default_rng(n + 1)
    _check(gpu, seg, img, 2, _crop_sample(rng2, want, *seg.shape, 40), (2, 0, 1))


@pytest.mark.parametrize('seed', range(3))
def test_many_wide_regions_in_one_tile(gpu, seed):
    rng = np.random.default_rng(100 + seed)
    seg = _short_runs_tile(rng).astype(np.uint8) * 255
    img = _image(rng, *seg.shape, 3)
    want, lab = oi.region_records(seg, img, 0)
    in_tile = np.unique(lab[32:64, 64:128])
    wide = (want[:, 4] - want[:, 2] > 1)[in_tile[in_tile > 0] - 1]
    assert wide.sum() > 64 and (want[:, 3] - want[:, 1] > 1).any()          # the case reaches what it is for
    _check(gpu, seg, img, 0, _crop_sample(rng, want, *seg.shape, 60))


def test_region_indices_equal_mod_64_in_one_tile(gpu):
    """Tile (0, 0) holds regions 0, 64, 128, .., 960: a row of the map is one run in column 0 followed by 63 dots in the
    tiles to its right, so every run in tile (0, 0) hashes to LDS slot 0 and probes past the runs before it.  Tiles (0, 1)
    and (0, 2) hold about 500 dots each (the table overflows there)."""
    seg = np.zeros((64, 192), np.uint8)
    for k, y in enumerate(range(0, 32, 2)):
        seg[y, 0:2 + k] = 255                                # runs of growing width: a wrong slot shows in the bbox
        seg[y, 64:190:2] = 255
    seg[40:60, 3:50] = 255                                   # tile (1, 0): one more block
    rng = np.random.default_rng(5)
    img = _image(rng, 64, 192, 3, (3, 1))
    _, lab, _ = _check(gpu, seg, img, 0, [[64 * k, 2 * k, 0, 1, 2 + k] for k in range(16)] + [[1, 0, 60, 3, 9]])
    assert np.array_equal(lab[0:32:2, 0], 1 + 64 * np.arange(16))


def test_isolated_pixel_lattice_over_a_full_image(gpu):
    # 361 920 regions: every tile overflows, and Handle.nuclei_regions retries past its default capacity of 4096
    seg = np.zeros((1040, 1392), np.uint8)
    seg[::2, ::2] = 255
    rng = np.random.default_rng(6)
    img = _image(rng, 1040, 1392, 3)
    n = 520 * 696

    def desc(rec, lab):
        assert len(rec) == n
        return [[r, int(rec[r, 1]) - int(rec[r, 1] > 0), int(rec[r, 2]), 3, 2] for r in rng.integers(0, n, 60)] + \
            [[n - 1, 1040 - 256, 1392 - 256, 256, 256], [0, 0, 0, 255, 1]]
    _check(gpu, seg, img, 2, desc, (0, 2, 1))


# ---- 64-bit sums ------------------------------------------------------------------------------------------------------
def test_sums_of_a_4096_square_exceed_2_to_the_32(gpu):
    seg = np.full((4096, 4096), 255, np.uint8)
    img = _image(np.random.default_rng(7), 4096, 4096, 1)
    want, _, _ = _check(gpu, seg, img, 0, [[0, 0, 0, 256, 256], [0, 3840, 3840, 256, 256], [0, 4095, 0, 1, 256], [0, 1000, 4093, 3, 3]],
                        (0, 0, 0))
    s = 4096 * (4095 * 4096 // 2)                            # sum of rows = sum of columns
    assert s > 2 ** 34 and want.tolist() == [[4096 * 4096, 0, 0, 4096, 4096, s, s, int(img.sum(dtype=np.int64))]]


def test_sum_of_columns_of_a_full_width_strip_exceeds_2_to_the_32(gpu):
    seg = np.full((1, 100000), 7, np.uint8)
    img = _image(np.random.default_rng(8), 1, 100000, 4, (2, 3))
    want, _, _ = _check(gpu, seg, img, 3, [[0, 0, 0, 1, 256], [0, 0, 99744, 1, 256], [0, 0, 50000, 1, 3], [0, 0, 99999, 1, 1]], (3, 1, 0))
    s = 99999 * 100000 // 2
    assert s > 2 ** 32 and want.tolist() == [[100000, 0, 0, 1, 100000, 0, s, int(img[0, :100000, 3].sum(dtype=np.int64))]]


# ---- geometry -----------------------------------------------------------------------------------------------------------
def _edge_windows(rec, lab, H, W, sizes=EDGE_HW):
    """Windows of every size in ``sizes`` (clipped to the map) at the map's corners and edge midpoints, each cropping the
    region that covers most of it (region 0 where none does)."""
    out = []
    for h in sizes:
        for w in sizes:
            hh, ww = min(h, H), min(w, W)
            for y, x in ((0, 0), (0, W - ww), (H - hh, 0), (H - hh, W - ww), ((H - hh) // 2, 0), (0, (W - ww) // 2)):
                c = np.bincount(lab[y:y + hh, x:x + ww].ravel(), minlength=2)
                c[0] = 0
                out.append([max(int(np.argmax(c)) - 1, 0), y, x, hh, ww])
    return out


GEOMS = [(1, 1), (1, 2), (2, 1), (2, 2), (1, 1025), (1025, 1), (31, 64), (32, 65), (33, 63), (63, 33), (64, 1024), (65, 31),
         (1023, 2), (32, 1), (1024, 1023), (1025, 1025), (512, 512), (512, 514)]


@pytest.mark.parametrize('H,W', GEOMS)
def test_geometry(gpu, H, W):
    rng = np.random.default_rng(H * 7919 + W)
    if (H, W) in ((512, 512), (512, 514)):                   # root-count chunks: exactly one scan pass, one past it
        assert (H * W + 1023) // 1024 == {512: 256, 514: 257}[W]
    for k, seg in enumerate(((rng.random((H, W)) < 0.3), _disks(rng, H, W, 20, max(1, min(H, W) // 5)), np.ones((H, W), bool))):
        img = _image(rng, H, W, 3, (k, 2 * k + 1))
        desc = lambda rec, lab: (_edge_windows(rec, lab, H, W, (1, 3, 256)) + _crop_sample(rng, rec, H, W, 30).tolist()) if len(rec) else []
        _check(gpu, seg.astype(np.uint8) * (40 + k), img, k, desc, ((0, 1, 2), (2, 0, 1), (1, 1, 1))[k])
    assert len(gpu.nuclei_regions(np.zeros((H, W), np.uint8), _image(rng, H, W, 3), 0)) == 0


def test_crop_windows_of_every_edge_size_at_the_map_edges(gpu):
    rng = np.random.default_rng(9)
    H, W = 300, 333
    seg = _disks(rng, H, W, 25, 40).astype(np.uint8) * 255
    img = _image(rng, H, W, 3, (4, 0))
    _check(gpu, seg, img, 0, lambda rec, lab: _edge_windows(rec, lab, H, W) + [_window(rng, rec, r, H, W) for r in range(len(rec))],
           (1, 2, 0))


def test_shapes(gpu):
    rng = np.random.default_rng(10)
    seg = _shapes(rng).astype(np.uint8) * 255
    H, W = seg.shape
    img = _image(rng, H, W, 3, (1, 1))

    def desc(rec, lab):
        n = len(rec)
        return _bbox_windows(rec, range(n)) + [_window(rng, rec, r, H, W) for r in range(n)] + \
            [_window(rng, rec, r, H, W, h, w) for r in range(n) for h, w in ((3, 255), (255, 3), (2, 2))]
    for ch, order in ((0, (0, 1, 2)), (2, (1, 2, 0))):
        _check(gpu, seg, img, ch, desc, order)


# ---- crop calls, channels, reuse -----------------------------------------------------------------------------------------
def test_600_crops_in_one_call(gpu):
    # 3 launches of 256 + 256 + 88 crops, each with its own channel_max memset and output offsets
    rng = np.random.default_rng(11)
    H, W = 700, 900
    seg = _disks(rng, H, W, 120, 30).astype(np.uint8) * 255
    img = _image(rng, H, W, 3)
    img[..., 1] //= (1 + np.arange(W) // 100).astype(np.uint8)[None, :]           # channel maxima that differ from crop to crop
    _, _, crops = _check(gpu, seg, img, 0, lambda rec, lab: _crop_sample(rng, rec, H, W, 600), (2, 1, 0))
    assert len(crops) == 600 and len({tuple(c.max(axis=(0, 1))) for c in crops}) > 20


@pytest.mark.parametrize('C,orders', [(1, [(0, 0, 0)]), (3, [(0, 1, 2), (2, 1, 0), (2, 2, 2), (1, 1, 0)]),
                                      (4, [(3, 1, 0), (2, 2, 2), (0, 3, 3), (3, 3, 3)])])
def test_channels(gpu, C, orders):
    rng = np.random.default_rng(12 + C)
    H, W = 150, 230
    seg = _disks(rng, H, W, 30, 20).astype(np.uint8) * 255
    img = _image(rng, H, W, C, (3, 5))
    for ch in range(C):
        _check(gpu, seg, img, ch)
    for order in orders:
        _check(gpu, seg, img, C - 1, lambda rec, lab: _crop_sample(rng, rec, H, W, 24), order)


def test_buffer_reuse_across_sizes(gpu):
    rng = np.random.default_rng(13)
    big = (_disks(rng, 1040, 1392, 300, 25) | (rng.random((1040, 1392)) < 0.02)).astype(np.uint8) * 255
    big_img = _image(rng, 1040, 1392, 3)
    small = _disks(rng, 40, 50, 6, 8).astype(np.uint8) * 3
    small_img = _image(rng, 40, 50, 4, (1, 2))
    big_desc = lambda rec, lab: _crop_sample(np.random.default_rng(14), rec, 1040, 1392, 40)
    first, _, first_crops = _check(gpu, big, big_img, 1, big_desc)
    _check(gpu, small, small_img, 3, lambda rec, lab: _crop_sample(rng, rec, 40, 50, 20), (3, 2, 1))
    again, _, again_crops = _check(gpu, big, big_img, 1, big_desc)
    assert np.array_equal(first, again) and np.array_equal(first_crops, again_crops)
    _check(gpu, small, small_img, 0, lambda rec, lab: _bbox_windows(rec, range(len(rec))), (0, 1, 3), capacity=0)


# ---- instance ids ---------------------------------------------------------------------------------------------------------
def test_instance_ids_are_refused(gpu):
    from ecseg_amd._lib import EcsegError
    one = np.zeros((64, 130), np.uint8)
    one[20:40, 50:80] = 255                                  # one region across a tile border, one pixel differs
    one[39, 79] = 254
    far = np.zeros((1040, 1392), np.uint8)
    far[0:3, 0:3] = 7                                        # two values in the first and the last stats tile
    far[1030:1035, 1380:1390] = 9
    for seg in (one, far):
        with pytest.raises(EcsegError) as e:
            gpu.nuclei_regions(seg, np.zeros(seg.shape + (3,), np.uint8), 0)
        assert e.value.code == -1 and 'instance' in str(e.value)
        with pytest.raises(EcsegError):                      # no region map left on the handle
            gpu.nucleus_crops(np.array([[0, 0, 0, 2, 2]], np.int32))


def test_mask_of_ones_is_accepted(gpu):
    rng = np.random.default_rng(15)
    m = _disks(rng, 200, 260, 20, 15)
    img = _image(rng, 200, 260, 3)
    desc = lambda rec, lab: _bbox_windows(rec, range(len(rec)))
    r255, _, c255 = _check(gpu, m.astype(np.uint8) * 255, img, 0, desc)
    r1, _, c1 = _check(gpu, m.astype(np.uint8), img, 0, desc)
    assert len(r1) > 5 and np.array_equal(r1, r255) and np.array_equal(c1, c255)
    dot = np.zeros((33, 65), np.uint8)
    dot[32, 64] = 1
    assert gpu.nuclei_regions(dot, _image(rng, 33, 65, 1), 0).tolist()[0][:5] == [1, 32, 64, 33, 65]


# ---- seeded random cases (the generator of tools/fuzz_interseg.py) ---------------------------------------------------------
@pytest.mark.parametrize('seed', range(8))
def test_random_cases(gpu, seed):
    seg, img, channel0, desc, order = _interseg_case(seed)
    _check(gpu, seg, img, channel0, desc, order)
