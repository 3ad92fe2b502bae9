"""Inputs shared by tests/test_stat_fish.py, tests/test_gpu_stat_fish.py and tools/fuzz_stat_fish.py: hand cases (one small map
per rule of the peak filter, the spot labelling, the pair and the boundaries) and a seeded scene generator.  Not a test module.

A pixel painted with the channel's maximum is a centre whatever the filter says (src/stat_fish.py:82), so spots painted at 255
have exactly the painted shape; softer Gaussian bumps exercise the float64 filter decision."""
import numpy as np

SCENE_SIZES = ((96, 130), (64, 64), (65, 63), (200, 257), (1, 300), (300, 1), (128, 192), (37, 411), (3, 64), (150, 150), (17, 16))
KERNELS = (7, 7, 3, 1, 23, 7, 15)
NAN1 = np.full((1, 1), np.nan)
N_SEEDS = 44                   # committed seeds of the scene generator: tests/test_stat_fish.py asserts that none is ambiguous


def proj_kernel(K, sigma):
    """The projected Gaussian kernel of src/stat_fish.py:28-55 written out: exp(-d^2 / (2 sigma^2)) normalised to sum 1, minus
    its mean, scaled to unit norm.  K = 1 gives 0 / 0."""
    a = np.arange(K) - (K - 1) / 2.0
    d2 = a[:, None] ** 2 + a[None, :] ** 2
    g = np.exp(-d2 / (2.0 * sigma * sigma))
    g = g / g.sum()
    p = g - g.mean()
    with np.errstate(divide='ignore', invalid='ignore'):
        return p / np.sqrt((p * p).sum())


def _case(img, seg, probes=(1, 0), weights=NAN1, normal=15.0, ithr=(70.0, 70.0), min_cc=1, line=1):
    return dict(img=np.ascontiguousarray(img, np.uint8), seg=np.ascontiguousarray(seg, np.int32), probes=tuple(probes),
                weights=np.ascontiguousarray(weights, np.float64), normal=float(normal), ithr=tuple(float(v) for v in ithr[:len(probes)]),
                min_cc=int(min_cc), line=int(line))


def args(case):
    return (case['img'], case['seg'], case['probes'], case['weights'], case['normal'], case['ithr'], case['min_cc'], case['line'])


def hand_cases():
    """name -> (case, expected dict of record columns {column: list over cells})."""
    cases = {}

    def blank(H, W):
        return np.zeros((H, W, 3), np.uint8), np.zeros((H, W), np.int32)
    # diagonal contacts do not join (4-connectivity): three pixels on a diagonal are three spots
    img, seg = blank(8, 8); seg[1:7, 1:7] = 1
    img[2, 2, 1] = img[3, 3, 1] = img[4, 4, 1] = 255
    cases['diagonal_is_three_spots'] = (_case(img, seg), {4: [3], 5: [3], 1: [36]})
    cases['diagonal_spots_below_min_cc_vanish'] = (_case(img, seg, min_cc=2), {4: [0], 5: [0]})
    # an L of three pixels is one spot
    img, seg = blank(8, 8); seg[1:7, 1:7] = 1
    img[2, 2, 1] = img[3, 2, 1] = img[3, 3, 1] = 255
    cases['l_shape_is_one_spot'] = (_case(img, seg, min_cc=3), {4: [3], 5: [1]})
    cases['l_shape_needs_min_cc_3'] = (_case(img, seg, min_cc=4), {4: [0], 5: [0]})
    # a spot straddling two touching cells: counted per cell, each part on its own size
    img, seg = blank(6, 12); seg[:, :6] = 4; seg[:, 6:] = 9
    img[2, 3:8, 0] = 255                                     # 3 pixels in cell 4, 2 pixels in cell 9 (probe 1 = channel 0)
    cases['straddling_spot_counts_per_cell'] = (_case(img, seg, min_cc=2), {0: [4, 9], 9: [3, 2], 10: [1, 1]})
    cases['straddling_spot_smaller_part_goes'] = (_case(img, seg, min_cc=3), {9: [3, 0], 10: [1, 0]})
    # the pair: AND of the cleaned masks, its own size rule for the count only
    img, seg = blank(8, 10); seg[:] = 1
    img[1, 1:6, 1] = 255; img[1, 4:9, 0] = 255; img[5, 5, 0] = 255      # green 5 px, red 5 px + 1 px; overlap 2 px
    cases['pair_overlap'] = (_case(img, seg, min_cc=2), {4: [5], 5: [1], 9: [5], 10: [1], 19: [2], 20: [1]})
    cases['pair_overlap_below_min_cc'] = (_case(img, seg, min_cc=3), {4: [5], 9: [5], 19: [0], 20: [0]})
    # a spot on the image border and raw intensities
    img, seg = blank(5, 5); seg[:] = 7
    img[0, 0, 1] = 255; img[0, 1, 1] = 255; img[4, 4, 1] = 60; img[2, 2, 0] = 10
    cases['border_spot_and_raw_sums'] = (_case(img, seg), {0: [7], 1: [25], 2: [50], 3: [50], 4: [2], 5: [1], 6: [570], 7: [3], 8: [255],
                                                          9: [0], 10: [0], 11: [10], 12: [1], 13: [10]})
    # a 3 x 3 filter by hand: centre 100 among 10s, coefficient 8 * 100 - 8 * 10 = 720 at the centre, negative elsewhere; the
    # channel's maximum (200) lies outside the cell
    img, seg = blank(5, 9); seg[1:4, 1:4] = 1
    img[1:4, 1:4, 1] = 10; img[2, 2, 1] = 100; img[0, 8, 1] = 200
    lap = -np.ones((3, 3)); lap[1, 1] = 8
    cases['laplacian_by_hand'] = (_case(img, seg, weights=lap, normal=100.0, ithr=(5.0, 5.0)), {4: [1], 5: [1], 6: [180], 7: [9], 8: [100]})
    cases['laplacian_threshold_above_720'] = (_case(img, seg, weights=lap, normal=720.5, ithr=(5.0, 5.0)), {4: [0], 5: [0]})
    cases['laplacian_threshold_below_720'] = (_case(img, seg, weights=lap, normal=719.5, ithr=(5.0, 5.0)), {4: [1], 5: [1]})
    # K = 1: the projected kernel is NaN, only the maximum is a centre
    img, seg = blank(6, 6); seg[:] = 1
    img[..., 1] = 90; img[3, 3, 1] = 91
    cases['k1_only_the_maximum'] = (_case(img, seg), {4: [1], 5: [1]})
    # all-zero channel: bool(max) is False, nothing is a centre
    img, seg = blank(6, 6); seg[:] = 1
    cases['all_zero_channel'] = (_case(img, seg, ithr=(-1.0, -1.0)), {4: [0], 5: [0], 8: [0]})
    # saturated channel: every pixel is the maximum, one spot per cell, diagonal cells stay apart
    img, seg = blank(6, 6); seg[:3, :3] = 1; seg[3:, 3:] = 2; img[..., 1] = 255
    cases['saturated_channel'] = (_case(img, seg, min_cc=9), {4: [9, 9], 5: [1, 1]})
    # zero nuclei
    img, seg = blank(7, 9); img[..., :2] = 255
    cases['zero_nuclei'] = (_case(img, seg), {})
    return cases


def scene(seed, size=None, K=None, line=None, n_probe=2):
    """A seeded scene -> case dict."""
    rng = np.random.default_rng(seed + 1000003)
    H, W = size if size is not None else SCENE_SIZES[seed % len(SCENE_SIZES)]
    K = KERNELS[seed % len(KERNELS)] if K is None else K
    line = 1 + seed % 3 if line is None else line
    scale = {1: 1.0, 3: 2.0, 7: 1.0, 15: 0.5, 23: 0.3}.get(K, 1.0)
    min_cc = int(rng.choice([1, 3, 7, 7, 12, 28]))
    C = int(rng.choice([3, 3, 4]))
    yy, xx = np.ogrid[:H, :W]
    seg = np.zeros((H, W), np.int32)
    mode = seed % 9
    if mode != 8:                                            # mode 8: zero nuclei
        label = 0
        for _ in range(max(1, H * W // 900)):
            label += int(rng.integers(1, 4))
            cy, cx = int(rng.integers(0, H)), int(rng.integers(0, W))
            for _ in range(int(rng.integers(1, 4))):         # blobby: a union of ellipses
                ry, rx = int(rng.integers(4, 16)), int(rng.integers(4, 16))
                oy, ox = int(rng.integers(-6, 7)), int(rng.integers(-6, 7))
                seg[((yy - cy - oy) / ry) ** 2 + ((xx - cx - ox) / rx) ** 2 <= 1.0] = label
    if seg.max() > seg.size:                                 # the entry point takes labels up to H * W: renumber by rank
        values = np.unique(seg[seg > 0])
        seg = np.where(seg > 0, np.searchsorted(values, seg) + 1, 0).astype(np.int32)
    img = rng.integers(0, 50, (H, W, C)).astype(np.float64)
    img[seg > 0] += 35
    probes = [1, 0, 2][:n_probe] if seed % 2 else [0, 1, 2][:n_probe]
    for c in probes:
        for _ in range(max(2, H * W // 250)):                # soft bumps: the filter decides
            cy, cx = rng.uniform(0, H), rng.uniform(0, W)
            s = rng.uniform(0.6, 3.5) / scale
            img[..., c] += rng.uniform(40, 190) * np.exp(-((yy - cy) ** 2 + (xx - cx) ** 2) / (2 * s * s))
    img = np.clip(np.rint(img), 0, 254).astype(np.uint8)
    for c in probes:                                         # painted spots at the maximum: exact shapes of 1..40 pixels
        for _ in range(max(2, H * W // 700)):
            cy, cx = int(rng.integers(0, H)), int(rng.integers(0, W))
            n = int(rng.integers(1, 41))
            y, x = cy, cx
            for _ in range(n):                               # a random walk, diagonal steps included
                img[min(max(y, 0), H - 1), min(max(x, 0), W - 1), c] = 255
                y += int(rng.integers(-1, 2)); x += int(rng.integers(-1, 2))
    if mode == 5:
        img[..., probes[0]] = 255                            # saturated channel
    if mode == 6:
        img[..., probes[-1]] = 0                             # all-zero channel
    weights = proj_kernel(K, 3.0 / scale)
    normal = float(rng.choice([15.0, 15.0, 8.0, 30.0]))
    ithr = [float(rng.choice([70.0, 70.0, 40.0, 120.5])) for _ in probes]
    return _case(img, seg, probes, weights, normal, ithr, min_cc, line)


def full_size_scene(seed=1):
    """1040 x 1392 with about 300 nuclei, the reference's default parameters."""
    rng = np.random.default_rng(seed)
    H, W = 1040, 1392
    yy, xx = np.ogrid[:H, :W]
    seg = np.zeros((H, W), np.int32)
    for k in range(300):                                     # a jittered 15 x 20 grid: the nuclei stay apart
        cy = int((k // 20 + 0.5) * H / 15 + rng.integers(-5, 6))
        cx = int((k % 20 + 0.5) * W / 20 + rng.integers(-5, 6))
        ry, rx = int(rng.integers(16, 29)), int(rng.integers(16, 29))
        seg[((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2 <= 1.0] = 1
    img = rng.integers(0, 50, (H, W, 3)).astype(np.float64)
    img[seg > 0] += 30
    for c in (0, 1):
        for _ in range(1500):
            cy, cx = int(rng.integers(4, H - 4)), int(rng.integers(4, W - 4))
            s = rng.uniform(0.8, 3.0)
            y0, y1, x0, x1 = max(cy - 12, 0), min(cy + 13, H), max(cx - 12, 0), min(cx + 13, W)
            img[y0:y1, x0:x1, c] += rng.uniform(60, 200) * np.exp(-((yy[y0:y1] - cy) ** 2 + (xx[:, x0:x1] - cx) ** 2) / (2 * s * s))
    img = np.clip(np.rint(img), 0, 255).astype(np.uint8)
    return img, (seg != 0).astype(np.uint8) * np.uint8(255)


def make_item(seed, size, K, C, source, min_cc=None, picture=False, mask_file=True):
    """A seeded scene of tests/stat_fish_cases.py as an item of ``stat_fish_many``.  source: 'mask' (the scene's cells as a 0 / 255
    mask), 'labels' (its label map as given), 'background', 'foreground' (all-zero / all-255 masks)."""
    case = scene(seed, size=size, K=K, n_probe=2)
    rng = np.random.default_rng(seed + 77)
    H, W = size
    img = case['img']
    if img.shape[2] != C:                                    # the scene drew its own channel count: cut or add the aqua channel
        img = np.ascontiguousarray(img[..., :3]) if C == 3 else np.dstack([img, rng.integers(0, 200, (H, W, 1)).astype(np.uint8)])
    probes = list(case['probes']) + ([3] if C == 4 else [])
    blue = [c for c in range(C) if c not in probes][0]
    item = dict(img=np.ascontiguousarray(img), channels=[blue] + probes, weights=NAN1 if K == 1 else case['weights'],
                normal_threshold=case['normal'], intensity_thresholds=list(case['ithr']) + ([55.0] if C == 4 else []),
                min_cc_size=case['min_cc'] if min_cc is None else min_cc)
    seg = case['seg']
    if source == 'labels':
        item['labels'] = seg
    else:
        mask = {'mask': (seg != 0), 'background': np.zeros((H, W), bool), 'foreground': np.ones((H, W), bool)}[source]
        item['mask'] = mask.astype(np.uint8) * np.uint8(255)
        if mask_file:
            item['mask_file'] = True
    if picture:
        item['picture'] = rng.integers(0, 256, (H, W, 3)).astype(np.uint8)
    return item
