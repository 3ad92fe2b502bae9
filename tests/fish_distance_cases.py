"""Inputs shared by tests/test_fish_distance.py, tests/test_gpu_fish_distance.py and tools/fuzz_fish_distance.py: the
hand-computed cases (one small map per rule of the gate, the spot limit, the cell mask and the distance) and a seeded random
scene generator.  Not a test module."""
import numpy as np

MAX_SPOTS = 3
SCENE_SIZES = ((96, 130), (64, 64), (65, 63), (200, 257), (1, 300), (300, 1), (128, 192), (37, 411), (3, 64), (150, 150))


def _blank(H, W, C=3):
    return np.zeros((H, W, C), np.uint8), np.zeros((H, W), np.int64)


def hand_cases():
    """name -> (lsq, seg, presets = (centromere index, fish index, max spots), expected list of values)."""
    cases = {}
    r8 = 8.0                                                 # sqrt(area) of the 8 x 8 cell below

    def cell8():
        lsq, seg = _blank(10, 12)
        seg[1:9, 1:9] = 1
        return lsq, seg
    lsq, seg = cell8(); lsq[2, 2, 0] = 9; lsq[5, 6, 1] = 7                   # dy = 3, dx = 4
    cases['triangle_3_4_5'] = (lsq, seg, (1, 0, MAX_SPOTS), [5 / r8])
    cases['triangle_swapped_colours'] = (lsq, seg, (0, 1, MAX_SPOTS), [5 / r8])
    lsq, seg = cell8(); lsq[2, 2, 0] = 9; lsq[5, 6, 1] = 7; lsq[4, 4, :2] = 1
    cases['pixel_of_both_colours'] = (lsq, seg, (1, 0, MAX_SPOTS), [0.0])
    lsq, seg = cell8(); lsq[2, 2, 0] = 9; lsq[5, 6, 1] = 7
    cases['same_colour_red'] = (lsq, seg, (0, 0, MAX_SPOTS), [0.0])
    cases['same_colour_green'] = (lsq, seg, (1, 1, MAX_SPOTS), [0.0])
    lsq, seg = cell8(); lsq[5, 6, 1] = 7; lsq[0, 0, 0] = 200; lsq[3, 3, 2] = 9     # red only outside the cell
    cases['gate_fails_on_channel_0'] = (lsq, seg, (1, 0, MAX_SPOTS), [])
    cases['gate_fails_on_channel_0_blue_probes'] = (lsq, seg, (2, 2, MAX_SPOTS), [])
    lsq, seg = cell8(); lsq[2, 2, 0] = 9; lsq[9, 9, 1] = 200
    cases['gate_fails_on_channel_1'] = (lsq, seg, (1, 0, MAX_SPOTS), [])
    lsq, seg = cell8(); lsq[7, 7, 1] = 7
    for k in range(MAX_SPOTS):
        lsq[1, 1 + 2 * k, 0] = 5
    cases['exactly_max_spots'] = (lsq, seg, (1, 0, MAX_SPOTS), [float(np.sqrt(36 + 4)) / r8])
    lsq = lsq.copy(); lsq[3, 1, 0] = 5
    cases['max_plus_one_spots'] = (lsq, seg, (1, 0, MAX_SPOTS), [])
    cases['max_plus_one_spots_allowed'] = (lsq, seg, (1, 0, MAX_SPOTS + 1), [float(np.sqrt(36 + 4)) / r8])   # the new spot is farther
    lsq, seg = cell8(); lsq[8, 8, 1] = 7; lsq[1, 1, 0] = lsq[2, 2, 0] = lsq[1, 3, 0] = 5      # one 8-connected spot
    cases['diagonal_touch_is_one_spot'] = (lsq, seg, (1, 0, 1), [float(np.sqrt(36 + 36)) / r8])
    lsq, seg = cell8(); lsq[8, 8, 1] = 7; lsq[1, 1, 0] = lsq[1, 3, 0] = 5                    # the same without the bridge
    cases['two_spots_over_a_limit_of_one'] = (lsq, seg, (1, 0, 1), [])
    lsq, seg = _blank(6, 12); seg[:, :6] = 1; seg[:, 6:] = 2
    lsq[2, 5, 0] = 5; lsq[2, 0, 1] = 7; lsq[2, 6, 1] = 7; lsq[0, 11, 0] = 5                  # cell 1: nearest own centromere is 5 away
    cases['nearer_centromere_of_the_neighbour_is_ignored'] = (lsq, seg, (1, 0, MAX_SPOTS), [5 / 6.0, float(np.sqrt(4 + 25)) / 6.0])
    lsq, seg = _blank(6, 12); seg[:, :6] = 1; seg[:, 6:] = 2
    lsq[2, 4:8, 0] = 5; lsq[4, 1, 0] = 5; lsq[0, 10, 0] = 5; lsq[5, 0, 1] = 7; lsq[5, 11, 1] = 7   # a spot across the border + one more each
    cases['spot_across_the_border_counts_once_per_cell'] = (lsq, seg, (1, 0, 2), [float(np.sqrt(1 + 1)) / 6.0, float(np.sqrt(9 + 16)) / 6.0])
    cases['spot_across_the_border_limit_one'] = (lsq, seg, (1, 0, 1), [])
    lsq, seg = cell8(); lsq[2, 2, 0] = 9; lsq[5, 6, 1] = 7
    cases['blue_fish_probe_is_empty'] = (lsq, seg, (1, 2, MAX_SPOTS), [float('inf')])
    cases['negative_limit_skips_even_without_fish'] = (lsq, seg, (1, 2, -1), [])
    lsq, seg = _blank(9, 9); seg[:] = -3; seg[0:3, 0:3] = 7; seg[6:9, 6:9] = 7; seg[4, 4] = 2   # two distant blobs of one label
    lsq[0, 0, 0] = 5; lsq[8, 8, 1] = 7; lsq[4, 4, :2] = 3
    cases['label_of_two_blobs_and_gaps_and_negatives'] = (lsq, seg, (1, 0, MAX_SPOTS), [0.0, float(np.sqrt(128)) / float(np.sqrt(18))])
    return cases


def scene(seed, size=None, C=3):
    """-> (lsq (H, W, C) uint8, seg (H, W) int64) with elliptical nuclei that overlap (adjacent cells, split labels), gaps in the
    label values, spots that spill over cell borders, and per cell one of the outcomes the reference distinguishes."""
    rng = np.random.default_rng(seed)
    H, W = size if size is not None else SCENE_SIZES[seed % len(SCENE_SIZES)]
    lsq = np.zeros((H, W, C), np.uint8)
    seg = np.zeros((H, W), np.int64)
    yy, xx = np.ogrid[:H, :W]
    n_cells = max(2, H * W // 350)
    label = 0
    for _ in range(n_cells):
        label += int(rng.integers(1, 4))
        ry, rx = int(rng.integers(3, 13)), int(rng.integers(3, 13))
        cy, cx = int(rng.integers(0, H)), int(rng.integers(0, W))
        seg[((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2 <= 1.0] = label
    if rng.integers(0, 4) == 0:
        seg[seg == label] = -int(rng.integers(1, 5))          # negative labels are background

    def spot(ch, y, x, big):
        r = int(rng.integers(1, 3)) if big else 0
        lsq[max(0, y - r):y + r + 1, max(0, x - r):x + r + 1, ch] = rng.integers(1, 256)
    for lab in np.unique(seg[seg > 0]):
        ys, xs = np.nonzero(seg == lab)
        mode = rng.choice(['normal', 'normal', 'many', 'no_red', 'no_green', 'both', 'empty'], p=[.3, .2, .15, .1, .1, .1, .05])

        def pick():
            k = int(rng.integers(0, len(ys)))
            return int(ys[k]), int(xs[k])
        if mode == 'empty':
            continue
        if mode == 'both':
            y, x = pick()
            lsq[y, x, 0] = lsq[y, x, 1] = 255
        if mode != 'no_red':
            for _ in range(int(rng.integers(4, 8)) if mode == 'many' else int(rng.integers(1, 4))):
                spot(0, *pick(), big=mode != 'many')
        if mode != 'no_green':
            for _ in range(int(rng.integers(1, 3))):
                spot(1, *pick(), big=True)
    if C > 2:
        lsq[..., 2] = (rng.random((H, W)) < 0.05) * 255        # the boundary drawing
    return lsq, seg


def outcomes(lsq, seg, fish_index, centromere_index, max_spots, records):
    """Counts of (finite > 0, 0.0, gate failure, skipped for spot count, inf) cells from the oracle's records."""
    fin = zero = gate = skip = inf = 0
    for r in records(lsq, seg, fish_index, centromere_index).tolist():
        if r[2] != 3:
            gate += 1
        elif r[5] > max_spots:
            skip += 1
        elif r[3] == 0:
            inf += 1
        elif r[6] == 0:
            zero += 1
        else:
            fin += 1
    return fin, zero, gate, skip, inf
