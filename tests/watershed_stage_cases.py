"""Cases for the STAGES of NuSeT's marker watershed (tests/watershed_ref.py: ``stages``; the device: ecseg_marker_watershed_stages_debug),
shared by tests/test_watershed_stages.py (the restatement against a second distance, and the mutants) and
tests/test_gpu_watershed_stages.py (device == restatement, stage by stage).  Plain numpy only.

A case is a dict: name, mask (uint8 0 / 1, H x W) and the ordered marker list rows, cols, labels (int32).  Unlike the cases of
tests/watershed_cases.py the list is given, not derived from proposals, so there is no 20-pixel edge and an extent may be 1.  The
images are small - the flood of the restatement is Python - and chosen for what a kernel gets wrong: extents below and beside the 64
columns of a block of the column pass and the 256 pixels of every other block, zeros placed so that every branch of the distance is
taken, labels whose order differs from the list's."""
import numpy as np

from watershed_cases import disc

INT32_MAX = 2 ** 31 - 1


def _case(name, mask, markers=()):
    """markers: (row, column, label) in list order."""
    mk = np.asarray(list(markers), np.int64).reshape(-1, 3)
    mask = np.ascontiguousarray(mask, np.uint8)
    assert mask.ndim == 2 and mask.max(initial=0) <= 1
    assert ((mk[:, 0] >= 0) & (mk[:, 0] < mask.shape[0]) & (mk[:, 1] >= 0) & (mk[:, 1] < mask.shape[1]) & (mk[:, 2] >= 1)).all(), name
    return dict(name=name, mask=mask, rows=mk[:, 0].astype(np.int32), cols=mk[:, 1].astype(np.int32), labels=mk[:, 2].astype(np.int32))


def ones(h, w):
    return np.ones((h, w), np.uint8)


EXTENTS = [(1, 1), (1, 64), (64, 1), (1, 200), (200, 1), (2, 2), (3, 65), (65, 3), (63, 64), (64, 65), (7, 129), (130, 5),
           (5, 51), (16, 16), (1, 257)]                    # the last three: 255, 256 and 257 pixels


def extent_case(H, W):
    """Foreground but for a zero in the last column of the first row and one in the middle of the last row (an image of fewer than 5
    pixels stays all ones); markers in the first and the last pixel and in the middle, the largest label first."""
    m = ones(H, W)
    if H * W >= 5:
        m[0, W - 1] = 0
        m[H - 1, W // 2] = 0
    mk = [(0, 0, 70000), (H - 1, W - 1, 3)]
    if H * W >= 5:
        mk.append((H // 2, W // 3, 12))
    return _case('extent_%dx%d' % (H, W), m, mk)


def fixed_cases():
    out = [extent_case(H, W) for H, W in EXTENTS]
    out.append(_case('one_pixel_background_with_marker', np.zeros((1, 1), np.uint8), [(0, 0, 4)]))
    out.append(_case('one_pixel_no_marker', ones(1, 1)))

    # ---- fill and distance ---------------------------------------------------------------------------------------------------
    out.append(_case('all_ones', ones(9, 70), [(4, 10, 2), (4, 60, 1)]))          # no zero: the distance to (-1, 0)
    out.append(_case('all_ones_tall', ones(70, 9), [(10, 4, 2), (60, 4, 1)]))
    out.append(_case('all_zeros', np.zeros((5, 7), np.uint8), [(2, 3, 1), (0, 0, 2)]))
    for name, (y, x) in (('top_left', (0, 0)), ('top_right', (0, 69)), ('bottom_left', (8, 0)), ('bottom_right', (8, 69)), ('middle', (4, 35))):
        m = ones(9, 70); m[y, x] = 0                         # one zero: the row search runs up to 69 columns (the one in the middle is a
                                                             # hole: `filled` is all ones under a mask that is not)
        out.append(_case('single_zero_' + name, m, [(4, 20, 1), (4, 50, 2)]))
    for x in (62, 63, 64, 65):                               # the other 129 columns hold no zero, in both blocks of the column pass
        m = ones(6, 130); m[:, x] = 0
        out.append(_case('zero_column_%d' % x, m, [(3, 10, 1), (3, 120, 2), (2, 66, 3)]))
    m = ones(6, 130); m[2, :] = 0
    out.append(_case('zero_row', m, [(0, 10, 1), (4, 100, 2), (5, 101, 3)]))
    m = ones(40, 70); m[23:, 5] = 0; m[20, 60:] = 0          # slits from the border (a lone inner zero is a hole); at (20, 5): 3 rows down
                                                             # or 55 columns along - the row search stops at dx = 3
    out.append(_case('zero_near_in_the_column_far_in_the_row', m, [(20, 5, 1), (20, 40, 2)]))
    m = ones(40, 70); m[5, 22:] = 0; m[35:, 20] = 0          # at (5, 20): 2 columns along or 30 rows down
    out.append(_case('zero_near_in_the_row_far_in_the_column', m, [(5, 20, 1), (30, 50, 2)]))
    m = ones(40, 70); m[0, 0] = 0; m[39, 69] = 0; m[0, 69] = 0   # the middle is about as far from three zeros: dx^2 >= best ends late
    out.append(_case('zeros_in_three_corners', m, [(20, 35, 1), (10, 10, 2), (30, 60, 3)]))

    m = np.zeros((14, 20), np.uint8); m[2:12, 3:17] = 1; m[5:8, 7:11] = 0
    out.append(_case('hole_closed', m, [(3, 4, 1), (10, 15, 2)]))
    m = np.zeros((14, 20), np.uint8); m[0:12, 3:17] = 1; m[0:8, 9] = 0          # a slit from the top border
    out.append(_case('hole_open_to_the_border', m, [(3, 4, 1), (3, 15, 2)]))
    m = np.zeros((9, 9), np.uint8); m[1:8, 1:8] = 1; m[3:6, 3:6] = 0; m[1, 1] = 0; m[2, 2] = 0     # (1, 1) - (2, 2) - (3, 3) touch by corners only
    out.append(_case('hole_closed_only_across_a_diagonal', m, [(1, 5, 1), (6, 6, 2)]))
    m = ones(12, 14); m[8:12, 5] = 0; m[3:6, 9] = 0
    out.append(_case('background_touching_the_last_row_only', m, [(2, 2, 1), (9, 11, 2)]))
    m = ones(12, 14); m[4, 9:14] = 0; m[8, 2:5] = 0
    out.append(_case('background_touching_the_last_column_only', m, [(2, 2, 1), (9, 11, 2)]))
    m = ones(12, 14); m[11, 13] = 0; m[5, 5] = 0
    out.append(_case('background_in_the_last_pixel_only', m, [(2, 2, 1), (9, 8, 2)]))

    # ---- markers -------------------------------------------------------------------------------------------------------------
    m = ones(10, 12); m[4:6, 5:7] = 0
    out.append(_case('markers_in_the_four_corners', m, [(0, 0, 4), (0, 11, 3), (9, 0, 2), (9, 11, 1)]))
    m = np.zeros((12, 24), np.uint8); m[2:10, 6:18] = 1
    out.append(_case('markers_on_the_background', m, [(5, 4, 1), (6, 19, 2), (0, 0, 3), (11, 12, 4)]))     # the discs reach in, or do not
    m = ones(11, 16); m[0, :] = 0
    out.append(_case('overlapping_discs_larger_label_first', m, [(5, 5, 9), (5, 8, 4)]))
    out.append(_case('overlapping_discs_larger_label_last', m, [(5, 5, 4), (5, 8, 9)]))
    out.append(_case('one_pixel_twice_smaller_label_last', m, [(5, 5, 7), (5, 5, 2), (5, 12, 5)]))
    out.append(_case('one_pixel_three_times', m, [(5, 5, 3), (5, 12, 5), (5, 5, 8), (5, 5, 1)]))
    out.append(_case('labels_up_to_int32_max', m, [(5, 4, INT32_MAX), (5, 11, INT32_MAX - 1), (8, 8, 1 << 30)]))
    m = ones(9, 11); m[3, 4:7] = 0; m[8, 0] = 0
    yy, xx = np.nonzero(m)
    out.append(_case('every_foreground_pixel_a_marker', m, [(y, x, 1 + (y * 11 + x) % 5) for y, x in zip(yy, xx)]))
    out.append(_case('every_foreground_pixel_the_same_marker', m, [(y, x, 6) for y, x in zip(yy, xx)]))
    out.append(_case('no_marker', m))

    # ---- the flood -----------------------------------------------------------------------------------------------------------
    m = np.zeros((8, 40), np.uint8); m[3:5, 1:39] = 1        # two rows: d2 = 1 on every pixel, every marker pixel ties
    out.append(_case('plateau_strip', m, [(3, 4, 1), (4, 20, 2), (3, 35, 3)]))
    m = np.zeros((16, 30), np.uint8); m[1:15, 1:29] = 1; m[4:12, 4:26] = 0      # a frame: its hole is filled, so d2 is the solid rectangle's - rings of one value
    out.append(_case('plateau_frame', m, [(2, 2, 1), (2, 27, 2), (13, 15, 3), (2, 15, 4)]))
    m = ones(11, 20); m[0, :] = 0
    out.append(_case('marker_pixels_become_lines', m, [(5, 5, 1), (5, 12, 2)]))  # the discs touch: columns 2..8 and 9..15
    m = np.zeros((20, 30), np.uint8); disc(m, 9, 8, 6); m[3:9, 20:27] = 1; m[15:18, 2:28] = 1
    out.append(_case('component_no_marker_reaches', m, [(9, 6, 1), (9, 11, 2), (16, 10, 3)]))

    m = ones(160, 160); m[0, 0] = 0; m[159, 100] = 0; m[60:64, 90:96] = 0; m[80, 64] = 0
    out.append(_case('large_160', m, [(40, 40, 5), (120, 100, 900000), (80, 130, 2), (40, 40, 1), (100, 30, INT32_MAX)]))
    return out


def random_case(seed):
    """A seeded scene over extents 1 .. 96: a density, rectangles set and cleared, markers anywhere (on background too, some pixels
    twice) with labels that tie, repeat or run up to 2^31 - 1."""
    rng = np.random.default_rng(7000 + seed)
    H, W = (int(v) for v in rng.integers(1, 97, 2))
    kind = int(rng.integers(0, 4))
    if kind == 0:
        m = (rng.random((H, W)) < rng.choice([0.5, 0.8, 0.95, 0.99])).astype(np.uint8)
    else:
        m = np.ones((H, W), np.uint8) if kind == 1 else np.zeros((H, W), np.uint8)
        for _ in range(int(rng.integers(1, 7))):
            y0, x0 = int(rng.integers(0, H)), int(rng.integers(0, W))
            y1, x1 = y0 + int(rng.integers(1, 40)), x0 + int(rng.integers(1, 40))
            m[y0:y1, x0:x1] = int(rng.random() < 0.6)
        if kind == 3:
            m[rng.random((H, W)) < 0.02] ^= 1
    n = int(rng.integers(0, 13))
    rows, cols = rng.integers(0, H, n), rng.integers(0, W, n)
    pool = [rng.integers(1, 4, n), rng.integers(1, INT32_MAX, n, endpoint=True), np.arange(n, 0, -1), np.arange(1, n + 1)][int(rng.integers(0, 4))]
    mk = [(int(r), int(c), int(l)) for r, c, l in zip(rows, cols, pool)]
    if n and rng.random() < 0.5:                             # a pixel of the list once more, with another label
        k = int(rng.integers(0, n))
        mk.append((mk[k][0], mk[k][1], int(rng.integers(1, 10))))
    return _case('stage_random_%d' % seed, m, mk)


SEEDS = range(48)


def all_cases():
    return fixed_cases() + [random_case(s) for s in SEEDS]
