"""Inputs shared by tests/test_overlay_cases.py, tests/test_gpu_overlay.py and tools/fuzz_overlay.py: hand cases for the
``meta_overlay`` row (one small scene per rule of the nine counts and per branch of the device driver, each with its expected
row written out) and a seeded scene generator.  Not a test module.

A case is a dict: ``labels`` (H, W) uint8, ``rgb`` (H, W, C) uint8, ``sens`` (colour sensitivity) and ``thr`` (HSR size
threshold).  A row is the nine cells in CSV column order:

    cc(ec), cc(A), cc(B), coloc(ec, fish), coloc(ec, fish2), coloc(A, B), coloc(ec, fish & fish2), HSR(chrom, fish2), HSR(chrom, fish)

with fish = green & ~nuclei, fish2 = red & ~nuclei, A = fish & ~chrom, B = fish2 & ~chrom; nuclei / chrom / ec are the label
bytes EQUAL to 1 / 2 / 3.  The rules, in this file's words: components of the label masks and of A and B are 8-connected; a
``cc`` cell is (components, their pixels) and its second field is the float 0.0 when there is no component; a mask without a
single background pixel loses its only component in every count that walks its components (the pixel sum of ``cc`` becomes
0.0, a colocalisation or an HSR becomes 0); an HSR is a chromosome component touching a fish component that has at least
``thr`` pixels under 4-connectivity, measured after the nucleus pixels have left the fish; a pixel is fish when its channel
is strictly above ``sens``; red is channel 0, green channel 1, further channels are ignored."""
import numpy as np

from ecseg_amd import synth
from oracle import overlay as oracle_overlay
from oracle import postproc

EXTENTS = ((1, 1), (1, 64), (64, 1), (2, 2), (31, 65), (32, 64), (33, 64), (63, 65), (64, 128), (65, 129), (96, 160), (150, 333),
           (200, 260))
SENSITIVITIES = (0, 30, 85, 120, 254, 255)
THRESHOLDS = (0, 1, 5, 20, 21, 400)
CHANNELS = (2, 3, 4)
N_MODES = 7
N_SEEDS = 40                   # committed seeds of the scene generator: tests/test_overlay_cases.py holds their coverage conditions
TILE_H, TILE_W = 32, 64        # the device labelling's tile


def _case(labels, rgb, sens=85, thr=20):
    labels = np.ascontiguousarray(labels, np.uint8)
    rgb = np.ascontiguousarray(rgb, np.uint8)
    assert labels.ndim == 2 and rgb.ndim == 3 and rgb.shape[:2] == labels.shape
    return dict(labels=labels, rgb=rgb, sens=int(sens), thr=int(thr))


def oracle_row(case):
    """The oracle's nine cells of a case: ``oracle.overlay.overlay_row``, its two HSR cells taken at the case's threshold."""
    labels, rgb, sens, thr = case['labels'], case['rgb'], case['sens'], case['thr']
    row = oracle_overlay.overlay_row(labels, rgb, sens)
    if thr != postproc.HSR_SIZE_THRESHOLD:
        red, green = oracle_overlay.split_fish(rgb, sens)
        chrom, not_nuclei = labels == 2, labels != 1
        row[7] = postproc.count_HSR(chrom, red & not_nuclei, thr)
        row[8] = postproc.count_HSR(chrom, green & not_nuclei, thr)
    return row


def same_row(a, b):
    """Exact equality of two rows of nine cells, the int / float kind of the pixel field included (it is CSV text)."""
    a, b = list(a), list(b)
    return len(a) == len(b) == 9 and a == b and all(type(x[1]) is type(y[1]) for x, y in zip(a[:3], b[:3]))


def _row(ec=(0, 0.0), a=(0, 0.0), b=(0, 0.0), ec_g=0, ec_r=0, ab=0, ec_rg=0, hsr_r=0, hsr_g=0):
    return [ec, a, b, ec_g, ec_r, ab, ec_rg, hsr_r, hsr_g]


R, G = 0, 1


def hand_cases():
    """name -> (case, expected row of nine cells)."""
    cases = {}

    def blank(H, W, C=3):
        return np.zeros((H, W), np.uint8), np.zeros((H, W, C), np.uint8)

    # ---- the missing-background quirk, per key -------------------------------------------------------------------------------
    lab, rgb = blank(4, 5); lab[:] = 3; rgb[..., :2] = 255
    cases['quirk_all_ec'] = (_case(lab, rgb), _row(ec=(1, 0.0), a=(1, 0.0), b=(1, 0.0)))
    lab, rgb = blank(4, 5); lab[:] = 3; lab[0, 0] = 0; rgb[..., :2] = 255              # A and B still cover the image
    cases['quirk_all_ec_but_one_pixel'] = (_case(lab, rgb), _row(ec=(1, 19), a=(1, 0.0), b=(1, 0.0), ec_g=1, ec_r=1, ec_rg=1))
    lab, rgb = blank(4, 5); lab[:] = 2; rgb[..., R] = 255                               # the red blob has 20 pixels: kept
    cases['quirk_all_chrom'] = (_case(lab, rgb, thr=20), _row())
    lab, rgb = blank(4, 5); lab[:] = 2; lab[0, 0] = 0; rgb[..., R] = 255
    cases['quirk_all_chrom_but_one_pixel'] = (_case(lab, rgb, thr=20), _row(b=(1, 1), hsr_r=1))
    lab, rgb = blank(4, 5); rgb[..., G] = 255; rgb[1, 1, R] = 255
    cases['quirk_all_green_on_empty_labels'] = (_case(lab, rgb), _row(a=(1, 0.0), b=(1, 1)))
    lab, rgb = blank(4, 5); rgb[..., G] = 255; rgb[0, 0, G] = 0; rgb[1, 1, R] = 255
    cases['quirk_all_green_but_one_pixel'] = (_case(lab, rgb), _row(a=(1, 19), b=(1, 1), ab=1))
    lab, rgb = blank(4, 5); lab[:] = 2; rgb[..., :2] = 255                              # no ecDNA at all: see quirk_batch()
    cases['quirk_all_chrom_both_colours'] = (_case(lab, rgb, thr=2), _row())

    # ---- chromosomes and ecDNA are labelled in one pass: the keys stay apart ----------------------------------------------------
    def touching():
        lab, rgb = blank(6, 8)
        lab[2:4, 2:4] = 2
        lab[2, 4] = 3                                         # 4-adjacent to the chromosome
        lab[4, 4] = 3                                         # diagonal to the chromosome; two rows from the other ec pixel
        return lab, rgb
    lab, rgb = touching(); rgb[2, 2, G] = rgb[3, 2, G] = 255
    cases['keys_apart_fish_on_chromosome'] = (_case(lab, rgb, thr=1), _row(ec=(2, 2), hsr_g=1))
    lab, rgb = touching(); rgb[2, 4, G] = 255
    cases['keys_apart_fish_on_adjacent_ec'] = (_case(lab, rgb, thr=1), _row(ec=(2, 2), a=(1, 1), ec_g=1))
    lab, rgb = touching(); rgb[2, 4, G] = rgb[4, 4, G] = 255
    cases['keys_apart_fish_on_both_ec'] = (_case(lab, rgb, thr=1), _row(ec=(2, 2), a=(2, 2), ec_g=2))

    # ---- connectivity -----------------------------------------------------------------------------------------------------------
    lab, rgb = blank(5, 5); lab[1, 1] = lab[2, 2] = lab[3, 3] = 3; rgb[3, 3, G] = 255
    cases['diagonal_ec_is_one_component'] = (_case(lab, rgb), _row(ec=(1, 3), a=(1, 1), ec_g=1))

    def two_pieces():
        lab, rgb = blank(8, 12)
        rgb[1:3, 1:6, R] = 255                                # 10 pixels
        rgb[3:5, 6:11, R] = 255                               # 10 pixels, touching the first piece only at (2, 5) - (3, 6)
        lab[2, 4] = lab[2, 5] = lab[3, 6] = lab[3, 7] = 2     # one chromosome under both pieces
        return lab, rgb
    lab, rgb = two_pieces()
    cases['red_pieces_touching_diagonally_are_too_small'] = (_case(lab, rgb, thr=20), _row(b=(2, 16)))
    lab, rgb = two_pieces(); rgb[2, 6, R] = 255               # the bridge: 21 pixels under 4-connectivity
    cases['red_pieces_with_a_bridge_are_one_blob'] = (_case(lab, rgb, thr=20), _row(b=(2, 17), hsr_r=1))

    # ---- the size threshold: strict '<' drops -----------------------------------------------------------------------------------
    def bar(n):
        lab, rgb = blank(6, 12)                               # H * W = 72
        rgb[1:3, 1:11, R] = 255                               # 20 pixels
        if n == 19:
            rgb[2, 10, R] = 0
        if n == 21:
            rgb[3, 1, R] = 255
        lab[1, 1] = lab[1, 2] = 2
        return lab, rgb
    for n, b_px in ((19, 17), (20, 18), (21, 19)):
        for thr, hsr in ((20, 1 if n >= 20 else 0), (0, 1), (1, 1), (2, 1), (73, 0)):
            lab, rgb = bar(n)
            cases['red_bar_of_%d_at_threshold_%d' % (n, thr)] = (_case(lab, rgb, thr=thr), _row(b=(1, b_px), hsr_r=hsr))
    for thr, hsr in ((0, 1), (1, 1), (2, 0), (10, 0)):
        lab, rgb = blank(3, 3); lab[1, 1] = 2; rgb[1, 1, R] = 255
        cases['one_red_pixel_at_threshold_%d' % thr] = (_case(lab, rgb, thr=thr), _row(hsr_r=hsr))

    # ---- nucleus pixels leave the fish before the size filter -------------------------------------------------------------------
    lab, rgb = blank(8, 8); rgb[1:6, 1:6, R] = 255; lab[1, 1:6] = 1; lab[2, 1] = 1; lab[5, 5] = 2
    cases['red_25_minus_6_under_a_nucleus'] = (_case(lab, rgb, thr=20), _row(b=(1, 18)))
    lab, rgb = blank(8, 8); rgb[1:6, 1:6, R] = 255; lab[1, 1:6] = 1; lab[5, 5] = 2
    cases['red_25_minus_5_under_a_nucleus'] = (_case(lab, rgb, thr=20), _row(b=(1, 19), hsr_r=1))
    lab, rgb = blank(7, 11); rgb[1:6, 1:10, R] = 255          # 45 pixels
    lab[1:4, 5] = 1; lab[4:6, 4] = 1                          # the cut: 18 pixels left of it, 22 right, diagonal contact only
    lab[1, 1] = 2; lab[1, 9] = 2                              # one chromosome in each part
    cases['red_45_cut_into_22_and_18'] = (_case(lab, rgb, thr=20), _row(b=(1, 38), hsr_r=1))
    lab, rgb = blank(3, 4); lab[1, 1] = 3; lab[1, 2] = 1; rgb[1, 2, G] = 255
    cases['green_on_a_nucleus_is_not_fish'] = (_case(lab, rgb), _row(ec=(1, 1)))

    # ---- flag bits are independent ----------------------------------------------------------------------------------------------
    lab, rgb = blank(3, 5); lab[1, 1:4] = 3; rgb[1, 1, R] = 255; rgb[1, 3, G] = 255
    cases['ec_with_red_and_green_on_different_pixels'] = (_case(lab, rgb), _row(ec=(1, 3), a=(1, 1), b=(1, 1), ec_g=1, ec_r=1))
    lab, rgb = blank(3, 5); lab[1, 1:4] = 3; rgb[1, 2, R] = rgb[1, 2, G] = 255
    cases['ec_with_red_and_green_on_one_pixel'] = (_case(lab, rgb), _row(ec=(1, 3), a=(1, 1), b=(1, 1), ec_g=1, ec_r=1, ab=1, ec_rg=1))
    lab, rgb = blank(4, 5); lab[1:3, 1:4] = 2; rgb[1:3, 1:3, G] = 255; rgb[2, 3, R] = 255
    cases['chromosome_with_large_green_and_small_red'] = (_case(lab, rgb, thr=4), _row(hsr_g=1))
    lab, rgb = blank(4, 5); lab[1:3, 1:4] = 2; rgb[1:3, 1:3, R] = 255; rgb[2, 3, G] = 255
    cases['chromosome_with_large_red_and_small_green'] = (_case(lab, rgb, thr=4), _row(hsr_r=1))

    # ---- flags reach the root across tiles --------------------------------------------------------------------------------------
    def hook(key):                                            # row 30 from x = 60 to 66, then down column 66 to row 34: 11 pixels
        lab, rgb = blank(36, 70)
        lab[30, 60:67] = key
        lab[31:35, 66] = key
        return lab, rgb
    lab, rgb = hook(3); rgb[34, 66, G] = 255                  # first raster pixel in tile (0, 0), the fish in tile (1, 1)
    cases['ec_across_four_tiles_fish_in_the_last'] = (_case(lab, rgb), _row(ec=(1, 11), a=(1, 1), ec_g=1))
    lab, rgb = hook(2); rgb[34, 66, R] = 255
    cases['chromosome_across_four_tiles_fish_in_the_last'] = (_case(lab, rgb, thr=1), _row(hsr_r=1))
    for key in (2, 3):                                        # a diagonal through the corner where the four tiles meet
        lab, rgb = blank(36, 70)
        for k in range(4):
            lab[30 + k, 62 + k] = key
        rgb[33, 65, G] = 255
        cases['diagonal_through_the_tile_corner_key_%d' % key] = (
            _case(lab, rgb, thr=1), _row(hsr_g=1) if key == 2 else _row(ec=(1, 4), a=(1, 1), ec_g=1))
    lab, rgb = blank(8, 8); lab[1, 1] = lab[5, 5] = 3; rgb[5, 5, G] = 255
    cases['second_ec_of_a_tile_has_the_fish'] = (_case(lab, rgb), _row(ec=(2, 2), a=(1, 1), ec_g=1))
    lab, rgb = blank(8, 8); lab[1, 1] = lab[5, 5] = 2; rgb[5, 5, R] = 255
    cases['second_chromosome_of_a_tile_has_the_fish'] = (_case(lab, rgb, thr=1), _row(hsr_r=1))

    # ---- full tiles: a 64 x 32 tile of one key has a single owner ----------------------------------------------------------------
    def full(key, tiles):
        lab, rgb = blank(96, 160)
        for ty, tx in tiles:
            lab[TILE_H * ty:TILE_H * (ty + 1), TILE_W * tx:TILE_W * (tx + 1)] = key
        y1, x1 = TILE_H * (1 + max(t[0] for t in tiles)), TILE_W * (1 + max(t[1] for t in tiles))
        lab[y1, 0:10] = key                                   # the component goes on into the tile below: 10 pixels
        lab[0:5, x1] = key                                    # and into the tile to the right: 5 pixels
        lab[80, 150] = key                                    # a second component, never with fish
        return lab, rgb
    ONE, ROW2, COL2 = ((0, 0),), ((0, 0), (0, 1)), ((0, 0), (1, 0))
    for name, tiles, px, inside, beside in (('one_full_tile', ONE, 2048 + 15, (10, 10), (32, 9)),
                                            ('two_full_tiles_side_by_side', ROW2, 4096 + 15, (5, 100), (32, 9)),
                                            ('two_full_tiles_one_above_the_other', COL2, 4096 + 15, (40, 63), (4, 64))):
        for where, (y, x) in (('inside', inside), ('beside', beside)):
            lab, rgb = full(2, tiles); rgb[y, x, R] = 255
            cases['chromosome_%s_fish_%s' % (name, where)] = (_case(lab, rgb, thr=1), _row(hsr_r=1))
            lab, rgb = full(3, tiles); rgb[y, x, G] = 255
            cases['ec_%s_fish_%s' % (name, where)] = (_case(lab, rgb), _row(ec=(2, px + 1), a=(1, 1), ec_g=1))
    lab, rgb = full(2, ONE); rgb[80, 150, R] = 255            # the fish on the small component only
    cases['chromosome_one_full_tile_fish_on_the_other_component'] = (_case(lab, rgb, thr=1), _row(hsr_r=1))
    lab, rgb = full(2, ONE); rgb[80, 150, R] = rgb[31, 63, R] = 255
    cases['chromosome_one_full_tile_fish_on_both_components'] = (_case(lab, rgb, thr=1), _row(hsr_r=2))
    lab, rgb = full(3, ONE)
    cases['ec_one_full_tile_without_fish'] = (_case(lab, rgb), _row(ec=(2, 2064)))

    # ---- the sensitivity is a strict '>' ------------------------------------------------------------------------------------------
    for sens, value, fish in ((100, 100, 0), (100, 101, 1), (0, 0, 0), (0, 1, 1), (254, 254, 0), (254, 255, 1), (255, 255, 0)):
        lab, rgb = blank(3, 3); lab[1, 1] = 3; rgb[1, 1, G] = value
        cases['green_%d_at_sensitivity_%d' % (value, sens)] = (
            _case(lab, rgb, sens=sens), _row(ec=(1, 1), a=(1, 1), ec_g=1) if fish else _row(ec=(1, 1)))

    # ---- channels: red is 0, green is 1, the rest is ignored ----------------------------------------------------------------------
    def two_colours(C):
        lab, rgb = blank(3, 6, C); lab[1, 1:5] = 3; rgb[1, 1:3, R] = 255; rgb[1, 4, G] = 255
        return lab, rgb
    want = dict(ec=(1, 4), a=(1, 1), b=(1, 2), ec_g=1, ec_r=1)
    lab, rgb = two_colours(2)
    cases['two_channels'] = (_case(lab, rgb), _row(**want))
    lab, rgb = two_colours(4); rgb[..., 2:] = 255
    cases['four_channels_the_last_two_saturated'] = (_case(lab, rgb), _row(**want))
    lab, rgb = two_colours(3); rgb[..., 2] = 255
    cases['saturated_blue'] = (_case(lab, rgb), _row(**want))

    # ---- label bytes above 3 are nothing: not nucleus, not chromosome, not ecDNA ----------------------------------------------------
    for v in (4, 5, 6, 7, 255):
        lab, rgb = blank(4, 4); lab[1:3, 1:3] = v; rgb[1:3, 1:3, :2] = 255
        cases['label_byte_%d_is_background' % v] = (_case(lab, rgb, thr=2), _row(a=(1, 4), b=(1, 4), ab=1))
    lab, rgb = blank(4, 24)
    for k, v in enumerate((4, 5, 6, 7, 255)):
        lab[1:3, 1 + 4 * k:3 + 4 * k] = v; rgb[1:3, 1 + 4 * k:3 + 4 * k, :2] = 255
    cases['label_bytes_above_3_together'] = (_case(lab, rgb, thr=2), _row(a=(5, 20), b=(5, 20), ab=5))
    lab, rgb = blank(3, 4); lab[1, 1] = 2; lab[1, 2] = 6; rgb[1, 2, R] = 255
    cases['label_byte_6_does_not_extend_a_chromosome'] = (_case(lab, rgb, thr=1), _row(b=(1, 1)))
    lab, rgb = blank(3, 4); lab[1, 1] = 3; lab[1, 2] = 7; rgb[1, 2, G] = 255
    cases['label_byte_7_does_not_extend_an_ec'] = (_case(lab, rgb), _row(ec=(1, 1), a=(1, 1)))
    lab, rgb = blank(4, 5); lab[:] = 2; lab[0, 0] = 6; rgb[..., R] = 255
    cases['label_byte_6_is_background_for_the_quirk'] = (_case(lab, rgb, thr=20), _row(b=(1, 1), hsr_r=1))
    lab, rgb = blank(96, 160); lab[:TILE_H, :TILE_W] = 6; rgb[3, 3, R] = 255
    cases['full_tile_of_label_byte_6'] = (_case(lab, rgb, thr=1), _row(b=(1, 1)))

    # ---- empty inputs ---------------------------------------------------------------------------------------------------------------
    lab, rgb = blank(6, 6); rgb[1, 1:4, G] = 255; rgb[4, 4:6, R] = 255
    cases['empty_labels_with_fish'] = (_case(lab, rgb), _row(a=(1, 3), b=(1, 2)))
    lab, rgb = blank(6, 6); lab[0, 0:2] = 3; lab[3, 3] = 2; lab[5, 5] = 1
    cases['labels_without_fish'] = (_case(lab, rgb), _row(ec=(1, 2)))
    lab, rgb = blank(1, 1)
    cases['one_empty_pixel'] = (_case(lab, rgb), _row())
    return cases


def quirk_batch():
    """Three 4 x 5 images for ONE call (sensitivity 85, threshold 2): all chromosome, all ecDNA and an ordinary one, each with
    its expected row.  A quirk of one image must not reach its neighbours' counters."""
    labels = np.zeros((3, 4, 5), np.uint8)
    rgb = np.zeros((3, 4, 5, 3), np.uint8)
    labels[0] = 2; rgb[0, ..., :2] = 255
    labels[1] = 3; rgb[1, ..., :2] = 255
    labels[2, 0] = [3, 3, 0, 2, 2]
    rgb[2, 0, [0, 3, 4], G] = 255                             # green: on the ec, and a 2-pixel blob on the chromosome
    rgb[2, 0, [1, 3], R] = 255                                # red: two single pixels, below the threshold
    rows = [_row(),
            _row(ec=(1, 0.0), a=(1, 0.0), b=(1, 0.0)),
            _row(ec=(1, 2), a=(1, 1), b=(1, 1), ec_g=1, ec_r=1, hsr_g=1)]
    return labels, rgb, 85, 2, rows


# ---- the seeded generator ---------------------------------------------------------------------------------------------------------
def _discs_and_rings(rng, H, W):
    lab = np.zeros((H, W), np.uint8)
    yy, xx = np.ogrid[:H, :W]
    for _ in range(max(3, H * W // 600)):
        cy, cx, r = int(rng.integers(0, H)), int(rng.integers(0, W)), int(rng.integers(1, 9))
        d2 = (yy - cy) ** 2 + (xx - cx) ** 2
        cls = int(rng.choice([1, 2, 2, 3, 3]))
        lab[d2 <= r * r] = cls
        if rng.random() < 0.4:
            lab[d2 <= (r // 2) ** 2] = int(rng.choice([0, 2, 3]))      # a ring, or a ring around another class
    return lab


def _fill_tiles(rng, lab):
    """One class over whole tiles of the device labelling (or over the whole image where it is smaller than a tile)."""
    H, W = lab.shape
    ny, nx = H // TILE_H, W // TILE_W
    cls = int(rng.choice([2, 3]))
    if ny == 0 or nx == 0:
        lab[:, :] = cls
        lab[int(rng.integers(0, H)), int(rng.integers(0, W))] = 0
        return
    for _ in range(int(rng.integers(1, 4))):
        ty, tx = int(rng.integers(0, ny)), int(rng.integers(0, nx))
        lab[TILE_H * ty:TILE_H * (ty + 1), TILE_W * tx:TILE_W * (tx + 1)] = cls


def _labels(rng, seed, mode, H, W):
    if mode == 0:
        return np.ascontiguousarray(synth.label_map(seed, max(H, 48), max(W, 48))[:H, :W])
    if mode == 1:
        return rng.choice(4, size=(H, W), p=rng.dirichlet([3.0, 1.0, 1.0, 1.0])).astype(np.uint8)
    if mode == 4:                                             # one class everywhere; the later rounds leave one pixel out
        lab = np.full((H, W), (3, 2, 0)[(seed // N_MODES) % 3], np.uint8)
        if (seed // N_MODES) % 6 >= 3:
            lab[int(rng.integers(0, H)), int(rng.integers(0, W))] = int(rng.choice([0, 1, 2, 3]))
        return lab
    lab = _discs_and_rings(rng, H, W)
    if mode in (3, 6):
        _fill_tiles(rng, lab)
    if mode in (5, 6):                                        # a few percent of bytes above 3
        m = rng.random((H, W)) < 0.04
        lab[m] = rng.choice([4, 5, 6, 7, 8, 127, 254, 255], size=int(m.sum()))
    return lab


def _blob(mask, y0, x0, n, w):
    """``n`` pixels in raster order inside a box ``w`` wide from (y0, x0): 4-connected; cut at the image border."""
    H, W = mask.shape
    k = np.arange(n)
    y, x = y0 + k // w, x0 + k % w
    ok = (y >= 0) & (y < H) & (x >= 0) & (x < W)
    mask[y[ok], x[ok]] = True


def _fish(rng, lab, thr, everywhere):
    """A boolean fish mask: blobs whose sizes straddle ``thr``, on, beside and diagonal to chromosome and ec components."""
    H, W = lab.shape
    m = np.zeros((H, W), bool)
    if everywhere:
        m[:] = True
        return m
    ys, xs = np.nonzero((lab == 2) | (lab == 3))
    sizes = [max(thr - 1, 1), max(thr, 1), thr + 1, 1, 2, 3 * thr + 2, max(thr // 2, 1)]
    for _ in range(max(3, H * W // 500)):
        n = int(rng.choice(sizes))
        w = int(rng.integers(1, max(2, int(2 * np.sqrt(n)) + 1)))
        if len(ys) and rng.random() < 0.75:                   # anchored on a labelled pixel, or one step / one diagonal step off it
            k = int(rng.integers(0, len(ys)))
            dy, dx = ((0, 0), (0, 0), (0, 1), (1, 0), (0, -1), (-1, 0), (1, 1), (-1, -1), (1, -1), (-1, 1))[int(rng.integers(0, 10))]
            y0, x0 = int(ys[k]) + dy, int(xs[k]) + dx
        else:
            y0, x0 = int(rng.integers(0, H)), int(rng.integers(0, W))
        _blob(m, y0, x0, n, w)
    return m


def _channel(rng, fish, sens):
    """A uint8 channel whose pixels above ``sens`` are exactly ``fish`` plus salt at ``sens + 1``; salt at ``sens`` stays off."""
    H, W = fish.shape
    low = rng.integers(0, sens + 1, (H, W))
    salt = rng.random((H, W))
    low[salt < 0.01] = sens                                   # the largest value that is not fish
    if sens >= 255:
        return low.astype(np.uint8)                           # nothing can be fish
    high = rng.integers(sens + 1, 256, (H, W))
    high[salt > 0.99] = sens + 1                              # the smallest value that is fish
    on = fish | (rng.random((H, W)) < 0.004)
    return np.where(on, high, low).astype(np.uint8)


def scene(seed, size=None, C=None, sens=None, thr=None):
    """A seeded scene -> case dict."""
    rng = np.random.default_rng(seed + 2000003)
    H, W = size if size is not None else EXTENTS[seed % len(EXTENTS)]
    pick = [int(rng.integers(0, 6)), int(rng.integers(0, 6)), int(rng.integers(0, 3))]
    sens = SENSITIVITIES[pick[0]] if sens is None else sens
    thr = THRESHOLDS[pick[1]] if thr is None else thr
    C = CHANNELS[pick[2]] if C is None else C
    mode = seed % N_MODES
    lab = _labels(rng, seed, mode, H, W)
    rgb = rng.integers(0, 256, (H, W, C)).astype(np.uint8)    # channels 2.. stay noise
    rgb[..., G] = _channel(rng, _fish(rng, lab, thr, everywhere=(mode == 4)), sens)
    rgb[..., R] = _channel(rng, _fish(rng, lab, thr, everywhere=(mode == 4 and (seed // N_MODES) % 2 == 1)), sens)
    return _case(lab, rgb, sens, thr)


def batch(n, extent, seed0=7000, sens=85, thr=20, C=3):
    """``n`` different scenes of one extent for one call -> (labels (n, H, W), rgb (n, H, W, C), sens, thr)."""
    scenes = [scene(seed0 + i, size=extent, C=C, sens=sens, thr=thr) for i in range(n)]
    return np.stack([s['labels'] for s in scenes]), np.stack([s['rgb'] for s in scenes]), sens, thr
