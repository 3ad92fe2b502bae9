"""Inputs for the tests of the clean-up stages of meta_inference one at a time (test_meta_stages.py on the host,
test_gpu_meta_stages.py on the device; references and stage numbers: meta_stage_ref.py).  Seeded and deterministic.

``cases(k)`` -> the list of ``Case`` for stage k: ``x`` is an (n, H, W) uint8 batch that is fed DIRECTLY to the stage, ``check``
(hand cases) takes the batch and says whether the branch the case is named for is taken, on the oracle's own intermediates.

  extents    seeded scenes (rectangles of every class with cores and holes, specks) at every extent of EXTENTS, three different
             images per call; (66, 131) is (66, 132) without its last column, which is empty: the v4 / not-v4 pair
  fuzz       test_gpu_fuzz._random_labels at three small extents - images no earlier stage would hand on
  hand       per stage, below
"""
import collections
import functools
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import meta_stage_ref as ref                     # noqa: E402
from test_gpu_fuzz import _random_labels         # noqa: E402

Case = collections.namedtuple('Case', 'name x check')

# degenerate extents (thinner than the halo of every tile kernel), one 64 x 32 tile exactly, one pixel more, one less, the
# v4 / not-v4 pair, and several tiles both ways
EXTENTS = [(1, 1), (1, 7), (7, 1), (2, 2), (2, 65), (65, 2), (1, 130), (32, 64), (33, 65), (31, 63), (66, 132), (66, 131), (96, 200)]
V4_PAIR = ((66, 132), (66, 131))
FUZZ_EXTENTS = [(31, 63), (33, 65), (66, 131)]
PAIR_STRIP, BINNED_STRIP = (3, 32770), (3, 2000)   # beyond NUCLEUS_BIN_EXTENT = 32768: the pair test; the same content cropped: binned
# columns next to the cut of the v4 pair that a stage's stencils can make differ (the wide image's last column is empty, so
# components, areas, centroids and holes are those of the cropped image): stage 3 erodes with radius 1 (pads with 1 at the cropped
# image's edge, sees the empty column in the wide one), stage 5 opens with radius 2 (reflect), stage 6 adds the dilation: 3
PAIR_FOOTPRINT = {1: 0, 2: 0, 3: 1, 4: 0, 5: 2, 6: 3}


def _scene(rng, H, W, speck):
    img = np.zeros((H, W), np.uint8)
    for _ in range(int(rng.integers(2, 5 + H * W // 120))):
        c = int(rng.choice([1, 2, 3, 3, 2, 1, 0]))
        h, w = int(rng.integers(1, max(2, H // 2 + 1))), int(rng.integers(1, max(2, W // 3 + 1)))
        y = int(rng.choice([0, max(H - h, 0), int(rng.integers(0, H))]))
        x = int(rng.choice([0, max(W - w, 0), int(rng.integers(0, W))]))
        img[y:y + h, x:x + w] = c
        if h >= 3 and w >= 3 and rng.random() < 0.6:          # a core of another class, or a hole
            img[y + 1:y + h - 1, x + 1:x + w - 1] = int(rng.integers(0, 4))
    if speck:
        m = rng.random((H, W)) < speck
        img[m] = rng.integers(0, 4, int(m.sum()))
    return img


@functools.lru_cache(maxsize=None)
def extent_batch(H, W):
    """Three different images of H x W (1 x 1: the four there are)."""
    if (H, W) == (1, 1):
        return np.arange(4, dtype=np.uint8).reshape(4, 1, 1)
    if (H, W) == V4_PAIR[1]:
        return np.ascontiguousarray(extent_batch(*V4_PAIR[0])[:, :, :W])
    rng = np.random.default_rng(7000 + 1000 * H + W)
    x = np.stack([_scene(rng, H, W, speck) for speck in (0.0, 0.03, 0.15)])
    if (H, W) == V4_PAIR[0]:
        x[:, :, -1] = 0
    return x


@functools.lru_cache(maxsize=None)
def fuzz_batch(H, W):
    rng = np.random.default_rng(8000 + 1000 * H + W)
    return np.stack([_random_labels(rng, H, W) for _ in range(3)])


def _canvas(H, W, fill=0):
    return np.full((H, W), fill, np.uint8)


def _one(img):
    return np.ascontiguousarray(img[None])


# ---- stages 1 and 2: fill_holes ----------------------------------------------------------------------------------------------
def _fill_cases(c):
    o = 3 - c                                                  # the other class, inside some holes
    out = []
    for H, W in ((33, 65), (40, 80)):                          # not v4 / v4
        # a wall of c closing a pocket against each image edge: the pocket touches that edge only, so it stays open
        for edge in ('top', 'bottom', 'left', 'right'):
            img = _canvas(H, W)
            img[10:20, 20:32] = c
            img[11:19, 21:31] = 0
            img[14, 25] = o
            pocket = _canvas(12, 14, c)
            pocket[:10, 2:12] = 0                              # open towards the top of the patch
            pocket[4, 6] = 3
            k = dict(top=0, left=1, bottom=2, right=3)[edge]
            p = np.rot90(pocket, k)
            ph, pw = p.shape
            y, x = dict(top=(0, 40), bottom=(H - ph, 40), left=(4, 0), right=(4, W - pw))[edge]
            img[y:y + ph, x:x + pw] = p

            def check(x, edge=edge, c=c):
                # the pocket is background of the fill pass that reaches this edge and no other; the closed ring is a real hole
                a = x[0]
                lab, n = ref.P.label4(a != c)
                rows = dict(top=lab[0, :], bottom=lab[-1, :], left=lab[:, 0], right=lab[:, -1])
                only = set(np.unique(rows[edge])) - {0}
                for e, r in rows.items():
                    if e != edge:
                        only -= set(np.unique(r))
                return len(only) >= 1 and (ref.stage(c, a) != a).any()
            out.append(Case('pocket_open_to_%s_%dx%d' % (edge, H, W), _one(img), check))
    # a ring of c that leaks through a diagonal gap only: closed for the 4-connected background, open for an 8-connected one
    img = _canvas(33, 65)
    img[5:15, 5:15] = c
    img[6:14, 6:14] = 0
    img[5, 14] = 0                                             # the corner pixel of the ring: (6, 13) inside touches (5, 14) diagonally
    img[8, 8] = o

    def check_diag(x, c=c):
        a = x[0]
        return ref.P.label4(a != c)[1] == ref.P.label8(a != c)[1] + 1 and a[6, 13] == 0 and ref.stage(c, a)[6, 13] == c
    out.append(Case('diagonal_leak', _one(img), check_diag))
    # a hole that holds a whole labelling tile (rows 32..63, columns 64..127) of other classes, and one at the tile corner
    img = _canvas(96, 200)
    img[20:76, 50:141] = c
    img[24:72, 54:137] = 0
    img[40:50, 80:100] = o
    img[44, 90] = 3
    img[0:8, 150:160] = c                                       # a ring cut by the top edge: open
    img[0:7, 151:159] = 0
    out.append(Case('hole_holds_a_tile', _one(img), lambda x, c=c: (x[0][32:64, 64:128] != c).all() and (ref.stage(c, x[0])[32:64, 64:128] == c).all()))
    return out


# ---- stage 3: size_thresh + ec_band_removal ----------------------------------------------------------------------------------
def _thresh_cases():
    out = []
    img = _canvas(33, 65)
    img[2:4, 2:9] = 3                                          # 14
    img[8:11, 2:7] = 3                                         # 15
    img[16:20, 2:6] = 3                                        # 16
    out.append(Case('ec_14_15_16', _one(img), lambda x: sorted(ref.areas(x[0], 3)) == [14, 15, 16]))

    img = _canvas(48, 96)
    img[28:36, 60:68] = 3
    out.append(Case('ec_on_tile_corner', _one(img), lambda x: (x[0][31:33, 63:65] == 3).all() and ref.stage(3, x[0])[31:33, 63:65].all()))

    for H, W in ((33, 65), (32, 64)):
        img = _canvas(H, W)
        img[0:5, 0:5] = 3                                       # a corner
        img[0:4, 20:26] = 3                                     # each edge
        img[H - 4:H, 30:36] = 3
        img[12:18, 0:4] = 3
        img[12:18, W - 4:W] = 3
        img[H - 5:H, W - 5:W] = 3

        def check(x):
            a, b = x[0], ref.stage(3, x[0])
            # the erosion pads with 1: ec pixels ON the image edge survive, the corner pixel included
            return all((b[s] == 3).any() for s in (np.s_[0, :], np.s_[-1, :], np.s_[:, 0], np.s_[:, -1])) and b[0, 0] == 3 and a[0, 0] == 3
        out.append(Case('ec_on_image_edges_%dx%d' % (H, W), _one(img), check))

    # an ec region whose run on the image edge is narrower than the rows behind it: the edge pixels survive only because the
    # erosion pads with 1 - and where they do not, the last ecDNA dilation of stage 6 grows them back from the row behind, so
    # the final image cannot tell (the masking this module is there for, shown on the border_value = 0 mutant)
    img = _canvas(33, 65)
    img[0, 20:30] = 3
    img[1:5, 18:32] = 3
    img[10:20, 0] = 3
    img[8:22, 1:5] = 3

    def check_masked(x):
        good, bad = ref.stage(3, x[0]), ref.MUTANTS[3]['erosion_border_0'](x[0])
        return (good[0, 21:29] == 3).all() and (good[11:19, 0] == 3).all() and not np.array_equal(good, bad) and \
            np.array_equal(ref.chain(4, 6, good), ref.chain(4, 6, bad))
    out.append(Case('edge_pixels_the_final_dilation_grows_back', _one(img), check_masked))

    img = _canvas(33, 65)
    img[10, 10] = 3
    img[20:24, 20:30] = 2
    out.append(Case('ec_of_one_pixel', _one(img), lambda x: ref.areas(x[0], 3).tolist() == [1]))
    img = img.copy()
    img[2:8, 40:48] = 3                                         # the same beside a large one: the mean is far above 1
    out.append(Case('ec_of_one_pixel_and_a_large_one', _one(img), lambda x: sorted(ref.areas(x[0], 3)) == [1, 48]))

    img = _canvas(33, 65)
    img[5:10, 5:10] = 3
    img[5:10, 11:16] = 3                                        # one empty column between them: both bands hold it
    out.append(Case('ec_bands_overlap', _one(img), lambda x: len(ref.areas(x[0], 3)) == 2 and not x[0][5:10, 10].any()))

    img = _canvas(33, 65)
    img[2:6, 2:6] = 1
    img[10:15, 10:16] = 3
    out.append(Case('no_chromosome', _one(img), lambda x: np.isnan(ref.mean_area(x[0], 2)) and (ref.stage(3, x[0]) == 1).sum() == 16))
    img = _canvas(33, 65)
    img[2:6, 2:6] = 1
    img[10:15, 10:16] = 2
    out.append(Case('no_ec', _one(img), lambda x: np.isnan(ref.mean_area(x[0], 3)) and (ref.stage(3, x[0]) == 2).sum() == 30))

    img = _canvas(33, 65)
    img[2:4, 2:4] = 2                                           # chromosomes of 4 and 8: mean 6
    img[2:4, 8:12] = 2
    img[10:12, 2:5] = 1                                         # nuclei of 6 (kept: strict <), 5 (erased) and 7
    img[10:15, 10] = 1
    img[10:17, 20] = 1
    out.append(Case('nucleus_area_equals_mean_chromosome', _one(img),
                    lambda x: ref.mean_area(x[0], 2) == 6.0 and sorted(ref.areas(x[0], 1)) == [5, 6, 7] and (ref.stage(3, x[0]) == 1).sum() == 13))

    img = _canvas(33, 65)
    img[2:6, 2:6] = 3                                           # ec of 16 and 20: mean 18
    img[2:6, 10:15] = 3
    img[12:15, 2:8] = 2                                         # chromosomes of 18 (stays), 17 (-> ec) and 19
    img[12:15, 12:17] = 2
    img[15, 12:14] = 2
    img[20:23, 2:8] = 2
    img[23, 2] = 2
    out.append(Case('chromosome_area_equals_mean_ec', _one(img),
                    lambda x: ref.mean_area(x[0], 3) == 18.0 and sorted(ref.areas(x[0], 2)) == [17, 18, 19] and (ref.stage(3, x[0]) == 2).sum() == 37))

    img = _canvas(33, 65)
    img[2:7, 2:8] = 3                                           # ec of 30 and 4: mean 17
    img[12:14, 10:12] = 3
    img[12:15, 12:17] = 2                                       # a chromosome of 15 < 17 touching the small ec region
    def check(x):
        a, b = x[0], ref.stage(3, x[0])
        # the small region goes (labelled before the reassignment), the reassigned chromosome stays although it touched it
        return ref.mean_area(a, 3) == 17.0 and ref.areas(a, 2).tolist() == [15] and not b[12:14, 10:12].any() and b[13, 13:16].tolist() == [3, 3, 3]
    out.append(Case('small_chromosome_touches_small_ec', _one(img), check))
    return out


# ---- stage 4: nucleus_in_metaphase -------------------------------------------------------------------------------------------
SIDES = ('left', 'right', 'bottom', 'top')


def _metaphase(H, W, ny, nx, counts, extra=()):
    """A 3 x 3 nucleus centred at (ny, nx) and one-pixel chromosomes: on the nucleus' row for the x bands (their cy == ny counts
    for no y band), on its column for the y bands; ``extra``: further chromosome pixels."""
    img = _canvas(H, W)
    img[ny - 1:ny + 2, nx - 1:nx + 2] = 1
    for side, n in zip(SIDES, counts):
        for i in range(n):
            d = 4 + 2 * i
            y, x = dict(left=(ny, nx + d), right=(ny, nx - d), bottom=(ny - d, nx), top=(ny + d, nx))[side]
            img[y, x] = 2
    for y, x in extra:
        img[y, x] = 2
    return img


def _nucleus_cases():
    out = []
    H, W, ny, nx = 96, 200, 48, 100
    imgs, want = [], []
    for s in range(4):
        for n in (5, 6):
            counts = [7] * 4
            counts[s] = n
            imgs.append(_metaphase(H, W, ny, nx, counts))
            want.append(tuple(counts))
    out.append(Case('five_and_six_on_each_side', np.stack(imgs),
                    lambda x, want=want: [ref.side_counts(a)[0] for a in x] == want and
                    [int(ref.kill_mask(a).any()) for a in x] == [0, 1] * 4))
    # a centroid at exactly nx + 70.0 (and the three other bounds): five inside the band and one ON its end
    for s, (cy0, cx0, ey, ex) in enumerate(((48, 100, 48, 170), (48, 100, 48, 30), (75, 100, 5, 100), (20, 100, 90, 100))):
        counts = [7] * 4
        counts[s] = 5
        img = _metaphase(H, W, cy0, cx0, counts, extra=[(ey, ex)])

        def check(x, s=s, cy0=cy0, cx0=cx0, ey=ey, ex=ex):
            cy, cx = ref.centroids(x[0], 2)
            ny_, nx_ = ref.centroids(x[0], 1)
            on = ((cx == nx_[0] + 70.0).any(), (cx == nx_[0] - 70.0).any(), (cy == ny_[0] - 70.0).any(), (cy == ny_[0] + 70.0).any())[s]
            return bool(on) and ref.side_counts(x[0])[0][s] == 5 and not ref.kill_mask(x[0]).any()
        out.append(Case('centroid_on_the_70_bound_%s' % SIDES[s], _one(img), check))
    # centroids at exactly nx / ny with areas above one: 1 x 3 and 3 x 1 chromosomes centred on the nucleus' column / row, the
    # nucleus 3 x 3: sums divisible by the areas, the float64 quotients exact.  They count for neither side: five stay five.
    img = _metaphase(H, W, ny, nx, (5, 7, 7, 7))
    img[20, nx - 1:nx + 2] = 2
    img[ny - 1:ny + 2, 30] = 2
    out.append(Case('centroid_at_exactly_nx', _one(img),
                    lambda x: (ref.centroids(x[0], 2)[1] == 100.0).sum() >= 15 and (ref.areas(x[0], 2) == 3).sum() == 2 and
                    ref.side_counts(x[0])[0][0] == 5 and not ref.kill_mask(x[0]).any()))
    # a nucleus at the image corner: centroid (0.5, 0.5), six chromosomes down the first column and six along the first row
    for n, name in ((6, 'erased'), (5, 'kept')):
        img = _canvas(33, 65)
        img[0:2, 0:2] = 1
        for i in range(6):
            img[4 + 2 * i, 0] = 2
        for i in range(n):
            img[0, 4 + 2 * i] = 2
        out.append(Case('nucleus_at_the_corner_' + name, _one(img),
                        lambda x, n=n: ref.side_counts(x[0])[0] == (n, 6, n, 6) and bool(ref.kill_mask(x[0]).any()) == (n == 6)))
    # a strip wider than the binned test takes (pair test), and its first 2000 columns (binned test): nuclei on the middle row,
    # chromosomes above and below in stretches of different density, so that some nuclei are erased and some are not
    H, W = PAIR_STRIP
    rng = np.random.default_rng(4242)
    strip = _canvas(H, W)
    for x0 in range(0, W, 200):
        p = float(rng.choice([0.0, 0.02, 0.08, 0.3]))
        if x0 < 400 or x0 >= W - 400:
            p = (0.3, 0.02)[(x0 // 200) % 2]
        xs = np.arange(x0, min(x0 + 200, W), 2)
        for row in (0, 2):
            strip[row, xs[rng.random(len(xs)) < p]] = 2
    strip[1, 10::37] = 1
    strip[1, W - 5:W - 2] = 1

    def check_strip(x):
        k = ref.kill_mask(x[0])
        nuc = x[0] == 1
        return k.any() and (nuc & (k == 0)).any() and k[:, -400:].any() and (nuc & (k == 0))[:, -400:].any()
    out.append(Case('strip_pair_test', _one(strip), lambda x: x.shape[2] > 32768 and check_strip(x)))
    out.append(Case('strip_binned_test', _one(np.ascontiguousarray(strip[:, :BINNED_STRIP[1]])), lambda x: x.shape[2] <= 32768 and check_strip(x)))
    return out


# ---- stages 5 and 6: merge_comp (+ the final dilation) -----------------------------------------------------------------------
def _last_label_has(img, c, want):
    m = 2 if c == 1 else 1
    lab, n = ref.P.label8((img != 0) & (img != m))
    return n >= 1 and bool((img[lab == n] == c).any()) == want


def _merge_cases(c):
    m = 2 if c == 1 else 1
    out = []
    img = _canvas(33, 65)
    for y, x in ((2, 2), (2, 30), (20, 10), (24, 40)):          # four blocks of ec with one pixel of c: all but the last one flood
        img[y:y + 5, x:x + 6] = 3
        img[y + 2, x + 2] = c
    out.append(Case('last_component_holds_c', _one(img),
                    lambda x: _last_label_has(x[0], c, True) and (ref.chain(c + 4, c + 4, x[0])[24:29, 40:46] == 3).any()))
    img = _canvas(33, 65)
    img[12:18, 20:30] = 3
    img[14, 24] = c
    out.append(Case('only_component', _one(img), lambda x: ref.P.label8((x[0] != 0) & (x[0] != m))[1] == 1 and _last_label_has(x[0], c, True)))
    img = _canvas(33, 65)
    img[2:7, 2:8] = 3                                           # without c: stays ec
    img[2:7, 20:26] = 3
    img[4, 22] = c                                              # with c: floods
    img[20:25, 30:36] = 3                                       # the last one, without c
    out.append(Case('component_without_c', _one(img),
                    lambda x: _last_label_has(x[0], c, False) and (ref.stage(c + 4, x[0])[2:7, 2:8] == 3).any() and
                    (ref.stage(c + 4, x[0])[2:7, 20:26] != 3).all()))
    # two-pixel bands of c along each image edge with ec pixels in the edge row / column: reflect keeps the band in the eroded
    # image and the opening turns the ec pixels into c; a constant border erodes the band away
    for H, W in ((33, 65), (32, 64)):
        img = _canvas(H, W)
        img[0:2, 6:W - 6] = c
        img[H - 2:H, 6:W - 6] = c
        img[6:H - 6, 0:2] = c
        img[6:H - 6, W - 2:W] = c
        img[0, 10:W - 10:3] = 3
        img[H - 1, 11:W - 10:3] = 3
        img[8:H - 8:3, 0] = 3
        img[9:H - 8:3, W - 1] = 3
        img[H // 2, 10:W - 10] = c                               # one-pixel lines of c and of ec in the open: the opening leaves them
        img[H // 2 + 3, 10:W - 10] = 3

        def check(x):
            a, b = x[0], ref.stage(c + 4, x[0])
            edge = np.zeros(a.shape, bool)
            edge[0, :] = edge[-1, :] = edge[:, 0] = edge[:, -1] = True
            return ((a == 3) & edge).sum() >= 20 and (b[edge & (a == 3)] == c).all()
        out.append(Case('bands_on_image_edges_%dx%d' % (H, W), _one(img), check))
    # one-pixel lines of ec across fields of c on the rows and columns either side of the tile edges (31 | 32, 63 | 64): opened
    # away; one-pixel lines of c over nothing: left alone
    img = _canvas(66, 132)
    img[20:44, 40:90] = c
    for y in (31, 32):
        img[y, 42:88:2] = 3
    img[22:42:2, 63] = 3
    img[23:42:2, 64] = 3
    img[50, 2:130] = c
    img[2:60, 100] = c
    img[31, 110:130] = 3
    img[2:64, 63][img[2:64, 63] == 0] = 3

    def check_tiles(x):
        a, b = x[0], ref.stage(c + 4, x[0])
        field = np.zeros(a.shape, bool)
        field[21:43, 41:89] = True
        return (a[field] == 3).sum() >= 40 and (b[field] == c).all() and (b[50, 2:130] == c).all()
    out.append(Case('lines_on_tile_edges', _one(img), check_tiles))
    # the lifted class next to everything: a lattice of m through fields of c, ec and nothing
    img = _canvas(40, 80)
    img[:, 0:26] = c
    img[:, 26:52] = 3
    img[10:30, 20:32] = c
    img[::3, :] = m
    img[:, ::5] = m
    img[17:23, 36:44] = 3
    out.append(Case('lifted_class_everywhere', _one(img),
                    lambda x: (x[0] == m).sum() > 1000 and (c == 2 or (ref.stage(5, x[0])[x[0] == m] == m).all())))
    if c == 2:
        # stage 6: single ec pixels on the image corners, the image edges and the four pixels of a tile corner, each with a
        # nucleus pixel on a diagonal (an 8-connected dilation would take it) - for the final dilation
        for H, W in ((66, 132), (66, 131), (33, 65)):
            img = _canvas(H, W)
            pts = [(0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1), (0, W // 2), (H - 1, W // 3), (H // 2, 0), (H // 3, W - 1)]
            if H > 40:
                pts += [(31, 63), (32, 70), (31, 76), (38, 64), (44, 63), (50, 64), (32, 90)]
            for y, x in pts:
                img[y, x] = 3
                for dy, dx in ((-1, -1), (1, 1), (-1, 1), (1, -1)):
                    if 0 <= y + dy < H and 0 <= x + dx < W:
                        img[y + dy, x + dx] = 1

            def check(x, pts=pts):
                a, b = x[0], ref.stage(6, x[0])
                return (a == 3).sum() == len(pts) and (b == 3).sum() > 3 * len(pts) and (b[a == 1] == 1).all()
            out.append(Case('ec_pixels_on_edges_and_corners_%dx%d' % (H, W), _one(img), check))
    return out


HAND = {1: lambda: _fill_cases(1), 2: lambda: _fill_cases(2), 3: _thresh_cases, 4: _nucleus_cases, 5: lambda: _merge_cases(1),
        6: lambda: _merge_cases(2)}


@functools.lru_cache(maxsize=None)
def cases(k):
    out = [Case('extent_%dx%d' % hw, extent_batch(*hw), None) for hw in EXTENTS]
    out += [Case('constant_2x2', np.repeat(np.arange(4, dtype=np.uint8), 4).reshape(4, 2, 2), None)]
    out += [Case('fuzz_%dx%d' % hw, fuzz_batch(*hw), None) for hw in FUZZ_EXTENTS]
    out += HAND[k]()
    for c in out:
        c.x.setflags(write=False)
    return out


def hand_cases(k):
    return [c for c in cases(k) if c.check is not None]
