"""Cases of ecseg_min_cut_regions and their expected outputs, computed from tests/min_cut_ref.py alone (``l1_distance``,
``centre_pixels``, scipy's labellings).  Not a test module.  A case is (mask, coeff, min_rad); ``expected`` gives everything the entry
point returns.  Hand cases are named for the branch they take; tests/test_min_cut_regions.py checks that they take it."""
import functools

import numpy as np
from scipy import ndimage

import min_cut_cases as cases
import min_cut_ref as ref


def expected(mask, coeff, min_rad):
    """-> dict(labels (H, W) int32, n_cells, regions (n, 8), centers (m, 8), windows [uint8 (h, w)], comp [int32 (h, w)]) as
    include/ecseg_hip.h states them."""
    lab, n = ndimage.label(np.asarray(mask) != 0)            # 4-connected, raster order of first pixels
    out = dict(labels=lab.astype(np.int32), n_cells=n, regions=[], centers=[], windows=[], comp=[])
    if n:
        areas = np.bincount(lab.reshape(-1), minlength=n + 1)[1:]
        median = np.median(areas)
        off = 0
        for k, box in enumerate(ndimage.find_objects(lab), start=1):
            if not areas[k - 1] > coeff * median:
                continue
            win = (lab[box] == k).astype(np.uint8)
            h, w = win.shape
            px = ref.centre_pixels(win, min_rad)
            comp, count = (ndimage.label(px, structure=ref.EIGHT) if px is not None else (np.zeros((h, w), np.int32), 0))
            first = len(out['centers'])
            for j in range(1, count + 1):
                ys, xs = np.nonzero(comp == j)
                c = np.round(np.array([ys.mean(), xs.mean()])).astype(int)
                out['centers'].append([len(out['regions']), int(c[0]), int(c[1]), int(win[c[0], c[1]] != 0), len(ys), int(ys[0]) * w + int(xs[0]), 0, 0])
            out['regions'].append([k, box[0].start, box[1].start, h, w, off, first, count])
            out['windows'].append(win)
            out['comp'].append(comp.astype(np.int32))
            off += h * w
    out['regions'] = np.array(out['regions'], np.int32).reshape(-1, 8)
    out['centers'] = np.array(out['centers'], np.int32).reshape(-1, 8)
    return out


def _place(shape, *parts):
    M = np.zeros(shape, np.uint8)
    for (r, c), part in parts:
        part = np.asarray(part, np.uint8)
        M[r:r + part.shape[0], c:c + part.shape[1]] |= part
    return M


def _ones(h, w):
    return np.ones((h, w), np.uint8)


def framed(h, w, top=1, left=1):
    """An h x w rectangle with one nub per corner - ``top`` pixels above its top left corner, ``left`` pixels left of its bottom left
    corner, one pixel below its bottom right and one right of its top right corner: its bounding box has zero pixels on every side,
    so the crop has a distance transform, every edge pixel still touches a zero pixel, and the rectangle starts at (top, left)."""
    return with_nubs(np.ones((h, w), np.uint8), top, left)


def with_nubs(shape, top=1, left=1):
    """``shape`` (its four corner pixels set) with the nubs of ``framed``."""
    h, w = shape.shape
    M = np.zeros((h + top + 1, w + left + 1), np.uint8)
    M[top:top + h, left:left + w] = shape
    M[:top, left] = 1
    M[top + h - 1, :left] = 1
    M[top + h, left + w - 1] = 1
    M[top, left + w] = 1
    return M


def ring(outer=10, inner=5):
    yy, xx = np.mgrid[-outer:outer + 1, -outer:outer + 1]
    r2 = yy * yy + xx * xx
    return ((r2 <= outer * outer) & (r2 >= inner * inner)).astype(np.uint8)


def lattice(side=70, step=4):
    M = np.ones((side, side), np.uint8)
    M[::step, ::step] = 0
    M[0, :] = M[-1, :] = M[:, 0] = M[:, -1] = 1              # the holes stay inside: the region is one 4-connected piece
    return M


SMALL = [((0, 0), _ones(2, 2)), ((0, 4), _ones(2, 2))]       # two regions of area 4 in the top rows: they set the median


def hand_cases():
    """name -> (mask, coeff, min_rad)."""
    out = {}
    out['fills_its_box'] = (_place((20, 30), *SMALL, ((4, 3), _ones(12, 12))), 1.25, 1)
    out['box_with_h_below_3'] = (_place((8, 30), *SMALL, ((4, 2), _ones(2, 20))), 1.25, 1)
    out['box_with_w_below_3'] = (_place((30, 12), *SMALL, ((4, 2), _ones(20, 2))), 1.25, 1)
    cross = _ones(17, 17)
    cross[:4, :4] = cross[:4, -4:] = cross[-4:, :4] = cross[-4:, -4:] = 0
    out['meets_all_four_borders'] = (cross, 0.5, 1)
    out['diagonal_touch'] = (_place((22, 22), ((0, 18), _ones(2, 2)), ((0, 12), _ones(2, 2)), ((3, 1), _ones(8, 8)), ((11, 9), _ones(8, 8))), 1.25, 1)
    ell = _ones(16, 16)
    ell[:8, 8:] = 0
    small_l = np.zeros((4, 3), np.uint8)
    small_l[:, 0] = small_l[3, :] = 1
    out['l_shaped_neighbour_in_the_box'] = (_place((22, 24), ((0, 0), _ones(1, 6)), ((0, 8), _ones(1, 6)), ((3, 2), ell), ((4, 14), small_l)), 1.25, 1)
    five = _ones(2, 3); five[1, 2] = 0
    out['areas_4_4_5_nothing_selected'] = (_place((6, 16), *SMALL, ((3, 8), five)), 1.25, 1)
    out['areas_4_4_6_one_selected'] = (_place((6, 16), *SMALL, ((3, 8), _ones(2, 3))), 1.25, 1)
    out['even_n_median_is_a_mean'] = (_place((10, 16), *SMALL, ((3, 8), _ones(2, 3)), ((6, 0), _ones(2, 5))), 1.25, 1)
    out['n_1_not_selected'] = (_place((8, 8), ((1, 1), _ones(6, 6))), 1.25, 1)
    out['n_1_selected'] = (_place((8, 8), ((1, 1), _ones(6, 6))), 0.5, 1)
    out['empty_mask'] = (np.zeros((7, 9), np.uint8), 1.25, 1)
    out['dumbbell_min_rad_10'] = (_place((33, 69), ((1, 1), with_nubs(cases.dumbbell()[0]))), 0.5, 10)
    out['bar_9x15_plateau_ridge'] = (_place((13, 19), ((1, 1), framed(9, 15))), 0.5, 1)
    out['two_pixel_component_rounds_up'] = (_place((10, 9), ((1, 1), framed(6, 5, top=1))), 0.5, 1)      # rows 3, 4: 3.5 -> 4
    out['two_pixel_component_rounds_down'] = (_place((11, 9), ((1, 1), framed(6, 5, top=2))), 0.5, 1)    # rows 4, 5: 4.5 -> 4
    out['2x2_component_half_on_both_axes'] = (_place((10, 11), ((1, 1), framed(6, 6, top=1, left=2))), 0.5, 1)   # rows 3.5 -> 4, columns 4.5 -> 4
    out['ring_centroid_in_the_hole'] = (_place((23, 23), ((1, 1), ring())), 0.5, 1)
    out['two_rings_two_draws'] = (_place((23, 46), ((1, 1), ring()), ((1, 24), ring())), 0.5, 1)
    out['more_than_255_components'] = (_place((72, 72), ((1, 1), lattice())), 0.5, 1)
    return out


SEEDS = range(1000, 1200)                                   # 200 scenes; tests/test_min_cut_regions.py holds the mix they must give


def seeded_case(seed):
    """A scene of at most 96 x 96 - one to four tiles, two zero pixels apart, each a ``cases.blob`` of its own kind - with min_rad in
    {1, 2, 3, 10} and coeff in {0.5, 1.25}."""
    rng = np.random.default_rng(seed * 104729 + 5)
    h, w = int(rng.integers(8, 97)), int(rng.integers(8, 97))
    mask = np.zeros((h, w), np.uint8)
    ny, nx = (int(rng.integers(1, 3)) if h >= 24 else 1), (int(rng.integers(1, 3)) if w >= 24 else 1)
    for i in range(ny):
        for j in range(nx):
            y0, y1, x0, x1 = i * h // ny, (i + 1) * h // ny - 2 * (i + 1 < ny), j * w // nx, (j + 1) * w // nx - 2 * (j + 1 < nx)
            mask[y0:y1, x0:x1] = cases.blob(rng, y1 - y0, x1 - x0, int(rng.integers(0, 3)))
    return mask, float(rng.choice([0.5, 1.25])), int(rng.choice([1, 2, 3, 10]))


def ring_scene(outer=32, inner=8, r=16):
    """70 x 200: two regions, each a ring of thickness 24 with a disc hanging on it by a narrow neck.  At min_rad 10 each has two centre
    components - the ring's, whose centroid falls in the hole (a seeded draw), and the disc's - so both are cut, after two draws."""
    M = np.zeros((2 * outer + 6, 2 * (2 * outer + 2 * r + 4)), np.uint8)
    yy, xx = np.mgrid[:M.shape[0], :M.shape[1]]
    for x0 in (0, M.shape[1] // 2):
        cy, cx = outer + 3, x0 + outer + 3
        d2 = (yy - cy) ** 2 + (xx - cx) ** 2
        M[(d2 <= outer * outer) & (d2 >= inner * inner)] = 255
        M[(yy - cy) ** 2 + (xx - (cx + outer + r - 2)) ** 2 <= r * r] = 255
    return M


def big_region():
    """One 300 x 300 region (a square with a few holes, so that its crop has a distance transform): 90 000 pixels, above the LDS
    threshold by itself."""
    M = np.ones((300, 300), np.uint8)
    for y, x in ((40, 50), (150, 150), (151, 150), (220, 90), (260, 270), (30, 250)):
        M[y, x] = 0
    return M, 0.5, 10


@functools.lru_cache(maxsize=None)
def _expected_of(kind, key):
    mask, coeff, min_rad = hand_cases()[key] if kind == 'hand' else seeded_case(key) if kind == 'seed' else big_region()
    return expected(mask, coeff, min_rad)


def expected_of(kind, key=None):
    """The expected outputs of a hand case ('hand', name), a seeded case ('seed', seed) or the big region ('big'), computed once
    per process and shared by the tests: treat them as read-only."""
    return _expected_of(kind, key)
