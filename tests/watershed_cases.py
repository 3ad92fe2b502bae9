"""Cases of NuSeT's marker watershed and clean-up, shared by tools/make_golden_watershed.py (which runs the reference's own
``_watershed`` / ``clean_image`` on them), tests/test_watershed.py (restatement == golden) and tests/test_gpu_watershed.py (device
== restatement).  Plain numpy only: the golden tool imports this file under an old interpreter.

A case is a dict: name, mask (uint8 0 / 1, H x W), scores (float32 n), proposals (float32 n x 4 as x1, y1, x2, y2), min_score and
sizes (the NUCLEI_SIZE_T values of the final threshold).  The 20-pixel edge mask admits a proposal marker only at rows
20 .. H - 21 and columns 20 .. W - 21, so extents are above 40 wherever a proposal matters.  No case makes the reference raise."""
import numpy as np


def disc(m, cy, cx, r, v=1):
    yy, xx = np.ogrid[:m.shape[0], :m.shape[1]]
    m[(yy - cy) ** 2 + (xx - cx) ** 2 <= r * r] = v


def box(row, col, half=5.0):
    """A proposal whose centre is (row, col)."""
    return [col - half, row - half, col + half, row + half]


def _case(name, mask, centres=(), scores=None, min_score=0.9, sizes=(0, 20), proposals=None):
    if proposals is None:
        proposals = [box(r, c) for r, c in centres]
    proposals = np.asarray(proposals, np.float32).reshape(-1, 4)
    if scores is None:
        scores = 0.99 - 0.001 * np.arange(len(proposals))          # descending, as the proposal layer returns them
    return dict(name=name, mask=np.ascontiguousarray(mask, np.uint8), scores=np.asarray(scores, np.float32).reshape(-1),
                proposals=proposals, min_score=float(min_score), sizes=tuple(int(s) for s in sizes))


def fixed_cases():
    out = []
    Z = lambda h=48, w=64: np.zeros((h, w), np.uint8)

    m = Z(); disc(m, 24, 25, 9); disc(m, 24, 39, 9)
    out.append(_case('two_discs', m, [(24, 25), (24, 39)]))
    out.append(_case('two_discs_swapped', m, [(24, 39), (24, 25)]))
    out.append(_case('two_discs_unequal', m, [(23, 24), (26, 41)]))
    m = Z(); m[12:36, 12:52] = 1
    out.append(_case('rectangle_plateau', m, [(24, 22), (24, 42)]))
    out.append(_case('rectangle_three_markers', m, [(22, 22), (27, 32), (23, 43)]))
    m = Z(); disc(m, 24, 32, 13); disc(m, 24, 32, 6, 0)
    out.append(_case('ring_with_hole', m, [(24, 21), (24, 43)]))
    m = Z(); disc(m, 24, 32, 13); disc(m, 24, 32, 8, 0); disc(m, 24, 32, 3)
    out.append(_case('ring_with_core', m, [(24, 21), (24, 32)]))
    m = Z(); m[5:8, 5:8] = 1; m[30:34, 8:12] = 1; disc(m, 24, 40, 6)
    out.append(_case('small_component_no_marker', m, [(24, 40)]))
    m = Z(); m[18:30, 32:50] = 1
    out.append(_case('marker_on_background', m, [(24, 30), (24, 44)]))
    m = Z(); disc(m, 24, 32, 10)
    out.append(_case('two_proposals_one_pixel', m, proposals=[box(24.2, 28.3), box(23.8, 27.9), box(24, 38)]))
    out.append(_case('half_centres', m, proposals=[[22.0, 19.0, 33.0, 30.0], [32.0, 20.0, 41.0, 31.0]]))   # (24.5, 27.5) -> (24, 28); (25.5, 36.5) -> (26, 36)
    m = Z(); disc(m, 10, 10, 7); disc(m, 36, 52, 8); disc(m, 24, 32, 5)
    out.append(_case('proposals_in_the_edge_only', m, [(10, 10), (36, 52), (19, 32), (24, 44)]))
    out.append(_case('scores_empty', m, []))
    out.append(_case('scores_all_low', m, [(24, 32), (10, 10)], scores=[0.9, 0.5], min_score=0.9))
    out.append(_case('one_score_above', m, [(24, 32), (22, 30)], scores=[0.95, 0.9], min_score=0.9))
    m = Z(); m[0:9, 20:40] = 1; m[40:48, 10:30] = 1; m[15:35, 0:7] = 1; m[10:30, 58:64] = 1; disc(m, 24, 30, 6); m[0:4, 0:4] = 1; m[44:48, 60:64] = 1
    out.append(_case('touching_all_borders', m, [(24, 30)]))
    m = Z(); m[14:24, 20:30] = 1; m[24:34, 30:40] = 1
    out.append(_case('diagonal_blobs', m, [(4, 4)]))                # one proposal in the edge: only the region marker remains
    out.append(_case('diagonal_blobs_two_markers', m, [(20, 25), (27, 34)]))
    m = Z(); m[20:28, 20:44] = 1; m[23:25, 30:34] = 0
    out.append(_case('bar_with_notch_hole', m, [(24, 23), (24, 40)]))
    out.append(_case('whole_image_160', np.ones((160, 160), np.uint8), [(50, 60), (110, 95), (80, 130)], sizes=(0, 160 * 160, 160 * 160 + 1)))
    m = np.ones((160, 160), np.uint8); m[0, 0] = 0; m[70:80, 70:80] = 0
    out.append(_case('nearly_whole_image_160', m, [(40, 40), (120, 100)]))

    rng = np.random.default_rng(11)
    m = np.zeros((64, 96), np.uint8)
    cells = [(r, c) for r in range(1, 62, 3) for c in range(1, 94, 3)]
    for k in rng.permutation(len(cells))[:300]:
        r, c = cells[k]
        m[r, c] = 1
        if rng.random() < 0.4: m[r, c + 1] = 1
        if rng.random() < 0.3: m[r + 1, c] = 1
    out.append(_case('three_hundred_specks', m, [(int(r), int(c)) for r, c in zip(rng.integers(20, 44, 40), rng.integers(20, 76, 40))]))

    # clean_image and the final threshold: no proposal, the watershed hands the mask through
    m = Z(); m[8:28, 8:30] = 1; m[12:14, 12:14] = 0; m[30:42, 34:56] = 1; m[32:40, 37:52] = 0
    m[4:6, 50:52] = 1; m[20:40, 0:8] = 1; m[28:30, 0:2] = 0
    out.append(_case('clean_holes_pocket_speck', m, [], sizes=(0, 4, 5, 440, 441)))
    out.append(_case('clean_all_zero', Z(), [], sizes=(0, 5)))
    out.append(_case('clean_all_ones', np.ones((48, 64), np.uint8), [], sizes=(0, 5)))
    m = Z(); m[10:20, 10:20] = 1; m[30:33, 40:47] = 1; m[40, 5] = 1
    out.append(_case('size_threshold_at_area', m, [], sizes=(0, 21, 22, 100, 101)))
    m = Z(); m[1:47, 1:63] = 1
    out.append(_case('clean_border_ring_background', m, [], sizes=(0,)))
    m = Z(); m[10:12, 10:12] = 1; m[12:14, 12:14] = 1; m[30:40, 30:50] = 1
    out.append(_case('clean_diagonal_object', m, [], sizes=(0, 5, 8, 9)))
    return out


def random_case(seed, max_extent=128):
    """A seeded scene: discs, some with holes, speckle, and proposals near the disc centres (some on half pixels, some in the edge,
    some duplicated).  Every centre stays inside the image, so the reference does not raise."""
    rng = np.random.default_rng(1000 + seed)
    H, W = (int(v) for v in rng.integers(41, max_extent + 1, 2))
    m = np.zeros((H, W), np.uint8)
    props, n = [], int(rng.integers(1, 10))
    for _ in range(n):
        cy, cx, r = int(rng.integers(0, H)), int(rng.integers(0, W)), int(rng.integers(2, 14))
        disc(m, cy, cx, r)
        if rng.random() < 0.25:
            disc(m, cy + int(rng.integers(-2, 3)), cx + int(rng.integers(-2, 3)), max(1, r // 3), 0)
        for _ in range(int(rng.integers(0, 3))):
            py = np.clip(cy + rng.integers(-r, r + 1) + 0.5 * rng.integers(0, 2), 0, H - 1)
            px = np.clip(cx + rng.integers(-r, r + 1) + 0.5 * rng.integers(0, 2), 0, W - 1)
            hy, hx = rng.integers(2, 12, 2) + 0.25 * rng.integers(0, 4, 2)
            b = [px - hx, py - hy, px + hx, py + hy]
            props.append(b)
            if rng.random() < 0.1:
                props.append(b)
    if rng.random() < 0.5:
        m[rng.random((H, W)) < 0.01] ^= 1
    if rng.random() < 0.2:
        m[:, :] = 1 - m
    props = np.asarray(props, np.float32).reshape(-1, 4)
    cy, cx = (props[:, 1] + props[:, 3]) / 2, (props[:, 0] + props[:, 2]) / 2
    ok = (np.rint(cy) <= H - 1) & (np.rint(cx) <= W - 1) & (np.rint(cy) >= 0) & (np.rint(cx) >= 0)
    props = props[ok]
    scores = np.sort(rng.random(len(props)).astype(np.float32) * np.float32(0.5) + np.float32(0.5))[::-1]
    area = int(m.sum())
    return _case('random_%d' % seed, m, scores=scores, proposals=props, min_score=0.7, sizes=(0, int(rng.integers(1, 60)), max(1, area // 4)))


SEEDS = range(40)
REGRESSION_SEEDS = (100332, 100697, 100938)              # seeds on which a campaign found a difference: marker pixels of equal d^2 decide


def all_cases():
    return fixed_cases() + [random_case(s) for s in list(SEEDS) + list(REGRESSION_SEEDS)]
