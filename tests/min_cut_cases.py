"""Case generators of the min-cut tests and tools: hand tasks with their hand-computed answers, seeded random tasks, and scenes of
nuclei with clumps for the whole function.  A task is (M, s, t, d): window, source pixel, sink pixel, distance."""
import numpy as np


def _rows(*rows):
    return np.array([[int(c) for c in r.replace(' ', '')] for r in rows], np.uint8)


def dumbbell(side=29, neck=3, length=7):
    """Two side x side squares joined by a neck-wide corridor in the middle rows -> (M, centre of the left, centre of the right)."""
    M = np.zeros((side, 2 * side + length), np.uint8)
    M[:, :side] = 1
    M[:, side + length:] = 1
    r0 = side // 2 - neck // 2
    M[r0:r0 + neck, side:side + length] = 1
    return M, (side // 2, side // 2), (side // 2, side + length + side // 2)


# A window on which depth-first augmenting paths that never cancel flow (min_cut_ref.solve_greedy) stop at 3 of the 4 units: the first
# path winds through the pixels the others need.  Found by search with that solver; kept literally so that it cannot drift.
CANCEL = (_rows('111111',
                '111111',
                '111110',
                '111110'), (2, 2), (0, 4), 1)


def hand_tasks():
    """name -> ((M, s, t, d), flow, side or None).  side None: only the flow is known by hand, the oracle decides the side."""
    out = {}
    M = _rows('11')
    out['adjacent_1x2'] = ((M, (0, 0), (0, 1), 1), 0, _rows('10'))
    M = np.ones((1, 9), np.uint8)
    out['corridor_d1'] = ((M, (0, 0), (0, 8), 1), 1, _rows('100000000'))
    M, left, right = dumbbell()
    want = np.zeros_like(M); want[:, :29] = 1
    out['dumbbell_from_the_left'] = ((M, left, right, 5), 3, want)
    want = np.zeros_like(M); want[:, 29 + 7:] = 1
    out['dumbbell_from_the_right'] = ((M, right, left, 5), 3, want)
    # pixel 2 lies in both balls and counts for the source alone: were it joined to the sink as well the flow would be 2
    out['both_balls'] = ((np.ones((1, 5), np.uint8), (0, 0), (0, 4), 2), 1, _rows('11100'))
    # (1, 2) is next to the sink and in its ball: two parallel arcs carry the two units that arrive over the upper and the lower row
    M = _rows('1110',
              '1011',
              '1110')
    out['capacity_two_into_the_sink'] = ((M, (1, 0), (1, 3), 1), 2, _rows('0000', '1000', '0000'))
    # the last pixel of row 1 and the first of row 2 are set, the bars share no column: no arc joins them
    M = np.zeros((5, 13), np.uint8)
    M[1, 5:] = 1
    M[2, :5] = 1
    want = np.zeros_like(M); want[1, 5:] = 1
    out['row_wrap_trap'] = ((M, (1, 8), (2, 2), 2), 0, want)
    # a piece of the mask that hangs on nothing
    M, left, right = dumbbell(9, 1, 3)
    M = np.pad(M, ((0, 4), (0, 0)))
    M[11:, 2:6] = 1
    want = np.zeros_like(M); want[:9, :9] = 1
    out['disconnected_piece'] = ((M, left, right, 2), 1, want)
    out['needs_a_cancelled_arc'] = (CANCEL, None, None)
    return out


def blob(rng, h, w, kind):
    yy, xx = np.mgrid[:h, :w]
    M = np.zeros((h, w), bool)
    if kind == 0:                                            # overlapping discs
        for _ in range(int(rng.integers(2, 5))):
            r = rng.uniform(0.15, 0.4) * min(h, w)
            cy, cx = rng.uniform(r / 2, h - r / 2), rng.uniform(r / 2, w - r / 2)
            M |= (yy - cy) ** 2 + (xx - cx) ** 2 <= r * r
    elif kind == 1:                                          # dense noise: many short detours, flows that need cancelling
        M = rng.random((h, w)) < rng.uniform(0.6, 0.9)
    else:                                                    # a full window with holes
        M[:] = True
        for _ in range(int(rng.integers(1, 8))):
            y, x = int(rng.integers(0, h)), int(rng.integers(0, w))
            M[y:y + int(rng.integers(1, 6)), x:x + int(rng.integers(1, 6))] = False
    return M.astype(np.uint8)


def random_task(seed, max_side=96):
    """A seeded task on a window of at most max_side x max_side pixels; source and sink are two pixels of the largest 4-connected piece
    most of the time (so that there is a flow), any two pixels otherwise."""
    from scipy import ndimage
    rng = np.random.default_rng(seed * 7919 + 17)
    while True:
        h, w = int(rng.integers(3, max_side + 1)), int(rng.integers(3, max_side + 1))
        M = blob(rng, h, w, int(rng.integers(0, 3)))
        lab, n = ndimage.label(M)
        if n == 0:
            continue
        big = 1 + int(np.argmax(np.bincount(lab.reshape(-1))[1:]))
        pool = np.argwhere(lab == big) if rng.random() < 0.85 else np.argwhere(M)
        if len(pool) < 2:
            continue
        i, j = rng.choice(len(pool), 2, replace=False)
        d = int(rng.choice([1, 1, 2, 3, 5, 5, 8, 32]))
        return M, (int(pool[i][0]), int(pool[i][1])), (int(pool[j][0]), int(pool[j][1])), d


def disc_scene(shape, discs):
    M = np.zeros(shape, np.uint8)
    yy, xx = np.mgrid[:shape[0], :shape[1]]
    for cy, cx, r in discs:
        M[(yy - cy) ** 2 + (xx - cx) ** 2 <= r * r] = 255
    return M


# 160 x 224: five single discs, a clump of two and a clump of three overlapping discs (radii >= 13).  The radii and offsets were chosen
# with the CPU oracle so that both clumps split and the clump of three is cut twice, the second cut inside one side of the first.
SCENE_DISCS = [(20, 22, 14), (22, 70, 15), (20, 120, 14), (24, 180, 16), (70, 24, 15),
               (75, 90, 17), (75, 118, 17),
               (125, 60, 18), (125, 90, 18), (125, 120, 18)]


def scene():
    return disc_scene((160, 224), SCENE_DISCS)


def big_scene(seed=0, shape=(1040, 1392), n=300, clump=0.1):
    """About n nuclei of radius 17 - 21 on a jittered grid, about ``clump`` of them replaced by two overlapping discs of radius 17 - 18
    whose centres lie 28 apart along a row or a column: large enough against the median to be examined, with a neck that the
    centre search separates (under the city-block distance it does so for axis-parallel pairs; oblique pairs keep one centre)."""
    rng = np.random.default_rng(seed)
    cols = int(np.ceil(np.sqrt(n * shape[1] / shape[0])))
    rows = int(np.ceil(n / cols))
    discs = []
    for k in range(n):
        cy = (k // cols + 0.5) * shape[0] / rows + rng.uniform(-2, 2)
        cx = (k % cols + 0.5) * shape[1] / cols + rng.uniform(-2, 2)
        if rng.random() < clump:
            r = rng.uniform(17, 18)
            a = float(rng.integers(0, 2)) * np.pi / 2
            discs.append((cy + 14 * np.sin(a), cx + 14 * np.cos(a), r))
            discs.append((cy - 14 * np.sin(a), cx - 14 * np.cos(a), r))
        else:
            discs.append((cy, cx, rng.uniform(17, 21)))
    return disc_scene(shape, discs)
