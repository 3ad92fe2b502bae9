"""CPU oracle of the min-cut nucleus splitter for the tests and tools (reference src/max_flow_binary_mask.py), written from the
contract of ecseg_min_cut in include/ecseg_hip.h.  Not a test module, and never the product's Python.

The task network is stated once, as a list of unit arcs (``arcs``), and solved twice, independently:
  (a) ``solve_scipy``: the arcs as a sparse capacity matrix (parallel arcs add up) through scipy.sparse.csgraph.maximum_flow,
      then a breadth-first search over the arcs with residual capacity;
  (b) ``solve_paths``: a hand-written augmenting-path solver on the NET flow per ordered node pair, depth-first.
Both return (side, flow): side = 1 on the nodes reachable from the source in the residual network of a maximum flow.  That set
is the same for every maximum flow (the source side of the minimal minimum cut), so every comparison is exact.
``solve_greedy`` pushes along depth-first paths WITHOUT ever cancelling flow: it is wrong on purpose and shows which cases need a
cancelled arc.

``instance_min_cut`` restates binary_seg_to_instance_min_cut (:202-233) on top of a pluggable task solver: scipy.ndimage.label
for the labellings (raster order of the first pixel, as skimage numbers them), a brute-force city-block distance transform,
the eight-neighbour form of the local-maximum test and np.round on the float centroid, as the reference computes it.
"""
import hashlib

import numpy as np
from scipy import ndimage
from scipy.sparse import coo_matrix
from scipy.sparse.csgraph import breadth_first_order, maximum_flow

FOUR = ((1, 0), (0, 1), (-1, 0), (0, -1))
EIGHT = np.ones((3, 3), int)


# ---- the task network ---------------------------------------------------------------------------------------------------------
def arcs(M, s, t, d):
    """get_graph (:59-72) -> list of unit arcs (u, v) over flat pixel indices, parallel arcs repeated."""
    M = np.asarray(M) != 0
    h, w = M.shape
    s, t = (int(s[0]), int(s[1])), (int(t[0]), int(t[1]))
    S, T = s[0] * w + s[1], t[0] * w + t[1]
    out = []
    for y in range(h):
        for x in range(w):
            if not M[y, x] or (y, x) == s or (y, x) == t:
                continue
            p = y * w + x
            if abs(y - s[0]) + abs(x - s[1]) <= d:
                out.append((S, p))
            elif abs(y - t[0]) + abs(x - t[1]) <= d:
                out.append((p, T))
            for dy, dx in FOUR:
                yy, xx = y + dy, x + dx
                if 0 <= yy < h and 0 <= xx < w and M[yy, xx]:
                    out.append((p, yy * w + xx))
    return out


def _check_task(M, s, t, d):
    M = np.asarray(M)
    h, w = M.shape
    assert d >= 1 and tuple(s) != tuple(t)
    for p in (s, t):
        assert 0 <= p[0] < h and 0 <= p[1] < w and M[p[0], p[1]]


def solve_scipy(M, s, t, d):
    _check_task(M, s, t, d)
    h, w = np.asarray(M).shape
    n = h * w
    S, T = int(s[0]) * w + int(s[1]), int(t[0]) * w + int(t[1])
    a = np.asarray(arcs(M, s, t, d), np.int64).reshape(-1, 2)
    side = np.zeros(n, np.uint8)
    side[S] = 1
    if len(a) == 0:
        return side.reshape(h, w), 0
    cap = coo_matrix((np.ones(len(a), np.int32), (a[:, 0], a[:, 1])), shape=(n, n)).tocsr()
    cap.sum_duplicates()
    res = maximum_flow(cap, S, T)
    left = (cap - res.flow).tocsr()                          # residual capacity; the flow matrix is antisymmetric
    left.data = (left.data > 0).astype(np.int8)
    left.eliminate_zeros()
    side[breadth_first_order(left, S, directed=True, return_predecessors=False)] = 1
    assert not side[T]
    return side.reshape(h, w), int(res.flow_value)


def _graph(M, s, t, d):
    cap, nbr = {}, {}
    for u, v in arcs(M, s, t, d):
        cap[(u, v)] = cap.get((u, v), 0) + 1
        nbr.setdefault(u, set()).add(v)
        nbr.setdefault(v, set()).add(u)
    return cap, nbr


def solve_paths(M, s, t, d):
    _check_task(M, s, t, d)
    h, w = np.asarray(M).shape
    S, T = int(s[0]) * w + int(s[1]), int(t[0]) * w + int(t[1])
    cap, nbr = _graph(M, s, t, d)
    net = {}                                                 # net flow u -> v for u < v

    def room(u, v):
        f = net.get((u, v), 0) if u < v else -net.get((v, u), 0)
        return cap.get((u, v), 0) - f

    def search():
        came = {S: None}
        stack = [S]
        while stack:
            u = stack.pop()
            if u == T:
                break
            for v in nbr.get(u, ()):
                if v not in came and room(u, v) > 0:
                    came[v] = u
                    stack.append(v)
        return came

    flow = 0
    while True:
        came = search()
        if T not in came:
            break
        v = T
        while came[v] is not None:
            u = came[v]
            if u < v:
                net[(u, v)] = net.get((u, v), 0) + 1
            else:
                net[(v, u)] = net.get((v, u), 0) - 1
            v = u
        flow += 1
    side = np.zeros(h * w, np.uint8)
    side[list(came)] = 1
    return side.reshape(h, w), flow


def solve_greedy(M, s, t, d):
    """Depth-first augmenting paths over arcs that still have room, never undoing flow -> the flow value it reaches (<= the
    maximum)."""
    h, w = np.asarray(M).shape
    S, T = int(s[0]) * w + int(s[1]), int(t[0]) * w + int(t[1])
    cap, nbr = _graph(M, s, t, d)
    used = {}
    flow = 0
    while True:
        came = {S: None}
        stack = [S]
        while stack and T not in came:
            u = stack.pop()
            for v in sorted(nbr.get(u, ())):
                if v not in came and cap.get((u, v), 0) - used.get((u, v), 0) > 0:
                    came[v] = u
                    stack.append(v)
        if T not in came:
            return flow
        v = T
        while came[v] is not None:
            used[(came[v], v)] = used.get((came[v], v), 0) + 1
            v = came[v]
        flow += 1


# ---- the whole function ----------------------------------------------------------------------------------------------------------
def flow_distance(flow_limit):
    return (-1 + int(np.sqrt(1 + (2 * flow_limit)))) // 2


def l1_distance(mask):
    """City-block distance to the nearest zero pixel of the crop, by brute force; 2^30 without one."""
    on = np.asarray(mask) != 0
    zy, zx = np.nonzero(~on)
    out = np.zeros(on.shape, np.int64)
    if len(zy) == 0:
        out[:] = 1 << 30
        return out
    for y in range(on.shape[0]):
        row = np.abs(zy - y)[None, :] + np.abs(zx[None, :] - np.arange(on.shape[1])[:, None])
        out[y] = row.min(axis=1)
    return out


def centre_pixels(mask, min_rad=10):
    """The padded ``centers`` image of get_centers (:196-199), or None when no pixel qualifies (:193-195)."""
    mask = np.asarray(mask)
    h, w = mask.shape
    if h < 3 or w < 3:
        return None
    d = l1_distance(mask)
    c = d[1:h - 1, 1:w - 1]
    ok = (mask[1:h - 1, 1:w - 1] != 0) & (c > min_rad)
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            if dy or dx:
                ok &= c >= d[1 + dy:h - 1 + dy, 1 + dx:w - 1 + dx]
    if not ok.any():
        return None
    return np.pad(c >= max(c[ok].min(), min_rad), 1)


def centres(mask, rng, min_rad=10):
    """get_centers + binary_img_to_centers (:143-199)."""
    px = centre_pixels(mask, min_rad)
    if px is None:
        return []
    lab, n = ndimage.label(px, structure=EIGHT)
    out = []
    for k in range(1, n + 1):
        ys, xs = np.nonzero(lab == k)
        c = np.round(np.array([ys.mean(), xs.mean()])).astype(int)
        if not mask[c[0], c[1]]:
            alternatives = list(zip(ys.tolist(), xs.tolist()))
            c = alternatives[rng.randint(len(alternatives))]
        out.append((int(c[0]), int(c[1])))
    return out


def segment(mask, centers, dist, solver, min_size=100, depth=0, trace=None):
    """segment_min_cut (:119-140), recursive as in the reference.  ``trace``: a list that receives the depth of every cut."""
    if not centers:
        return []
    if len(centers) == 1:
        return [mask]
    c1, c2 = centers[:2]
    if trace is not None:
        trace.append(depth)
    g1 = solver(mask, c1, c2, dist)[0].astype(mask.dtype)
    g2 = mask - g1
    centers = list(centers)
    if g1.sum() < min_size:
        g1, g2 = np.zeros_like(mask), mask
        centers.remove(c1)
    elif g2.sum() < min_size:
        g1, g2 = mask, np.zeros_like(mask)
        centers.remove(c2)
    first = [c for c in centers if g1[c[0], c[1]]]
    second = [c for c in centers if g2[c[0], c[1]]]
    return segment(g1, first, dist, solver, min_size, depth + 1, trace) + segment(g2, second, dist, solver, min_size, depth + 1, trace)


def colour(label, seed=1):
    """(r, g) of one label (:228)."""
    if not label:
        return 0, 0
    return tuple(int(hashlib.blake2b(str(label).encode(), digest_size=1, salt=('%d_%s' % (seed, c)).encode()).hexdigest(), 16) for c in 'rg')


def visualization(labels, mask, seed=1):
    out = np.zeros(labels.shape + (3,), np.uint8)
    for v in np.unique(labels).tolist():
        r, g = colour(v, seed)
        out[labels == v] = (r, g, min(max(384 - r - g, 0), 255))
    out[..., 2] *= (np.asarray(mask) != 0).astype(np.uint8)
    return out


def instance_min_cut(segmented_cells, flow_limit, coeff, seed=1, solver=solve_scipy, trace=None):
    """binary_seg_to_instance_min_cut (:202-233) -> (labels int64, visualization uint8)."""
    seg = np.asarray(segmented_cells) != 0
    rng = np.random.RandomState(seed)
    lab, n = ndimage.label(seg)                              # 4-connected (:204)
    out = lab.astype(np.int64)
    if n == 0:
        return out, visualization(out, seg, seed)
    areas = np.bincount(lab.reshape(-1))[1:]
    median = np.median(areas)
    dist = flow_distance(flow_limit)
    assert dist > 0
    total = n
    for k, box in enumerate(ndimage.find_objects(lab), start=1):
        if not areas[k - 1] > coeff * median:
            continue
        mask = (lab[box] == k).astype(np.int64)
        cs = centres(mask, rng)
        if len(cs) > 1:
            cells = segment(mask, cs, dist, solver, trace=trace)
            out[box] -= mask * k
            for i, cell in enumerate(cells, start=1):
                if i == 1:
                    out[box] += cell * k
                else:
                    total += 1
                    out[box] += cell * total
    assert total == out.max()
    return out, visualization(out, seg, seed)


class OracleSolverHandle:
    """``ccl_labels`` and ``min_cut`` of a ``_lib.Handle``, computed by this oracle (for the product's host code without a GPU)."""

    def __init__(self, solver=solve_scipy):
        self.solver = solver
        self.batches = []

    def ccl_labels(self, mask, connectivity=8):
        m = np.asarray(mask) != 0
        lab = ndimage.label(m, structure=EIGHT if connectivity == 8 else None)[0]
        first = np.zeros(lab.max() + 1, np.int64)            # 1 + raster index of the first pixel, as the device numbers them
        flat = lab.reshape(-1)
        idx = np.flatnonzero(flat)
        first[flat[idx[::-1]]] = idx[::-1] + 1
        return first[lab].astype(np.int32)

    def min_cut(self, tasks, dist):
        self.batches.append(len(tasks))
        got = [self.solver(np.asarray(m), s, t, dist) for m, s, t in tasks]
        return [g[0] for g in got], np.array([g[1] for g in got], np.int32)
