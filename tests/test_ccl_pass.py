"""Host tests for the tests of one labelling pass: the reference (ccl_pass_ref.py) against a plain flood fill and against the
oracle where they overlap, and the case list (ccl_pass_cases.py) against the tile geometry it was chosen for - asserted from the host
tile model, so that the device tests cannot lose a path without this failing."""
import itertools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ccl_pass_cases as cc          # noqa: E402
import ccl_pass_ref as ref           # noqa: E402

from oracle import postproc          # noqa: E402


def test_entry_point_is_registered_as_an_addition_to_abi_5():
    from ecseg_amd import _lib
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'ecseg_hip.h')).read()
    assert 'still 5 - additive: ecseg_ccl_pass_debug' in hdr and '#define ECSEG_ABI_VERSION 6' in hdr and _lib.ABI_VERSION == 6
    assert 'ecseg_ccl_pass_debug' in _lib.EXPORTS and hasattr(_lib.Handle, 'ccl_pass')
    assert C_sizeof(_lib.CclPassDesc) == 4 * (10 + 5 + 5)          # ecseg_ccl_pass_desc: 20 32-bit words, no padding


def C_sizeof(t):
    import ctypes
    return ctypes.sizeof(t)


# ---- the reference against a brute-force flood fill -------------------------------------------------------------------------
def _flood(img, lut, conn, aux_mode=0, aux_c=0, aux=None):
    """Plain Python: visit the pixels in raster order, flood every unvisited keyed pixel over neighbours of the same key.  ->
    (root per pixel, {root: (key, area, sumy, sumx, flag)})."""
    H, W = img.shape
    table = [(lut >> (8 * k)) & 0xff for k in range(4)]
    key = [[(1 if img[y, x] else 0) if lut == ref.LUT_NONZERO else table[img[y, x] & 3] for x in range(W)] for y in range(H)]
    nb = [(-1, 0), (1, 0), (0, -1), (0, 1)] + ([(-1, -1), (-1, 1), (1, -1), (1, 1)] if conn == 8 else [])
    root = [[-1] * W for _ in range(H)]
    comps = {}
    for y0 in range(H):
        for x0 in range(W):
            if not key[y0][x0] or root[y0][x0] >= 0:
                continue
            r = y0 * W + x0
            root[y0][x0] = r
            todo = [(y0, x0)]
            area = sy = sx = flag = 0
            while todo:
                y, x = todo.pop()
                area, sy, sx = area + 1, sy + y, sx + x
                if aux_mode == ref.AUX_BORDER:
                    flag |= int(y == 0 or y == H - 1 or x == 0 or x == W - 1)
                elif aux_mode == ref.AUX_VALUE_EQ:
                    flag |= int(img[y, x] == aux_c)
                elif aux_mode == ref.AUX_IMAGE:
                    flag |= int(aux[y, x]) & 31
                for dy, dx in nb:
                    v, u = y + dy, x + dx
                    if 0 <= v < H and 0 <= u < W and root[v][u] < 0 and key[v][u] == key[y0][x0]:
                        root[v][u] = r
                        todo.append((v, u))
            comps[r] = (key[y0][x0], area, sy, sx, flag)
    return np.asarray(root, np.int32).reshape(H, W), comps


def _hold_to_flood(img, lut, conn, aux_mode=0, aux_c=0, aux=None):
    lab = ref.Labelling(img, lut, conn)
    root, comps = _flood(img, lut, conn, aux_mode, aux_c, aux)
    assert np.array_equal(lab.root_px, root)
    flags = lab.flags(aux_mode, aux_c, aux)
    assert sorted(comps) == sorted(lab.root.tolist())
    for c in range(lab.n):
        assert comps[int(lab.root[c])] == (int(lab.key[c]), int(lab.area[c]), int(lab.sumy[c]), int(lab.sumx[c]), int(flags[c]))
    for k in (1, 2, 3):
        assert lab.ncomp[k - 1] == sum(1 for v in comps.values() if v[0] == k)
        assert lab.npx[k - 1] == sum(v[1] for v in comps.values() if v[0] == k)
    assert lab.last_root == (max(comps) + 1 if comps else 0)
    assert lab.list1.tolist() == sorted(r for r in comps if img.ravel()[r] == 1)
    assert lab.list2.tolist() == sorted(r for r in comps if img.ravel()[r] == 2)
    for qk, qn in [(0, 1), (1, 0), (2, 0), (0, 0b10100), (3, 2), (0, 32)]:
        assert lab.query(flags, qk, qn) == sum(1 for v in comps.values() if (not qk or v[0] == qk) and (v[4] & qn) == qn)


def test_reference_equals_flood_fill_on_every_3x3_binary_image():
    for bits in itertools.product((0, 7), repeat=9):
        img = np.asarray(bits, np.uint8).reshape(3, 3)
        for conn in (4, 8):
            _hold_to_flood(img, ref.LUT_NONZERO, conn, ref.AUX_BORDER)


@pytest.mark.parametrize('seed', range(6))
def test_reference_equals_flood_fill_on_seeded_images(seed):
    r = np.random.RandomState(seed)
    luts = [ref.LUT_MULTI, ref.LUT_NONZERO, ref.lut_ne(1), ref.lut_ne(2), ref.lut_nonzero_except(1), ref.lut_nonzero_except(2),
            ref.lut_eq(3), 0x03020000]
    for k in range(40):
        H, W = r.randint(1, 10, 2)
        img = np.where(r.random_sample((H, W)) < r.choice([0.3, 0.6, 0.9]), r.randint(1, 4, (H, W)), 0).astype(np.uint8)
        if k % 5 == 0:
            img = r.randint(0, 256, (H, W)).astype(np.uint8)
        aux = r.randint(0, 256, (H, W)).astype(np.uint8)
        for conn in (4, 8):
            _hold_to_flood(img, luts[k % len(luts)], conn, k % 4, 1 + k % 3, aux)


# ---- the reference against the oracle ----------------------------------------------------------------------------------------
def _same_partition(a, b):
    """Two labellings of one image split it the same way."""
    pairs = np.unique(np.stack([a.ravel(), b.ravel()], 1), axis=0)
    return len(np.unique(pairs[:, 0])) == len(pairs) == len(np.unique(pairs[:, 1])) and np.array_equal(a > 0, b > 0)


@pytest.mark.parametrize('name', ['noise30', 'noise55', 'checker', 'rings', 'spiral', 'dirichlet'])
def test_reference_equals_the_oracle_where_they_overlap(name):
    img = cc.PATTERNS[name](70, 131, 5)
    mask = img != 0
    for conn, label in ((8, postproc.label8), (4, postproc.label4)):
        lab = ref.Labelling(cc.as_mask(img), ref.LUT_NONZERO, conn)
        olab, n = label(mask)
        assert n == lab.n and _same_partition(lab.comp, olab)
        # scipy numbers components by their first pixel in raster order: the oracle's label order is the order of the roots
        order = np.argsort(lab.root)
        assert np.array_equal(olab.ravel()[lab.root[order]], np.arange(1, n + 1))
        assert np.array_equal(postproc._areas(olab, n), lab.area[order])
        if n:
            cy, cx = postproc._centroids(olab, n)
            assert np.array_equal(cy, lab.sumy[order].astype(np.float64) / lab.area[order].astype(np.float64))
            assert np.array_equal(cx, lab.sumx[order].astype(np.float64) / lab.area[order].astype(np.float64))
    lab8 = ref.Labelling(cc.as_mask(img), ref.LUT_NONZERO, 8)
    n, px = postproc.count_cc(mask)
    assert n == lab8.ncomp[0] and (px == lab8.npx[0] or (px == 0.0 and (n == 0 or mask.all())))
    for c in (1, 2, 3):                          # one multi-key labelling = the class masks labelled one by one
        multi = ref.Labelling(img, ref.LUT_MULTI, 8)
        assert multi.ncomp[c - 1] == postproc.count_cc(img == c)[0]


# ---- the case list against the geometry it is meant to reach -----------------------------------------------------------------
def _all_images(src):
    for case in cc.cases():
        for i, name in enumerate(case.names):
            yield case, name, getattr(case, src)[i]


def test_case_list_has_the_shapes_batches_and_modes():
    cases = cc.cases()
    assert sorted({c.labels.shape[1:] for c in cases}) == sorted(cc.SHAPES)
    assert sorted(c.labels.shape[0] for c in cases if c.labels.shape[1:] == cc.BATCH_SHAPE) == sorted(cc.BATCHES)
    for c in cases:
        n = c.labels.shape[0]
        assert set(np.unique(c.mask)) <= {0, 4, 8, 252, 1, 255}
        if c.labels.shape[1:] == cc.BATCH_SHAPE:         # a wrong block-to-image decoding cannot hide behind equal images
            for src in (c.labels, c.mask):
                assert len({src[i].tobytes() for i in range(n)}) == n, 'two images of %s are equal' % c.name
        if c.labels.shape[1:] != cc.BATCH_SHAPE:
            assert c.names == list(cc.PATTERNS)          # every pattern at every shape
    assert {n for c in cases if c.labels.shape[1:] == cc.BATCH_SHAPE for n in c.names} == set(cc.PATTERNS)
    # every pass a driver builds is in the list, and the cross on LUT_MULTI is complete
    named = {n for m in cc.DRIVER_MODES for n in m.name.split('__')}
    assert named == set(cc.DRIVER_PASSES)
    assert len({m[2:] for m in cc.CROSS_MODES}) == 2 * 3 * 4 * 2 == len(cc.CROSS_MODES)
    assert len({m.name for m in cc.MODES}) == len(cc.MODES)
    for m in cc.MODES:
        assert all(len(g) <= 5 for g in cc.queries_of(m)) and (not m.count_only or not cc.queries_of(m))


def test_case_list_reaches_every_tile_state_in_both_positions():
    """tile_any 0, 1 and 2, each on a tile the 8-byte pre-passes take (W % 8 == 0, whole tile inside) and on one they do not."""
    fill = [m for m in cc.DRIVER_MODES if m.allow_full]
    assert len(fill) == 2 and all(ref.allow_full_effective(m.conn, m.stat, m.need, m.count_only, m.allow_full) for m in fill)
    assert not any(ref.allow_full_effective(m.conn, m.stat, m.need, m.count_only, m.allow_full) for m in cc.MODES if m not in fill)
    for m in fill:
        seen = set()
        for case, _, img in _all_images(m.src):
            tiles = ref.tile_model(ref.keys_of(img, m.lut), True)
            elig = ref.tile_eligible(*img.shape)
            seen |= {(int(v), bool(e)) for v, e in zip(tiles.ravel(), elig.ravel())}
        assert seen == {(v, e) for v in (0, 1, 2) for e in (False, True)}, (m.name, seen)
    # the sparse passes without full tiles: empty and busy tiles in both positions
    for m in cc.MODES:
        if m.sparse and not m.allow_full:
            seen = set()
            for case, _, img in _all_images(m.src):
                tiles = ref.tile_model(ref.keys_of(img, m.lut), False)
                seen |= {(int(v), bool(e)) for v, e in zip(tiles.ravel(), ref.tile_eligible(*img.shape).ravel())}
            assert seen == {(v, e) for v in (0, 1) for e in (False, True)}, (m.name, seen)


def test_case_list_has_the_runs_owners_spans_and_holes():
    run64 = owners512 = span6 = hole = False
    fill = next(m for m in cc.DRIVER_MODES if m.name == 'fill_holes_1')
    for case, name, img in _all_images('labels'):
        H, W = img.shape
        keys = ref.keys_of(img, ref.LUT_MULTI)
        for tx in range(W // 64):                                 # a run of one key over all 64 lanes of a chunk
            chunk = keys[:, tx * 64:(tx + 1) * 64]
            run64 |= bool(((chunk != 0) & (chunk == chunk[:, :1])).all(axis=1).any())
        if name == 'checker':
            owners512 |= bool((ref.tile_owner_counts(img, ref.LUT_MULTI, 4) >= 512).any())
        if name in ('spiral', 'comb_v31', 'full_1'):
            lab = ref.Labelling(img, ref.LUT_MULTI, 8)
            yy, xx = np.indices((H, W))
            tile = (yy // ref.TILE_H) * 100 + xx // ref.TILE_W
            span6 |= any(len(np.unique(tile[lab.comp == c + 1])) >= 6 for c in range(lab.n))
        if name == 'moat':
            # an enclosed hole of the fill pass that holds a FULL tile: a component without the border bit over a tile_any == 2 tile
            lab = ref.Labelling(img, fill.lut, 4)
            border = lab.flags(ref.AUX_BORDER)
            tiles = ref.tile_model(ref.keys_of(img, fill.lut), True)
            for ty, tx in zip(*np.nonzero(tiles == 2)):
                c = lab.comp[ty * ref.TILE_H, tx * ref.TILE_W]
                hole |= c > 0 and not border[c - 1] & 1
    assert run64 and owners512 and span6 and hole, (run64, owners512, span6, hole)
