"""Reference of ONE connected-component labelling pass of csrc/ccl_kernels.hip (what ``Handle.ccl_pass`` exports), in numpy and
``scipy.ndimage.label`` alone: the key of a pixel, the components of every key, their root (first pixel in raster order), area,
coordinate sums and flag word, the per-image counters, the two root lists, the answers to the flag queries, and a host model of the
64 x 32 labelling tiles (``tile_any``).  Nothing here knows how the device gets there."""
import numpy as np
from scipy import ndimage as ndi

LUT_MULTI = 0x03020100      # key = value & 3
LUT_NONZERO = 0xffffffff    # key = (value != 0)
AUX_NONE, AUX_BORDER, AUX_VALUE_EQ, AUX_IMAGE = 0, 1, 2, 3
STAT_AREA, STAT_SUMS = 1, 2
NEED_NCOMP, NEED_NPX, NEED_LAST, NEED_LISTS = 1, 2, 4, 8
TILE_H, TILE_W = 32, 64

_FULL = np.ones((3, 3), int)
_CROSS = ndi.generate_binary_structure(2, 1)


def lut_eq(c):
    return 1 << (8 * c)


def lut_ne(c):
    return 0x01010101 & ~(0xff << (8 * c))


def lut_nonzero_except(m):
    return 0x01010100 & ~(0xff << (8 * m))


def lut_keys(lut):
    """The non-zero keys a LUT can give."""
    return [1] if lut == LUT_NONZERO else sorted({(lut >> (8 * k)) & 0xff for k in range(4)} - {0})


def keys_of(img, lut):
    """key_of per pixel: LUT_NONZERO -> value != 0, anything else -> byte (value & 3) of the LUT."""
    img = np.asarray(img, np.uint8)
    if lut == LUT_NONZERO:
        return (img != 0).astype(np.uint8)
    table = np.array([(lut >> (8 * k)) & 0xff for k in range(4)], np.uint8)
    return table[img & 3]


def components(img, lut, conn):
    """(H, W) uint8 -> (comp, key_of_comp): comp int64 (H, W), 0 where the key is 0, else 1 .. n; every key value is labelled on its
    own with the 4- or the 8-structure.  key_of_comp[c - 1] is component c's key."""
    assert conn in (4, 8)
    keys = keys_of(img, lut)
    comp = np.zeros(keys.shape, np.int64)
    key_of_comp = []
    for k in lut_keys(lut):
        lab, n = ndi.label(keys == k, structure=_FULL if conn == 8 else _CROSS)
        comp[lab > 0] = lab[lab > 0] + len(key_of_comp)
        key_of_comp += [k] * n
    return comp, np.asarray(key_of_comp, np.int64)


def pixel_bits(img, aux_mode, aux_c=0, aux=None):
    """The bits a keyed pixel ORs into its component's flag word."""
    img = np.asarray(img, np.uint8)
    H, W = img.shape
    if aux_mode == AUX_BORDER:
        b = np.zeros((H, W), bool)
        b[0, :] = b[H - 1, :] = True
        b[:, 0] = b[:, W - 1] = True
        return b.astype(np.uint32)
    if aux_mode == AUX_VALUE_EQ:
        return (img == aux_c).astype(np.uint32)
    if aux_mode == AUX_IMAGE:
        return (np.asarray(aux, np.uint8) & 31).astype(np.uint32)
    return np.zeros((H, W), np.uint32)


class Labelling:
    """The components of one image under (lut, conn) and what does not depend on the aux mode."""

    def __init__(self, img, lut, conn):
        self.img = np.asarray(img, np.uint8)
        self.lut, self.conn = lut, conn
        H, W = self.img.shape
        assert H * W * max(H, W) < 2 ** 53          # the float64 bincounts below are exact integer sums
        self.comp, self.key = components(self.img, lut, conn)
        n = self.n = len(self.key)
        flat = self.comp.ravel()
        # the root is the component's minimum raster index = its first occurrence in the raveled image
        ids, first = np.unique(flat, return_index=True)
        self.root = first[ids > 0].astype(np.int64)                          # [c - 1]
        assert len(self.root) == n
        yy, xx = np.indices((H, W))
        self.area = np.bincount(flat, minlength=n + 1)[1:].astype(np.int64)
        self.sumy = np.bincount(flat, weights=yy.ravel(), minlength=n + 1)[1:].astype(np.int64)
        self.sumx = np.bincount(flat, weights=xx.ravel(), minlength=n + 1)[1:].astype(np.int64)
        assert int(self.sumy.sum()) == int(yy[self.comp > 0].sum()) and int(self.sumx.sum()) == int(xx[self.comp > 0].sum())
        # per pixel: the root of its component, -1 where the key is 0
        self.root_px = np.concatenate([[-1], self.root])[self.comp].astype(np.int32)
        self.ncomp = np.array([np.count_nonzero(self.key == k) for k in (1, 2, 3)], np.int64)
        keys = keys_of(self.img, lut)
        self.npx = np.array([np.count_nonzero(keys == k) for k in (1, 2, 3)], np.int64)
        self.last_root = int(self.root.max()) + 1 if n else 0
        value_at_root = self.img.ravel()[self.root]
        self.list1 = np.sort(self.root[value_at_root == 1])                  # roots of class 1 / 2 = the VALUE of the root pixel
        self.list2 = np.sort(self.root[value_at_root == 2])

    def at_roots(self, per_comp, dtype):
        """(H, W) array holding per_comp[c - 1] at component c's root pixel and 0 elsewhere."""
        out = np.zeros(self.img.size, dtype)
        out[self.root] = per_comp
        return out.reshape(self.img.shape)

    def flags(self, aux_mode, aux_c=0, aux=None):
        """Per component: OR of its pixels' bits."""
        bits = pixel_bits(self.img, aux_mode, aux_c, aux).ravel()
        flat = self.comp.ravel()
        f = np.zeros(self.n, np.int64)
        for b in range(5):
            hit = np.bincount(flat, weights=(bits >> b) & 1, minlength=self.n + 1)[1:] > 0
            f |= hit.astype(np.int64) << b
        return f

    def query(self, flags, key, need_bits):
        """Roots with this key (0: any) whose flag word holds all of need_bits."""
        ok = (flags & need_bits) == need_bits
        if key:
            ok &= self.key == key
        return int(np.count_nonzero(ok))


def allow_full_effective(conn, stat, need, count_only, allow_full):
    return bool(allow_full) and conn == 4 and stat == 0 and need == 0 and not count_only


def tile_model(keys, full_effective):
    """tile_any of the 64 x 32 tiles of one key image: 2 when full tiles are in effect and every valid pixel of the tile is keyed,
    else 1 when any is, else 0."""
    H, W = keys.shape
    ny, nx = -(-H // TILE_H), -(-W // TILE_W)
    out = np.zeros((ny, nx), np.uint8)
    for ty in range(ny):
        for tx in range(nx):
            t = keys[ty * TILE_H:(ty + 1) * TILE_H, tx * TILE_W:(tx + 1) * TILE_W] != 0
            out[ty, tx] = 2 if (full_effective and t.all()) else (1 if t.any() else 0)
    return out


def tile_eligible(H, W):
    """(ny, nx) bool: the tiles whose 8-byte pre-passes can run - W % 8 == 0 and the whole 64 x 32 tile inside the image."""
    ny, nx = -(-H // TILE_H), -(-W // TILE_W)
    e = np.zeros((ny, nx), bool)
    if W % 8 == 0:
        for ty in range(ny):
            for tx in range(nx):
                e[ty, tx] = (ty + 1) * TILE_H <= H and (tx + 1) * TILE_W <= W
    return e


def tile_owner_counts(img, lut, conn):
    """Per tile: the components of the tile labelled as an image of its own (the tile roots, 'owners', of the first phase)."""
    H, W = np.asarray(img).shape
    ny, nx = -(-H // TILE_H), -(-W // TILE_W)
    out = np.zeros((ny, nx), np.int64)
    for ty in range(ny):
        for tx in range(nx):
            out[ty, tx] = len(components(np.asarray(img)[ty * TILE_H:(ty + 1) * TILE_H, tx * TILE_W:(tx + 1) * TILE_W], lut, conn)[1])
    return out


# ---- the comparison of one device call with the reference (tests/test_gpu_ccl_pass.py, tests/test_gpu_scratch.py) ----
def check_queries(got, labs, aux, mode, queries, what):
    for i, lab in enumerate(labs):
        flags = lab.flags(mode.aux_mode, mode.aux_c, None if aux is None else aux[i])
        want = [lab.query(flags, qk, qn) for qk, qn in queries]
        assert got['cnt'][i, :len(queries)].tolist() == want, (what, i, queries)


def check_pass(got, imgs, aux, mode, labs, queries, what):
    """Everything one ``Handle.ccl_pass`` call exported (``got``) against the Labellings ``labs`` of its images, image by image."""
    full = allow_full_effective(mode.conn, mode.stat, mode.need, mode.count_only, mode.allow_full)
    for i, lab in enumerate(labs):
        w = (what, i)
        px = imgs[i].size
        idx = np.arange(px)
        assert np.array_equal(got['tile_any'][i], tile_model(keys_of(imgs[i], mode.lut), full)), w
        root = got['root'][i].ravel()
        zero = np.zeros(imgs[i].shape, np.int64)
        if mode.count_only:
            # no resolved roots: the pixels counted as roots are exactly the components' first pixels
            assert np.array_equal(np.flatnonzero(root >= 0), np.sort(lab.root)), w
            assert np.array_equal(root[root >= 0], idx[root >= 0]) and root.min(initial=-1) >= -1, w
            flags = None
            for k in ('area', 'sumy', 'sumx', 'flag'):
                assert not got[k][i].any(), (w, k)
        else:
            assert np.array_equal(got['root'][i], lab.root_px), w
            keyed = root >= 0
            assert np.array_equal(root[root[keyed]], root[keyed]) and (root[keyed] <= idx[keyed]).all(), w
            flags = lab.flags(mode.aux_mode, mode.aux_c, None if aux is None else aux[i])
            if mode.aux_mode == AUX_NONE:
                assert not flags.any()
            assert np.array_equal(got['flag'][i], lab.at_roots(flags, np.uint32)), w
            assert np.array_equal(got['area'][i], lab.at_roots(lab.area, np.uint32) if mode.stat & STAT_AREA else zero), w
            assert np.array_equal(got['sumy'][i], lab.at_roots(lab.sumy, np.uint64) if mode.stat & STAT_SUMS else zero), w
            assert np.array_equal(got['sumx'][i], lab.at_roots(lab.sumx, np.uint64) if mode.stat & STAT_SUMS else zero), w
        if mode.need & NEED_NCOMP:
            assert got['ncomp'][i].tolist() == lab.ncomp.tolist(), w
        if mode.need & NEED_NPX:
            assert got['npx'][i].tolist() == lab.npx.tolist(), w
        if mode.need & NEED_LAST:
            assert got['last_root'][i] == lab.last_root, w
        if mode.need & NEED_LISTS:
            for k, want in (('1', lab.list1), ('2', lab.list2)):
                lst = np.sort(got['list' + k][i])
                assert got['nlist' + k][i] == len(want) and np.array_equal(lst, want) and len(np.unique(lst)) == len(lst), (w, k)
    if queries:
        check_queries(got, labs, aux, mode, queries, what)
