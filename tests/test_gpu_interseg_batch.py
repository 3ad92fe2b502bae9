"""The regions, crops and classifiers of many interSeg images in one device call (ecseg_interseg_batch, ``Handle.interseg_many``;
csrc/interseg_kernels.hip, csrc/iseg_batch.h).  Every case is held to ``nuclei_regions`` + ``classify_nucleus_crops`` called per image
on the same handle and models: records, crop owners, maxima, ``ran_*`` and the predictions bit for bit - both paths feed the same
float32 inputs to the same plans, and no kernel of the two classifiers depends on the batch (tests/test_gpu_iseg_classify.py), so
nothing but equality is acceptable.  The classifiers are the seeded synthetic ones of ``synth.classifier_config``."""
import ctypes as C

import numpy as np
import pytest

from ecseg_amd import interseg, synth
from ecseg_amd._lib import EcsegError, Handle
from ecseg_amd.model import MetasegModel

pytestmark = pytest.mark.gpu


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.fixture(scope='module')
def models():
    hs = [Handle(0), Handle(0)]
    out = []
    for kind, h, seed in (('interseg', hs[0], 3), ('ecseg_c', hs[1], 4)):
        cfg = synth.classifier_config(kind)
        out.append(MetasegModel(cfg, synth.classifier_weights(cfg, seed=seed), handle=h))
    yield tuple(out)
    for h in hs:
        h.close()


# ---- scenes ---------------------------------------------------------------------------------------------------------------------
def image_for(rng, seg, C=3, extra=(0, 0), bright=True):
    """A (h + extra, w + extra, C) image over ``seg``: random, the two FISH channels raised above the brightness gate and the
    centromere gate under a part of the nuclei (``bright``), or all below the brightness gate."""
    H, W = seg.shape[0] + extra[0], seg.shape[1] + extra[1]
    img = rng.integers(0, 256 if bright else 12, (H, W, C), dtype=np.uint8)
    if bright:
        img[:seg.shape[0], :seg.shape[1], :2][seg != 0] |= 64
    return img


def boxes_mask(h, w, boxes):
    seg = np.zeros((h, w), np.uint8)
    for y, x, bh, bw in boxes:
        seg[y:y + bh, x:x + bw] = 255
    return seg


def grid_nuclei(h, w, n, size=3, pitch=5):
    """n nuclei of size x size on a lattice: n regions, one crop each when they pass the gate"""
    per_row = (w - 1) // pitch
    assert n <= per_row * ((h - 1) // pitch)
    return boxes_mask(h, w, [(1 + pitch * (k // per_row), 1 + pitch * (k % per_row), size, size) for k in range(n)])


def three_extents(rng):
    """40 x 56, 41 x 43 and 300 x 280; the last holds a nucleus 290 rows tall: the tiled path, whose one 256 x 30 tile is all zero
    (an empty tile) while the rows below it carry the nucleus over the brightness gate."""
    a = boxes_mask(40, 56, [(2, 3, 9, 11), (20, 30, 15, 20), (38, 0, 2, 5)])
    b = boxes_mask(41, 43, [(0, 0, 5, 5), (10, 12, 21, 23), (40, 42, 1, 1)])
    c = boxes_mask(300, 280, [(3, 4, 290, 30), (5, 60, 40, 50), (100, 100, 33, 31)])
    imgs = [image_for(rng, s) for s in (a, b, c)]
    imgs[2][3:259, 4:34, :] = 0                              # the 256-row tile of the tall nucleus is all zero: an empty tile ...
    imgs[2][259:293, 4:34, 0] = 255                          # ... of a nucleus that still passes the brightness gate below it
    return imgs, [a, b, c]


# ---- the reference: image by image ----------------------------------------------------------------------------------------------
def alone(handle, mi, mc, img, seg, fish, run_c):
    """(records, owner, maxima, pred_i, ran_i, pred_c, ran_c) of one image through today's two calls, or the EcsegError."""
    try:
        rec = handle.nuclei_regions(seg, img, fish)
    except EcsegError as e:
        return e
    _, _, desc, tiled, owner = interseg.region_rows(rec)
    if not len(desc):
        return rec, owner, np.zeros((0, 3), np.int32), np.zeros((0, 3), np.float32), np.zeros(0, bool), np.zeros(0, np.float32), np.zeros(0, bool)
    mx, pi, ri, pc, rc = handle.classify_nucleus_crops(desc, (fish, 1 - fish, 2), tiled, bool(run_c) and mc is not None, mi, mc)
    return rec, owner, mx, pi, ri, pc, rc


def same_predictions(got, want, who):
    owner, pi, ri, pc, rc = got
    _, w_owner, _, w_pi, w_ri, w_pc, w_rc = want
    assert np.array_equal(owner, w_owner), who
    assert np.array_equal(ri, w_ri) and np.array_equal(rc, w_rc), who
    assert np.array_equal(bits(pi[ri]), bits(w_pi[w_ri])), who               # NaN included
    assert np.array_equal(bits(pc[rc]), bits(w_pc[w_rc])), who


def check_many(handle, mi, mc, imgs, segs, fish=0, run_c=None, **kw):
    run_c = [True] * len(imgs) if run_c is None else run_c
    want = [alone(handle, mi, mc, im, sg, fish, rc) for im, sg, rc in zip(imgs, segs, run_c)]
    got = handle.interseg_many(imgs, segs, fish, run_c, mi, mc, **kw)
    assert len(got) == len(imgs)
    for k, (g, w) in enumerate(zip(got, want)):
        if isinstance(w, EcsegError):
            assert isinstance(g, EcsegError) and g.code == -1 and str(g) == str(w), k
            continue
        assert not isinstance(g, Exception), (k, g)
        assert g[0].dtype == np.int64 and np.array_equal(g[0], w[0]), 'records of image %d' % k
        same_predictions(g[1], w, 'image %d' % k)
    print('%s: %d images, regions %s, crops %s, ecSeg-c ran %s' % (handle.device_name, len(imgs), [len(w[0]) if not isinstance(w, Exception) else 'E' for w in want],
                                                                 [len(w[1]) if not isinstance(w, Exception) else 'E' for w in want],
                                                                 [int(w[6].sum()) if not isinstance(w, Exception) else 'E' for w in want]))
    return got, want


def pack(imgs, segs, run_c, gaps):
    """The packed buffer (gap bytes 0xAB) and the table, image k preceded by gaps[2k] bytes and its mask by gaps[2k + 1]."""
    parts, tab, off = [], np.zeros((len(imgs), 8), np.int64), 0
    for k, (im, sg) in enumerate(zip(imgs, segs)):
        g0, g1 = gaps[2 * k], gaps[2 * k + 1]
        parts += [np.full(g0, 0xAB, np.uint8), im.reshape(-1), np.full(g1, 0xAB, np.uint8), sg.reshape(-1)]
        tab[k] = (off + g0, im.shape[0], im.shape[1], im.shape[2], off + g0 + im.size + g1, sg.shape[0], sg.shape[1], int(run_c[k]))
        off += g0 + im.size + g1 + sg.size
    return np.concatenate(parts), tab


def check_packed(handle, mi, mc, imgs, segs, fish, run_c, gaps):
    want = [alone(handle, mi, mc, im, sg, fish, rc) for im, sg, rc in zip(imgs, segs, run_c)]
    buf, tab = pack(imgs, segs, run_c, gaps)
    nr, ncr = sum(len(w[0]) for w in want), sum(len(w[1]) for w in want)
    out, rec, region, mx, pi, ri, pc, rc = handle.interseg_batch_packed(buf, tab, fish, mi, mc, nr, ncr)      # exactly enough room
    r0 = c0 = 0
    for k, w in enumerate(want):
        assert out[k].tolist() == [0, len(w[0]), r0, len(w[1]), c0, out[k, 5], out[k, 6], 0], (k, out[k])
        assert np.array_equal(rec[r0:r0 + len(w[0])], w[0])
        sl = slice(c0, c0 + len(w[1]))
        assert np.array_equal(mx[sl], w[2])
        same_predictions((region[sl], pi[sl], ri[sl], pc[sl], rc[sl]), w, 'image %d' % k)
        r0 += len(w[0])
        c0 += len(w[1])


# ---- cases ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('reverse', [False, True])
@pytest.mark.parametrize('fish', [0, 1])
def test_three_extents_in_one_call_with_gaps(gpu, models, reverse, fish):
    mi, mc = models
    rng = np.random.default_rng(5)
    imgs, segs = three_extents(rng)
    if reverse:
        imgs, segs = imgs[::-1], segs[::-1]
    _, want = check_many(gpu, mi, mc, imgs, segs, fish)
    tall = want[0 if reverse else 2]
    assert len(tall[0]) == 3 and not tall[4].all() and tall[4].sum() == 2     # the tall nucleus: one tile, empty, ecSeg-i did not run
    check_packed(gpu, mi, mc, imgs, segs, fish, [True] * 3, gaps=[0, 7, 1, 2, 3, 5] if reverse else [5, 0, 7, 3, 0, 1])


def test_segmentations_smaller_than_their_images(gpu, models):
    mi, mc = models
    rng = np.random.default_rng(6)
    segs = [boxes_mask(33, 70, [(1, 1, 20, 30), (30, 60, 3, 10)]), boxes_mask(65, 20, [(0, 0, 65, 3), (10, 10, 8, 8)])]
    imgs = [image_for(rng, segs[0], C=4, extra=(9, 5)), image_for(rng, segs[1], C=3, extra=(1, 40))]
    check_many(gpu, mi, mc, imgs, segs, 1)


def test_crops_cross_the_256_boundary_between_images(gpu, models):
    mi, mc = models
    rng = np.random.default_rng(7)
    segs = [grid_nuclei(60, 60, 100), grid_nuclei(70, 70, 157), grid_nuclei(12, 30, 3)]
    imgs = [image_for(rng, s) for s in segs]
    _, want = check_many(gpu, mi, mc, imgs, segs, 0)
    assert [len(w[1]) for w in want] == [100, 157, 3]        # 256 + 4: the first chunk ends inside image 1, the last holds 4 crops


@pytest.mark.parametrize('where', [0, 1, 2])
def test_an_image_without_nuclei(gpu, models, where):
    mi, mc = models
    rng = np.random.default_rng(8)
    segs = [boxes_mask(30, 40, [(2, 2, 10, 10)]), boxes_mask(20, 70, [(1, 50, 12, 9), (15, 3, 4, 4)])]
    segs.insert(where, np.zeros((25, 33), np.uint8))
    imgs = [image_for(rng, s) for s in segs]
    got, _ = check_many(gpu, mi, mc, imgs, segs, 0)
    assert got[where][0].shape == (0, 8) and len(got[where][1][0]) == 0


def test_one_image_and_no_image(gpu, models):
    mi, mc = models
    rng = np.random.default_rng(9)
    seg = boxes_mask(50, 45, [(3, 3, 20, 20), (30, 5, 10, 30)])
    check_many(gpu, mi, mc, [image_for(rng, seg)], [seg], 1)
    assert gpu.interseg_many([], [], 0, [], mi, mc) == []


def test_an_instance_id_image_fails_alone(gpu, models):
    mi, mc = models
    rng = np.random.default_rng(10)
    segs = [boxes_mask(30, 40, [(2, 2, 10, 10)]), boxes_mask(28, 36, [(1, 1, 5, 5), (10, 10, 6, 6)]), boxes_mask(20, 70, [(1, 50, 12, 9)])]
    segs[1][10:16, 10:16] = 7                                # two different non-zero values
    imgs = [image_for(rng, s) for s in segs]
    got, _ = check_many(gpu, mi, mc, imgs, segs, 0)
    assert isinstance(got[1], EcsegError) and '7 .. 255' in str(got[1]) and not isinstance(got[0], Exception) and not isinstance(got[2], Exception)


def test_run_c_is_per_image_and_model_c_may_be_missing(gpu, models):
    mi, mc = models
    rng = np.random.default_rng(11)
    segs = [boxes_mask(30, 40, [(2, 2, 10, 10), (15, 20, 9, 9)]), boxes_mask(28, 36, [(1, 1, 5, 5), (10, 10, 6, 6)]), boxes_mask(20, 70, [(1, 50, 12, 9)])]
    imgs = [image_for(rng, s) for s in segs]
    got, _ = check_many(gpu, mi, mc, imgs, segs, 0, run_c=[True, False, True])
    assert got[0][1][4].all() and not got[1][1][4].any() and got[2][1][4].all()
    got, _ = check_many(gpu, mi, None, imgs, segs, 0, run_c=[True, False, True])
    assert not any(g[1][4].any() for g in got)


def test_more_regions_than_the_lds_table_in_one_tile_beside_a_normal_image(gpu, models):
    mi, mc = models
    rng = np.random.default_rng(12)
    lattice = np.zeros((96, 192), np.uint8)                  # 512 isolated pixels in statistics tile (1, 1): 8 regions per LDS slot
    sites = np.arange(512)
    lattice[32 + 2 * (sites // 32), 64 + 2 * (sites % 32)] = 255
    lattice[2:6, 2:40] = 255
    normal = boxes_mask(50, 45, [(3, 3, 20, 20), (30, 5, 10, 30)])
    imgs = [image_for(rng, lattice, bright=False), image_for(rng, normal)]    # (below the gate: 513 regions, no crop)
    for order in ((0, 1), (1, 0)):
        got, want = check_many(gpu, mi, mc, [imgs[k] for k in order], [[lattice, normal][k] for k in order], 0)
        assert sorted(len(w[0]) for w in want) == [2, 513]


def test_equal_region_indices_of_two_images_do_not_mix(gpu, models):
    mi, mc = models
    rng = np.random.default_rng(13)
    seg = boxes_mask(40, 70, [(2, 2, 10, 10), (5, 30, 20, 25), (30, 1, 6, 60)])
    imgs = [image_for(rng, seg), image_for(rng, seg)]        # the same regions 0, 1, 2 in the same tiles, other pixel values
    got, _ = check_many(gpu, mi, mc, imgs, [seg, seg], 0)
    assert np.array_equal(got[0][0][:, :7], got[1][0][:, :7]) and not np.array_equal(got[0][0][:, 7], got[1][0][:, 7])


def test_capacity_one_short_is_reported_for_its_image_and_nothing_is_written_behind(gpu, models):
    mi, mc = models
    rng = np.random.default_rng(14)
    segs = [boxes_mask(30, 40, [(2, 2, 10, 10), (15, 20, 9, 9)]), boxes_mask(28, 36, [(1, 1, 5, 5), (10, 10, 6, 6), (20, 2, 4, 30)]),
            boxes_mask(20, 70, [(1, 50, 12, 9)])]
    imgs = [image_for(rng, s) for s in segs]
    want = [alone(gpu, mi, mc, im, sg, 0, True) for im, sg in zip(imgs, segs)]
    assert [len(w[0]) for w in want] == [2, 3, 1] and [len(w[1]) for w in want] == [2, 3, 1]
    buf, tab = pack(imgs, segs, [1, 1, 1], [0] * 6)
    hi, hc = mi.handle, mc.handle
    GUARD = 16

    def call(rcap, ccap):
        out = np.full((3 + 1, 8), -77, np.int32)
        rec = np.full((rcap + GUARD, 8), -77, np.int64)
        region, mx = np.full(ccap + GUARD, -77, np.int32), np.full((ccap + GUARD, 3), -77, np.int32)
        pi, pc = np.full((ccap + GUARD, 3), -77.5, np.float32), np.full(ccap + GUARD, -77.5, np.float32)
        ri, rc = np.full(ccap + GUARD, 77, np.uint8), np.full(ccap + GUARD, 77, np.uint8)
        p = lambda a: a.ctypes.data_as(C.c_void_p)
        status = gpu.lib.ecseg_interseg_batch(gpu.h, hi.h, hc.h, p(buf), buf.size, p(tab), 3, 0, rcap, ccap, p(out), p(rec), p(region), p(mx), p(pi),
                                              p(ri), p(pc), p(rc))
        assert status == 0
        assert (out[3] == -77).all() and (rec[rcap:] == -77).all() and (region[ccap:] == -77).all() and (mx[ccap:] == -77).all()
        assert (pi[ccap:] == -77.5).all() and (pc[ccap:] == -77.5).all() and (ri[ccap:] == 77).all() and (rc[ccap:] == 77).all()
        return out[:3], rec, region, pi, ri

    # records: 6 needed, 5 given - image 1 (3 regions) fits behind image 0, image 2 (1 region) does not ... so give 4: image 1 does not fit
    out, rec, region, pi, ri = call(4, 6)
    assert out[:, 0].tolist() == [0, gpu.ISEG_RECORDS_OVERFLOW, 0] and out[:, 1].tolist() == [2, 3, 1]
    assert out[:, 2].tolist() == [0, -1, 2] and out[:, 4].tolist() == [0, -1, 2]
    assert np.array_equal(rec[:2], want[0][0]) and np.array_equal(rec[2:3], want[2][0]) and (rec[3:] == -77).all()
    assert np.array_equal(bits(pi[:2]), bits(want[0][3])) and np.array_equal(bits(pi[2:3]), bits(want[2][3])) and (pi[3:] == -77.5).all()
    out, rec, _, _, _ = call(5, 6)                           # one short in all: the last image is the one without room
    assert out[:, 0].tolist() == [0, 0, gpu.ISEG_RECORDS_OVERFLOW] and (rec[5:] == -77).all()
    # crops: 6 needed, 5 given
    out, rec, region, pi, ri = call(6, 5)
    assert out[:, 0].tolist() == [0, 0, gpu.ISEG_CROPS_OVERFLOW] and out[:, 3].tolist() == [2, 3, 1] and out[:, 4].tolist() == [0, 2, -1]
    assert np.array_equal(rec[:6], np.concatenate([w[0] for w in want]))
    assert np.array_equal(bits(pi[:5]), bits(np.concatenate([want[0][3], want[1][3]])))
    out, _, _, _, _ = call(6, 4)                             # image 1's three crops do not fit, image 2's one does
    assert out[:, 0].tolist() == [0, gpu.ISEG_CROPS_OVERFLOW, 0] and out[:, 4].tolist() == [0, -1, 2]
    # and interseg_many comes back for what did not fit
    check_many(gpu, mi, mc, imgs, segs, 0, record_capacity=4, crop_capacity=2)


def test_the_same_call_twice_after_a_larger_one(gpu, models):
    mi, mc = models
    rng = np.random.default_rng(15)
    big = [grid_nuclei(120, 150, 40), boxes_mask(200, 90, [(5, 5, 150, 60)])]
    check_many(gpu, mi, mc, [image_for(rng, s) for s in big], big, 0)
    segs = [boxes_mask(30, 40, [(2, 2, 10, 10), (15, 20, 9, 9)]), boxes_mask(28, 36, [(1, 1, 5, 5), (10, 10, 6, 6)])]
    imgs = [image_for(rng, s) for s in segs]
    first = gpu.interseg_many(imgs, segs, 0, [True, True], mi, mc)
    second = gpu.interseg_many(imgs, segs, 0, [True, True], mi, mc)
    for a, b in zip(first, second):
        assert np.array_equal(a[0], b[0])
        for x, y in zip(a[1], b[1]):
            assert np.array_equal(bits(x), bits(y)) if x.dtype == np.float32 else np.array_equal(x, y)
    check_many(gpu, mi, mc, imgs, segs, 0)
    # the region map nuclei_regions left on the handle is not the batch's to touch
    rec = gpu.nuclei_regions(segs[0], imgs[0], 0)
    _, _, desc, _, _ = interseg.region_rows(rec)
    crops = gpu.nucleus_crops(desc)[0]
    gpu.interseg_many(imgs[::-1], segs[::-1], 0, [True, True], mi, mc)
    assert np.array_equal(gpu.nucleus_crops(desc)[0], crops)


def test_bad_tables_are_refused_before_anything_is_read(gpu, models):
    mi, mc = models
    rng = np.random.default_rng(16)
    seg = boxes_mask(30, 40, [(2, 2, 10, 10)])
    img = image_for(rng, seg)
    buf, tab = pack([img, img], [seg, seg], [1, 1], [0, 0, 0, 0])
    for row, col, value in ((1, 0, tab[1, 0] - 1), (1, 4, tab[1, 4] - 1), (1, 4, buf.size), (0, 5, 31), (0, 3, 2), (0, 7, 2), (1, 0, 0)):
        bad = tab.copy()
        bad[row, col] = value
        with pytest.raises(EcsegError) as e:
            gpu.interseg_batch_packed(buf, bad, 0, mi, mc, 8, 8)
        assert e.value.code == -1 and 'image %d' % row in str(e.value)
    with pytest.raises(EcsegError):
        gpu.interseg_batch_packed(buf, tab, 2, mi, mc, 8, 8)
    with pytest.raises(EcsegError):
        gpu.interseg_batch_packed(buf, tab, 0, mc, mc, 8, 8)     # ecSeg-c's plan is no ecSeg-i
