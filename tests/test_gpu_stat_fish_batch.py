"""ecseg_stat_fish_batch (csrc/drivers_fish.hip, the fsb_* kernels of csrc/fishspot_kernels.hip, csrc/fish_batch.h), its binding
``Handle.stat_fish_many`` and ``stat_fish.batch`` of ``make stat_fish`` on the device.  Every comparison is ``array_equal`` or byte
equality against two yardsticks that are not the code under test: the numpy restatement tests/stat_fish_ref.py, and the single-image
chain on the same handle (``ccl_labels`` -> ``fish_spots`` -> ``fish_render_tiff`` / ``tiff_encode``).  No committed case holds a pixel
within 2 B of its ``normal_threshold`` (``ref.records`` counts them, as tests/test_gpu_stat_fish.py asserts it): that is
a condition on the inputs, checked on the CPU, not a tolerance."""
import os
import sys

import numpy as np
import pytest
import yaml

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import stat_fish_cases as cases              # noqa: E402
import stat_fish_ref as ref                  # noqa: E402
from ecseg_amd import image_io               # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the inputs -----------------------------------------------------------------------------------------------------------------
make_item = cases.make_item                 # (shared with tests/test_gpu_scratch.py)


def _disconnected(item):
    """a given-labels image with a cell in two parts: two far corners share label 3"""
    lab = np.zeros(item['img'].shape[:2], np.int32)
    lab[2:20, 3:30] = 3; lab[70:90, 150:190] = 3; lab[30:60, 60:120] = 2; lab[5:25, 100:140] = 1
    item['labels'] = lab
    return item


def _sparse_values(item):
    """a given-labels image whose label values exceed the cell count"""
    lab = np.zeros(item['img'].shape[:2], np.int32)
    lab[1:20, 1:20] = 4000; lab[25:50, 10:60] = 5; lab[40:63, 30:64] = 900; lab[0:10, 40:64] = -7
    item['labels'] = lab
    return item


def _one_pixel():
    img = np.array([[[9, 200, 30]]], np.uint8)
    return dict(img=img, channels=[0, 1, 2], labels=np.array([[1]], np.int32), weights=cases.NAN1, normal_threshold=15.0,
                intensity_thresholds=[70.0, 70.0], min_cc_size=1)


_CHUNK = None


def chunk():
    """The chunk with everything in it, built once: C = 3 and 4, K = 1 (NaN weights), 3, 7 and 63, a min_cc_size per image, an
    all-background and an all-foreground mask, a disconnected cell, label values above the cell count, a picture; 41 x 43 (it ends on
    an odd byte) beside 128 x 127, 1 x 1, 16 x 64 and 17 x 65 around the 64 x 16 threshold tile, 96 x 200."""
    global _CHUNK
    if _CHUNK is None:
        _CHUNK = [make_item(601, (41, 43), 3, 3, 'mask', min_cc=2),
                  make_item(610, (128, 127), 7, 4, 'mask', min_cc=5, picture=True),
                  _one_pixel(),
                  make_item(603, (16, 64), 7, 3, 'background'),
                  make_item(604, (17, 65), 3, 4, 'foreground', min_cc=1, mask_file=False),
                  _disconnected(make_item(605, (96, 200), 63, 3, 'labels', min_cc=3)),
                  _sparse_values(make_item(606, (64, 64), 7, 3, 'labels', min_cc=1, picture=True))]
    return _CHUNK


_WANT = {}


def reference(item, line):
    """tests/stat_fish_ref.py on an item -> (ranks, records, thresholded, boundaries, ambiguous); computed once per (item, line)."""
    key = (id(item), line)
    if key not in _WANT:
        seg = ref.nuclei(item['mask']) if item.get('mask') is not None else item['labels']
        rec, thr, bnd, amb = ref.records(item['img'], seg, item['channels'][1:], item['weights'], item['normal_threshold'],
                                         item['intensity_thresholds'], item['min_cc_size'], line)
        _WANT[key] = (ref.ranks(seg)[0].astype(np.int32), rec, thr, bnd, amb)
    return _WANT[key]


_CHAIN = {}


def chain(gpu, item, line):
    """The single-image chain on the handle -> (ranks, records, files, thresholded, boundaries); once per (item, line)."""
    key = (id(item), line)
    if key not in _CHAIN:
        labels = gpu.ccl_labels(item['mask'], 8) if item.get('mask') is not None else np.ascontiguousarray(item['labels'], np.int32)
        rec, thr, bnd = gpu.fish_spots(labels, item['img'], item['channels'][1:], item['weights'], item['normal_threshold'],
                                       item['intensity_thresholds'], item['min_cc_size'], line)
        lut = np.zeros(labels.size + 1, np.int32)
        lut[rec[:, 0]] = np.arange(1, len(rec) + 1, dtype=np.int32)
        ranks = lut[np.maximum(labels, 0)]
        mask_file = item.get('mask_file')
        mask_file = item['mask'] if mask_file is True else mask_file
        files = tuple(gpu.fish_render_tiff(item['img'], item['channels'], thr, bnd)) + \
            (None if mask_file is None else gpu.tiff_encode(mask_file), None if item.get('picture') is None else gpu.tiff_encode(item['picture']))
        _CHAIN[key] = (ranks, rec, files, thr, bnd)
    return _CHAIN[key]


def assert_same(got, want, what):
    assert np.array_equal(got[0], want[0]), what + ': ranks'
    assert got[1].shape == want[1].shape and np.array_equal(got[1], want[1]), what + ': records'
    assert got[2] == want[2], what + ': files'
    if len(got) > 3:
        assert np.array_equal(got[3], want[3]), what + ': thresholded'
        assert np.array_equal(got[4], want[4]), what + ': boundaries'


def assert_matches_reference(got, item, line, what):
    ranks, rec, thr, bnd, amb = reference(item, line)
    assert amb == 0
    assert np.array_equal(got[0], ranks), what + ': ranks against the oracle'
    assert got[1].shape == rec.shape, what + ': cells'
    cols = slice(1, None) if item.get('mask') is not None else slice(0, None)   # (a labelled mask numbers its cells by first pixel)
    assert np.array_equal(got[1][:, cols], rec[:, cols]), what + ': records against the oracle'
    assert np.array_equal(got[3], thr) and np.array_equal(got[4], bnd), what + ': masks against the oracle'


# ---- the inputs' condition ------------------------------------------------------------------------------------------------------
def test_no_case_holds_a_pixel_within_2b_of_the_threshold():
    for k, item in enumerate(chunk()):
        for line in (1, 2):
            assert reference(item, line)[4] == 0, 'item %d holds ambiguous pixels: not a committed case' % k


# ---- a batch of one -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('k', range(7))
def test_batch_of_one_equals_the_single_chain(gpu, k):
    item = chunk()[k]
    got = gpu.stat_fish_many([item], 1, want_masks=True)[0]
    assert_same(got, chain(gpu, item, 1), 'item %d' % k)
    assert_matches_reference(got, item, 1, 'item %d' % k)


# ---- the chunk, and the same chunk laid out differently -------------------------------------------------------------------------
@pytest.mark.parametrize('line', [1, 2])
def test_chunk_equals_chain_and_oracle(gpu, line):
    got = gpu.stat_fish_many(chunk(), line, want_masks=True)
    for k, (g, item) in enumerate(zip(got, chunk())):
        assert_same(g, chain(gpu, item, line), 'item %d' % k)
        assert_matches_reference(g, item, line, 'item %d' % k)
    assert len(got[3][1]) == 0 and not got[3][0].any()       # the all-background image: no ranks, no records, its files all the same
    assert len(got[4][1]) == 1


def _gapped(items):
    """the same items with every raster a view into one buffer, 0..7 bytes between a raster and the next"""
    total = sum(sum(np.asarray(v).nbytes + 8 for v in it.values() if isinstance(v, np.ndarray)) for it in items)
    buf = np.zeros(total + 64, np.uint8)
    at, gap, out = 0, 0, []
    for it in items:
        new = dict(it)
        for key in ('img', 'mask', 'labels', 'picture'):
            v = it.get(key)
            if not isinstance(v, np.ndarray):
                continue
            at += gap
            gap = (gap + 3) % 8
            view = buf[at:at + v.nbytes].view(v.dtype).reshape(v.shape) if at % v.dtype.itemsize == 0 else \
                np.ndarray(v.shape, v.dtype, buffer=buf.data, offset=at)
            view[...] = v
            new[key] = view
            at += v.nbytes
        out.append(new)
    return out


def test_order_and_gaps_do_not_change_an_image(gpu):
    items = chunk()
    base = gpu.stat_fish_many(items, 1, want_masks=True)
    n = len(items)
    for order in (list(range(n))[::-1], [(k + 3) % n for k in range(n)]):
        got = gpu.stat_fish_many([items[k] for k in order], 1, want_masks=True)
        for g, k in zip(got, order):
            assert_same(g, base[k], 'item %d moved' % k)
    got = gpu.stat_fish_many(_gapped(items), 1, want_masks=True)
    for k, g in enumerate(got):
        assert_same(g, base[k], 'item %d with gaps' % k)


def test_two_calls_give_identical_bytes(gpu):
    a = gpu.stat_fish_many(chunk(), 2, want_masks=True)
    gpu.stat_fish_many(chunk()[:2], 1)
    b = gpu.stat_fish_many(chunk(), 2, want_masks=True)
    for x, y in zip(a, b):
        assert_same(x, y, 'second call')
        assert all(p.tobytes() == q.tobytes() for p, q in zip((x[0], x[1], x[3], x[4]), (y[0], y[1], y[3], y[4])))


# ---- the capacities ---------------------------------------------------------------------------------------------------------------
def test_record_capacity_one_short_returns_the_counts_alone(gpu):
    items = chunk()
    prepared = [gpu._stat_fish_item(it) for it in items]
    want = [len(reference(it, 1)[1]) for it in items]
    total = sum(want)
    res = gpu.stat_fish_packed(prepared, 1, total - 1, want_masks=True, poison=0x5a)
    assert res['n_cells'].tolist() == want
    for key in ('ranks', 'records', 'out', 'ranges', 'thresholded', 'boundaries'):
        assert (res[key].view(np.uint8) == 0x5a).all(), key + ' was written'
    full = gpu.stat_fish_packed(prepared, 1, total, want_masks=True, poison=0x5a)
    assert full['n_cells'].tolist() == want and not (full['records'].view(np.uint8) == 0x5a).all()
    got = gpu.stat_fish_many(items, 1, record_capacity=total - 1, want_masks=True)      # the binding grows it and comes back once
    for k, (g, item) in enumerate(zip(got, items)):
        assert_same(g, chain(gpu, item, 1), 'item %d' % k)


def test_out_cap_one_short_is_refused_with_nothing_written(gpu):
    from ecseg_amd._lib import EcsegError
    items = chunk()[:3]
    prepared = [gpu._stat_fish_item(it) for it in items]
    need = sum(len(f) for it in items for f in chain(gpu, it, 1)[2] if f is not None)
    with pytest.raises(EcsegError) as e:
        gpu.stat_fish_packed(prepared, 1, 4096, out_capacity=need - 1)
    assert e.value.code == -1 and 'do not fit' in str(e.value)
    from ecseg_amd._lib import C, _ptr
    res = {}
    orig_check = gpu._check
    try:                                                     # once more through the same call, keeping the buffers: none was touched
        gpu._check = lambda rc, what: res.setdefault('rc', rc)
        out = gpu.stat_fish_packed(prepared, 1, 4096, out_capacity=need - 1, want_masks=True, poison=0x5a)
    finally:
        gpu._check = orig_check
    assert res['rc'] == -1
    for key in ('ranks', 'records', 'out', 'ranges', 'thresholded', 'boundaries'):
        assert (out[key].view(np.uint8) == 0x5a).all(), key + ' was written'
    ok = gpu.stat_fish_packed(prepared, 1, 4096, out_capacity=need)
    assert int(ok['ranges'][..., 1].sum()) == need


# ---- argument errors name the image --------------------------------------------------------------------------------------------
def test_argument_errors_name_the_middle_image(gpu):
    from ecseg_amd._lib import EcsegError
    items = chunk()[:3]
    good = [gpu._stat_fish_item(it) for it in items]

    def broken(**change):
        im, ch, mask, labels, w, normal, ithr, min_cc, mask_file, picture = good[1]
        d = dict(im=im, ch=ch, mask=mask, labels=labels, w=w, normal=normal, ithr=ithr, min_cc=min_cc, mask_file=mask_file, picture=picture)
        d.update(change)
        return [good[0], (d['im'], d['ch'], d['mask'], d['labels'], d['w'], d['normal'], d['ithr'], d['min_cc'], d['mask_file'], d['picture']), good[2]]
    H, W = good[1][0].shape[:2]
    too_big = np.ones((H, W), np.int32); too_big[5, 5] = H * W + 1
    for change, text in ((dict(ch=np.array([0, 1, 2, 7], np.int32)), 'channel index out of range'),
                         (dict(w=np.zeros((2, 2))), 'odd'), (dict(w=np.zeros((65, 65))), 'odd'),
                         (dict(im=np.zeros((H, W, 5), np.uint8)), '3 or 4 channels'),
                         (dict(labels=np.ones((H, W), np.int32)), 'exactly one'),
                         (dict(mask=None, mask_file=None), 'exactly one'),
                         (dict(mask=None, mask_file=None, labels=too_big), 'larger than H \\* W')):
        with pytest.raises(EcsegError, match=text) as e:
            gpu.stat_fish_packed(broken(**change), 1, 4096)
        assert e.value.code == -1 and 'image 1:' in str(e.value), str(e.value)
    for line in (0, 17):
        with pytest.raises(EcsegError, match='line_thickness'):
            gpu.stat_fish_packed(good, line, 4096)
    got = gpu.stat_fish_many(items, 1)                       # the handle is usable afterwards
    for k, (g, item) in enumerate(zip(got, items)):
        assert_same(g, chain(gpu, item, 1)[:3], 'item %d' % k)
    # the binding's own validation: the exception stands in the item's place, the neighbours run
    bad = dict(items[1]); bad['mask'] = bad['mask'][:-1]
    got = gpu.stat_fish_many([items[0], bad, items[2]], 1)
    assert isinstance(got[1], ValueError)
    assert_same(got[0], chain(gpu, items[0], 1)[:3], 'item 0')
    assert_same(got[2], chain(gpu, items[2], 1)[:3], 'item 2')


# ---- many, large and small ------------------------------------------------------------------------------------------------------
def test_301_tiny_images_in_one_call(gpu):
    rng = np.random.default_rng(12)
    items = []
    for k in range(301):
        H, W = int(rng.integers(1, 6)), int(rng.integers(1, 6))
        img = rng.integers(0, 256, (H, W, 3)).astype(np.uint8)
        items.append(dict(img=img, channels=[2, 1, 0], mask=(rng.random((H, W)) < 0.6).astype(np.uint8), weights=cases.NAN1,
                          normal_threshold=15.0, intensity_thresholds=[70.0, 70.0], min_cc_size=1 + k % 2))
    prepared = [gpu._stat_fish_item(it) for it in items]
    assert gpu.stat_fish_batch_bytes(prepared, 4096) < 8 << 30
    got = gpu.stat_fish_many(items, 1, want_masks=True)
    for k in range(0, 301, 1):
        item = items[k]
        seg = ref.nuclei(item['mask'])
        rec, thr, bnd, amb = ref.records(item['img'], seg, [1, 0], cases.NAN1, 15.0, [70.0, 70.0], item['min_cc_size'], 1)
        assert amb == 0
        assert np.array_equal(got[k][0], seg) and np.array_equal(got[k][1][:, 1:], rec[:, 1:]), k
        assert np.array_equal(got[k][3], thr) and np.array_equal(got[k][4], bnd), k
    for k in (0, 150, 300):
        assert_same(got[k], chain(gpu, items[k], 1), 'tiny %d' % k)


def test_arena_reuse_large_tiny_large(gpu):
    big = [make_item(613, (200, 257), 7, 3, 'mask'), make_item(612, (150, 150), 3, 4, 'mask')]
    for it in big:
        assert reference(it, 1)[4] == 0
    a = gpu.stat_fish_many(big, 1, want_masks=True)
    tiny = gpu.stat_fish_many([_one_pixel()], 1, want_masks=True)
    b = gpu.stat_fish_many(big, 1, want_masks=True)
    assert_same(tiny[0], chain(gpu, chunk()[2], 1), 'tiny')
    for k, (x, y, it) in enumerate(zip(a, b, big)):
        assert_same(x, y, 'large again %d' % k)
        assert_same(x, chain(gpu, it, 1), 'large %d' % k)
        assert_matches_reference(x, it, 1, 'large %d' % k)


def test_a_budget_that_forces_three_calls_gives_the_same_list(gpu):
    items = chunk()
    needs = [gpu.stat_fish_batch_bytes([gpu._stat_fish_item(it)], 0) for it in items]
    assert all(n > 0 for n in needs)
    calls = []
    packed = gpu.stat_fish_packed
    budget = max(max(needs), (sum(needs) + 2) // 3)
    assert len(gpu._split_by_budget(needs, budget)) >= 3
    gpu.stat_fish_packed = lambda chunk_, *a, **k: (calls.append(len(chunk_)), packed(chunk_, *a, **k))[1]
    try:
        got = gpu.stat_fish_many(items, 1, budget_bytes=budget, want_masks=True)
    finally:
        del gpu.stat_fish_packed
    assert len(calls) >= 3 and sum(calls) == len(items)
    for k, (g, item) in enumerate(zip(got, items)):
        assert_same(g, chain(gpu, item, 1), 'item %d' % k)


# ---- make stat_fish ---------------------------------------------------------------------------------------------------------------
def _tree(root):
    out = {}
    for d, _, files in os.walk(root):
        for f in files:
            if not f.startswith('config_'):                  # (the copy of config.yaml differs by the batch key it holds)
                out[os.path.relpath(os.path.join(d, f), root)] = open(os.path.join(d, f), 'rb').read()
    return out


@pytest.mark.parametrize('extra', [dict(), dict(use_min_cut=True), dict(scale='auto'), dict(tiff_read_on_device=True, tiff_read_batch=4)],
                         ids=['plain', 'min_cut', 'scale_auto', 'read_batch_4'])
def test_make_stat_fish_writes_the_same_tree_at_batch_1_2_and_8(gpu, tmp_path, monkeypatch, capsys, extra):
    from ecseg_amd import stat_fish as sf
    trees, outs = [], []
    for batch in (1, 2, 8):
        work = tmp_path / ('b%d' % batch)
        inp = work / 'in'
        (inp / 'nuclei_masks').mkdir(parents=True)
        for k in range(6):
            img, mask = cases.full_size_scene(seed=20 + k)
            y0, x0 = 40 * k, 30 * k
            H, W = (150, 200) if k % 2 else (131, 173)
            image_io.write_tiff_rgb8(str(inp / ('img_%d.tif' % k)), np.ascontiguousarray(img[y0:y0 + H, x0:x0 + W]))
            image_io.write_tiff_gray8(str(inp / 'nuclei_masks' / ('img_%d.tif' % k)), np.ascontiguousarray(mask[y0:y0 + H, x0:x0 + W]))
        cfg = yaml.safe_load(open(os.path.join(ROOT, 'config.yaml')))
        cfg['stat_fish'].update(inpath='in', tiff_on_device=True, batch=batch, **extra)
        yaml.safe_dump(cfg, open(work / 'config.yaml', 'w'))
        monkeypatch.chdir(work)
        code = 0
        try:
            sf.main([], handle=gpu)
        except SystemExit as e:
            code = e.code
        assert code == 0
        outs.append(capsys.readouterr().out)
        trees.append(_tree(str(inp / 'annotated')))
    assert len(trees[0]) == 6 * 5 + (6 if extra.get('use_min_cut') else 0) + 2 and len(trees[0]['stat_fish_lsq.csv']) > 200
    for t, o in zip(trees[1:], outs[1:]):
        assert sorted(t) == sorted(trees[0])
        for name in t:
            assert t[name] == trees[0][name], name
        assert o == outs[0]
