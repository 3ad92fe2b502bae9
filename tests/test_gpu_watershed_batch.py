"""The batched marker watershed on the device (ecseg_marker_watershed_batch: one flood wave per image, every other stage on a grid
whose second axis is the image) against the reference's own outputs (tests/golden/nuset_watershed.npz) and against the single-image
call on the same handle, byte for byte: every case of tests/watershed_cases.py in ONE batch, with gaps between the images; the same
list reversed and rotated; the shapes at which the grid or the per-image state could go wrong; repeated calls and arena reuse;
argument errors; ``NuSeT.segment_many`` against ``segment``; ``make stat_fish`` with ``nuset_batch: 4`` against ``nuset_batch: 1``."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import watershed_cases as cases              # noqa: E402
import watershed_ref as ref                  # noqa: E402

from ecseg_amd import _lib, nuset            # noqa: E402
from ecseg_amd import stat_fish as sf        # noqa: E402

pytestmark = pytest.mark.gpu
CASES = cases.all_cases()
NAMES = [c['name'] for c in CASES]
INVALID = -1                                 # ECSEG_E_INVALID


@pytest.fixture(scope='module')
def golden():
    with np.load(os.path.join(HERE, 'golden', 'nuset_watershed.npz')) as z:
        return [z['ws_%d' % k].astype(np.uint8) for k in range(len(CASES))]


@pytest.fixture(scope='module')
def markers():
    """Per case the marker list of the restatement (tests/test_gpu_watershed.py ties the device's own list to it), None for the two
    early branches."""
    return [ref.marker_list(c['scores'], c['proposals'], c['mask'], c['min_score']) for c in CASES]


def _pack(masks, marker_lists, gaps=None):
    """-> (buffer, table, rows, cols, labels): image k starts ``gaps[k]`` bytes behind the end of the one in front; the bytes in the gaps
    are 1, so that a kernel reading them as mask would show."""
    gaps = gaps if gaps is not None else [0] * len(masks)
    tab = np.zeros((len(masks), 5), np.int64)
    off = first = 0
    for k, (m, mk) in enumerate(zip(masks, marker_lists)):
        off += gaps[k]
        tab[k] = (off, m.shape[0], m.shape[1], first, len(mk[0]))
        off += m.size
        first += len(mk[0])
    buf = np.ones(off + 5, np.uint8)                         # five more bytes behind the last image
    for row, m in zip(tab, masks):
        buf[row[0]:row[0] + m.size] = m.reshape(-1)
    cat = lambda j: np.concatenate([np.asarray(mk[j], np.int32).reshape(-1) for mk in marker_lists] + [np.zeros(0, np.int32)])
    return buf, tab, cat(0), cat(1), cat(2)


def _unpack(out, tab):
    return [out[o:o + H * W].reshape(H, W) for o, H, W, _, _ in tab.tolist()]


def _outside(out, tab):
    keep = np.ones(out.size, bool)
    for o, H, W, _, _ in tab.tolist():
        keep[o:o + H * W] = False
    return out[keep]


NONE = (np.zeros(0, np.int32),) * 3


@pytest.fixture(scope='module')
def everything(gpu, markers):
    """ALL cases in ONE call, gaps of 0 .. 3 bytes between them; a case without a marker list goes in with no marker."""
    masks = [c['mask'] for c in CASES]
    lists = [mk if mk is not None else NONE for mk in markers]
    gaps = [(3 * k) % 4 for k in range(len(masks))]
    buf, tab, r, c, l = _pack(masks, lists, gaps)
    out = gpu.marker_watershed_packed(buf, tab, r, c, l)
    return masks, lists, tab, out


def test_every_case_in_one_batch_equals_the_reference_and_the_single_call(gpu, golden, markers, everything):
    masks, lists, tab, out = everything
    assert len(tab) == len(CASES) == 28 + 40 + 3 and out.dtype == np.uint8 and out.size == tab[-1, 0] + masks[-1].size + 5
    assert len({m.shape for m in masks}) > 30 and any(o % 2 for o in tab[:, 0].tolist()) and any(o % 8 for o in tab[:, 0].tolist())
    assert sum(mk is None for mk in markers) >= 2 and any(not m.any() for m in masks) and any(m.all() for m in masks)
    got = _unpack(out, tab)
    for k, (g, mk) in enumerate(zip(got, markers)):
        if mk is None:
            assert not g.any(), NAMES[k]                     # no marker: nothing is flooded
        else:
            assert np.array_equal(g, golden[k]), NAMES[k]
            assert np.array_equal(g, gpu.marker_watershed(masks[k], *mk)), NAMES[k]
    assert not _outside(out, tab).any()                      # the gaps (which held 1) and the tail are 0
    # the binding: None entries stay as they are, and then EVERY case equals the reference's _watershed
    through = gpu.marker_watershed_batch(masks, markers)
    assert len(through) == len(CASES)
    for k, g in enumerate(through):
        assert g.dtype == np.uint8 and np.array_equal(g, golden[k]), NAMES[k]


@pytest.mark.parametrize('order', ['reversed', 'rotated'])
def test_the_order_of_the_images_does_not_show(gpu, everything, order):
    masks, lists, tab, out = everything
    n = len(masks)
    perm = list(range(n))[::-1] if order == 'reversed' else list(range(1, n)) + [0]
    buf, tab2, r, c, l = _pack([masks[k] for k in perm], [lists[k] for k in perm])
    got = _unpack(gpu.marker_watershed_packed(buf, tab2, r, c, l), tab2)
    want = _unpack(out, tab)
    for g, k in zip(got, perm):
        assert np.array_equal(g, want[k]), NAMES[k]


def test_a_batch_of_one(gpu, golden, markers):
    k = NAMES.index('ring_with_core')
    got = gpu.marker_watershed_batch([CASES[k]['mask']], [markers[k]])
    assert len(got) == 1 and np.array_equal(got[0], golden[k])


def test_more_images_than_compute_units(gpu, golden, markers):
    """300 copies of one 48 x 64 case and another image in the middle: 301 flood workgroups, more than the device has CUs."""
    a, b = NAMES.index('two_discs'), NAMES.index('random_5')
    ks = [a] * 150 + [b] + [a] * 150
    got = gpu.marker_watershed_batch([CASES[k]['mask'] for k in ks], [markers[k] for k in ks])
    assert len(got) == 301 and markers[a] is not None and markers[b] is not None and golden[a].any()
    for g, k in zip(got, ks):
        assert np.array_equal(g, golden[k])


def _disc_scene(H, W, centres, r):
    m = np.zeros((H, W), np.uint8)
    for cy, cx in centres:
        cases.disc(m, cy, cx, r)
    rows, cols = (np.array(v, np.int32) for v in zip(*centres))
    return m, (rows, cols, np.arange(1, len(centres) + 1, dtype=np.int32))


def test_a_short_image_beside_a_long_one(gpu):
    """41 x 43 = 1763 and 128 x 127 = 16256 pixels, neither a multiple of 64 or 256: the grid is the larger image's, and the smaller
    image's blocks past its end return; in either order."""
    small = _disc_scene(41, 43, [(15, 14), (22, 27)], 10)
    large = _disc_scene(128, 127, [(40, 40), (52, 70), (90, 60), (100, 110)], 21)
    want = [ref.watershed_from_markers(m, *mk).astype(np.uint8) for m, mk in (small, large)]
    assert all((w != m).any() and w.any() for w, (m, _) in zip(want, (small, large)))      # both have a watershed line
    for pair, ws in (((small, large), want), ((large, small), want[::-1])):
        got = gpu.marker_watershed_batch([p[0] for p in pair], [p[1] for p in pair])
        assert all(np.array_equal(g, w) for g, w in zip(got, ws))


def test_an_all_foreground_image_beside_others(gpu, golden, markers):
    """`filled` without a zero takes scipy's (-1, 0) branch: the flag is the image's own."""
    ks = [NAMES.index(n) for n in ('two_discs', 'whole_image_160', 'ring_with_hole', 'nearly_whole_image_160', 'whole_image_160')]
    assert CASES[ks[1]]['mask'].all() and not CASES[ks[3]]['mask'].all()
    got = gpu.marker_watershed_batch([CASES[k]['mask'] for k in ks], [markers[k] for k in ks])
    for g, k in zip(got, ks):
        assert np.array_equal(g, golden[k]), NAMES[k]


def test_two_calls_agree_and_the_single_call_still_works(gpu, golden, markers, everything):
    masks, lists, tab, out = everything
    buf, tab2, r, c, l = _pack(masks, lists, [(3 * k) % 4 for k in range(len(masks))])
    assert np.array_equal(tab, tab2)
    assert np.array_equal(gpu.marker_watershed_packed(buf, tab2, r, c, l), out)
    assert gpu.timings()['count'] > 0                        # the kernels' device time is reported
    for name in ('whole_image_160', 'two_discs'):            # a larger and a smaller need than the arena now holds
        k = NAMES.index(name)
        assert np.array_equal(gpu.marker_watershed(CASES[k]['mask'], *markers[k]), golden[k])
    assert np.array_equal(gpu.marker_watershed_packed(buf, tab2, r, c, l), out)


def test_argument_errors(gpu, golden, markers):
    k = NAMES.index('two_discs')
    m, mk = CASES[k]['mask'], markers[k]
    H, W = m.shape
    buf, tab, r, c, l = _pack([m, m], [mk, mk])
    out = np.empty_like(buf)
    ptr = _lib._ptr

    def call(tab, n=None, buf=buf, r=r, c=c, l=l, nbytes=None, n_markers=None, out=out):
        t = np.ascontiguousarray(tab, np.int64)
        return gpu.lib.ecseg_marker_watershed_batch(gpu.h, ptr(buf), buf.size if nbytes is None else nbytes, ptr(t), len(t) if n is None else n,
                                                    ptr(r), ptr(c), ptr(l), len(r) if n_markers is None else n_markers, ptr(out))

    def message():
        return gpu.lib.ecseg_last_error(gpu.h).decode()
    assert call(tab) == 0
    bad = tab.copy(); bad[1, 0] -= 1
    assert call(bad) == INVALID and 'image 1' in message() and 'overlap' in message()
    assert call(tab, nbytes=buf.size - 6) == INVALID and 'image 1' in message()            # the second image leaves mask_bytes
    bad = tab.copy(); bad[1, 0] += 6
    assert call(bad) == INVALID and 'image 1' in message()
    # a marker of image 0 outside it, but at a pixel the NEXT image has: row H + 3 of image 0 is row 3 of image 1
    r2 = r.copy(); r2[0] += H
    assert call(tab, r=r2) == INVALID and 'image 0' in message() and 'marker 0' in message()
    c2 = c.copy(); c2[len(mk[0])] = W
    assert call(tab, c=c2) == INVALID and 'image 1' in message() and 'marker %d' % len(mk[0]) in message()
    l2 = l.copy(); l2[1] = 0
    assert call(tab, l=l2) == INVALID and 'label' in message()
    bad = tab.copy(); bad[1, 4] += 1
    assert call(bad) == INVALID and 'lists' in message()                                    # a marker range leaving the lists
    big = np.zeros((1025, 5), np.int64); big[:, 1:3] = 1; big[:, 0] = np.arange(1025)
    assert call(big, buf=np.zeros(2000, np.uint8), out=np.zeros(2000, np.uint8), n_markers=0) == INVALID and '1024' in message()
    assert call(tab, n=-1) == INVALID
    for col, v in ((1, 0), (2, 16385), (1, -4)):
        bad = tab.copy(); bad[0, col] = v
        assert call(bad) == INVALID and 'extent' in message()
    assert gpu.lib.ecseg_marker_watershed_batch(gpu.h, None, buf.size, ptr(tab), 2, ptr(r), ptr(c), ptr(l), len(r), ptr(out)) == INVALID
    assert gpu.lib.ecseg_marker_watershed_batch(gpu.h, ptr(buf), buf.size, ptr(tab), 2, ptr(r), ptr(c), ptr(l), len(r), None) == INVALID
    assert gpu.lib.ecseg_marker_watershed_batch(gpu.h, ptr(buf), buf.size, ptr(tab), 2, None, ptr(c), ptr(l), len(r), ptr(out)) == INVALID
    assert gpu.lib.ecseg_marker_watershed_batch(gpu.h, None, 0, None, 0, None, None, None, 0, None) == 0       # an empty batch does nothing
    with pytest.raises(_lib.EcsegError):
        gpu.marker_watershed_batch([m], [([H], [1], [1])])
    got = gpu.marker_watershed_batch([m, m], [mk, mk])       # the handle still works
    assert np.array_equal(got[0], golden[k]) and np.array_equal(got[1], golden[k])


# ---- NuSeT.segment_many and make stat_fish -----------------------------------------------------------------------------------------
BASE = 8


def _raw_image(h, w, seed):
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[:h, :w]
    img = rng.normal(20.0, 4.0, (h, w))
    for _ in range(7):
        cy, cx, r = rng.uniform(0, h), rng.uniform(0, w), rng.uniform(4, 10)
        img += 150.0 * np.exp(-((yy - cy) ** 2 + (xx - cx) ** 2) / (2 * r * r))
    return np.clip(img, 0, 255).astype(np.uint8)


@pytest.fixture(scope='module')
def weights():
    return nuset.synth_weights(nuset.nuset_config(16, 16, BASE), seed=21)


@pytest.mark.parametrize('scale_ratio', [1, 0.5])
def test_segment_many_equals_segment(gpu, weights, scale_ratio):
    net = nuset.NuSeT(weights, BASE, handle=gpu)
    f = int(round(1 / scale_ratio))
    images = [_raw_image(f * h + 5, f * w + 3, 7 * h + w) for h, w in ((64, 96), (96, 128), (64, 96))]
    want = [net.segment(im, 0.5, 0.1, 12, scale_ratio=scale_ratio) for im in images]
    got = net.segment_many(images, 0.5, 0.1, 12, scale_ratio=scale_ratio)
    assert len(got) == 3 and any(w.any() for w in want)
    for g, w in zip(got, want):
        assert g.dtype == np.uint8 and g.shape == w.shape and np.array_equal(g, w)


def test_make_stat_fish_nuset_batch_4_equals_1(gpu, weights, tmp_path, monkeypatch):
    import yaml
    from PIL import Image
    np.savez(str(tmp_path / 'w.npz'),
             **{'%s/%s' % (nuset.CHECKPOINT_SCOPE[n], part): a for n, arrs in weights.items() for part, a in zip(('kernel', 'bias'), arrs)})
    (tmp_path / 'src').mkdir()
    yaml.safe_dump({'min_score': 0.5, 'nms_threshold': 0.1}, open(tmp_path / 'src' / 'stat_fish_params.yaml', 'w'))
    runs = {}
    for batch in (1, 4):
        inp = tmp_path / ('run%d' % batch)
        inp.mkdir()
        for k, name in enumerate('abcdef'):                  # 6 scenes in chunks of 4 and 2; `c` has another extent
            h, w = (96, 128) if name == 'c' else (64, 96)
            rgb = np.dstack([_raw_image(h, w, 50 + 3 * k + j) for j in range(3)])
            Image.fromarray(rgb).save(str(inp / ('img_%s.tif' % name)), compression='tiff_lzw')
        cfg = dict(inpath=str(inp), scale=1, use_min_cut=False, nuclei_size_T=10, nuset_weights=[str(tmp_path / 'w.npz')], nuset_base=BASE,
                   nuset_batch=batch)
        yaml.safe_dump({'stat_fish': cfg}, open(tmp_path / 'config.yaml', 'w'))
        monkeypatch.chdir(tmp_path)
        sf.main([], handle=gpu)
        files = {}
        for root, _, names in os.walk(str(inp / 'annotated')):
            for f in names:
                if not f.startswith('config_'):
                    files[os.path.relpath(os.path.join(root, f), str(inp / 'annotated'))] = open(os.path.join(root, f), 'rb').read()
        runs[batch] = files
    assert sorted(runs[4]) == sorted(runs[1]) and len(runs[1]) == 2 + 6 * 5
    for f in runs[1]:
        assert runs[4][f] == runs[1][f], f
