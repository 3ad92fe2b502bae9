"""The batched marker watershed without a GPU: the two new symbols and the arena arithmetic of ecseg_marker_watershed_batch_bytes
against a layout written out by hand; ``Handle.marker_watershed_batch``'s packing, ``None`` entries and chunking by the byte budget
on a handle whose device call is the restatement (tests/watershed_ref.py) per image; ``NuSeT.segment_many`` against
``[segment(...)]`` on an oracle-backed handle; ``make stat_fish`` with ``nuset_batch: 3`` against ``nuset_batch: 1``, file by file."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import yaml

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import rescale_ref                           # noqa: E402
import test_nuset as tn                      # noqa: E402
import test_stat_fish as tsf                 # noqa: E402
import watershed_cases as cases              # noqa: E402
import watershed_ref as ref                  # noqa: E402

from ecseg_amd import _lib, nuset            # noqa: E402
from ecseg_amd import stat_fish as sf        # noqa: E402

BASE = 8


# ---- the symbols and the arena arithmetic ---------------------------------------------------------------------------------------
def _slot(nbytes):
    """One slot of the carver (csrc/scratch.h): rounded up to 256 bytes, and 256 bytes when empty."""
    return (nbytes + 255) // 256 * 256 if nbytes else 256


def _by_hand(span, n_images, n_markers, heap):
    """mask, out, work, filled (1 byte per packed byte); idx, rw, g, d2, lab, par, sz (4); 4 int32 flags and one 40-byte table row per
    image; rows, cols, labels (4 bytes per entry); heap keys and payloads (8 bytes per element each)."""
    return (4 * _slot(span) + 7 * _slot(4 * span) + _slot(16 * n_images) + _slot(40 * n_images) + 3 * _slot(4 * n_markers) +
            2 * _slot(8 * heap))


def _bytes(images, foreground):
    lib = _lib.load_library()
    tab = np.ascontiguousarray(images, np.int64).reshape(-1, 5)
    fg = np.ascontiguousarray(foreground, np.int64)
    return lib.ecseg_marker_watershed_batch_bytes(_lib._ptr(tab) if len(tab) else None, len(tab), _lib._ptr(fg) if len(fg) else None)


def test_symbols_and_arena_bytes_by_hand():
    lib = _lib.load_library()
    assert hasattr(lib, 'ecseg_marker_watershed_batch') and hasattr(lib, 'ecseg_marker_watershed_batch_bytes')
    assert {'ecseg_marker_watershed_batch', 'ecseg_marker_watershed_batch_bytes'} <= set(_lib.EXPORTS)
    header = open(os.path.join(HERE, '..', 'include', 'ecseg_hip.h')).read()
    assert '#define ECSEG_WATERSHED_BATCH_MAX_IMAGES 1024' in header and _lib.Handle.WATERSHED_BATCH_MAX_IMAGES == 1024
    assert 'int ecseg_marker_watershed_batch(ecseg_ctx* h, const uint8_t* masks, long long mask_bytes, const int64_t* images, int n_images,' in header
    assert 'long long ecseg_marker_watershed_batch_bytes(const int64_t* images, int n_images, const long long* foreground);' in header
    # 41 x 43 = 1763 bytes, then 64 x 96 = 6144 from the odd offset 1763: 7907 bytes; 3 + 2 markers; heaps 5 * 500 + 1 and 5 * 3000 + 1
    two = [[0, 41, 43, 0, 3], [1763, 64, 96, 3, 2]]
    want = _by_hand(7907, 2, 5, 2501 + 15001)
    assert want == 4 * 7936 + 7 * 31744 + 256 + 256 + 3 * 256 + 2 * 140032 == 535296
    assert _bytes(two, [500, 3000]) == want
    assert _bytes(np.zeros((0, 5)), []) == 0                                               # the empty batch asks for nothing
    assert _bytes([[0, 48, 64, 0, 0]], [0]) == _by_hand(3072, 1, 0, 1) == 4 * 3072 + 7 * 12288 + 7 * 256      # seven more slots: flags, table, three empty lists, a heap of one
    assert _bytes([[10, 41, 43, 0, 0]], [7]) == _by_hand(1773, 1, 0, 36)                   # a gap in front counts
    # what the call refuses has no size
    assert _bytes([[0, 41, 43, 0, 0], [1762, 8, 8, 0, 0]], [0, 0]) == -1                   # overlap
    assert _bytes([[0, 0, 43, 0, 0]], [0]) == -1 and _bytes([[0, 41, 16385, 0, 0]], [0]) == -1
    assert _bytes([[0, 41, 43, 0, 0]], [1764]) == -1 and _bytes([[0, 41, 43, -1, 2]], [0]) == -1
    assert lib.ecseg_marker_watershed_batch_bytes(None, 1, None) == -1
    assert lib.ecseg_marker_watershed_batch_bytes(_lib._ptr(np.zeros((1025, 5), np.int64)), 1025, _lib._ptr(np.zeros(1025, np.int64))) == -1


# ---- Handle.marker_watershed_batch on a handle whose device call is the restatement ----------------------------------------------
class PackedRefHandle(_lib.Handle):
    """The binding's own packing and chunking (and the library's host arithmetic), with ecseg_marker_watershed_batch replaced by
    tests/watershed_ref.py per table row; every call's table is kept."""

    def __init__(self):                                      # no device is opened
        self.lib, self.h, self.tables = _lib.load_library(), None, []

    def marker_watershed_packed(self, masks, images, rows, cols, labels):
        tab = np.asarray(images, np.int64).reshape(-1, 5)
        self.tables.append(tab.copy())
        out = np.zeros(masks.size, np.uint8)
        end = 0
        for off, H, W, first, n in tab.tolist():
            assert off >= end
            end = off + H * W
            sl = slice(first, first + n)
            m = masks[off:end].reshape(H, W)
            out[off:end] = ref.watershed_from_markers(m, rows[sl], cols[sl], labels[sl]).astype(np.uint8).reshape(-1)
        assert end <= masks.size and len(rows) == len(cols) == len(labels)
        return out


@pytest.fixture(scope='module')
def some_cases():
    """Seven small cases with their marker lists and the restatement's answers; one has no marker list at all."""
    names = ['two_discs', 'scores_empty', 'rectangle_three_markers', 'ring_with_core', 'marker_on_background', 'diagonal_blobs', 'half_centres']
    by_name = {c['name']: c for c in cases.fixed_cases()}
    picked = [by_name[n] for n in names] + [cases.random_case(3, max_extent=60)]
    masks = [c['mask'] for c in picked]
    markers = [ref.marker_list(c['scores'], c['proposals'], c['mask'], c['min_score']) for c in picked]
    want = [c['mask'] if mk is None else ref.watershed_from_markers(c['mask'], *mk).astype(np.uint8) for c, mk in zip(picked, markers)]
    assert markers[1] is None and sum(mk is None for mk in markers) == 1 and len({m.shape for m in masks}) > 1
    return masks, markers, want


def test_batch_packs_skips_none_and_unpacks(some_cases):
    masks, markers, want = some_cases
    h = PackedRefHandle()
    got = h.marker_watershed_batch(masks, markers)
    assert len(h.tables) == 1 and len(h.tables[0]) == len(masks) - 1                       # the None entry did not go to the device
    assert got[1] is masks[1]                                                             # ... and comes back as it is
    for g, w in zip(got, want):
        assert g.dtype == np.uint8 and g.shape == w.shape and np.array_equal(g, w)
    tab = h.tables[0]
    sizes = [m.size for m, mk in zip(masks, markers) if mk is not None]
    assert tab[:, 0].tolist() == np.concatenate([[0], np.cumsum(sizes)[:-1]]).tolist()    # back to back
    counts = [len(mk[0]) for mk in markers if mk is not None]
    assert tab[:, 4].tolist() == counts and tab[:, 3].tolist() == np.concatenate([[0], np.cumsum(counts)[:-1]]).tolist()
    assert h.marker_watershed_batch([], []) == [] and len(h.tables) == 1                   # nothing to do: no call
    assert h.marker_watershed_batch([masks[1]], [None])[0] is masks[1] and len(h.tables) == 1
    with pytest.raises(ValueError):
        h.marker_watershed_batch(masks, markers[:-1])
    with pytest.raises(ValueError):
        h.marker_watershed_batch([masks[0]], [([1, 2], [1], [1])])
    with pytest.raises(TypeError):
        h.marker_watershed_batch([masks[0].astype(np.float32)], [markers[0]])


def test_chunking_by_the_byte_budget_gives_the_same_list(some_cases):
    masks, markers, want = some_cases
    sent = [(m, mk) for m, mk in zip(masks, markers) if mk is not None]
    need = [_bytes([[0, m.shape[0], m.shape[1], 0, len(mk[0])]], [int(np.count_nonzero(m))]) for m, mk in sent]
    whole = PackedRefHandle()
    whole.marker_watershed_batch(masks, markers)
    tab = whole.tables[0]
    total = _bytes(tab, [int(np.count_nonzero(m)) for m, _ in sent])
    budget = total * 2 // 5                                   # more than any one image, less than half of all: three calls or more
    assert max(need) <= budget
    h = PackedRefHandle()
    got = h.marker_watershed_batch(masks, markers, budget_bytes=budget)
    assert len(h.tables) >= 3 and sum(len(t) for t in h.tables) == len(sent)
    lo = 0
    for t in h.tables:                                        # every call within the budget, every table starting at 0
        fg = [int(np.count_nonzero(m)) for m, _ in sent[lo:lo + len(t)]]
        assert t[0, 0] == 0 and t[0, 3] == 0 and _bytes(t, fg) <= budget
        lo += len(t)
    assert all(np.array_equal(g, w) for g, w in zip(got, want))
    # a budget below every image: one image per call, still the same list
    one = PackedRefHandle()
    got = one.marker_watershed_batch(masks, markers, budget_bytes=1)
    assert [len(t) for t in one.tables] == [1] * len(sent) and all(np.array_equal(g, w) for g, w in zip(got, want))


# ---- NuSeT.segment_many on an oracle-backed handle -------------------------------------------------------------------------------
class FakeHandle(tn.OracleHandle, tsf.OracleHandle):
    """``tests/test_nuset.py``'s oracle-backed handle plus the calls behind the network by the restatements, the calls of ``make
    stat_fish`` by tests/test_stat_fish.py's handle, and ``marker_watershed_batch`` = the restatement per image.  The network's
    outputs are kept per input, since every comparison here runs the same images twice."""

    def __init__(self, weights, base):
        tn.OracleHandle.__init__(self, weights, base)
        tsf.OracleHandle.__init__(self)
        self.seen, self.single, self.batches = {}, 0, []

    def outputs(self, x):
        key = (x.shape, x.tobytes())
        if key not in self.seen:
            self.seen[key] = tn.OracleHandle.outputs(self, x)
        return self.seen[key]

    def marker_watershed(self, mask, rows, cols, labels):
        self.single += 1
        return ref.watershed_from_markers(mask, rows, cols, labels).astype(np.uint8)

    def marker_watershed_batch(self, masks, markers):
        self.batches.append(len(masks))
        return [m if mk is None else ref.watershed_from_markers(m, *mk).astype(np.uint8) for m, mk in zip(masks, markers)]

    def clean_nuclei(self, mask, nuclei_size_T, want_cleaned=False):
        cl, mean = ref.clean_image(mask)
        out = ref.final_mask(cl, nuclei_size_T)
        return (out, mean, cl) if want_cleaned else (out, mean)

    def rescale_down(self, image, scale):
        return rescale_ref.rescale_down(image, scale)

    def rescale_mask_up(self, cleaned, scale, nuclei_size_T):
        return rescale_ref.rescale_mask_up(cleaned, scale, nuclei_size_T)


def _raw_image(h, w, seed, n=5):
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[:h, :w]
    img = rng.normal(20.0, 4.0, (h, w))
    for _ in range(n):
        cy, cx, r = rng.uniform(0, h), rng.uniform(0, w), rng.uniform(4, 9)
        img += 150.0 * np.exp(-((yy - cy) ** 2 + (xx - cx) ** 2) / (2 * r * r))
    return np.clip(img, 0, 255).astype(np.uint8)


@pytest.fixture(scope='module')
def weights():
    return nuset.synth_weights(nuset.nuset_config(16, 16, BASE), seed=21)


def _same(a, b):
    if isinstance(a, Exception) or isinstance(b, Exception):
        return type(a) is type(b) and str(a) == str(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b)


def _segment_or_error(net, im, *args, **kw):
    try:
        return net.segment(im, *args, **kw)
    except ValueError as e:
        return e


def test_segment_many_equals_segment_per_image(weights):
    h = FakeHandle(weights, BASE)
    net = nuset.NuSeT(weights, BASE, handle=h)
    dark = np.zeros((50, 70), np.uint8)
    images = [_raw_image(69, 99, 1), _raw_image(48, 64, 2), dark, _raw_image(69, 99, 3), _raw_image(64, 48, 4)]
    m1 = net.mask(nuset.whole_image_norm(dark[:48, :64]))
    if m1.any():                                             # the image "whose first mask is empty": make it so whatever the seeded net says of zeros
        pytest.fail('the seeded network marks pixels of an all-zero image: pick another dark image')
    args = (0.5, 0.1, 12)
    want = [_segment_or_error(net, im, *args) for im in images]
    singles = h.single
    got = net.segment_many(images, *args)
    assert h.single == singles and h.batches == [len(images)]                              # ONE batched call, no single one
    assert len(got) == len(want) and all(_same(g, w) for g, w in zip(got, want))
    assert [g.shape for g in got] == [(64, 96), (48, 64), (48, 64), (64, 96), (64, 48)] and not got[2].any()
    assert sum(int(g.any()) for g in got) >= 2                                             # (something was segmented)
    # scale_ratio 0.3: 48 x 64 becomes 14 x 19, below 16 x 16 - its error stands in its place, the neighbours are intact
    big = [_raw_image(120, 150, 5, 9), images[1], _raw_image(110, 160, 6, 9)]
    want = [_segment_or_error(net, im, *args, scale_ratio=0.3) for im in big]
    h.batches = []
    got = net.segment_many(big, *args, scale_ratio=0.3)
    assert isinstance(got[1], ValueError) and '16 x 16' in str(got[1]) and h.batches == [2]
    assert all(_same(g, w) for g, w in zip(got, want)) and got[0].dtype == np.uint8 and got[0].shape == want[0].shape
    assert net.segment_many([], *args) == []
    for s in (0, 1.5, -1):
        with pytest.raises(ValueError, match='scale_ratio'):
            net.segment_many(images, *args, scale_ratio=s)


# ---- make stat_fish with nuset_batch -----------------------------------------------------------------------------------------------
def _scenes(tmp_path, run, weights, **section):
    from PIL import Image
    inp = tmp_path / run / 'in'
    inp.mkdir(parents=True)
    np.savez(str(tmp_path / run / 'w.npz'),
             **{'%s/%s' % (nuset.CHECKPOINT_SCOPE[n], part): a for n, arrs in weights.items() for part, a in zip(('kernel', 'bias'), arrs)})
    for k, name in enumerate('abcdefg'):                     # 7 scenes: `c` cannot be read, `e` has another extent
        h, w = (64, 80) if name == 'e' else (48, 64)
        rgb = np.dstack([_raw_image(h, w, 30 + 3 * k + j) for j in range(3)])
        Image.fromarray(rgb).save(str(inp / ('img_%s.tif' % name)), compression='tiff_lzw')
    (inp / 'img_c.tif').write_bytes(b'II*\0garbage')
    (tmp_path / run / 'src').mkdir()
    yaml.safe_dump({'min_score': 0.5, 'nms_threshold': 0.1}, open(tmp_path / run / 'src' / 'stat_fish_params.yaml', 'w'))
    cfg = dict(inpath=str(inp), scale=1, use_min_cut=False, nuclei_size_T=10, nuset_weights=[str(tmp_path / run / 'w.npz')], nuset_base=BASE)
    cfg.update(section)
    yaml.safe_dump({'stat_fish': cfg}, open(tmp_path / run / 'config.yaml', 'w'))
    return inp


def _tree(root):
    out = {}
    for d, _, names in os.walk(str(root)):
        for f in names:
            if not f.startswith('config_'):
                out[os.path.relpath(os.path.join(d, f), str(root))] = open(os.path.join(d, f), 'rb').read()
    return out


def test_make_stat_fish_nuset_batch_3_equals_1(tmp_path, monkeypatch, capsys, weights):
    h = FakeHandle(weights, BASE)                            # one handle: the second run finds the network's outputs of the first
    runs = {}
    for run, section in (('one', {'nuset_batch': 1}), ('three', {'nuset_batch': 3}), ('absent', {})):
        inp = _scenes(tmp_path, run, weights, **section)
        monkeypatch.chdir(tmp_path / run)
        h.single, h.batches = 0, []
        with pytest.raises(SystemExit) as e:
            sf.main([], handle=h)
        runs[run] = (e.value.code, capsys.readouterr().out.replace(str(tmp_path / run), ''), _tree(inp / 'annotated'), h.single, h.batches)
    code, text, tree, single, batches = runs['one']
    assert code == 1 and '1 image(s) were NOT processed' in text and 'img_c.tif' in text.split('NOT processed')[1]
    assert batches == [] and len(tree) == 2 + 6 * 5 and 'stat_fish_lsq.csv' in tree
    assert runs['absent'][:3] == runs['one'][:3] and runs['absent'][4] == []              # the key absent: today's loop
    code3, text3, tree3, single3, batches3 = runs['three']
    assert single3 == 0 and batches3 == [2, 3, 1]            # (a, b, [c unreadable]), (d, e, f), (g)
    assert code3 == code and text3 == text                   # the Processing order and the failure report
    assert sorted(tree3) == sorted(tree)
    for f in tree:
        assert tree3[f] == tree[f], f
    assert tree['stat_fish_lsq.csv'].count(b'\n') >= 2       # header and at least one nucleus: the comparison is not of empty files


@pytest.mark.parametrize('value', [0, -1, 1.5, True, 'a'])
def test_a_bad_nuset_batch_exits_with_code_2(tmp_path, monkeypatch, capsys, weights, value):
    inp = _scenes(tmp_path, 'bad', weights, nuset_batch=value)
    monkeypatch.chdir(tmp_path / 'bad')
    with pytest.raises(SystemExit) as e:
        sf.main([], handle=FakeHandle(weights, BASE))
    assert e.value.code == 2 and 'nuset_batch' in capsys.readouterr().out
    assert not [d for d in os.listdir(inp) if d.startswith(('tmp_', 'annotated'))]


def test_nuset_batch_is_ignored_without_weights_and_needs_the_batched_call(tmp_path, monkeypatch, capsys, weights):
    tsf._folder(tmp_path, nuset_batch='a')                   # the mask folder is read: the key is not looked at
    monkeypatch.chdir(tmp_path)
    sf.main([], handle=tsf.OracleHandle())
    assert os.path.exists(tmp_path / 'in' / 'annotated' / 'stat_fish_lsq.csv')

    class NoBatch(FakeHandle):
        marker_watershed_batch = property()                  # hasattr() is False
    _scenes(tmp_path, 'nobatch', weights, nuset_batch=2)
    monkeypatch.chdir(tmp_path / 'nobatch')
    with pytest.raises(SystemExit) as e:
        sf.main([], handle=NoBatch(weights, BASE))
    assert e.value.code == 2 and 'marker_watershed_batch' in capsys.readouterr().out
    assert C.sizeof(C.c_longlong) == 8                       # (the int64 table and the long long counts of the binding are one type)
