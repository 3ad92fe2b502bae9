"""NuSeT's marker watershed and clean-up on the device (csrc/watershed_kernels.hip: ecseg_marker_watershed, ecseg_clean_nuclei)
against the numpy / scipy restatement (tests/watershed_ref.py, which tests/test_watershed.py ties to the reference's own outputs),
byte for byte: every case of tests/watershed_cases.py and its seeded range through both calls and every NUCLEI_SIZE_T of the
case; the host marker list on the device's own region records; one handle over calls of changing size; argument errors;
``NuSeT.segment`` against the restatement fed the device's own mask, scores and proposals; ``make stat_fish`` with
``nuset_weights`` against the same run reading that mask from a folder."""
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


@pytest.fixture(scope='module')
def golden():
    with np.load(os.path.join(HERE, 'golden', 'nuset_watershed.npz')) as z:
        return {k: z[k] for k in z.files}


def _same_mean(a, b):
    return (np.isnan(a) and np.isnan(b)) or a == b


@pytest.mark.parametrize('k', range(len(CASES)), ids=NAMES)
def test_clean_nuclei_equals_the_restatement(gpu, golden, k):
    ws = golden['ws_%d' % k]
    cl, mean = ref.clean_image(ws)
    for t in CASES[k]['sizes']:
        out, got_mean, got_cl = gpu.clean_nuclei(ws, t, want_cleaned=True)
        assert np.array_equal(got_cl, cl), t
        assert _same_mean(got_mean, mean), (got_mean, mean)
        assert out.dtype == np.uint8 and np.array_equal(out, ref.final_mask(cl, t)), t
        assert np.array_equal(out, golden['final_%d_%d' % (k, t)]), t


def test_clean_nuclei_on_the_raw_masks(gpu):
    """The masks themselves (before any watershed line) are inputs as good as any; bool arrays are taken too."""
    for c in CASES:
        out, mean = gpu.clean_nuclei(c['mask'].astype(bool), c['sizes'][-1])
        cl, want_mean = ref.clean_image(c['mask'])
        assert np.array_equal(out, ref.final_mask(cl, c['sizes'][-1])) and _same_mean(mean, want_mean), c['name']


def test_one_handle_over_changing_sizes(gpu, golden):
    big, tiny = NAMES.index('whole_image_160'), NAMES.index('size_threshold_at_area')
    first = gpu.clean_nuclei(golden['ws_%d' % big], 20)
    small = gpu.clean_nuclei(golden['ws_%d' % tiny], 22)
    again = gpu.clean_nuclei(golden['ws_%d' % big], 20)
    assert np.array_equal(first[0], again[0]) and first[1] == again[1]
    assert np.array_equal(small[0], golden['final_%d_22' % tiny])
    assert np.array_equal(first[0], ref.final_mask(ref.clean_image(golden['ws_%d' % big])[0], 20))


def test_argument_errors(gpu):
    m = np.ones((8, 8), np.uint8)
    out = np.empty_like(m)
    call = lambda *a: gpu.lib.ecseg_clean_nuclei(gpu.h, *a)
    ptr = _lib._ptr
    assert call(ptr(m), 8, 8, -1, ptr(out), None, None) == -1                 # ECSEG_E_INVALID
    assert call(None, 8, 8, 0, ptr(out), None, None) == -1
    assert call(ptr(m), 8, 8, 0, None, None, None) == -1
    assert call(ptr(m), 0, 8, 0, ptr(out), None, None) == -1
    assert call(ptr(m), 8, -3, 0, ptr(out), None, None) == -1
    assert call(ptr(m), 65536, 32768, 0, ptr(out), None, None) == -1          # 2^31 pixels: refused before anything is touched
    with pytest.raises(_lib.EcsegError):
        gpu.clean_nuclei(m, -5)
    with pytest.raises(ValueError):
        gpu.clean_nuclei(np.ones((2, 3, 4), np.uint8), 0)
    assert gpu.clean_nuclei(m, 0)[0].max() == 0              # the handle still works


# ---- the marker watershed -----------------------------------------------------------------------------------------------------
def _device_watershed(gpu, c):
    mk = nuset.watershed_markers(c['scores'], c['proposals'], c['mask'], c['min_score'], gpu)
    return c['mask'].copy() if mk is None else gpu.marker_watershed(c['mask'], *mk)


@pytest.mark.parametrize('k', range(len(CASES)), ids=NAMES)
def test_marker_watershed_equals_the_reference(gpu, golden, k):
    c = CASES[k]
    want = ref.marker_list(c['scores'], c['proposals'], c['mask'], c['min_score'])
    got = nuset.watershed_markers(c['scores'], c['proposals'], c['mask'], c['min_score'], gpu)    # the device's region records
    assert (want is None) == (got is None)
    if want is not None:
        assert all(np.array_equal(a, b) for a, b in zip(want, got))
    ws = _device_watershed(gpu, c)
    assert ws.dtype == np.uint8 and np.array_equal(ws, ref.watershed(c['scores'], c['proposals'], c['mask'], c['min_score']))
    assert np.array_equal(ws, golden['ws_%d' % k])


def test_more_regions_than_the_default_capacity(gpu):
    """4200 regions of 12 pixels each: ``nuclei_regions`` has to grow past its 4096 records, and every region gets its marker."""
    m = np.zeros((60 * 5, 70 * 6), np.uint8)
    for r in range(60):
        for c in range(70):
            m[5 * r:5 * r + 3, 6 * c:6 * c + 4] = 1
    scores, props = np.array([0.99], np.float32), np.array([[0, 0, 8, 8]], np.float32)       # one proposal, in the edge
    want = ref.marker_list(scores, props, m, 0.9)
    got = nuset.watershed_markers(scores, props, m, 0.9, gpu)
    assert len(want[0]) == 4200 and all(np.array_equal(a, b) for a, b in zip(want, got))
    assert np.array_equal(gpu.marker_watershed(m, *got), ref.watershed_from_markers(m, *want))


def test_marker_watershed_one_handle_over_changing_sizes(gpu, golden):
    big, tiny = CASES[NAMES.index('whole_image_160')], CASES[NAMES.index('two_discs')]
    first = _device_watershed(gpu, big)
    small = _device_watershed(gpu, tiny)
    again = _device_watershed(gpu, big)
    assert np.array_equal(first, again) and np.array_equal(first, golden['ws_%d' % NAMES.index('whole_image_160')])
    assert np.array_equal(small, golden['ws_%d' % NAMES.index('two_discs')])


def test_marker_watershed_labels_and_order(gpu):
    """Arbitrary labels: the dilation takes the maximum LABEL, and a later entry on the same pixel replaces an earlier one."""
    c = CASES[NAMES.index('rectangle_three_markers')]
    r, cc, _ = ref.marker_list(c['scores'], c['proposals'], c['mask'], c['min_score'])
    for labels in ([7, 3, 900000], [5, 5, 1]):
        l = np.asarray(labels, np.int32)
        assert np.array_equal(gpu.marker_watershed(c['mask'], r, cc, l), ref.watershed_from_markers(c['mask'], r, cc, l)), labels
    r2, c2, l2 = np.append(r, r[0]).astype(np.int32), np.append(cc, cc[0]).astype(np.int32), np.array([1, 2, 3, 9], np.int32)
    assert np.array_equal(gpu.marker_watershed(c['mask'], r2, c2, l2), ref.watershed_from_markers(c['mask'], r2, c2, l2))
    # a later entry with a SMALLER label on the shared pixel (9 over 1 above: "the last wins" and "the largest wins" agree there).  The
    # The second marker lies four columns beside the first: the discs overlap, and the overlap goes to 5 (over 2) or to 8 (had 8 stayed).
    r3, c3 = np.array([r[0]] * 3, np.int32), np.array([cc[0], cc[0] + 4, cc[0]], np.int32)
    l3 = np.array([8, 5, 2], np.int32)
    want = ref.watershed_from_markers(c['mask'], r3, c3, l3)
    assert not np.array_equal(want, ref.watershed_from_markers(c['mask'], r3[:2], c3[:2], l3[:2]))      # 8 on the shared pixel moves the line
    assert np.array_equal(gpu.marker_watershed(c['mask'], r3, c3, l3), want)
    assert gpu.marker_watershed(c['mask'], [], [], []).max() == 0            # no marker: nothing is flooded


def test_marker_watershed_argument_errors(gpu):
    m = np.ones((8, 8), np.uint8)
    out = np.empty_like(m)
    one = lambda v: np.array([v], np.int32)
    ptr = _lib._ptr
    call = lambda mask, H, W, r, c, l, n, o: gpu.lib.ecseg_marker_watershed(gpu.h, mask, H, W, r, c, l, n, o)
    ok = (ptr(one(1)), ptr(one(1)), ptr(one(1)))
    assert call(None, 8, 8, *ok, 1, ptr(out)) == -1
    assert call(ptr(m), 8, 8, *ok, 1, None) == -1
    assert call(ptr(m), 0, 8, *ok, 1, ptr(out)) == -1
    assert call(ptr(m), 8, 16385, *ok, 1, ptr(out)) == -1
    assert call(ptr(m), 8, 8, *ok, -1, ptr(out)) == -1
    assert call(ptr(m), 8, 8, *ok, 1 << 31, ptr(out)) == -1
    assert call(ptr(m), 8, 8, None, ok[1], ok[2], 1, ptr(out)) == -1
    assert call(ptr(m), 8, 8, ptr(one(8)), ok[1], ok[2], 1, ptr(out)) == -1       # row == H
    assert call(ptr(m), 8, 8, ok[0], ptr(one(-1)), ok[2], 1, ptr(out)) == -1      # column < 0
    assert call(ptr(m), 8, 8, ok[0], ok[1], ptr(one(0)), 1, ptr(out)) == -1       # label < 1
    with pytest.raises(_lib.EcsegError):
        gpu.marker_watershed(m, [9], [1], [1])
    with pytest.raises(ValueError):
        gpu.marker_watershed(m, [1, 2], [1], [1])
    assert np.array_equal(gpu.marker_watershed(m, [3], [3], [1]), m)             # the handle still works


def test_integer_masks_are_taken(gpu):
    c = CASES[NAMES.index('two_discs')]
    ws = ref.watershed(c['scores'], c['proposals'], c['mask'], c['min_score'])  # int32, as the reference returns it
    assert ws.dtype == np.int32
    assert np.array_equal(gpu.clean_nuclei(ws, 20)[0], ref.final_mask(ref.clean_image(ws)[0], 20))
    mk = ref.marker_list(c['scores'], c['proposals'], c['mask'], c['min_score'])
    assert np.array_equal(gpu.marker_watershed(c['mask'].astype(np.int64) * 7, *mk), ws)
    with pytest.raises(TypeError):
        gpu.clean_nuclei(ws.astype(np.float32), 0)


# ---- NuSeT.segment and make stat_fish ------------------------------------------------------------------------------------------
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


@pytest.mark.parametrize('h,w', [(64, 96), (96, 128)])
def test_segment_equals_the_restatement_on_the_device_outputs(gpu, weights, h, w):
    net = nuset.NuSeT(weights, BASE, handle=gpu)
    img = _raw_image(h + 5, w + 3, h)                        # cropped to multiples of 16
    for min_score, size_t in ((0.5, 0), (0.7, 12)):
        got = net.segment(img, min_score, 0.1, size_t)
        m, scores, proposals = net.nuclei_masks(img, min_score, 0.1)
        print('segment %d x %d: %d foreground pixels, %d proposals above %.2f' % (h, w, int(m.sum()), len(scores), min_score))
        assert got.shape == (h, w) and got.dtype == np.uint8
        assert np.array_equal(got, ref.segment_tail(scores, proposals, m, min_score, size_t))


def test_make_stat_fish_with_nuset_weights_equals_the_mask_folder_run(gpu, weights, tmp_path, monkeypatch):
    import yaml
    from PIL import Image
    from ecseg_amd import image_io
    npz = {}
    for name, arrs in weights.items():
        for part, a in zip(('kernel', 'bias'), arrs):
            npz['%s/%s' % (nuset.CHECKPOINT_SCOPE[name], part)] = a
    np.savez(str(tmp_path / 'w.npz'), **npz)
    (tmp_path / 'src').mkdir()
    yaml.safe_dump({'min_score': 0.5, 'nms_threshold': 0.1}, open(tmp_path / 'src' / 'stat_fish_params.yaml', 'w'))
    net = nuset.NuSeT(weights, BASE, handle=gpu)
    runs = {}
    for run in ('nuset', 'folder'):
        inp = tmp_path / run
        (inp / 'masks').mkdir(parents=True)
        for k, name in enumerate(('a_img', 'b_img')):
            rgb = np.dstack([_raw_image(96, 128, 50 + 3 * k + j) for j in range(3)])
            Image.fromarray(rgb).save(str(inp / (name + '.tif')), compression='tiff_lzw')
            if run == 'folder':
                I, (blue, _, _) = sf.read_image(str(inp / (name + '.tif')), gpu)
                image_io.write_tiff_gray8(str(inp / 'masks' / (name + '.tif')), net.segment(I[:, :, blue], 0.5, 0.1, 10))
        cfg = dict(inpath=str(inp), scale=1, use_min_cut=False, nuclei_size_T=10, masks=str(inp / 'masks'))
        if run == 'nuset':
            cfg.update(nuset_weights=[str(tmp_path / 'w.npz')], nuset_base=BASE)
        yaml.safe_dump({'stat_fish': cfg}, open(tmp_path / 'config.yaml', 'w'))
        monkeypatch.chdir(tmp_path)
        sf.main([], handle=gpu)
        files = {}
        for root, _, names in os.walk(str(inp / 'annotated')):
            for f in names:
                if not f.startswith('config_'):
                    files[os.path.relpath(os.path.join(root, f), str(inp / 'annotated'))] = open(os.path.join(root, f), 'rb').read()
        runs[run] = files
    assert sorted(runs['nuset']) == sorted(runs['folder']) and len(runs['nuset']) >= 2 + 2 * 5
    for f in runs['nuset']:
        assert runs['nuset'][f] == runs['folder'][f], f
