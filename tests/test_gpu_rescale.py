"""NuSeT's two ``rescale`` calls on the device (csrc/rescale_kernels.hip: ecseg_rescale_down, ecseg_rescale_mask_up) against
scikit-image 0.18.3's own outputs (tests/golden/nuset_rescale.npz) and the numpy restatement (tests/rescale_ref.py, which
tests/test_rescale.py ties to them): the Gaussian stage and the final masks byte for byte, the float64 image bit for bit against
the restatement and within twice the stored ``down_maxdiff`` of scikit-image's, on every case of tests/rescale_cases.py and its seeded
range; one handle over calls of changing size; identical bytes on a second call; argument errors; ``NuSeT.segment`` with a
``scale_ratio`` against the composition of the restatement and the device's own stages; ``make stat_fish`` with ``scale_ratio: 0.5``
against the same run reading that mask from a folder."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import rescale_cases as cases                # noqa: E402
import rescale_ref as ref                    # noqa: E402

from ecseg_amd import _lib, nuset            # noqa: E402
from ecseg_amd import stat_fish as sf        # noqa: E402

pytestmark = pytest.mark.gpu
DOWN, UP = cases.down_cases(), cases.up_cases()
DOWN_NAMES, UP_NAMES = [c['name'] for c in DOWN], [c['name'] for c in UP]


@pytest.fixture(scope='module')
def golden():
    with np.load(os.path.join(HERE, 'golden', 'nuset_rescale.npz')) as z:
        return {k: z[k] for k in z.files}


@pytest.mark.parametrize('k', range(len(DOWN)), ids=DOWN_NAMES)
def test_rescale_down_equals_golden_and_restatement(gpu, golden, k):
    c = DOWN[k]
    out, filtered = gpu.rescale_down(c['image'], c['scale'])
    want, want_f = ref.rescale_down(c['image'], c['scale'])
    assert filtered.dtype == np.uint8 and np.array_equal(filtered, golden['down_filtered_%d' % k])
    assert out.dtype == np.float64 and np.array_equal(out, want)                       # bit for bit
    diff = float(np.abs(out - golden['down_out_%d' % k]).max())
    print('%s: |device - golden| = %.3g (bound %.3g)' % (c['name'], diff, 2 * float(golden['down_maxdiff'])))
    assert diff <= 2 * float(golden['down_maxdiff'])


def test_rescale_down_on_the_seeded_range(gpu):
    for seed in cases.SEEDS:
        c = cases.random_down(seed)
        out, filtered = gpu.rescale_down(c['image'], c['scale'])
        want, want_f = ref.rescale_down(c['image'], c['scale'])
        assert np.array_equal(filtered, want_f) and np.array_equal(out, want), c['name']


@pytest.mark.parametrize('k', range(len(UP)), ids=UP_NAMES)
def test_rescale_mask_up_equals_golden(gpu, golden, k):
    c = UP[k]
    for t in c['sizes']:
        got = gpu.rescale_mask_up(c['mask'], c['scale'], t)
        assert got.dtype == np.uint8 and np.array_equal(got, golden['up_final_%d_%d' % (k, t)]), t


def test_rescale_mask_up_on_the_seeded_range(gpu):
    for seed in cases.SEEDS:
        c = cases.random_up(seed)
        for t in c['sizes']:
            assert np.array_equal(gpu.rescale_mask_up(c['mask'], c['scale'], t), ref.rescale_mask_up(c['mask'], c['scale'], t)), (c['name'], t)


def test_one_handle_over_changing_sizes_and_twice_the_same_bytes(gpu, golden):
    big, tiny = DOWN_NAMES.index('scene_203x331_s0.3'), DOWN_NAMES.index('scene_30x30_s0.7')
    first = gpu.rescale_down(DOWN[big]['image'], 0.3)
    small = gpu.rescale_down(DOWN[tiny]['image'], 0.7)
    again = gpu.rescale_down(DOWN[big]['image'], 0.3)
    assert first[0].tobytes() == again[0].tobytes() and first[1].tobytes() == again[1].tobytes()
    assert np.array_equal(small[1], golden['down_filtered_%d' % tiny]) and np.array_equal(first[1], golden['down_filtered_%d' % big])
    big, tiny = UP_NAMES.index('blobs_304x416'), UP_NAMES.index('lone_pixel')
    first = gpu.rescale_mask_up(UP[big]['mask'], UP[big]['scale'], 400)
    small = gpu.rescale_mask_up(UP[tiny]['mask'], UP[tiny]['scale'], 3)
    again = gpu.rescale_mask_up(UP[big]['mask'], UP[big]['scale'], 400)
    assert first.tobytes() == again.tobytes() and np.array_equal(first, golden['up_final_%d_400' % big])
    assert np.array_equal(small, golden['up_final_%d_3' % tiny])
    assert gpu.timings()['count'] > 0                            # device time of the kernels


def test_an_axis_of_radius_zero_is_copied(gpu):
    """Extents that one axis keeps: that axis has sigma 0 and is copied; the filter runs along the other alone."""
    img = cases.scene(40, 48, 9)
    ptr = _lib._ptr
    for oh, ow in ((40, 16), (13, 48), (40, 48)):
        wy, wx = _lib.rescale_weights(40, oh), _lib.rescale_weights(48, ow)
        out, filtered = np.empty((oh, ow), np.float64), np.empty_like(img)
        assert gpu.lib.ecseg_rescale_down(gpu.h, ptr(img), 40, 48, oh, ow, ptr(wy), len(wy) // 2, ptr(wx), len(wx) // 2, ptr(filtered),
                                          ptr(out)) == 0
        want_f = ref.filter_axis(ref.filter_axis(img, wy, 0), wx, 1)
        assert np.array_equal(filtered, want_f) and np.array_equal(out, ref.bilinear(want_f.astype(np.float64) / 255, oh, ow))
    assert np.array_equal(filtered, img)


def test_argument_errors(gpu):
    img = np.full((32, 40), 7, np.uint8)
    out, filtered = np.empty((16, 20), np.float64), np.empty_like(img)
    w3, w1 = _lib.rescale_weights(32, 16), np.ones(1)
    big = np.ones(2 * 65 + 1)
    ptr = _lib._ptr
    down = lambda *a: gpu.lib.ecseg_rescale_down(gpu.h, *a)
    ok = (ptr(img), 32, 40, 16, 20, ptr(w3), 2, ptr(w3), 2, ptr(filtered), ptr(out))
    assert down(*ok) == 0 and down(*ok[:9], None, ptr(out)) == 0                        # `filtered` may be null
    bad = lambda i, v: down(*(ok[:i] + (v,) + ok[i + 1:]))
    assert bad(0, None) == -1 and bad(10, None) == -1                                   # ECSEG_E_INVALID: null image, null out
    assert bad(1, 0) == -1 and bad(2, -4) == -1 and bad(3, 0) == -1 and bad(4, 0) == -1              # extents < 1
    assert down(ptr(img), 65536, 32768, 16, 20, ptr(w3), 2, ptr(w3), 2, None, ptr(out)) == -1        # 2^31 pixels
    assert bad(3, 33) == -1 and bad(4, 41) == -1                                        # an output extent above the input's
    assert bad(6, 32) == -1 and bad(8, 40) == -1                                        # ry >= H, rx >= W
    assert bad(6, -1) == -1 and down(ptr(img), 80, 16, 16, 16, ptr(big), 65, ptr(w1), 0, None, ptr(out)) == -1     # radius < 0, above the maximum
    assert bad(5, None) == -1 and bad(7, None) == -1                                    # no weights for a radius above 0
    m = np.ones((8, 8), np.uint8)
    res = np.empty((16, 16), np.uint8)
    up = lambda *a: gpu.lib.ecseg_rescale_mask_up(gpu.h, *a)
    assert up(ptr(m), 8, 8, 16, 16, 0, ptr(res)) == 0
    assert up(None, 8, 8, 16, 16, 0, ptr(res)) == -1 and up(ptr(m), 8, 8, 16, 16, 0, None) == -1
    assert up(ptr(m), 0, 8, 16, 16, 0, ptr(res)) == -1 and up(ptr(m), 8, -3, 16, 16, 0, ptr(res)) == -1
    assert up(ptr(m), 8, 8, 0, 16, 0, ptr(res)) == -1 and up(ptr(m), 8, 8, 16, 0, 0, ptr(res)) == -1
    assert up(ptr(m), 8, 8, 65536, 32768, 0, ptr(res)) == -1                            # 2^31 output pixels: refused before anything is touched
    assert up(ptr(m), 8, 8, 16, 16, -1, ptr(res)) == -1
    assert up(ptr(m), 8, 8, 7, 16, 0, ptr(res)) == -1 and up(ptr(m), 8, 8, 16, 7, 0, ptr(res)) == -1   # an output extent below the input's
    with pytest.raises(_lib.EcsegError):
        gpu.rescale_mask_up(m, 0.5, 0)
    with pytest.raises(_lib.EcsegError):
        gpu.rescale_down(img, 2.0)
    with pytest.raises(ValueError):
        gpu.rescale_down(img.astype(np.float32), 0.5)
    assert gpu.rescale_mask_up(m, 2.0, 0).max() == 0             # the handle still works; an image of one value comes out all zero


# ---- NuSeT.segment and make stat_fish ------------------------------------------------------------------------------------------
BASE = 8


def _raw_image(h, w, seed):
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[:h, :w]
    img = rng.normal(20.0, 4.0, (h, w))
    for _ in range(9):
        cy, cx, r = rng.uniform(0, h), rng.uniform(0, w), rng.uniform(6, 16)
        img += 150.0 * np.exp(-((yy - cy) ** 2 + (xx - cx) ** 2) / (2 * r * r))
    return np.clip(img, 0, 255).astype(np.uint8)


@pytest.fixture(scope='module')
def weights():
    return nuset.synth_weights(nuset.nuset_config(16, 16, BASE), seed=21)


def _composition(net, img, scale_ratio, min_score, nms, size_t):
    """The restatement's down-scale, the device's own network, markers, watershed and clean-up, the restatement's up-scale."""
    small, _ = ref.rescale_down(img, scale_ratio)
    m, scores, proposals = net.nuclei_masks(small, min_score, nms)
    mk = nuset.watershed_markers(scores, proposals, m, min_score, net.handle)
    ws = m if mk is None else net.handle.marker_watershed(m, *mk)
    cleaned = net.handle.clean_nuclei(ws, 0, want_cleaned=True)[2]
    return ref.rescale_mask_up(cleaned, 1 / scale_ratio, size_t), int(cleaned.sum())


def test_segment_with_a_scale_ratio_equals_the_composition(gpu, weights):
    net = nuset.NuSeT(weights, BASE, handle=gpu)
    img = _raw_image(128, 160, 128)
    for min_score, size_t in ((0.5, 0), (0.7, 40)):
        got = net.segment(img, min_score, 0.1, size_t, scale_ratio=0.5)
        want, fg = _composition(net, img, 0.5, min_score, 0.1, size_t)
        print('segment 128 x 160 at 0.5: %d cleaned foreground pixels at 64 x 80, %d in the final mask' % (fg, int((got != 0).sum())))
        assert got.shape == (128, 160) and got.dtype == np.uint8 and np.array_equal(got, want)
    # 0.3: 38 x 48 after rescale, cropped to 32 x 48, back up to round(32 / 0.3) x round(48 / 0.3)
    got = net.segment(img, 0.5, 0.1, 0, scale_ratio=0.3)
    assert got.shape == (107, 160) and np.array_equal(got, _composition(net, img, 0.3, 0.5, 0.1, 0)[0])
    with pytest.raises(ValueError):
        net.segment(img[:40, :40], scale_ratio=0.3)              # 12 x 12
    with pytest.raises(ValueError):
        net.segment(img.astype(np.float32), scale_ratio=0.5)     # rescale filters in the input's dtype: uint8 only


def test_scale_ratio_one_is_todays_path(gpu, weights):
    net = nuset.NuSeT(weights, BASE, handle=gpu)
    img = _raw_image(96 + 5, 128 + 3, 96)
    m, scores, proposals = net.nuclei_masks(img, 0.5, 0.1)
    mk = nuset.watershed_markers(scores, proposals, m, 0.5, gpu)
    want = gpu.clean_nuclei(m if mk is None else gpu.marker_watershed(m, *mk), 12)[0]
    assert np.array_equal(net.segment(img, 0.5, 0.1, 12), want) and np.array_equal(net.segment(img, 0.5, 0.1, 12, scale_ratio=1), want)
    assert np.array_equal(net.segment(img, 0.5, 0.1, 12, scale_ratio=1.0), want) and want.shape == (96, 128)


def test_make_stat_fish_with_a_scale_ratio_equals_the_mask_folder_run(gpu, weights, tmp_path, monkeypatch):
    import yaml
    from PIL import Image
    from ecseg_amd import image_io
    npz = {}
    for name, arrs in weights.items():
        for part, a in zip(('kernel', 'bias'), arrs):
            npz['%s/%s' % (nuset.CHECKPOINT_SCOPE[name], part)] = a
    np.savez(str(tmp_path / 'w.npz'), **npz)
    net = nuset.NuSeT(weights, BASE, handle=gpu)
    runs = {}
    for run in ('nuset', 'folder'):
        inp = tmp_path / run
        (inp / 'masks').mkdir(parents=True)
        (tmp_path / 'src').mkdir(exist_ok=True)
        yaml.safe_dump({'min_score': 0.5, 'nms_threshold': 0.1, 'scale_ratio': 0.5}, open(tmp_path / 'src' / 'stat_fish_params.yaml', 'w'))
        for k, name in enumerate(('a_img', 'b_img')):
            rgb = np.dstack([_raw_image(128, 160, 50 + 3 * k + j) for j in range(3)])
            Image.fromarray(rgb).save(str(inp / (name + '.tif')), compression='tiff_lzw')
            if run == 'folder':
                I, (blue, _, _) = sf.read_image(str(inp / (name + '.tif')), gpu)
                image_io.write_tiff_gray8(str(inp / 'masks' / (name + '.tif')), net.segment(I[:, :, blue], 0.5, 0.1, 10, scale_ratio=0.5))
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
