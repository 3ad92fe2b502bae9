"""interSeg's classifiers on the device (ecseg_classify_nucleus_crops, csrc/iseg_classify_kernels.hip): one call takes the crop
descriptors and returns what the host path gives - the same crops and maxima as ``Handle.nucleus_crops``, the same choice of crops
as ``classify_crops`` makes, and predictions bit-identical to ``model.predict`` on the same crops in the same order through the
host path (both feed the same float32 inputs to the same plan).  The input kernel alone against ``preprocess_ecseg_c``, bit for
bit; ``make interseg`` with ``classify_on_device`` on and off."""
import os
import shutil

import numpy as np
import pytest
import yaml
from PIL import Image

from ecseg_amd import hdf5_min, image_io, interseg
from ecseg_amd.model import MetasegModel

pytestmark = pytest.mark.gpu
SENTINEL = np.float32(-12345.5)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.fixture(scope='module')
def models(golden_dir):
    from ecseg_amd._lib import Handle
    hs = [Handle(0), Handle(0)]
    mi = MetasegModel(*hdf5_min.load_keras_h5(os.path.join(golden_dir, 'interseg_synth.h5')), handle=hs[0])
    mc = MetasegModel(*hdf5_min.load_keras_h5(os.path.join(golden_dir, 'ecseg_c_synth.h5')), handle=hs[1])
    yield mi, mc
    for h in hs:
        h.close()


def hand_scene():
    """(seg, img, names): nuclei as rectangles, channels (target FISH, probe, DAPI).  `wide` is 600 px wide: two 256-px tiles, the
    second all zero; `p10` / `p11`: probe maxima exactly 10 and 11; `nodapi`: DAPI all zero under a bright probe (NaN in the ecSeg-c
    input); `dot`: a 1 x 1 window; `full`: a 256 x 256 window."""
    rng = np.random.default_rng(11)
    H, W = 312, 610
    seg = np.zeros((H, W), np.uint8)
    img = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    boxes = {'wide': (2, 2, 40, 600), 'full': (50, 2, 256, 256), 'p10': (50, 270, 30, 33), 'p11': (50, 320, 31, 30), 'nodapi': (50, 370, 29, 41),
             'dot': (50, 430, 1, 1)}
    for y, x, h, w in boxes.values():
        seg[y:y + h, x:x + w] = 255
    img[2:42, 258:, :] = 0                                                    # the second tile of `wide` (and its dropped remainder)
    img[2:42, 2:258, 0] |= 128                                                # ... which still passes the brightness gate
    y, x, h, w = boxes['p10']
    img[y:y + h, x:x + w, 1] = 10
    y, x, h, w = boxes['p11']
    img[y:y + h, x:x + w, 1] = 11
    y, x, h, w = boxes['nodapi']
    img[y:y + h, x:x + w, 2] = 0
    img[y:y + h, x:x + w, 1] |= 64
    img[50, 430] = (200, 77, 3)
    return seg, img, boxes


def host_path(handle, mi, mc, desc, order, tiled, centromeric):
    """What process_image computes today: the crops on the host, the choice of classify_crops, predict on the chosen crops in order."""
    crops, cmax = handle.nucleus_crops(desc, order)
    ran_i = ~(np.asarray(tiled, bool) & (cmax.max(axis=1) == 0))
    ran_c = ran_i & bool(centromeric and mc is not None) & (cmax[:, 1] > 10)
    pred_i = mi.predict(crops[ran_i][..., 0]) if ran_i.any() else np.zeros((0, 3), np.float32)
    pred_c = mc.predict(np.stack([interseg.preprocess_ecseg_c(c) for c in crops[ran_c]])).reshape(-1) if ran_c.any() else np.zeros(0, np.float32)
    return crops, cmax, ran_i, ran_c, pred_i, pred_c


def assert_same_as_host(handle, mi, mc, desc, order, tiled, centromeric, want_crops=True):
    n = len(desc)
    crops, cmax, ran_i, ran_c, pred_i, pred_c = host_path(handle, mi, mc, desc, order, tiled, centromeric)
    got_i = np.full((n, 3), SENTINEL, np.float32)
    got_c = np.full(n, SENTINEL, np.float32)
    out = handle.classify_nucleus_crops(desc, order, tiled, centromeric, mi, mc, want_crops=want_crops, pred_i=got_i, pred_c=got_c)
    assert out[1] is got_i and out[3] is got_c
    print('%s: %d crops, ecSeg-i ran for %d, ecSeg-c for %d; first rows %s / %s (host %s / %s); device ms: crops %.4f, inputs %.4f, plans %.4f / %s'
          % (handle.device_name, n, ran_i.sum(), ran_c.sum(), bits(got_i[ran_i][:1]).tolist(), bits(got_c[ran_c][:1]).tolist(),
             bits(pred_i[:1]).tolist(), bits(pred_c[:1]).tolist(), handle.timings()['count'], handle.timings()['tile'],
             mi.handle.timings()['unet'], '%.4f' % mc.handle.timings()['unet'] if mc is not None else '-'))
    assert np.array_equal(out[0], cmax) and out[0].dtype == np.int32
    if want_crops:
        assert out[5].dtype == np.uint8 and np.array_equal(out[5], crops)
    assert np.array_equal(out[2], ran_i) and np.array_equal(out[4], ran_c)
    assert np.array_equal(bits(got_i[ran_i]), bits(pred_i))                    # NaN included
    assert np.array_equal(bits(got_c[ran_c]), bits(pred_c))
    assert (got_i[~ran_i] == SENTINEL).all() and (got_c[~ran_c] == SENTINEL).all()       # rows of models that did not run: untouched
    return crops, cmax, ran_i, ran_c, got_i, got_c


@pytest.mark.parametrize('crops_handle', ['third', 'ecseg_i'])
@pytest.mark.parametrize('fish_index', [0, 1])
def test_hand_scene_equals_the_host_path(gpu, models, crops_handle, fish_index):
    mi, mc = models
    handle = gpu if crops_handle == 'third' else mi.handle
    seg, img, boxes = hand_scene()
    if fish_index:
        img = np.ascontiguousarray(img[..., [1, 0, 2]])
    rec = handle.nuclei_regions(seg, img, fish_index)
    centers, low, desc, tiled, owner = interseg.region_rows(rec)
    assert not low.any() and len(desc) == 7 and tiled.tolist() == [True, True] + [False] * 5
    order = (fish_index, 1 - fish_index, 2)
    crops, cmax, ran_i, ran_c, pred_i, pred_c = assert_same_as_host(handle, mi, mc, desc, order, tiled, True)
    by_box = {name: k for k, d in enumerate(desc.tolist()) for name, (y, x, h, w) in boxes.items() if d[1:3] == [y, x]}
    k10, k11, knd, kdot, kfull = (by_box[n] for n in ('p10', 'p11', 'nodapi', 'dot', 'full'))
    assert desc[kdot, 3:].tolist() == [1, 1] and desc[kfull, 3:].tolist() == [256, 256]
    assert not crops[1].any() and not ran_i[1] and not ran_c[1] and ran_i.sum() == 6          # the all-zero tile
    assert cmax[k10, 1] == 10 and not ran_c[k10] and cmax[k11, 1] == 11 and ran_c[k11]
    assert cmax[knd, 2] == 0 and cmax[knd, 1] > 10 and ran_c[knd] and ran_c.sum() == 5
    _, x_c = handle.iseg_classifier_inputs(crops[knd:knd + 1], cmax[knd:knd + 1], [], [0])
    assert np.isnan(x_c[..., 2]).all() and np.isfinite(x_c[..., :2]).all()                     # 0 / 0 in the DAPI channel went into ecSeg-c
    assert np.isfinite(pred_i[ran_i]).all() and np.isfinite(pred_c[ran_c & (np.arange(7) != knd)]).all()
    assert (crops[kdot] == crops[kdot][0, 0]).all()


def test_without_ecseg_c_or_its_flag_nothing_of_it_is_written(gpu, models):
    mi, mc = models
    seg, img, _ = hand_scene()
    _, _, desc, tiled, _ = interseg.region_rows(gpu.nuclei_regions(seg, img, 0))
    for cent, model_c in ((False, mc), (True, None), (False, None)):
        _, _, ran_i, ran_c, _, got_c = assert_same_as_host(gpu, mi, model_c, desc, (0, 1, 2), tiled, cent, want_crops=False)
        assert not ran_c.any() and ran_i.sum() == 6 and (got_c == SENTINEL).all()
    out = gpu.classify_nucleus_crops(desc, (0, 1, 2), tiled, True, mi, mc)
    assert len(out) == 5 and out[4].sum() == 5


def test_region_map_and_buffers_serve_calls_in_any_order(gpu, models):
    mi, mc = models
    seg, img, _ = hand_scene()
    _, _, desc, tiled, _ = interseg.region_rows(gpu.nuclei_regions(seg, img, 0))
    first = gpu.classify_nucleus_crops(desc, (0, 1, 2), tiled, True, mi, mc, want_crops=True)
    crops, cmax = gpu.nucleus_crops(desc, (0, 1, 2))
    second = gpu.classify_nucleus_crops(desc, (0, 1, 2), tiled, True, mi, mc, want_crops=True)
    assert np.array_equal(first[5], crops) and np.array_equal(first[0], cmax)
    for a, b in zip(first, second):
        assert np.array_equal(bits(a), bits(b)) if a.dtype == np.float32 else np.array_equal(a, b)
    assert gpu.timings()['count'] > 0 and gpu.timings()['tile'] > 0 and mi.handle.timings()['unet'] > 0 and mc.handle.timings()['unet'] > 0


def test_chunk_borders_and_odd_runs(gpu, models):
    """257 tiny windows of one nucleus: a chunk of 256 and one of 1; with 35 windows per group, runs of 35, an odd rest and 1."""
    mi, mc = models
    rng = np.random.default_rng(5)
    seg = np.zeros((48, 80), np.uint8)
    seg[4:44, 4:76] = 255
    img = rng.integers(1, 256, (48, 80, 3), dtype=np.uint8)
    img[4:44, 4:28, 1] = rng.integers(0, 11, (40, 24), dtype=np.uint8)         # the probe too dim on the left third
    img[4:44, 28:40, :] = 0                                                    # a dark stripe: empty tiles
    img[20:25, 60:63, 1] = 200
    gpu.nuclei_regions(seg, img, 0)
    n = 257
    h, w = rng.integers(1, 7, n), rng.integers(1, 7, n)
    desc = np.stack([np.zeros(n, int), rng.integers(4, 44 - h + 1), rng.integers(4, 76 - w + 1), h, w], axis=1).astype(np.int32)
    desc[255] = (0, 10, 30, 4, 4)                                              # the dark stripe at both sides of the border
    desc[256] = (0, 20, 60, 5, 3)
    tiled = rng.random(n) < 0.7
    tiled[255] = True
    for m in (mi, mc):
        m.handle.set_images_per_group(1)
    try:
        _, _, ran_i, ran_c, _, _ = assert_same_as_host(gpu, mi, mc, desc, (0, 1, 2), tiled, True)
    finally:
        for m in (mi, mc):
            m.handle.set_images_per_group(0)
    assert not ran_i[255] and ran_i[256] and ran_c[256]
    assert ran_i[:256].sum() > 35 * 6 and ran_i[:256].sum() % 35 not in (0, 1) and 35 < ran_c.sum() < 200 and (~ran_i).sum() > 3


def test_input_kernel_alone_is_preprocess_ecseg_c_bit_for_bit(gpu):
    rng = np.random.default_rng(2)
    crops = np.zeros((3, 256, 256, 3), np.uint8)
    ramp = (np.arange(65536) % 256).astype(np.uint8).reshape(256, 256)
    crops[0] = np.stack([ramp, ramp[::-1], ramp.T], axis=-1)                  # every byte value in every channel
    crops[1, ..., 0] = rng.integers(0, 2, (256, 256))                         # maxima 1, 255 and 0
    crops[1, ..., 1] = rng.integers(0, 256, (256, 256))
    crops[1, 7, 9, 0], crops[1, 100, 3, 1] = 1, 255
    crops[2] = rng.integers(0, 200, (256, 256, 3))
    cmax = crops.max(axis=(1, 2)).astype(np.int32)
    assert cmax[0].tolist() == [255, 255, 255] and cmax[1].tolist() == [1, 255, 0]
    pre = np.stack([interseg.preprocess_ecseg_c(c) for c in crops])
    assert np.isnan(pre[1, ..., 2]).all() and set(np.unique(pre[1, ..., 0]).tolist()) == {0.0, 1.0}
    as_f32 = crops[..., :1].astype(np.float32)
    for sel_i, sel_c in (([0], [0]), ([1], [1]), ([2, 2, 1, 0, 0], [2, 1, 1, 0]), ([0, 1, 2], []), ([], [1, 0]), ([1], [2, 0, 1])):
        out_i, out_c = gpu.iseg_classifier_inputs(crops, cmax, sel_i, sel_c)
        assert out_i.shape == (len(sel_i), 256, 256, 1) and out_c.shape == (len(sel_c), 256, 256, 3)
        assert np.array_equal(bits(out_i), bits(as_f32[sel_i]))
        assert np.array_equal(bits(out_c), bits(pre[sel_c])), (sel_i, sel_c)
    from ecseg_amd._lib import EcsegError
    for bad_i, bad_c in (([3], []), ([], [-1])):
        with pytest.raises(EcsegError):
            gpu.iseg_classifier_inputs(crops, cmax, bad_i, bad_c)


def test_models_of_another_shape_and_bad_descriptors_are_refused(gpu, models):
    from ecseg_amd._lib import EcsegError
    mi, mc = models
    seg, img, _ = hand_scene()
    _, _, desc, tiled, _ = interseg.region_rows(gpu.nuclei_regions(seg, img, 0))
    with pytest.raises(EcsegError, match='ecSeg-i') as e:
        gpu.classify_nucleus_crops(desc, (0, 1, 2), tiled, True, mc, mc)
    assert e.value.code == -1
    with pytest.raises(EcsegError, match='ecSeg-c'):
        gpu.classify_nucleus_crops(desc, (0, 1, 2), tiled, True, mi, mi)
    with pytest.raises(EcsegError, match='ecSeg-i'):
        gpu.classify_nucleus_crops(desc, (0, 1, 2), tiled, True, gpu, mc)       # (the session handle holds whatever plan a test left, or none)
    bad = desc.copy()
    bad[3, 3] = 257
    with pytest.raises(EcsegError, match='crop 3'):
        gpu.classify_nucleus_crops(bad, (0, 1, 2), tiled, True, mi, mc)
    with pytest.raises(EcsegError, match='channel_order'):
        gpu.classify_nucleus_crops(desc, (0, 1, 3), tiled, True, mi, mc)
    out = gpu.classify_nucleus_crops(desc[:0], (0, 1, 2), tiled[:0], True, mi, mc)
    assert [len(a) for a in out] == [0] * 5


# ---- `make interseg` with the key on --------------------------------------------------------------------------------------------
SCENES = ['interseg_scene_small.npz', 'interseg_scene_large.npz']


def _folder(root, golden_dir, on):
    """Two scenes and a grayscale file that fails alone, as tests/test_gpu_interseg_driver.py builds its folder."""
    os.makedirs(root / 'interseg_models')
    shutil.copy(os.path.join(golden_dir, 'interseg_synth.h5'), root / 'interseg_models' / 'interseg.h5')
    shutil.copy(os.path.join(golden_dir, 'ecseg_c_synth.h5'), root / 'interseg_models' / 'ecseg_c.h5')
    inp = root / 'images'
    os.makedirs(inp)
    for scene in SCENES:
        z = np.load(os.path.join(golden_dir, scene))
        stem = scene[:-4]
        Image.fromarray(z['image']).save(str(inp / (stem + '.tif')))
        os.makedirs(inp / 'annotated' / stem)
        image_io.write_tiff_gray8(str(inp / 'annotated' / stem / (stem + '_segmentation.tif')), z['seg'])
    image_io.write_tiff_gray8(str(inp / 'zz_gray.tif'), np.full((30, 30), 100, np.uint8))
    lines = ['image_name,Avg fish intensity (red),Avg fish intensity (green)']
    lines += ['interseg_scene_small,%s,1.0' % v for v in (3.1, 4.2, 5.0, 4.4, 3.9)]
    lines += ['interseg_scene_large,%s,1.0' % v for v in (1, 1, 1, 1, 1, 1, 1, 1, 1, 90)]      # kurtosis > 3: fails the quality score
    (inp / 'annotated' / 'stat_fish_lsq.csv').write_text('\n'.join(lines) + '\n')
    cfg = {'inpath': str(inp), 'FISH_color': 'green', 'has_centromeric_probe': True}
    if on is not None:
        cfg['classify_on_device'] = on
    with open(root / 'config.yaml', 'w') as f:
        yaml.safe_dump({'interseg': cfg}, f)
    return inp


def test_make_interseg_writes_the_same_csv_with_the_key_on(tmp_path, golden_dir, monkeypatch, capsys):
    from ecseg_amd import image_tools
    monkeypatch.setattr(image_tools, '_default', image_tools._default)          # load_model makes its handle the default one: put back after
    runs = {}
    for name, on in (('absent', None), ('on', True)):
        root = tmp_path / name
        os.makedirs(root)
        inp = _folder(root, golden_dir, on)
        monkeypatch.chdir(root)
        with pytest.raises(SystemExit) as e:
            interseg.main([])
        runs[name] = (e.value.code, open(inp / 'interphase_prediction_green.csv', 'rb').read(), capsys.readouterr().out.replace(str(root), ''))
    assert runs['on'] == runs['absent']
    code, text, out = runs['on']
    assert code == 1 and "zz_gray.tif - isn't an RGB image" in out and '1 image(s) were NOT processed' in out
    assert text.count(b'\n') > 10 and interseg.EMPTY.encode() in text and interseg.FAILED_QUALITY.encode() in text
    assert b'Focal-amp' in text or interseg.LOW_CENT.encode() in text          # ecSeg-c's column is filled for the image that passed
