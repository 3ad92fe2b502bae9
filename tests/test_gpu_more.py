"""Wider parity cases on the GPU: Keras layer vocabulary beyond the canonical U-Net, odd image geometries for the
union-find kernels (widths below one 64-pixel chunk, heights below one 32-row tile, single rows / columns), and randomised
label maps for meta_inference."""
import os

import numpy as np
import pytest

from ecseg_amd import csvio, keras_plan, synth
from oracle import overlay as oracle_overlay
from oracle import postproc
from oracle import unet as oracle_unet

pytestmark = pytest.mark.gpu


def _L(cls, name, inbound, **cfg):
    return {'class_name': cls, 'name': name, 'config': dict(cfg, name=name),
            'inbound_nodes': [[[i, 0, 0, {}] for i in inbound]] if inbound else []}


def test_keras_layer_vocabulary(gpu):
    """Conv valid/same, BatchNorm before and after the activation, LeakyReLU / sigmoid / tanh / elu, ZeroPadding2D,
    Cropping2D, Add, bilinear UpSampling2D, Conv2DTranspose 3x3/s2 (generic path), Rescaling, Softmax layer."""
    rng = np.random.default_rng(42)
    H = W = 64
    layers = [
        _L('InputLayer', 'in', [], batch_input_shape=[None, H, W, 3]),
        _L('Rescaling', 'rs', ['in'], scale=1.0 / 255, offset=-0.5),
        _L('Conv2D', 'c1', ['rs'], filters=16, kernel_size=[3, 3], strides=[1, 1], padding='same', activation='linear', use_bias=False),
        _L('BatchNormalization', 'bn1', ['c1'], axis=[3], epsilon=1e-3, center=True, scale=True),
        _L('LeakyReLU', 'lr1', ['bn1'], alpha=0.2),
        _L('Conv2D', 'c2', ['lr1'], filters=16, kernel_size=[3, 3], strides=[1, 1], padding='valid', activation='tanh', use_bias=True),
        _L('ZeroPadding2D', 'zp', ['c2'], padding=[[1, 1], [1, 1]]),
        _L('Add', 'add', ['zp', 'lr1']),
        _L('MaxPooling2D', 'mp', ['add'], pool_size=[2, 2], strides=[2, 2], padding='valid'),
        _L('Conv2D', 'c3', ['mp'], filters=32, kernel_size=[3, 3], strides=[1, 1], padding='same', activation='elu', use_bias=True),
        _L('BatchNormalization', 'bn2', ['c3'], axis=[3], epsilon=1e-5, center=False, scale=True),
        _L('UpSampling2D', 'up', ['bn2'], size=[2, 2], interpolation='bilinear'),
        _L('Conv2DTranspose', 'ct', ['mp'], filters=8, kernel_size=[3, 3], strides=[2, 2], padding='same', activation='sigmoid',
           use_bias=True, output_padding=None),
        _L('Concatenate', 'cat', ['up', 'ct', 'add'], axis=-1),
        _L('Cropping2D', 'cr', ['cat'], cropping=[[2, 2], [4, 0]]),
        _L('Conv2D', 'c4', ['cr'], filters=4, kernel_size=[1, 1], strides=[1, 1], padding='same', activation='linear', use_bias=True),
        _L('Softmax', 'sm', ['c4'], axis=-1),
    ]
    cfg = {'class_name': 'Functional', 'config': {'name': 'm', 'layers': layers, 'input_layers': [['in', 0, 0]],
                                                  'output_layers': [['sm', 0, 0]]}}
    k = lambda *s: (rng.normal(size=s) / np.sqrt(np.prod(s[:-1]))).astype(np.float32)
    weights = {'c1': [k(3, 3, 3, 16)],
               'bn1': [rng.uniform(.5, 1.5, 16).astype(np.float32), rng.normal(size=16).astype(np.float32) * .1,
                       rng.normal(size=16).astype(np.float32) * .1, rng.uniform(.5, 1.5, 16).astype(np.float32)],
               'c2': [k(3, 3, 16, 16), rng.normal(size=16).astype(np.float32) * .1],
               'c3': [k(3, 3, 16, 32), rng.normal(size=32).astype(np.float32) * .1],
               'bn2': [rng.uniform(.5, 1.5, 32).astype(np.float32), rng.normal(size=32).astype(np.float32) * .1,
                       rng.uniform(.5, 1.5, 32).astype(np.float32)],
               'ct': [(rng.normal(size=(3, 3, 8, 16)) * .2).astype(np.float32), rng.normal(size=8).astype(np.float32) * .1],
               'c4': [k(1, 1, 56, 4), rng.normal(size=4).astype(np.float32) * .1]}
    x = rng.integers(0, 256, size=(2, H, W, 3), dtype=np.uint8)
    want = oracle_unet.forward(cfg, weights, x)
    for fuse in (False, True):
        gpu.load_plan(keras_plan.build_plan(cfg, weights, fuse=fuse))
        got = gpu.forward_patches(x)
        assert got.shape == want.shape == (2, 60, 60, 4)
        assert np.abs(got - want).max() < 1e-4, (fuse, np.abs(got - want).max())


@pytest.mark.parametrize('H,W', [(1, 1), (1, 200), (200, 1), (5, 63), (31, 65), (33, 64), (70, 130), (3, 3)])
def test_ccl_and_meta_inference_odd_geometries(gpu, H, W):
    rng = np.random.default_rng(H * 1000 + W)
    masks = (rng.random((6, H, W)) < np.array([0.0, 1.0, 0.3, 0.5, 0.62, 0.9])[:, None, None]).astype(np.uint8)
    for conn, lab_fn in ((8, postproc.label8), (4, postproc.label4)):
        got = gpu.ccl_labels(masks, conn)
        for k in range(len(masks)):
            lab, n = lab_fn(masks[k])
            assert got[k].max(initial=0) == 0 if n == 0 else True
            # same partition: every oracle component maps to exactly one GPU label and back
            pairs = set(zip(lab.ravel().tolist(), got[k].ravel().tolist()))
            assert len(pairs) == n + (1 if (masks[k] == 0).any() else 0), (H, W, conn, k)
    n, px = gpu.count_cc(masks)
    for k in range(len(masks)):
        wn, wpx = postproc.count_cc(masks[k])
        assert n[k] == wn and (px[k] == -1) == isinstance(wpx, float) and (px[k] == wpx or px[k] == -1)
    labs = rng.choice(4, size=(5, H, W), p=[.55, .2, .15, .1]).astype(np.uint8)
    out, nec = gpu.meta_inference(labs)
    for k in range(len(labs)):
        want = postproc.meta_inference(labs[k])
        assert np.array_equal(out[k], want), (H, W, k)
        assert nec[k] == postproc.count_cc(want == 3)[0]


def test_meta_inference_randomised_scenes(gpu):
    """40 seeded scenes of varying size / density, batched by size; bit-exact against the oracle."""
    rng = np.random.default_rng(7)
    for (H, W) in [(96, 160), (130, 97), (257, 129)]:
        labs = []
        for i in range(12):
            a = synth.label_map(int(rng.integers(0, 10 ** 6)), H, W, salt=float(rng.choice([0, 0.001, 0.01, 0.05])))
            if i % 4 == 0:          # blocky noise: big components of every class with ragged borders
                b = rng.integers(0, 4, size=(H // 8 + 1, W // 8 + 1)).astype(np.uint8)
                a = np.kron(b, np.ones((8, 8), np.uint8))[:H, :W]
                a[rng.random((H, W)) < 0.05] = 0
            labs.append(a)
        labs = np.stack(labs)
        out, nec = gpu.meta_inference(labs)
        for k in range(len(labs)):
            want = postproc.meta_inference(labs[k])
            assert np.array_equal(out[k], want), (H, W, k)
            assert nec[k] == postproc.count_cc(want == 3)[0]


def test_input_normalisation_lambdas(gpu):
    """The two ways public Keras U-Nets normalise their uint8 input: a TFOpLambda (``inputs / 255.``) and a Python
    ``Lambda(lambda x: x / 255)`` (needs lambda_overrides, its bytecode is opaque)."""
    rng = np.random.default_rng(3)
    for kind in ('tfop', 'lambda'):
        norm = (_L('TFOpLambda', 'tf.math.truediv', [], function='math.truediv') if kind == 'tfop'
                else _L('Lambda', 'lambda', ['in'], function=['4wEAAAA=', None, None], function_type='lambda'))
        if kind == 'tfop':
            norm['inbound_nodes'] = [['in', 0, 0, {'y': 255.0, 'name': None}]]
        layers = [_L('InputLayer', 'in', [], batch_input_shape=[None, 32, 48, 1]), norm,
                  _L('Conv2D', 'c', [norm['name']], filters=8, kernel_size=[3, 3], strides=[1, 1], padding='same',
                     activation='relu', use_bias=True)]
        cfg = {'class_name': 'Functional', 'config': {'name': 'm', 'layers': layers, 'input_layers': [['in', 0, 0]],
                                                      'output_layers': [['c', 0, 0]]}}
        weights = {'c': [rng.normal(size=(3, 3, 1, 8)).astype(np.float32), rng.normal(size=8).astype(np.float32) * .1]}
        x = rng.integers(0, 256, size=(2, 32, 48, 1), dtype=np.uint8)
        want = oracle_unet.forward(cfg, weights, x, lambda_fns={'lambda': lambda t: t / 255.0})
        if kind == 'lambda':
            with pytest.raises(keras_plan.PlanError):
                keras_plan.build_plan(cfg, weights)
        gpu.load_plan(keras_plan.build_plan(cfg, weights, lambda_overrides={'lambda': (1 / 255.0, 0.0)}))
        got = gpu.forward_patches(x)
        assert np.abs(got - want).max() < 1e-5, kind


def test_preprocess_on_second_source_otsu_fixtures(gpu, golden_dir):
    """Device meta_preprocess on the skimage-pinned Otsu fixtures (tests/golden/otsu_skimage.npz) and the hand-computed
    convertScaleAbs answers: same result as the oracle, image by image."""
    import os
    from oracle import preprocess
    z = np.load(os.path.join(golden_dir, 'otsu_skimage.npz'))
    n = len([k for k in z.files if k.startswith('img_')])
    for k in range(n):
        im = z['img_%02d' % k]
        gray, inv = gpu.preprocess(im[None])
        want = preprocess.meta_preprocess(im)
        assert np.array_equal(gray[0], want), k
        assert bool(inv[0]) == (not np.array_equal(want, im))
    x = np.array([0, 1, 128, 129, 257, 32767, 32768, 32896, 65534, 65535], np.uint16)
    assert gpu.u16_to_u8(x).tolist() == [0, 0, 0, 1, 1, 127, 128, 128, 255, 255]


def test_edge_cases_empty_small_and_large_images(gpu):
    """Empty batches are no-ops, images smaller than one 256x256 window are rejected as by the reference (which crashes on
    them), and a 2304x2304 image (121 windows: the launch group shrinks to keep the activation memory bounded) goes through
    with the same invariants as any other size."""
    from ecseg_amd import keras_plan
    from ecseg_amd._lib import EcsegError
    from oracle import postproc
    cfg = synth.unet_config(base=16, depth=2)
    gpu.load_plan(keras_plan.build_plan(cfg, synth.unet_weights(cfg, seed=4)))
    raw, post, nec = gpu.segment_images(np.zeros((0, 300, 300), np.uint8))
    assert post.shape == (0, 300, 300) and nec.shape == (0,)
    assert gpu.forward_patches(np.zeros((0, 256, 256, 1), np.uint8)).shape[0] == 0
    assert gpu.count_cc(np.zeros((0, 8, 8), np.uint8))[0].shape == (0,)
    with pytest.raises(EcsegError):
        gpu.segment_images(np.zeros((1, 200, 300), np.uint8))
    big = np.stack([synth.dapi_image(70 + i, 2304, 2304) for i in range(2)])
    raw, post, nec = gpu.segment_images(big, want_raw=True)
    for i in range(2):
        want = postproc.meta_inference(raw[i])
        assert np.array_equal(post[i], want)
        assert nec[i] == postproc.count_cc(want == 3)[0]
    one = gpu.segment_images(big[1:2], want_raw=True)
    assert np.array_equal(one[0][0], raw[1]) and np.array_equal(one[1][0], post[1])


def test_real_weights_kit_diffs_labels_counts_and_csv(tmp_path, golden_dir):
    """VERDICT r03 item 7 / SURVEY 8(f)3: the validation kit carries the reference's final labels, n_ec and CSV text, and
    `check` diffs every stage - exercised here on the synthetic .h5 fixture with this repository's CPU oracle standing in
    for TensorFlow (`dump --oracle`; with TF 2.8 + metaseg.h5 the same two commands validate the real weights)."""
    import subprocess
    import sys
    from PIL import Image
    from ecseg_amd import synth
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    h5 = os.path.join(golden_dir, 'metaseg_synth_b8.h5')
    img = tmp_path / 'input.tif'
    Image.fromarray(synth.dapi_image(61, 300, 420, rgb=True)).save(str(img), compression='tiff_lzw')
    ref = str(tmp_path / 'keras_ref.npz')
    tool = os.path.join(root, 'tools', 'validate_real_weights.py')
    env = dict(os.environ, PYTHONPATH=root)
    d = subprocess.run([sys.executable, tool, 'dump', '--oracle', h5, str(img), ref], capture_output=True, text=True, env=env)   # CPU only
    assert d.returncode == 0, d.stderr
    r = np.load(ref)
    assert str(r['csv']) == 'image_name,# of ec\ninput.tif,%d\n' % int(r['n_ec']) and r['final'].shape == r['raw'].shape == r['gray'].shape
    for flags in ([], ['--exact']):
        c = subprocess.run([sys.executable, tool, 'check', h5, ref] + flags, capture_output=True, text=True, env=env)
        # 0: everything identical; 3: only tie-risk pixels differ (float32 summation order) - both are a pass of the kit;
        # 1 would be a probability above the bar or a mismatch outside the tie-risk set
        assert c.returncode in (0, 3), c.stdout + c.stderr
        assert 'outside the reference' in c.stdout and 'ec_quantification.csv:' in c.stdout and 'labels after meta_inference' in c.stdout
        assert ' 0 of them outside' in c.stdout, c.stdout


def test_device_timers_of_overlay_and_preprocess(gpu):
    """bench.py's overlay_ms_per_image / preprocess_ms_per_image legs read ECSEG_T_COUNT: the device time of the kernels of the last
    ecseg_overlay / ecseg_preprocess / ecseg_count_* call (HIP events inside the entry point, copies excluded)."""
    from ecseg_amd import synth
    H, W = 256, 320
    rgb = np.stack([synth.dapi_image(11 + i, H, W, rgb=True) for i in range(3)])
    lab = np.stack([synth.label_map(11 + i, H, W) for i in range(3)])
    rows = gpu.overlay(lab, rgb, 85)
    t = gpu.timings()
    assert rows.shape == (3, 12) and t['count'] > 0.0 and t['unet'] == 0.0 and t['post'] == 0.0
    gpu.preprocess(rgb)
    t2 = gpu.timings()
    assert 0.0 < t2['count'] < t['count']                       # one gather + histogram against five labellings
    n, px = gpu.count_cc(lab == 3)
    assert gpu.timings()['count'] > 0.0 and len(n) == 3


@pytest.mark.parametrize('base,up', [(16, 'transpose'), (32, 'transpose'), (64, 'transpose')])
def test_window_lanes_do_not_change_results(gpu, base, up):
    """Small batches run the U-Net as several window lanes on their own streams (plan_run.hip: run_plan - a lane is whole images,
    or a slice of ONE image's windows with the matching slice of every crop list); same kernels, same per-window arithmetic:
    raw labels, cleaned labels, counts and the stitched probabilities are bit-identical for every lane count."""
    cfg = synth.unet_config(base=base, up=up)
    gpu.load_plan(keras_plan.build_plan(cfg, synth.unet_weights(cfg, seed=9)))
    try:
        for n_img, lane_counts in ((1, (1, 2, 3, 5, 8)), (3, (1, 2, 3)), (2, (1, 2, 4))):
            imgs = np.stack([synth.dapi_image(40 + i) for i in range(n_img)])
            ref = None
            for lanes in lane_counts:
                gpu.set_option('unet_lanes', lanes)
                got = gpu.segment_images(imgs, want_raw=True, want_tie_risk=True, want_probs=(n_img == 1))
                if ref is None:
                    ref = got
                    continue
                for a, b in zip(ref, got):
                    assert np.array_equal(a, b), (n_img, lanes)
        # another image size: 5 x 5 windows, other crop lists
        img = synth.dapi_image(77, 1100, 1100)[None]
        gpu.set_option('unet_lanes', 1)
        ref = gpu.segment_images(img, want_raw=True)
        gpu.set_option('unet_lanes', 3)
        got = gpu.segment_images(img, want_raw=True)
        for a, b in zip(ref, got):
            assert np.array_equal(a, b)
    finally:
        gpu.set_option('unet_lanes', 0)


@pytest.mark.parametrize('n_img', [1, 7, 8, 9, 13, 16, 19])
def test_clean_up_and_counts_for_every_batch_remainder(gpu, n_img):
    """The CCL kernels map complete groups of 8 images to one XCD per image and deal the tiles of the remaining images (all of them
    below 8) over all XCDs (ccl.h: decode_block): every image of every batch size gets the same answer as alone, and
    that answer is the oracle's."""
    rng = np.random.default_rng(100 + n_img)
    H, W = 150, 333                                             # 5 x 6 tiles, the last ones partial
    labs = np.stack([synth.label_map(300 + i, H, W) if i % 3 else rng.integers(0, 4, size=(H, W)).astype(np.uint8) for i in range(n_img)])
    post, nec = gpu.meta_inference(labs)
    cnt, px = gpu.count_cc(labs == 3)
    rgbs = np.stack([synth.dapi_image(500 + i, H, W, rgb=True) for i in range(n_img)])
    rows = gpu.overlay(labs, rgbs, 85)
    for i in range(n_img):
        want = postproc.meta_inference(labs[i])
        assert np.array_equal(post[i], want), i
        assert nec[i] == postproc.count_cc(want == 3)[0]
        assert (cnt[i], px[i]) == tuple(postproc.count_cc(labs[i] == 3)), i
        assert csvio.overlay_cells(rows[i]) == oracle_overlay.overlay_row(labs[i], rgbs[i], 85), i
    one = gpu.overlay(labs[-1], synth.dapi_image(500 + n_img - 1, H, W, rgb=True), 85)
    assert np.array_equal(np.asarray(one).reshape(-1), np.asarray(rows[-1]).reshape(-1))


# ---- round 5: the wider Keras vocabulary ---------------------------------------------------------
def _F(layers, ins, outs, name='m'):
    return {'class_name': 'Functional', 'config': {'name': name, 'layers': layers, 'input_layers': [[i, 0, 0] for i in ins],
                                                   'output_layers': [[o, 0, 0] for o in outs]}}


def _check(gpu, cfg, weights, x, tol=1e-3, output=0, **okw):
    """Whole chains within ``tol``; tests/test_gpu_layers.py holds each non-convolution kernel alone to a derived per-op bound."""
    want = oracle_unet.forward(cfg, weights, x, output=output, **okw)
    scale = max(1.0, float(np.abs(want).max()))
    for fuse in (True, False):
        gpu.load_plan(keras_plan.build_plan(cfg, weights, fuse=fuse, output=output))
        got = gpu.forward_patches(x)
        assert got.shape == want.shape, (got.shape, want.shape)
        err = float(np.abs(got - want).max()) / scale
        assert np.isfinite(got).all() and err < tol, (fuse, err)
    return want


def _he(rng, *s):
    return (rng.normal(size=s) / np.sqrt(np.prod(s[:-1]))).astype(np.float32)


@pytest.mark.parametrize('case', [
    # (H, W, cin, cout, k, stride, dilation, padding): the tap-by-tap MFMA kernel (dilated taps, 5x5 / 7x7 / 1x3 taps, stride 3)
    (32, 48, 16, 32, 3, 1, 2, 'same'), (24, 24, 8, 16, 3, 1, 3, 'same'), (40, 40, 64, 64, 3, 1, 6, 'same'), (33, 20, 32, 128, 3, 1, 2, 'valid'),
    (32, 32, 12, 24, 3, 1, 4, 'same'), (32, 32, 36, 40, 5, 1, 1, 'same'), (64, 64, 16, 32, 7, 2, 1, 'same'), (32, 32, 16, 16, 3, 3, 1, 'valid'),
    (16, 16, 256, 96, 3, 1, 12, 'same'), (32, 32, 6, 10, 3, 1, 2, 'same'), (32, 32, 16, 4, 3, 1, 2, 'same'), (32, 32, 1, 8, 3, 1, 2, 'same')])
def test_dilated_and_odd_tap_convolutions(gpu, case):
    H, W, cin, cout, k, st, dil, pad = case
    rng = np.random.default_rng(hash(case) % 2 ** 31)
    layers = [_L('InputLayer', 'in', [], batch_input_shape=[None, H, W, cin]),
              _L('Conv2D', 'c', ['in'], filters=cout, kernel_size=[k, k], strides=[st, st], dilation_rate=[dil, dil], padding=pad,
                 activation='relu', use_bias=True),
              _L('Conv2D', 'c13', ['c'], filters=16, kernel_size=[1, 3], strides=[1, 1], padding='same', activation='linear', use_bias=True)]
    w = {'c': [_he(rng, k, k, cin, cout), _he(rng, cout)], 'c13': [_he(rng, 1, 3, cout, 16), _he(rng, 16)]}
    x = rng.normal(size=(3, H, W, cin)).astype(np.float32)
    _check(gpu, _F(layers, ['in'], ['c13']), w, x)


@pytest.mark.parametrize('case', [
    # (H, W, cin, cout, (kh, kw), (stride_y, stride_x), (dilation_y, dilation_x), padding): per-axis strides / dilation rates (round 6)
    (32, 48, 16, 32, (3, 3), (2, 1), (1, 1), 'same'), (33, 47, 8, 24, (3, 3), (1, 3), (1, 1), 'valid'), (24, 40, 16, 16, (3, 3), (1, 1), (2, 3), 'same'),
    (20, 64, 4, 8, (1, 5), (1, 2), (1, 1), 'same'), (31, 29, 12, 20, (2, 3), (3, 2), (1, 1), 'same'), (40, 24, 32, 64, (3, 1), (1, 1), (4, 1), 'valid'),
    (16, 16, 1, 4, (3, 3), (1, 1), (1, 2), 'same'), (256, 256, 1, 8, (3, 3), (2, 1), (1, 1), 'same')])
def test_anisotropic_convolutions(gpu, case):
    """Conv2D with strides / dilation_rate that differ per axis runs on the device (the scalar kernel: the
    horizontal values travel in the CONV op's `mode`), followed by an isotropic 3x3 so that the shapes reach the fast kernels too."""
    H, W, cin, cout, kk, st, dil, pad = case
    rng = np.random.default_rng(hash(case) % 2 ** 31)
    layers = [_L('InputLayer', 'in', [], batch_input_shape=[None, H, W, cin]),
              _L('Conv2D', 'c', ['in'], filters=cout, kernel_size=list(kk), strides=list(st), dilation_rate=list(dil), padding=pad,
                 activation='relu', use_bias=True),
              _L('Conv2D', 'c3', ['c'], filters=16, kernel_size=[3, 3], strides=[1, 1], padding='same', activation='linear', use_bias=True)]
    w = {'c': [_he(rng, kk[0], kk[1], cin, cout), _he(rng, cout)], 'c3': [_he(rng, 3, 3, cout, 16), _he(rng, 16)]}
    x = rng.normal(size=(3, H, W, cin)).astype(np.float32)
    _check(gpu, _F(layers, ['in'], ['c3']), w, x)
    # the anisotropic layer alone, and the restatement without torch on it (oracle/unet.py conv_general_numpy)
    alone = _check(gpu, _F(layers[:2], ['in'], ['c']), {'c': w['c']}, x)
    first = np.maximum(oracle_unet.conv_general_numpy(x, w['c'][0], w['c'][1], pad, st, dil), 0)
    assert first.shape == alone.shape and float(np.abs(first - alone).max()) < 1e-4


@pytest.mark.parametrize('case', [
    # (H, W, c, k, stride, dilation, multiplier, padding)
    (32, 32, 32, 3, 1, 1, 1, 'same'), (33, 47, 64, 3, 2, 1, 1, 'same'), (24, 24, 24, 5, 1, 1, 1, 'same'), (20, 28, 96, 3, 1, 2, 1, 'same'),
    (16, 16, 6, 3, 1, 1, 1, 'same'), (16, 16, 8, 3, 1, 1, 2, 'valid'), (40, 40, 128, 7, 2, 1, 1, 'same'), (32, 32, 16, 3, 1, 6, 1, 'same'),
    (9, 9, 4, 3, 1, 1, 3, 'same')])
def test_depthwise_separable_and_grouped_convolutions(gpu, case):
    H, W, c, k, st, dil, m, pad = case
    rng = np.random.default_rng(hash(case) % 2 ** 31)
    if dil > 1:
        st = 1
    layers = [_L('InputLayer', 'in', [], batch_input_shape=[None, H, W, c]),
              _L('DepthwiseConv2D', 'dw', ['in'], kernel_size=[k, k], strides=[st, st], dilation_rate=[dil, dil], depth_multiplier=m, padding=pad,
                 activation='linear', use_bias=False),
              _L('BatchNormalization', 'bn', ['dw'], axis=[3], epsilon=1e-3, center=True, scale=True),
              _L('ReLU', 'r6', ['bn'], max_value=6.0, negative_slope=0.0, threshold=0.0),
              _L('SeparableConv2D', 'sep', ['r6'], filters=16, kernel_size=[3, 3], strides=[1, 1], dilation_rate=[1, 1], depth_multiplier=1,
                 padding='same', activation='relu', use_bias=True),
              _L('Conv2D', 'grp', ['sep'], filters=24, kernel_size=[3, 3], strides=[1, 1], padding='same', groups=4, activation='tanh', use_bias=True),
              _L('Conv2D', 'dwg', ['grp'], filters=48, kernel_size=[3, 3], strides=[1, 1], padding='same', groups=24, activation='linear', use_bias=True)]
    cm = c * m
    w = {'dw': [_he(rng, k, k, c, m) * np.float32(np.sqrt(c))],
         'bn': [rng.uniform(.5, 1.5, cm).astype(np.float32), _he(rng, cm), _he(rng, cm), rng.uniform(.5, 1.5, cm).astype(np.float32)],
         'sep': [_he(rng, 3, 3, cm, 1) * np.float32(np.sqrt(cm)), _he(rng, 1, 1, cm, 16), _he(rng, 16)],
         'grp': [_he(rng, 3, 3, 4, 24), _he(rng, 24)], 'dwg': [_he(rng, 3, 3, 1, 48), _he(rng, 48)]}
    x = rng.normal(size=(2, H, W, c)).astype(np.float32)
    _check(gpu, _F(layers, ['in'], ['dwg']), w, x)


def test_keras_layer_vocabulary_round5(gpu):
    """Multiply / Subtract / Maximum / Minimum / Average with broadcasting (the squeeze-and-excite gate), PReLU (per channel and per
    element), Normalization, LayerNormalization, 'same' pooling, every activation name, ELU(alpha), ReLU(max_value), a nested
    Functional and a nested Sequential sub-model, a model with two outputs - each against the oracle."""
    rng = np.random.default_rng(55)
    H, W, C = 24, 40, 16
    conv = lambda name, src, f, k=3, act='relu', **kw: _L('Conv2D', name, [src], filters=f, kernel_size=[k, k], strides=[1, 1], padding='same',
                                                          activation=act, use_bias=True, **kw)
    x = rng.normal(size=(3, H, W, C)).astype(np.float32)
    # --- squeeze-and-excite + the merge layers
    layers = [_L('InputLayer', 'in', [], batch_input_shape=[None, H, W, C]),
              conv('c1', 'in', 32),
              _L('GlobalAveragePooling2D', 'gap', ['c1'], keepdims=True),
              conv('se1', 'gap', 8, k=1), conv('se2', 'se1', 32, k=1, act='hard_sigmoid'),
              _L('Multiply', 'mul', ['c1', 'se2']),
              conv('att', 'c1', 1, k=1, act='sigmoid'),                     # (h, w, 1) spatial attention map
              _L('Multiply', 'mul2', ['att', 'mul']),                       # the broadcast operand FIRST
              _L('Subtract', 'sub', ['mul2', 'c1']),
              _L('Maximum', 'mx', ['sub', 'mul', 'c1']),
              _L('Minimum', 'mn', ['mx', 'se2']),
              _L('Average', 'avg', ['mn', 'mul2', 'c1']),
              _L('Add', 'addb', ['avg', 'se2'])]
    w = {'c1': [_he(rng, 3, 3, C, 32), _he(rng, 32)], 'se1': [_he(rng, 1, 1, 32, 8), _he(rng, 8)], 'se2': [_he(rng, 1, 1, 8, 32), _he(rng, 32)],
         'att': [_he(rng, 1, 1, 32, 1), _he(rng, 1)]}
    _check(gpu, _F(layers, ['in'], ['addb']), w, x)
    # --- PReLU x2, Normalization, LayerNormalization (8 / 32 / 96 channels: 4, 16 and 64 lanes per pixel), 'same' pooling
    for cc in (8, 32, 96):
        layers = [_L('InputLayer', 'in', [], batch_input_shape=[None, H, W, C]),
                  _L('Normalization', 'norm', ['in'], axis=[-1], mean=None, variance=None),
                  conv('c1', 'norm', cc, act='linear'),
                  _L('PReLU', 'p1', ['c1'], shared_axes=[1, 2]),
                  _L('LayerNormalization', 'ln', ['p1'], axis=[3], epsilon=1e-3, center=True, scale=True),
                  _L('MaxPooling2D', 'mp', ['ln'], pool_size=[3, 3], strides=[2, 2], padding='same'),
                  _L('PReLU', 'p2', ['mp'], shared_axes=None),
                  _L('AveragePooling2D', 'ap', ['p2'], pool_size=[2, 2], strides=[1, 1], padding='same'),
                  _L('LayerNormalization', 'ln2', ['ap'], axis=-1, epsilon=1e-5, center=False, scale=False)]
        w = {'norm': [rng.normal(size=C).astype(np.float32), rng.uniform(.5, 2, C).astype(np.float32), np.array(5, np.int64)],
             'c1': [_he(rng, 3, 3, C, cc), _he(rng, cc)], 'p1': [rng.uniform(-.3, .3, (1, 1, cc)).astype(np.float32)],
             'ln': [rng.uniform(.5, 1.5, cc).astype(np.float32), _he(rng, cc)], 'p2': [rng.uniform(-.3, .3, (12, 20, cc)).astype(np.float32)]}
        _check(gpu, _F(layers, ['in'], ['ln2']), w, x)
    # --- activations: as a convolution's own activation (fused or split off by the plan) and as layers
    for name in ('relu6', 'selu', 'softplus', 'softsign', 'swish', 'gelu', 'hard_sigmoid', 'exponential', 'elu', 'tanh', 'sigmoid'):
        layers = [_L('InputLayer', 'in', [], batch_input_shape=[None, H, W, C]),
                  conv('c1', 'in', 32, act=name), conv('c2', 'c1', 16, act='linear'), _L('Activation', 'a', ['c2'], activation=name),
                  _L('DepthwiseConv2D', 'dw', ['a'], kernel_size=[3, 3], strides=[1, 1], depth_multiplier=1, padding='same', activation=name, use_bias=True),
                  _L('ELU', 'elu', ['dw'], alpha=0.6), _L('ReLU', 'clip', ['elu'], max_value=2.5, negative_slope=0.0, threshold=0.0)]
        w = {'c1': [_he(rng, 3, 3, C, 32), _he(rng, 32)], 'c2': [_he(rng, 3, 3, 32, 16), _he(rng, 16)], 'dw': [_he(rng, 3, 3, 16, 1) * 4, _he(rng, 16)]}
        _check(gpu, _F(layers, ['in'], ['clip']), w, x)
    # --- nested Functional (with a skip connection) + nested Sequential + two outputs
    bn = lambda name, src: _L('BatchNormalization', name, [src], axis=[3], epsilon=1e-3, center=True, scale=True)
    inner = _F([_L('InputLayer', 'bin', [], batch_input_shape=[None, H, W, C]), conv('b1', 'bin', 32), bn('bbn', 'b1'), conv('b2', 'bbn', C),
                _L('Add', 'badd', ['b2', 'bin'])], ['bin'], ['badd'], name='backbone')
    seq = {'class_name': 'Sequential', 'name': 'headseq',
           'config': {'name': 'headseq', 'layers': [_L('Conv2D', 's1', [], filters=8, kernel_size=[1, 1], strides=[1, 1], padding='same',
                                                       activation='linear', use_bias=True, batch_input_shape=[None, H, W, C]),
                                                    _L('Softmax', 's2', [], axis=-1)]}}
    outer = _F([_L('InputLayer', 'in', [], batch_input_shape=[None, H, W, C]), dict(inner, name='backbone', inbound_nodes=[[['in', 0, 0, {}]]]),
                dict(seq, inbound_nodes=[[['backbone', 0, 0, {}]]]), _L('GlobalMaxPooling2D', 'gmp', ['backbone'])], ['in'], ['headseq', 'gmp'])
    wi = {'b1': [_he(rng, 3, 3, C, 32), _he(rng, 32)],
          'bbn': [rng.uniform(.5, 1.5, 32).astype(np.float32), _he(rng, 32), _he(rng, 32), rng.uniform(.5, 1.5, 32).astype(np.float32)],
          'b2': [_he(rng, 3, 3, 32, C), _he(rng, C)]}
    w = {'backbone': wi, 'headseq': {'s1': [_he(rng, 1, 1, C, 8), _he(rng, 8)]}}
    a = _check(gpu, outer, w, x, output=0)
    b = _check(gpu, outer, w, x, output='gmp')
    assert a.shape == (3, H, W, 8) and b.shape == (3, C)


def test_mobilenet_style_fixture_matches_oracle(gpu, golden_dir):
    """The h5py-written MobileNet-style classifier (tests/golden/mobilenet_synth.h5: nested backbone, depthwise + squeeze-and-excite
    Multiply + dilated + grouped + separable convolutions, PReLU, LayerNormalization) loads through hdf5_min - no h5py here - and
    its class probabilities match the oracle; the interSeg decision logic (src/interseg.py:153-190) runs on it."""
    import json
    from ecseg_amd import hdf5_min, interseg
    from ecseg_amd.model import MetasegModel
    path = os.path.join(golden_dir, 'mobilenet_synth.h5')
    cfg_txt, weights = hdf5_min.load_keras_h5(path)
    rng = np.random.default_rng(8)
    x = rng.integers(0, 256, size=(5, 96, 96, 3), dtype=np.uint8)
    want = oracle_unet.forward(json.loads(cfg_txt), weights, x)
    m = MetasegModel.from_h5(path, handle=gpu)
    got = m.predict(x)
    assert got.shape == want.shape == (5, 3)
    assert np.abs(got - want).max() < 1e-3 and np.abs(got.sum(1) - 1).max() < 1e-5
    assert [int(np.argmax(r)) for r in got] == [int(np.argmax(r)) for r in want]


def test_shared_layers_on_the_device(gpu):
    """Round 6: a convolution and a BatchNormalization that are each called twice (two inbound nodes, shared weights) - the plan runs
    one op per call; result vs the oracle's call-by-call evaluation."""
    from oracle import unet as oracle_unet
    from tests.test_oracle_layers import _shared_model
    rng = np.random.default_rng(33)
    c = 16
    cfg = _shared_model(64, 64, c)
    w = {'sc': [(rng.normal(size=(3, 3, c, c)) / 12).astype(np.float32), rng.normal(size=c).astype(np.float32)],
         'sbn': [rng.uniform(.5, 1.5, c).astype(np.float32), rng.normal(size=c).astype(np.float32), rng.normal(size=c).astype(np.float32),
                 rng.uniform(.5, 1.5, c).astype(np.float32)]}
    x = rng.integers(0, 256, size=(3, 64, 64, c), dtype=np.uint8)
    want = oracle_unet.forward(cfg, w, x)
    for fuse in (True, False):
        gpu.load_plan(keras_plan.build_plan(cfg, w, fuse=fuse))
        got = gpu.forward_patches(x)
        assert got.shape == want.shape and np.abs(got - want).max() < 1e-3 * max(1.0, float(np.abs(want).max())), fuse


def test_channels_first_model_on_the_device(gpu):
    """Round 6: a channels_first Keras U-Net ((N, C, H, W) tensors, channel axis 1) is lowered through its channels_last twin
    (keras_plan.channels_first_to_last) and MetasegModel transposes at the boundary: predict_on_batch((N, 1, 256, 256)) ->
    (N, 4, 256, 256), within 1e-3 of the oracle's native channels_first evaluation."""
    from ecseg_amd.model import MetasegModel
    from tests.test_oracle_layers import channels_first_twin
    cfg = channels_first_twin(synth.unet_config(base=16, depth=2, batchnorm=True))
    w = synth.unet_weights(synth.unet_config(base=16, depth=2, batchnorm=True), seed=6)
    x = np.stack([synth.dapi_image(300 + i, 256, 256) for i in range(2)])[:, None]          # (N, 1, H, W)
    want = oracle_unet.forward(cfg, w, x)
    m = MetasegModel(cfg, w, handle=gpu)
    assert m.plan.channels_first
    got = m.predict_on_batch(x)
    assert got.shape == want.shape == (2, 4, 256, 256) and np.abs(got - want).max() < 1e-3
    with pytest.raises(keras_plan.PlanError, match='mixes'):
        bad = channels_first_twin(synth.unet_config(base=16, depth=1))
        bad['config']['layers'][1]['config']['data_format'] = 'channels_last'
        keras_plan.build_plan(bad, synth.unet_weights(synth.unet_config(base=16, depth=1)))
