"""SHA-256 digests of single F(4x4) layers at the smallest shapes that reach every arm of conv_wino4r_kernel, conv_wino4s_kernel and
conv_wino4_kernel (tests/test_gpu_wino4_layout.py compares a build against tests/golden/wino4_layer_digests.json).

    python tools/wino4_layer_digests.py --write          # on an MI355X, from the build whose results are the reference

A change of the LDS layout of these kernels (csrc/wino4_lds_layout.h) moves values in LDS and nothing else: every output must keep
its bits.  The committed file was written from a build of the commit BEFORE the layout changed (ECSEG_HIP_LIB names another build of
the library, ecseg_amd/_lib.py).
"""
import argparse
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'wino4_layer_digests.json')

WINOGRAD = (2, 3)                      # fp32 MFMA kernels | bf16x3 split kernel where it applies (Cout % 64 == 0)
ACTS = ('relu', 'linear', 'tanh')
# name: (N, H, W, Cin, Cout, tail) - what each reaches is in the test's docstring
LAYERS = {
    'odd_regions': (3, 16, 16, 8, 64, None),
    'tail4': (2, 32, 48, 12, 64, None),
    'cout96': (2, 32, 32, 64, 96, None),
    'split_k': (2, 32, 32, 64, 32, None),
    'pool': (2, 32, 32, 24, 64, 'pool'),
    'head': (2, 32, 32, 16, 64, 'head'),
}
CROP_IMAGE = (300, 462)                # one image -> 256 x 256 windows of a base-64 depth-1 U-Net, cropped plan (region lists, input boxes)


def _layer(cls, name, inbound, **cfg):
    cfg = dict(cfg, name=name)
    return {'class_name': cls, 'name': name, 'config': cfg, 'inbound_nodes': [[[i, 0, 0, {}] for i in inbound]] if inbound else []}


def layer_model(case, act):
    """-> (config, weights, input) of one case: seeded, independent of the activation."""
    n, H, W, cin, cout, tail = LAYERS[case]
    rng = np.random.default_rng(sorted(LAYERS).index(case) + 1)
    layers = [_layer('InputLayer', 'in', [], batch_input_shape=[None, H, W, cin]),
              _layer('Conv2D', 'c', ['in'], filters=cout, kernel_size=[3, 3], strides=[1, 1], padding='same', activation=act, use_bias=True)]
    w = {'c': [(rng.normal(size=(3, 3, cin, cout)) / np.sqrt(9 * cin)).astype(np.float32), rng.normal(size=cout).astype(np.float32)]}
    out = 'c'
    if tail == 'pool':
        layers.append(_layer('MaxPooling2D', 'p', ['c'], pool_size=[2, 2], strides=[2, 2], padding='valid'))
        out = 'p'
    elif tail == 'head':
        layers.append(_layer('Conv2D', 'h', ['c'], filters=4, kernel_size=[1, 1], strides=[1, 1], padding='same', activation='softmax', use_bias=True))
        w['h'] = [(rng.normal(size=(1, 1, cout, 4)) / np.sqrt(cout)).astype(np.float32), rng.normal(size=4).astype(np.float32)]
        out = 'h'
    cfg = {'class_name': 'Functional', 'config': {'name': 'm', 'layers': layers, 'input_layers': [['in', 0, 0]], 'output_layers': [[out, 0, 0]]}}
    x = rng.normal(size=(n, H, W, cin)).astype(np.float32)
    return cfg, w, x


def _sha(a):
    a = np.ascontiguousarray(a)
    return hashlib.sha256(str(a.dtype).encode() + str(a.shape).encode() + a.tobytes()).hexdigest()


def layer_digest(handle, case, act, winograd):
    from ecseg_amd import keras_plan
    cfg, w, x = layer_model(case, act)
    handle.set_option('winograd', winograd)
    try:
        handle.load_plan(keras_plan.build_plan(cfg, w, fuse=True))
        return _sha(handle.forward_patches(x))
    finally:
        handle.set_option('winograd', 2)


def crop_digest(handle, winograd):
    """Raw labels and probabilities of one small image through the cropped plan of a base-64, depth-1 U-Net."""
    from ecseg_amd import keras_plan, synth
    cfg = synth.unet_config(base=64, depth=1)
    weights = synth.unet_weights(cfg, seed=3)
    img = synth.dapi_image(7, *CROP_IMAGE)
    handle.set_option('winograd', winograd)
    handle.set_option('crop', 1)
    try:
        handle.load_plan(keras_plan.build_plan(cfg, weights, fuse=True))
        raw, post, nec, probs = handle.segment_images(img[None], want_raw=True, want_probs=True)
        return _sha(probs) + _sha(raw)
    finally:
        handle.set_option('winograd', 2)


def all_keys():
    return ['%s/%s/winograd%d' % (c, a, wg) for c in LAYERS for a in ACTS for wg in WINOGRAD] + ['crop/winograd%d' % wg for wg in WINOGRAD]


def digest(handle, key):
    parts = key.split('/')
    if parts[0] == 'crop':
        return crop_digest(handle, int(parts[1][len('winograd'):]))
    return layer_digest(handle, parts[0], parts[1], int(parts[2][len('winograd'):]))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--write', action='store_true', help='write tests/golden/wino4_layer_digests.json (default: compare with it)')
    ap.add_argument('--out', default=GOLDEN)
    ap.add_argument('--kinds', action='store_true', help='print which kernel ran each launch (kind, fused pool / head bits, computed fraction of a cropped launch)')
    a = ap.parse_args()
    from ecseg_amd._lib import LIB_PATH, Handle
    h = Handle(0)
    try:
        got = {}
        if a.kinds:
            h.set_kernel_profiling(True)
        for k in all_keys():
            got[k] = digest(h, k)
            if a.kinds:
                print(k, ['kind 0x%x computed %.2f' % (r['kind'], r['executed_flops'] / max(r['flops'] * (0.25 if (r['kind'] & 255) in (2, 5, 6) else 1.0), 1.0))
                          for r in h.conv_launch_profile()], flush=True)
    finally:
        h.close()
    if a.write:
        with open(a.out, 'w') as f:
            json.dump({'digests': got}, f, indent=1, sort_keys=True)
            f.write('\n')
        print('wrote %d digests of %s to %s' % (len(got), LIB_PATH, a.out))
        return 0
    with open(a.out) as f:
        want = json.load(f)['digests']
    bad = [k for k in all_keys() if got[k] != want.get(k)]
    print('%d of %d digests differ%s' % (len(bad), len(got), ': ' + ', '.join(bad) if bad else ''))
    return 1 if bad else 0


if __name__ == '__main__':
    sys.exit(main())
