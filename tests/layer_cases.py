"""The cases of tests/test_layers_ref.py (CPU) and tests/test_gpu_layers.py (device): one Keras config per case with an
InputLayer, the op under test and nothing after it.  TEST INFRASTRUCTURE ONLY.

A plan takes one input, so a second operand of a merge layer is made from the input by layers that are EXACT in float32: a
shifted copy (ZeroPadding2D + Cropping2D), the (1, 1, c) channel maxima (GlobalMaxPooling2D, keepdims) and an (h, w, k)
channel selection (a bias-free 1x1 Conv2D whose kernel is one-hot: every product is x * 1 or x * 0).  The strided-view cases
put the op between two fused Concatenates made of such copies.

A case is a dict: ``name``, ``group``, ``cfg``, ``weights``, ``x`` (float32 NHWC), ``kind`` (the op and what its bound needs:
tests/test_gpu_layers.py) and ``fuses`` (the ``fuse`` values of ``build_plan`` to run it with).  Parameters that the device
receives as float32 scalars (alpha, max_value, slopes) are chosen so that float32 holds them exactly; epsilon enters float64
arithmetic on the host (BatchNormalization) or is rounded once (LayerNormalization: counted in its bound).

``all_cases()`` = the hand-made groups + ``random_case(seed)`` over ``RANDOM_SEEDS``.
"""
import zlib

import numpy as np

GROUPS = ('pool_valid', 'pool_same', 'global_pool', 'upsample', 'pad_crop', 'merge', 'prelu', 'batchnorm', 'layernorm', 'softmax',
          'activation', 'strided')
RANDOM_SEEDS = range(40)


def _L(cls, name, inbound, **cfg):
    return {'class_name': cls, 'name': name, 'config': dict(cfg, name=name),
            'inbound_nodes': [[[i, 0, 0, {}] for i in inbound]] if inbound else []}


def _F(layers, outs, name='m'):
    return {'class_name': 'Functional', 'config': {'name': name, 'layers': layers, 'input_layers': [['in', 0, 0]],
                                                   'output_layers': [[o, 0, 0] for o in outs]}}


def _in(h, w, c):
    return _L('InputLayer', 'in', [], batch_input_shape=[None, h, w, c])


def _rng(name):
    return np.random.default_rng(zlib.crc32(name.encode()))


def _case(name, group, layers, weights, x, kind, fuses=(True,)):
    return dict(name=name, group=group, cfg=_F(layers, [layers[-1]['config']['name']]), weights=weights,
                x=np.ascontiguousarray(x, np.float32), kind=kind, fuses=tuple(fuses))


def _f32(a):
    return np.ascontiguousarray(a, np.float32)


# ---- pooling ---------------------------------------------------------------------------------------------------------
def pool_case(group, avg, padding, k, s, N, H, W, C, tag=''):
    name = '%s_%s_k%d_s%d_%dx%dx%dx%d%s' % ('avg' if avg else 'max', padding, k, s, N, H, W, C, tag)
    x = _rng(name).normal(size=(N, H, W, C))
    layers = [_in(H, W, C), _L('AveragePooling2D' if avg else 'MaxPooling2D', 'op', ['in'], pool_size=[k, k], strides=[s, s], padding=padding)]
    return _case(name, group, layers, {}, x, dict(op='avgpool' if avg else 'select', k=k, padding=padding))


def pool_valid_cases():
    out = []
    for avg in (False, True):
        for k in (2, 3):
            for s in (1, 2, 3):
                # the extent equal to the window on one axis, a stride remainder on the other ((H - k) % s = 1 for s > 1);
                # C = 5: scalar kernel
                out.append(pool_case('pool_valid', avg, 'valid', k, s, 2, k, k + 2 * s + 1, 5))
                # C = 8: the f32x4 kernel, several windows, remainders on both axes
                out.append(pool_case('pool_valid', avg, 'valid', k, s, 1, k + 3 * s + (1 if s > 1 else 0), 11 + (s == 3), 8))
    return out


SAME_EXTENTS = ((1, 1), (2, 2), (5, 7), (7, 33), (33, 5), (1, 5), (2, 33), (33, 1))


def pool_same_cases():
    out = [pool_case('pool_same', True, 'same', 5, 1, 1, 2, 2, 3, '_divides_by_4')]      # every window holds the whole 2 x 2 image
    q = 0
    for avg in (False, True):
        for k in (2, 3, 5):
            for s in (1, 2, 3):
                for _ in range(2):
                    H, W = SAME_EXTENTS[q % len(SAME_EXTENTS)]
                    out.append(pool_case('pool_same', avg, 'same', k, s, 1 + q % 2, H, W, (3, 4, 8, 1)[q % 4]))
                    q += 3
    return out


GLOBAL_C = (1, 3, 64, 65, 130)
GLOBAL_HW = ((1, 1), (1, 3), (2, 2), (5, 1), (35, 37))


def global_case(avg, H, W, C, N=2, keepdims=False, flavour='plain', tag=''):
    name = 'global_%s_%dx%dx%dx%d_%s%s%s' % ('avg' if avg else 'max', N, H, W, C, flavour, '_keep' if keepdims else '', tag)
    x = _rng(name).normal(size=(N, H, W, C))
    if flavour == 'negative':            # a maximum that starts at 0 would win
        x = -np.abs(x) - 0.5
    elif flavour == 'offset':            # mean 1e3: a sum that loses low bits with the pixel count shows
        x = x + 1e3
    layers = [_in(H, W, C), _L('GlobalAveragePooling2D' if avg else 'GlobalMaxPooling2D', 'op', ['in'], keepdims=keepdims)]
    return _case(name, 'global_pool', layers, {}, x, dict(op='global_avg' if avg else 'select', npx=H * W))


def global_pool_cases():
    out = []
    for ci, C in enumerate(GLOBAL_C):
        for hi, (H, W) in enumerate(GLOBAL_HW):
            q = ci + hi
            out.append(global_case(False, H, W, C, keepdims=bool(q % 2), flavour='negative' if q % 3 else 'plain'))
            out.append(global_case(True, H, W, C, keepdims=not q % 2, flavour='offset' if q % 3 else 'plain'))
    return out


# ---- resampling ------------------------------------------------------------------------------------------------------
UP_SHAPES = ((1, 1), (1, 5), (5, 1), (3, 4), (17, 9))


def upsample_case(interp, f, H, W, C, N=2, tag=''):
    name = 'up_%s_f%d_%dx%dx%dx%d%s' % (interp, f, N, H, W, C, tag)
    x = _rng(name).normal(size=(N, H, W, C))
    layers = [_in(H, W, C), _L('UpSampling2D', 'op', ['in'], size=[f, f], interpolation=interp)]
    return _case(name, 'upsample', layers, {}, x, dict(op='bilinear', f=f, h=H, w=W) if interp == 'bilinear' else dict(op='select'))


def upsample_cases():
    out, q = [], 0
    for interp in ('nearest', 'bilinear'):
        for f in (2, 3, 4):
            for (H, W) in UP_SHAPES:
                out.append(upsample_case(interp, f, H, W, (1, 4, 5)[q % 3], N=1 + q % 2))
                q += 1
    return out


def pad_crop_cases():
    out = []
    for cls, key, val, (H, W, C) in (('ZeroPadding2D', 'padding', [[0, 3], [2, 0]], (5, 4, 3)), ('ZeroPadding2D', 'padding', [[2, 1], [0, 5]], (1, 1, 8)),
                                     ('ZeroPadding2D', 'padding', [[1, 1], [1, 1]], (7, 9, 5)), ('Cropping2D', 'cropping', [[0, 3], [2, 0]], (9, 7, 3)),
                                     ('Cropping2D', 'cropping', [[3, 1], [0, 6]], (5, 7, 5)),          # down to 1 x 1
                                     ('Cropping2D', 'cropping', [[1, 0], [0, 2]], (6, 8, 4))):
        name = '%s_%s_%dx%dx%d' % (cls, '_'.join(str(v) for p in val for v in p), H, W, C)
        x = _rng(name).normal(size=(2, H, W, C))
        out.append(_case(name, 'pad_crop', [_in(H, W, C), _L(cls, 'op', ['in'], **{key: val})], {}, x, dict(op='select')))
    return out


# ---- merge layers ----------------------------------------------------------------------------------------------------
def _shifted(name):
    """The input moved down by one row (zeros come in at the top): an exact second operand of the input's shape."""
    return [_L('ZeroPadding2D', name + '_p', ['in'], padding=[[1, 0], [0, 0]]), _L('Cropping2D', name, [name + '_p'], cropping=[[0, 1], [0, 0]])]


def _onehot(name, src, cin, picks):
    """(h, w, len(picks)): channel picks[j] of ``src`` as output channel j - a bias-free 1x1 Conv2D with a one-hot kernel."""
    k = np.zeros((1, 1, cin, len(picks)), np.float32)
    for j, p in enumerate(picks):
        k[0, 0, p, j] = 1.0
    return _L('Conv2D', name, [src], filters=len(picks), kernel_size=[1, 1], strides=[1, 1], padding='same', activation='linear', use_bias=False), {name: [k]}


MERGE_PATTERNS = ('equal', 'hw1_second', 'hw1_first', 'c_second', 'c_first')


def merge_case(cls, pattern, H, W, C, N=2, third=None, tag=''):
    name = 'merge_%s_%s%s_%dx%dx%dx%d%s' % (cls, pattern, '_' + third if third else '', N, H, W, C, tag)
    rng = _rng(name)
    if cls in ('Maximum', 'Minimum'):                            # ties and signed zeros
        x = rng.choice(np.array([-1.5, -0.0, 0.0, 0.25, 1.0, 1.0, -1.5, 3.0]), size=(N, H, W, C))
    else:
        x = rng.normal(size=(N, H, W, C))
    layers, weights = [_in(H, W, C)], {}

    def operand(kind, nm):
        if kind == 'shift':
            layers.extend(_shifted(nm))
        elif kind == 'hw1':
            L, w = _onehot(nm, 'in', C, [C - 1])
            layers.append(L)
            weights.update(w)
        else:
            layers.append(_L('GlobalMaxPooling2D', nm, ['in'], keepdims=True))
        return nm

    if pattern == 'equal':
        ops = ['in', operand('shift', 'b')]
    elif pattern.startswith('hw1'):
        ops = ['in', operand('hw1', 'b')]
    else:
        ops = ['in', operand('c', 'b')]
    if pattern.endswith('first'):
        ops.reverse()
    if third:
        ops.append(operand(third, 'c'))
    layers.append(_L(cls, 'op', ops))
    if cls in ('Maximum', 'Minimum'):
        kind = dict(op='select')
    elif cls == 'Average':
        kind = dict(op='sum', n_ops=len(ops) - 1 + 2)            # n - 1 additions, the rounding of 1 / n, one multiplication
    elif cls == 'Multiply' or len(ops) == 2:
        kind = dict(op='round1')
    else:
        kind = dict(op='sum', n_ops=len(ops) - 1)
    return _case(name, 'merge', layers, weights, x, kind)


def merge_cases():
    out, q = [], 0
    for cls in ('Add', 'Subtract', 'Multiply', 'Maximum', 'Minimum'):
        for pattern in MERGE_PATTERNS:
            out.append(merge_case(cls, pattern, 5 + q % 3, 7 - q % 2, (3, 4, 20)[q % 3]))
            q += 1
    for pattern, third in (('equal', 'c'), ('hw1_first', 'shift'), ('c_second', 'hw1')):
        for cls in ('Maximum', 'Average', 'Add'):
            out.append(merge_case(cls, pattern, 6, 5, (3, 4, 20)[q % 3], third=third))
            q += 1
    out.append(merge_case('Average', 'equal', 4, 9, 4))
    out.append(merge_case('Average', 'c_first', 4, 9, 3))
    return out


# ---- Add of two same-shape inputs, bit for bit -----------------------------------------------------------------------------
# (a, b) pairs that meet in one element: signed zeros, values that cancel to 0, large values (a finite sum, an overflow), infinities
# beside finite values and beside their own sign.  No inf + -inf (NaN) and no denormals.
ADD_EXACT_PAIRS = ((0.0, 0.0), (-0.0, -0.0), (0.0, -0.0), (-0.0, 0.0), (1.5, -1.5), (-2.75e-3, 2.75e-3), (1e38, 1e38), (3e38, 3e38),
                   (-3e38, -3e38), (3e38, -3e38), (1e30, 1.0), (np.inf, 1.0), (-np.inf, -1.0), (np.inf, np.inf), (-np.inf, -np.inf),
                   (np.inf, -3e38), (1.0, np.inf))


def add_exact_case(C, view=False, N=2, H=5, W=7):
    """Add([a, b]) with a = the input (or an exact copy of it) and b = the input moved down a row (``_shifted``), so element
    (y, x, c) adds x[y] and x[y - 1], and row 0 adds +0.  Rows 1 and 0 of image 0 hold ``ADD_EXACT_PAIRS``, over and over; the
    rest is random.  ``view``: a is the member at channel offset 2 of a 12-channel Concatenate - stride and channel count are
    multiples of 4 and only the pointer is not 16-byte aligned; the members beside it are channel selections of the input
    clipped to [0, 1] (finite, so that their one-hot products are)."""
    name = 'add_exact_c%d%s' % (C, '_view' if view else '')
    x = _f32(_rng(name).normal(size=(N, H, W, C)))
    pairs = np.array(ADD_EXACT_PAIRS, np.float32)
    idx = np.arange(W * C) % len(pairs)
    x[0, 1] = pairs[idx, 0].reshape(W, C)
    x[0, 0] = pairs[idx, 1].reshape(W, C)
    layers, weights, a = [_in(H, W, C)], {}, 'in'
    if view:
        layers.append(_L('ReLU', 'f', ['in'], max_value=1.0, negative_slope=0.0, threshold=0.0))
        (Ls, ws), (Lt, wt) = _onehot('s', 'f', C, [0, 1]), _onehot('t', 'f', C, [3, 2])
        layers.extend([Ls, _L('ZeroPadding2D', 'a', ['in'], padding=[[0, 0], [0, 0]]), Lt, _L('Concatenate', 'cat1', ['s', 'a', 't'], axis=-1)])
        weights.update(ws, **wt)
        a = 'a'
    layers.extend(_shifted('b'))
    layers.append(_L('Add', 'op', [a, 'b']))
    # vector: launch_binary's test - every view of the op has all channels, a multiple of 4 of them, and is 16-byte aligned
    return _case(name, 'add_exact', layers, weights, x, dict(op='add_exact', vector=C % 4 == 0 and not view, view=view))


def add_exact_operands(case):
    """-> (a, b) float32, the two operands of the case's Add as the layers above make them."""
    a = case['x']
    b = np.zeros_like(a)
    b[:, 1:] = a[:, :-1]
    return a, b


def add_exact_cases():
    return [add_exact_case(8), add_exact_case(6), add_exact_case(8, view=True)]


# ---- PReLU -----------------------------------------------------------------------------------------------------------
PRELU_SHARED = (None, [1], [2], [3], [1, 2], [1, 3], [2, 3], [1, 2, 3])


def prelu_alpha_shape(shared, H, W, C):
    return tuple(1 if (a + 1) in (shared or []) else v for a, v in enumerate((H, W, C)))


def prelu_case(shared, H, W, C, N=2, tag=''):
    name = 'prelu_%s_%dx%dx%dx%d%s' % ('none' if shared is None else ''.join(str(a) for a in shared), N, H, W, C, tag)
    rng = _rng(name)
    x = rng.normal(size=(N, H, W, C))
    shp = prelu_alpha_shape(shared, H, W, C)
    alpha = rng.choice(np.array([-0.75, 0.0, 0.1, 0.25, 1.0, 1.75, 3.0], np.float32), size=shp).astype(np.float32)      # negative, zero, above 1
    layers = [_in(H, W, C), _L('PReLU', 'op', ['in'], shared_axes=shared)]
    return _case(name, 'prelu', layers, {'op': [alpha]}, x, dict(op='round1'))


def prelu_cases():
    return [prelu_case(sh, 5, 7, (3, 4, 5)[q % 3]) for q, sh in enumerate(PRELU_SHARED)]


# ---- BatchNormalization / Normalization --------------------------------------------------------------------------------
def bn_case(eps, center, scale, H, W, C, N=2, tag=''):
    name = 'bn_eps%g_%s%s_%dx%dx%dx%d%s' % (eps, 'c' if center else '', 's' if scale else '', N, H, W, C, tag)
    rng = _rng(name)
    x = rng.normal(size=(N, H, W, C))
    var = (10.0 ** rng.uniform(-4, 0.3, C)).astype(np.float32)
    var[0] = 1e-4                                               # the epsilon decides the scale of this channel
    w = ([_f32(rng.uniform(.5, 1.5, C))] if scale else []) + ([_f32(rng.normal(size=C))] if center else []) + [_f32(rng.normal(size=C)), var]
    layers = [_in(H, W, C), _L('BatchNormalization', 'op', ['in'], axis=[3], epsilon=eps, center=center, scale=scale)]
    return _case(name, 'batchnorm', layers, {'op': w}, x, dict(op='affine'))


def norm_case(H, W, C, N=2):
    name = 'normalization_%dx%dx%dx%d' % (N, H, W, C)
    rng = _rng(name)
    x = rng.normal(size=(N, H, W, C)) * 3 + 1
    var = (10.0 ** rng.uniform(-4, 0.3, C)).astype(np.float32)
    w = [_f32(rng.normal(size=C)), var, np.array(5, np.int64)]
    layers = [_in(H, W, C), _L('Normalization', 'op', ['in'], axis=[-1], mean=None, variance=None)]
    return _case(name, 'batchnorm', layers, {'op': w}, x, dict(op='affine'))


def batchnorm_cases():
    out, q = [], 0
    for eps in (1e-3, 1e-5):
        for center in (True, False):
            for scale in (True, False):
                out.append(bn_case(eps, center, scale, 4 + q % 2, 5, (3, 4, 5, 8)[q % 4]))
                q += 1
    return out + [norm_case(5, 4, 3), norm_case(3, 3, 8)]


# ---- LayerNormalization ----------------------------------------------------------------------------------------------
LN_C = (1, 3, 15, 16, 17, 63, 64, 65, 100)
LN_NPIX = ((1, 1, 1), (1, 5, 1), (1, 1, 17), (67, 1, 1))       # N, H, W: the last wave holds fewer live pixels than slots


def ln_case(C, nhw, eps, offset, center=True, scale=True, tag=''):
    N, H, W = nhw
    name = 'ln_c%d_%dx%dx%d_eps%g_mean%g%s%s%s' % (C, N, H, W, eps, offset, '' if center else '_nocentre', '' if scale else '_noscale', tag)
    rng = _rng(name)
    x = rng.normal(size=(N, H, W, C)) + offset
    if N * H * W > 1:
        x[-1, -1, -1, :] = 2.5                                  # a constant pixel: the variance is exactly 0
    w = ([_f32(rng.uniform(.5, 1.5, C))] if scale else []) + ([_f32(rng.normal(size=C))] if center else [])
    layers = [_in(H, W, C), _L('LayerNormalization', 'op', ['in'], axis=[3], epsilon=eps, center=center, scale=scale)]
    return _case(name, 'layernorm', layers, {'op': w}, x, dict(op='layernorm', c=C))


def layernorm_cases():
    out = []
    for q, C in enumerate(LN_C):
        out.append(ln_case(C, LN_NPIX[q % 4], (1e-3, 1e-5)[q % 2], 0.0, center=q % 3 != 1, scale=q % 3 != 2))
        out.append(ln_case(C, LN_NPIX[(q + 2) % 4], (1e-5, 1e-3)[q % 2], 1e3))
    out.append(ln_case(1, (1, 1, 1), 1e-5, 0.0))               # one channel, one pixel: the output is beta
    out.append(ln_case(100, (67, 1, 1), 1e-3, 0.0))
    out.append(ln_case(63, (67, 1, 1), 1e-3, 0.0))
    out.append(ln_case(3, (1, 1, 17), 1e-3, 0.0))
    return out


# ---- Softmax ---------------------------------------------------------------------------------------------------------
def softmax_case(C, as_activation=False, N=1, tag=''):
    name = 'softmax_c%d_n%d%s%s' % (C, N, '_activation' if as_activation else '', tag)
    rng = _rng(name)
    P = 4 * N                                                                                      # pixels per kind of row
    rows = [np.full((P, C), 3.25), np.full((P, C), -80.0),                                       # all equal
            np.where(np.arange(C)[None, :] == rng.integers(0, C, P)[:, None], 80.0, 0.0) + rng.normal(size=(P, C)),   # one 80 above
            rng.uniform(-80, 80, (P, C)), rng.choice([-80.0, 0.0, 80.0], (P, C)),                 # spread over +-80
            rng.choice([-2.0, 0.5, 0.5, 7.0], (P, C)),                                            # exact ties
            rng.normal(size=(P, C))]
    x = np.stack(rows).reshape(len(rows), N, 4, C).transpose(1, 0, 2, 3)                           # every image holds every kind
    op = _L('Activation', 'op', ['in'], activation='softmax') if as_activation else _L('Softmax', 'op', ['in'], axis=-1)
    return _case(name, 'softmax', [_in(len(rows), 4, C), op], {}, x, dict(op='softmax', c=C))


def softmax_cases():
    return [softmax_case(C) for C in (1, 2, 3, 4, 5, 33)] + [softmax_case(4, as_activation=True)]


# ---- activations -----------------------------------------------------------------------------------------------------
ACTIVATION_NAMES = ('linear', 'relu', 'relu6', 'sigmoid', 'tanh', 'elu', 'selu', 'softplus', 'softsign', 'swish', 'silu', 'gelu',
                    'hard_sigmoid', 'exponential')
EXP_MAX = 88.72          # exp(float32(88.72)) = 3.3935e38 < FLT_MAX = 3.4028e38 = exp(88.7228...): the float32 overflow point


def sweep(limit=90.0):
    """The fixed input of every activation case: 321 points of [-8, 8] (step 0.05), +-1e-6, +-1e-3, +-20, +-50, +-88, +-limit, +-0."""
    special = [1e-6, 1e-3, 20.0, 50.0, 88.0, limit, 0.0]
    v = np.concatenate([np.linspace(-8.0, 8.0, 321), special, [-s for s in special]])
    return v.astype(np.float32).reshape(1, 1, -1, 1)


def act_case(name, layer, fn, alpha=None):
    x = sweep(EXP_MAX if fn == 'exponential' else 90.0)
    return _case(name, 'activation', [_in(1, x.shape[2], 1), layer], {}, x, dict(op='act', fn=fn, alpha=alpha))


def activation_cases():
    out = [act_case('act_' + n, _L('Activation', 'op', ['in'], activation=n), n) for n in ACTIVATION_NAMES]
    out.append(act_case('elu_layer_0.625', _L('ELU', 'op', ['in'], alpha=0.625), 'elu', 0.625))
    out.append(act_case('elu_layer_1.5', _L('ELU', 'op', ['in'], alpha=1.5), 'elu', 1.5))
    out.append(act_case('relu_layer', _L('ReLU', 'op', ['in'], max_value=None, negative_slope=0.0, threshold=0.0), 'relu'))
    out.append(act_case('relu_layer_max2.5', _L('ReLU', 'op', ['in'], max_value=2.5, negative_slope=0.0, threshold=0.0), 'relu_clip', 2.5))
    out.append(act_case('relu_layer_slope0.125', _L('ReLU', 'op', ['in'], max_value=None, negative_slope=0.125, threshold=0.0), 'leaky_relu', 0.125))
    out.append(act_case('leaky_0.25', _L('LeakyReLU', 'op', ['in'], alpha=0.25), 'leaky_relu', 0.25))
    out.append(act_case('leaky_0.0078125', _L('LeakyReLU', 'op', ['in'], alpha=0.0078125), 'leaky_relu', 0.0078125))
    return out


# ---- strided channel views -------------------------------------------------------------------------------------------
STRIDED_OPS = ('maxpool', 'bilinear', 'affine', 'prelu', 'multiply', 'layernorm', 'softmax', 'copy')


def strided_case(op, H=6, W=8, N=2):
    """in (4 channels) -> cat1 = Concatenate([a (4), s (2), b (4), t (2)]) of exact copies / channel selections of the input: the
    members are written into the concatenated buffer (channel stride 12, offsets 0, 4, 6, 10).  The op under test runs on each
    member - reading offset 0 and 6 with 4 channels (16-byte aligned, and not), offset 4 and 10 with 2 - and its four outputs
    are the members of cat2, so it writes strided views too.  A zero Cropping2D copies cat2 out."""
    name = 'strided_' + op
    rng = _rng(name)
    x = rng.normal(size=(N, H, W, 4))
    (Ls, ws), (Lt, wt) = _onehot('s', 'in', 4, [0, 1]), _onehot('t', 'in', 4, [3, 2])
    layers = [_in(H, W, 4), _L('ZeroPadding2D', 'a', ['in'], padding=[[0, 0], [0, 0]]), Ls,
              _L('Cropping2D', 'b', ['in'], cropping=[[0, 0], [0, 0]]), Lt]
    weights = dict(ws, **wt)
    members = ['a', 's', 'b', 't']
    layers.append(_L('Concatenate', 'cat1', members, axis=-1))
    outs = []
    for src, c in zip(members, (4, 2, 4, 2)):
        nm = 'op_' + src
        if op == 'maxpool':
            layers.append(_L('MaxPooling2D', nm, [src], pool_size=[2, 2], strides=[2, 2], padding='valid'))
        elif op == 'bilinear':
            layers.append(_L('UpSampling2D', nm, [src], size=[2, 2], interpolation='bilinear'))
        elif op == 'affine':
            layers.append(_L('BatchNormalization', nm, [src], axis=[3], epsilon=1e-3, center=True, scale=True))
            weights[nm] = [_f32(rng.uniform(.5, 1.5, c)), _f32(rng.normal(size=c)), _f32(rng.normal(size=c)), _f32(rng.uniform(.5, 1.5, c))]
        elif op == 'prelu':
            layers.append(_L('PReLU', nm, [src], shared_axes=[1, 2]))
            weights[nm] = [_f32(rng.choice([-0.75, 0.25, 1.75], size=(1, 1, c)))]
        elif op == 'multiply':
            layers.append(_L('Multiply', nm, [src, {'a': 'b', 'b': 'a', 's': 't', 't': 's'}[src]]))
        elif op == 'layernorm':
            layers.append(_L('LayerNormalization', nm, [src], axis=[3], epsilon=1e-3, center=True, scale=True))
            weights[nm] = [_f32(rng.uniform(.5, 1.5, c)), _f32(rng.normal(size=c))]
        elif op == 'softmax':
            layers.append(_L('Softmax', nm, [src], axis=-1))
        elif op == 'copy':
            layers.append(_L('ZeroPadding2D', nm, [src], padding=[[1, 0], [0, 2]]))
        else:
            raise ValueError(op)
        outs.append(nm)
    layers.append(_L('Concatenate', 'cat2', outs, axis=-1))
    layers.append(_L('Cropping2D', 'out', ['cat2'], cropping=[[0, 0], [0, 0]]))
    member_c = np.repeat((4, 2, 4, 2), (4, 2, 4, 2))          # per output channel: the channel count of the member it belongs to
    kind = {'maxpool': dict(op='select'), 'bilinear': dict(op='bilinear', f=2, h=H, w=W), 'affine': dict(op='affine'), 'prelu': dict(op='round1'),
            'multiply': dict(op='round1'), 'layernorm': dict(op='layernorm', c=member_c), 'softmax': dict(op='softmax', c=member_c), 'copy': dict(op='select')}[op]
    return _case(name, 'strided', layers, weights, x, dict(kind, strided=op), fuses=(True, False))


def strided_cases():
    return [strided_case(op) for op in STRIDED_OPS]


STRIDED_OP_CODE = {'maxpool': 'OP_MAXPOOL', 'bilinear': 'OP_UPSAMPLE', 'affine': 'OP_AFFINE', 'prelu': 'OP_PRELU', 'multiply': 'OP_ADD',
                   'layernorm': 'OP_LAYERNORM', 'softmax': 'OP_ACT', 'copy': 'OP_COPY'}


def strided_views(plan, op, codes):
    """-> (channel offsets of the strided views that the instances of the op under test read, ... write) in a lowered plan;
    ``codes``: the module that names the op codes (ecseg_amd.keras_plan)."""
    reads, writes = [], []
    for o in plan.ops:
        if o['op'] != getattr(codes, STRIDED_OP_CODE[op]):
            continue
        if op == 'copy' and (o['pad_top'], o['pad_left']) == (0, 0):
            continue                                            # the copies that build the views, not the op under test
        ti, to = plan.tensors[o['in0']], plan.tensors[o['out']]
        if ti['c_stride'] != ti['c']:
            reads.append(ti['c_offset'])
        if to['c_stride'] != to['c']:
            writes.append(to['c_offset'])
    return reads, writes


# ---- the seeded range ------------------------------------------------------------------------------------------------
def random_case(seed):
    """Op, shape, C and N drawn from the lists above."""
    rng = np.random.default_rng(seed)
    pick = lambda seq: seq[int(rng.integers(0, len(seq)))]
    op = pick(('pool_valid', 'pool_same', 'global_pool', 'upsample', 'merge', 'prelu', 'batchnorm', 'layernorm', 'softmax'))
    N = int(rng.integers(1, 4))
    C = pick((1, 3, 4, 5, 20))
    tag = '_seed%d' % seed
    if op == 'pool_valid':
        k, s = pick((2, 3)), pick((1, 2, 3))
        c = pool_case('random', bool(rng.integers(0, 2)), 'valid', k, s, N, k + int(rng.integers(0, 9)), k + int(rng.integers(0, 9)), C, tag)
    elif op == 'pool_same':
        H, W = pick(SAME_EXTENTS)
        c = pool_case('random', bool(rng.integers(0, 2)), 'same', pick((2, 3, 5)), pick((1, 2, 3)), N, H, W, C, tag)
    elif op == 'global_pool':
        H, W = pick(GLOBAL_HW)
        c = global_case(bool(rng.integers(0, 2)), H, W, pick(GLOBAL_C), N=N, keepdims=bool(rng.integers(0, 2)), flavour=pick(('plain', 'negative', 'offset')),
                        tag=tag)
    elif op == 'upsample':
        H, W = pick(UP_SHAPES)
        c = upsample_case(pick(('nearest', 'bilinear')), pick((2, 3, 4)), H, W, pick((1, 4, 5)), N=N, tag=tag)
    elif op == 'merge':
        c = merge_case(pick(('Add', 'Subtract', 'Multiply', 'Maximum', 'Minimum', 'Average')), pick(MERGE_PATTERNS), int(rng.integers(2, 9)),
                       int(rng.integers(2, 9)), pick((3, 4, 20)), N=N, tag=tag)
    elif op == 'prelu':
        c = prelu_case(pick(PRELU_SHARED), int(rng.integers(1, 9)), int(rng.integers(1, 9)), C, N=N, tag=tag)
    elif op == 'batchnorm':
        c = bn_case(pick((1e-3, 1e-5)), bool(rng.integers(0, 2)), bool(rng.integers(0, 2)), int(rng.integers(1, 9)), int(rng.integers(1, 9)), C, N=N, tag=tag)
    elif op == 'layernorm':
        _, H, W = pick(LN_NPIX[:3])                               # 1, 5 or 17 pixels per image, N images
        c = ln_case(pick(LN_C), (N, H, W), pick((1e-3, 1e-5)), pick((0.0, 1e3)), tag=tag)
    else:
        c = softmax_case(pick((1, 2, 3, 4, 5, 33)), N=N, tag=tag)
    return dict(c, name='random%02d_%s' % (seed, c['name']), group='random')


def group_cases(group):
    if group == 'random':
        return [random_case(s) for s in RANDOM_SEEDS]
    return {'pool_valid': pool_valid_cases, 'pool_same': pool_same_cases, 'global_pool': global_pool_cases, 'upsample': upsample_cases,
            'pad_crop': pad_crop_cases, 'merge': merge_cases, 'prelu': prelu_cases, 'batchnorm': batchnorm_cases, 'layernorm': layernorm_cases,
            'softmax': softmax_cases, 'activation': activation_cases, 'strided': strided_cases}[group]()


def all_cases():
    return [c for g in GROUPS + ('random',) for c in group_cases(g)]
