"""Small Keras graphs aimed at one rewrite of ``ecseg_amd/keras_plan.py::build_plan`` each, and a seeded generator of random ones,
for tests/test_plan_ref.py (CPU) and tests/test_gpu_plan.py (device).  TEST INFRASTRUCTURE ONLY; imports nothing from ``ecseg_amd``.

A case is a dict: ``name`` (after its rewrite), ``group``, ``cfg`` / ``weights`` (Keras ``model_config`` and ``{layer: [arrays]}``),
``x`` (batch 2, in the layout the Keras model takes; uint8 where the graph starts with an input normalisation, float32 otherwise),
``lambda_affine`` ({Lambda layer: (scale, offset)}), ``keep`` / ``output`` (the arguments of ``build_plan``), and what the plan's own
record must show with ``fuse=True``:

* ``fused``: [(layer, convolution it disappears into)] - both names map to one tensor in ``Plan.layer_tensor``;
* ``unfused``: [(layer, producer)] - the layer keeps a tensor and an op of its own (the "must not fold" cases);
* ``folded_up``: [(UpSampling2D, convolution)] - the convolution became a transposed one and carries the ``also`` note;
* ``views``: {layer: (channel offset, channel stride)} of a tensor written straight into a concatenation;
* ``copies``: explicit OP_COPY ops of concatenation inputs that cannot be views;
* ``count_ops``: the op count is ``layers that compute - len(fused) - len(folded_up)`` (and ``layers that compute`` with
  ``fuse=False``); False for shared / nested graphs, whose layer list is not their call list;
* ``fewer_buffers``: the allocator re-uses (buffers < tensors).

The bound of both test files, per output element:  |result - y| <= C_BOUND * 2^-24 * A,  with (y, A) of tests/plan_ref.py.
"""
import numpy as np

U = 2.0 ** -24
# Measured on the CPU (tests/test_plan_ref.py::test_float32_oracle_within_bound prints it): the largest |f32 - y| / (2^-24 A) of
# oracle/unet.py's float32 forward over every committed case, seed and checked tensor is C_MEASURED.  Times 4 for the device's other
# summation orders and its Winograd paths, rounded up to a power of two.
C_MEASURED = 4.52
C_BOUND = 32.0
N_SEEDS = 40
KILL = 10.0               # a mutant is killed where it moves an element by more than KILL * C_BOUND * 2^-24 * A

SPATIAL = ('Conv2D', 'Conv2DTranspose', 'DepthwiseConv2D', 'SeparableConv2D', 'MaxPooling2D', 'AveragePooling2D', 'UpSampling2D',
           'ZeroPadding2D', 'Cropping2D')
NO_OP_CLASSES = ('InputLayer', 'Concatenate', 'Dropout', 'SpatialDropout2D', 'Flatten', 'Reshape')


def _same_out(n, s):
    return -(-n // s)


class G:
    """Builds a Functional config, its weights and an input, tracking (h, w, c) per tensor.  Every method returns the tensor's name."""

    def __init__(self, seed, h, w, c, u8=False, cf=False):
        self.rng = np.random.default_rng(seed)
        self.layers, self.weights, self.shape, self.cf, self.n = [], {}, {}, cf, 0
        self._add('InputLayer', 'in', [], (h, w, c), batch_input_shape=[None, c, h, w] if cf else [None, h, w, c])
        if u8:
            x = self.rng.integers(0, 256, size=(2, h, w, c), dtype=np.uint8)
        else:
            x = self.rng.normal(size=(2, h, w, c)).astype(np.float32)
        self.x = np.ascontiguousarray(np.transpose(x, (0, 3, 1, 2))) if cf else x

    @staticmethod
    def _ref(s):
        if '/call' in s:
            nm, j = s.rsplit('/call', 1)
            return [nm, int(j), 0, {}]
        return [s, 0, 0, {}]

    def _add(self, cls, name, srcs, shape, **cfg):
        if self.cf and cls in SPATIAL:
            cfg['data_format'] = 'channels_first'
        self.layers.append({'class_name': cls, 'name': name, 'config': dict(cfg, name=name),
                            'inbound_nodes': [[self._ref(s) for s in srcs]] if srcs else []})
        self.shape[name] = tuple(shape)
        return name

    def _name(self, stem, name):
        self.n += 1
        return name or '%s%d' % (stem, self.n)

    def f32(self, a):
        return np.ascontiguousarray(a, np.float32)

    def _kernel(self, shape, fan_in):
        return self.f32(self.rng.normal(size=shape) / np.sqrt(fan_in))

    def conv(self, src, f, k=3, s=1, act=None, bias=True, pad='same', name=None, dil=1, groups=1, positive=False):
        h, w, c = self.shape[src]
        name = self._name('conv', name)
        kh, kw = (k, k) if isinstance(k, int) else k
        ws = [self._kernel((kh, kw, c // groups, f), kh * kw * c // groups)]
        if positive:                # no cancellation: A stays at |y| through a deep chain (gain about 1 per layer)
            ws = [self.f32(np.abs(ws[0]) * 1.25 / np.sqrt(kh * kw * c // groups))]
        if bias:
            ws.append(self.f32(self.rng.normal(size=f) * 0.3))
        self.weights[name] = ws
        ekh, ekw = (kh - 1) * dil + 1, (kw - 1) * dil + 1
        oh, ow = (_same_out(h, s), _same_out(w, s)) if pad == 'same' else ((h - ekh) // s + 1, (w - ekw) // s + 1)
        extra = {'groups': groups} if groups != 1 else {}
        return self._add('Conv2D', name, [src], (oh, ow, f), filters=f, kernel_size=[kh, kw], strides=[s, s], padding=pad,
                         dilation_rate=[dil, dil], activation=act or 'linear', use_bias=bias, **extra)

    def convt(self, src, f, k=2, s=2, act=None, bias=True, pad='same', name=None):
        h, w, c = self.shape[src]
        name = self._name('convt', name)
        ws = [self._kernel((k, k, f, c), max(k * k * c // (s * s), 1))]
        if bias:
            ws.append(self.f32(self.rng.normal(size=f) * 0.3))
        self.weights[name] = ws
        oh, ow = (h * s, w * s) if pad == 'same' else ((h - 1) * s + max(k, s), (w - 1) * s + max(k, s))
        return self._add('Conv2DTranspose', name, [src], (oh, ow, f), filters=f, kernel_size=[k, k], strides=[s, s], padding=pad,
                         activation=act or 'linear', use_bias=bias)

    def dw(self, src, mult=1, k=3, s=1, act=None, bias=True, name=None):
        h, w, c = self.shape[src]
        name = self._name('dw', name)
        ws = [self._kernel((k, k, c, mult), k * k)]
        if bias:
            ws.append(self.f32(self.rng.normal(size=c * mult) * 0.3))
        self.weights[name] = ws
        return self._add('DepthwiseConv2D', name, [src], (_same_out(h, s), _same_out(w, s), c * mult), kernel_size=[k, k], strides=[s, s],
                         padding='same', depth_multiplier=mult, dilation_rate=[1, 1], activation=act or 'linear', use_bias=bias)

    def sep(self, src, f, mult=1, k=3, act=None, bias=True, name=None):
        h, w, c = self.shape[src]
        name = self._name('sep', name)
        ws = [self._kernel((k, k, c, mult), k * k), self._kernel((1, 1, c * mult, f), c * mult)]
        if bias:
            ws.append(self.f32(self.rng.normal(size=f) * 0.3))
        self.weights[name] = ws
        return self._add('SeparableConv2D', name, [src], (h, w, f), filters=f, kernel_size=[k, k], strides=[1, 1], padding='same',
                         depth_multiplier=mult, dilation_rate=[1, 1], activation=act or 'linear', use_bias=bias)

    def bn(self, src, eps=None, scale=True, center=True, stats='hard', name=None):
        """``stats``: 'hard' - moving variance from 1e-6 to 1e2 across channels, gamma of both signs, beta and mean large against the
        signal; 'mild' - everything of order 1; 'near1' - scale within 1e-3 of 1; 'near_identity' - scale 1, shift 5e-4."""
        h, w, c = self.shape[src]
        name = self._name('bn', name)
        r, e = self.rng, (1e-3 if eps is None else eps)
        if stats == 'hard':
            var = 10.0 ** np.linspace(-6, 2, c)[r.permutation(c)]
            gamma, beta, mean = r.normal(size=c), 5.0 * r.normal(size=c), 5.0 * r.normal(size=c)
            gamma[0] = -abs(gamma[0]) - 0.1
        elif stats == 'mild':
            var = r.uniform(0.5, 2.0, size=c)
            gamma, beta, mean = r.uniform(0.5, 1.5, size=c) * np.where(r.random(c) < 0.3, -1, 1), 0.1 * r.normal(size=c), 0.1 * r.normal(size=c)
        elif stats == 'near1':
            var = np.full(c, 1.0 - e)
            gamma, beta, mean = 1.0 + 3e-4 * r.normal(size=c), 0.01 * r.normal(size=c), 0.01 * r.normal(size=c)
        else:
            var, gamma, beta, mean = np.full(c, 1.0 - e), np.ones(c), np.full(c, 5e-4), np.zeros(c)
        ws = ([self.f32(gamma)] if scale else []) + ([self.f32(beta)] if center else []) + [self.f32(mean), self.f32(var)]
        self.weights[name] = ws
        cfg = dict(axis=[1] if self.cf else [3], scale=scale, center=center, momentum=0.99)
        if eps is not None:
            cfg['epsilon'] = eps
        return self._add('BatchNormalization', name, [src], (h, w, c), **cfg)

    def layer(self, cls, src, name=None, shape=None, **cfg):
        return self._add(cls, self._name(cls.lower(), name), [src] if isinstance(src, str) else list(src), shape or self.shape[src if isinstance(src, str) else src[0]], **cfg)

    def act(self, src, fn, name=None):
        return self.layer('Activation', src, name, activation=fn)

    def leaky(self, src, alpha, name=None):
        return self.layer('LeakyReLU', src, name, alpha=alpha)

    def relu(self, src, max_value=None, negative_slope=0.0, name=None):
        return self.layer('ReLU', src, name, max_value=max_value, negative_slope=negative_slope, threshold=0.0)

    def prelu(self, src, name=None):
        h, w, c = self.shape[src]
        name = self._name('prelu', name)
        al = self.f32(self.rng.uniform(-0.2, 0.5, size=(c, 1, 1) if self.cf else (1, 1, c)))
        self.weights[name] = [al]
        return self._add('PReLU', name, [src], (h, w, c), shared_axes=[2, 3] if self.cf else [1, 2])

    def pool(self, src, avg=False, k=2, s=2, pad='valid', name=None):
        h, w, c = self.shape[src]
        oh, ow = (_same_out(h, s), _same_out(w, s)) if pad == 'same' else ((h - k) // s + 1, (w - k) // s + 1)
        return self.layer('AveragePooling2D' if avg else 'MaxPooling2D', src, name, (oh, ow, c), pool_size=[k, k], strides=[s, s], padding=pad)

    def up(self, src, f=2, interp='nearest', name=None):
        h, w, c = self.shape[src]
        return self.layer('UpSampling2D', src, name, (h * f, w * f, c), size=[f, f], interpolation=interp)

    def cat(self, srcs, name=None):
        h, w, _ = self.shape[srcs[0]]
        return self.layer('Concatenate', srcs, name, (h, w, sum(self.shape[s][2] for s in srcs)), axis=1 if self.cf else -1)

    def merge(self, cls, srcs, name=None):
        return self.layer(cls, srcs, name)

    def zpad(self, src, t, b, l, r, name=None):
        h, w, c = self.shape[src]
        return self.layer('ZeroPadding2D', src, name, (h + t + b, w + l + r, c), padding=[[t, b], [l, r]])

    def crop(self, src, t, b, l, r, name=None):
        h, w, c = self.shape[src]
        return self.layer('Cropping2D', src, name, (h - t - b, w - l - r, c), cropping=[[t, b], [l, r]])

    def again(self, name, src):
        """Another call of layer ``name`` (shared weights) on ``src`` -> the call's tensor name."""
        L = [l for l in self.layers if l['name'] == name][0]
        L['inbound_nodes'].append([self._ref(s) for s in ([src] if isinstance(src, str) else src)])
        key = '%s/call%d' % (name, len(L['inbound_nodes']) - 1)
        self.shape[key] = self.shape[name]
        return key

    def nested(self, inner, src, name):
        """The model built by the G ``inner`` as one layer called on ``src``."""
        cfg = inner.model([inner.layers[-1]['name']])
        self.weights[name] = {k: v for k, v in inner.weights.items()}
        self.layers.append({'class_name': 'Functional', 'name': name, 'config': dict(cfg['config'], name=name), 'inbound_nodes': [[self._ref(src)]]})
        self.shape[name] = inner.shape[inner.layers[-1]['name']]
        return name

    def model(self, outputs):
        return {'class_name': 'Functional', 'config': {'name': 'm', 'layers': self.layers, 'input_layers': [['in', 0, 0]],
                                                       'output_layers': [self._ref(o)[:3] for o in outputs]}}

    def case(self, name, group, outputs, **kw):
        d = dict(name=name, group=group, cfg=self.model(outputs if isinstance(outputs, (list, tuple)) else [outputs]), weights=self.weights,
                 x=self.x, lambda_affine={}, keep=(), output=0, fused=[], unfused=[], folded_up=[], views={}, copies=0, count_ops=True,
                 fewer_buffers=False, channels_first=self.cf)
        d.update(kw)
        return d


# ---------------------------------------------------------------------------------------------------------------- hand cases
def _bn_cases():
    out = []
    for tag, eps in (('1e-5', 1e-5), ('default', None), ('0.1', 0.1)):
        for stats in ('hard', 'mild'):
            g = G(100 + len(out), 18, 22, 5)
            c = g.conv('in', 12, name='c')
            b = g.bn(c, eps=eps, stats=stats, name='bn')
            out.append(g.case('bn_fold_eps_%s_%s' % (tag, stats), 'bn', b, fused=[('bn', 'c')]))
    g = G(110, 17, 23, 4)
    b = g.bn(g.conv('in', 9, bias=False, name='c'), eps=1e-4, name='bn')
    out.append(g.case('bn_fold_conv_without_bias', 'bn', b, fused=[('bn', 'c')]))
    for k, (sc, ce) in enumerate(((False, True), (True, False))):
        g = G(111 + k, 17, 23, 4)
        b = g.bn(g.conv('in', 9, k=(1, 3), name='c'), scale=sc, center=ce, name='bn')
        out.append(g.case('bn_fold_%s' % ('scale_false' if not sc else 'center_false'), 'bn', b, fused=[('bn', 'c')]))
    g = G(113, 11, 13, 8)
    b = g.bn(g.convt('in', 8, k=2, s=2, name='ct'), stats='near1', name='bn')
    out.append(g.case('bn_fold_convt_in_eq_out_near_one', 'bn', b, fused=[('bn', 'ct')]))
    g = G(114, 11, 13, 8)
    b = g.bn(g.convt('in', 8, k=3, s=2, name='ct'), stats='hard', eps=1e-5, name='bn')
    out.append(g.case('bn_fold_convt_in_eq_out_hard', 'bn', b, fused=[('bn', 'ct')]))
    g = G(115, 11, 13, 6)
    b = g.bn(g.convt('in', 10, k=3, s=2, name='ct'), stats='hard', name='bn')
    out.append(g.case('bn_fold_convt_in_ne_out', 'bn', b, fused=[('bn', 'ct')]))
    g = G(116, 19, 21, 5)
    b = g.bn(g.dw('in', mult=3, name='d'), stats='hard', eps=1e-5, name='bn')
    out.append(g.case('bn_fold_depthwise_multiplier_3', 'bn', b, fused=[('bn', 'd')]))
    g = G(117, 19, 21, 8)
    b = g.bn(g.sep('in', 8, mult=1, name='s'), stats='hard', name='bn')
    out.append(g.case('bn_fold_separable', 'bn', b, fused=[('bn', 's')]))
    g = G(118, 18, 22, 5)
    ct = g.cat([g.conv('in', 3, name='a'), g.conv('in', 6, k=1, name='b')], name='cat')
    b = g.bn(ct, stats='hard', eps=1e-5, name='bn')
    out.append(g.case('bn_after_concat_not_folded', 'bn', b, unfused=[('bn', 'cat')], views={'a': (0, 9), 'b': (3, 9)}))
    g = G(119, 18, 22, 5)
    c = g.conv('in', 7, name='c')
    b = g.bn(c, stats='hard', name='bn')
    out.append(g.case('bn_producer_has_second_consumer_not_folded', 'bn', g.merge('Add', [c, b], name='sum'), unfused=[('bn', 'c')]))
    for stats in ('near_identity', 'hard'):
        g = G(120, 18, 22, 5)
        b = g.bn(g.conv('in', 7, act='relu', name='c'), stats=stats, name='bn')
        out.append(g.case('bn_after_conv_relu_not_folded_%s' % stats, 'bn', b, unfused=[('bn', 'c')]))
    g = G(121, 21, 27, 4)
    p = g.pool(g.leaky(g.bn(g.conv('in', 10, name='c'), stats='mild', name='bn'), 0.01, name='act'), name='pool')
    out.append(g.case('bn_leaky_maxpool_chain', 'bn', p, fused=[('bn', 'c'), ('act', 'c')]))
    g = G(122, 21, 27, 4)
    p = g.pool(g.relu(g.bn(g.conv('in', 10, name='c'), stats='hard', eps=1e-5, name='bn'), name='act'), avg=True, name='pool')
    out.append(g.case('bn_relu_avgpool_chain', 'bn', p, fused=[('bn', 'c'), ('act', 'c')]))
    return out


def _input_cases():
    out = []
    g = G(200, 17, 25, 4)
    mean = g.f32([0.0, 0.5, 0.0, 2.0])
    var = g.f32([1e-16, 4.0, 1e-15, 0.25])
    x = g.x.copy()
    x[..., 0] = (x[..., 0] * 1e-8).astype(np.float32)                 # the channels of tiny variance carry a signal of that size
    x[..., 2] = (x[..., 2] * 3e-8).astype(np.float32)
    g.x = x
    n = g._add('Normalization', 'norm', ['in'], (17, 25, 4), axis=[-1])
    g.weights['norm'] = [mean, var, np.zeros((), np.int64)]
    out.append(g.case('normalization_variance_below_1e-14', 'input', g.conv(n, 6, act='relu', name='c')))
    for kind in ('tfop', 'lambda'):
        g = G(201, 32, 48, 1, u8=True)
        if kind == 'tfop':
            n = g._add('TFOpLambda', 'tf.math.truediv', [], (32, 48, 1), function='math.truediv')
            g.layers[-1]['inbound_nodes'] = [['in', 0, 0, {'y': 255.0, 'name': None}]]
            lam = {}
        else:
            n = g._add('Lambda', 'lambda', ['in'], (32, 48, 1), function=['4wEAAAA=', None, None], function_type='lambda')
            lam = {'lambda': (1 / 255.0, 0.0)}
        out.append(g.case('input_lambda_%s_div_255' % kind, 'input', g.conv(n, 8, act='relu', name='c'), lambda_affine=lam))
    g = G(202, 19, 29, 3, u8=True)
    n = g._add('Rescaling', 'rescale', ['in'], (19, 29, 3), scale=1 / 127.5, offset=-1.0)
    out.append(g.case('input_rescaling_scale_then_offset', 'input', g.conv(n, 8, act='relu', name='c')))
    g = G(203, 19, 29, 3, u8=True)
    a = g._add('TFOpLambda', 'tf.math.subtract', [], (19, 29, 3), function='math.subtract')
    g.layers[-1]['inbound_nodes'] = [['in', 0, 0, {'y': 127.5, 'name': None}]]
    b = g._add('TFOpLambda', 'tf.math.multiply', [], (19, 29, 3), function='math.multiply')
    g.layers[-1]['inbound_nodes'] = [[a, 0, 0, {'y': 0.0078125, 'name': None}]]
    out.append(g.case('input_tfop_subtract_then_multiply', 'input', g.conv(b, 8, act='relu', name='c')))
    return out


def _act_cases():
    out = []
    for alpha in (0.01, 0.3):
        g = G(300, 18, 26, 3)
        out.append(g.case('leaky_relu_layer_alpha_%g' % alpha, 'act', g.leaky(g.conv('in', 9, name='c'), alpha, name='act'), fused=[('act', 'c')]))
    g = G(301, 18, 26, 3)
    out.append(g.case('relu_negative_slope_layer', 'act', g.relu(g.convt('in', 9, name='c'), negative_slope=0.01, name='act'), fused=[('act', 'c')]))
    g = G(302, 18, 26, 3)
    out.append(g.case('relu_max_value_layer', 'act', g.relu(g.conv('in', 9, name='c'), max_value=0.75, name='act'), fused=[('act', 'c')]))
    g = G(303, 18, 26, 3)
    out.append(g.case('relu6_activation_key', 'act', g.conv(g.conv('in', 9, act='relu6', name='c'), 4, k=1, name='d')))
    g = G(304, 18, 26, 3)
    out.append(g.case('prelu_layer_after_conv', 'act', g.prelu(g.conv('in', 9, name='c'), name='act'), unfused=[('act', 'c')]))
    for fn in ('elu', 'sigmoid', 'tanh'):
        g = G(305, 17, 19, 3)
        a = g.act(g.dw('in', mult=2, name='c'), fn, name='act')
        k = g.conv('in', 6, act=fn, name='k')
        out.append(g.case('%s_layer_and_activation_key' % fn, 'act', g.merge('Add', [a, k], name='sum'), fused=[('act', 'c')]))
    # x >= 0 with exact zeros, one positive tap, bias -2e-3: the pre-activation is -2e-3 exactly where x is 0, so a lost slope or a pool
    # moved in front of the activation changes the result by less than 1e-3 of its range
    for tail in ('leaky', 'avgpool'):
        g = G(306, 18, 26, 1)
        g.x = np.maximum(g.x, 0).astype(np.float32)
        c = g.conv('in', 4, k=1, name='c')
        g.weights['c'] = [g.f32(np.array([0.5, 1.0, 1.5, 2.0]).reshape(1, 1, 1, 4)), g.f32(np.full(4, -2e-3))]
        if tail == 'leaky':
            out.append(g.case('leaky_relu_small_negatives', 'act', g.leaky(c, 0.01, name='act'), fused=[('act', 'c')]))
        else:
            out.append(g.case('relu_avgpool_small_negatives', 'act', g.pool(g.relu(c, name='act'), avg=True, name='pool'), fused=[('act', 'c')]))
    return out


def _up_cases():
    out = []
    for f, k in ((2, 2), (2, 3), (3, 2), (3, 3)):
        g = G(400 + f * 4 + k, 9, 13, 6)
        u = g.up('in', f, name='up')
        c = g.conv(u, 10, k=k, act='relu', name='c')
        fold = f == 2 and k == 2
        out.append(g.case('upsample_%d_conv_%dx%d' % (f, k, k), 'up', c, folded_up=[('up', 'c')] if fold else [], unfused=[] if fold else [('c', 'up')]))
    g = G(420, 9, 13, 6)
    u = g.up('in', 2, name='up')
    c = g.conv(u, 10, k=2, name='c')
    out.append(g.case('upsample_2_conv_2x2_second_consumer_not_folded', 'up', g.cat([c, u], name='cat'), unfused=[('c', 'up')]))
    return out


def _concat_cases():
    out = []
    g = G(500, 18, 22, 4)
    ct = g.cat([g.conv('in', 3, name='a'), g.conv('in', 8, k=1, name='b'), g.conv('in', 5, k=2, name='c')], name='cat')
    out.append(g.case('concat_3_8_5_as_views', 'concat', g.conv(ct, 6, name='d'), views={'a': (0, 16), 'b': (3, 16), 'c': (11, 16)}))
    g = G(501, 18, 22, 4)
    a, b, c = g.conv('in', 3, name='a'), g.conv('in', 6, k=1, name='b'), g.conv('in', 5, k=2, name='c')
    s = g.merge('Add', [g.conv(g.cat([a, b], name='cat1'), 7, name='d'), g.conv(g.cat([c, a], name='cat2'), 7, k=1, name='e')], name='sum')
    out.append(g.case('concat_tensor_in_two_concatenations', 'concat', s, views={'a': (0, 9), 'b': (3, 9), 'c': (0, 8)}, copies=1))
    g = G(502, 18, 22, 4)
    a = g.conv('in', 5, name='a')
    out.append(g.case('concat_of_a_tensor_with_itself', 'concat', g.conv(g.cat([a, a], name='cat'), 6, k=1, name='d'), copies=2))
    g = G(503, 18, 22, 4)
    a, b, c = g.conv('in', 3, name='a'), g.conv('in', 6, k=1, name='b'), g.conv('in', 5, k=2, name='c')
    ct = g.cat([g.cat([a, b], name='cat1'), c], name='cat2')
    out.append(g.case('concat_feeding_a_concatenation', 'concat', g.conv(ct, 6, name='d'), views={'a': (0, 9), 'b': (3, 9), 'c': (9, 14)}, copies=1))
    g = G(504, 18, 22, 4)
    a = g.crop(g.conv('in', 3, name='a'), 1, 2, 3, 0, name='crop')
    b = g.zpad(g.conv('in', 6, k=3, pad='valid', s=2, name='b'), 3, 4, 5, 4, name='pad')
    ct = g.cat([a, b], name='cat')
    out.append(g.case('concat_of_crop_and_zero_pad', 'concat', g.conv(ct, 6, name='d'), views={'crop': (0, 9), 'pad': (3, 9)}))
    return out


def _alloc_cases():
    out = []
    g = G(600, 18, 22, 3)
    t = [g.conv('in', 8, act='relu', name='t0', positive=True)]
    skips = {3: 1, 5: 2, 8: 5, 11: 11}
    for i in range(1, 12):
        src = t[-1]
        if i in skips:
            src = g.merge('Add', [t[-1], t[max(i - 1 - skips[i], 0)]], name='add%d' % i)
        t.append(g.conv(src, 8, act='relu' if i % 2 else None, name='t%d' % i, positive=True))
    out.append(g.case('alloc_ladder_of_12_with_skips_1_2_5_11', 'alloc', t[-1], fewer_buffers=True))
    g = G(601, 18, 22, 3)
    a = g.conv('in', 8, name='a', positive=True)
    long = a
    for i in range(4):
        long = g.conv(long, 8, act='relu', name='l%d' % i, positive=True)
    short = g.conv(a, 8, k=1, name='s', positive=True)
    out.append(g.case('alloc_diamond_long_arm_outlives_short', 'alloc', g.conv(g.merge('Add', [short, long], name='sum'), 4, name='o', positive=True),
                      fewer_buffers=True))
    g = G(602, 18, 22, 3)
    tr = g.conv(g.conv('in', 8, act='relu', name='t0', positive=True), 8, act='relu', name='t1', positive=True)
    cls, box = g.conv(tr, 2, k=1, name='cls'), g.conv(tr, 8, k=1, name='bbox')
    m = tr
    for i in range(4):
        m = g.conv(m, 8, act='relu', name='m%d' % i, positive=True)
    out.append(g.case('alloc_outputs_kept_by_keep', 'alloc', [g.conv(m, 2, k=1, name='mask'), cls, box], keep=('cls', 'bbox'), fewer_buffers=True))
    g = G(603, 18, 22, 3)
    m = 'in'
    for i in range(6):
        m = g.conv(m, 8, act='relu', name='m%d' % i, positive=True)
    out.append(g.case('alloc_output_in_the_middle', 'alloc', ['m2', m], fewer_buffers=True))
    return out


def _structure_cases():
    out = []
    g = G(700, 18, 22, 4)
    sh = g.conv('in', 6, act='relu', name='shared')
    r1 = g._add('Rescaling', 'r1', ['in'], (18, 22, 4), scale=-0.5, offset=0.25)
    r2 = g.pool(g.up('in', 2, name='u'), avg=True, name='r2')
    ct = g.cat([sh, g.again('shared', r1), g.again('shared', r2)], name='cat')
    out.append(g.case('shared_layer_called_three_times', 'structure', g.conv(ct, 5, k=1, name='o'), count_ops=False))
    g = G(701, 18, 22, 4)
    sh = g.conv('in', 6, name='shared')
    r1 = g._add('Rescaling', 'r1', ['in'], (18, 22, 4), scale=1.0 + 2.0 ** -12, offset=0.0)
    out.append(g.case('shared_layer_on_nearly_equal_inputs', 'structure', g.cat([sh, g.again('shared', r1)], name='cat'), count_ops=False))
    inner = G(702, 18, 22, 6)
    inner.relu(inner.bn(inner.conv('in', 6, name='ic'), stats='mild', name='ibn'), name='iact')
    g = G(703, 18, 22, 6)
    n0 = g.nested(inner, 'in', 'sub')
    n1 = g.again('sub', g.conv('in', 6, k=1, name='c'))
    out.append(g.case('nested_model_used_twice', 'structure', g.merge('Add', [n0, n1], name='sum'), count_ops=False))
    g = G(704, 18, 22, 5, cf=True)
    b = g.bn(g.conv('in', 12, name='c'), eps=1e-5, stats='hard', name='bn')
    out.append(g.case('channels_first_bn_fold', 'structure', g.prelu(b, name='act'), fused=[('bn', 'c')]))
    g = G(705, 18, 22, 4, cf=True)
    ct = g.cat([g.conv('in', 3, name='a'), g.conv('in', 8, k=1, name='b'), g.conv('in', 5, k=2, name='c')], name='cat')
    out.append(g.case('channels_first_concat_3_8_5', 'structure', g.conv(ct, 6, name='d'), views={'a': (0, 16), 'b': (3, 16), 'c': (11, 16)}))
    return out


GROUPS = ('bn', 'input', 'act', 'up', 'concat', 'alloc', 'structure')
_HAND = None


def hand_cases():
    global _HAND
    if _HAND is None:
        _HAND = _bn_cases() + _input_cases() + _act_cases() + _up_cases() + _concat_cases() + _alloc_cases() + _structure_cases()
        names = [c['name'] for c in _HAND]
        assert len(set(names)) == len(names)
    return _HAND


def outputs_of(case):
    """The tensor names both test files check: the output ``build_plan`` is asked for, then every kept layer."""
    outs = [r[0] if not r[1] else '%s/call%d' % (r[0], r[1]) for r in case['cfg']['config']['output_layers']]
    return [outs[case['output']]] + list(case['keep'])


def x_nhwc(case):
    return np.ascontiguousarray(np.transpose(case['x'], (0, 2, 3, 1))) if case['channels_first'] else case['x']


# ---------------------------------------------------------------------------------------------------------------- random graphs
def _random_once(seed):
    r = np.random.default_rng(seed)
    h, w, c = int(r.integers(16, 41)), int(r.integers(16, 57)), int(r.integers(1, 9))
    g = G(seed, h, w, c)
    g.rng = r
    live = ['in']
    n_layers = int(r.integers(6, 21))
    while len(g.layers) - 1 < n_layers:
        src = live[-1] if r.random() < 0.7 else live[int(r.integers(len(live)))]
        sh, sw_, sc = g.shape[src]
        kind = r.choice(['conv', 'conv', 'conv', 'bn', 'act', 'pool', 'up', 'cat', 'add', 'dw', 'sep', 'convt', 'pad', 'crop', 'drop'])
        f = int(r.integers(1, 25))
        if kind == 'conv':
            s = int(r.choice([1, 1, 1, 2]))
            k = int(r.choice([1, 2, 3])) if min(sh, sw_) >= 3 else 1
            t = g.conv(src, f, k=k, s=s, act=str(r.choice(['linear', 'linear', 'relu', 'sigmoid', 'tanh', 'elu', 'relu6'])), bias=bool(r.random() < 0.8),
                       pad=str(r.choice(['same', 'same', 'valid'])) if s == 1 else 'same')
        elif kind == 'bn':
            t = g.bn(src, eps=[None, 1e-5, 1e-2][int(r.integers(3))], scale=bool(r.random() < 0.8), center=bool(r.random() < 0.8), stats='mild')
        elif kind == 'act':
            which = int(r.integers(5))
            t = (g.leaky(src, float(r.choice([0.01, 0.1, 0.3]))) if which == 0 else g.relu(src) if which == 1 else g.relu(src, max_value=1.0)
                 if which == 2 else g.prelu(src) if which == 3 else g.act(src, str(r.choice(['relu', 'sigmoid', 'tanh', 'softmax']))))
        elif kind == 'pool':
            if min(sh, sw_) < 4:
                continue
            t = g.pool(src, avg=bool(r.random() < 0.4), pad=str(r.choice(['valid', 'same'])))
        elif kind == 'up':
            if sh * 2 > 40 or sw_ * 2 > 56:
                continue
            t = g.up(src, 2, interp=str(r.choice(['nearest', 'nearest', 'bilinear'])))
            if r.random() < 0.6:
                t = g.conv(t, f, k=2, act=str(r.choice(['linear', 'relu'])))
        elif kind in ('cat', 'add'):
            same = [o for o in live if o != src and g.shape[o][:2] == (sh, sw_) and (kind == 'cat' or g.shape[o][2] == sc)]
            if not same or (kind == 'cat' and sc + g.shape[same[-1]][2] > 24):
                continue
            other = same[int(r.integers(len(same)))]
            if kind == 'cat' and sc + g.shape[other][2] > 24:
                continue
            t = g.cat([src, other]) if kind == 'cat' else g.merge(str(r.choice(['Add', 'Add', 'Subtract', 'Maximum', 'Average'])), [src, other])
        elif kind == 'dw':
            mult = int(r.choice([1, 2]))
            if sc * mult > 24:
                continue
            t = g.dw(src, mult=mult, s=int(r.choice([1, 2])), act=str(r.choice(['linear', 'relu'])))
        elif kind == 'sep':
            t = g.sep(src, f, act=str(r.choice(['linear', 'relu'])))
        elif kind == 'convt':
            if sh * 2 > 40 or sw_ * 2 > 56:
                continue
            t = g.convt(src, f, k=int(r.choice([2, 3])), s=2, act=str(r.choice(['linear', 'relu'])))
        elif kind == 'pad':
            if sh + 3 > 40 or sw_ + 3 > 56:
                continue
            t = g.zpad(src, 1, 2, 0, 3)
        elif kind == 'crop':
            if min(sh, sw_) < 8:
                continue
            t = g.crop(src, 2, 1, 0, 3)
        else:
            t = g.layer('Dropout', src, rate=0.5)
        live.append(t)
    return g.case('random_%d' % seed, 'random', live[-1], count_ops=False)


def random_graph(seed):
    """A DAG of 6 to 20 layers over the vocabulary of the hand cases, with the same size limits and random skip connections (a layer
    reads a random earlier tensor three times in ten; Concatenate and the merge layers pick a second earlier tensor).  The weights are
    redrawn until A stays within 1e3 of |y|.max() at the output."""
    import plan_ref
    for attempt in range(50):
        case = _random_once(seed * 1000 + attempt)
        y, A = plan_ref.forward(case['cfg'], case['weights'], case['x'])[outputs_of(case)[0]]
        if np.isfinite(A).all() and A.max() <= 1e3 * np.abs(y).max():
            case['name'] = 'random_%d' % seed
            return case
    raise AssertionError('seed %d: no draw keeps A within 1e3 of |y|.max()' % seed)


_RANDOM = {}


def random_cases():
    for s in range(N_SEEDS):
        if s not in _RANDOM:
            _RANDOM[s] = random_graph(s)
    return [_RANDOM[s] for s in range(N_SEEDS)]


def group_cases(group):
    return random_cases() if group == 'random' else [c for c in hand_cases() if c['group'] == group]
