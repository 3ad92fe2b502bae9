"""The cases of tests/test_conv_tails.py (CPU) and tests/test_gpu_conv_tails.py (device): what a convolution kernel does BEHIND its
accumulated sum - activation, fused 2 x 2 max-pool, fused 1 x 1 head - held to float64.  TEST INFRASTRUCTURE ONLY.

A   ``exact_case``: conv_exact_cases' delta-filter construction (one tap 1.0, bias 0 on that output channel) on every exact path, with the
    activation sweep of tests/layer_cases.py as data: the argument of the activation is a float32 known bit for bit.  ``routing_case`` and
    ``first_case`` are the same construction on the 16 / 32 / 64-channel 3 x 3 'same' layers and on conv_wino16_kernel<FIRST>.
B   ``f4_case``: the ``dense`` family of tests/wino4_cases.py under other activations than linear / relu.
C   ``pool_case`` / ``head_case`` on the F(4x4) kernels (dense data) and on conv_wino16_kernel (dyadic lattice data: the sum is exact).

An activation is a key of ``ACTS``: (activation name in the Conv2D config, the Keras layer behind it or None, the (name, alpha) that
tests/wino4_ref.py evaluates and bounds).  Slopes, alphas and max_value are exact in float32.
"""
import zlib

import numpy as np

from ecseg_amd import keras_plan
from tests import conv_exact_cases as cx
from tests import conv_exact_ref as cref
from tests import layer_cases
from tests import wino4_cases as wc
from tests import wino4_ref as ref

ACTS = {
    'linear': ('linear', None, 'linear'),
    'relu': ('relu', None, 'relu'),
    'leaky0.25': ('linear', ('LeakyReLU', dict(alpha=0.25)), ('leaky_relu', 0.25)),
    'leaky0.0078125': ('linear', ('LeakyReLU', dict(alpha=0.0078125)), ('leaky_relu', 0.0078125)),
    'leaky0.125': ('linear', ('LeakyReLU', dict(alpha=0.125)), ('leaky_relu', 0.125)),
    'sigmoid': ('sigmoid', None, 'sigmoid'),
    'tanh': ('tanh', None, 'tanh'),
    'elu': ('elu', None, ('elu', 1.0)),
    'elu0.625': ('linear', ('ELU', dict(alpha=0.625)), ('elu', 0.625)),
    'elu1.5': ('linear', ('ELU', dict(alpha=1.5)), ('elu', 1.5)),
    'relu_max2.5': ('linear', ('ReLU', dict(max_value=2.5, negative_slope=0.0, threshold=0.0)), ('relu_clip', 2.5)),
    'swish': ('swish', None, 'swish'),
    'softmax': ('softmax', None, 'softmax'),
}
A_ACTS = ('relu', 'leaky0.25', 'leaky0.0078125', 'sigmoid', 'tanh', 'elu', 'elu0.625', 'elu1.5', 'relu_max2.5', 'swish')
B_ACTS = ('leaky0.25', 'sigmoid', 'tanh', 'elu')
CORE_ACTS = ('linear', 'relu', 'leaky0.25', 'leaky0.0078125', 'leaky0.125', 'sigmoid', 'tanh', 'elu')   # what apply_act_core implements (act_core_ok)
LATE_ACTS = ('swish',)      # no convolution kernel implements it: the plan splits it off and the convolution in front of it is linear
KEEPS_KERNEL = CORE_ACTS + LATE_ACTS     # a layer with one of these runs on the kernel its shape alone selects
ACT_CODE_ELU = 6            # include/ecseg_hip.h: ECSEG_ACT_ELU, the last code apply_act_core implements


def spec(act):
    return ACTS[act][2]


def _rng(*key):
    return np.random.default_rng(zlib.crc32('/'.join(str(k) for k in key).encode()))


def _f32(a):
    return np.ascontiguousarray(a, np.float32)


def layer_with_act(name, src, act, cout, k, s=1, padding='same', bias=True, dil=1, cls='Conv2D'):
    """-> (layers, name of the last one): the convolution, and the activation layer behind it where the activation is one."""
    conv_act, extra, _ = ACTS[act]
    layers = [cx.conv_layer(name, src, cout, k, s, padding, conv_act, bias, dil, cls=cls)]
    if extra is not None:
        layers.append(cx._L(extra[0], name + '_act', [name], **extra[1]))
    return layers, layers[-1]['config']['name']


def expected_kinds(plan, opts):
    """conv_exact_cases.profile_kinds with plan_run.hip's act_core_ok: a layer whose activation apply_act_core does not implement
    (a code above ELU, or ELU with alpha != 1) leaves the F(4x4) kernels and conv_wino16_kernel for the F(2x2) kernels.  The rule is
    stated here a second time ON PURPOSE, from the activation codes of include/ecseg_hip.h: the test must not read it from the code it
    checks."""
    paths = {d['op']: d for d in cx.conv_paths(plan)}
    out = []
    for op, kind in cx.profile_kinds(plan, opts):
        o, d = plan.ops[op], paths[op]
        core = o['act'] <= ACT_CODE_ELU and not (o['act'] == ACT_CODE_ELU and o['alpha'] != 1.0)
        if kind in (2, 4, 5) and not core:
            if opts['winograd'] and d['wino'] and d['h'] >= 4 and d['w'] >= 8:
                kind = 3 if (opts['wino_resident'] and d['cout'] <= 32 and d['cin'] <= 32) else 1
            else:
                kind = 0
        out.append((op, kind))
    return out


# ---- A: the activation of every exact path -----------------------------------------------------------------------------------------------
_IMP = cx.IMPULSE_FAMILIES
FAMILIES = {k: _IMP[k] for k in ('mfma', 'mfma_s2', 'mfma_k2_valid', 'convt_gemm', 'convt_phase_k3', 'convt_subpixel', 'tap_k5', 'first', 'small_cin',
                                 'generic', 'generic_dil', 'convt_generic', 'convt_split', 'dw')}
FAMILIES.update(
    wino=('Conv2D', 3, 1, 1, 'same', 8, 48, (9, 17), cx.WINO_OPTS['wino'], 'wino', 1),
    wino_res=('Conv2D', 3, 1, 1, 'same', 12, 20, (9, 17), cx.WINO_OPTS['wino_res'], 'wino_res', 3),
    wino16_c16=('Conv2D', 3, 1, 1, 'same', 16, 16, (17, 33), cx.WINO_OPTS['wino16'], 'wino16', 4),
    wino16_c32=('Conv2D', 3, 1, 1, 'same', 32, 32, (17, 33), cx.WINO_OPTS['wino16'], 'wino16', 4))
FAMILIES.update({'head_c%d' % c: ('Conv2D', 1, 1, 1, 'same', 16, c, (9, 17), None, 'head', None) for c in range(1, 9)})
FAMILY_ORDER = tuple(sorted(FAMILIES))      # fixed here: a case's default tap never depends on what was built before it
F2_FAMILIES = ('wino', 'wino_res', 'wino16_c16', 'wino16_c32')         # an input transform adds four inputs: dyadic data only
GRID_BITS = 10
N_IMAGES = 24


def sweep_values(snapped):
    """layer_cases.sweep(): 321 points of [-8, 8], +-1e-6 .. +-90, +-0; ``snapped``: onto m 2^-10 with |x| <= 8 (the tiny points become 0 and
    2^-10, the huge ones 8)."""
    v = layer_cases.sweep()[0, 0, :, 0].astype(np.float64)
    if snapped:
        v = np.clip(np.round(v * 2.0 ** GRID_BITS) / 2.0 ** GRID_BITS, -8.0, 8.0)
    return v.astype(np.float32)


def sweep_image(n, H, W, c, snapped):
    """The sweep spread over an NHWC image: every channel holds every point about n H W / 335 times, in a seeded shuffle of its own (a
    regular tiling meets the strides of the strided, dilated and transposed layers and leaves points out)."""
    v = sweep_values(snapped)
    P = n * H * W
    rng = _rng('tail_sweep', n, H, W, c)
    idx = np.stack([rng.permutation(np.tile(np.arange(len(v)), -(-P // len(v))))[:P] for _ in range(c)], axis=-1)
    return _f32(v[idx].reshape(n, H, W, c))


def _delta_weights(family, i, rng):
    """Tap i of a family tuple: (kernel with one 1.0, bias of full significands with 0 on the tapped output channel, output channel)."""
    cls, k, s, dil, padding, cin, cout = family[:7]
    shape = {'Conv2D': (k, k, cin, cout), 'Conv2DTranspose': (k, k, cout, cin), 'DepthwiseConv2D': (k, k, cin, cout)}[cls]
    r, q, ci, co = i % k, (i // k) % k, (5 * i + 1) % cin, (7 * i + 2) % cout
    w = np.zeros(shape, np.float32)
    if cls == 'Conv2DTranspose':
        w[r, q, co, ci] = 1.0
    else:
        w[r, q, ci, co] = 1.0
    oc = ci * cout + co if cls == 'DepthwiseConv2D' else co
    b = wc.full_significands(rng, (cin * cout if cls == 'DepthwiseConv2D' else cout,), -2, 2)
    b[oc] = 0.0
    return w, b, oc


def exact_case(fam, act, i=None, family=None):
    """One layer of family ``fam`` with a delta filter (tap ``i``, by default the activation's position in A_ACTS: the taps move along) and
    activation ``act`` -> dict(name, cfg, lin_cfg (the same layer, linear), weights, x, opts, path, kind, oc, act, expm1)."""
    family = family or FAMILIES[fam]
    cls, k, s, dil, padding, cin, cout, (H, W), opts, path, kind = family
    if i is None:
        i = A_ACTS.index(act) + FAMILY_ORDER.index(fam)
    w, b, oc = _delta_weights(family, i, _rng('tail_exact', fam, i))
    x = sweep_image(N_IMAGES, H, W, cin, fam in F2_FAMILIES)
    layers, out = layer_with_act('op', 'in', act, cout, k, s, padding, True, dil, cls)
    lin = [cx.conv_layer('op', 'in', cout, k, s, padding, 'linear', True, dil, cls=cls)]
    return dict(name='%s/%s' % (fam, act), fam=fam, act=act, cfg=cx._F([cx._in(H, W, cin)] + layers, out), lin_cfg=cx._F([cx._in(H, W, cin)] + lin, 'op'),
                weights={'op': [w, b]}, x=x, opts=dict(cx.OPTION_DEFAULTS, **(opts or {})), path=path, kind=kind, oc=oc, expm1=path == 'dw',
                f2=fam in F2_FAMILIES, bits=0)


def pre_activation(case):
    """The float64 value in front of the last activation, from conv_exact_ref on ``lin_cfg``: every sum has one non-zero term."""
    return cref.forward(case['lin_cfg'], case['weights'], case['x'])[0].astype(np.float64)


def f2_exact(values, taps=1):
    """The exactness precondition of the F(2x2) kernels on a delta filter: data on the grid m 2^-g with |x| <= 8.  B^T d B adds four of them
    (|V| <= 32, grid 2^-g), U = G e G^T is 1, 1/2 or 1/4 (exact products, grid 2^-(g+2)), A^T M A adds nine of those (< 2^9): 9 + g + 2
    bits, which must not exceed 24.  -> the smallest g that holds the values."""
    v = np.asarray(values, np.float64)
    assert np.abs(v).max() <= 8.0
    for g in range(0, 14):
        if np.array_equal(v * 2.0 ** g, np.rint(v * 2.0 ** g)):
            assert 9 + g + 2 <= 24
            return g
    raise AssertionError('not on a dyadic grid of at most 13 bits')


ROUTING_SHAPES = {'c16': (16, 16, (16, 32)), 'c32': (32, 32, (16, 32)), 'c64': (64, 64, (16, 32))}
ROUTING_AWAY = ('elu0.625', 'elu1.5', 'relu_max2.5')
ROUTING_STAY = ('elu', 'leaky0.25')
ROUTING_OPTS = (dict(cx.LIBRARY_DEFAULTS), dict(cx.LIBRARY_DEFAULTS, winograd=3))


def routing_case(shape, act):
    cin, cout, (H, W) = ROUTING_SHAPES[shape]
    family = ('Conv2D', 3, 1, 1, 'same', cin, cout, (H, W), None, 'mfma', None)
    c = exact_case('routing_' + shape, act, i=(ROUTING_AWAY + ROUTING_STAY).index(act) + 3, family=family)
    c['x'] = sweep_image(N_IMAGES, H, W, cin, True)
    c['f2'] = True
    return c


FIRST_PAIRS = (('leaky0.25', 'leaky0.0078125'), ('leaky0.0078125', 'leaky0.25'), ('tanh', 'relu'), ('relu', 'tanh'))


def first_case(c, act1, act2, H=17, W=36):
    """Conv2D(1 -> c, act1) computed into the halo of Conv2D(c -> c, act2) by conv_wino16_kernel<FIRST> (0x400), both with a delta filter
    through channel ``ca``: the output channel is act2(shift(act1(shift(x)))).  -> the case, with ``mid_cfg`` (the first layer alone)."""
    name = 'first_c%d/%s/%s' % (c, act1, act2)
    rng = _rng('tail_first', name)
    ca, co = 5 % c, 11 % c
    w1 = np.zeros((3, 3, 1, c), np.float32)
    w1[0, 2, 0, ca] = 1.0
    b1 = _f32(rng.integers(-512, 513, size=c) / 1024.0)
    b1[ca] = 0.0
    w2 = np.zeros((3, 3, c, c), np.float32)
    w2[2, 1, ca, co] = 1.0
    b2 = wc.full_significands(rng, (c,), -2, 2)
    b2[co] = 0.0
    l1, o1 = layer_with_act('c1', 'in', act1, c, 3)
    l2, o2 = layer_with_act('op', o1, act2, c, 3)
    # on the grid m 2^-3: LeakyReLU(2^-7) in the first layer leaves the second one's input on m 2^-10
    x = _f32(np.round(sweep_image(4, H, W, 1, True) * 8.0) / 8.0)
    weights = {'c1': [w1, b1], 'op': [w2, b2]}
    mid = cx._F([cx._in(H, W, 1), cx.conv_layer('c1', 'in', c, 3, act='linear')], 'c1')
    return dict(name=name, cfg=cx._F([cx._in(H, W, 1)] + l1 + l2, o2), mid_cfg=mid, weights=weights, x=x, opts=dict(cx.OPTION_DEFAULTS, **cx.WINO_OPTS['wino16']),
                kind=4, bits=0x400, oc=co, ca=ca, act1=act1, act2=act2, tap2=(2, 1))


def first_parts(c):
    """-> (mid, f1, lin, pre2, want) of a FIRST case in float64: the first layer's sum and activation, the second layer alone as a linear
    model, its sum, and act2 of it - act2(shift(act1(shift(x)))) on the tapped channel, act2(bias) on the others."""
    mid = cref.forward(c['mid_cfg'], {'c1': c['weights']['c1']}, c['x'])[0].astype(np.float64)
    f1 = ref.act64(mid, spec(c['act1']))
    n, H, W, ch = f1.shape
    lin = cx._F([cx._in(H, W, ch), cx.conv_layer('op', 'in', ch, 3, act='linear')], 'op')
    pre2 = cref.forward(lin, {'op': c['weights']['op']}, f1)[0].astype(np.float64)
    return mid, f1, lin, pre2, ref.act64(pre2, spec(c['act2']))


def first_truth(c):
    return first_parts(c)[4]


def f2_scale(d, tap):
    """Q of the F(2x2) kernels for ONE input channel d (N, H, W) >= 0 against a delta filter at ``tap``: |A^T| ((|G| e |G^T|) . (|B^T| d |B|)) |A|
    at every output pixel, the magnitude every rounding of the transforms is relative to."""
    BT = np.abs(np.array([[1, 0, -1, 0], [0, 1, 1, 0], [0, -1, 1, 0], [0, 1, 0, -1]], np.float64))
    G = np.abs(np.array([[1, 0, 0], [.5, .5, .5], [.5, -.5, .5], [0, 0, 1]], np.float64))
    AT = np.abs(np.array([[1, 1, 1, 0], [0, 1, -1, -1]], np.float64))
    n, H, W = d.shape
    ty, tx = -(-H // 2), -(-W // 2)
    xp = np.zeros((n, 2 * ty + 2, 2 * tx + 2))
    xp[:, 1:H + 1, 1:W + 1] = d
    D = np.stack([np.stack([xp[:, j:j + 2 * ty:2, k:k + 2 * tx:2] for k in range(4)], axis=-1) for j in range(4)], axis=-2)     # (n, ty, tx, j, k)
    V = np.einsum('ij,ntxjk,lk->ntxil', BT, D, BT)
    P = V * np.outer(G[:, tap[0]], G[:, tap[1]])
    Y = np.einsum('yi,ntxil,zl->ntyxz', AT, P, AT).reshape(n, 2 * ty, 2 * tx)
    return Y[:, :H, :W]


# ---- B / C: the F(4x4) kernels and conv_wino16_kernel behind a real sum ------------------------------------------------------------------
B_SHAPES = ('odd_regions', 'tail4', 'cout96', 'split_k')
POOL_ACTS = ('linear', 'tanh', 'leaky0.25')
# (classes, head activation, head bias, activation of the convolution): every class count with softmax, one class with sigmoid, every head
# activation at least once, every convolution activation with every class count
HEAD_COMBOS = ((1, 'softmax', True, 'relu'), (2, 'softmax', False, 'tanh'), (3, 'softmax', True, 'leaky0.25'), (4, 'softmax', True, 'relu'),
               (1, 'sigmoid', True, 'relu'), (2, 'tanh', True, 'leaky0.25'), (3, 'relu', False, 'tanh'), (4, 'linear', True, 'relu'),
               (3, 'sigmoid', False, 'leaky0.25'), (2, 'linear', False, 'tanh'), (4, 'sigmoid', True, 'tanh'), (1, 'relu', True, 'leaky0.25'),
               (1, 'tanh', False, 'tanh'), (2, 'relu', True, 'relu'), (3, 'linear', True, 'relu'), (4, 'tanh', False, 'leaky0.25'))
# what must NOT fuse: (classes, head activation, activation of the convolution)
UNFUSED_COMBOS = ((3, 'leaky0.125', 'leaky0.25'), (2, 'elu', 'relu'), (4, 'relu_max2.5', 'tanh'), (5, 'softmax', 'relu'))
KERNELS = ('f4_winograd2', 'f4_winograd3', 'w16_c16', 'w16_c32')


def kernel_setup(kernel):
    """-> (options, profile kind of the 3 x 3 layer, 'fp32' / 'bf16x3' / None for the exact conv_wino16_kernel)."""
    if kernel.startswith('f4'):
        w = int(kernel[-1])
        return dict(cx.LIBRARY_DEFAULTS, winograd=w), (5 if w == 3 else 2), ('bf16x3' if w == 3 else 'fp32')
    return dict(cx.OPTION_DEFAULTS, **cx.WINO_OPTS['wino16']), 4, None


B_SCALES = (0, -20)          # data and bias times 2^0 and 2^-20


def f4_case(shape, act, log2_scale=0):
    """The dense family; ``log2_scale`` = -20: data and bias times 2^-20 (exact scalings), so that the sum, Q and with them every term of
    the bound are ~1e-6 times what they were - an activation whose ABSOLUTE error near 0 is a float32 rounding of 1 (tanh written as
    2 / (1 + exp(-2 v)) - 1, ~3e-8) is then far outside a bound of ~1e-10, which at full scale is ~1e-5 and hides it."""
    x, w, b = wc.dense_data(shape)
    x, b = _f32(x * 2.0 ** log2_scale), _f32(b * 2.0 ** log2_scale)
    n, H, W, cin, cout, _ = wc.SHAPES[shape]
    layers, out = layer_with_act('op', 'in', act, cout, 3)
    return dict(name='%s/dense%s/%s' % (shape, '' if log2_scale == 0 else '_2^%d' % log2_scale, act), shape=shape, log2_scale=log2_scale, cfg=cx._F([cx._in(H, W, cin)] + layers, out), weights={'op': [w, b]}, x=x,
                layer=(x, w, b, act), tail=None, head=None, bits=0)


def lattice_data(c, H, W, key):
    """conv_wino16_kernel behind an exact sum: x = m 2^-6 with |m| <= 3, weights in {-4, 0, 4}, bias = -1 + m 2^-6: every partial result of
    the F(2x2) transforms is an integer multiple of 2^-6 below 81 Cin 3 4 + 2^7 < 2^24 (tests/test_gpu_conv_exact.py's precondition on 2^6
    times the data), and the pre-activation has a standard deviation of about 1.5 around -1."""
    rng = _rng('tail_lattice', key, c)
    x = _f32(rng.integers(-3, 4, size=(2, H, W, c)) / 64.0)
    w = _f32(rng.integers(-1, 2, size=(3, 3, c, c)) * 4.0)
    b = _f32(-1.0 + rng.integers(-32, 33, size=c) / 64.0)
    assert 81.0 * c * 3 * 4 + 128 < 2.0 ** 24
    return x, w, b


def _tail_data(kernel, what):
    if kernel.startswith('f4'):
        n, H, W, cin, cout, _ = wc.SHAPES[what]
        x, w, b = wc.dense_data(what, 'tail_' + what)
        if what == 'pool':
            b = _f32(b - 1.5)                            # so that a pooling window is often all negative
        return x, w, b, (H, W, cin, cout)
    c = int(kernel[-2:])
    H, W = (18, 34) if what == 'pool' else (17, 33)      # one 16 x 32 block + 1 (even extents for the pool)
    x, w, b = lattice_data(c, H, W, what)
    return x, w, b, (H, W, c, c)


def pool_case(kernel, act):
    x, w, b, (H, W, cin, cout) = _tail_data(kernel, 'pool')
    layers, out = layer_with_act('c', 'in', act, cout, 3)
    layers.append(cx._L('MaxPooling2D', 'p', [out], pool_size=[2, 2], strides=[2, 2], padding='valid'))
    return dict(name='%s/pool/%s' % (kernel, act), kernel=kernel, cfg=cx._F([cx._in(H, W, cin)] + layers, 'p'), weights={'c': [w, b]}, x=x,
                layer=(x, w, b, act), tail='pool', head=None, head_act=None, bits=0x100)


def head_case(kernel, k, head_act, head_bias, act, fused=True):
    x, w, b, (H, W, cin, cout) = _tail_data(kernel, 'head')
    rng = _rng('tail_head', kernel, k, head_act, head_bias, act)
    hw = _f32(rng.normal(size=(1, 1, cout, k)) / np.sqrt(cout) * 2.0)
    hb = _f32(rng.normal(size=k)) if head_bias else None
    layers, out = layer_with_act('c', 'in', act, cout, 3)
    hl, hout = layer_with_act('h', out, head_act, k, 1, bias=head_bias)
    return dict(name='%s/head/k%d_%s_%s_%s' % (kernel, k, head_act, 'bias' if head_bias else 'nobias', act), kernel=kernel,
                cfg=cx._F([cx._in(H, W, cin)] + layers + hl, hout), weights={'c': [w, b], 'h': [hw] + ([hb] if head_bias else [])}, x=x,
                layer=(x, w, b, act), tail='head', head=(hw.reshape(cout, k), hb if head_bias else np.zeros(k, np.float32)), head_act=head_act,
                bits=0x200 if fused else 0)


class TailRef:
    """Truth and bound of a B / C case.

    With y the float64 pre-activation, Q the F(4x4) scale (0 on conv_wino16_kernel's lattice: the sum is exact) and n = hard_count:

        pre   = n u Q + u |y|                                          tests/test_gpu_wino4_accuracy.py's hard bound (0 where the sum is exact)
        feat  = L pre SECOND + act_own(y)                              L = the largest |act'|; the activation's own float32 evaluation.  The
                device evaluates the activation at v = y + e, |e| <= pre, not at y: act_own is n u (n <= 10) times a function whose slope
                is at most L, so act_own(v) <= act_own(y) + 10 u L pre - inside SECOND = 1 + 2^-10 on the L pre term, as are the
                second-order terms of pre itself
        pool  = the largest ``feat`` of the window                     a maximum moves by at most the largest move of its inputs
        head  = L_h (sum_o |h_ok| feat_o + HEAD_OWN u (sum_o |h_ok| |f_o| + |hb_k|)) SECOND + act_own(l_k)       per class k; softmax:
                the maximum over the classes + (SOFTMAX_OWN + classes beyond 4) u + 2 u (max l - min l)
    """

    def __init__(self, case):
        x, w, b, act = case['layer']
        self.case, self.act = case, act
        self.exact_sum = not case.get('kernel', 'f4').startswith('f4')
        if self.exact_sum:
            lin = cx._F([cx._in(x.shape[1], x.shape[2], x.shape[3]), cx.conv_layer('c', 'in', w.shape[3], 3, act='linear')], 'c')
            y = cref.forward(lin, {'c': [w, b]}, x)[0].astype(np.float64)
            assert np.array_equal(y * 64.0, np.rint(y * 64.0)) and np.abs(y).max() * 64.0 < 2.0 ** 24
            self.y, self.q, self.t = y, np.zeros_like(y), None
        else:
            self.t = t = ref.Tiles(x, w)
            assert t.active.all() and len(t.chans) == t.cout
            self.y = t.scatter(ref.truth_tiles(t, b), np.zeros(t.cout))
            self.q = t.scatter(ref.scale_tiles(t), 0.0)
        self.feat = ref.act64(self.y, spec(act))
        self.b = b

    def feat_bound(self, mode):
        pre = 0.0 if self.exact_sum else ref.hard_count(self.case['layer'][0].shape[3], mode) * ref.U32 * self.q + ref.U32 * np.abs(self.y)
        return ref.act_lip(spec(self.act)) * pre * ref.SECOND + ref.act_own(self.y, spec(self.act))[0]

    @property
    def truth(self):
        c = self.case
        if c['tail'] == 'pool':
            return ref.pool2(self.feat)
        if c['tail'] == 'head':
            l = self.feat @ c['head'][0].astype(np.float64) + c['head'][1].astype(np.float64)
            return ref.softmax64(l) if c['head_act'] == 'softmax' else ref.act64(l, spec(c['head_act']))
        return self.feat

    def bound(self, mode):
        c, fb = self.case, self.feat_bound(mode)
        if c['tail'] == 'pool':
            return ref.pool2(fb)
        if c['tail'] == 'head':
            S, own = ref.head_scale(np.zeros_like(self.feat), self.feat, c['head'], spec(c['head_act']) if c['head_act'] != 'softmax' else 'softmax',
                                    feat_own=fb)
            k = c['head'][0].shape[1]
            return own + (max(k - 4, 0) * ref.U32 if c['head_act'] == 'softmax' else 0.0)
        return fb

    def replay(self, mode):
        """The kernels' float32 arithmetic on the CPU (F(4x4) cases; the exact sum of the lattice cases is its own replay)."""
        x, w, b, act = self.case['layer']
        c = self.case
        if self.exact_sum:
            f = ref.act32(self.y, spec(act))
        else:
            f = ref.act32(self.t.scatter(ref.replay_tiles(self.t, b, mode), ref.f32(b)), spec(act))
        if c['tail'] == 'pool':
            return ref.pool2(f)
        if c['tail'] == 'head':
            hw, hb = c['head']
            if f.shape[-1] == 64 and hw.shape[1] <= 4:
                return ref.head_replay(f, hw, hb, spec(c['head_act']) if c['head_act'] != 'softmax' else 'softmax')
            l = ref.f32(ref.f32(f @ hw.astype(np.float64)) + hb.astype(np.float64))     # (the narrow heads: any order is inside HEAD_OWN)
            if c['head_act'] == 'softmax':
                e = ref.f32(np.exp(ref.f32(l - l.max(axis=-1, keepdims=True))))
                return ref.f32(e / ref.f32(e.sum(axis=-1, keepdims=True)))
            return ref.act32(l, spec(c['head_act']))
        return f

    def worst(self, vals, mode):
        """-> (outputs beyond the bound, the largest error / bound)."""
        err, bound = np.abs(np.asarray(vals, np.float64) - self.truth), self.bound(mode)
        with np.errstate(divide='ignore', invalid='ignore'):
            ratio = np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), np.where(err > 0, np.inf, 0.0))
        return int((err > bound).sum()) + int((~np.isfinite(np.asarray(vals))).sum()), float(ratio.max())


def plan_of(case, fuse=True):
    return keras_plan.build_plan(case['cfg'], case['weights'], fuse=fuse)
