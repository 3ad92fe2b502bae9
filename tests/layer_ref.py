"""Float64 restatements of the non-convolution Keras layers, one function per op.  TEST INFRASTRUCTURE ONLY.

Plain numpy: no torch and nothing from ``ecseg_amd``.  Every function takes float64 NHWC arrays and returns ``(y, mag)``:
``y`` is the layer's value and ``mag >= |y|`` the magnitude its rounding errors are measured against - the sum of |terms| of a
reduction, the largest corner of a lerp, ``|x| inv + |shift|`` of an affine map; for an op without cancellation ``mag = |y|``.
A bound has the form ``n_ops * 2^-24 * mag`` (tests/test_gpu_layers.py) or ``k * 2^-53 * mag`` (tests/test_layers_ref.py).
Some functions return a third value, a dict of what their bound needs beyond ``mag``.

``forward(cfg, weights, x)`` evaluates the small Functional configs of tests/layer_cases.py layer by layer and returns
``(y, mag, aux)`` of the output layer.  Layer parameters (alpha, epsilon, slopes, statistics) are used as they are given: the cases
choose values that float32 holds exactly wherever the device receives them as float32.
"""
import math

import numpy as np

_erf = np.vectorize(math.erf, otypes=[np.float64])
_erfc = np.vectorize(math.erfc, otypes=[np.float64])


def same_pad(k, s, n):
    """TensorFlow's 'same': output ceil(n / s), total padding max((out - 1) s + k - n, 0), the smaller half in front."""
    out = -(-n // s)
    total = max((out - 1) * s + k - n, 0)
    return total // 2, total - total // 2


# ---- pooling ---------------------------------------------------------------------------------------------------------
def pool(x, k, s, padding, avg):
    """MaxPooling2D / AveragePooling2D, square window k, stride s.  'valid': floor((n - k) / s) + 1 windows.  'same': the window
    may hang over the edge; the maximum and the average run over the pixels inside the image, and the average divides by
    their number (TensorFlow leaves the padding out of the divisor).  mag (average) = sum |x| over the window / count."""
    N, H, W, C = x.shape
    if padding == 'same':
        Ho, Wo = -(-H // s), -(-W // s)
        pt, pl = same_pad(k, s, H)[0], same_pad(k, s, W)[0]
    else:
        Ho, Wo = (H - k) // s + 1, (W - k) // s + 1
        pt = pl = 0
    y = np.zeros((N, Ho, Wo, C))
    mag = np.zeros((N, Ho, Wo, C))
    for oy in range(Ho):
        for ox in range(Wo):
            y0, x0 = oy * s - pt, ox * s - pl
            win = x[:, max(y0, 0):min(y0 + k, H), max(x0, 0):min(x0 + k, W), :]
            cnt = win.shape[1] * win.shape[2]
            if avg:
                y[:, oy, ox] = win.sum(axis=(1, 2)) / cnt
                mag[:, oy, ox] = np.abs(win).sum(axis=(1, 2)) / cnt
            else:
                y[:, oy, ox] = win.max(axis=(1, 2))
                mag[:, oy, ox] = np.abs(y[:, oy, ox])
    return y, mag


def global_pool(x, avg, keepdims=False):
    """GlobalAveragePooling2D / GlobalMaxPooling2D -> (N, C), or (N, 1, 1, C) with keepdims.  mag (average) = mean |x|."""
    if avg:
        y, mag = x.mean(axis=(1, 2)), np.abs(x).mean(axis=(1, 2))
    else:
        y = x.max(axis=(1, 2))
        mag = np.abs(y)
    if keepdims:
        y, mag = y[:, None, None, :], mag[:, None, None, :]
    return y, mag


# ---- resampling ------------------------------------------------------------------------------------------------------
def upsample(x, f, interpolation):
    """UpSampling2D by the integer factor f.  nearest: out[y] = in[y // f].  bilinear: tf.image.resize with half-pixel centres -
    source coordinate (dst + 0.5) / f - 0.5, the two neighbours clamped to the image, weights from the fractional part.
    mag (bilinear) = the largest |corner| of the four."""
    N, H, W, C = x.shape
    if interpolation == 'nearest':
        y = x[:, np.arange(H * f) // f][:, :, np.arange(W * f) // f]
        return y, np.abs(y)

    def axis(n):
        src = (np.arange(n * f) + 0.5) / f - 0.5
        lo = np.floor(src)
        return np.clip(lo, 0, n - 1).astype(int), np.clip(lo + 1, 0, n - 1).astype(int), src - lo

    r0, r1, rf = axis(H)
    c0, c1, cf = axis(W)
    rf, cf = rf[None, :, None, None], cf[None, None, :, None]
    tl, tr, bl, br = x[:, r0][:, :, c0], x[:, r0][:, :, c1], x[:, r1][:, :, c0], x[:, r1][:, :, c1]
    y = (tl * (1 - cf) + tr * cf) * (1 - rf) + (bl * (1 - cf) + br * cf) * rf
    mag = np.maximum(np.maximum(np.abs(tl), np.abs(tr)), np.maximum(np.abs(bl), np.abs(br)))
    return y, mag


def zero_pad(x, padding):
    (t, b), (l, r) = padding
    y = np.pad(x, ((0, 0), (t, b), (l, r), (0, 0)))
    return y, np.abs(y)


def crop(x, cropping):
    (t, b), (l, r) = cropping
    y = x[:, t:x.shape[1] - b, l:x.shape[2] - r, :]
    return y, np.abs(y)


# ---- merge layers ----------------------------------------------------------------------------------------------------
def merge(kind, xs):
    """Add / Subtract / Multiply / Maximum / Minimum / Average of n inputs, folded left to right with numpy broadcasting
    (extents of 1 stretch).  mag = sum |x_i| for Add / Subtract, that sum / n for Average, |y| otherwise."""
    y = xs[0]
    mag = np.abs(xs[0])
    for t in xs[1:]:
        if kind in ('Add', 'Average'):
            y = y + t
        elif kind == 'Subtract':
            y = y - t
        elif kind == 'Multiply':
            y = y * t
        elif kind == 'Maximum':
            y = np.maximum(y, t)
        elif kind == 'Minimum':
            y = np.minimum(y, t)
        else:
            raise NotImplementedError(kind)
        mag = mag + np.abs(t)
    if kind == 'Average':
        return y / len(xs), mag / len(xs)
    if kind in ('Add', 'Subtract'):
        return y, mag
    return y, np.abs(y)


def prelu(x, alpha):
    """PReLU: alpha has the input's (h, w, c) shape with 1 on the shared axes."""
    y = np.where(x > 0, x, alpha[None] * x)
    return y, np.abs(y)


# ---- normalisation ---------------------------------------------------------------------------------------------------
def affine(x, scale, shift):
    """y = x * scale + shift per channel.  mag = |x scale| + |shift|."""
    return x * scale + shift, np.abs(x * scale) + np.abs(shift)


def batchnorm(x, gamma, beta, mean, var, eps):
    """BatchNormalization at inference: the affine map with scale = gamma / sqrt(var + eps), shift = beta - mean * scale."""
    C = x.shape[-1]
    g = np.ones(C) if gamma is None else gamma
    b = np.zeros(C) if beta is None else beta
    inv = g / np.sqrt(var + eps)
    return affine(x, inv, b - mean * inv)


def normalization(x, mean, var):
    """Normalization: (x - mean) / max(sqrt(var), 1e-7) as the affine map it is."""
    inv = 1.0 / np.maximum(np.sqrt(var), 1e-7)
    return affine(x, inv, -mean * inv)


def layernorm(x, gamma, beta, eps):
    """LayerNormalization over the last axis: mean, variance as the mean square of the CENTRED values, then
    (x - mean) * inv + beta with inv = gamma / sqrt(var + eps).  The device (and TensorFlow) evaluates
    x * inv + (beta - mean * inv), which cancels when |mean| >> the standard deviation; so
    mag = A |inv| + |beta| + |y| with A = mean |x| >= |mean|, which contains |mean| inv.
    aux['q'] = A^2 / (var + eps): the weight of the squared error of the mean in the variance (test_gpu_layers.py)."""
    C = x.shape[-1]
    g = np.ones(C) if gamma is None else gamma
    b = np.zeros(C) if beta is None else beta
    mean = x.mean(-1, keepdims=True)
    var = ((x - mean) ** 2).mean(-1, keepdims=True)
    inv = g / np.sqrt(var + eps)
    y = (x - mean) * inv + b
    A = np.abs(x).mean(-1, keepdims=True)
    mag = A * np.abs(inv) + np.abs(b) + np.abs(y)
    return y, mag, {'q': np.broadcast_to(A * A / (var + eps), y.shape)}


def softmax(x):
    """Softmax over the last axis.  aux['d'] = x - max (<= 0), aux['w'] = sum_c y_c |d_c|: what the bound needs."""
    d = x - x.max(-1, keepdims=True)
    e = np.exp(d)
    y = e / e.sum(-1, keepdims=True)
    return y, np.abs(y), {'d': d, 'w': np.broadcast_to((y * np.abs(d)).sum(-1, keepdims=True), y.shape)}


# ---- activations -----------------------------------------------------------------------------------------------------
ACTIVATIONS = ('linear', 'relu', 'relu6', 'sigmoid', 'tanh', 'elu', 'selu', 'softplus', 'softsign', 'swish', 'silu', 'gelu', 'hard_sigmoid',
               'exponential')
SELU_SCALE, SELU_ALPHA = 1.0507009873554804934193349852946, 1.6732632423543772848170429916717


def _sigmoid(x):
    e = np.exp(-np.abs(x))
    return np.where(x >= 0, 1.0 / (1.0 + e), e / (1.0 + e))


def activation(name, x, alpha=None):
    """The activation functions by their published formulas, each in the form that does not cancel in float64.
    ``alpha``: ELU's alpha, LeakyReLU's slope, ReLU's max_value ('relu_clip').  mag = |y| except where the formula itself
    cancels (hard_sigmoid near -2.5: |0.2 x| + 0.5; gelu for x << 0: |x / 2| (1 + |erf|))."""
    with np.errstate(over='ignore', under='ignore'):
        if name == 'linear':
            y = x
        elif name == 'relu':
            y = np.maximum(x, 0.0)
        elif name == 'relu6':
            y = np.clip(x, 0.0, 6.0)
        elif name == 'relu_clip':
            y = np.clip(x, 0.0, alpha)
        elif name == 'leaky_relu':
            y = np.where(x > 0, x, alpha * x)
        elif name == 'sigmoid':
            y = _sigmoid(x)
        elif name == 'tanh':
            y = np.tanh(x)
        elif name == 'elu':
            y = np.where(x > 0, x, (1.0 if alpha is None else alpha) * np.expm1(np.minimum(x, 0.0)))
        elif name == 'selu':
            y = SELU_SCALE * np.where(x > 0, x, SELU_ALPHA * np.expm1(np.minimum(x, 0.0)))
        elif name == 'softplus':
            y = np.maximum(x, 0.0) + np.log1p(np.exp(-np.abs(x)))
        elif name == 'softsign':
            y = x / (1.0 + np.abs(x))
        elif name in ('swish', 'silu'):
            y = x * _sigmoid(x)
        elif name == 'gelu':
            y = 0.5 * x * _erfc(-x / math.sqrt(2.0))
            return y, np.abs(0.5 * x) * (1.0 + np.abs(_erf(x / math.sqrt(2.0))))
        elif name == 'hard_sigmoid':
            return np.clip(0.2 * x + 0.5, 0.0, 1.0), np.abs(0.2 * x) + 0.5
        elif name == 'exponential':
            y = np.exp(x)
        else:
            raise NotImplementedError(name)
    return y, np.abs(y)


# ---- the graph walker ------------------------------------------------------------------------------------------------
def _w(weights, name):
    return [np.asarray(a, np.float64) for a in weights.get(name, [])]


def forward(cfg, weights, x, output=0):
    """The Functional configs of tests/layer_cases.py -> (y, mag, aux) of the chosen output layer, float64."""
    c = cfg['config']
    vals = {}
    for L in c['layers']:
        cls, lc, name = L['class_name'], L['config'], L['config']['name']
        if cls == 'InputLayer':
            v = np.asarray(x, np.float64)
            vals[name] = (v, np.abs(v), {})
            continue
        ins = [vals[r[0]][0] for r in L['inbound_nodes'][0]]
        a = ins[0]
        w = _w(weights, name)
        aux = {}
        if cls in ('MaxPooling2D', 'AveragePooling2D'):
            k, s = lc['pool_size'][0], (lc.get('strides') or lc['pool_size'])[0]
            y, mag = pool(a, k, s, lc.get('padding', 'valid'), cls == 'AveragePooling2D')
        elif cls in ('GlobalAveragePooling2D', 'GlobalMaxPooling2D'):
            y, mag = global_pool(a, cls == 'GlobalAveragePooling2D', bool(lc.get('keepdims')))
        elif cls == 'UpSampling2D':
            y, mag = upsample(a, lc['size'][0], lc.get('interpolation', 'nearest'))
        elif cls in ('ZeroPadding2D', 'Cropping2D'):
            # a copy: the magnitude and the bound's other terms travel with the values (the strided cases copy their result out)
            fn, arg = (zero_pad, lc['padding']) if cls == 'ZeroPadding2D' else (crop, lc['cropping'])
            src = vals[L['inbound_nodes'][0][0][0]]
            y, mag = fn(a, arg)[0], fn(src[1], arg)[0]
            aux = {k: fn(v, arg)[0] for k, v in src[2].items()}
        elif cls in ('Add', 'Subtract', 'Multiply', 'Maximum', 'Minimum', 'Average'):
            y, mag = merge(cls, ins)
        elif cls == 'Concatenate':
            y = np.concatenate(ins, axis=-1)
            mag = np.concatenate([vals[r[0]][1] for r in L['inbound_nodes'][0]], axis=-1)
            keys = set.intersection(*[set(vals[r[0]][2]) for r in L['inbound_nodes'][0]])
            aux = {k: np.concatenate([vals[r[0]][2][k] for r in L['inbound_nodes'][0]], axis=-1) for k in keys}
        elif cls == 'PReLU':
            y, mag = prelu(a, w[0])
        elif cls == 'BatchNormalization':
            gamma = w.pop(0) if lc.get('scale', True) else None
            beta = w.pop(0) if lc.get('center', True) else None
            y, mag = batchnorm(a, gamma, beta, w[0], w[1], lc.get('epsilon', 1e-3))
        elif cls == 'Normalization':
            y, mag = normalization(a, w[0].reshape(-1), w[1].reshape(-1))
        elif cls == 'LayerNormalization':
            gamma = w.pop(0) if lc.get('scale', True) else None
            beta = w.pop(0) if lc.get('center', True) else None
            y, mag, aux = layernorm(a, gamma, beta, lc.get('epsilon', 1e-3))
        elif cls == 'Softmax' or (cls == 'Activation' and lc['activation'] == 'softmax'):
            y, mag, aux = softmax(a)
        elif cls == 'Activation':
            y, mag = activation(lc['activation'], a)
        elif cls == 'ELU':
            y, mag = activation('elu', a, float(lc.get('alpha', 1.0)))
        elif cls == 'LeakyReLU':
            y, mag = activation('leaky_relu', a, float(lc.get('alpha', 0.3)))
        elif cls == 'ReLU':
            if lc.get('max_value') is not None:
                y, mag = activation('relu_clip', a, float(lc['max_value']))
            elif lc.get('negative_slope'):
                y, mag = activation('leaky_relu', a, float(lc['negative_slope']))
            else:
                y, mag = activation('relu', a)
        elif cls == 'Conv2D':
            # only the 1x1, bias-free, linear channel selections the cases use to make an (h, w, k) operand of the input
            assert lc['kernel_size'] == [1, 1] and not lc.get('use_bias', True) and lc.get('activation') in (None, 'linear')
            y = np.einsum('nhwc,co->nhwo', a, w[0][0, 0])
            mag = np.einsum('nhwc,co->nhwo', np.abs(a), np.abs(w[0][0, 0]))
        else:
            raise NotImplementedError(cls)
        vals[name] = (y, mag, aux)
    out = c['output_layers'][[r[0] for r in c['output_layers']].index(output) if isinstance(output, str) else int(output)][0]
    return vals[out]
