"""Plain numpy restatement of the convolution layers for tests/test_conv_exact.py (CPU) and tests/test_gpu_conv_exact.py (device):
Conv2D (stride, dilation rate, groups, per-axis strides / rates), DepthwiseConv2D, SeparableConv2D, Conv2DTranspose, Dense, and
what a case puts around them (2x2 MaxPooling2D, Flatten, Concatenate).  TEST INFRASTRUCTURE ONLY.

Arithmetic is int64 when the input and every weight are integers (the lattice cases: nothing rounds), float64 otherwise (the impulse
cases: every sum has one non-zero term, so nothing rounds either).  Geometry follows what ecseg_amd/keras_plan.py lowers
(``_conv_geometry`` and the Conv2DTranspose branch of ``build_plan``):

* 'same': out = ceil(n / s); total padding max((out - 1) s + (k - 1) d + 1 - n, 0), the smaller half in front;
* 'valid': out = (n - ((k - 1) d + 1)) // s + 1, no padding;
* transposed: the full result has (n - 1) s + max(k, s) rows; 'valid' keeps it, 'same' keeps n s rows from row max(k - s, 0) // 2 on.

Every layer function returns (y, S): S = sum |x| |w| + |b| over the receptive field of each output element, the quantity the
exactness preconditions are stated in.  ``forward`` returns the model output, the S of the layer that produced it, and one record per
weighted layer (max |input|, max |weight|, max |bias|, max S, input channels) for the per-layer preconditions.
"""
import numpy as np


def same_pad(k_eff, s, n):
    out = -(-n // s)
    total = max((out - 1) * s + k_eff - n, 0)
    return total // 2, total - total // 2


def _pair(v, default=1):
    if v is None:
        return default, default
    return (int(v), int(v)) if isinstance(v, int) else (int(v[0]), int(v[1]))


def _windows(x, kh, kw, strides, dilation, padding):
    """-> (zero-padded x, out_h, out_w)."""
    (sh, sw), (dh, dw) = strides, dilation
    n, h, w, c = x.shape
    ekh, ekw = (kh - 1) * dh + 1, (kw - 1) * dw + 1
    if padding == 'same':
        (pt, pb), (pl, pr) = same_pad(ekh, sh, h), same_pad(ekw, sw, w)
        oh, ow = -(-h // sh), -(-w // sw)
        x = np.pad(x, ((0, 0), (pt, pb), (pl, pr), (0, 0)))
    else:
        assert padding == 'valid', padding
        oh, ow = (h - ekh) // sh + 1, (w - ekw) // sw + 1
    assert oh > 0 and ow > 0
    return x, oh, ow


def _both(fn, x, w, b):
    """fn(x, w) on the values and on their magnitudes -> (y, S), the bias added to both."""
    y, s = fn(x, w), fn(np.abs(x), np.abs(w))
    if b is not None:
        y, s = y + b, s + np.abs(b)
    return y, s


def conv2d(x, w, b, strides=(1, 1), dilation=(1, 1), padding='same', groups=1):
    """x (N, H, W, C), w (kh, kw, C / groups, F): Keras Conv2D."""
    kh, kw, cg, f = w.shape
    fg = f // groups
    assert x.shape[3] == cg * groups and fg * groups == f

    def run(x, w):
        xp, oh, ow = _windows(x, kh, kw, strides, dilation, padding)
        y = np.zeros((x.shape[0], oh, ow, f), w.dtype)
        for r in range(kh):
            for q in range(kw):
                y0, x0 = r * dilation[0], q * dilation[1]
                win = xp[:, y0:y0 + (oh - 1) * strides[0] + 1:strides[0], x0:x0 + (ow - 1) * strides[1] + 1:strides[1], :]
                for g in range(groups):
                    y[..., g * fg:(g + 1) * fg] += win[..., g * cg:(g + 1) * cg] @ w[r, q, :, g * fg:(g + 1) * fg]
        return y
    return _both(run, x, w, b)


def depthwise2d(x, w, b, strides=(1, 1), dilation=(1, 1), padding='same'):
    """w (kh, kw, C, m): output channel c m + j = sum over taps of x[c] w[:, :, c, j]."""
    kh, kw, c, m = w.shape
    assert x.shape[3] == c

    def run(x, w):
        xp, oh, ow = _windows(x, kh, kw, strides, dilation, padding)
        y = np.zeros((x.shape[0], oh, ow, c * m), w.dtype)
        for r in range(kh):
            for q in range(kw):
                y0, x0 = r * dilation[0], q * dilation[1]
                win = xp[:, y0:y0 + (oh - 1) * strides[0] + 1:strides[0], x0:x0 + (ow - 1) * strides[1] + 1:strides[1], :]
                y += (win[..., :, None] * w[r, q]).reshape(y.shape)
        return y
    return _both(run, x, w, b)


def conv2d_transpose(x, w, b, stride, padding='same'):
    """w (kh, kw, F, C): input pixel (i, j) adds x[i, j] w[a, b] to the full result at (i s + a, j s + b)."""
    kh, kw, f, c = w.shape
    n, h, wd, _ = x.shape
    s = stride

    def run(x, w):
        full = np.zeros((n, (h - 1) * s + max(kh, s), (wd - 1) * s + max(kw, s), f), w.dtype)
        for a in range(kh):
            for q in range(kw):
                full[:, a:a + (h - 1) * s + 1:s, q:q + (wd - 1) * s + 1:s, :] += x @ w[a, q].T
        if padding == 'same':
            ct, cl = max(kh - s, 0) // 2, max(kw - s, 0) // 2
            return full[:, ct:ct + h * s, cl:cl + wd * s, :]
        assert padding == 'valid', padding
        return full
    return _both(run, x, w, b)


def maxpool2x2(x):
    n, h, w, c = x.shape
    x = x[:, :h // 2 * 2, :w // 2 * 2, :].reshape(n, h // 2, 2, w // 2, 2, c)
    return x.max(axis=(2, 4))


def _act(name, y):
    if name in (None, 'linear'):
        return y
    assert name == 'relu', name
    return np.maximum(y, 0)


def forward(cfg, weights, x):
    """-> (output, S of the output's layer, [per weighted layer: dict(name, cls, cin, max_x, max_w, max_b, max_s, w_mult4)])."""
    exact = np.asarray(x).dtype.kind in 'ui' or bool(np.all(np.asarray(x) == np.rint(x)))
    for ws in weights.values():
        exact = exact and all(bool(np.all(np.asarray(a) == np.rint(a))) for a in ws)
    dt = np.int64 if exact else np.float64
    conv = lambda a: np.asarray(a, np.float64).astype(dt)
    vals, mags, recs = {}, {}, []
    layers = cfg['config']['layers']
    for L in layers:
        cls, lc = L['class_name'], L['config']
        name = lc['name']
        if cls == 'InputLayer':
            vals[name] = conv(x)
            mags[name] = np.abs(vals[name])
            continue
        ins = [r[0] for r in L['inbound_nodes'][0]]
        a = vals[ins[0]]
        w = [conv(v) for v in weights.get(name, [])]
        use_bias = lc.get('use_bias', True)

        def rec(cin, xin, ws, bias, s):
            recs.append(dict(name=name, cls=cls, cin=cin, max_x=float(np.abs(xin).max()), max_w=max(float(np.abs(v).max()) for v in ws),
                             max_b=float(np.abs(bias).max()) if bias is not None else 0.0, max_s=float(s.max()),
                             w_mult4=all(bool(np.all(np.asarray(v) % 4 == 0)) for v in ws)))

        if cls == 'Conv2D':
            bias = w[1] if use_bias else None
            y, s = conv2d(a, w[0], bias, _pair(lc.get('strides')), _pair(lc.get('dilation_rate')), lc['padding'], int(lc.get('groups', 1) or 1))
            rec(w[0].shape[2], a, [w[0]], bias, s)
            y = _act(lc.get('activation'), y)
        elif cls == 'DepthwiseConv2D':
            bias = w[1] if use_bias else None
            y, s = depthwise2d(a, w[0], bias, _pair(lc.get('strides')), _pair(lc.get('dilation_rate')), lc['padding'])
            rec(1, a, [w[0]], bias, s)
            y = _act(lc.get('activation'), y)
        elif cls == 'SeparableConv2D':
            bias = w[2] if use_bias else None
            mid, s0 = depthwise2d(a, w[0], None, _pair(lc.get('strides')), _pair(lc.get('dilation_rate')), lc['padding'])
            rec(1, a, [w[0]], None, s0)
            y, s = conv2d(mid, w[1], bias, padding='valid')
            rec(w[1].shape[2], mid, [w[1]], bias, s)
            y = _act(lc.get('activation'), y)
        elif cls == 'Conv2DTranspose':
            bias = w[1] if use_bias else None
            st = _pair(lc['strides'])
            assert st[0] == st[1]
            y, s = conv2d_transpose(a, w[0], bias, st[0], lc['padding'])
            rec(w[0].shape[3], a, [w[0]], bias, s)
            y = _act(lc.get('activation'), y)
        elif cls == 'Dense':
            bias = w[1] if use_bias else None
            y, s = _both(lambda p, q: p @ q, a, w[0], bias)
            rec(w[0].shape[0], a, [w[0]], bias, s)
            y = _act(lc.get('activation'), y)
        elif cls == 'MaxPooling2D':
            assert list(lc['pool_size']) == [2, 2] and list(lc.get('strides') or [2, 2]) == [2, 2] and lc.get('padding', 'valid') == 'valid'
            y, s = maxpool2x2(a), maxpool2x2(mags[ins[0]])
        elif cls == 'Flatten':
            y, s = a.reshape(a.shape[0], -1), mags[ins[0]].reshape(a.shape[0], -1)
        elif cls == 'Concatenate':
            y, s = np.concatenate([vals[i] for i in ins], axis=-1), np.concatenate([mags[i] for i in ins], axis=-1)
        else:
            raise AssertionError('conv_exact_ref has no layer %s' % cls)
        vals[name], mags[name] = y, s
    out = cfg['config']['output_layers'][0][0]
    return vals[out], mags[out], recs
