"""A float64 interpreter of a Keras ``model_config`` for tests/test_plan_ref.py (CPU) and tests/test_gpu_plan.py (device).
TEST INFRASTRUCTURE ONLY.

It holds ``ecseg_amd/keras_plan.py::build_plan`` - the step that rewrites a Keras graph into what the kernels run - to the graph as
Keras defines it: every layer is evaluated on its own, in numpy float64, NHWC, in dependency order over ``inbound_nodes``.  Nothing is
folded, fused, viewed or re-used here, and nothing is imported from ``ecseg_amd``; the per-layer arithmetic comes from
tests/layer_ref.py and tests/conv_exact_ref.py.

``forward(cfg, weights, x)`` returns ``{tensor name: (y, A)}`` for every tensor of the graph.  ``A >= |y|`` is the same graph evaluated
on ``|x|`` with ``|weights|`` and ``|bias|``: a convolution of ``A`` with ``|w|`` plus ``|b|``; BatchNormalization as
``|gamma| / sqrt(var + eps) * (A + |mean|) + |beta|``; an activation by its Lipschitz bound ``L A + |f(0)|``; pools, concatenations,
crops and pads passed through.  A float32 evaluation of the graph in any summation order, with any of the legitimate rewrites
(a scale folded into a filter, two filters summed before they are applied), errs by a small multiple of ``2^-24 A`` per element; that
multiple is ``C_BOUND`` of tests/plan_cases.py.

Tensor names: a layer's name; call ``j >= 1`` of a shared layer is ``name/call<j>``; layer ``l`` of a nested model ``m`` is ``m/l``
(the names ``Plan.layer_tensor`` uses, so that a test can look both up by one key).

Every keyword argument of ``forward`` is a slip a graph rewrite could make (the manner of tests/stitch_pre_ref.py): the mutant differs
from the reference by that switch alone.

* ``bn_eps``: every BatchNormalization uses this epsilon instead of its own;
* ``bn_fold_axis``: a BatchNormalization that is the only consumer of a linear convolution scales the filter along its INPUT channel
  axis (possible when in == out: Conv2D (kh, kw, in, out), Conv2DTranspose (kh, kw, out, in)), or along the transposed
  (multiplier, channel) order of a depthwise filter (kh, kw, c, m);
* ``bn_after_activation``: conv(act) -> BN evaluated as act(BN(conv));
* ``leaky_alpha``: every LeakyReLU slope forced to this value;
* ``norm_floor=False``: Normalization divides by sqrt(var) without the floor of 1e-7;
* ``lambda_order``: an affine input map (Rescaling, an overridden Lambda) adds its offset before it scales;
* ``upsample_nearest_phase``: nearest UpSampling2D reads in[(y + 1) // f] (clamped) instead of in[y // f];
* ``concat_order``: Concatenate takes its inputs in reverse;
* ``pool_before_activation``: act -> pool evaluated as act(pool(.));
* ``same_pad_low``: 'same' padding of a convolution puts the larger half in front;
* ``shared_second_call_first_input``: calls 1.. of a shared layer read what call 0 read;
* ``stale_buffer=(producer, victim)``: once ``producer`` is computed, readers of ``victim`` see the producer's values (a buffer handed
  on while its tensor was still to be read).  ``stale_pairs`` lists the pairs that are a fault: equal shape, the victim read later.
"""
import numpy as np

import conv_exact_ref as cx
import layer_ref as lr

MODEL_CLASSES = ('Functional', 'Model', 'Sequential')
IDENTITY = ('Dropout', 'SpatialDropout2D', 'GaussianNoise', 'GaussianDropout', 'AlphaDropout', 'ActivityRegularization')
MERGES = ('Add', 'Subtract', 'Multiply', 'Maximum', 'Minimum', 'Average')
SWITCHES = dict(bn_eps=None, bn_fold_axis=False, bn_after_activation=False, leaky_alpha=None, norm_floor=True, lambda_order=False,
                upsample_nearest_phase=False, concat_order=False, pool_before_activation=False, same_pad_low=False,
                shared_second_call_first_input=False, stale_buffer=None)
# activation -> (Lipschitz constant, |f(0)|) of the magnitude rule A' = L A + |f(0)|
LIPSCHITZ = {'linear': (1.0, 0.0), 'relu': (1.0, 0.0), 'sigmoid': (0.25, 0.5), 'tanh': (1.0, 0.0), 'selu': (lr.SELU_SCALE * lr.SELU_ALPHA, 0.0),
             'softplus': (1.0, float(np.log(2.0))), 'softsign': (1.0, 0.0), 'swish': (1.1, 0.0), 'silu': (1.1, 0.0), 'gelu': (1.13, 0.0),
             'hard_sigmoid': (0.2, 0.5)}


def _pair(v, default=1):
    if v is None:
        return default, default
    return (int(v), int(v)) if isinstance(v, int) else (int(v[0]), int(v[1]))


def activate(name, alpha, y, A):
    """(y, A) through the activation ``name`` (a Keras activation name, or 'leaky_relu' / 'relu_clip' / 'elu' with ``alpha``)."""
    if isinstance(name, dict):
        name = (name.get('config') or {}).get('name', name.get('class_name'))
    name = 'linear' if name is None else name
    if name == 'softmax':
        v = lr.softmax(y)[0]
        return v, 0.5 * A.max(-1, keepdims=True) + v
    if name == 'exponential':
        v = np.exp(y)
        return v, v * (1.0 + A)
    if name == 'leaky_relu':
        return lr.activation(name, y, alpha)[0], A * max(1.0, abs(alpha))
    if name == 'relu_clip' or name == 'relu6':
        cap = 6.0 if name == 'relu6' else alpha
        return np.clip(y, 0.0, cap), A
    if name == 'elu':
        al = 1.0 if alpha is None else alpha
        return lr.activation('elu', y, al)[0], A * max(1.0, abs(al))
    L, f0 = LIPSCHITZ[name]
    return lr.activation(name, y)[0], L * A + f0


def _pad_same(a, ek, s, axis, low):
    lo, hi = lr.same_pad(ek, s, a.shape[axis])
    if low:
        lo, hi = hi, lo
    pads = [(0, 0)] * 4
    pads[axis] = (lo, hi)
    return np.pad(a, pads)


def _conv_like(cls, lc, w, sw):
    """-> (fn(x, kernel, bias) -> linear result, kernel, bias, output-channel count) of a Conv2D / DepthwiseConv2D / Conv2DTranspose /
    Dense config.  'same' padding is applied here (so that ``same_pad_low`` can move it) and the layer function runs 'valid'."""
    bias = None
    if cls == 'Dense':
        if lc.get('use_bias', True):
            bias = w[1]
        return (lambda x, k, b: x @ k + (0.0 if b is None else b)), w[0], bias
    if cls == 'Conv2DTranspose':
        st = _pair(lc['strides'])
        assert st[0] == st[1]
        if lc.get('use_bias', True):
            bias = w[1]
        return (lambda x, k, b: cx.conv2d_transpose(x, k, b, st[0], lc['padding'])[0]), w[0], bias
    st, dil = _pair(lc.get('strides')), _pair(lc.get('dilation_rate'))
    kh, kw = lc['kernel_size']
    if lc.get('use_bias', True):
        bias = w[1]

    def run(x, k, b):
        if lc['padding'] == 'same':
            x = _pad_same(x, (kh - 1) * dil[0] + 1, st[0], 1, sw['same_pad_low'])
            x = _pad_same(x, (kw - 1) * dil[1] + 1, st[1], 2, sw['same_pad_low'])
        if cls == 'DepthwiseConv2D':
            return cx.depthwise2d(x, k, b, st, dil, 'valid')[0]
        return cx.conv2d(x, k, b, st, dil, 'valid', int(lc.get('groups', 1) or 1))[0]
    return run, w[0], bias


def _abs(a):
    return None if a is None else np.abs(a)


def _consumers(calls):
    n = {}
    for key, (_, _, refs) in calls.items():
        for r in refs:
            n[r[0]] = n.get(r[0], 0) + 1
    return n


def _norm_node(node):
    if isinstance(node, dict):
        raise NotImplementedError('Keras 3 model_config')
    if node and isinstance(node[0], str):
        node = [node]
    return [list(r) for r in node]


def call_key(name, j):
    return name if not j else '%s/call%d' % (name, j)


def _calls(model):
    """A Functional / Sequential model -> (ordered {call key: (layer, call index, [(key of the consumed call, tensor index, kwargs)])},
    [input call keys], [(output call key, tensor index)])."""
    cfg = model['config']
    layers = cfg['layers'] if isinstance(cfg, dict) else cfg
    pending = []
    if model['class_name'] == 'Sequential':
        prev, ins = None, []
        for L in layers:
            name = L['config']['name']
            if L['class_name'] == 'InputLayer':
                pending.append((name, L, 0, []))
                ins.append(name)
            else:
                if prev is None:
                    first = dict(class_name='InputLayer', config=dict(name='__input__', batch_input_shape=L['config'].get('batch_input_shape')))
                    pending.append(('__input__', first, 0, []))
                    ins.append('__input__')
                    prev = '__input__'
                pending.append((name, L, 0, [(prev, 0, {})]))
            prev = name
        outs = [(prev, 0)]
    else:
        for L in layers:
            name = L['config']['name']
            nodes = L.get('inbound_nodes', [])
            if not nodes:
                pending.append((name, L, 0, []))
            for j, node in enumerate(nodes):
                refs = [(call_key(r[0], r[1] if len(r) > 1 and isinstance(r[1], int) else 0), r[2] if len(r) > 2 and isinstance(r[2], int) else 0,
                         r[3] if len(r) > 3 and isinstance(r[3], dict) else {}) for r in _norm_node(node)]
                pending.append((call_key(name, j), L, j, refs))
        ins = [call_key(r[0], r[1]) for r in cfg['input_layers']]
        outs = [(call_key(r[0], r[1]), r[2]) for r in cfg['output_layers']]
    calls, ready = {}, set()
    while pending:                      # stable dependency order: a later call of a shared layer may consume layers listed after it
        rest = []
        for item in pending:
            if all(r[0] in ready for r in item[3]):
                calls[item[0]] = (item[1], item[2], item[3])
                ready.add(item[0])
            else:
                rest.append(item)
        assert len(rest) < len(pending), 'the layer graph has a cycle or a dangling reference'
        pending = rest
    return calls, ins, outs


def _nested_weights(ws):
    if ws is None or isinstance(ws, dict):
        return ws or {}
    d = {}
    for nm, a in zip(ws.names, ws):
        parts = str(nm).split(':')[0].split('/')
        d.setdefault(parts[-2] if len(parts) >= 2 else parts[0], []).append(a)
    return d


def forward(cfg, weights, x, lambda_affine=None, **switches):
    """-> {tensor name: (y, A)}, float64 NHWC (rank-2 tensors (N, K)); ``x`` is what the Keras model takes ((N, C, H, W) for a
    channels_first model).  ``lambda_affine``: {Lambda layer name: (scale, offset)}.  Keys ``'@order'``: the tensor names in the order
    they were computed; ``'@outputs'``: the names of the model's outputs."""
    sw = dict(SWITCHES)
    for k in switches:
        if k not in sw:
            raise TypeError('unknown switch %r' % k)
    sw.update(switches)
    layers = cfg['config']['layers'] if isinstance(cfg['config'], dict) else cfg['config']
    cf = any(L['config'].get('data_format') == 'channels_first' for L in layers)
    v = np.asarray(x, np.float64)
    if v.ndim == 3:
        v = v[..., None]
    if cf:
        v = np.transpose(v, (0, 2, 3, 1))
    vals = {'@order': []}
    outs = _run(cfg, weights, [(v, np.abs(v))], '', cf, lambda_affine or {}, sw, vals)
    vals['@outputs'] = outs
    return vals


def _run(model, weights, inputs, prefix, cf, lam, sw, vals):
    calls, in_keys, out_refs = _calls(model)
    ncons = _consumers(calls)
    for k, _ in out_refs:
        ncons[k] = ncons.get(k, 0) + 1
    rec = {}                                 # call key -> what the mutants need of a producer
    chan_ok = (lambda ax: ax in (1, -3)) if cf else (lambda ax: ax in (-1, 3))

    def get(ref):
        val = vals[prefix + ref[0]]
        return val[ref[1]] if isinstance(val, list) else val

    for key, (L, j, refs) in calls.items():
        cls, lc = L['class_name'], L['config']
        name = lc['name']
        full = prefix + key
        if cls == 'InputLayer':
            vals[full] = inputs[in_keys.index(key)]
            vals['@order'].append(full)
            continue
        if j and sw['shared_second_call_first_input']:
            refs = calls[call_key(name, 0)][2]
        ins = [get(r) for r in refs]
        a, A = ins[0]
        w = [np.asarray(t, np.float64) for t in (weights.get(name) or [])] if cls not in MODEL_CLASSES else None
        src = rec.get(refs[0][0]) if ncons.get(refs[0][0], 0) == 1 else None      # the producer, when this call is its only reader
        r = None
        if cls in MODEL_CLASSES:
            outs = _run({'class_name': cls, 'config': lc}, _nested_weights(weights.get(name)), ins, full + '/', cf, lam, sw, vals)
            vals[full] = [vals[o] for o in outs]
            continue
        elif cls in ('Conv2D', 'DepthwiseConv2D', 'Conv2DTranspose', 'Dense'):
            fn, k, b = _conv_like(cls, lc, w, sw)
            pre = fn(a, k, b)
            preA = fn(A, np.abs(k), _abs(b))
            wrong = None
            if cls == 'DepthwiseConv2D':
                c, m = k.shape[2], k.shape[3]
                wrong = lambda s, fn=fn, a=a, k=k, c=c, m=m: fn(a, k, None) * s.reshape(m, c).T.reshape(-1)
            elif k.shape[-1] == k.shape[-2] and int(lc.get('groups', 1) or 1) == 1:
                wrong = lambda s, fn=fn, a=a, k=k: fn(a * s, k, None)
            act = lc.get('activation')
            y, A2 = activate(act, None, pre, preA)
            r = dict(pre=(pre, preA), act=(act, None), linear=act in (None, 'linear'), wrong=wrong, bias=b)
        elif cls == 'SeparableConv2D':
            dfn, dk, _ = _conv_like('DepthwiseConv2D', dict(lc, use_bias=False), w, sw)
            mid, midA = dfn(a, dk, None), dfn(A, np.abs(dk), None)
            b = w[2] if lc.get('use_bias', True) else None
            pk = w[1][0, 0]
            pre = mid @ pk + (0.0 if b is None else b)
            preA = midA @ np.abs(pk) + (0.0 if b is None else np.abs(b))
            wrong = (lambda s, mid=mid, pk=pk: (mid * s) @ pk) if pk.shape[0] == pk.shape[1] else None
            act = lc.get('activation')
            y, A2 = activate(act, None, pre, preA)
            r = dict(pre=(pre, preA), act=(act, None), linear=act in (None, 'linear'), wrong=wrong, bias=b)
        elif cls in ('MaxPooling2D', 'AveragePooling2D'):
            kk, ss = _pair(lc['pool_size']), _pair(lc.get('strides') or lc['pool_size'])
            assert kk[0] == kk[1] and ss[0] == ss[1]
            avg = cls == 'AveragePooling2D'
            pool = lambda t: lr.pool(t, kk[0], ss[0], lc.get('padding', 'valid'), avg)[0]
            if sw['pool_before_activation'] and src is not None and not src['linear']:
                y, A2 = activate(src['act'][0], src['act'][1], pool(src['pre'][0]), pool(src['pre'][1]))
            else:
                y, A2 = pool(a), pool(A)
        elif cls in ('GlobalAveragePooling2D', 'GlobalMaxPooling2D'):
            avg, kd = cls == 'GlobalAveragePooling2D', bool(lc.get('keepdims'))
            y, A2 = lr.global_pool(a, avg, kd)[0], lr.global_pool(A, avg, kd)[0]
        elif cls == 'Flatten':
            y, A2 = a.reshape(a.shape[0], -1), A.reshape(a.shape[0], -1)
        elif cls == 'Reshape':
            ts = [int(t) for t in lc['target_shape']]
            ts = ts + [1] if len(ts) == 2 else ts
            y, A2 = a.reshape([a.shape[0]] + ts), A.reshape([a.shape[0]] + ts)
        elif cls == 'UpSampling2D':
            f = _pair(lc['size'])
            assert f[0] == f[1]
            interp = lc.get('interpolation', 'nearest')
            if interp == 'nearest' and sw['upsample_nearest_phase']:
                iy = np.minimum((np.arange(a.shape[1] * f[0]) + 1) // f[0], a.shape[1] - 1)
                ix = np.minimum((np.arange(a.shape[2] * f[0]) + 1) // f[0], a.shape[2] - 1)
                y, A2 = a[:, iy][:, :, ix], A[:, iy][:, :, ix]
            else:
                y, A2 = lr.upsample(a, f[0], interp)[0], lr.upsample(A, f[0], interp)[0]
        elif cls == 'Concatenate':
            assert chan_ok(lc.get('axis', -1)), 'Concatenate over the channel axis only'
            parts = ins[::-1] if sw['concat_order'] else ins
            y, A2 = np.concatenate([p[0] for p in parts], -1), np.concatenate([p[1] for p in parts], -1)
        elif cls in MERGES:
            y = lr.merge(cls, [p[0] for p in ins])[0]
            mags = [p[1] for p in ins]
            if cls in ('Add', 'Subtract', 'Average'):
                A2 = sum(mags) / (len(ins) if cls == 'Average' else 1)
            elif cls == 'Multiply':
                A2 = np.prod(np.broadcast_arrays(*mags), axis=0)
            else:
                A2 = np.max(np.broadcast_arrays(*mags), axis=0)
        elif cls == 'PReLU':
            al = w[0]
            if cf and al.ndim == 3:
                al = np.transpose(al, (1, 2, 0))
            y, A2 = lr.prelu(a, al)[0], A * np.maximum(1.0, np.abs(al))
            r = dict(pre=(a, A), act=None, linear=False)
        elif cls == 'LayerNormalization':
            wl = list(w)
            g = wl.pop(0) if lc.get('scale', True) else np.ones(a.shape[-1])
            b = wl.pop(0) if lc.get('center', True) else np.zeros(a.shape[-1])
            eps = lc.get('epsilon', 1e-3)
            y = lr.layernorm(a, g, b, eps)[0]
            var = ((a - a.mean(-1, keepdims=True)) ** 2).mean(-1, keepdims=True)
            A2 = np.abs(g) / np.sqrt(var + eps) * (A + A.mean(-1, keepdims=True)) + np.abs(b)
        elif cls == 'Normalization':
            if lc.get('mean') is not None:
                mean, var = np.asarray(lc['mean'], np.float64).reshape(-1), np.asarray(lc['variance'], np.float64).reshape(-1)
            else:
                mean, var = w[0].reshape(-1), w[1].reshape(-1)
            inv = 1.0 / (np.maximum(np.sqrt(var), 1e-7) if sw['norm_floor'] else np.sqrt(var))
            y, A2 = (a - mean) * inv, (A + np.abs(mean)) * inv
        elif cls == 'BatchNormalization':
            ax = lc.get('axis', -1)
            ax = ax[0] if isinstance(ax, (list, tuple)) else ax
            assert chan_ok(ax) or a.ndim == 2, 'BatchNormalization over the channel axis only'
            wl = list(w)
            C = a.shape[-1]
            g = wl.pop(0) if lc.get('scale', True) else np.ones(C)
            b = wl.pop(0) if lc.get('center', True) else np.zeros(C)
            mean, var = wl[0], wl[1]
            eps = lc.get('epsilon', 1e-3) if sw['bn_eps'] is None else sw['bn_eps']
            s = g / np.sqrt(var + eps)
            t = b - mean * s
            y, A2 = a * s + t, np.abs(s) * (A + np.abs(mean)) + np.abs(b)
            if sw['bn_fold_axis'] and src is not None and src.get('wrong') is not None and src['linear']:
                y = src['wrong'](s) + ((0.0 if src['bias'] is None else src['bias']) * s + t)
            elif sw['bn_after_activation'] and src is not None and src.get('act') is not None and not src['linear']:
                y = activate(src['act'][0], src['act'][1], src['pre'][0] * s + t, A2)[0]
        elif cls == 'Rescaling' or cls == 'Lambda':
            sc, of = (float(lc['scale']), float(lc.get('offset', 0.0))) if cls == 'Rescaling' else (float(t) for t in lam[name])
            y = (a + of) * sc if sw['lambda_order'] else a * sc + of
            A2 = A * abs(sc) + abs(of)
        elif cls == 'TFOpLambda':
            fn = lc.get('function', '')
            kw = refs[0][2]
            c = kw.get('y', kw.get('x'))
            if fn in ('cast', 'identity', 'stop_gradient'):
                y, A2 = a, A
            elif fn in ('math.truediv', 'math.divide', '__operators__.truediv'):
                y, A2 = a / float(c), A / abs(float(c))
            elif fn in ('math.multiply', '__operators__.mul'):
                y, A2 = a * float(c), A * abs(float(c))
            elif fn in ('math.add', '__operators__.add'):
                y, A2 = a + float(c), A + abs(float(c))
            elif fn in ('math.subtract', '__operators__.sub'):
                y, A2 = a - float(c), A + abs(float(c))
            else:
                raise NotImplementedError('TFOpLambda %s' % fn)
        elif cls in IDENTITY:
            y, A2 = a, A
            r = rec.get(refs[0][0])
        elif cls in ('Activation', 'ReLU', 'LeakyReLU', 'ELU', 'Softmax'):
            if cls == 'Activation':
                act = (lc['activation'], None)
            elif cls == 'ReLU':
                assert not lc.get('threshold')
                if lc.get('max_value') is not None:
                    act = ('relu_clip', float(lc['max_value']))
                elif lc.get('negative_slope'):
                    act = ('leaky_relu', float(lc['negative_slope']) if sw['leaky_alpha'] is None else sw['leaky_alpha'])
                else:
                    act = ('relu', None)
            elif cls == 'LeakyReLU':
                act = ('leaky_relu', float(lc.get('alpha', 0.3)) if sw['leaky_alpha'] is None else sw['leaky_alpha'])
            elif cls == 'ELU':
                act = ('elu', float(lc.get('alpha', 1.0)))
            else:
                assert chan_ok(lc.get('axis', -1)) or a.ndim == 2, 'Softmax over the channel axis only'
                act = ('softmax', None)
            y, A2 = activate(act[0], act[1], a, A)
            r = dict(pre=(a, A), act=act, linear=False)
        elif cls == 'ZeroPadding2D':
            y, A2 = lr.zero_pad(a, lc['padding'])[0], lr.zero_pad(A, lc['padding'])[0]
        elif cls == 'Cropping2D':
            y, A2 = lr.crop(a, lc['cropping'])[0], lr.crop(A, lc['cropping'])[0]
        else:
            raise NotImplementedError('Keras layer %s' % cls)
        if r is not None:
            rec[key] = r
        vals[full] = (y, A2)
        vals['@order'].append(full)
        st = sw['stale_buffer']
        if st is not None and st[0] == full and isinstance(vals.get(st[1]), tuple) and vals[st[1]][0].shape == y.shape:
            vals[st[1]] = (y, A2)
    return [prefix + k for k, _ in out_refs]


def stale_pairs(cfg, weights, x, outputs=()):
    """The (producer, victim) pairs of a flat graph that a buffer allocator must not merge: two tensors of equal shape, the victim
    computed first and still to be read - by a layer that runs after the producer, or as an output (``outputs``: further kept names) -
    when the producer is written.  A victim whose last reader is the producer itself, or runs before it, is a legitimate re-use and
    changes nothing, so it is no pair."""
    vals = forward(cfg, weights, x)
    order = vals['@order']
    pos = {k: i for i, k in enumerate(order)}
    calls = _calls(cfg)[0]
    last_read = {k: -1 for k in order}
    for key, (_, _, refs) in calls.items():
        for r in refs:
            last_read[r[0]] = max(last_read[r[0]], pos[key])
    for k in tuple(vals['@outputs']) + tuple(outputs):
        last_read[k] = len(order)
    pairs = []
    for v in order:
        for p in order:
            if pos[p] > pos[v] and vals[p][0].shape == vals[v][0].shape and last_read[v] > pos[p]:
                pairs.append((p, v))
    return pairs
