"""Every non-convolution layer kernel ALONE against tests/layer_ref.py's float64 restatement, element by element, on the cases of
tests/layer_cases.py (the maxpool / pool_pad / global_pool / upsample / affine / binary / prelu / copy / layernorm / softmax
kernels of csrc/layer_kernels.hip and the activation codes of device_util.h).  tests/test_layers_ref.py ties layer_ref to the
float64 oracle.  Every Add of a plan runs on binary_kernel: test_add_of_two_inputs_is_exact holds it to numpy's float32 sum, bit for bit.

Bounds.  u = 2^-24 is the relative error of one correctly rounded float32 operation (half an ulp), so a library function
with an error ceiling of k ulp contributes 2k u.  Every bound but round1's is |got - want64| <= n_ops * u * mag * SECOND + floor, with
``mag`` from layer_ref and n_ops counted from the kernel's own operation sequence (a fused multiply-add only removes
roundings).  SECOND = 1 + 2^-10 stands for the products of errors that a first-order count leaves out.

  class       ops                                 n_ops and where they come from
  ----------  ----------------------------------  -----------------------------------------------------------------------
  select      max pool, global max, nearest,      0: the output is one of the inputs (or 0 / the clip value): equal to
              pad / crop, Maximum / Minimum,      float32(want64).  Only a zero whose sign differs is let through
              ReLU, ReLU(max_value), linear       (fmaxf(+0, -0), v > 0 ? v : 0): counted, and nothing else may differ.
  round1      Add / Subtract / Multiply (two      one operation on exact float32 operands: u |want64|, however far the operands
              inputs), LeakyReLU, PReLU           cancel, and no SECOND.  Floor: one float32 denormal, 2^-149.
  sum         Add of n inputs                     n - 1 additions; mag = sum |x_i|
              Average of n inputs                 (n - 1) additions + rounding of 1 / n + 1 multiplication; mag = sum |x_i| / n
  avgpool     AveragePooling2D, window k x k      k^2 - 1 additions + rounding of 1 / k^2 + 1 multiplication = k^2 + 1 ('same':
                                                  count - 1 additions + 1 division, which is less); mag = sum |x| / count
  global_avg  GlobalAveragePooling2D, P pixels    ceil(P / 4) - 1 additions in a wave + 3 to join the four waves + rounding of
                                                  1 / P + 1 multiplication = ceil(P / 4) + 4; mag = mean |x|
  affine      BatchNormalization, Normalization   4: the float32 roundings of the folded scale and shift, the multiplication,
                                                  the addition; mag = |x scale| + |shift|
  bilinear    UpSampling2D(bilinear), factor f    10: each of the three lerps a + (b - a) t is 3 operations on values <= 2 mag,
                                                  <= mag after the weight (5 u mag); the two row lerps feed the column lerp
                                                  with their 5, which adds its own 5.  f = 3 only: 1 / 3 is rounded, so the source
                                                  coordinate (dst + 0.5) * (1/3) - 0.5 carries 3 roundings of a value <= the input
                                                  extent and moves the lerp by that times |b - a| <= 2 mag: + 6 (h + w).
                                                  mag = the largest |corner|
  layernorm   LayerNormalization, C channels,     D = ceil(C / LPP) - 1 + log2(LPP) additions per sum.  mean: D + rounding of
              LPP = 4 / 16 / 64 lanes per pixel   1 / C + 1 multiplication = D + 2, times A |inv| (A = mean |x| >= |mean|).
              (C < 16, < 64, >= 64)               inv = gamma rsqrt(var + eps): rsqrt 2 ulp = 4; var * (1/C) + eps with eps rounded = 4
                                                  on the argument = 2; var itself 2 (the centred values) + D + 1 (the sum) = D + 3 on
                                                  the argument = (D + 3) / 2; times gamma 1: 8.5 + D / 2, times |y - beta|.
                                                  x * inv + (beta - mean * inv): 3.  Sum: 1.5 D + 13.5.  The error e of the mean
                                                  enters the variance only as e^2 (sum of the centred values = 0):
                                                  + (D + 2)^2 u q / 2, q = A^2 / (var + eps) from layer_ref.
                                                  mag = A |inv| + |beta| + |y|: it contains |mean| inv, the cancellation of the formula
  softmax     softmax_kernel, C channels (of      x - max: 1 on |d| -> |d| on exp; expf 3 ulp = 6: 6 + |d_c| per term; the sum carries
              the view the kernel reads)          the terms' weighted mean 6 + w (w = sum y_c |d_c|) and C - 1 additions; 1 division:
                                                  13 + C + |d_c| + w.  Floor: FLT_MIN
  act         apply_act / apply_act_ext           OCML's ceilings are OpenCL's single-precision table: exp 3, expm1 3, log1p 2, tanh 5,
                                                  erf 16 ulp; division and the basic operations are correctly rounded.  Per formula:
              sigmoid  1 / (1 + expf(-v))         expf 6 (at most that on the sum) + addition 1 + division 1 = 8
              swish    v / (1 + expf(-v))         8; where expf(-v) overflows (-v > ln FLT_MAX) the quotient is 0: floor |v| / FLT_MAX
              tanh     tanhf                      10
              elu      alpha * expm1f(v)          6 + 1 = 7
              selu     s * (a * expm1f(v))        6 + two rounded constants + two multiplications = 10
              softplus max(v, 0) + log1pf(expf(-|v|))   l = log1p(e): e carries 6, d log1p(e) = de / (1 + e) <= l * 6, log1pf 2 ulp = 4:
                                                  10 on l, + 1 on the sum: (10 l + y) u
              softsign v / (1 + |v|)              2
              exponential expf                    6
              hard_sigmoid clip(0.2f v + 0.5)     3 on mag = |0.2 v| + 0.5: the constant, the multiplication, the addition
              gelu  0.5 v (1 + erff(v c))         c = 1/sqrt 2 rounded + 1 multiplication: 2 on t = v c, i.e. 2 |t| erf'(t); erff 16 ulp =
                                                  32 |erf|; the addition 1 |s|: ds = 32 |erf| + 2 |t| erf'(t) + |s|; |0.5 v| ds + 1 |y|
                                                  Floor for all of them: FLT_MIN (results below it are denormal)

Every case also asserts the output shape, that the output is finite wherever float32 holds the reference, and identical
bytes from a second call.  The worst error of each activation is printed next to its ceiling, in ulp = 2^-23 of the float64
value (of ``mag`` for hard_sigmoid and gelu, whose formulas cancel), over the elements whose bound is not its floor (DESIGN.md
records the table).
"""
import math

import numpy as np
import pytest

from ecseg_amd import keras_plan

from tests import layer_cases, layer_ref

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
SECOND = 1.0 + 2.0 ** -10
DENORMAL = 2.0 ** -149
FLT_MIN = 2.0 ** -126
FLT_MAX = float(np.finfo(np.float32).max)

SELECT_ACTS = ('linear', 'relu', 'relu6', 'relu_clip')
# n_ops of the activations whose bound is n_ops * u * mag (+ FLT_MIN); softplus, gelu and swish's overflow floor are formulas below
ACT_OPS = {'sigmoid': 8, 'swish': 8, 'silu': 8, 'tanh': 10, 'elu': 7, 'selu': 10, 'softsign': 2, 'exponential': 6,
           'hard_sigmoid': 3}


def _ln_ops(c, q):
    c = np.asarray(c)                                           # a scalar, or per output channel (strided views of 2 and 4 channels)
    lpp = np.where(c >= 64, 64, np.where(c >= 16, 16, 4))
    d = -(-c // lpp) - 1 + np.log2(lpp)
    return 1.5 * d + 13.5 + 0.5 * (d + 2) ** 2 * U * q


def tolerance(case, x, want, mag, aux):
    """-> None for the select class (exact), else (relative part, floor) of the per-element bound: their sum is the bound."""
    k = case['kind']
    op = k['op']
    if op == 'act' and k['fn'] in SELECT_ACTS:
        op = 'select'
    if op == 'act' and k['fn'] == 'leaky_relu':
        op = 'round1'
    if op == 'select':
        return None
    floor = DENORMAL
    if op == 'round1':
        return U * np.abs(want), floor                          # one correctly rounded operation: no magnitude but |want|, no second order
    elif op == 'sum':
        n = float(k['n_ops'])
    elif op == 'avgpool':
        n = k['k'] ** 2 + 1.0
    elif op == 'global_avg':
        n = -(-k['npx'] // 4) + 4.0
    elif op == 'affine':
        n = 4.0
    elif op == 'bilinear':
        n = 10.0 + (6.0 * (k['h'] + k['w']) if k['f'] == 3 else 0.0)
    elif op == 'layernorm':
        n = _ln_ops(k['c'], aux['q'])
    elif op == 'softmax':
        n = 13.0 + np.asarray(k['c']) + np.abs(aux['d']) + aux['w']
        floor = FLT_MIN
    elif op == 'act':
        fn = k['fn']
        v = x.astype(np.float64).reshape(want.shape)
        floor = FLT_MIN
        if fn == 'softplus':
            return (10.0 * np.log1p(np.exp(-np.abs(v))) + np.abs(want)) * U * SECOND, floor
        if fn == 'gelu':
            t = v / math.sqrt(2.0)
            erf = np.abs(layer_ref._erf(t))
            ds = 32.0 * erf + 2.0 * np.abs(t) * 2.0 / math.sqrt(math.pi) * np.exp(-t * t) + np.abs(1.0 + layer_ref._erf(t))
            return (np.abs(0.5 * v) * ds + np.abs(want)) * U * SECOND, floor
        n = float(ACT_OPS[fn])
        if fn in ('swish', 'silu'):
            floor = np.where(-v > math.log(FLT_MAX), np.abs(v) / FLT_MAX, FLT_MIN)
    else:
        raise AssertionError('no bound for %r' % (op,))
    return n * U * mag * SECOND, floor


def run_case(gpu, case, stats):
    """Runs one case with each of its ``fuse`` values -> list of failure messages."""
    bad = []
    want, mag, aux = layer_ref.forward(case['cfg'], case['weights'], case['x'])
    want32 = want.astype(np.float32)
    tol = tolerance(case, case['x'], want, mag, aux)
    if tol is not None:
        rel, floor = (np.broadcast_to(t, want.shape) for t in tol)
        tol = rel + floor
    for fuse in case['fuses']:
        tag = '%s[fuse=%s]' % (case['name'], fuse)
        plan = keras_plan.build_plan(case['cfg'], case['weights'], fuse=fuse)
        if 'strided' in case['kind']:
            # the case must not silently test the plain path
            r, w = layer_cases.strided_views(plan, case['kind']['strided'], keras_plan)
            assert {o % 4 == 0 for o in r} == {True, False} and {o % 4 == 0 for o in w} == {True, False}, (tag, r, w)
        gpu.load_plan(plan)
        got = gpu.forward_patches(case['x'])
        again = gpu.forward_patches(case['x'])
        if got.shape != want.shape:
            bad.append('%s: shape %s, expected %s' % (tag, got.shape, want.shape))
            continue
        if got.tobytes() != again.tobytes():
            bad.append('%s: a second call gives other bytes' % tag)
        if not np.isfinite(got[np.isfinite(want32)]).all():
            bad.append('%s: not finite where the reference is' % tag)
        if tol is None:
            differ = got.view(np.uint32) != want32.view(np.uint32)
            signed_zero = differ & (got == 0) & (want32 == 0)      # the one named exclusion: a zero of the other sign
            stats['signed_zero'] = stats.get('signed_zero', 0) + int(signed_zero.sum())
            wrong = differ & ~signed_zero
            if wrong.any():
                i = np.unravel_index(np.argmax(wrong), wrong.shape)
                bad.append('%s: %d of %d differ, first at %s: %r, expected %r' % (tag, wrong.sum(), wrong.size, i, got[i], want32[i]))
            stats['worst'] = max(stats.get('worst', 0.0), float(wrong.any()))
        else:
            err = np.abs(got.astype(np.float64) - want)
            ratio = err / tol
            stats['worst'] = max(stats.get('worst', 0.0), float(ratio.max()))
            if case['kind']['op'] == 'act':
                # in ulp = 2^-23 of the magnitude (|want64| unless the formula cancels), over the elements whose bound is not its floor
                live = rel > floor
                ulps = float((err[live] / (2.0 * U * mag[live])).max())
                fn = case['kind']['fn']
                old = stats.setdefault('ulp', {}).get(fn, (0.0, 0.0))
                stats['ulp'][fn] = (max(old[0], ulps), max(old[1], float(ratio.max())))
            if not (err <= tol).all():
                i = np.unravel_index(np.argmax(ratio), ratio.shape)
                bad.append('%s: |got - want| = %.4g > bound %.4g at %s (got %r, want %r; %d of %d over)'
                           % (tag, err[i], tol[i], i, got[i], want[i], (err > tol).sum(), err.size))
    return bad


@pytest.mark.parametrize('group', layer_cases.GROUPS + ('random',))
def test_layer_kernels_against_float64(gpu, group):
    cases = layer_cases.group_cases(group)
    bad, stats = [], {}
    for case in cases:
        bad.extend(run_case(gpu, case, stats))
    print('\n%s: %d cases, worst |error| / bound = %.3f, zeros of the other sign let through: %d'
          % (group, len(cases), stats.get('worst', 0.0), stats.get('signed_zero', 0)))
    if 'ulp' in stats:
        # ceiling in ulp of the result where the formula does not cancel (n_ops / 2); '-' where the bound is a formula of its own
        print('  activation      worst observed, ulp   derived ceiling, ulp   worst |error| / bound')
        for fn, (v, r) in sorted(stats['ulp'].items()):
            print('  %-15s %-21.2f %-22s %.3f' % (fn, v, '0.5' if fn == 'leaky_relu' else ('%.1f' % (ACT_OPS[fn] / 2.0)) if fn in ACT_OPS else 'per element', r))
    assert not bad, '\n'.join(bad)


@pytest.mark.parametrize('act', ('linear', 'relu'))
@pytest.mark.parametrize('case', layer_cases.add_exact_cases(), ids=lambda c: c['name'])
def test_add_of_two_inputs_is_exact(gpu, case, act):
    """Add of two same-shape inputs = numpy.float32(a) + numpy.float32(b), then the op's own activation (linear | ReLU: v > 0 ? v : +0),
    bit for bit, on both branches of launch_binary: 16 bytes per lane (C = 8), one float per lane because C % 4 != 0 (C = 6), and one
    float per lane because an operand's pointer is not 16-byte aligned (C = 8 at channel offset 2 of a 12-channel buffer)."""
    a, b = layer_cases.add_exact_operands(case)
    with np.errstate(over='ignore'):
        want = a + b
    assert want.dtype == np.float32 and not np.isnan(want).any()
    assert np.isinf(want).any() and (want == 0).any() and np.signbit(want[want == 0]).any()      # the hand-picked pairs are in
    if act == 'relu':
        want = np.where(want > 0, want, np.float32(0.0))
    plan = keras_plan.build_plan(case['cfg'], case['weights'])
    adds = [o for o in plan.ops if o['op'] == keras_plan.OP_ADD]
    assert len(adds) == 1 and adds[0]['mode'] == 0 and adds[0]['act'] == 0
    views = [plan.tensors[adds[0][k]] for k in ('in0', 'in1', 'out')]
    assert all((t['h'], t['w'], t['c']) == want.shape[1:] for t in views)
    # the case takes the branch it is meant for: launch_binary's test on the views, and for the view case the pointer alone decides
    assert all(t['c'] % 4 == 0 and t['c_stride'] % 4 == 0 and t['c_offset'] % 4 == 0 for t in views) == case['kind']['vector']
    if case['kind']['view']:
        assert all(t['c'] % 4 == 0 and t['c_stride'] % 4 == 0 for t in views) and [t['c_offset'] % 4 for t in views] == [2, 0, 0]
    adds[0]['act'] = keras_plan.ACT[act]                      # the activation of the ADD op itself (ecseg_op_desc.act), inside binary_kernel
    gpu.load_plan(plan)
    got = gpu.forward_patches(case['x'])
    assert got.shape == want.shape and got.dtype == np.float32
    differ = got.view(np.uint32) != want.view(np.uint32)
    i = np.unravel_index(np.argmax(differ), differ.shape)
    assert not differ.any(), '%d of %d differ, first at %s: %r + %r = %r, expected %r' % (differ.sum(), differ.size, i, a[i], b[i], got[i], want[i])
