"""The output stages of the convolution kernels - activation, fused 2 x 2 max-pool, fused 1 x 1 head - against float64, with a bound at every
output.  Cases: tests/conv_tail_cases.py; activations, their bounds and the head's: tests/wino4_ref.py; tests/test_conv_tails.py ties the
truths to oracle/unet.py and asserts every precondition without a GPU.

u = 2^-24 is the relative error of one correctly rounded float32 operation; a library function with a ceiling of k ulp contributes 2 k u.
OCML's ceilings are OpenCL's single-precision table (exp 3, expm1 3, tanh 5 ulp; division and the basic operations correctly rounded), as in
tests/test_gpu_layers.py, whose table these rows continue.  SECOND = 1 + 2^-10 stands for the products of errors; FLT_MIN is the floor of
every bound whose result may be denormal.  The own error of an activation at a float32 argument v (``wino4_ref.act_own``):

  relu, ReLU(max_value), linear     select class: the result is v, 0 or the clip value - equal to float32(act64(v)); only a zero of the other
                                    sign is let through
  LeakyReLU                         v > 0 ? v : alpha * v - one rounding: u |want| + 2^-149
  sigmoid   1 / (1 + expf(-v))      expf 6 + addition 1 + division 1 = 8 u |want|
  tanh      tanhf                   10 u |want|
  swish     v / (1 + expf(-v))      8 u |want| (an op of its own, apply_act_ext); floor |v| / FLT_MAX where expf(-v) overflows
  elu       dwconv_kernel           alpha * expm1f(v): 6 + 1 = 7 u |want|
  elu       the convolution         alpha * (expf(v) - 1.f) for v <= 0.  expf(v) = e^v (1 + d), |d| <= 6 u: an ABSOLUTE error of 6 u e^v, which the
            kernels                 subtraction does not shrink - the difference is rounded once more, u |e^v - 1|, and so is the product with alpha,
                                    u alpha |e^v - 1| (apply_act_core has alpha = 1 and no product: one rounding less).  Together
                                    alpha u (6 e^v + 2 |e^v - 1|): at v = -1e-6 that is 6 u against a result of 1e-6 - no relative bound holds,
                                    which is why this row is not tests/test_gpu_layers.py's.  v > 0: the result is v.

A   the argument is known bit for bit (delta filter; dyadic data on the kernels with an input transform): |got - act64(v)| <= act_own(v), on
    every exact path, for every activation the convolution kernels implement and for one (swish) that the plan must split off; the launch
    profile shows the kernel the case names, and for ELU(alpha != 1) and ReLU(max_value) that it is NOT an F(4x4) kernel or
    conv_wino16_kernel (apply_act_core has neither alpha nor clip).  conv_wino16_kernel<FIRST> carries two activations and two alphas: with
    LeakyReLU both layers are exact; with tanh in front the second layer's F(2x2) transforms round tanh values:
    6 u Q2 (two roundings in B^T d B, four in A^T M A; U = G e G^T is exact; Q2 = conv_tail_cases.f2_scale) + 10 u |tanh| carried through.
B   the F(4x4) kernels with v = the float64 sum y, known to pre = hard_count u Q + u |y| (tests/test_gpu_wino4_accuracy.py):
    |got - act64(y)| <= L pre SECOND + act_own(y), L = the largest |act'| (1/4 sigmoid, 1 tanh / elu, max(1, slope) LeakyReLU); SECOND on the
    L pre term also covers act_own at the device's argument instead of y (conv_tail_cases.TailRef).  Every case runs a second time with
    data and bias times 2^-20: every term of the bound scales with them, so near 0 it is ~1e-10 and holds the activations' arithmetic there
    to a few u of their result - where a tanh or elu that cancels is wrong by a rounding of 1, ~3e-8.
C   pool: the largest such bound of the window.  Head: per class sum_o |h_ok| (feature bound)_o + HEAD_OWN u (sum_o |h_ok| |f_o| + |hb_k|), times
    the head activation's L, plus its act_own at the logit; softmax: wino4_ref.head_scale.  HEAD_OWN = 12 covers the roundings behind a
    product on every head: fused F(4x4) 12 (wino4_ref), fused conv_wino16_kernel C / 4 fmas + 2 adds across lanes + bias = 7 / 11,
    conv_head_kernel C / LPP = 4 fmas + log2(LPP) <= 4 adds + bias <= 9.  On conv_wino16_kernel the 3 x 3 sum is exact (dyadic lattice).
    Every head case runs fused (0x200) and with fuse_head = 0 (conv_head_kernel) against the same bound.

No bound is read off the device; each test prints worst error / bound (-s).  Every case must give identical bytes on a second call.
"""
import numpy as np
import pytest

from tests import conv_exact_cases as cx
from tests import conv_exact_ref as cref
from tests import conv_tail_cases as tc
from tests import wino4_cases as wc
from tests import wino4_ref as ref

pytestmark = pytest.mark.gpu


class _Options:
    def __init__(self, gpu, opts, **more):
        self.gpu, self.opts, self.more = gpu, opts, more

    def __enter__(self):
        for k, v in dict(self.opts, **self.more).items():
            self.gpu.set_option(k, v)
        return self.opts

    def __exit__(self, *exc):
        self.gpu.set_kernel_profiling(False)
        for k, v in dict(cx.LIBRARY_DEFAULTS, fuse_head=1).items():
            self.gpu.set_option(k, v)


def _run(gpu, plan, x):
    """-> (result, [(op, kind)] of the launch profile, whether a second call gives the same bytes)."""
    gpu.load_plan(plan)
    gpu.set_kernel_profiling(True)
    got = gpu.forward_patches(x)
    recs = [(r['op'], r['kind']) for r in gpu.conv_launch_profile()]
    gpu.set_kernel_profiling(False)
    again = gpu.forward_patches(x)
    return got, recs, got.tobytes() == again.tobytes()


def _bits(recs):
    b = 0
    for _, k in recs:
        b |= k & 0x700
    return b


def _hold(tag, got, want, bound, exact, bad):
    """|got - want| <= bound at every element (``exact``: float32(want) bit for bit, a zero of the other sign let through) -> worst ratio."""
    if got.shape != want.shape:
        bad.append('%s: shape %s, expected %s' % (tag, got.shape, want.shape))
        return 0.0
    if exact:
        want32 = want.astype(np.float32)
        wrong = (got.view(np.uint32) != want32.view(np.uint32)) & ~((got == 0) & (want32 == 0))
        if wrong.any():
            i = np.unravel_index(np.argmax(wrong), wrong.shape)
            bad.append('%s: %d of %d differ, first at %s: %r, expected %r' % (tag, wrong.sum(), wrong.size, i, got[i], want32[i]))
        return float(wrong.any())
    err = np.abs(got.astype(np.float64) - want)
    with np.errstate(divide='ignore', invalid='ignore'):
        ratio = np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), np.where(err > 0, np.inf, 0.0))
    if not (err <= bound).all() or not np.isfinite(got).all():
        i = np.unravel_index(np.argmax(ratio), ratio.shape)
        bad.append('%s: |got - want| = %.4g > bound %.4g at %s (got %r, want %r; %d of %d over)' % (tag, err[i], bound[i], i, got[i], want[i], (err > bound).sum(), err.size))
    return float(ratio.max())


def _exact_run(gpu, c, bad, opts=None, must_kind=True):
    """One part-A case: profile, bytes, bound.  -> (worst ratio, kinds)."""
    pre = tc.pre_activation(c)
    want = ref.act64(pre, tc.spec(c['act']))
    bound, exact = ref.act_own(pre, tc.spec(c['act']), expm1=c['expm1'])
    plan = tc.plan_of(c)
    opts = opts or c['opts']
    with _Options(gpu, opts):
        got, recs, same = _run(gpu, plan, c['x'])
    tag = '%s [winograd%d]' % (c['name'], opts['winograd'])
    kinds = [(o, k & 0xff) for o, k in recs]
    if kinds != tc.expected_kinds(plan, opts):
        bad.append('%s: launch profile %s, expected kinds %s' % (tag, recs, tc.expected_kinds(plan, opts)))
    if must_kind and c['kind'] is not None and c['act'] in tc.KEEPS_KERNEL and c['kind'] not in [k for _, k in kinds]:
        bad.append('%s: launch profile %s without kind %d' % (tag, recs, c['kind']))
    if _bits(recs):
        bad.append('%s: fusion bits 0x%x' % (tag, _bits(recs)))
    if not same:
        bad.append('%s: a second call gives other bytes' % tag)
    return _hold(tag, got, want, bound, exact, bad), [k for _, k in kinds]


@pytest.mark.parametrize('fam', sorted(tc.FAMILIES))
def test_activation_behind_an_exactly_known_sum(gpu, fam):
    bad, line = [], []
    for act in tc.A_ACTS:
        worst, _ = _exact_run(gpu, tc.exact_case(fam, act), bad)
        line.append('%s %.3f' % (act, worst))
    print('\n%s: worst |error| / bound: %s' % (fam, ', '.join(line)))
    assert not bad, '\n'.join(bad)


@pytest.mark.parametrize('shape', sorted(tc.ROUTING_SHAPES))
def test_activations_apply_act_core_lacks_leave_the_winograd_output_stages(gpu, shape):
    bad = []
    for act in tc.ROUTING_AWAY + tc.ROUTING_STAY:
        c = tc.routing_case(shape, act)
        for opts in tc.ROUTING_OPTS:
            plan = tc.plan_of(c)
            if set(k for _, k in tc.expected_kinds(plan, opts)) & {2, 5}:
                # an F(4x4) kernel: nothing is exact there (part B holds its values, at full scale and at 2^-20) - the routing, finite
                # values and the same bytes twice
                with _Options(gpu, opts):
                    got, recs, same = _run(gpu, plan, c['x'])
                kinds = [k & 0xff for _, k in recs]
                if not same or not np.isfinite(got).all():
                    bad.append('%s [winograd%d]: %s' % (c['name'], opts['winograd'], 'not finite' if same else 'a second call gives other bytes'))
            else:
                _, kinds = _exact_run(gpu, c, bad, opts, must_kind=False)
            away = not set(kinds) & {2, 4, 5}
            if act in tc.ROUTING_AWAY and not away:
                bad.append('%s [winograd%d]: kinds %s - apply_act_core has no alpha and no clip' % (c['name'], opts['winograd'], kinds))
            if act in tc.ROUTING_STAY and not (kinds and set(kinds) <= {2, 4, 5}):
                bad.append('%s [winograd%d]: kinds %s, expected an F(4x4) kernel or conv_wino16_kernel' % (c['name'], opts['winograd'], kinds))
    assert not bad, '\n'.join(bad)


@pytest.mark.parametrize('c16', [16, 32])
def test_wino16_first_keeps_its_two_activations_apart(gpu, c16):
    bad, line = [], []
    for a1, a2 in tc.FIRST_PAIRS:
        c = tc.first_case(c16, a1, a2)
        plan = tc.plan_of(c)
        with _Options(gpu, c['opts']):
            got, recs, same = _run(gpu, plan, c['x'])
        if [k & 0xff for _, k in recs] != [4] or _bits(recs) != 0x400:
            bad.append('%s: launch profile %s, expected kind 4 with 0x400' % (c['name'], recs))
        if not same:
            bad.append('%s: a second call gives other bytes' % c['name'])
        mid, f1, lin, pre2, want = tc.first_parts(c)
        n, H, W, ch = f1.shape
        own2, exact2 = ref.act_own(pre2, tc.spec(a2))
        own1 = ref.act_own(mid, tc.spec(a1))[0]
        # what the first activation's own error and (tanh: the second layer's transforms of inexact data) leave on the second pre-activation
        carried = np.zeros_like(pre2)
        if a1 == 'tanh':
            z = np.zeros((n, H, W, ch))
            z[..., c['ca']] = own1[..., c['ca']]
            carried = cref.forward(lin, {'op': [c['weights']['op'][0], np.zeros(ch, np.float32)]}, z)[0].astype(np.float64)
            carried[..., c['oc']] += 6 * ref.U32 * tc.f2_scale(np.abs(f1[..., c['ca']]), c['tap2'])
        bound = (ref.act_lip(tc.spec(a2)) * carried + own2) * ref.SECOND
        exact = exact2 and a1 != 'tanh'
        if not exact:
            bound = bound + ref.FLT_MIN
        line.append('%s/%s %.3f' % (a1, a2, _hold(c['name'], got, want, bound, exact, bad)))
    print('\nfirst_c%d: worst |error| / bound: %s' % (c16, ', '.join(line)))
    assert not bad, '\n'.join(bad)


@pytest.mark.parametrize('shape', tc.B_SHAPES)
def test_f4x4_activations_against_float64(gpu, shape):
    bad = []
    for act, ls in [(a, s) for s in tc.B_SCALES for a in tc.B_ACTS]:
        case = tc.f4_case(shape, act, ls)
        R, plan = tc.TailRef(case), tc.plan_of(case)
        for opts in wc.options(shape):
            mode, kind = wc.mode_of(shape, opts), wc.kind_of(shape, opts)
            tag = '%s [%s]' % (case['name'], wc.opts_id(opts))
            with _Options(gpu, opts):
                got, recs, same = _run(gpu, plan, case['x'])
            if [(o, k & 0xff) for o, k in recs] != tc.expected_kinds(plan, opts) or [k & 0xff for _, k in recs] != [kind] or _bits(recs):
                bad.append('%s: launch profile %s, expected kind %d' % (tag, recs, kind))
            if not same:
                bad.append('%s: a second call gives other bytes' % tag)
            worst = _hold(tag, got, R.truth, R.bound(mode), False, bad)
            print('\n%s kind %d %s: worst |error| / bound %.3f' % (tag, kind, mode, worst))
    assert not bad, '\n'.join(bad)


@pytest.mark.parametrize('kernel', tc.KERNELS)
def test_fused_pool_of_negative_values(gpu, kernel):
    opts, kind, mode = tc.kernel_setup(kernel)
    bad = []
    for act in tc.POOL_ACTS:
        case = tc.pool_case(kernel, act)
        R, plan = tc.TailRef(case), tc.plan_of(case)
        assert (R.truth < 0).mean() >= 0.25
        with _Options(gpu, opts):
            got, recs, same = _run(gpu, plan, case['x'])
        if [k & 0xff for _, k in recs] != [kind] or _bits(recs) != 0x100:
            bad.append('%s: launch profile %s, expected kind %d with 0x100' % (case['name'], recs, kind))
        if not same:
            bad.append('%s: a second call gives other bytes' % case['name'])
        exact = mode is None and ref.act_own(R.y, tc.spec(act))[1]
        worst = _hold(case['name'], got, R.truth, R.bound(mode), exact, bad)
        print('\n%s: worst |error| / bound %.3f' % (case['name'], worst))
    assert not bad, '\n'.join(bad)


def _head_run(gpu, case, opts, kind, mode, fuse_head, expect_bits, bad):
    R, plan = tc.TailRef(case), tc.plan_of(case)
    tag = '%s [fuse_head=%d]' % (case['name'], fuse_head)
    with _Options(gpu, opts, fuse_head=fuse_head):
        got, recs, same = _run(gpu, plan, case['x'])
    if [k & 0xff for _, k in recs if (k & 0xff) in (2, 4, 5)] != [kind] or _bits(recs) != expect_bits:
        bad.append('%s: launch profile %s, expected kind %d with bits 0x%x' % (tag, recs, kind, expect_bits))
    if not same:
        bad.append('%s: a second call gives other bytes' % tag)
    k = case['head'][0].shape[1]
    if case['head_act'] == 'softmax' and k == 1 and not (got == 1.0).all():
        bad.append('%s: a softmax over one class is not exactly 1' % tag)
    return _hold(tag, got, R.truth, R.bound(mode), False, bad)


@pytest.mark.parametrize('kernel', tc.KERNELS)
def test_fused_head_and_conv_head_kernel_behind_a_real_sum(gpu, kernel):
    opts, kind, mode = tc.kernel_setup(kernel)
    bad = []
    for k, ha, hb, act in tc.HEAD_COMBOS:
        case = tc.head_case(kernel, k, ha, hb, act)
        a = _head_run(gpu, case, opts, kind, mode, 1, 0x200, bad)
        b = _head_run(gpu, case, opts, kind, mode, 0, 0, bad)
        print('\n%s: worst |error| / bound %.4f fused, %.4f on conv_head_kernel' % (case['name'], a, b))
    assert not bad, '\n'.join(bad)


@pytest.mark.parametrize('kernel', tc.KERNELS)
def test_heads_the_fused_stage_cannot_compute_do_not_fuse(gpu, kernel):
    opts, kind, mode = tc.kernel_setup(kernel)
    bad = []
    for k, ha, act in tc.UNFUSED_COMBOS:
        case = tc.head_case(kernel, k, ha, True, act, fused=False)
        worst = _head_run(gpu, case, opts, kind, mode, 1, 0, bad)
        print('\n%s: not fused, worst |error| / bound %.4f' % (case['name'], worst))
    assert not bad, '\n'.join(bad)
