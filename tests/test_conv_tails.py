"""tests/conv_tail_cases.py without a GPU: every case's truth is oracle/unet.py's float64 evaluation, the exactness preconditions of part A
hold (the argument of the activation is a float32 known bit for bit, every point of the sweep reaches the tapped channel, every case lowers
to the path it names), the pooled truths of part C are negative often enough to see a pool accumulator that starts at 0, and the float32
replay of every B / C case stays inside the bound tests/test_gpu_conv_tails.py holds the device to.  Prints the replay's margins (-s)."""
import numpy as np
import pytest

from ecseg_amd import keras_plan
from oracle import unet as oracle_unet
from tests import conv_exact_cases as cx
from tests import conv_exact_ref as cref
from tests import conv_tail_cases as tc
from tests import wino4_cases as wc
from tests import wino4_ref as ref


def _oracle(case):
    return np.asarray(oracle_unet.forward(case['cfg'], case['weights'], case['x'], dtype=np.float64), np.float64)


def _close(a, b, tol=1e-12, unit=1.0):
    """|a - b| <= tol (unit + |b|); ``unit``: the size of the data (2^-20 for the small-argument cases)."""
    return a.shape == b.shape and bool((np.abs(a - b) <= tol * (unit + np.abs(b))).all())


def test_act64_is_layer_refs_activation():
    from tests import layer_ref
    v = tc.sweep_values(False).astype(np.float64)
    for act in tc.ACTS:
        name, alpha = ref._spec(tc.spec(act))
        if name == 'softmax':
            continue
        assert np.array_equal(ref.act64(v, tc.spec(act)), layer_ref.activation(name, v, alpha)[0]), act


@pytest.mark.parametrize('fam', sorted(tc.FAMILIES))
def test_exact_cases_know_the_argument_of_the_activation_bit_for_bit(fam):
    for act in tc.A_ACTS:
        c = tc.exact_case(fam, act)
        pre = tc.pre_activation(c)
        assert np.array_equal(pre.astype(np.float32).astype(np.float64), pre), c['name']
        ind = lambda a: (np.asarray(a) != 0).astype(np.float32)
        terms = cref.forward(c['lin_cfg'], {'op': [ind(c['weights']['op'][0]), ind(c['weights']['op'][1])]}, ind(c['x']))[0]
        assert terms.max() <= 1, c['name']                                   # one product or one bias per sum
        if c['f2']:
            assert tc.f2_exact(c['x']) <= tc.GRID_BITS
        assert set(tc.sweep_values(c['f2']).tolist()) <= set(pre[..., c['oc']].astype(np.float32).ravel().tolist()), c['name']
        want = ref.act64(pre, tc.spec(act))
        assert _close(_oracle(c), want), c['name']
        plan = tc.plan_of(c)
        kinds = tc.expected_kinds(plan, c['opts'])
        if act in tc.KEEPS_KERNEL:
            assert kinds == cx.profile_kinds(plan, c['opts']) and c['path'] in cx.plan_labels(plan, c['opts']), c['name']
            assert c['kind'] is None or c['kind'] in [k for _, k in kinds], c['name']
        else:
            assert not {k for _, k in kinds} & {2, 4, 5}, c['name']
        convs = [o for o in plan.ops if o['op'] in (keras_plan.OP_CONV, keras_plan.OP_CONVT, keras_plan.OP_DWCONV)]
        assert len(convs) == 1
        if act == 'swish' and c['path'] != 'dw':                              # the late activation is an op of its own behind a linear convolution
            assert convs[0]['act'] == 0 and [o['op'] for o in plan.ops].count(keras_plan.OP_ACT) == 1, c['name']
        else:
            assert keras_plan.OP_ACT not in [o['op'] for o in plan.ops], c['name']
            assert convs[0]['act'] != 0


def test_a_case_does_not_depend_on_what_was_built_before_it():
    before = tc.exact_case('wino', 'tanh')
    fams = dict(tc.FAMILIES)
    for shape in tc.ROUTING_SHAPES:
        tc.routing_case(shape, 'elu')
    after = tc.exact_case('wino', 'tanh')
    assert tc.FAMILIES == fams and tc.FAMILY_ORDER == tuple(sorted(fams)) and before['oc'] == after['oc']
    assert all(np.array_equal(a, b) for a, b in zip(before['weights']['op'], after['weights']['op']))


def test_routing_cases():
    for shape in tc.ROUTING_SHAPES:
        for act in tc.ROUTING_AWAY + tc.ROUTING_STAY:
            c = tc.routing_case(shape, act)
            pre = tc.pre_activation(c)
            assert np.array_equal(pre.astype(np.float32).astype(np.float64), pre) and tc.f2_exact(c['x']) <= tc.GRID_BITS
            assert _close(_oracle(c), ref.act64(pre, tc.spec(act))), c['name']
            plan = tc.plan_of(c)
            for opts in tc.ROUTING_OPTS:
                ks = {k for _, k in tc.expected_kinds(plan, opts)}
                assert {k for _, k in cx.profile_kinds(plan, opts)} <= {2, 4, 5}, c['name']        # the shape is one these kernels take
                assert (not ks & {2, 4, 5}) if act in tc.ROUTING_AWAY else ks <= {2, 4, 5}, (c['name'], ks)


def test_first_cases():
    for c16 in (16, 32):
        for a1, a2 in tc.FIRST_PAIRS:
            c = tc.first_case(c16, a1, a2)
            assert tc.f2_exact(c['x']) <= tc.GRID_BITS
            mid = cref.forward(c['mid_cfg'], {'c1': c['weights']['c1']}, c['x'])[0].astype(np.float64)
            assert np.array_equal(mid.astype(np.float32).astype(np.float64), mid)
            f1 = ref.act64(mid, tc.spec(a1))
            if a1 != 'tanh':                                                  # the second layer's input is dyadic: its sum is exact too
                assert tc.f2_exact(f1[..., c['ca']]) <= 12
            plan = tc.plan_of(c)
            assert [k for _, k in tc.expected_kinds(plan, c['opts'])] == [4], c['name']
            assert 'first_fused' in cx.plan_labels(plan, c['opts']), c['name']
            want = tc.first_truth(c)
            assert _close(_oracle(c), want), c['name']


def _tie(case, R):
    assert _close(_oracle(case), R.truth, 1e-11, 2.0 ** case.get('log2_scale', 0)), case['name']


@pytest.mark.parametrize('shape', tc.B_SHAPES)
def test_f4x4_activation_cases(shape):
    for act, ls in [(a, s) for s in tc.B_SCALES for a in tc.B_ACTS]:
        case = tc.f4_case(shape, act, ls)
        R = tc.TailRef(case)
        _tie(case, R)
        assert np.abs(R.y).max() < 2.0 ** (ls + 4) and (ls == 0 or np.median(np.abs(R.y)) > 2.0 ** (ls - 3))
        plan = tc.plan_of(case)
        d = wc.layer_under_test(plan)
        for opts in wc.options(shape):
            assert dict(tc.expected_kinds(plan, opts))[d['op']] == wc.kind_of(shape, opts), (case['name'], opts)
        for mode in sorted({wc.mode_of(shape, o) for o in wc.options(shape)}):
            over, worst = R.worst(R.replay(mode), mode)
            print('\n%s %s: replay at %.3g of its bound' % (case['name'], mode, worst))
            assert over == 0, (case['name'], mode, over, worst)


@pytest.mark.parametrize('kernel', tc.KERNELS)
def test_pool_cases(kernel):
    opts, kind, mode = tc.kernel_setup(kernel)
    for act in tc.POOL_ACTS:
        case = tc.pool_case(kernel, act)
        R = tc.TailRef(case)
        _tie(case, R)
        assert (R.truth < 0).mean() >= 0.25, (case['name'], (R.truth < 0).mean())
        plan = tc.plan_of(case)
        assert [k for _, k in tc.expected_kinds(plan, opts)] == [kind], case['name']
        over, worst = R.worst(R.replay(mode), mode)
        print('\n%s: %.0f %% of the pooled truths negative, replay at %.3g of its bound' % (case['name'], 100 * (R.truth < 0).mean(), worst))
        assert over == 0, (case['name'], over, worst)


@pytest.mark.parametrize('kernel', tc.KERNELS)
def test_head_cases(kernel):
    opts, kind, mode = tc.kernel_setup(kernel)
    combos = [(k, ha, hb, act, True) for k, ha, hb, act in tc.HEAD_COMBOS] + [(k, ha, True, act, False) for k, ha, act in tc.UNFUSED_COMBOS]
    for k in (1, 2, 3, 4):
        assert any(c[0] == k and c[1] == 'softmax' for c in combos)
    assert any(c[0] == 1 and c[1] == 'sigmoid' for c in combos) and {c[1] for c in tc.HEAD_COMBOS} == {'softmax', 'sigmoid', 'tanh', 'relu', 'linear'}
    assert {c[3] for c in tc.HEAD_COMBOS} == {'relu', 'tanh', 'leaky0.25'} and {c[2] for c in tc.HEAD_COMBOS} == {True, False}
    for k, ha, hb, act, fused in combos:
        case = tc.head_case(kernel, k, ha, hb, act, fused)
        R = tc.TailRef(case)
        _tie(case, R)
        if ha == 'softmax' and k == 1:
            assert (R.truth == 1.0).all()
        plan = tc.plan_of(case)
        assert [kk for _, kk in tc.expected_kinds(plan, opts)] == [kind], case['name']
        heads = [d for d in cx.conv_paths(plan) if d['path'] == 'head']
        assert len(heads) == 1 and heads[0]['cout'] == k, case['name']
        over, worst = R.worst(R.replay(mode), mode)
        print('\n%s: replay at %.3g of its bound' % (case['name'], worst))
        assert over == 0, (case['name'], over, worst)
