"""CPU checks of the float64 graph interpreter (tests/plan_ref.py) and of the cases (tests/plan_cases.py) that hold
``keras_plan.build_plan``'s rewrites on the device (tests/test_gpu_plan.py): the interpreter against the float32 oracle and against
spelled-out numpy, the plan's own record of each rewrite, and the mutant table - every slip the interpreter can model must move some
committed case past the bound the device is held to."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import plan_cases as pc                      # noqa: E402
import plan_ref                              # noqa: E402
from ecseg_amd import keras_plan as kp       # noqa: E402
from oracle import unet as oracle_unet       # noqa: E402

_REF = {}


def reference(case):
    if case['name'] not in _REF:
        _REF[case['name']] = plan_ref.forward(case['cfg'], case['weights'], case['x'], case['lambda_affine'])
    return _REF[case['name']]


def ratio_of(got, y, A):
    """max |got - y| / (2^-24 A); where A is 0 (zero padding) the result must be 0 too."""
    err = np.abs(np.asarray(got, np.float64) - y)
    with np.errstate(invalid='ignore', divide='ignore'):
        r = np.where(A > 0, err / (pc.U * A), np.where(err == 0, 0.0, np.inf))
    return float(r.max())


def oracle_outputs(case):
    names = [r[0] if not r[1] else '%s/call%d' % (r[0], r[1]) for r in case['cfg']['config']['output_layers']]
    lam = {k: (lambda t, s=s, o=o: t * s + o) for k, (s, o) in case['lambda_affine'].items()}
    out = {}
    for nm in pc.outputs_of(case):
        f = oracle_unet.forward(case['cfg'], case['weights'], case['x'], lambda_fns=lam, output=names.index(nm))
        out[nm] = np.transpose(f, (0, 2, 3, 1)) if case['channels_first'] else f
    return out


def build(case, fuse):
    return kp.build_plan(case['cfg'], case['weights'], fuse=fuse, lambda_overrides=case['lambda_affine'] or None, output=case['output'],
                         keep=case['keep'])


def test_case_list_is_what_the_files_say():
    cases = pc.hand_cases()
    assert {c['group'] for c in cases} == set(pc.GROUPS)
    for c in cases + pc.random_cases():
        n, h, w = pc.x_nhwc(c).shape[:3]
        assert n == 2 and h <= 40 and w <= 56, c['name']
        for ws in c['weights'].values():
            for a in (ws.values() if isinstance(ws, dict) else [ws]):
                assert all(np.asarray(t).shape[-1] <= 24 for t in a if np.asarray(t).ndim), c['name']
    assert len(pc.random_cases()) == pc.N_SEEDS == 40
    for c in pc.random_cases():
        assert 6 <= len(c['cfg']['config']['layers']) - 1 <= 21, c['name']
    assert pc.random_graph(7)['cfg'] == pc.random_cases()[7]['cfg']


def test_float32_oracle_within_bound(capsys):
    """The project's float32 reference against the interpreter on every case, seed and checked tensor: measures the constant of the
    bound (the print-out is where C_MEASURED comes from) and guards the interpreter itself."""
    worst, rows = 0.0, []
    for case in pc.hand_cases() + pc.random_cases():
        vals = reference(case)
        for nm, f in oracle_outputs(case).items():
            y, A = vals[nm]
            assert f.shape == y.shape, (case['name'], nm, f.shape, y.shape)
            r = ratio_of(f, y, A)
            rows.append('%-52s %-18s %.3f' % (case['name'], nm, r))
            worst = max(worst, r)
    with capsys.disabled():
        print('\nfloat32 oracle against the float64 interpreter: |f32 - y| / (2^-24 A)')
        print('\n'.join(rows))
        print('largest ratio %.3f (C_MEASURED %.3f, C_BOUND %g)' % (worst, pc.C_MEASURED, pc.C_BOUND))
    assert worst <= pc.C_BOUND / 4, 'the float32 oracle needs %.3f: C_BOUND must leave it a factor 4' % worst
    assert pc.C_BOUND == 2.0 ** np.ceil(np.log2(4 * pc.C_MEASURED))


def _case(name):
    return [c for c in pc.hand_cases() if c['name'] == name][0]


def test_interpreter_against_spelled_out_numpy():
    # Conv2D 3x3 'same' (one pixel of zeros on every side) + BatchNormalization, epsilon 1e-5
    c = _case('bn_fold_eps_1e-5_hard')
    x = c['x'].astype(np.float64)
    k, b = (a.astype(np.float64) for a in c['weights']['c'])
    g, beta, mean, var = (a.astype(np.float64) for a in c['weights']['bn'])
    xp = np.pad(x, ((0, 0), (1, 1), (1, 1), (0, 0)))
    conv = sum(np.einsum('nhwc,co->nhwo', xp[:, r:r + 18, q:q + 22], k[r, q]) for r in range(3) for q in range(3)) + b
    want = g * (conv - mean) / np.sqrt(var + 1e-5) + beta
    y, A = reference(c)['bn']
    assert np.abs(y - want).max() <= 2.0 ** -40 * A.max()
    wantA = np.abs(g) / np.sqrt(var + 1e-5) * (sum(np.einsum('nhwc,co->nhwo', np.abs(xp)[:, r:r + 18, q:q + 22], np.abs(k[r, q]))
                                                   for r in range(3) for q in range(3)) + np.abs(b) + np.abs(mean)) + np.abs(beta)
    assert np.allclose(A, wantA, rtol=1e-12) and (A >= np.abs(y)).all()
    # 1x1 convolution of one channel + LeakyReLU(0.01)
    c = _case('leaky_relu_small_negatives')
    pre = c['x'].astype(np.float64) * np.array([0.5, 1.0, 1.5, 2.0]) + np.float64(np.float32(-2e-3))
    y, _ = reference(c)['act']
    assert np.array_equal(y, np.where(pre > 0, pre, 0.01 * pre))
    assert (pre < 0).any() and pre.min() == np.float32(-2e-3)
    # UpSampling2D(2) + Conv2D 2x2 'same' (nothing in front, one row / column of zeros behind) + relu
    c = _case('upsample_2_conv_2x2')
    x = c['x'].astype(np.float64)
    k, b = (a.astype(np.float64) for a in c['weights']['c'])
    up = np.repeat(np.repeat(x, 2, axis=1), 2, axis=2)
    upp = np.pad(up, ((0, 0), (0, 1), (0, 1), (0, 0)))
    want = np.maximum(sum(np.einsum('nhwc,co->nhwo', upp[:, r:r + 18, q:q + 26], k[r, q]) for r in range(2) for q in range(2)) + b, 0)
    y, A = reference(c)['c']
    assert np.abs(y - want).max() <= 2.0 ** -40 * A.max()


def _emitting(case):
    n = 0
    for L in case['cfg']['config']['layers']:
        if L['class_name'] not in pc.NO_OP_CLASSES:
            n += 2 if L['class_name'] == 'SeparableConv2D' else 1
    return n + case['copies']


@pytest.mark.parametrize('group', pc.GROUPS)
def test_rewrites_fire_where_the_case_says(group):
    for case in pc.group_cases(group):
        tag = case['name']
        plan, plain = build(case, True), build(case, False)
        lt = plan.layer_tensor
        for layer, into in case['fused']:
            assert lt[layer] == lt[into], (tag, layer, 'not fused into', into)
            assert plain.layer_tensor[layer] != plain.layer_tensor[into], tag
        for layer, prod in case['unfused']:
            assert lt[layer] != lt[prod], (tag, layer, 'must keep a tensor of its own')
        for up, conv in case['folded_up']:
            note = up + ' (UpSampling2D folded into the convolution)'
            assert lt.get(note) == lt[conv], (tag, 'UpSampling2D not folded')
            op = [o for o in plan.ops if o['out'] == lt[conv]]
            assert len(op) == 1 and (op[0]['op'], op[0]['kh'], op[0]['kw'], op[0]['stride']) == (kp.OP_CONVT, 3, 3, 2), tag
            assert not [o for o in plan.ops if o['op'] == kp.OP_UPSAMPLE], tag
        if not case['folded_up'] and group == 'up':
            assert len([o for o in plan.ops if o['op'] == kp.OP_UPSAMPLE]) == 1, tag
        for p in (plan, plain):
            for layer, (off, stride) in case['views'].items():
                t = p.tensors[p.layer_tensor[layer]]
                assert (t['c_offset'], t['c_stride']) == (off, stride), (tag, layer, t)
            assert len([o for o in p.ops if o['op'] == kp.OP_COPY and o['pad_top'] == 0 and o['pad_left'] == 0 and
                        p.tensors[o['out']]['c_stride'] != p.tensors[o['out']]['c']]) >= case['copies'], tag
        if case['count_ops']:
            # one op per layer without fusion; each fused layer and each folded UpSampling2D is one op fewer
            assert len(plain.ops) == _emitting(case), (tag, len(plain.ops), _emitting(case))
            assert len(plan.ops) == _emitting(case) - len(case['fused']) - len(case['folded_up']), (tag, len(plan.ops))
        if case['fewer_buffers']:
            assert plan.n_buffers < len(plan.tensors) and plan.n_buffers < len(case['cfg']['config']['layers']) - 2, (tag, plan.n_buffers)
        for nm in pc.outputs_of(case):
            # the model's output and every kept tensor own a buffer: whatever else lives there is a channel view of that very tensor
            t = plan.tensors[lt[nm]]
            assert all(q['c_stride'] == t['c_stride'] and (q['h'], q['w']) == (t['h'], t['w']) and q['c_offset'] + q['c'] <= t['c_offset'] + t['c']
                       for q in plan.tensors if q['buffer'] == t['buffer']), (tag, nm)


# ---------------------------------------------------------------------------------------------------------------- mutants
MUTANTS = [('bn_eps=1e-3', dict(bn_eps=1e-3)), ('bn_eps=1e-5', dict(bn_eps=1e-5)), ('bn_fold_axis', dict(bn_fold_axis=True)),
           ('bn_after_activation', dict(bn_after_activation=True)), ('leaky_alpha=0.3', dict(leaky_alpha=0.3)),
           ('norm_floor removed', dict(norm_floor=False)), ('lambda_order', dict(lambda_order=True)),
           ('upsample_nearest_phase', dict(upsample_nearest_phase=True)), ('concat_order', dict(concat_order=True)),
           ('pool_before_activation', dict(pool_before_activation=True)), ('same_pad_low', dict(same_pad_low=True)),
           ('shared_layer_second_call_uses_first_input', dict(shared_second_call_first_input=True))]


def mutant_effect(case, switches):
    """-> (killed, largest change / kill threshold, below the old whole-network bound) of one mutant on one case."""
    vals = reference(case)
    with np.errstate(all='ignore'):
        mut = plan_ref.forward(case['cfg'], case['weights'], case['x'], case['lambda_affine'], **switches)
    worst, sneaky = 0.0, True
    for nm in pc.outputs_of(case):
        y, A = vals[nm]
        d = np.abs(mut[nm][0] - y)
        thr = pc.KILL * pc.C_BOUND * pc.U * A
        with np.errstate(invalid='ignore', divide='ignore'):
            r = np.where(thr > 0, d / thr, np.where(d == 0, 0.0, np.inf))
        r = np.where(np.isnan(r), np.inf, r)
        worst = max(worst, float(r.max()))
        sneaky = sneaky and bool(np.nanmax(d) < 1e-3 * max(1.0, float(np.abs(y).max()))) and bool(np.isfinite(d).all())
    return worst > 1.0, worst, sneaky


def test_every_mutant_is_killed_and_half_pass_the_old_bound(capsys):
    rows, unkilled, n_sneaky = [], [], 0
    for label, switches in MUTANTS:
        kills = []
        for case in pc.hand_cases():
            killed, ratio, sneaky = mutant_effect(case, switches)
            if killed:
                kills.append((case['name'], ratio, sneaky))
        under = [k[0] for k in kills if k[2]]
        n_sneaky += bool(under)
        rows.append('%-44s killed by %2d case(s), largest change %9.3g x threshold; below the old 1e-3 bound on: %s'
                    % (label, len(kills), max([k[1] for k in kills] or [0.0]), ', '.join(under) or '-'))
        rows.extend('    %-52s %9.3g' % (k[0], k[1]) for k in kills)
        if not kills:
            unkilled.append(label)
    with capsys.disabled():
        print('\nmutant table (threshold = %g * %g * 2^-24 * A per element)' % (pc.KILL, pc.C_BOUND))
        print('\n'.join(rows))
        print('%d of %d mutants stay below 1e-3 * max(1, |y|.max()) on a case that kills them' % (n_sneaky, len(MUTANTS)))
    assert not unkilled, 'no case kills: %s' % unkilled
    assert 2 * n_sneaky >= len(MUTANTS), 'only %d of %d mutants would have passed the old bound' % (n_sneaky, len(MUTANTS))


@pytest.mark.parametrize('name,n_pairs', [('alloc_ladder_of_12_with_skips_1_2_5_11', 21), ('alloc_diamond_long_arm_outlives_short', 5)])
def test_every_stale_buffer_pair_is_killed(name, n_pairs, capsys):
    case = _case(name)
    pairs = plan_ref.stale_pairs(case['cfg'], case['weights'], case['x'])
    assert len(pairs) == n_pairs, pairs
    alive, weakest = [], np.inf
    for p in pairs:
        killed, ratio, _ = mutant_effect(case, dict(stale_buffer=p))
        weakest = min(weakest, ratio)
        if not killed:
            alive.append((p, ratio))
    with capsys.disabled():
        print('\nstale_buffer on %s: %d (producer, victim) pairs, weakest kill %.3g x threshold' % (name, len(pairs), weakest))
    assert not alive, alive
