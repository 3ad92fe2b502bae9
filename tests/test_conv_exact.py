"""tests/conv_exact_ref.py and the cases of tests/conv_exact_cases.py, without a GPU: every case meets the precondition under which
tests/test_gpu_conv_exact.py may ask for bit equality (derived there), the reference equals oracle/unet.py's float64 evaluation with
``==`` (both are exact on these inputs), every case lowers to the path it names, and the committed seed range holds every path.
"""
import numpy as np
import pytest

from ecseg_amd import keras_plan
from oracle import unet as oracle_unet

from tests import conv_exact_cases as cases
from tests import conv_exact_ref as ref

LIMIT = 2.0 ** 24


def precondition(case, plan, recs):
    """-> list of violations.  Direct kernels: max S < 2^24 per weighted layer.  F(2x2) kernels (profile kinds 1, 3, 4): weights multiples
    of 4 and 81 Cin max|x| max|w| + max|b| < 2^24.  The bf16x3 GEMM (kind 6): that, and operands of at most 8 bits."""
    kinds = dict(cases.profile_kinds(plan, case['opts']))
    by_out = {}
    for i, o in enumerate(plan.ops):
        by_out.setdefault(o['out'], []).append(kinds.get(i))
    bad = []
    for r in recs:
        k = set(by_out.get(plan.layer_tensor.get(r['name'], -1), []))
        if not r['max_s'] < LIMIT:
            bad.append('%s: max S = %g' % (r['name'], r['max_s']))
        if k & {1, 3, 4}:
            bound = 81.0 * r['cin'] * r['max_x'] * r['max_w'] + r['max_b']
            if not (r['w_mult4'] and bound < LIMIT):
                bad.append('%s on F(2x2): multiples of 4: %s, 81 Cin max|x| max|w| + max|b| = %g' % (r['name'], r['w_mult4'], bound))
        if 6 in k and not (r['max_x'] <= 255 and r['max_w'] <= 255):
            bad.append('%s on the bf16x3 GEMM: max|x| = %g, max|w| = %g' % (r['name'], r['max_x'], r['max_w']))
    return bad


@pytest.mark.parametrize('group', cases.LATTICE_GROUPS + ('random',))
def test_lattice_cases_meet_the_precondition_and_equal_the_float64_oracle(group):
    cs = cases.lattice_cases(group)
    assert cs
    bad = []
    for c in cs:
        want, S, recs = ref.forward(c['cfg'], c['weights'], c['x'])
        assert want.dtype == np.int64 and recs, c['name']
        plan = keras_plan.build_plan(c['cfg'], c['weights'])
        bad.extend('%s: %s' % (c['name'], b) for b in precondition(c, plan, recs))
        assert (S >= np.abs(want)).all(), c['name']
        other = oracle_unet.forward(c['cfg'], c['weights'], c['x'], dtype=np.float64)
        if other.shape != want.shape or not np.array_equal(other, want.astype(np.float64)):
            bad.append('%s: the reference differs from the float64 oracle' % c['name'])
        labels = cases.plan_labels(plan, c['opts'])
        if c['path'] not in labels:
            bad.append('%s: lowers to %s, not to %s' % (c['name'], sorted(labels), c['path']))
        ks = [k for _, k in cases.profile_kinds(plan, c['opts'])]
        if c['kind'] is not None and c['kind'] not in ks:
            bad.append('%s: profile kinds %s, expected %d' % (c['name'], ks, c['kind']))
    assert not bad, '\n'.join(bad)


def test_the_seed_range_is_committed_and_holds_every_path():
    cs = cases.all_lattice_cases()
    names = [c['name'] for c in cs]
    assert len(set(names)) == len(names)
    seeded = [c for c in cs if c['group'] == 'random']
    assert len(cases.RANDOM_SEEDS) == 42 and len(seeded) == 42
    # every seed draws data of its own: no two cases share their input or their weights
    data = [(c['x'].shape, c['x'].dtype.str, c['x'].tobytes()) for c in cs]
    assert len(set(data)) == len(data)
    wdata = [tuple(a.tobytes() for ws in c['weights'].values() for a in ws) for c in cs]
    assert len(set(wdata)) == len(wdata)
    a, b = cases.random_case(7), cases.random_case(7)
    assert a['name'] == b['name'] and np.array_equal(a['x'], b['x'])
    seen = set()
    for c in seeded:
        seen |= cases.plan_labels(keras_plan.build_plan(c['cfg'], c['weights']), c['opts'])
    assert set(cases.PATHS) <= seen, sorted(set(cases.PATHS) - seen)
    fixed = set()
    for c in cs:
        if c['group'] != 'random':
            fixed.add(c['path'])
    assert set(cases.PATHS) <= fixed, sorted(set(cases.PATHS) - fixed)
    # both entry points, both activations, bias on and off, batches of 1 and 3
    assert {c['x'].dtype.str for c in cs} == {'|u1', '<f4'} and {c['x'].shape[0] for c in cs} == {1, 3}
    # the channel counts on both sides of every padding rule
    cin = {c['x'].shape[3] for c in cs}
    cout = {ref.forward(c['cfg'], c['weights'], c['x'][:1])[0].shape[-1] for c in cs if c['group'] in ('mfma', 'direct')}
    assert set(cases.CIN_LIST) <= cin and set(cases.COUT_LIST) <= cout, (sorted(cin), sorted(cout))


def test_the_view_cases_write_at_channel_offsets_4_and_6():
    for c in cases.fusion_cases():
        if c['path'] != 'concat_view':
            continue
        plan = keras_plan.build_plan(c['cfg'], c['weights'])
        offs = [plan.tensors[plan.layer_tensor[n]]['c_offset'] for n in 'abc']
        assert offs == [0, 4, 6] and all(plan.tensors[plan.layer_tensor[n]]['buffer'] == plan.tensors[plan.output_tensor]['buffer'] for n in 'abc'), c['name']


def _nonzero_terms(c):
    """Per output element: how many products of its sum are non-zero, plus one for a non-zero bias."""
    ind = lambda a: (np.asarray(a) != 0).astype(np.float32)
    return ref.forward(c['cfg'], {k: [ind(a) for a in ws] for k, ws in c['weights'].items()}, ind(c['x']))[0]


@pytest.mark.parametrize('fam', sorted(cases.IMPULSE_FAMILIES))
def test_impulse_cases_have_one_term_per_sum_and_equal_the_float64_oracle(fam):
    cs = cases.impulse_cases(fam)
    cls, k, s, dil, padding, cin, cout = cases.IMPULSE_FAMILIES[fam][:7]
    # the delta filters: every tap, and a channel of every 4-channel group (so of every 8-channel group) of Cin and of Cout
    taps = [c['tap'] for c in cs if 'tap' in c]
    assert {t[:2] for t in taps} == {(r, q) for r in range(k) for q in range(k)}
    for n, picked in ((cin, {t[2] for t in taps}), (cout, {t[3] for t in taps})):
        for lo, hi in cases.channel_groups(n):
            assert picked & set(range(lo, hi)), (fam, n, lo, sorted(picked))
        assert all(picked & set(range(g, min(g + 8, n))) for g in range(0, n, 8))
    # the delta input: every input channel, every corner, and both sides of every tile seam on both axes (there is one on each)
    x0 = cs[0]['x']
    H, W = x0.shape[1:3]
    where = np.argwhere(x0 == 1.0)
    assert len(where) == x0.shape[0] == int(x0.sum()) and set(where[:, 3]) == set(range(cin))
    pos = {(int(y), int(x)) for _, y, x, _ in where}
    assert {(0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1)} <= pos
    rows, cols = cases.impulse_seams(fam)
    assert len(rows) >= 2 and len(cols) >= 2 and {(y, x) for y in rows for x in cols} <= pos, (fam, rows, cols)
    for c in cs:
        assert _nonzero_terms(c).max() <= 1, c['name']
        want, _, _ = ref.forward(c['cfg'], c['weights'], c['x'])
        assert want.dtype == np.float64 and np.isfinite(want).all()
        assert np.array_equal(want.astype(np.float32).astype(np.float64), want), c['name']          # float32 holds it: nothing rounds
        other = oracle_unet.forward(c['cfg'], c['weights'], c['x'], dtype=np.float64)
        assert np.array_equal(other, want), c['name']
        plan = keras_plan.build_plan(c['cfg'], c['weights'])
        assert c['path'] in cases.plan_labels(plan, c['opts']), (c['name'], cases.plan_labels(plan, c['opts']))
        if 'tap' in c:                                          # the chosen output channel moves the data, the others hold their bias
            oc = c['tap'][4]
            others = np.delete(want, oc, axis=-1)
            assert np.array_equal(others, np.broadcast_to(np.delete(c['weights']['op'][1].astype(np.float64), oc), others.shape))
            assert np.abs(want[..., oc]).max() > 0
        else:
            w = c['weights']['op'][0]
            assert np.isin(np.abs(want[want != 0]), np.abs(w.astype(np.float64))).all() and (want != 0).any()
            mant = np.frexp(w.astype(np.float64))[0] * 2.0 ** 24
            assert (mant % 2 == 1).all() and 1e-20 < np.abs(w).min() and np.abs(w).max() < 1e20


def test_identity_cases_lower_to_the_f4x4_kernels():
    for c in cases.identity_cases():
        for opts in cases.IDENTITY_OPTS:
            o = dict(cases.OPTION_DEFAULTS, **opts)
            for cc in [c] + ([cases.identity_case(*[s for s in cases.IDENTITY_SHAPES if s[0] == c['name']][0], pad_to=cases.IDENTITY_PADS[c['x'].shape[3]])]
                             if c['x'].shape[3] in cases.IDENTITY_PADS else []):
                plan = keras_plan.build_plan(cc['cfg'], cc['weights'])
                ks = [k for _, k in cases.profile_kinds(plan, o)]
                cout = cc['weights']['op'][0].shape[3]
                assert ks == [5 if (o['winograd'] == 3 and cout % 64 == 0) else 2], (cc['name'], ks)
    shapes = cases.IDENTITY_SHAPES
    assert any(s[1] % 8 == 4 for s in shapes) and any(s[2] % 64 == 32 for s in shapes)
    assert any((s[3][0] // 16) * (s[3][1] // 16) % 2 == 1 and s[4] > 1 for s in shapes)       # odd regions per patch: a pair spans two patches
