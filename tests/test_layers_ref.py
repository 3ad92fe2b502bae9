"""tests/layer_ref.py (numpy, float64) against oracle/unet.py's ``forward(..., dtype=np.float64)`` (torch) on every case of
tests/layer_cases.py: two independent float64 evaluations must agree to float64 rounding, which guards the reference that
tests/test_gpu_layers.py holds the device to.  No GPU needed.

Tolerance: ``TIE_OPS * 2^-53 * mag`` per element, ``mag`` being layer_ref's magnitude term (|y| where the op does not cancel).
TIE_OPS = 64 covers the few-ulp differences between numpy's and torch's exp / tanh / erf / log1p and the different but
equivalent operation orders (x * inv + shift against (x - mean) / std, sum / count against mean).  Two ops need more and say why:
* bilinear upsampling by 3: torch multiplies by the float64 1 / 3 where layer_ref divides by 3, so the two source
  coordinates differ by 2^-53 * extent and the lerp moves by that times |tr - tl| <= 2 mag: + 4 * (h + w) ops;
* LayerNormalization: the rounding of the mean (C additions) enters through the variance with the weight aux['q'] of the
  device bound's last term (tests/test_gpu_layers.py) - here C * q ops, which is 0.1 ulp unless the variance is 0.
"""
import numpy as np
import pytest

from ecseg_amd import keras_plan
from oracle import unet as oracle_unet

from tests import layer_cases, layer_ref

TIE_OPS = 64.0
EPS64 = 2.0 ** -53


def _tie_ops(case, aux):
    k = case['kind']
    if k['op'] == 'bilinear' and k['f'] == 3:
        return TIE_OPS + 4.0 * (k['h'] + k['w'])
    if k['op'] == 'layernorm':
        return TIE_OPS + k['c'] * (1.0 + EPS64 * k['c'] * aux['q'])
    return TIE_OPS


@pytest.mark.parametrize('group', layer_cases.GROUPS + ('random',))
def test_layer_ref_equals_the_float64_oracle(group):
    cases = layer_cases.group_cases(group)
    assert cases
    bad = []
    for case in cases:
        want, mag, aux = layer_ref.forward(case['cfg'], case['weights'], case['x'])
        other = oracle_unet.forward(case['cfg'], case['weights'], case['x'], dtype=np.float64)
        assert other.dtype == np.float64 and other.shape == want.shape, case['name']
        assert np.isfinite(want).all() and (mag >= np.abs(want) * (1 - 1e-12)).all(), case['name']
        err = np.abs(want - other)
        tol = _tie_ops(case, aux) * EPS64 * mag
        if not (err <= tol).all():
            i = np.unravel_index(np.argmax(err - tol), err.shape)
            bad.append('%s: |ref - oracle| = %.3g > %.3g at %s' % (case['name'], err[i], tol[i], i))
    assert not bad, '\n'.join(bad)


def test_case_names_are_unique_and_the_seeded_range_is_committed():
    cases = layer_cases.all_cases()
    names = [c['name'] for c in cases]
    assert len(set(names)) == len(names)
    assert len(layer_cases.RANDOM_SEEDS) == 40 and sum(c['group'] == 'random' for c in cases) == 40
    # every seed gives data of its own: no two seeded cases, and no seeded and hand-made case, share their input
    data = [(c['x'].shape, c['x'].tobytes()) for c in cases if c['group'] != 'activation']
    assert len(set(data)) == len(data)
    again = layer_cases.random_case(7)
    first = layer_cases.random_case(7)
    assert again['name'] == first['name'] and np.array_equal(again['x'], first['x'])
    # every case is small: the largest extent is 37; the activation sweep is one row of 335 values
    assert max(max(c['x'].shape[1:3]) for c in cases if c['group'] != 'activation') <= 40


def test_every_activation_name_of_the_plan_has_a_case():
    """keras_plan.ACT lists what an ``activation=`` may say; 'leaky_relu' and 'relu_clip' are the plan's own names of the
    LeakyReLU / ReLU(max_value) layers' codes, 'softmax' runs as the softmax kernel, None is 'linear'."""
    names = set(keras_plan.ACT) - {None, 'leaky_relu', 'relu_clip', 'softmax'}
    assert names == set(layer_cases.ACTIVATION_NAMES)
    fns = {c['kind']['fn'] for c in layer_cases.activation_cases()}
    assert {'leaky_relu', 'relu_clip', 'elu', 'relu'} <= fns
    assert set(layer_cases.ACTIVATION_NAMES) <= set(layer_ref.ACTIVATIONS)


def test_prelu_shared_axes_are_lowered_or_refused():
    """Every subset of (1, 2, 3) lowers when alpha has the matching shape; an alpha of any other shape is a PlanError, never a
    silent broadcast."""
    H, W, C = 5, 7, 3
    for shared in layer_cases.PRELU_SHARED:
        case = layer_cases.prelu_case(shared, H, W, C)
        plan = keras_plan.build_plan(case['cfg'], case['weights'])
        ops = [o for o in plan.ops if o['op'] == keras_plan.OP_PRELU]
        assert len(ops) == 1
        per_channel = set(shared or []) >= {1, 2}
        assert ops[0]['mode'] == int(not per_channel) and plan.weights[ops[0]['w0']].size == (C if per_channel else H * W * C)
        for other in layer_cases.PRELU_SHARED:
            shp = layer_cases.prelu_alpha_shape(other, H, W, C)
            if shp == layer_cases.prelu_alpha_shape(shared, H, W, C):
                continue
            with pytest.raises(keras_plan.PlanError):
                keras_plan.build_plan(case['cfg'], {'op': [np.zeros(shp, np.float32)]})


def test_strided_cases_really_run_on_strided_views():
    """The fused plan of every strided case has the op under test reading a view with c_stride != c at a channel offset that is a
    multiple of 4 and at one that is not, and writing such views (asserted again where the device runs them)."""
    for case in layer_cases.strided_cases():
        for fuse in case['fuses']:
            plan = keras_plan.build_plan(case['cfg'], case['weights'], fuse=fuse)
            r, w = layer_cases.strided_views(plan, case['kind']['strided'], keras_plan)
            assert {o % 4 == 0 for o in r} == {True, False}, (case['name'], r)
            assert {o % 4 == 0 for o in w} == {True, False}, (case['name'], w)
