"""``keras_plan.build_plan``'s graph rewrites on the device against the float64 interpreter of the Keras graph (tests/plan_ref.py): every
hand case and seed of tests/plan_cases.py runs through ``build_plan`` and ``load_plan`` with ``fuse=True`` and ``fuse=False``, and the
model's output and every kept tensor are held, element by element, to

    |device - y| <= C_BOUND * 2^-24 * A

(C_BOUND and how it was measured: tests/plan_cases.py; which slips this bound catches: the mutant table of tests/test_plan_ref.py).
The whole-network tests beside this file (test_gpu_unet.py, test_gpu_nuset.py, test_gpu_more.py) keep their 1e-3 bound on the
committed topologies; this one aims a graph at each rewrite."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import plan_cases as pc                      # noqa: E402
import plan_ref                              # noqa: E402
from ecseg_amd import keras_plan             # noqa: E402

pytestmark = pytest.mark.gpu


def build(case, fuse):
    return keras_plan.build_plan(case['cfg'], case['weights'], fuse=fuse, lambda_overrides=case['lambda_affine'] or None,
                                 output=case['output'], keep=case['keep'])


def device_outputs(gpu, case, plan, x):
    """-> {tensor name: float32 array} of the plan's output and its kept tensors for the NHWC batch ``x``."""
    gpu.load_plan(plan)
    names = pc.outputs_of(case)
    got = {names[0]: gpu.forward_patches(x)}
    for nm in names[1:]:
        got[nm] = gpu.read_tensor(plan.layer_tensor[nm], len(x))
    return got


def ratio_of(got, y, A):
    err = np.abs(got.astype(np.float64) - y)
    with np.errstate(invalid='ignore', divide='ignore'):
        r = np.where(A > 0, err / (pc.U * A), np.where(err == 0, 0.0, np.inf))
    return np.where(np.isnan(r), np.inf, r)


def case_mismatches(gpu, case, x=None, fuses=(True, False)):
    """Runs one case with each ``fuse`` value -> (failure messages, worst ratio |device - y| / (C_BOUND 2^-24 A))."""
    bad, worst = [], 0.0
    if x is None:
        x, kx = pc.x_nhwc(case), case['x']
    else:
        kx = np.ascontiguousarray(np.transpose(x, (0, 3, 1, 2))) if case['channels_first'] else x
    vals = plan_ref.forward(case['cfg'], case['weights'], kx, case['lambda_affine'])
    for fuse in fuses:
        got = device_outputs(gpu, case, build(case, fuse), x)
        for nm, g in got.items():
            y, A = vals[nm]
            tag = '%s[fuse=%s] %s' % (case['name'], fuse, nm)
            if g.shape != y.shape:
                bad.append('%s: shape %s, expected %s' % (tag, g.shape, y.shape))
                continue
            r = ratio_of(g, y, A) / pc.C_BOUND
            worst = max(worst, float(r.max()))
            if not (r <= 1.0).all():
                i = np.unravel_index(np.argmax(r), r.shape)
                bad.append('%s: |got - y| = %.4g is %.3g x the bound at %s (got %r, y %r, A %.4g; %d of %d over)'
                           % (tag, abs(float(g[i]) - y[i]), r[i], i, g[i], y[i], A[i], int((r > 1.0).sum()), r.size))
    return bad, worst


@pytest.mark.parametrize('group', pc.GROUPS + ('random',))
def test_plan_against_float64_graph(gpu, group, capsys):
    bad, rows = [], []
    for case in pc.group_cases(group):
        b, worst = case_mismatches(gpu, case)
        bad.extend(b)
        rows.append('%-52s %.4f' % (case['name'], worst))
    with capsys.disabled():
        print('\n%s: worst |device - y| / (%g * 2^-24 * A) per case, fuse=True and fuse=False\n%s' % (group, pc.C_BOUND, '\n'.join(rows)))
    assert not bad, '\n'.join(bad)


@pytest.mark.parametrize('batch', [1, 3])
def test_allocator_cases_at_other_batch_sizes(gpu, batch, capsys):
    """Buffer sizes, and with them what the allocator may re-use, follow the batch."""
    bad, rows = [], []
    for case in pc.group_cases('alloc'):
        x = pc.x_nhwc(case)
        x = x[:1] if batch == 1 else np.concatenate([x, x[:1][:, ::-1].copy()])
        b, worst = case_mismatches(gpu, case, x=np.ascontiguousarray(x))
        bad.extend(b)
        rows.append('%-52s %.4f' % (case['name'], worst))
    with capsys.disabled():
        print('\nalloc, batch %d:\n%s' % (batch, '\n'.join(rows)))
    assert not bad, '\n'.join(bad)


def test_reloading_a_plan_gives_identical_bytes(gpu):
    """Two loads of one plan on one handle, another plan loaded in between: nothing of the first load or of the other plan is left."""
    names = ('alloc_ladder_of_12_with_skips_1_2_5_11', 'concat_tensor_in_two_concatenations', 'alloc_outputs_kept_by_keep', 'random_3')
    cases = [c for c in pc.hand_cases() + pc.random_cases() if c['name'] in names]
    assert len(cases) == len(names)
    for k, case in enumerate(cases):
        other = cases[(k + 1) % len(cases)]
        plan = build(case, True)
        first = device_outputs(gpu, case, plan, pc.x_nhwc(case))
        device_outputs(gpu, other, build(other, True), pc.x_nhwc(other))
        again = device_outputs(gpu, case, build(case, True), pc.x_nhwc(case))
        for nm in first:
            assert first[nm].tobytes() == again[nm].tobytes(), (case['name'], nm)
