"""Every convolution path of the library against tests/conv_exact_ref.py with NO tolerance, on the cases of tests/conv_exact_cases.py
(tests/test_conv_exact.py ties them to the float64 oracle and asserts their preconditions without a GPU).

Why bit equality may be asked for.

lattice   Inputs, weights and biases are integers.  A float32 holds every integer below 2^24 exactly, so a sum of integer products
          whose every partial sum stays below 2^24 in magnitude is exact in any order, with or without fused multiply-adds, on the
          vector ALU and on the matrix cores alike.  With S = sum |x| |w| + |b| over the receptive field of an output, every partial
          sum of that output is at most S.
          * direct kernels (conv_mfma / first / small_cin / head / generic / dwconv / the transposed ones): max S < 2^24.
          * F(2x2, 3x3) kernels (conv_wino, conv_wino_res, conv_wino16) compute Y = A^T [ sum_c (G g G^T) . (B^T d B) ] A with
            B^T = [1 0 -1 0; 0 1 1 0; 0 -1 1 0; 0 1 0 -1], G = [1 0 0; 1/2 1/2 1/2; 1/2 -1/2 1/2; 0 0 1], A^T = [1 1 1 0; 0 1 -1 -1].
            B has entries 0, +-1 and two non-zeros per row: B^T d B is integral, at most 4 max|x|.  G has row sums of magnitudes <= 3/2:
            G g G^T is at most 9/4 max|w|, and integral when the weights are multiples of 4 (two factors 1/2).  The element-wise product
            summed over Cin is at most 9 Cin max|x| max|w|, and A^T M A adds 3 x 3 = 9 of those: every intermediate stays below
            4 * 9/4 * 9 * Cin max|x| max|w| + max|b| = 81 Cin max|x| max|w| + max|b|, which must be < 2^24.
          * the bf16x3 GEMM (convs_kernel, winograd = 3) splits each operand into three bf16 pieces; an integer of at most 8 bits is
            its own first piece and the other two are zero, so the six piece products are the integer product and five zeros.
impulse   direct kernels only (no transform).  Delta input: one 1.0 in an all-zero input, arbitrary float32 weights (24 significant
          bits, 1e-20 .. 1e20), no bias: every output is one product w * 1.0 plus exact zeros - the flipped filter around the pixel.
          Delta filter: one 1.0 in an all-zero filter, arbitrary data, bias 0 on that output channel: the output channel is the moved
          input channel, the others their bias.  On the bf16x3 GEMM the three pieces of a float32 hold its 24 bits in 8 + 8 + 8, the
          products by 1.0 are the pieces, and their float32 sum in any order is the value: a dropped piece product shows.
identity  the F(4x4) kernels (conv_wino4 / wino4r / wino4s): G has 225, 2975 and 1071 in its denominators, nothing is exact.  What
          holds whatever the rounding: an image's result does not depend on the batch around it, and input channels that are zero with
          zero filter slices add exact zeros in the order the shorter layer's padding does.  Cin = 4 against 8 is not asked: a Cin <= 4
          layer runs on conv_small_cin_kernel by ecseg_amd/csrc/model_load.hip's rule and never reaches these kernels.

Each case runs under the options it names; the launch profile must show the kernel kinds (bits 0-7) that tests/conv_exact_cases.py
derives from the plan, and the fusion bits (0x100 pool, 0x200 head, 0x400 first layer) that the case expects.  Equality is
``np.array_equal(got, float32(reference))``; a second call must return the same bytes.
"""
import numpy as np
import pytest

from ecseg_amd import keras_plan

from tests import conv_exact_cases as cases
from tests import conv_exact_ref as ref

pytestmark = pytest.mark.gpu


class _Options:
    def __init__(self, gpu, opts):
        self.gpu, self.opts = gpu, dict(cases.OPTION_DEFAULTS, **opts)

    def __enter__(self):
        for k, v in self.opts.items():
            self.gpu.set_option(k, v)
        return self.opts

    def __exit__(self, *exc):
        self.gpu.set_kernel_profiling(False)
        for k, v in cases.LIBRARY_DEFAULTS.items():
            self.gpu.set_option(k, v)


def _run_profiled(gpu, x):
    gpu.set_kernel_profiling(True)
    got = gpu.forward_patches(x)
    recs = [(r['op'], r['kind']) for r in gpu.conv_launch_profile()]
    gpu.set_kernel_profiling(False)
    return got, recs


def run_case(gpu, case, seen):
    """-> list of failure messages."""
    want = ref.forward(case['cfg'], case['weights'], case['x'])[0]
    want32 = want.astype(np.float32)
    assert np.array_equal(want32.astype(np.float64), want.astype(np.float64)), case['name']
    plan = keras_plan.build_plan(case['cfg'], case['weights'])
    bad = []
    with _Options(gpu, case['opts']) as opts:
        gpu.load_plan(plan)
        got, recs = _run_profiled(gpu, case['x'])
        again = gpu.forward_patches(case['x'])
    expect = cases.profile_kinds(plan, opts)
    if [(o, k & 0xff) for o, k in recs] != expect:
        bad.append('%s: launch profile %s, expected kinds %s' % (case['name'], recs, expect))
    bits = 0
    for _, k in recs:
        bits |= k & 0x700
    if bits != case['bits']:
        bad.append('%s: fusion bits 0x%x, expected 0x%x' % (case['name'], bits, case['bits']))
    if not bad:
        seen |= cases.plan_labels(plan, opts)
    if got.shape != want32.shape:
        return bad + ['%s: shape %s, expected %s' % (case['name'], got.shape, want32.shape)]
    if got.tobytes() != again.tobytes():
        bad.append('%s: a second call gives other bytes' % case['name'])
    if not np.array_equal(got, want32):
        wrong = got != want32
        i = np.unravel_index(np.argmax(wrong), wrong.shape)
        bad.append('%s: %d of %d differ, first at %s: %r, expected %r' % (case['name'], wrong.sum(), wrong.size, i, got[i], want32[i]))
    return bad


_DONE = {}          # lattice group -> (failures, path labels seen), so that the coverage test does not run a group twice


def _lattice(gpu, group):
    if group not in _DONE:
        bad, seen = [], set()
        for case in cases.lattice_cases(group):
            bad.extend(run_case(gpu, case, seen))
        _DONE[group] = (bad, seen)
    return _DONE[group]


@pytest.mark.parametrize('group', cases.LATTICE_GROUPS + ('random',))
def test_lattice_cases_bit_equal(gpu, group):
    bad, seen = _lattice(gpu, group)
    print('\n%s: %d cases, paths seen: %s' % (group, len(cases.lattice_cases(group)), ' '.join(sorted(seen))))
    assert not bad, '\n'.join(bad)


def test_every_kernel_family_is_seen_in_the_launch_profile(gpu):
    """Over the fixed groups, and again over the seeded range alone: every path of conv_exact_cases.PATHS ran with the launch profile
    (where it reports the kernel) showing the expected kind and fusion bits."""
    fixed = set()
    for group in cases.LATTICE_GROUPS:
        fixed |= _lattice(gpu, group)[1]
    assert set(cases.PATHS) <= fixed, sorted(set(cases.PATHS) - fixed)
    seeded = _lattice(gpu, 'random')[1]
    assert set(cases.PATHS) <= seeded, sorted(set(cases.PATHS) - seeded)


@pytest.mark.parametrize('fam', sorted(cases.IMPULSE_FAMILIES))
def test_impulse_cases_bit_equal(gpu, fam):
    bad, seen = [], set()
    cs = cases.impulse_cases(fam)
    for case in cs:
        bad.extend(run_case(gpu, case, seen))
    assert not bad, '\n'.join(bad)
    assert cs[0]['path'] in seen


def _identity_run(gpu, case, opts, x=None):
    plan = keras_plan.build_plan(case['cfg'], case['weights'])
    with _Options(gpu, opts) as o:
        gpu.load_plan(plan)
        got, recs = _run_profiled(gpu, case['x'] if x is None else x)
    assert [(i, k & 0xff) for i, k in recs] == cases.profile_kinds(plan, o) and all((k & 0xff) in (2, 5) for _, k in recs), (case['name'], recs)
    return got


@pytest.mark.parametrize('opts', cases.IDENTITY_OPTS, ids=lambda o: 'winograd%d_split%d' % (o['winograd'], o['wino4_split']))
def test_f4x4_image_does_not_depend_on_its_batch(gpu, opts):
    bad = []
    for case in cases.identity_cases():
        full = _identity_run(gpu, case, opts)
        assert np.isfinite(full).all() and np.abs(full).max() > 0
        for k in range(case['x'].shape[0]):
            alone = _identity_run(gpu, case, opts, case['x'][k:k + 1])
            if alone[0].tobytes() != full[k].tobytes():
                bad.append('%s: image %d of %d differs from the same image alone in %d values (largest difference %g)'
                           % (case['name'], k, case['x'].shape[0], (alone[0] != full[k]).sum(), np.abs(alone[0] - full[k]).max()))
    assert not bad, '\n'.join(bad)


@pytest.mark.parametrize('opts', cases.IDENTITY_OPTS, ids=lambda o: 'winograd%d_split%d' % (o['winograd'], o['wino4_split']))
def test_f4x4_zero_input_channels_change_nothing(gpu, opts):
    bad, n = [], 0
    for shape in cases.IDENTITY_SHAPES:
        if shape[1] not in cases.IDENTITY_PADS:
            continue
        short = cases.identity_case(*shape)
        padded = cases.identity_case(*shape, pad_to=cases.IDENTITY_PADS[shape[1]])
        a, b = _identity_run(gpu, short, opts), _identity_run(gpu, padded, opts)
        n += 1
        if a.tobytes() != b.tobytes():
            bad.append('%s: Cin = %d differs from Cin = %d with zero channels in %d of %d values (largest difference %g)'
                       % (shape[0], shape[1], cases.IDENTITY_PADS[shape[1]], (a != b).sum(), a.size, np.abs(a - b).max()))
    assert n >= 3 and not bad, '\n'.join(bad)
