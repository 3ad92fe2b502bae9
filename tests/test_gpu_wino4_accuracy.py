"""The three F(4x4) Winograd kernels (conv_wino4r_kernel, conv_wino4_kernel, conv_wino4s_kernel) against a float64 direct convolution, with
a bound at every single output.  Cases and data families: tests/wino4_cases.py; truth, scale, replay and count: tests/wino4_ref.py;
tests/test_wino4_ref.py holds the replay to the same bound without a GPU.

For every case, family and option set (winograd 2 | 3, the lone 32-channel block also with wino4_split = 0):

1. the launch profile shows the expected kernel kind (2 fp32, 5 bf16x3; Cout % 64 != 0 under winograd = 3 stays on 2) and fusion bits, and a
   second call returns the same bytes;
2. HARD BOUND  |got - truth| <= hard_count u Q + u |truth| at every output (u = 2^-24; Q: the per-output scale |A^T| (sum_c |G g G^T| .
   |B^T d B|) |A| with absolute values taken factor by factor; hard_count: the roundings on an output's path, derived in
   wino4_ref.hard_count);
3. SHARP GATE  with rho = |got - truth| / (u Q):  rho_rms(device) <= 1.5 rho_rms(replay)  and  rho_max(device) <= 3 rho_max(replay), both
   measured against the float64 truth on the same data in the same run - never device against replay, never a limit taken from the device.
   The replay is the kernels' float32 arithmetic on the CPU.  The order of float32 accumulation on the matrix cores and across split-K
   differs from the replay's: that moves single errors, not their distribution, so the rms is the stable statistic and gets the tight
   margin - below the 2.2 x between the textbook points {1, 2} and the chosen {5/8, 3/2}, which must fail it; the maximum is the tail of
   the same distribution over at most 2 10^5 outputs;
4. EXACT  a tile whose 6 x 6 x Cin inputs are all zero gives exact zeros (delta_input), an output channel whose filter slice is zero gives
   its bias bit for bit (delta_filter): V = 0 or U = 0 makes every step add exact zeros, whatever the rounding.

Each test prints its rho values (-s).
"""
import numpy as np
import pytest

from tests import conv_exact_cases as cx
from tests import wino4_cases as wc

pytestmark = pytest.mark.gpu

RMS_MARGIN, MAX_MARGIN = 1.5, 3.0


class _Options:
    def __init__(self, gpu, opts):
        self.gpu, self.opts = gpu, opts

    def __enter__(self):
        for k, v in self.opts.items():
            self.gpu.set_option(k, v)
        return self.opts

    def __exit__(self, *exc):
        self.gpu.set_kernel_profiling(False)
        for k, v in cx.LIBRARY_DEFAULTS.items():
            self.gpu.set_option(k, v)


def _forward(gpu, x):
    """forward_patches in batches of wc.BATCH images; the launch records of the first batch."""
    outs, recs = [], None
    for i in range(0, x.shape[0], wc.BATCH):
        if recs is None:
            gpu.set_kernel_profiling(True)
        outs.append(gpu.forward_patches(x[i:i + wc.BATCH]))
        if recs is None:
            recs = [(r['op'], r['kind']) for r in gpu.conv_launch_profile()]
            gpu.set_kernel_profiling(False)
    return (outs[0] if len(outs) == 1 else np.concatenate(outs)), recs


class _Pool:
    """rho over all outputs of the cases of one (shape, family, options)."""

    def __init__(self):
        self.sq, self.n, self.max = 0.0, 0, 0.0

    def add(self, m):
        self.sq += m['rho_rms'] ** 2 * m['n']
        self.n += m['n']
        self.max = max(self.max, m['rho_max'])

    @property
    def rms(self):
        return float(np.sqrt(self.sq / max(self.n, 1)))


@pytest.mark.parametrize('shape,family', wc.all_groups(), ids=lambda v: v)
def test_f4x4_against_float64(gpu, shape, family):
    refs = wc.references(shape, family)
    plans = [wc.plan_of(case) for case, _ in refs]
    bad = []
    for opts in wc.options(shape):
        mode, kind = wc.mode_of(shape, opts), wc.kind_of(shape, opts)
        dev, rep = _Pool(), _Pool()
        with _Options(gpu, opts):
            for (case, R), plan in zip(refs, plans):
                tag = '%s [%s]' % (case['name'], wc.opts_id(opts))
                gpu.load_plan(plan)
                got, recs = _forward(gpu, case['x'])
                again, _ = _forward(gpu, case['x'])
                # 1. the kernel that ran
                expect = cx.profile_kinds(plan, opts)
                under_test = wc.layer_under_test(plan)['op']
                if [(o, k & 0xff) for o, k in recs] != expect or dict(expect)[under_test] != kind:
                    bad.append('%s: launch profile %s, expected kinds %s with kind %d on op %d' % (tag, recs, expect, kind, under_test))
                bits = 0
                for _, k in recs:
                    bits |= k & 0x700
                if bits != case['bits']:
                    bad.append('%s: fusion bits 0x%x, expected 0x%x' % (tag, bits, case['bits']))
                if got.tobytes() != again.tobytes():
                    bad.append('%s: a second call gives other bytes' % tag)
                if got.shape != R.truth.shape and case['tail'] is not None:
                    bad.append('%s: shape %s, expected %s' % (tag, got.shape, R.truth.shape))
                    continue
                # 4. exact zeros / biases outside the active tiles and channels
                vals, rest_ok = R.select(got)
                if not rest_ok:
                    bad.append('%s: an output with an all-zero input tile or an all-zero filter slice is not act(bias) bit for bit' % tag)
                # 2. the hard bound, at every output
                m = R.measure(vals, mode)
                if m['over'] or not np.isfinite(vals).all():
                    bad.append('%s: %d of %d outputs beyond hard_count u Q + u |truth| (hard_count %d), the worst at %.3g of its bound'
                               % (tag, m['over'], vals.size, R.count(mode), m['worst']))
                dev.add(m)
                rep.add(R.measure(R.replay(mode), mode))
        # 3. the sharp gate
        print('\n%s/%s [%s] %s: device rho_max %.4g rho_rms %.4g | replay rho_max %.4g rho_rms %.4g | %d outputs'
              % (shape, family, wc.opts_id(opts), mode, dev.max, dev.rms, rep.max, rep.rms, dev.n))
        assert rep.n == dev.n and rep.n > 0
        if dev.rms > RMS_MARGIN * rep.rms:
            bad.append('%s/%s [%s]: rho_rms %.4g on the device, %.4g in the replay: beyond %.1f x' % (shape, family, wc.opts_id(opts), dev.rms, rep.rms, RMS_MARGIN))
        if dev.max > MAX_MARGIN * rep.max:
            bad.append('%s/%s [%s]: rho_max %.4g on the device, %.4g in the replay: beyond %.0f x' % (shape, family, wc.opts_id(opts), dev.max, rep.max, MAX_MARGIN))
    assert not bad, '\n'.join(bad)
