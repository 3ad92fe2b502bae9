"""NuSeT's network stage on the device (csrc/nuset_kernels.hip, ecseg_nuset_forward, ecseg_rpn_proposals[_last]): the three-output
plan against the CPU oracle (oracle/unet.py), the argmax mask against the device's own logits, and the proposal layer against its
float32 restatement (tests/nuset_ref.py) on the cases of tests/nuset_cases.py - selected candidates and scores exactly, coordinates
within a few float32 ulp.  tests/test_nuset.py shows without a GPU that no decision of those cases hangs on a rounding.

Beyond the hand-made cases: the boundary cases (sort lengths 2048 .. 32768 with none, one and thousands of padding keys, K = 8192,
ties across sort blocks, cuts by pre_nms_top_n and post_nms_top_n, thousands of filtered candidates, and ``whole_order``, whose
result is the device's entire sorted order), the decided seeds of the committed random range, one handle over calls of changing
size, and the seeds that tools/fuzz_nuset.py once found failing.  ``case_mismatches`` is the comparison of all of them and of
that campaign (tests/nuset_ref.py)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import nuset_cases as cases                  # noqa: E402
import nuset_ref as ref                      # noqa: E402

from ecseg_amd import _lib, keras_plan, nuset          # noqa: E402
from oracle import unet as oracle_unet       # noqa: E402

pytestmark = pytest.mark.gpu
TOL = 1e-3                                   # the bound of tests/test_gpu_unet.py for the NuSeT-shaped U-Net: TOL * max(1, |oracle|.max())
BASE = 8


def _image(h, w, seed):
    """A normalised image: smooth blobs plus noise, zero mean and unit variance."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[:h, :w]
    img = rng.normal(0.0, 0.3, (h, w))
    for _ in range(6):
        cy, cx, r = rng.uniform(0, h), rng.uniform(0, w), rng.uniform(3, 9)
        img += 3.0 * np.exp(-((yy - cy) ** 2 + (xx - cx) ** 2) / (2 * r * r))
    return nuset.whole_image_norm(img)


@pytest.fixture(scope='module')
def weights():
    return nuset.synth_weights(nuset.nuset_config(16, 16, BASE), seed=21)


@pytest.mark.parametrize('h,w', [(32, 48), (64, 96)])
def test_three_output_plan_and_mask(gpu, weights, h, w):
    cfg = nuset.nuset_config(h, w, BASE)
    plan = keras_plan.build_plan(cfg, weights, keep=nuset.RPN_LAYERS[1:])
    gpu.load_plan(plan)
    x = _image(h, w, h + w)
    cls_t, bbox_t = (plan.layer_tensor[n] for n in nuset.RPN_LAYERS[1:])
    mask = gpu.nuset_forward(x, cls_t, bbox_t)
    got = [gpu.read_tensor(t, 1)[0] for t in (plan.output_tensor, cls_t, bbox_t)]
    want = [oracle_unet.forward(cfg, weights, x[None, :, :, None], output=k)[0] for k in range(3)]
    assert [g.shape for g in got] == [(h, w, 2), (h // 16, w // 16, 42), (h // 16, w // 16, 84)]
    bounds = []
    for name, g, o in zip(('final', 'rpn_cls_score', 'rpn_bbox_pred'), got, want):
        assert g.shape == o.shape, name
        bound = TOL * max(1.0, float(np.abs(o).max()))
        err = float(np.abs(g - o).max())
        print(name, 'max error', err, 'bound', bound)
        assert err < bound, (name, err, bound)
        bounds.append(bound)
    # the mask is the argmax of the device's own logits, a tie giving 0 ...
    assert mask.dtype == np.uint8 and mask.shape == (h, w)
    assert np.array_equal(mask, (got[0][..., 1] > got[0][..., 0]).astype(np.uint8))
    assert 0 < int(mask.sum()) < mask.size
    # ... and the oracle's wherever the oracle's two logits differ by more than the bound
    sure = np.abs(want[0][..., 1] - want[0][..., 0]) > bounds[0]
    assert sure.mean() > 0.9
    assert np.array_equal(mask[sure], (want[0][..., 1] > want[0][..., 0]).astype(np.uint8)[sure])


def test_argmax_tie_gives_zero(gpu):
    """All-zero weights without biases in front of ``final``: both logits are 0 everywhere, and tf.argmax returns the first."""
    cfg = nuset.nuset_config(32, 32, 4)
    w = {k: [np.zeros_like(a) for a in v] for k, v in nuset.synth_weights(cfg, seed=1).items()}
    plan = keras_plan.build_plan(cfg, w, keep=nuset.RPN_LAYERS[1:])
    gpu.load_plan(plan)
    mask = gpu.nuset_forward(_image(32, 32, 3), plan.layer_tensor['rpn_cls_score'], plan.layer_tensor['rpn_bbox_pred'])
    assert not mask.any()
    assert not gpu.read_tensor(plan.output_tensor, 1).any()


@pytest.fixture(scope='module')
def expected():
    """The float32 restatement of every case, computed once."""
    out = {}
    for make in cases.ALL:
        c = make()
        out[c['name']] = (c, ref.proposals(c['cls'], c['bbox'], c['ref'], c['stride'], c['im_h'], c['im_w'], c['thr'], c['pre'], c['post']))
    return out


@pytest.mark.parametrize('name', [f.__name__ for f in cases.ALL])
def test_proposals_from_given_tensors(gpu, expected, name):
    c, want = expected[name]
    scores, props, idx = gpu.rpn_proposals(c['cls'], c['bbox'], c['ref'], c['stride'], c['im_h'], c['im_w'], c['thr'], c['pre'], c['post'])
    assert scores.dtype == np.float32 and props.dtype == np.float32 and idx.dtype == np.int32
    assert len(scores) == len(props) == len(idx) and props.shape == (len(idx), 4)
    print(name, 'n_out', len(idx), 'expected', len(want['indices']))
    assert idx.tolist() == want['indices'].tolist()
    assert np.array_equal(scores, want['scores'])
    if len(idx):
        err = float(np.abs(props.astype(np.float64) - want['proposals'].astype(np.float64)).max())
        tol = 4 * float(np.spacing(np.float32(max(c['im_h'], c['im_w']))))
        print(name, 'max coordinate error', err, 'tolerance', tol)
        assert err <= tol
        assert np.all(np.diff(scores) <= 0)
        assert props[:, [0, 2]].min() >= 0 and props[:, [0, 2]].max() <= c['im_w'] - 1 and props[:, [1, 3]].max() <= c['im_h'] - 1


def test_expected_counts_cover_every_branch(expected):
    n = {k: len(v[1]['indices']) for k, v in expected.items()}
    assert n['all_filtered'] == 0 and n['top_k_cut'] == 800 and n['cap'] == 800 and 0 < n['small'] < 20
    assert expected['top_k_cut'][1]['kept'] == 6069 and expected['small'][1]['kept'] < expected['small'][0]['pre']


def test_run_last_variant_equals_host_tensor_variant(gpu, weights):
    h, w = 64, 96
    net = nuset.NuSeT(weights, base=BASE, handle=gpu)
    x = _image(h, w, 5)
    mask, scores, props = net.run(x, nms_threshold=0.3)
    assert mask.shape == (h, w) and len(scores) > 0 and props.shape == (len(scores), 4)
    cls, bbox = (gpu.read_tensor(net.plan.layer_tensor[n], 1)[0] for n in nuset.RPN_LAYERS[1:])
    size = nuset.anchor_size(mask, gpu)
    assert size is not None and size >= 1
    s2, p2, i2 = gpu.rpn_proposals(cls, bbox, nuset.reference_anchors(size), nuset.STRIDE, h, w, 0.3)
    s3, p3, i3 = gpu.rpn_proposals_last(nuset.reference_anchors(size), nuset.STRIDE, h, w, 0.3)
    assert np.array_equal(scores, s2) and np.array_equal(props, p2)
    assert np.array_equal(s3, s2) and np.array_equal(p3, p2) and np.array_equal(i3, i2)
    assert len(np.unique(i2)) == len(i2) and i2.min() >= 0 and i2.max() < 4 * 6 * 21
    # the same plan serves the next image of that extent; a second mask is the first one again
    before = gpu.plan
    assert np.array_equal(net.mask(x), mask) and gpu.plan is before


def test_error_paths(gpu, weights):
    plan = keras_plan.build_plan(nuset.nuset_config(32, 48, BASE), weights, keep=nuset.RPN_LAYERS[1:])
    gpu.load_plan(plan)
    cls_t, bbox_t = (plan.layer_tensor[n] for n in nuset.RPN_LAYERS[1:])
    ref_a = nuset.reference_anchors(12.0)
    with pytest.raises(_lib.EcsegError, match='ecseg_nuset_forward') as e:
        gpu.nuset_forward(np.zeros((32, 32), np.float32), cls_t, bbox_t)            # another extent than the plan's
    assert e.value.code == -1                                # ECSEG_E_INVALID
    with pytest.raises(_lib.EcsegError, match='call ecseg_nuset_forward first'):
        gpu.rpn_proposals_last(ref_a, 16, 32, 48, 0.3)                              # a fresh plan has no RPN tensors yet
    with pytest.raises(_lib.EcsegError):
        gpu.nuset_forward(np.zeros((32, 48), np.float32), cls_t, cls_t)
    gpu.nuset_forward(np.zeros((32, 48), np.float32), cls_t, bbox_t)
    with pytest.raises(_lib.EcsegError, match='anchors per position'):
        gpu.rpn_proposals_last(ref_a[:5], 16, 32, 48, 0.3)
    c = cases.small()
    with pytest.raises(_lib.EcsegError, match='pre_nms_top_n'):
        gpu.rpn_proposals(c['cls'], c['bbox'], c['ref'], 16, 32, 48, 0.3, pre_nms_top_n=_lib.Handle.RPN_MAX_PRE_NMS + 1)
    with pytest.raises(ValueError):
        gpu.rpn_proposals(c['cls'], c['bbox'][..., :8], c['ref'], 16, 32, 48, 0.3)


# ---- boundary cases, the seeded range, handle reuse ---------------------------------------------------------------------------
def _want(c):
    return ref.run_case(c, gaps=False)                       # (decided already: tests/test_nuset.py)


case_mismatches = ref.case_mismatches


@pytest.fixture(scope='module')
def boundary():
    """name -> (case, float32 restatement), each computed when first asked for and then shared."""
    made = {}

    def get(name):
        if name not in made:
            c = getattr(cases, name)()
            made[name] = (c, _want(c))
        return made[name]
    return get


@pytest.mark.parametrize('name', [f.__name__ for f in cases.BOUNDARY])
def test_boundary_cases(gpu, boundary, name):
    c, want = boundary(name)
    bad, err, unequal, (scores, props, idx) = case_mismatches(gpu, c, want, raw=True)
    print(name, 'n_out', len(idx), 'expected', len(want['indices']), 'max coordinate error', err, 'coordinates not bit-equal', unequal)
    assert not bad, (name, bad)
    if name == 'whole_order':
        assert len(idx) == 8192 and sorted(idx.tolist()) == list(range(8192))


def test_random_cases(gpu):
    decided = [s for s in cases.RANDOM_SEEDS if s not in cases.RANDOM_UNDECIDED]
    assert 10 * len(decided) >= 9 * len(cases.RANDOM_SEEDS)
    failing, worst, unequal, compared = {}, 0.0, 0, 0
    for seed in decided:
        c = cases.random_case(seed)
        want = _want(c)
        bad, err, ne = case_mismatches(gpu, c, want)
        worst, unequal, compared = max(worst, err), unequal + ne, compared + len(want['indices'])
        if bad:
            failing[seed] = bad
    print('seeds', len(decided), 'skipped as undecided', list(cases.RANDOM_UNDECIDED), 'proposals compared', compared,
          'max coordinate error', worst, 'coordinates not bit-equal', unequal)
    assert not failing, failing


def test_handle_reuse_across_sizes(gpu, boundary):
    """The key and matrix buffers only grow and are never cleared, and the row pitch of the matrix changes from call to call: a
    large call, two smaller ones, and the large one again on one handle."""
    out = []
    for name, (c, want) in (('n21504', boundary('n21504')), ('small', (cases.small(), _want(cases.small()))), ('n2050', boundary('n2050')),
                            ('n21504', boundary('n21504'))):
        bad, err, unequal, got = case_mismatches(gpu, c, want, raw=True)
        print(name, 'n_out', len(got[2]), 'max coordinate error', err)
        assert not bad, (name, len(out), bad)
        out.append([a.copy() for a in got])
    assert all(a.tobytes() == b.tobytes() for a, b in zip(out[0], out[3]))


# Seeds of tools/fuzz_nuset.py that once failed, as (seed, max_positions); none so far
CAMPAIGN_REGRESSIONS = ()


def test_regressions(gpu):
    for seed, max_positions in CAMPAIGN_REGRESSIONS:
        c = cases.random_case(seed, max_positions)
        reason, want = ref.judge(c)
        assert reason is None, (seed, max_positions, reason)
        bad, err, unequal = case_mismatches(gpu, c, want)
        assert not bad, (seed, max_positions, bad)
