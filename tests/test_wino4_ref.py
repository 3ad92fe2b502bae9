"""tests/wino4_ref.py and tests/wino4_cases.py without a GPU: the truth agrees with the project's other float64 oracles, the replay is the
arithmetic tools/wino_points.py chose the points with, it stays under the hard bound of tests/test_gpu_wino4_accuracy.py at every output
of every case in both modes, and every case reaches an F(4x4) kernel.  Prints each case's rho_max / rho_rms (run with -s)."""
import numpy as np
import pytest

from oracle import unet as oracle_unet
from tests import conv_exact_cases as cx
from tests import conv_exact_ref
from tests import wino4_cases as wc
from tests import wino4_ref as ref


def _layer_cfg(H, W, cin, cout, act, extra=()):
    return cx._F([cx._in(H, W, cin), cx.conv_layer('c', 'in', cout, 3, act=act)] + list(extra), extra[-1]['config']['name'] if extra else 'c')


@pytest.mark.parametrize('act', ['linear', 'relu'])
def test_truth_agrees_with_the_exact_suites_oracle(act):
    rng = np.random.default_rng(5)
    x = rng.normal(size=(2, 8, 12, 5)).astype(np.float32)
    w, b = rng.normal(size=(3, 3, 5, 7)).astype(np.float32), rng.normal(size=7).astype(np.float32)
    want = conv_exact_ref.forward(_layer_cfg(8, 12, 5, 7, act), {'c': [w, b]}, x)[0]
    got = ref.truth(x, w, b, act)
    assert got.dtype == np.float64 and np.abs(got - want).max() <= 1e-13 * np.abs(want).max()
    pool = cx._L('MaxPooling2D', 'p', ['c'], pool_size=[2, 2], strides=[2, 2], padding='valid')
    want = conv_exact_ref.forward(_layer_cfg(8, 12, 5, 7, act, [pool]), {'c': [w, b]}, x)[0]
    assert np.abs(ref.truth(x, w, b, act, tail='pool') - want).max() <= 1e-13 * np.abs(want).max()


def test_truth_agrees_with_oracle_unet_on_a_softmax_head():
    rng = np.random.default_rng(6)
    x = rng.normal(size=(1, 8, 8, 8)).astype(np.float32)
    w, b = (rng.normal(size=(3, 3, 8, 64)) / 8).astype(np.float32), rng.normal(size=64).astype(np.float32)
    hw, hb = (rng.normal(size=(1, 1, 64, 4)) / 8).astype(np.float32), rng.normal(size=4).astype(np.float32)
    head = cx.conv_layer('h', 'c', 4, 1, act='softmax')
    want = oracle_unet.forward(_layer_cfg(8, 8, 8, 64, 'relu', [head]), {'c': [w, b], 'h': [hw, hb]}, x, dtype=np.float64)
    got = ref.truth(x, w, b, 'relu', tail='head', head=(hw, hb))
    assert np.abs(got - np.asarray(want, np.float64)).max() <= 1e-12


def test_replay_is_the_arithmetic_the_points_were_chosen_with():
    """The values tools/wino_points.py's kernel_order_error printed before its body moved to tests/wino4_ref.py, to the last digit; the tool
    now imports the replay."""
    a, b = ref.points()
    assert (a, b) == (0.625, 1.5)
    assert repr(ref.kernel_order_error(a, b, 64)) == '6.021283808887239e-07'
    assert repr(ref.kernel_order_error(a, b, 8)) == '3.5113575591246043e-07'
    import inspect
    from tools import wino_points
    assert 'wino4_ref.kernel_order_error' in inspect.getsource(wino_points.kernel_order_error)


def test_transform_matrices_are_a_convolution():
    """A^T [(G g G^T) . (B^T d B)] A is the 3 x 3 correlation of a 6 x 6 tile, in float64."""
    BT, G, AT = ref.matrices()
    rng = np.random.default_rng(1)
    d, g = rng.normal(size=(6, 6)), rng.normal(size=(3, 3))
    y = AT @ ((G @ g @ G.T) * (BT @ d @ BT.T)) @ AT.T
    want = sum(g[r, q] * d[r:r + 4, q:q + 4] for r in range(3) for q in range(3))
    assert np.abs(y - want).max() < 1e-12


def test_hard_count():
    assert ref.hard_count(8, 'fp32') == 23 and ref.hard_count(12, 'fp32') == 31 and ref.hard_count(256, 'bf16x3') == 274


@pytest.mark.parametrize('shape,family', wc.all_groups(), ids=lambda v: v)
def test_every_case_resolves_to_an_f4x4_kernel(shape, family):
    for case in wc.build(shape, family)[:3]:
        plan = wc.plan_of(case)
        d = wc.layer_under_test(plan)
        assert d['path'] == 'mfma' and d['wino4'] and d['in_view'] == bool(case.get('in_view')), (case['name'], d)
        for opts in wc.options(shape):
            kinds = dict(cx.profile_kinds(plan, opts))
            assert kinds[d['op']] == wc.kind_of(shape, opts), (case['name'], opts, kinds)
            assert wc.kind_of(shape, opts) == (5 if opts['winograd'] == 3 and wc.SHAPES[shape][4] % 64 == 0 else 2)


def test_cases_cover_what_they_claim():
    for shape in wc.PLAIN:
        n, H, W, cin, cout, tail = wc.SHAPES[shape]
        pairs = wc.delta_filter_pairs(shape)
        assert {(r, q) for r, q, _, _ in pairs} == {(r, q) for r in range(3) for q in range(3)}
        assert {ci // 4 for _, _, ci, _ in pairs} == set(range(cin // 4)) and {co // 32 for _, _, _, co in pairs} == set(range(cout // 32))
        pos = wc.delta_positions(H, W)
        ys, xs = {p[0] for p in pos}, {p[1] for p in pos}
        assert {0, H - 1} <= ys and {0, W - 1} <= xs
        assert all({t - 1, t} <= ys for t in range(4, H, 4)) and all({t - 1, t} <= xs for t in range(4, W, 4))
        chs = wc.delta_channels(cin)
        assert set(range(8)) <= set(chs) and set(range((cin - 1) // 8 * 8, cin)) <= set(chs) and len(pos) >= len(chs)
    k = wc._rng('disparate_k', 'deep').integers(-10, 11, size=256)
    assert k.min() == -10 and k.max() == 10


@pytest.mark.parametrize('shape,family', wc.all_groups(), ids=lambda v: v)
def test_replay_stays_under_the_hard_bound(shape, family):
    modes = sorted({wc.mode_of(shape, o) for o in wc.options(shape)})
    worst = {}
    for case, R in wc.references(shape, family):
        for mode in modes:
            m = R.measure(R.replay(mode), mode)
            assert m['over'] == 0, '%s %s: %d outputs beyond the bound, worst %.3g of it' % (case['name'], mode, m['over'], m['worst'])
            w = worst.setdefault(mode, dict(rho_max=0.0, rho_rms=0.0, worst=0.0))
            for k in w:
                w[k] = max(w[k], m[k])
    for mode, w in worst.items():
        print('\n%s/%s %s: rho_max %.4g rho_rms %.4g, largest error / hard bound %.3g' % (shape, family, mode, w['rho_max'], w['rho_rms'], w['worst']))


def test_replay_gives_exact_zeros_and_biases():
    """The exact assertions of the device test on the replay, with NOTHING skipped (every tile and channel replayed): a tile whose 6 x 6 x Cin
    inputs are all zero gives exact zeros, an output channel whose filter slice is zero gives its bias."""
    case = wc.delta_input('odd_regions')
    x, w, b, act = case['layer']
    sparse = ref.Tiles(x, w)
    full = ref.Tiles(x, w, everything=True)
    assert len(full.idx) == x.shape[0] * 16 and 0 < len(sparse.idx) <= 4 * x.shape[0]
    for mode in ('fp32', 'bf16x3'):
        y = full.scatter(ref.replay_tiles(full, None, mode), np.zeros(64))
        assert sparse.rest_equals(y.astype(np.float32), np.zeros(64)) and np.abs(y).max() > 0
        assert np.array_equal(sparse.gather(y), ref.replay_tiles(sparse, None, mode))
    case = wc.delta_filter('odd_regions')[4]
    x, w, b, act = case['layer']
    sparse, full = ref.Tiles(x, w), ref.Tiles(x, w, everything=True)
    assert list(sparse.chans) == [case['tap'][3]] and len(full.chans) == 64
    for mode in ('fp32', 'bf16x3'):
        y = full.scatter(ref.replay_tiles(full, b, mode), b)
        assert sparse.rest_equals(y.astype(np.float32), b)
        # the moved input channel: one product x * 1.0, nothing else on the path is non-zero, but U = G e G^T is not a delta: it rounds
        assert np.abs(sparse.gather(y) - ref.truth_tiles(sparse, b)).max() > 0
