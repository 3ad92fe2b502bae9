"""NuSeT's two ``rescale`` calls without a GPU: the numpy restatement (tests/rescale_ref.py) against scikit-image 0.18.3's own outputs
(tests/golden/nuset_rescale.npz, written by tools/make_golden_rescale.py) on every case of tests/rescale_cases.py - the Gaussian
stage and the final masks byte for byte, the float64 image within twice the stored ``down_maxdiff`` -; the host half of the binding
(extent and weights); ``scale_ratio`` through ``make stat_fish``'s ``nuset_weights`` key on injected handles; the new entry points
are declared, exported and built."""
import os
import sys

import numpy as np
import pytest
import yaml

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import rescale_cases as cases                # noqa: E402
import rescale_ref as ref                    # noqa: E402

import test_stat_fish as tsf                 # noqa: E402  (the oracle-backed handle and the folder builder)

from ecseg_amd import _lib, build, nuset     # noqa: E402
from ecseg_amd import stat_fish as sf        # noqa: E402

DOWN, UP = cases.down_cases(), cases.up_cases()
DOWN_NAMES, UP_NAMES = [c['name'] for c in DOWN], [c['name'] for c in UP]


@pytest.fixture(scope='module')
def golden():
    with np.load(os.path.join(HERE, 'golden', 'nuset_rescale.npz')) as z:
        return {k: z[k] for k in z.files}


def test_golden_holds_the_cases(golden):
    assert list(golden['down_names']) == DOWN_NAMES and list(golden['up_names']) == UP_NAMES
    for k, c in enumerate(DOWN):
        assert np.array_equal(golden['down_image_%d' % k], c['image']) and float(golden['down_scale_%d' % k]) == c['scale'], c['name']
    for k, c in enumerate(UP):
        assert np.array_equal(golden['up_mask_%d' % k], c['mask']) and float(golden['up_scale_%d' % k]) == c['scale'], c['name']
        assert tuple(golden['up_sizes_%d' % k]) == c['sizes'], c['name']
    # the restatement against skimage: below 1e-12 against a grey step of 3.9e-3, or the restatement is wrong
    assert 0 <= float(golden['down_maxdiff']) < 1e-12


@pytest.mark.parametrize('k', range(len(DOWN)), ids=DOWN_NAMES)
def test_down_restatement_equals_golden(golden, k):
    c = DOWN[k]
    out, filtered = ref.rescale_down(c['image'], c['scale'])
    want = golden['down_out_%d' % k]
    assert filtered.dtype == np.uint8 and np.array_equal(filtered, golden['down_filtered_%d' % k])
    assert out.dtype == np.float64 and out.shape == want.shape
    diff = float(np.abs(out - want).max())
    print('%s: |restatement - golden| = %.3g (bound %.3g)' % (c['name'], diff, 2 * float(golden['down_maxdiff'])))
    assert diff <= 2 * float(golden['down_maxdiff'])


@pytest.mark.parametrize('k', range(len(UP)), ids=UP_NAMES)
def test_up_restatement_equals_golden(golden, k):
    c = UP[k]
    for t in c['sizes']:
        got = ref.rescale_mask_up(c['mask'], c['scale'], t)
        assert got.dtype == np.uint8 and np.array_equal(got, golden['up_final_%d_%d' % (k, t)]), t


def test_cases_cover_what_they_name(golden):
    d = lambda name, key: golden['down_%s_%d' % (key, DOWN_NAMES.index(name))]
    u = lambda name, t: golden['up_final_%d_%d' % (UP_NAMES.index(name), t)]
    f = d('constant_200_s0.7', 'filtered')
    assert f.min() == f.max() == 198                                                   # the truncation of the two uint8 passes
    assert d('constant_255_s0.25', 'filtered').min() == 255 and d('constant_0_s0.25', 'out').max() == 0
    assert d('scene_53x47_s0.3', 'out').shape == (16, 14) and d('scene_203x331_s0.3', 'out').shape == (61, 99)
    assert len(_lib.rescale_weights(64, 19)) == 11 and len(_lib.rescale_weights(30, 21)) == 3 and len(_lib.rescale_weights(40, 10)) == 13
    v, t = ref.mask_up_values(UP[UP_NAMES.index('lone_pixel')]['mask'], 1 / 0.3)
    assert 0 < v.max() < 1 / 255 and u('lone_pixel', 0).max() == 255                   # vmin / vmax are not constants
    assert u('all_zero', 0).max() == 0 and u('all_one', 0).max() == 0                  # 0 / 0: all zero
    m = u('row1_col1', 0)
    assert m[0].max() == 255 and m[:, 0].max() == 255                                  # the mirrored row / column -1 reaches the border
    c = UP[UP_NAMES.index('size_at_area')]
    _, area, above = c['sizes']
    assert u('size_at_area', area)[70:, :35].sum() == 255 * area and u('size_at_area', above)[70:, :35].max() == 0
    assert u('size_at_area', above).max() == 255                                       # the larger component stays
    assert u('diagonal_blobs', 700).max() == 255 and u('diagonal_blobs', 1500).max() == 0           # one 4-connected component of 1091
    assert u('blobs_304x416', 0).shape == (1013, 1387)
    for c in UP:                                                                       # no undecided pixel in any stored case
        _, t = ref.mask_up_values(c['mask'], c['scale'])
        assert not (np.abs(t - 1) < 1e-9).any(), c['name']


def test_host_side_of_the_binding():
    assert _lib.rescale_extent((1040, 1392), 0.3) == (312, 418) and _lib.rescale_extent((5, 15), 0.5) == (2, 8)     # half to even
    for n_in, n_out in ((64, 19), (53, 16), (47, 14), (30, 21), (40, 40), (1040, 312)):
        assert np.array_equal(_lib.rescale_weights(n_in, n_out), ref.gaussian_weights(n_in / n_out))
    assert np.array_equal(_lib.rescale_weights(40, 40), [1.0])
    w = _lib.rescale_weights(1040, 52)                                                 # s = 0.05
    assert len(w) // 2 == 38 and abs(w.sum() - 1) < 1e-15


# ---- make stat_fish: scale_ratio with the nuset_weights key --------------------------------------------------------------------
class NusetishHandle(tsf.OracleHandle):
    """Has the names of NuSeT's device calls but not the two rescale calls."""
    nuset_forward = rpn_proposals_last = marker_watershed = clean_nuclei = None


class RescalingHandle(NusetishHandle):
    rescale_down = rescale_mask_up = None


def _weights_file(tmp_path):
    w = nuset.synth_weights(nuset.nuset_config(16, 16, 8), seed=1)
    np.savez(str(tmp_path / 'base8.npz'),
             **{'%s/%s' % (nuset.CHECKPOINT_SCOPE[n], part): a for n, arrs in w.items() for part, a in zip(('kernel', 'bias'), arrs)})
    return str(tmp_path / 'base8.npz')


def _params(tmp_path, monkeypatch, **params):
    (tmp_path / 'src').mkdir(exist_ok=True)
    with open(tmp_path / 'src' / 'stat_fish_params.yaml', 'w') as f:
        f.write(yaml.safe_dump(params).replace("'.nan'", '.nan'))
    monkeypatch.chdir(tmp_path)


def test_scale_ratio_is_accepted_on_a_handle_with_the_calls(tmp_path, monkeypatch):
    """Fails without the feature: ``scale_ratio: 0.3`` was a configuration error on every handle."""
    _params(tmp_path, monkeypatch, scale_ratio=0.3)
    var = dict(nuset_weights=[_weights_file(tmp_path)], nuset_base=8, nuclei_size_T=10)
    assert callable(sf.load_nuset_segmenter(var, RescalingHandle()))
    assert callable(sf.load_nuset_segmenter(var, None))          # main opens the library's own Handle, which has them
    assert hasattr(_lib.Handle, 'rescale_down') and hasattr(_lib.Handle, 'rescale_mask_up')


@pytest.mark.parametrize('value', [0, -0.3, 1.5, float('nan'), float('inf')])
def test_scale_ratio_outside_the_built_range_is_a_configuration_error(tmp_path, monkeypatch, value):
    _params(tmp_path, monkeypatch, scale_ratio=value)
    var = dict(nuset_weights=[_weights_file(tmp_path)], nuset_base=8, nuclei_size_T=10)
    with pytest.raises(sf.ConfigError) as e:
        sf.load_nuset_segmenter(var, RescalingHandle())
    assert 'scale_ratio' in str(e.value)


def test_a_handle_without_the_calls_still_exits_with_code_2(tmp_path, monkeypatch, capsys):
    tsf._folder(tmp_path, nuset_weights=['w.npz'])               # the check comes before the weights are read
    _params(tmp_path, monkeypatch, scale_ratio=0.3)
    with pytest.raises(SystemExit) as e:
        sf.main([], handle=NusetishHandle())
    text = capsys.readouterr().out
    assert e.value.code == 2 and 'scale_ratio' in text and 'rescale' in text
    assert not os.path.exists(tmp_path / 'in' / 'annotated')


def test_segment_refuses_what_is_not_built():
    class NoCalls:
        pass
    net = nuset.NuSeT({}, 8, handle=NoCalls())
    img = np.zeros((64, 64), np.uint8)
    for s in (0, -1, 1.5, float('nan')):
        with pytest.raises(ValueError, match='scale_ratio'):
            net.segment(img, scale_ratio=s)
    with pytest.raises(ValueError, match='16 x 16'):
        net.segment(img, scale_ratio=0.2)                        # 13 x 13
    assert sf.NUSET_DEFAULT_PARAMS['scale_ratio'] == 1


def test_non_uint8_input_is_refused_by_the_binding():
    h = object.__new__(_lib.Handle)                               # no device: the check comes before the library is touched
    for call, args in ((h.rescale_down, (0.5,)), (h.rescale_mask_up, (2.0, 0))):
        with pytest.raises(ValueError, match='uint8'):
            call(np.zeros((32, 32), np.float64), *args)
        with pytest.raises(ValueError):
            call(np.zeros((2, 32, 32), np.uint8), *args)


def test_entry_points_declared_exported_and_built():
    with open(os.path.join(HERE, '..', 'include', 'ecseg_hip.h')) as f:
        header = f.read()
    assert 'int ecseg_rescale_down(ecseg_ctx* h, const uint8_t* img, int H, int W, int out_h, int out_w, const double* wy, int ry' in header
    assert 'int ecseg_rescale_mask_up(ecseg_ctx* h, const uint8_t* cleaned, int H, int W, int out_h, int out_w, int nuclei_size_T' in header
    assert '#define ECSEG_RESCALE_MAX_RADIUS 64' in header
    assert 'ecseg_rescale_down' in _lib.EXPORTS and 'ecseg_rescale_mask_up' in _lib.EXPORTS
    assert 'rescale_kernels.hip' in build.SOURCES and build.EXTRA_FLAGS['rescale_kernels.hip'] == ['-ffp-contract=off']
    if os.path.exists(_lib.LIB_PATH):                            # the unchanged spill test of test_host_cpu.py covers every kernel in it
        blob = open(_lib.LIB_PATH, 'rb').read()
        for name in (b'ecseg_rescale_down', b'ecseg_rescale_mask_up', b'rs_gauss_y_kernel', b'rs_gauss_x_kernel', b'rs_bilinear_kernel',
                     b'rs_threshold_kernel', b'rs_unite_kernel', b'rs_final_kernel'):
            assert name in blob, name
