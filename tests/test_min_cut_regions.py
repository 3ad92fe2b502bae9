"""``min_cut_regions_on_device`` without a GPU: the hand cases of tests/min_cut_region_cases.py take the branches they are named for and
the seeded scenes give the mix the device tests need (decided with tests/min_cut_ref.py alone); the host side of the key -
``binary_seg_to_instance_min_cut(regions_on_device=True)``, ``main`` and its configuration errors - on a handle whose
``min_cut_regions`` is computed by the oracle; the layout header under ASan + UBSan (``make asan_min_cut_regions``); the export."""
import ctypes
import filecmp
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest
import yaml

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import min_cut_cases as cases                # noqa: E402
import min_cut_ref as ref                    # noqa: E402
import min_cut_region_cases as rc            # noqa: E402
import stat_fish_ref as sf_ref               # noqa: E402
from ecseg_amd import _lib, image_io         # noqa: E402
from ecseg_amd import min_cut as mc          # noqa: E402
from ecseg_amd import stat_fish as sf        # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HAND = rc.hand_cases()


def want(name):
    return rc.expected_of('hand', name)


def distance(name, region=0):
    return ref.l1_distance(want(name)['windows'][region])


# ---- the hand cases take their branches ----------------------------------------------------------------------------------------------
def test_selection_cases():
    areas = lambda name: np.bincount(want(name)['labels'].reshape(-1))[1:].tolist()      # noqa: E731
    assert areas('areas_4_4_5_nothing_selected') == [4, 4, 5] and len(want('areas_4_4_5_nothing_selected')['regions']) == 0
    assert areas('areas_4_4_6_one_selected') == [4, 4, 6] and want('areas_4_4_6_one_selected')['regions'][:, 0].tolist() == [3]
    even = areas('even_n_median_is_a_mean')
    assert len(even) % 2 == 0 and np.median(even) not in even and want('even_n_median_is_a_mean')['regions'][:, 0].tolist() == [4]
    assert want('n_1_not_selected')['n_cells'] == 1 and len(want('n_1_not_selected')['regions']) == 0
    assert want('n_1_selected')['n_cells'] == 1 and len(want('n_1_selected')['regions']) == 1
    e = want('empty_mask')
    assert e['n_cells'] == 0 and len(e['regions']) == 0 and not e['labels'].any()


def test_shape_cases():
    e = want('fills_its_box')
    assert e['windows'][0].all() and (distance('fills_its_box') == 1 << 30).all() and e['regions'][0, 7] == 1     # FAR everywhere, one centre
    assert e['centers'][0, 4] == 10 * 10                     # every interior pixel is a centre pixel
    assert want('box_with_h_below_3')['regions'][0, 3:5].tolist() == [2, 20] and want('box_with_h_below_3')['regions'][0, 7] == 0
    assert want('box_with_w_below_3')['regions'][0, 3:5].tolist() == [20, 2] and want('box_with_w_below_3')['regions'][0, 7] == 0
    e = want('meets_all_four_borders')
    assert e['regions'][0, 1:5].tolist() == [0, 0, 17, 17] == [0, 0] + list(HAND['meets_all_four_borders'][0].shape) and not e['windows'][0].all()
    e = want('diagonal_touch')
    assert e['n_cells'] == 4 and e['regions'][:, 0].tolist() == [3, 4]
    assert ref.ndimage.label(HAND['diagonal_touch'][0], structure=ref.EIGHT)[1] == 3     # 8-connectivity would join the two squares
    e = want('l_shaped_neighbour_in_the_box')
    k, r0, c0, h, w = e['regions'][0, :5].tolist()
    inside = set(np.unique(e['labels'][r0:r0 + h, c0:c0 + w]).tolist())
    assert inside == {0, k, k + 1} and not e['windows'][0][e['labels'][r0:r0 + h, c0:c0 + w] == k + 1].any()      # foreign pixels are zero pixels


def test_centre_cases():
    e = want('dumbbell_min_rad_10')
    assert e['regions'][0, 7] == 2 and e['centers'][:, 3].tolist() == [1, 1]
    # the bar's ridge is a plateau: neighbouring candidates of equal distance, which strict tests would all reject
    d = distance('bar_9x15_plateau_ridge')
    comp = want('bar_9x15_plateau_ridge')['comp'][0]
    ys, xs = np.nonzero(comp)
    assert len(ys) > 1 and len(set(d[ys, xs].tolist())) == 1 and (np.diff(xs[ys == ys[0]]) == 1).all()
    for name, rows, row in (('two_pixel_component_rounds_up', [3, 4], 4), ('two_pixel_component_rounds_down', [4, 5], 4)):
        e = want(name)
        ys, xs = np.nonzero(e['comp'][0])
        assert ys.tolist() == rows and len(set(xs.tolist())) == 1 and e['centers'][0, 1] == row and e['centers'][0, 4] == 2
    e = want('2x2_component_half_on_both_axes')
    ys, xs = np.nonzero(e['comp'][0])
    assert sorted(set(ys.tolist())) == [3, 4] and sorted(set(xs.tolist())) == [4, 5] and e['centers'][0, [1, 2, 4]].tolist() == [4, 4, 4]
    for name, n in (('ring_centroid_in_the_hole', 1), ('two_rings_two_draws', 2)):
        e = want(name)
        assert len(e['regions']) == n and e['centers'][:, 3].tolist() == [0] * n and e['centers'][:, 1:3].tolist() == [[10, 10]] * n
        assert all(w[10, 10] == 0 for w in e['windows'])
    assert want('more_than_255_components')['regions'][0, 7] > 255


def test_the_seeded_scenes_give_the_mix():
    two = off = far = 0
    for seed in rc.SEEDS:
        mask, coeff, min_rad = rc.seeded_case(seed)
        assert max(mask.shape) <= 96 and min_rad in (1, 2, 3, 10) and coeff in (0.5, 1.25)
        e = rc.expected_of('seed', seed)
        two += bool((e['regions'][:, 7] >= 2).any())
        off += bool((e['centers'][:, 3] == 0).any())
        far += any(w.all() for w in e['windows'])
    assert len(rc.SEEDS) == 200 and two >= 50 and off >= 5 and far >= 5, (two, off, far)


# ---- the host side of the key ----------------------------------------------------------------------------------------------------------
class RegionsHandle(ref.OracleSolverHandle):
    """``min_cut_regions`` of a ``_lib.Handle`` from the oracle, beside the oracle's ``ccl_labels``, ``min_cut`` and ``fish_spots``."""
    region_calls = 0

    def min_cut_regions(self, mask, coeff, min_rad=10):
        self.region_calls += 1
        e = rc.expected(mask, coeff, min_rad)
        return e['labels'], e['regions'], e['centers'], e['windows'], e['comp']

    def fish_spots(self, labels, img, probes, weights, normal, ithr, min_cc, line, capacity=4096):
        rec, thr, bnd, _ = sf_ref.loop(img, labels, probes, np.asarray(weights, np.float64), normal, ithr, min_cc, line)
        return rec, thr, bnd


class NoRegionsHandle(ref.OracleSolverHandle):
    fish_spots = RegionsHandle.fish_spots


@pytest.mark.parametrize('scene,coeff,cells', [('discs', 1.25, 10), ('rings', 0.5, 4), ('two_rings', 0.5, 2)])
def test_whole_function_with_the_key_on(scene, coeff, cells):
    mask = {'discs': cases.scene, 'rings': rc.ring_scene, 'two_rings': lambda: HAND['two_rings_two_draws'][0]}[scene]()
    want_labels, want_vis = ref.instance_min_cut(mask, 60, coeff)
    assert want_labels.max() == cells
    h = RegionsHandle()
    off, off_vis = mc.binary_seg_to_instance_min_cut(mask, 60, coeff, handle=h)
    stats = {}
    on, on_vis = mc.binary_seg_to_instance_min_cut(mask, 60, coeff, handle=h, stats=stats, regions_on_device=True)
    assert h.region_calls == 1 and on.dtype == np.int32
    assert np.array_equal(on, want_labels) and np.array_equal(on, off) and np.array_equal(on_vis, want_vis) and np.array_equal(on_vis, off_vis)
    assert set(stats) >= {'centers', 'regions'} and stats['regions'] == (0 if scene == 'two_rings' else 2)
    empty, vis = mc.binary_seg_to_instance_min_cut(np.zeros((5, 6), np.uint8), 60, 1.25, handle=h, regions_on_device=True)
    assert not empty.any() and not vis.any()


def test_the_draws_come_in_the_reference_order():
    """Both rings of the ring scene draw a pixel: the device path must hand region 1 the first draw."""
    mask = rc.ring_scene()
    rng_a, rng_b = np.random.RandomState(1), np.random.RandomState(1)
    lab, found = mc.device_regions(RegionsHandle(), mask, 0.5, rng_a)
    assert len(found) == 2
    for k, box, win, centers in found:
        assert centers == ref.centres(np.asarray(win), rng_b, 10) and win[centers[0]] and win[centers[1]]
    assert rng_a.randint(1 << 30) == rng_b.randint(1 << 30)   # the same number of draws was taken


def _folder(top, **section):
    inp = top / 'in'
    (inp / 'nuclei_masks').mkdir(parents=True)
    for name, mask in (('clumps', cases.scene()), ('rings', rc.ring_scene())):
        rng = np.random.default_rng(3)
        img = rng.integers(0, 40, mask.shape + (3,), dtype=np.uint8)
        img[5:8, 5:8, 1] = 200
        image_io.write_tiff_rgb8(str(inp / (name + '.tif')), img)
        image_io.write_tiff_gray8(str(inp / 'nuclei_masks' / (name + '.tif')), mask)
    cfg = dict(inpath='in', scale=1, use_min_cut=True, nuclei_size_T=5000)
    cfg.update(section)
    yaml.safe_dump({'stat_fish': cfg}, open(top / 'config.yaml', 'w'))
    return inp


def _same_tree(a, b):
    cmp = filecmp.dircmp(a, b)
    assert not cmp.left_only and not cmp.right_only and not cmp.funny_files
    for name in cmp.common_files:
        one, two = open(os.path.join(a, name), 'rb').read(), open(os.path.join(b, name), 'rb').read()
        if name.endswith('.yaml') and b'min_cut_regions_on_device' in one:      # the echo of the configuration: it names the key's value
            one, two = (t.replace(b'min_cut_regions_on_device: true', b'min_cut_regions_on_device: false') for t in (one, two))
        assert one == two, name
    for sub in cmp.common_dirs:
        _same_tree(os.path.join(a, sub), os.path.join(b, sub))


def test_main_writes_the_same_files_with_the_key_on(tmp_path, monkeypatch, capsys):
    said = []
    for key in (False, True):
        top = tmp_path / ('on' if key else 'off')
        top.mkdir()
        _folder(top, min_cut_regions_on_device=key)
        monkeypatch.chdir(top)
        h = RegionsHandle()
        sf.main([], handle=h)
        assert h.region_calls == (2 if key else 0)
        said.append(capsys.readouterr().out)
    assert said[0] == said[1]
    _same_tree(str(tmp_path / 'off' / 'in' / 'annotated'), str(tmp_path / 'on' / 'in' / 'annotated'))
    assert len(os.listdir(tmp_path / 'on' / 'in' / 'annotated' / 'rings')) == 6
    assert open(tmp_path / 'on' / 'in' / 'annotated' / 'stat_fish_lsq.csv').read().count('\n') == 1 + 10 + int(ref.instance_min_cut(rc.ring_scene(), 60, 1.25)[0].max())


@pytest.mark.parametrize('value,handle', [('yes please', RegionsHandle), (1, RegionsHandle), (0, RegionsHandle), (True, NoRegionsHandle)])
def test_the_keys_configuration_errors(tmp_path, monkeypatch, capsys, value, handle):
    inp = _folder(tmp_path, min_cut_regions_on_device=value)
    monkeypatch.chdir(tmp_path)
    with pytest.raises(SystemExit) as e:
        sf.main([], handle=handle())
    assert e.value.code == 2 and 'min_cut_regions_on_device' in capsys.readouterr().out
    assert not os.path.exists(inp / 'annotated')


def test_the_key_is_ignored_without_the_splitter(tmp_path, monkeypatch):
    _folder(tmp_path, min_cut_regions_on_device=True, use_min_cut=False)
    monkeypatch.chdir(tmp_path)
    h = NoRegionsHandle()                                    # no min_cut_regions, and none is needed
    sf.main([], handle=h)
    assert len(os.listdir(tmp_path / 'in' / 'annotated' / 'rings')) == 5     # no min-cut picture


# ---- header, export, layout ------------------------------------------------------------------------------------------------------------
def test_header_export_and_defaults():
    header = open(os.path.join(ROOT, 'include', 'ecseg_hip.h')).read()
    assert 'int ecseg_min_cut_regions(ecseg_ctx* h, const uint8_t* mask, int H, int W, double coeff, int min_rad, int region_capacity,' in header
    assert '#define ECSEG_MIN_CUT_CENTERS_LDS_PIXELS 8192' in header and '"min_cut_centers_lds_pixels"' in header
    assert 'ecseg_min_cut_regions' in _lib.EXPORTS and hasattr(_lib.Handle, 'min_cut_regions')
    assert ctypes.CDLL(_lib.LIB_PATH).ecseg_min_cut_regions  # the built library exports it
    assert yaml.safe_load(open(os.path.join(ROOT, 'config.yaml')))['stat_fish']['min_cut_regions_on_device'] is False
    import ecseg_amd.build as build
    assert 'mincut_centers_kernels.hip' in build.SOURCES
    import inspect
    assert inspect.signature(mc.binary_seg_to_instance_min_cut).parameters['regions_on_device'].default is False


def test_make_asan_min_cut_regions_builds_and_runs_clean(tmp_path):
    if not shutil.which('g++') or not shutil.which('make'):
        pytest.skip('no host toolchain')
    exe = str(tmp_path / 'min_cut_regions_check')
    out = subprocess.run(['make', '-C', ROOT, 'asan_min_cut_regions', 'MIN_CUT_REGIONS_CHECK=' + exe], capture_output=True, text=True, timeout=900)
    if 'cannot find' in out.stderr and 'asan' in out.stderr:
        pytest.skip('libasan not installed')
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-3000:]
    assert 'min_cut_regions_check: ok' in out.stdout
    mk = open(os.path.join(ROOT, 'Makefile')).read()
    assert 'asan_min_cut_regions:' in mk and '-fsanitize=address,undefined' in mk.split('asan_min_cut_regions:')[1]
