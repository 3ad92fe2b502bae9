"""ecseg_min_cut_regions on the device against tests/min_cut_ref.py (through tests/min_cut_region_cases.py): labels, counts, region and
centre records, windows and components, exactly, with the per-crop state in LDS and in global memory; the capacity protocol, the
refusals, and the whole splitter and ``make stat_fish`` with ``min_cut_regions_on_device`` on and off."""
import filecmp
import os
import subprocess
import sys

import numpy as np
import pytest
import yaml

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import min_cut_cases as cases                # noqa: E402
import min_cut_ref as ref                    # noqa: E402
import min_cut_region_cases as rc            # noqa: E402
from ecseg_amd import image_io               # noqa: E402
from ecseg_amd import min_cut as mc          # noqa: E402
from ecseg_amd._lib import EcsegError        # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HAND = rc.hand_cases()
LDS_PIXELS = 8192                            # ECSEG_MIN_CUT_CENTERS_LDS_PIXELS


@pytest.fixture(params=[LDS_PIXELS, 0], ids=['lds', 'global'])
def path(request, gpu):
    """Both homes of the per-pixel state: LDS, and the crop's own part of ``comp`` forced onto small crops."""
    gpu.set_option('min_cut_centers_lds_pixels', request.param)
    yield request.param
    gpu.set_option('min_cut_centers_lds_pixels', LDS_PIXELS)


def mismatches(gpu, case, want):
    """Differences between one device call and the oracle -> list of strings."""
    mask, coeff, min_rad = case
    labels, regions, centers, windows, comp = gpu.min_cut_regions(mask, coeff, min_rad)
    bad = []
    if labels.dtype != np.int32 or not np.array_equal(labels, want['labels']):
        bad.append('labels differ')
    if int(labels.max(initial=0)) != want['n_cells']:
        bad.append('n_cells %d, oracle %d' % (labels.max(initial=0), want['n_cells']))
    if not np.array_equal(regions, want['regions']):
        bad.append('regions %s, oracle %s' % (regions.tolist()[:4], want['regions'].tolist()[:4]))
    if not np.array_equal(centers, want['centers']):
        bad.append('centers %s, oracle %s' % (centers.tolist()[:4], want['centers'].tolist()[:4]))
    if len(windows) != len(want['windows']) or not all(a.dtype == np.uint8 and np.array_equal(a, b) for a, b in zip(windows, want['windows'])):
        bad.append('windows differ')
    if len(comp) != len(want['comp']) or not all(a.dtype == np.int32 and np.array_equal(a, b) for a, b in zip(comp, want['comp'])):
        bad.append('comp differs')
    return bad


@pytest.mark.parametrize('name', sorted(HAND))
def test_hand_cases(gpu, path, name):
    assert mismatches(gpu, HAND[name], rc.expected_of('hand', name)) == []
    mask, coeff, min_rad = HAND[name]
    raw = gpu.min_cut_regions_raw(mask, coeff, min_rad, 64, 512, 1 << 16)
    assert raw[1][0] == rc.expected_of('hand', name)['n_cells']                 # *n_cells as the call wrote it


def test_seeded_scenes(gpu, path):
    bad = {}
    for seed in rc.SEEDS:
        got = mismatches(gpu, rc.seeded_case(seed), rc.expected_of('seed', seed))
        if got:
            bad[seed] = got
    assert bad == {}


def test_one_300x300_region_runs_in_global_memory(gpu):
    case, want = rc.big_region(), rc.expected_of('big')
    assert want['regions'][0, 3] * want['regions'][0, 4] == 90000 > LDS_PIXELS and len(want['centers']) >= 2
    assert mismatches(gpu, case, want) == []


@pytest.mark.parametrize('short', ['regions', 'centers', 'windows'])
def test_a_capacity_one_short_writes_the_counts_alone(gpu, short):
    mask, coeff, min_rad = HAND['two_rings_two_draws']
    want = rc.expected_of('hand', 'two_rings_two_draws')
    n_reg, n_cen, wpx = len(want['regions']), len(want['centers']), sum(w.size for w in want['windows'])
    caps = [n_reg, n_cen, wpx]
    caps[['regions', 'centers', 'windows'].index(short)] -= 1
    labels, counts, regions, centers, windows, comp = gpu.min_cut_regions_raw(mask, coeff, min_rad, *caps)
    assert counts == (want['n_cells'], n_reg, n_cen, wpx) and np.array_equal(labels, want['labels'])
    assert (regions == -1).all() and (centers == -1).all() and (windows == 255).all() and (comp == -1).all()     # untouched
    labels, counts, regions, centers, windows, comp = gpu.min_cut_regions_raw(mask, coeff, min_rad, n_reg, n_cen, wpx)
    assert counts == (want['n_cells'], n_reg, n_cen, wpx) and np.array_equal(labels, want['labels'])
    assert np.array_equal(regions, want['regions']) and np.array_equal(centers, want['centers'])
    assert np.array_equal(windows, np.concatenate([w.reshape(-1) for w in want['windows']]))
    assert np.array_equal(comp, np.concatenate([c.reshape(-1) for c in want['comp']]))


def test_bad_arguments_are_refused(gpu):
    import ctypes as C
    mask = HAND['n_1_selected'][0]
    for coeff, min_rad in ((float('nan'), 1), (float('inf'), 1), (-float('inf'), 1), (1.25, -1)):
        with pytest.raises(EcsegError) as e:
            gpu.min_cut_regions(mask, coeff, min_rad)
        assert e.value.code == -1
    lab = np.zeros(mask.shape, np.int32)
    out = np.zeros(4, np.int32)
    wpx = C.c_longlong(0)
    p = lambda a: a.ctypes.data_as(C.c_void_p)               # noqa: E731
    call = gpu.lib.ecseg_min_cut_regions
    good = [gpu.h, p(mask), mask.shape[0], mask.shape[1], 0.5, 1, 0, 0, 0, p(lab), p(out[0:]), None, p(out[1:]), None, p(out[2:]), None, None, C.byref(wpx)]
    assert call(*good) == 0 and out[:3].tolist() == [1, 1, 1] and wpx.value == 36       # capacities of 0: the counts alone
    for at, value in ((1, None), (9, None), (10, None), (12, None), (14, None), (17, None), (2, 0), (3, 0), (6, -1), (7, -1), (8, -1),
                      (2, 1 << 16)):                         # null pointers; H, W < 1; negative capacities; H * W = 2^31
        args = list(good)
        args[at] = value
        if at == 2 and value == 1 << 16:
            args[3] = 1 << 15
        assert call(*args) == -1, at
    for at in (6, 7, 8):                                     # a capacity above 0 with a null buffer
        args = list(good)
        args[at] = 1
        assert call(*args) == -1, at


def test_two_calls_give_identical_bytes(gpu, path):
    for case in (HAND['more_than_255_components'], rc.seeded_case(1003), (rc.ring_scene(), 0.5, 10)):
        a = gpu.min_cut_regions_raw(*case, 64, 1024, 1 << 16)
        b = gpu.min_cut_regions_raw(*case, 64, 1024, 1 << 16)
        assert a[1] == b[1] and a[1][1] > 0 and all(x.tobytes() == y.tobytes() for x, y in zip((a[0],) + a[2:], (b[0],) + b[2:]))


@pytest.mark.parametrize('scene,coeff', [('discs', 1.25), ('rings', 0.5)])
def test_whole_function_with_the_key_on(gpu, path, scene, coeff):
    mask = cases.scene() if scene == 'discs' else rc.ring_scene()
    want, want_vis = ref.instance_min_cut(mask, 60, coeff)
    assert want.max() == (10 if scene == 'discs' else 4)
    off, off_vis = mc.binary_seg_to_instance_min_cut(mask, 60, coeff, handle=gpu)
    stats = {}
    on, on_vis = mc.binary_seg_to_instance_min_cut(mask, 60, coeff, handle=gpu, stats=stats, regions_on_device=True)
    assert on.dtype == np.int32 and np.array_equal(on, want) and np.array_equal(on, off)
    assert np.array_equal(on_vis, want_vis) and np.array_equal(on_vis, off_vis)
    assert stats['regions'] == 2 and stats['centers'] > 0 and stats['tasks'] == (3 if scene == 'discs' else 2)


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
    return len(cmp.common_files) + len(cmp.common_dirs)


@pytest.mark.parametrize('batch', [1, 2])
def test_make_stat_fish_writes_the_same_files_with_the_key_on(tmp_path, batch):
    outs = []
    for key in (False, True):
        top = tmp_path / ('on' if key else 'off')
        inp = top / 'in'
        (inp / 'nuclei_masks').mkdir(parents=True)
        for name, mask in (('clumps', cases.scene()), ('rings', rc.ring_scene())):
            rng = np.random.default_rng(3)
            img = rng.integers(0, 40, mask.shape + (3,), dtype=np.uint8)
            img[5:8, 5:8, 1] = 200
            image_io.write_tiff_rgb8(str(inp / (name + '.tif')), img)
            image_io.write_tiff_gray8(str(inp / 'nuclei_masks' / (name + '.tif')), mask)
        cfg = yaml.safe_load(open(os.path.join(ROOT, 'config.yaml')))
        assert cfg['stat_fish']['min_cut_regions_on_device'] is False            # the shipped default
        cfg['stat_fish'].update(inpath='in', use_min_cut=True, scale=1, min_cut_regions_on_device=key)
        if batch > 1:
            cfg['stat_fish'].update(batch=batch, tiff_on_device=True)
        yaml.safe_dump(cfg, open(top / 'config.yaml', 'w'))
        os.symlink(os.path.join(ROOT, 'src'), top / 'src')
        os.symlink(os.path.join(ROOT, 'ecseg_amd'), top / 'ecseg_amd')
        out = subprocess.run(['make', '-f', os.path.join(ROOT, 'Makefile'), 'stat_fish'], cwd=top, capture_output=True, text=True, timeout=600)
        assert out.returncode == 0, out.stdout + out.stderr
        outs.append(out.stdout.replace(str(top), '<top>'))
    assert outs[0] == outs[1]                                # the messages
    assert _same_tree(str(tmp_path / 'off' / 'in' / 'annotated'), str(tmp_path / 'on' / 'in' / 'annotated')) >= 3
    assert len(os.listdir(tmp_path / 'on' / 'in' / 'annotated' / 'rings')) == 6
