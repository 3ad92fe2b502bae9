"""ecseg_min_cut (csrc/mincut_kernels.hip), ``binary_seg_to_instance_min_cut`` and ``make stat_fish`` with ``use_min_cut: True`` on the
device.  ``side`` and the max-flow value are compared exactly with the oracle tests/min_cut_ref.py (scipy's maximum flow and a
residual search), never with the product's own Python: the set reachable from the source in the residual network is the same for
every maximum flow, so there is no tolerance and no case is left out.  ``task_mismatches`` is also the check of
tools/fuzz_min_cut.py; a failing seed of that campaign becomes a case here."""
import os
import subprocess
import sys

import numpy as np
import pytest
import yaml

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import min_cut_cases as cases                # noqa: E402
import min_cut_ref as ref                    # noqa: E402
from ecseg_amd import image_io               # noqa: E402
from ecseg_amd import fish_distance_calculation as fdc   # noqa: E402
from ecseg_amd import min_cut as mc          # noqa: E402
from ecseg_amd._lib import EcsegError        # noqa: E402

pytestmark = pytest.mark.gpu
HAND = cases.hand_tasks()
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LDS_PIXELS = 10240                           # ECSEG_MIN_CUT_LDS_PIXELS
_ORACLE = {}


def oracle(key, task):
    """The oracle's answer of a committed task, computed once per session."""
    if key not in _ORACLE:
        _ORACLE[key] = ref.solve_scipy(*task)
    return _ORACLE[key]


def task_mismatches(gpu, tasks, d, want=None):
    """Differences between one device call over ``tasks`` [(M, s, t)] and the oracle -> list of strings."""
    sides, flows = gpu.min_cut(tasks, d)
    want = want or [ref.solve_scipy(M, s, t, d) for M, s, t in tasks]
    bad = []
    for k, ((M, s, t), side, flow, (wside, wflow)) in enumerate(zip(tasks, sides, flows, want)):
        if side.shape != M.shape or side.dtype != np.uint8:
            bad.append('task %d: side is %s %s' % (k, side.shape, side.dtype))
        elif int(flow) != wflow or not np.array_equal(side, wside):
            bad.append('task %d (%s, s %s, t %s, d %d): flow %d, oracle %d; side differs in %d pixel(s)'
                       % (k, M.shape, s, t, d, flow, wflow, int((side != wside).sum())))
    return bad


@pytest.fixture(params=[LDS_PIXELS, 0], ids=['lds', 'global'])
def path(request, gpu):
    """Both homes of the per-pixel state: LDS, and the global scratch region forced onto small windows."""
    gpu.set_option('min_cut_lds_pixels', request.param)
    yield request.param
    gpu.set_option('min_cut_lds_pixels', LDS_PIXELS)


# ---- single tasks ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', sorted(HAND))
def test_hand_tasks(gpu, path, name):
    (M, s, t, d), flow, side = HAND[name]
    want = oracle(name, (M, s, t, d))
    if flow is not None:
        assert want[1] == flow and np.array_equal(want[0], side)
    assert not task_mismatches(gpu, [(M, s, t)], d, [want])


def test_the_cancelled_arc_case_defeats_the_greedy_solver(gpu, path):
    M, s, t, d = cases.CANCEL
    want = oracle('needs_a_cancelled_arc', cases.CANCEL)
    assert ref.solve_greedy(M, s, t, d) < want[1]
    sides, flows = gpu.min_cut([(M, s, t)], d)
    assert int(flows[0]) == want[1] == 4 and np.array_equal(sides[0], want[0])


@pytest.mark.parametrize('d', [1, 5, 32])
def test_distances_and_border_pixels(gpu, path, d):
    """Source and sink on the window border (corners included), on a full 41 x 67 window (w no multiple of 64) and on a dumbbell."""
    full = np.ones((41, 67), np.uint8)
    M, left, right = cases.dumbbell(29, 3, 7)
    tasks = [(full, (0, 0), (40, 66)), (full, (40, 0), (20, 66)), (full, (20, 33), (0, 33)), (M, (0, 0), (28, 64)), (M, left, right),
             (M, right, (14, 0))]
    want = [oracle(('border', d, k), task + (d,)) for k, task in enumerate(tasks)]
    assert not task_mismatches(gpu, tasks, d, want)


def test_random_blob_tasks(gpu, path):
    """40 seeded windows of at most 96 x 96 (discs, dense noise, windows with holes), grouped by distance: one call per distance."""
    groups = {}
    for seed in range(40):
        M, s, t, d = cases.random_task(seed)
        groups.setdefault(d, []).append((seed, (M, s, t)))
    assert len(groups) >= 5
    total = 0
    for d, members in sorted(groups.items()):
        tasks = [m[1] for m in members]
        want = [oracle(('blob', seed), task + (d,)) for seed, task in members]
        total += sum(w[1] for w in want)
        assert not task_mismatches(gpu, tasks, d, want), 'seeds %s' % [m[0] for m in members]
    assert total > 300                                       # not vacuous


def test_batches_on_both_sides_of_the_lds_threshold(gpu):
    """100 x 102 = 10200 pixels stay in LDS, 100 x 103 = 10300 do not; both orders in one call each, and the empty batch."""
    assert 100 * 102 <= LDS_PIXELS < 100 * 103
    rng = np.random.default_rng(5)
    small = (rng.random((100, 102)) < 0.8).astype(np.uint8)
    large = (rng.random((100, 103)) < 0.8).astype(np.uint8)
    small[[10, 90], [10, 90]] = 1
    large[[10, 90], [10, 90]] = 1
    M, left, right = cases.dumbbell()
    tasks = [(small, (10, 10), (90, 90)), (large, (10, 10), (90, 90)), (M, left, right), (large, (90, 90), (10, 10)), (small, (90, 90), (10, 10))]
    want = [oracle(('mixed', k), task + (5,)) for k, task in enumerate(tasks)]
    assert min(w[1] for w in want) > 0
    assert not task_mismatches(gpu, tasks, 5, want)
    assert not task_mismatches(gpu, tasks[::-1], 5, want[::-1])
    sides, flows = gpu.min_cut([], 5)
    assert sides == [] and flows.shape == (0,)


def test_repeats_are_byte_identical(gpu, path):
    tasks = [cases.random_task(seed)[:3] for seed in (0, 7, 9, 30)]
    first = gpu.min_cut(tasks, 5)
    for _ in range(3):
        again = gpu.min_cut(tasks, 5)
        assert np.array_equal(first[1], again[1]) and all(a.tobytes() == b.tobytes() for a, b in zip(first[0], again[0]))
    assert 0 < gpu.timings()['count'] < 1000


def test_bad_arguments(gpu):
    M, left, right = cases.dumbbell()
    good = [(M, left, right)]
    for tasks, d, text in (([(M, left, left)], 5, 'same pixel'), ([(M, (0, 30), right)], 5, 'zero pixel'), ([(M, left, (0, 30))], 5, 'zero pixel'),
                           ([(M, (29, 0), right)], 5, 'outside'), ([(M, left, (0, -1))], 5, 'outside'), (good, 0, 'dist'), (good, 33, 'dist'),
                           (good + [(M, left, left)], 5, 'task 1')):
        with pytest.raises(EcsegError) as e:
            gpu.min_cut(tasks, d)
        assert e.value.code == -1 and text in str(e.value)
        assert not task_mismatches(gpu, good, 5, [oracle('dumbbell_from_the_left', (M, left, right, 5))])     # the handle goes on
    with pytest.raises(EcsegError, match='unknown option or bad value'):
        gpu.set_option('min_cut_lds_pixels', LDS_PIXELS + 1)
    # overlapping windows, straight through the C interface
    import ctypes as C
    desc = np.zeros((2, 8), np.int32)
    desc[0, :7] = (0, 1, 4, 0, 0, 0, 3)
    desc[1, :7] = (2, 1, 4, 0, 0, 0, 3)
    buf, side, flow = np.ones(8, np.uint8), np.zeros(8, np.uint8), np.zeros(2, np.int32)
    rc = gpu.lib.ecseg_min_cut(gpu.h, buf.ctypes.data_as(C.c_void_p), 8, desc.ctypes.data_as(C.c_void_p), 2, 1,
                               side.ctypes.data_as(C.c_void_p), flow.ctypes.data_as(C.c_void_p))
    assert rc == -1 and b'overlaps' in gpu.lib.ecseg_last_error(gpu.h)


# ---- the whole function ------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def scene_answer():
    trace = []
    mask = cases.scene()
    labels, vis = ref.instance_min_cut(mask, 60, 1.25, trace=trace)
    return mask, labels, vis, trace


def test_whole_function_on_the_disc_scene(gpu, path, scene_answer):
    """Five single discs, a clump of two and a clump of three: 7 regions become 10 cells, and the clump of three is cut a second time
    inside one side of its first cut (recursion level 2, ``trace`` holds level - 1)."""
    mask, want, want_vis, trace = scene_answer
    assert mask.shape == (160, 224) and want.max() == 10 and sorted(trace) == [0, 0, 1]
    stats = {}
    labels, vis = mc.binary_seg_to_instance_min_cut(mask, 60, 1.25, handle=gpu, stats=stats)
    assert labels.dtype == np.int32 and np.array_equal(labels, want)
    assert vis.dtype == np.uint8 and np.array_equal(vis, want_vis)
    assert stats['calls'] == 2 and stats['tasks'] == 3 and stats['kernel_ms'] > 0      # one call per recursion level


def test_make_stat_fish_with_min_cut_then_fish_distances(tmp_path, monkeypatch, scene_answer):
    mask, want, want_vis, _ = scene_answer
    inp = tmp_path / 'in'
    (inp / 'nuclei_masks').mkdir(parents=True)
    rng = np.random.default_rng(3)
    img = rng.integers(0, 40, mask.shape + (3,), dtype=np.uint8)
    for cy, cx, _ in cases.SCENE_DISCS:                      # a green and a red spot in every disc
        img[cy - 3:cy, cx - 3:cx, 1] = 200
        img[cy + 1:cy + 4, cx + 1:cx + 4, 0] = 220
    image_io.write_tiff_rgb8(str(inp / 'clumps.tif'), img)
    image_io.write_tiff_gray8(str(inp / 'nuclei_masks' / 'clumps.tif'), mask)
    cfg = yaml.safe_load(open(os.path.join(ROOT, 'config.yaml')))
    assert cfg['stat_fish']['use_min_cut'] is False          # the shipped default
    cfg['stat_fish'].update(inpath=str(inp), use_min_cut=True, scale=1)
    cfg['fish_distance_calculation'].update(inpath=str(inp))
    yaml.safe_dump(cfg, open(tmp_path / 'config.yaml', 'w'))
    os.symlink(os.path.join(ROOT, 'src'), tmp_path / 'src')
    os.symlink(os.path.join(ROOT, 'ecseg_amd'), tmp_path / 'ecseg_amd')
    out = subprocess.run(['make', '-f', os.path.join(ROOT, 'Makefile'), 'stat_fish'], cwd=tmp_path, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout + out.stderr
    d = inp / 'annotated' / 'clumps'
    assert len(os.listdir(d)) == 6
    saved = np.load(d / 'clumps__segmentation_min_cut.npy')
    assert saved.dtype == np.int64 and np.array_equal(saved, want)
    assert np.array_equal(image_io.imread(str(d / 'clumps_segmentation_corrected_min_cut.tif')), want_vis[..., ::-1])
    rows = open(inp / 'annotated' / 'stat_fish_lsq.csv').read().strip().split('\n')
    assert len(rows) == 1 + 10                               # one row per cell of the split label map
    monkeypatch.chdir(tmp_path)
    try:
        fdc.main([])
        code = 0
    except SystemExit as e:
        code = e.code
    assert code in (0, None), code
    assert len(open(inp / 'centromere_distances.csv').read().strip().split('\n')) > 1
