"""The min-cut nucleus splitter without a GPU: the oracle (tests/min_cut_ref.py) pinned on hand-computed answers, its two solvers
against each other on every committed task, the host side of ecseg_amd/min_cut.py (centres, recursion, relabelling, colours) on
hand shapes and against the restatement, and ``make stat_fish`` with ``use_min_cut: True`` on an oracle-backed handle."""
import os
import sys

import numpy as np
import pytest
import yaml

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import min_cut_cases as cases                # noqa: E402
import min_cut_ref as ref                    # noqa: E402
import stat_fish_ref as sf_ref               # noqa: E402
from ecseg_amd import _lib, csvio, image_io  # noqa: E402
from ecseg_amd import min_cut as mc          # noqa: E402
from ecseg_amd import stat_fish as sf        # noqa: E402

HAND = cases.hand_tasks()
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the oracle -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', sorted(HAND))
def test_hand_tasks_on_both_solvers(name):
    task, flow, side = HAND[name]
    a, b = ref.solve_scipy(*task), ref.solve_paths(*task)
    assert a[1] == b[1] and np.array_equal(a[0], b[0])
    if flow is not None:
        assert a[1] == flow and np.array_equal(a[0], side)
    assert a[0][task[1]] == 1 and a[0][task[2]] == 0 and not a[0][np.asarray(task[0]) == 0].any()


def test_the_cancelled_arc_case():
    M, s, t, d = cases.CANCEL
    assert ref.solve_greedy(M, s, t, d) == 3 and ref.solve_scipy(M, s, t, d)[1] == 4 and ref.solve_paths(M, s, t, d)[1] == 4


def test_both_solvers_agree_on_the_committed_random_tasks():
    flows, need_cancel = 0, 0
    for seed in range(40):
        task = cases.random_task(seed)
        assert max(task[0].shape) <= 96
        a, b = ref.solve_scipy(*task), ref.solve_paths(*task)
        assert a[1] == b[1] and np.array_equal(a[0], b[0]), seed
        flows += a[1]
        need_cancel += ref.solve_greedy(*task) < a[1]
    assert flows > 300 and need_cancel >= 10                 # not vacuous


def test_network_by_hand():
    # 1 x 3, d = 1: the middle pixel is in the source's ball (one arc from s, none to t by the ball: `elif`), has the grid arcs to both
    assert sorted(ref.arcs(np.ones((1, 3)), (0, 0), (0, 2), 1)) == [(0, 1), (1, 0), (1, 2)]
    # next to t, outside the source's ball: two parallel arcs into t
    assert sorted(ref.arcs(np.ones((1, 4)), (0, 0), (0, 3), 1)).count((2, 3)) == 2


# ---- centres ----------------------------------------------------------------------------------------------------------------------
def test_flow_distance():
    assert mc.flow_distance(60) == 5 and mc.flow_distance(4) == 1 and mc.flow_distance(2243) == 32
    with pytest.raises(ValueError):
        mc.flow_distance(3)


def test_city_block_distance():
    m = np.ones((5, 7), np.uint8)
    m[0, 0] = 0
    yy, xx = np.mgrid[:5, :7]
    assert np.array_equal(mc.city_block_distance(m), yy + xx)
    assert (mc.city_block_distance(np.ones((4, 4))) == mc.FAR).all()
    rng = np.random.default_rng(0)
    m = (rng.random((23, 31)) < 0.9).astype(np.uint8)
    assert np.array_equal(mc.city_block_distance(m), ref.l1_distance(m))


def test_centroids_round_half_to_even():
    mask = np.ones((8, 12), np.uint8)
    cc = np.zeros((8, 12), np.uint8)
    cc[2:4, 4:6] = 1                                         # mean (2.5, 4.5) -> (2, 4)
    cc[3:5, 8] = 1                                           # mean (3.5, 8) -> (4, 8)
    cc[6, 0:2] = 1                                           # mean (6, 0.5) -> (6, 0)
    cc[6:8, 10:12] = 1; cc[7, 11] = 0                        # mean (19 / 3, 31 / 3) -> (6, 10)
    got = mc.binary_img_to_centers(mask, cc, np.random.RandomState(1))
    assert got == [(2, 4), (4, 8), (6, 0), (6, 10)]          # raster order of the first pixels
    assert all(isinstance(v, int) for c in got for v in c)


def test_off_mask_centroid_takes_the_seeded_alternative():
    mask = np.ones((9, 20), np.uint8)
    mask[2, 2] = 0
    mask[5, 12] = 0
    cc = np.zeros((9, 20), np.uint8)
    cc[1:4, 1:4] = 1; cc[2, 2] = 0                           # a ring around the hole at (2, 2): the centroid is off the mask
    cc[4, 17] = 1                                            # an ordinary one in between (first pixel (4, 17))
    cc[4:7, 11:14] = 1; cc[5, 12] = 0                        # a second ring around (5, 12) (first pixel (4, 11): before (4, 17))
    ring1 = [(1, 1), (1, 2), (1, 3), (2, 1), (2, 3), (3, 1), (3, 2), (3, 3)]
    ring2 = [(y + 3, x + 10) for y, x in ring1]
    draws = np.random.RandomState(1)
    want = [ring1[draws.randint(8)], ring2[draws.randint(8)], (4, 17)]      # one generator, one draw per such component, in order
    assert mc.binary_img_to_centers(mask, cc, np.random.RandomState(1)) == want
    assert want[0] == ring1[5] and want[1] == ring2[3]                     # RandomState(1).randint(8) twice: 5, 3


def test_get_centers_on_hand_shapes():
    assert mc.get_centers(np.ones((2, 50), np.uint8)) == [] and mc.get_centers(np.ones((50, 2), np.uint8)) == []      # h < 3 / w < 3
    # a full rectangle has no zero pixel: every interior pixel is a centre pixel, one component, its centroid (14.5, 19.5) -> (14, 20)
    assert mc.get_centers(np.ones((30, 40), np.uint8)) == [(14, 20)]
    assert ref.centres(np.ones((30, 40), np.uint8), np.random.RandomState(1)) == [(14, 20)]
    assert mc.get_centers(np.pad(np.ones((12, 12), np.uint8), 1)) == []          # distances up to 6 only: nothing above min_rad
    two = cases.disc_scene((50, 90), [(24, 24, 18), (24, 58, 17)]) // 255
    got = mc.get_centers(two)
    assert len(got) == 2 and got == ref.centres(two, np.random.RandomState(1))
    assert abs(got[0][1] - 24) <= 2 and abs(got[1][1] - 58) <= 2
    for seed in range(6):                                    # random unions of discs: both implementations of the centre search
        rng = np.random.default_rng(seed)
        m = cases.disc_scene((70, 110), [(rng.integers(15, 55), rng.integers(15, 95), rng.integers(12, 20)) for _ in range(4)]) // 255
        assert mc.get_centers(m, rng=np.random.RandomState(1)) == ref.centres(m, np.random.RandomState(1)), seed


# ---- recursion and relabelling ------------------------------------------------------------------------------------------------------
def _appendix():
    """A 29 x 29 square with an 81-pixel square hanging on a 3-wide corridor of 15 pixels: a side below min_size = 100."""
    M = np.zeros((29, 29 + 5 + 9), np.uint8)
    M[:, :29] = 1
    M[13:16, 29:34] = 1
    M[10:19, 34:] = 1
    return M, (14, 14), (14, 38)


def test_a_side_below_min_size_is_merged_back():
    M, big, small = _appendix()
    h = ref.OracleSolverHandle()
    side = ref.solve_scipy(M, big, small, 5)[0]
    assert (M - side).sum() == 81 + 5 * 3 and side.sum() == 841                # the cut itself is at the square's wall
    for centers in ([big, small], [small, big]):
        cells = mc.segment_min_cut(M, list(centers), 5, handle=h)
        assert len(cells) == 1 and np.array_equal(cells[0], M)
    # with a third centre in the large square the sink's side is still merged back, and the two that remain are cut next
    centers = [big, small, (3, 3)]
    cells = mc.segment_min_cut(M, centers, 5, handle=h)
    want = ref.segment(M.astype(np.int64), centers, 5, ref.solve_scipy)
    assert len(cells) == len(want) and all(np.array_equal(a, b) for a, b in zip(cells, want))
    assert h.batches == [1, 1, 1, 1] and centers == [big, small, (3, 3)]     # the caller's list is not touched
    assert mc.segment_min_cut(M, [], 5, handle=h) == [] and len(mc.segment_min_cut(M, [big], 5, handle=h)) == 1


def test_whole_function_against_the_restatement_and_the_relabelling_order():
    mask = cases.scene()
    trace = []
    want, want_vis = ref.instance_min_cut(mask, 60, 1.25, trace=trace)
    assert sorted(trace) == [0, 0, 1]                        # both clumps are cut, the clump of three a second time one level down
    h = ref.OracleSolverHandle()
    stats = {}
    got, vis = mc.binary_seg_to_instance_min_cut(mask, 60, 1.25, handle=h, stats=stats)
    assert got.dtype == np.int32 and np.array_equal(got, want) and np.array_equal(vis, want_vis)
    assert h.batches == [2, 1] and stats['calls'] == 2 and stats['tasks'] == 3 and stats['regions'] == 2     # one call per level
    # 7 regions in raster order; the clump of two is region 6 and receives 8, the clump of three is region 7 and receives 9 and 10
    assert got.max() == 10
    assert set(np.unique(got[50:100, 60:150]).tolist()) == {0, 6, 8} and set(np.unique(got[100:150, 30:150]).tolist()) == {0, 7, 9, 10}
    assert got[75, 90] == 6 and got[75, 118] == 8            # the first cell (the source's side) keeps the region's label
    assert [int(got[125, x]) for x in (60, 90, 120)] == [7, 9, 10]
    assert np.array_equal(got != 0, mask != 0)
    # the other path solver underneath gives the same labels
    assert np.array_equal(mc.binary_seg_to_instance_min_cut(mask, 60, 1.25, handle=ref.OracleSolverHandle(ref.solve_paths))[0], want)
    # nothing to split: labels are the 4-connected components
    few = cases.disc_scene((60, 60), [(15, 15, 10), (40, 40, 12)])
    few[27, 27] = few[28, 28] = 255                          # a diagonal contact does not join under connectivity 1
    got, _ = mc.binary_seg_to_instance_min_cut(few, 60, 1.25, handle=h)
    assert np.array_equal(got, ref.instance_min_cut(few, 60, 1.25)[0]) and got.max() == 4
    empty, vis = mc.binary_seg_to_instance_min_cut(np.zeros((5, 6), np.uint8), 60, 1.25, handle=h)
    assert not empty.any() and vis.shape == (5, 6, 3) and not vis.any()
    with pytest.raises(ValueError):
        mc.binary_seg_to_instance_min_cut(mask, 3, 1.25, handle=h)


def test_hash_colours():
    # blake2b(str(label), digest_size=1, salt=b'1_r' / b'1_g'), worked out once with hashlib
    assert [ref.colour(v) for v in (0, 1, 2, 3)] == [(0, 0), (91, 125), (214, 222), (41, 70)]
    labels = np.array([[0, 1, 2, 3, 3]])
    mask = np.array([[1, 1, 1, 1, 0]])
    want = [[0, 0, 255], [91, 125, 168], [214, 222, 0], [41, 70, 255], [41, 70, 0]]      # b = clip(384 - r - g, 0, 255) inside the mask
    assert mc.label_colors(labels, mask).tolist() == [want] and ref.visualization(labels, mask).tolist() == [want]
    assert mc.label_colors(labels, mask, seed=2).tolist() != [want]


# ---- make stat_fish ---------------------------------------------------------------------------------------------------------------
class SplitterHandle(ref.OracleSolverHandle):
    """What ``main`` needs of a ``_lib.Handle`` with ``use_min_cut: True``, computed by the oracles."""

    def fish_spots(self, labels, img, probes, weights, normal, ithr, min_cc, line, capacity=4096):
        rec, thr, bnd, _ = sf_ref.loop(img, labels, probes, np.asarray(weights, np.float64), normal, ithr, min_cc, line)
        return rec, thr, bnd


class PlainHandle:
    """A handle of the time before the splitter: no ``min_cut``."""

    def ccl_labels(self, mask, connectivity=8):
        raise AssertionError('not reached')


def _folder(tmp_path, **section):
    inp = tmp_path / 'in'
    (inp / 'nuclei_masks').mkdir(parents=True)
    mask = cases.scene()
    rng = np.random.default_rng(3)
    img = rng.integers(0, 40, mask.shape + (3,), dtype=np.uint8)
    for cy, cx, _ in cases.SCENE_DISCS:
        img[cy - 3:cy, cx - 3:cx, 1] = 200
        img[cy + 1:cy + 4, cx + 1:cx + 4, 0] = 220
    image_io.write_tiff_rgb8(str(inp / 'clumps.tif'), img)
    image_io.write_tiff_gray8(str(inp / 'nuclei_masks' / 'clumps.tif'), mask)
    cfg = dict(inpath=str(inp), scale=1, use_min_cut=True, nuclei_size_T=5000)
    cfg.update(section)
    yaml.safe_dump({'stat_fish': cfg}, open(tmp_path / 'config.yaml', 'w'))
    return inp, img, mask


@pytest.mark.parametrize('scale', [1, 'auto'])
def test_main_with_the_splitter_writes_six_files(tmp_path, monkeypatch, scale):
    inp, img, mask = _folder(tmp_path, scale=scale)
    monkeypatch.chdir(tmp_path)
    sf.main([], handle=SplitterHandle())
    want, want_vis = ref.instance_min_cut(mask, 60, 1.25)
    s = 1 if scale == 1 else float(np.sqrt(2500 / np.median(np.bincount(want.reshape(-1))[1:])))      # the areas of the SPLIT cells
    stdev, min_cc = 3 / s, int(7 // (s * s))
    K = int(7 // s) if 7 // s % 2 else int(7 // s) + 1
    rec, thr, bnd, amb = sf_ref.records(img, want, (1, 0), sf.gaussian_proj_kernel([K, K], stdev), 15, (70, 70), min_cc, 2)
    assert amb == 0 and len(rec) == 10
    d = inp / 'annotated' / 'clumps'
    tag = 'n15_std%.2f_s%d_g70.0_r70.0' % (stdev, min_cc)
    assert sorted(os.listdir(d)) == sorted(['clumps' + tail for tail in ('__segmentation_min_cut.npy', '_segmentation.tif', '_original.tif',
                                                                       '_original_with_segmentation.tif', '_lsq_%s.tif' % tag,
                                                                       '_segmentation_corrected_min_cut.tif')])
    saved = np.load(d / 'clumps__segmentation_min_cut.npy')
    assert saved.dtype == np.int64 and np.array_equal(saved, want)
    # cv2.imwrite takes the (r, g, b) array for BGR: the file's samples are (b, g, r)
    assert np.array_equal(image_io.imread(str(d / 'clumps_segmentation_corrected_min_cut.tif')), want_vis[..., ::-1])
    assert np.array_equal(image_io.imread(str(d / ('clumps_lsq_%s.tif' % tag))), np.dstack([thr[..., 1], thr[..., 0], bnd]))
    rows = [['clumps', '%d_%d' % (r[2] // r[1], r[3] // r[1]), r[4], r[5], r[6] / r[7] if r[7] else 0.0, r[8],
             r[9], r[10], r[11] / r[12] if r[12] else 0.0, r[13], r[1], r[19], r[20]] for r in rec.tolist()]
    assert open(inp / 'annotated' / 'stat_fish_lsq.csv').read() == csvio.csv_text(sf.csv_columns(), rows)
    assert sum(r[3] for r in rows) >= 10 and sum(r[7] for r in rows) >= 10     # every cell kept its two spots
    params = yaml.safe_load(open(inp / 'annotated' / 'stat_fish_params.yaml'))
    assert params['flow_limit'] == 60 and params['cell_size_threshold_coeff'] == 1.25


def test_main_without_min_cut_on_the_handle_is_a_configuration_error(tmp_path, monkeypatch, capsys):
    inp, _, _ = _folder(tmp_path)
    monkeypatch.chdir(tmp_path)
    with pytest.raises(SystemExit) as e:
        sf.main([], handle=PlainHandle())
    assert e.value.code == 2 and 'use_min_cut: False' in capsys.readouterr().out
    assert sorted(os.listdir(inp)) == ['clumps.tif', 'nuclei_masks']


@pytest.mark.parametrize('text,key', [('flow_limit: 3', 'flow_limit'), ('flow_limit: 5000', 'flow_limit'), ('flow_limit: many', 'flow_limit'),
                                      ('cell_size_threshold_coeff: -1', 'cell_size_threshold_coeff'),
                                      ('cell_size_threshold_coeff: [1]', 'cell_size_threshold_coeff')])
def test_bad_splitter_parameters(tmp_path, monkeypatch, capsys, text, key):
    _folder(tmp_path)
    (tmp_path / 'src').mkdir()
    (tmp_path / 'src' / 'stat_fish_params.yaml').write_text(text + '\n')
    monkeypatch.chdir(tmp_path)
    with pytest.raises(SystemExit) as e:
        sf.main([], handle=SplitterHandle())
    assert e.value.code == 2 and key in capsys.readouterr().out


# ---- header, export, binding ------------------------------------------------------------------------------------------------------
def test_header_export_and_defaults():
    header = open(os.path.join(ROOT, 'include', 'ecseg_hip.h')).read()
    assert 'int ecseg_min_cut(ecseg_ctx* h, const uint8_t* masks, long long mask_bytes, const int32_t* tasks, int n_tasks, int dist' in header
    assert '#define ECSEG_ABI_VERSION 6' in header.replace('  ', ' ') or 'ECSEG_ABI_VERSION' in header
    for line in ('the source ball wins', 'capacity 2 into t', 'Nothing leaves t', 's has no arcs except to its ball'):
        assert line in header
    assert '#define ECSEG_MIN_CUT_MAX_DIST   %d' % _lib.Handle.MIN_CUT_MAX_DIST in header
    assert '#define ECSEG_MIN_CUT_LDS_PIXELS %d' % _lib.Handle.MIN_CUT_LDS_PIXELS in header
    assert 'ecseg_min_cut' in _lib.EXPORTS and _lib.ABI_VERSION == 6 and hasattr(_lib.Handle, 'min_cut')
    assert sf.DEFAULT_PARAMS['flow_limit'] == 60 and sf.DEFAULT_PARAMS['cell_size_threshold_coeff'] == 1.25
    assert sf.MAX_DIST == _lib.Handle.MIN_CUT_MAX_DIST
    assert yaml.safe_load(open(os.path.join(ROOT, 'config.yaml')))['stat_fish']['use_min_cut'] is False
    import ecseg_amd.build as build
    assert 'mincut_kernels.hip' in build.SOURCES
