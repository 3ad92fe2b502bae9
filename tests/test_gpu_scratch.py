"""The drivers' scratch arenas on the device (csrc/ctx.h: post_arena, call_arena, count_arena, keep_arena): what a driver returns
depends on its arguments alone, not on what the handle did before, and the region map of nuclei_regions outlives every other
driver.  Every comparison is byte for byte against a fresh handle; the inputs come from the *_cases.py generators."""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fish_distance_cases as fd_cases       # noqa: E402
import min_cut_cases as mc_cases             # noqa: E402
import nuset_cases as nu_cases               # noqa: E402
import rescale_cases as rs_cases             # noqa: E402
import stat_fish_cases as sf_cases           # noqa: E402

from ecseg_amd._lib import Handle            # noqa: E402

pytestmark = pytest.mark.gpu

GROW, REUSE, PROBE = (130, 257), (17, 40), (33, 70)    # every arena regrows; stale contents at other offsets; the shape compared
POST_CHUNK = 64                                        # ecseg_ctx::post_chunk


@functools.lru_cache(maxsize=None)
def _fish_scene(size):
    lsq, seg = fd_cases.scene(3, size)
    return lsq, seg.astype(np.int32)


@functools.lru_cache(maxsize=None)
def _spot_case(size):
    return sf_cases.scene(1, size=size, K=7)           # (seed 1: nuclei present, two probes)


@functools.lru_cache(maxsize=None)
def _cut_tasks(size):
    return tuple(mc_cases.random_task(seed, max_side=size[0])[:3] for seed in range(4))     # (130: windows above the LDS bound too)


@functools.lru_cache(maxsize=None)
def _rpn_case(size):
    return nu_cases._sized('scratch', 2, size[0] // 4, size[1] // 4, 3, 6000, 800)          # (130 x 257: more than one sort block)


@functools.lru_cache(maxsize=None)
def _blobs(size):
    return rs_cases.blobs(size[0], size[1], 21)


@functools.lru_cache(maxsize=None)
def _markers(size):
    rows, cols = np.nonzero(_blobs(size))
    pick = np.arange(0, len(rows), max(1, len(rows) // 12))
    return rows[pick].astype(np.int32), cols[pick].astype(np.int32), np.arange(1, len(pick) + 1, dtype=np.int32)


@functools.lru_cache(maxsize=None)
def _gray(size):
    return rs_cases.scene(size[0], size[1], 22)


def _regions(h, size):
    lsq, seg = _fish_scene(size)
    return (h.nuclei_regions((seg > 0).astype(np.uint8), lsq, 0),)


def _crops(h, rec):
    """Windows (at most 256 x 256) at the bounding boxes of the first regions of the map on the handle."""
    win = [(k, r[1], r[2], min(r[3] - r[1], 256), min(r[4] - r[2], 256)) for k, r in enumerate(rec[:6])]
    return h.nucleus_crops(np.asarray(win, np.int32), (2, 0, 1))


def _regions_and_crops(h, size):
    rec, = _regions(h, size)
    return (rec,) + tuple(_crops(h, rec))


def _fish_distances(h, size, capacity=4096):
    lsq, seg = _fish_scene(size)
    return (h.fish_distances(seg, lsq, 0, 1, capacity=capacity),)


def _fish_spots(h, size, capacity=4096):
    c = _spot_case(size)
    return h.fish_spots(c['seg'], c['img'], c['probes'], c['weights'], c['normal'], c['ithr'], c['min_cc'], c['line'], capacity=capacity)


def _min_cut(h, size):
    sides, flow = h.min_cut(_cut_tasks(size), 5)
    return tuple(sides) + (flow,)


def _rpn_proposals(h, size):
    c = _rpn_case(size)
    return h.rpn_proposals(c['cls'], c['bbox'], c['ref'], c['stride'], c['im_h'], c['im_w'], c['thr'], c['pre'], c['post'])


def _clean_nuclei(h, size):
    out, mean, cleaned = h.clean_nuclei(_blobs(size), 20, want_cleaned=True)
    return out, np.float64(mean), cleaned


def _marker_watershed(h, size):
    return (h.marker_watershed(_blobs(size), *_markers(size)),)


def _rescale_down(h, size):
    return h.rescale_down(_gray(size), 0.5)


def _rescale_mask_up(h, size):
    return (h.rescale_mask_up(_blobs(size), 1 / 0.5, 5),)


OTHERS = {'fish_distances': _fish_distances, 'fish_spots': _fish_spots, 'min_cut': _min_cut, 'rpn_proposals': _rpn_proposals,
          'clean_nuclei': _clean_nuclei, 'marker_watershed': _marker_watershed, 'rescale_down': _rescale_down,
          'rescale_mask_up': _rescale_mask_up}
DRIVERS = dict(OTHERS, nuclei_regions=_regions_and_crops)


def _assert_same(got, want, what):
    assert len(got) == len(want), what
    for k, (g, w) in enumerate(zip(got, want)):
        g, w = np.asarray(g), np.asarray(w)
        assert g.dtype == w.dtype and g.shape == w.shape, (what, k, g.dtype, w.dtype, g.shape, w.shape)
        assert g.tobytes() == w.tobytes(), (what, k)


def _fresh(run, *args, **kw):
    h = Handle(0)
    try:
        return run(h, *args, **kw)
    finally:
        h.close()


def test_region_map_survives_every_other_driver():
    """nuclei_regions at 96 x 130, then every other driver at 130 x 257 - each arena regrows - then nucleus_crops: the crops and
    the channel maxima are those of a handle that ran regions and crops alone."""
    size = (96, 130)
    want = _fresh(_regions_and_crops, size)
    h = Handle(0)
    try:
        rec, = _regions(h, size)
        for run in OTHERS.values():
            run(h, GROW)
        got = (rec,) + tuple(_crops(h, rec))
    finally:
        h.close()
    assert len(rec) > 1
    _assert_same(got, want, 'nucleus_crops after the other drivers')


@pytest.mark.parametrize('name', sorted(DRIVERS))
def test_a_driver_does_not_depend_on_the_handles_history(name):
    """33 x 70 on a fresh handle against 33 x 70 on a handle that ran every driver at 130 x 257 (the arenas grow) and then at
    17 x 40 (they are reused, with stale contents at other offsets)."""
    want = _fresh(DRIVERS[name], PROBE)
    h = Handle(0)
    try:
        for size in (GROW, REUSE):
            for run in DRIVERS.values():
                run(h, size)
        got = DRIVERS[name](h, PROBE)
    finally:
        h.close()
    _assert_same(got, want, name)


@pytest.mark.parametrize('name', ['fish_distances', 'fish_spots'])
def test_two_stage_drivers_come_back_with_a_larger_capacity(name):
    """capacity below the cell count (the call returns the count alone, the cell index stays in the call arena), then enough: the
    same as one sufficient call on a fresh handle."""
    run = DRIVERS[name]
    want = _fresh(run, PROBE)
    assert len(want[0]) > 1                                   # (capacity 1 is too small)
    _assert_same(_fresh(run, PROBE, capacity=1), want, name)


def _label_stack(n, size):
    """n uint8 class images (0 .. 3) cut from the FISH scene's label map, each shifted differently."""
    _, seg = _fish_scene(size)
    base = np.where(seg > 0, 1 + seg % 3, 0).astype(np.uint8)
    return np.stack([np.roll(base, (3 * k, 5 * k), (0, 1)) for k in range(n)])


def test_post_workspace_grows_in_images_and_in_pixels():
    """meta_inference and count_cc with 1, post_chunk + 1 and 1 images again, on 33 x 70 and then on 130 x 257: the workspace
    grows in both dimensions and is reused below its capacity; the results are a fresh handle's."""
    h = Handle(0)
    try:
        for size in (PROBE, GROW):
            for n in (1, POST_CHUNK + 1, 1):
                lab = _label_stack(n, size)
                _assert_same(h.meta_inference(lab), _fresh(Handle.meta_inference, lab), ('meta_inference', size, n))
                _assert_same(h.count_cc(lab == 3), _fresh(Handle.count_cc, lab == 3), ('count_cc', size, n))
    finally:
        h.close()
