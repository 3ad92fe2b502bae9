"""The drivers' scratch arenas on the device (csrc/ctx.h: post_arena, call_arena, count_arena, keep_arena, pre_arena): what a driver returns
depends on its arguments alone, not on what the handle did before, and the region map of nuclei_regions outlives every other
driver.  Every comparison is byte for byte against a fresh handle; the inputs come from the *_cases.py generators.

One handle under test is open at a time.  The exception: the two synthetic classifiers of classify_nucleus_crops and interseg_batch
live on handles of their own (``_classifiers``), opened at their first use and closed when the module ends - the entries take the
plans' handles as arguments, and the handle under test holds the crops, never the plans."""
import functools
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ccl_pass_cases as cc_cases            # noqa: E402
import fish_distance_cases as fd_cases       # noqa: E402
import lzw_ref                               # noqa: E402
import min_cut_cases as mc_cases             # noqa: E402
import nuset_cases as nu_cases               # noqa: E402
import png_gray_cases as pg_cases             # noqa: E402
import png_label_cases as pl_cases            # noqa: E402
import rescale_cases as rs_cases             # noqa: E402
import scratch_drivers                       # noqa: E402
import stat_fish_cases as sf_cases           # noqa: E402
import tiff_decode_cases as td_cases         # noqa: E402

from ecseg_amd._lib import Handle            # noqa: E402

pytestmark = pytest.mark.gpu

GROW, REUSE, PROBE = (130, 257), (17, 40), (33, 70)    # every arena regrows; stale contents at other offsets; the shape compared
POST_CHUNK = 64                                        # ecseg_ctx::post_chunk
MCR_LDS_PIXELS = int(re.search(r'#define\s+ECSEG_MIN_CUT_CENTERS_LDS_PIXELS\s+(\d+)',
                               open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'ecseg_hip.h')).read()).group(1))


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


# ---- the drivers added since the first scratch test ----------------------------------------------------------------------------
def _sizes(size):
    """Three extents for one batch call, all at most ``size`` and all different: the offsets of the images within the chunk differ
    from those of any call at another ``size``."""
    H, W = size
    return [(H, W), (2 * H // 3 + 1, W // 2 + 3), (H // 2, W)]


def _file(data):
    return np.zeros(0, np.uint8) if data is None else np.frombuffer(bytes(data), np.uint8)


def _flat(values):
    """lists, tuples, bytes and None inside a driver's answer, flattened to arrays in a fixed order"""
    out = []
    for v in values:
        if isinstance(v, (list, tuple)):
            out += _flat(v)
        else:
            out.append(_file(v) if v is None or isinstance(v, (bytes, bytearray)) else np.asarray(v))
    return out


_MODELS = {}


def _classifiers():
    """The two synthetic classifiers of tests/test_gpu_interseg_batch.py, each on a handle of its own that stays open for the module:
    the handle under test holds the crops, never the plans."""
    if not _MODELS:
        from ecseg_amd import synth
        from ecseg_amd.model import MetasegModel
        for kind, seed in (('interseg', 3), ('ecseg_c', 4)):
            cfg = synth.classifier_config(kind)
            _MODELS[kind] = MetasegModel(cfg, synth.classifier_weights(cfg, seed=seed), handle=Handle(0))
    return _MODELS['interseg'], _MODELS['ecseg_c']


def teardown_module(module):
    for m in _MODELS.values():
        m.handle.close()
    _MODELS.clear()


def _classify_nucleus_crops(h, size):
    from ecseg_amd import interseg
    mi, mc = _classifiers()
    rec, = _regions(h, size)
    _, _, desc, tiled, _ = interseg.region_rows(rec)
    return (rec,) + tuple(h.classify_nucleus_crops(desc[:4], (0, 1, 2), tiled[:4], True, mi, mc))


@functools.lru_cache(maxsize=None)
def _crop_stack(size):
    rng = np.random.default_rng(size[0])
    k = 1 + size[0] // 40                                    # 4, 1 and 1 crops
    crops = rng.integers(0, 256, (k, 256, 256, 3), dtype=np.uint8)
    return crops, crops.reshape(k, -1, 3).max(axis=1).astype(np.int32)


def _iseg_classifier_inputs(h, size):
    crops, mx = _crop_stack(size)
    k = len(crops)
    return h.iseg_classifier_inputs(crops, mx, list(range(k)), list(range(k - 1, -1, -1)))


def _interseg_batch(h, size):
    mi, mc = _classifiers()
    scenes = [_fish_scene(sz) for sz in _sizes(size)]
    got = h.interseg_many([s[0] for s in scenes], [(s[1] > 0).astype(np.uint8) for s in scenes], 0, [True, False, True], mi, mc)
    return _flat(got)


@functools.lru_cache(maxsize=None)
def _fish_items(size):
    """a mask, given labels and a 4-channel image with a picture: K = 3, 7 and 1"""
    a, b, c = _sizes(size)
    return (sf_cases.make_item(601, a, 3, 3, 'mask', min_cc=2), sf_cases.make_item(605, b, 7, 3, 'labels', min_cc=1),
            sf_cases.make_item(610, c, 1, 4, 'mask', min_cc=3, picture=True))


def _stat_fish_batch(h, size):
    items = list(_fish_items(size))
    need = h.stat_fish_batch_bytes([h._stat_fish_item(it) for it in items], 4096)        # (a pure function of the table: no arena)
    return _flat(h.stat_fish_many(items, 1, want_masks=True)) + [np.int64(need)]


def _min_cut_regions(h, size):
    """the per-crop state in LDS, then in global memory (``comp`` in count_arena)"""
    out = []
    try:
        for lds in (MCR_LDS_PIXELS, 0):
            h.set_option('min_cut_centers_lds_pixels', lds)
            out += _flat(h.min_cut_regions(_blobs(size), 0.5, 2))
    finally:
        h.set_option('min_cut_centers_lds_pixels', MCR_LDS_PIXELS)          # (a handle's default: the option has no getter)
    return out


def _marker_watershed_batch(h, size):
    sizes = _sizes(size)
    return h.marker_watershed_batch([_blobs(sz) for sz in sizes], [_markers(sz) for sz in sizes])


@functools.lru_cache(maxsize=None)
def _nuset_plan(size):
    """NuSeT's network at base 8 on the extent rounded down to a multiple of 16 (the smallest synthetic plan of tests/test_gpu_nuset.py)"""
    from ecseg_amd import keras_plan, nuset
    hh, ww = max(16, size[0] // 16 * 16), max(16, size[1] // 16 * 16)
    cfg = nuset.nuset_config(hh, ww, 8)
    plan = keras_plan.build_plan(cfg, nuset.synth_weights(nuset.nuset_config(16, 16, 8), seed=21), keep=nuset.RPN_LAYERS[1:])
    x = nuset.whole_image_norm(rs_cases.scene(hh, ww, 23).astype(np.float64))
    return plan, x, hh, ww


def _nuset_forward(h, size):
    from ecseg_amd import nuset
    plan, x, hh, ww = _nuset_plan(size)
    h.load_plan(plan)
    mask = h.nuset_forward(x, plan.layer_tensor['rpn_cls_score'], plan.layer_tensor['rpn_bbox_pred'])
    return (mask,) + tuple(h.rpn_proposals_last(nuset.reference_anchors(8.0), nuset.STRIDE, hh, ww, 0.3))


@functools.lru_cache(maxsize=None)
def _render_case(size, C=4):
    """(img, channels, thresholded, boundaries) as tests/test_gpu_stat_fish_aqua.py draws them"""
    rng = np.random.default_rng(31 + size[0])
    H, W = size
    img = rng.integers(0, 256, (H, W, C), dtype=np.uint8)
    thr = (rng.random((H, W, C - 1)) < 0.4).astype(np.uint8) * np.uint8(255)
    bnd = (rng.random((H, W)) < 0.5).astype(np.uint8) * np.uint8(255)
    return img, (2, 1, 0, 3)[:C], thr, bnd


def _fish_render(h, size):
    return h.fish_render(*_render_case(size))


def _fish_render_tiff(h, size):
    files, rasters = h.fish_render_tiff(*_render_case(size), want_rasters=True)
    return _flat([files, rasters])


def _fish_render_tiff_batch(h, size):
    a, b, c = _sizes(size)
    items = [_render_case(a) + (_blobs(a) * np.uint8(255), None), _render_case(b, 3) + (None, _picture(b)), _render_case(c) + (None, None)]
    return _flat(h.fish_render_tiff_many(items))


@functools.lru_cache(maxsize=None)
def _picture(size):
    """an (H, W, 3) raster with runs and noise: LZW strips of very different lengths"""
    rng = np.random.default_rng(41 + size[1])
    pic = rng.integers(0, 256, size + (3,), dtype=np.uint8)
    pic[size[0] // 3:] = pic[size[0] // 3:] // 64 * 64
    return pic


def _tiff_encode(h, size):
    return _flat([h.tiff_encode(_picture(size)), h.tiff_encode(_gray(size), invert=True)])


def _tiff_rasters(size):
    a, b, c = _sizes(size)
    return [_picture(a), _gray(b), _blobs(c) * np.uint8(255)], [False, True, False]


def _tiff_encode_batch(h, size):
    return _flat(h.tiff_encode_many(*_tiff_rasters(size)))


@functools.lru_cache(maxsize=None)
def _tiff_files(size):
    """the files tests/lzw_ref.py writes for the three rasters: the decoder's inputs"""
    rasters, inverts = _tiff_rasters(size)
    return tuple(lzw_ref.tiff_file(r, invert=v) for r, v in zip(rasters, inverts))


def _tiff_decode(h, size):
    return [h.tiff_decode(f) for f in _tiff_files(size)[:2]]


def _tiff_decode_batch(h, size):
    return h.tiff_decode_many(list(_tiff_files(size)))


def _png_labels_encode(h, size):
    return _flat([h.png_labels_encode(_label_stack(3, size)), h.png_labels_encode(pl_cases.mixed(np.random.default_rng(5), *size))])


def _png_channel_encode(h, size):
    return _flat([h.png_channel_encode(_channel_pixels(size), 0, invert=True), h.png_channel_encode(_channel_pixels(size), 1)])


@functools.lru_cache(maxsize=None)
def _channel_pixels(size):
    rng = np.random.default_rng(6)
    return np.stack([np.dstack([pg_cases.fish_raster(size[0], size[1], rng), _gray(size)]) for _ in range(2)])


def _overlay_images(size):
    return np.stack([_picture(size), _picture(size)[::-1]])


def _overlay_files(h, size):
    img = _overlay_images(size).astype(np.uint16) * np.uint16(257)      # 16-bit: the 8-bit image is made in call_arena
    return _flat(h.overlay_files(_label_stack(2, size), img, 120))


CCL_MODE = cc_cases._mode('scratch', 'labels', 0x03020100, 8, stat=3, need=7)      # multi-key, 8-connected: areas, sums, counts, last root
CCL_KEYS = ('area', 'cnt', 'flag', 'last_root', 'ncomp', 'nlist1', 'nlist2', 'npx', 'root', 'sumx', 'sumy', 'tile_any')


def _ccl_pass(h, size):
    """one pass with everything but the root lists, whose order is free"""
    m = CCL_MODE
    got = h.ccl_pass(_label_stack(3, size), lut=m.lut, conn=m.conn, stat=m.stat, need=m.need)
    return [np.asarray(got[k]) for k in CCL_KEYS]


def _post_workspace(h, size):
    """the clean-up workspace through its first users: meta_inference and count_cc, two images"""
    lab = _label_stack(2, size)
    return _flat([h.meta_inference(lab), h.count_cc(lab == 3)])


# ---- the file and TIFF forms of meta_segment: a U-Net's stitch needs 256 x 256, so these two rows run at shapes of their own ------
UNET_SIZES = {GROW: (300, 270), REUSE: (256, 256), PROBE: (260, 300)}


@functools.lru_cache(maxsize=None)
def _unet16():
    """the smallest synthetic U-Net of tests/test_gpu_metaseg_files.py"""
    from ecseg_amd import synth
    cfg = synth.unet_config(base=16)
    return cfg, synth.unet_weights(cfg, seed=0)


def _with_unet(h):
    from ecseg_amd.model import MetasegModel
    if getattr(h, '_scratch_unet', None) is None or h.plan is not h._scratch_unet.plan:
        h._scratch_unet = MetasegModel(*_unet16(), handle=h)
    return h


@functools.lru_cache(maxsize=None)
def _dapi_images(size, seed0=60):
    from ecseg_amd import synth
    H, W = UNET_SIZES[size]
    imgs = np.stack([synth.dapi_image(seed0 + i, H, W, rgb=True) for i in range(2)])
    imgs[1, ..., 2] = 255 - imgs[1, ..., 2]                 # a bright background: the inverting branch of the pre-processing
    return imgs


def _meta_segment_files(h, size):
    return _flat(_with_unet(h).meta_segment_files(_dapi_images(size)))


@functools.lru_cache(maxsize=None)
def _dapi_tiffs(size, seed0, corrupt=False):
    """two gray LZW files of one row per strip; ``corrupt``: the second one's middle strip is no LZW stream"""
    imgs = _dapi_images(size, seed0)[..., 2]
    files = [td_cases.file_of(np.ascontiguousarray(im), 1) for im in imgs]
    if corrupt:
        H, W = imgs[1].shape
        strips = [td_cases.pack(td_cases.lzw_codes(imgs[1][r].tobytes())) for r in range(H)]
        strips[H // 2] = b'\xff' * len(strips[H // 2])
        files[1] = td_cases.tiff_file(strips, H, W, 1)
    return tuple(files)


def _pinned(h, files):
    """the files as views of one page-locked buffer: what a caller names with prefetch_tiffs and then passes"""
    buf = h.host_empty((sum(len(f) for f in files),))
    at, views = 0, []
    for f in files:
        buf[at:at + len(f)] = np.frombuffer(f, np.uint8)
        views.append(buf[at:at + len(f)])
        at += len(f)
    return buf, views


def _meta_segment_tiffs(h, size):
    """B named ahead, A called (B is decoded under it, in pre_arena), B called (it takes the rasters), then the file form on A"""
    _with_unet(h)
    H, W = UNET_SIZES[size]
    shape = (H, W, 1, 8)
    bufs = [_pinned(h, _dapi_tiffs(size, 60)), _pinned(h, _dapi_tiffs(size, 80, True))]
    try:
        A, B = bufs[0][1], bufs[1][1]
        h.prefetch_tiffs(B, shape)
        out = [h.meta_segment_tiffs(A, shape), h.meta_segment_tiffs(B, shape), h.meta_segment_tiffs_files(A, shape)]
    finally:
        h.prefetch_tiffs(None)
        for buf, _ in bufs:
            h.host_release(buf)
    return _flat(out)


# The first scratch test's drivers but nuclei_regions: the region map outlives every one of them and every driver below.
OTHERS = {'fish_distances': _fish_distances, 'fish_spots': _fish_spots, 'min_cut': _min_cut, 'rpn_proposals': _rpn_proposals,
          'clean_nuclei': _clean_nuclei, 'marker_watershed': _marker_watershed, 'rescale_down': _rescale_down,
          'rescale_mask_up': _rescale_mask_up}
# Added since.  classify_nucleus_crops runs nuclei_regions itself (it needs a map), so it stands outside ADDED's survivors.
ADDED = {'iseg_classifier_inputs': _iseg_classifier_inputs, 'interseg_batch': _interseg_batch, 'stat_fish_batch': _stat_fish_batch,
         'min_cut_regions': _min_cut_regions, 'marker_watershed_batch': _marker_watershed_batch, 'nuset_forward': _nuset_forward,
         'fish_render': _fish_render, 'fish_render_tiff': _fish_render_tiff, 'fish_render_tiff_batch': _fish_render_tiff_batch,
         'tiff_encode': _tiff_encode, 'tiff_encode_batch': _tiff_encode_batch, 'tiff_decode': _tiff_decode,
         'tiff_decode_batch': _tiff_decode_batch, 'png_labels_encode': _png_labels_encode, 'png_channel_encode': _png_channel_encode,
         'overlay_files': _overlay_files, 'ccl_pass': _ccl_pass, 'post_workspace': _post_workspace,
         'meta_segment_files': _meta_segment_files, 'meta_segment_tiffs': _meta_segment_tiffs}
DRIVERS = dict(OTHERS, nuclei_regions=_regions_and_crops, classify_nucleus_crops=_classify_nucleus_crops, **ADDED)
assert set(DRIVERS) == set(scratch_drivers.ROWS), sorted(set(DRIVERS) ^ set(scratch_drivers.ROWS))


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
    the channel maxima are those of a handle that ran regions and crops alone.  (classify_nucleus_crops makes a map of its own.)"""
    size = (96, 130)
    want = _fresh(_regions_and_crops, size)
    h = Handle(0)
    try:
        rec, = _regions(h, size)
        for run in list(OTHERS.values()) + list(ADDED.values()):
            run(h, GROW)
        got = (rec,) + tuple(_crops(h, rec))
    finally:
        h.close()
    assert len(rec) > 1
    _assert_same(got, want, 'nucleus_crops after the other drivers')


def test_the_fill_withdraws_the_region_map():
    """scratch_fill_debug is the one call that touches keep_arena: nucleus_crops afterwards finds no region map, and reads no fill."""
    from ecseg_amd._lib import EcsegError
    h = Handle(0)
    try:
        rec, = _regions(h, PROBE)
        h.scratch_fill_debug(0xFF)
        with pytest.raises(EcsegError, match='no region map on the handle') as e:
            _crops(h, rec)
        assert e.value.code == -1
        with pytest.raises(EcsegError):
            h.scratch_fill_debug(256)
        _assert_same(_regions_and_crops(h, PROBE), _fresh(_regions_and_crops, PROBE), 'regions and crops after the fill')
    finally:
        h.close()


def test_the_fill_between_prefetch_and_the_call_withdraws_the_decode_ahead():
    """B named, A called - B lies decoded in d_pre, its status words in pre_arena - then the fill: the call on B decodes B itself and
    reports the corrupt file from its own status words, not from the fill; every result is that of the plain calls.  And the TIFF
    form gives what meta_segment gives on the samples the files were written from."""
    size = PROBE
    H, W = UNET_SIZES[size]
    shape = (H, W, 1, 8)
    for byte in (0x00, 0xFF):
        h = _with_unet(Handle(0))
        try:
            bufs = [_pinned(h, _dapi_tiffs(size, 60)), _pinned(h, _dapi_tiffs(size, 80, True))]
            A, B = bufs[0][1], bufs[1][1]
            plain_a, plain_b = h.meta_segment_tiffs(A, shape), h.meta_segment_tiffs(B, shape)
            assert plain_a[4] == [0, 0] and plain_b[4] == [0, -1]
            _assert_same(plain_a[:4], h.meta_segment(np.ascontiguousarray(_dapi_images(size, 60)[..., 2])), 'the samples')
            h.prefetch_tiffs(B, shape)
            _assert_same(_flat(h.meta_segment_tiffs(A, shape)), _flat(plain_a), ('A', byte))
            h.scratch_fill_debug(byte)
            _assert_same(_flat(h.meta_segment_tiffs(B, shape)), _flat(plain_b), ('B after the fill', byte))
            h.prefetch_tiffs(B, shape)                       # named, filled before any call took it, then called
            h.scratch_fill_debug(byte)
            _assert_same(_flat(h.meta_segment_tiffs(A, shape)), _flat(plain_a), ('A after the fill', byte))
            _assert_same(_flat(h.meta_segment_tiffs(B, shape)), _flat(plain_b), ('B again', byte))
        finally:
            h.prefetch_tiffs(None)
            h.close()


_FRESH = {}


def _fresh_answer(name, size):
    """a fresh handle's answer, computed once per (driver, size) and shared by the tests: read-only"""
    if (name, size) not in _FRESH:
        _FRESH[name, size] = _flat(_fresh(DRIVERS[name], size))
    return _FRESH[name, size]


@pytest.mark.parametrize('name', sorted(DRIVERS))
def test_a_driver_does_not_depend_on_the_handles_history(name):
    """33 x 70 on a fresh handle against 33 x 70 on a handle that ran every driver at 130 x 257 (the arenas grow) and then at
    17 x 40 (they are reused, with stale contents at other offsets).  The drivers of the first scratch test keep that whole history
    of one another; each driver added since runs behind one fixed history - itself and the first nine at both sizes - which keeps a
    case at a few seconds (the poisoned test below is the complete one)."""
    want = _fresh_answer(name, PROBE)
    first = dict(OTHERS, nuclei_regions=_regions_and_crops)
    history = first if name in first else dict(first, **{name: DRIVERS[name]})
    h = Handle(0)
    try:
        for size in (GROW, REUSE):
            for run in history.values():
                run(h, size)
        got = _flat(DRIVERS[name](h, PROBE))
    finally:
        h.close()
    _assert_same(got, want, name)


@pytest.mark.parametrize('byte', [0x00, 0xFF], ids=['0x00', '0xFF'])
@pytest.mark.parametrize('name', sorted(DRIVERS))
def test_a_driver_gives_its_answer_on_poisoned_arenas(name, byte):
    """The driver at 130 x 257 (its arenas at their largest), every arena filled with ``byte`` over its whole capacity, then 33 x 70
    against a fresh handle; filled again, then 130 x 257 against a fresh handle (the last slots of the layout lie in the fill too).
    0x00 breaks what assumes a -1 or INT_MAX preset; 0xFF what assumes zeroed counters, flags, marks, status words and sizes."""
    run = DRIVERS[name]
    h = Handle(0)
    try:
        run(h, GROW)
        h.scratch_fill_debug(byte)
        small = _flat(run(h, PROBE))
        h.scratch_fill_debug(byte)
        large = _flat(run(h, GROW))
    finally:
        h.close()
    _assert_same(small, _fresh_answer(name, PROBE), (name, 'PROBE after the fill'))
    _assert_same(large, _fresh_answer(name, GROW), (name, 'GROW after the fill'))


# ---- a fresh handle is no reference: the 33 x 70 answers against the CPU restatements, compared as each driver's own module does ----
def _tmp_file(write, *args, **kw):
    import tempfile
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, 'f')
        write(path, *args, **kw)
        return np.frombuffer(open(path, 'rb').read(), np.uint8)


def _ref_fish_distances(got):
    import fish_distance_ref
    lsq, seg = _fish_scene(PROBE)
    assert np.array_equal(got[0], fish_distance_ref.records(lsq, seg, 0, 1))


def _ref_fish_spots(got):
    import stat_fish_ref
    c = _spot_case(PROBE)
    rec, thr, bnd, amb = stat_fish_ref.records(c['img'], c['seg'], c['probes'], c['weights'], c['normal'], c['ithr'], c['min_cc'], c['line'])
    assert amb == 0, 'the case holds pixels within 2 B of the threshold: not a committed case'
    assert np.array_equal(got[0], rec) and np.array_equal(got[1], thr) and np.array_equal(got[2], bnd)


def _ref_min_cut(got):
    import min_cut_ref
    tasks = _cut_tasks(PROBE)
    for k, (M, s, t) in enumerate(tasks):
        side, flow = min_cut_ref.solve_scipy(M, s, t, 5)
        assert int(got[len(tasks)][k]) == flow and np.array_equal(got[k], side), k


def _ref_rpn_proposals(got):
    import nuset_ref
    c = _rpn_case(PROBE)
    want = nuset_ref.proposals(c['cls'], c['bbox'], c['ref'], c['stride'], c['im_h'], c['im_w'], c['thr'], c['pre'], c['post'])
    scores, props, idx = got
    assert idx.tolist() == want['indices'].tolist() and np.array_equal(scores, want['scores'])
    if len(idx):                                             # (tests/test_gpu_nuset.py: coordinates within 4 ulp of the extent)
        assert np.abs(props.astype(np.float64) - want['proposals'].astype(np.float64)).max() <= 4 * float(np.spacing(np.float32(max(c['im_h'], c['im_w']))))


def _ref_clean_nuclei(got):
    import watershed_ref
    cl, mean = watershed_ref.clean_image(_blobs(PROBE))
    assert np.array_equal(got[2], cl) and np.array_equal(got[0], watershed_ref.final_mask(cl, 20))
    assert (np.isnan(got[1]) and np.isnan(mean)) or float(got[1]) == mean


def _ref_marker_watershed(got):
    import watershed_ref
    assert np.array_equal(got[0], watershed_ref.watershed_from_markers(_blobs(PROBE), *_markers(PROBE)))


def _ref_marker_watershed_batch(got):
    import watershed_ref
    for g, sz in zip(got, _sizes(PROBE)):
        assert np.array_equal(g, watershed_ref.watershed_from_markers(_blobs(sz), *_markers(sz)).astype(np.uint8)), sz


def _ref_rescale_down(got):
    import rescale_ref
    want, want_f = rescale_ref.rescale_down(_gray(PROBE), 0.5)
    out, filtered = (got[0], got[1]) if got[0].dtype == np.float64 else (got[1], got[0])
    assert np.array_equal(out, want) and np.array_equal(filtered, want_f)


def _ref_rescale_mask_up(got):
    import rescale_ref
    assert np.array_equal(got[0], rescale_ref.rescale_mask_up(_blobs(PROBE), 1 / 0.5, 5))


def _ref_stat_fish_batch(got):
    """ranks, records (cells of a labelled mask are numbered by first pixel: column 0 apart), masks; the files against tests/lzw_ref.py"""
    import aqua_ref
    import stat_fish_ref as ref
    at = 0
    for item in _fish_items(PROBE):
        ranks, records, f0, f1, f2, fm, fp, thr, bnd = got[at:at + 9]
        at += 9
        seg = ref.nuclei(item['mask']) if item.get('mask') is not None else item['labels']
        rec, w_thr, w_bnd, amb = ref.records(item['img'], seg, item['channels'][1:], item['weights'], item['normal_threshold'],
                                             item['intensity_thresholds'], item['min_cc_size'], 1)
        assert amb == 0, 'the item holds pixels within 2 B of the threshold: not a committed case'
        cols = slice(1, None) if item.get('mask') is not None else slice(0, None)
        assert np.array_equal(ranks, ref.ranks(seg)[0].astype(np.int32)) and records.shape == rec.shape
        assert np.array_equal(records[:, cols], rec[:, cols]) and np.array_equal(thr, w_thr) and np.array_equal(bnd, w_bnd)
        I = item['img'][..., item['channels']]
        for f, raster in zip((f0, f1, f2), aqua_ref.files(I, w_thr, w_bnd)):
            assert f.tobytes() == lzw_ref.tiff_file(raster)
        assert fm.tobytes() == (lzw_ref.tiff_file(item['mask']) if item.get('mask_file') is True else b'')
        assert fp.tobytes() == (lzw_ref.tiff_file(item['picture']) if item.get('picture') is not None else b'')


def _ref_min_cut_regions(got):
    import min_cut_region_cases
    want = min_cut_region_cases.expected(_blobs(PROBE), 0.5, 2)
    n = len(want['windows'])
    assert len(want['regions']) > 0 and len(got) == 2 * (3 + 2 * n)
    for half in (got[:3 + 2 * n], got[3 + 2 * n:]):           # LDS, then global memory
        assert np.array_equal(half[0], want['labels']) and np.array_equal(half[1], want['regions']) and np.array_equal(half[2], want['centers'])
        assert all(np.array_equal(a, b) for a, b in zip(half[3:3 + n], want['windows']))
        assert all(np.array_equal(a, b) for a, b in zip(half[3 + n:], want['comp']))


def _want_renders(case):
    import aqua_ref
    img, channels, thr, bnd = case
    return aqua_ref.files(img[..., list(channels)], thr, bnd)


def _ref_fish_render(got):
    for g, w in zip(got, _want_renders(_render_case(PROBE))):
        assert g.tobytes() == w.tobytes()


def _ref_fish_render_tiff(got):
    want = _want_renders(_render_case(PROBE))
    for f, r, w in zip(got[:3], got[3:], want):
        assert r.tobytes() == w.tobytes() and f.tobytes() == lzw_ref.tiff_file(w)


def _ref_fish_render_tiff_batch(got):
    a, b, c = _sizes(PROBE)
    want = []
    for case, mask, pic in ((_render_case(a), _blobs(a) * np.uint8(255), None), (_render_case(b, 3), None, _picture(b)), (_render_case(c), None, None)):
        want += [lzw_ref.tiff_file(w) for w in _want_renders(case)] + [b'' if mask is None else lzw_ref.tiff_file(mask), b'' if pic is None else lzw_ref.tiff_file(pic)]
    assert [g.tobytes() for g in got] == want


def _ref_tiff_encode(got):
    assert got[0].tobytes() == lzw_ref.tiff_file(_picture(PROBE)) and got[1].tobytes() == lzw_ref.tiff_file(_gray(PROBE), invert=True)


def _ref_tiff_encode_batch(got):
    assert [g.tobytes() for g in got] == list(_tiff_files(PROBE))


def _ref_tiff_decode(got, n=2):
    """the rasters the files of tests/lzw_ref.py were written from (an inverted file holds 255 - raster)"""
    rasters, inverts = _tiff_rasters(PROBE)
    for g, r, v in list(zip(got, rasters, inverts))[:n]:
        assert g.dtype == np.uint8 and np.array_equal(g, 255 - r if v else r)


def _ref_tiff_decode_batch(got):
    _ref_tiff_decode(got, 3)


def _ref_png_labels_encode(got):
    from ecseg_amd import image_io
    labels = list(_label_stack(3, PROBE)) + [pl_cases.mixed(np.random.default_rng(5), *PROBE)]
    for g, lab in zip(got, labels):                          # (tests/test_gpu_png_encode.py: the host writer's file)
        assert g.tobytes() == _tmp_file(image_io.write_label_png, lab).tobytes()


def _ref_post_workspace(got):
    from oracle import postproc
    lab = _label_stack(2, PROBE)
    for i in range(2):
        assert np.array_equal(got[0][i], postproc.meta_inference(lab[i]))
        n, px = postproc.count_cc(lab[i] == 3)                # (px: float 0.0 where the reference has no count: -1 on the device)
        assert int(got[2][i]) == n and int(got[3][i]) == (-1 if isinstance(px, float) else px)


def _ref_nuclei_regions(got):
    """tests/test_gpu_interseg_kernels.py: the records, the crops and their channel maxima of oracle/interseg.py"""
    from oracle import interseg as oi
    lsq, seg = _fish_scene(PROBE)
    want, lab = oi.region_records((seg > 0).astype(np.uint8), lsq, 0)
    rec, crops, cmax = got
    assert len(want) > 1 and np.array_equal(rec, want)
    for k, r in enumerate(want[:6]):
        ref = oi.nucleus_crop(lsq, lab, k, int(r[1]), int(r[2]), int(min(r[3] - r[1], 256)), int(min(r[4] - r[2], 256)), order=(2, 0, 1))
        assert np.array_equal(crops[k], ref) and cmax[k].tolist() == ref.max(axis=(0, 1)).tolist(), k


def _ref_iseg_classifier_inputs(got):
    """tests/test_gpu_iseg_classify.py: (float)channel 0, and the host's preprocess_ecseg_c bit for bit"""
    from ecseg_amd import interseg
    crops, _ = _crop_stack(PROBE)
    k = len(crops)
    x_i, x_c = got
    assert np.array_equal(np.asarray(x_i).reshape(k, 256, 256), crops[..., 0].astype(np.float32))
    want = np.stack([interseg.preprocess_ecseg_c(crops[j]) for j in range(k - 1, -1, -1)]).astype(np.float32)
    assert np.asarray(x_c).shape == want.shape and np.asarray(x_c).view(np.uint32).tolist() == want.view(np.uint32).tolist()


def _ref_ccl_pass(got):
    """the comparison of tests/test_gpu_ccl_pass.py (ccl_pass_ref.check_pass)"""
    import ccl_pass_ref
    imgs = _label_stack(3, PROBE)
    labs = [ccl_pass_ref.Labelling(im, CCL_MODE.lut, CCL_MODE.conn) for im in imgs]
    ccl_pass_ref.check_pass(dict(zip(CCL_KEYS, got)), imgs, None, CCL_MODE, labs, [], 'scratch')


def _ref_png_channel_encode(got):
    from ecseg_amd import image_io
    px = _channel_pixels(PROBE)
    want = [_tmp_file(image_io.write_png_channel, px[i], ch, invert=inv) for ch, inv in ((0, True), (1, False)) for i in range(2)]
    assert [g.tobytes() for g in got] == [w.tobytes() for w in want]


def _ref_overlay_files(got):
    """the rows of oracle/overlay.py (tests/overlay_cases.py) and the host writer's red and green files of the 8-bit image"""
    import overlay_cases
    from ecseg_amd import csvio, image_io
    lab, img = _label_stack(2, PROBE), _overlay_images(PROBE)          # (v * 257 >> 8 = v: the 8-bit image is the picture)
    rows = np.asarray(got[0]).reshape(-1, 12)
    for i in range(2):
        assert overlay_cases.same_row(csvio.overlay_cells(rows[i]), overlay_cases.oracle_row(overlay_cases._case(lab[i], img[i], 120))), i
    want = [_tmp_file(image_io.write_png_channel, img[i], ch, invert=True) for ch in (0, 1) for i in range(2)]
    assert [g.tobytes() for g in got[1:]] == [w.tobytes() for w in want]


def _ref_meta_segment_files(got):
    """tests/test_gpu_metaseg_files.py: the host writers' files of the call's own gray and label images (the U-Net between the
    two has no exact CPU restatement)"""
    from ecseg_amd import image_io
    gray, post = got[0], got[1]
    for i in range(2):
        assert got[4 + i].tobytes() == _tmp_file(image_io.write_tiff_gray8, gray[i], invert=True).tobytes()
        assert got[6 + i].tobytes() == _tmp_file(image_io.write_label_png, post[i]).tobytes()


REFERENCES = {
    'nuclei_regions': _ref_nuclei_regions, 'iseg_classifier_inputs': _ref_iseg_classifier_inputs, 'ccl_pass': _ref_ccl_pass,
    'png_channel_encode': _ref_png_channel_encode, 'overlay_files': _ref_overlay_files, 'meta_segment_files': _ref_meta_segment_files,
    'fish_distances': _ref_fish_distances, 'fish_spots': _ref_fish_spots, 'min_cut': _ref_min_cut, 'rpn_proposals': _ref_rpn_proposals,
    'clean_nuclei': _ref_clean_nuclei, 'marker_watershed': _ref_marker_watershed, 'rescale_down': _ref_rescale_down,
    'rescale_mask_up': _ref_rescale_mask_up, 'stat_fish_batch': _ref_stat_fish_batch, 'min_cut_regions': _ref_min_cut_regions,
    'marker_watershed_batch': _ref_marker_watershed_batch, 'fish_render': _ref_fish_render, 'fish_render_tiff': _ref_fish_render_tiff,
    'fish_render_tiff_batch': _ref_fish_render_tiff_batch, 'tiff_encode': _ref_tiff_encode, 'tiff_encode_batch': _ref_tiff_encode_batch,
    'tiff_decode': _ref_tiff_decode, 'tiff_decode_batch': _ref_tiff_decode_batch, 'png_labels_encode': _ref_png_labels_encode,
    'post_workspace': _ref_post_workspace,
    # No CPU reference exists for classify_nucleus_crops, interseg_batch, nuset_forward and meta_segment_tiffs: float32 networks, which
    # their own modules hold to the host path on the device or to the oracle within a bound.  (meta_segment_tiffs is held below to
    # meta_segment on the samples the files were written from.)
}


@pytest.mark.parametrize('name', sorted(REFERENCES))
def test_the_fresh_answer_is_the_references(name):
    REFERENCES[name](_fresh_answer(name, PROBE))


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
