#!/usr/bin/env python3
"""``make stat_fish``: per-nucleus FISH spot statistics (reference src/stat_fish.py), everything behind ``nuclei_segment``.

The nucleus mask of every image comes from NuSeT on the device (config key ``nuset_weights``: ``NuSeT.segment`` on channel 0; with
``nuset_batch: k`` the sorted images are taken k at a time and their marker watersheds share one device call, ``NuSeT.segment_many`` -
the same files, k blue channels held at once) or, without
that key, is read from ``<masks>/<name>.tif`` (config key ``masks``, default ``<inpath>/nuclei_masks``):
any segmenter writing an 8-bit single-sample TIFF there, non-zero = nucleus, will do (NuSeT's weights come as an ``.npz``: TF1
checkpoints are not read).  Per image the nuclei are labelled on the device (``Handle.ccl_labels``, 8-connected,
skimage's order) - or, with ``use_min_cut: True``, labelled 4-connected and split by the min-cut splitter (src/max_flow_binary_mask.py
-> ecseg_amd/min_cut.py, whose maximum flows run on the device: ``Handle.min_cut``), which also adds the sixth file
``<name>_segmentation_corrected_min_cut.tif`` - and one more device call (``Handle.fish_spots`` -> ecseg_fish_spots, csrc/fishspot_kernels.hip) returns the
per-nucleus integers, the cleaned spot masks and the boundary drawing; the host computes the projected Gaussian kernel
(src/stat_fish.py:28-55) with numpy / scipy, forms the means as ``sum / count`` in float64 (exact: the sums are far below
2^53) and writes the five files per image and ``stat_fish_lsq.csv``; the three colour files of every image (``_original``,
``_original_with_segmentation``, ``_lsq_``) are composed by a third device call (``Handle.fish_render`` -> ecseg_fish_render), or by
``render`` in numpy on a handle without it - the same bytes.  ``make interseg`` and ``make fish_distance_calculation``
read the ``annotated/`` folder this leaves behind.

The parameters of the reference's ``src/stat_fish_params.yaml`` are built in (``DEFAULT_PARAMS``); a ``src/stat_fish_params.yaml``
in the working directory overrides them key by key.  The file, or the effective values when there is none, is copied into the
output folder.

The reference indexes its arrays as BGR (``cv2.imread``); the TIFF reader here returns RGB, so a TIFF's blue / green / red are
channels 2 / 1 / 0 and the indices are mapped, the image is not copied.  A ``.npy`` image is indexed as the reference indexes
it: channel 0 blue, 1 green, 2 red.

The third probe, aqua (:193): an ``(H, W, 4)`` uint8 / uint16 ``.npy`` image (blue, green, red, aqua) is taken when
``color_sensitivity`` has at least three entries.  Its probes are green, red and aqua, the "green and red" pair stays probes 0 and
1, the CSV gains the four aqua columns after red's (:280-284) and the ``_lsq_`` name its ``aq`` part (:291).  ``merge_channels``
(:110-115) folds the aqua channel into the colour files twice, with ``aqua_rgb = [233, 137, 54]``: into the image (:295), where
``coeff * I[..., -1]`` is a Python int times a uint8 array and wraps modulo 256 before ``/ 255``, so that a colour channel gains 1
where ``(coeff * aqua) & 255 == 255`` and the merge is almost a no-op (aqua 255 leaves blue 3 at 3; on an int copy it would become 57) -
the reference's behaviour, reproduced and not corrected, and ``_original.tif`` holds that merged image (:307); and into the ``_lsq_``
array (:297-299), an int array, where nothing wraps: an aqua spot adds (54, 137, 233) to (boundaries, green, red), lights all three
channels, and ``make fish_distance_calculation`` then reads it as green and red FISH - the reference's behaviour too, kept.  A
4-sample TIFF keeps losing its fourth sample, as ``cv2.imread`` drops it.

The NaN-scale branch (:238-240; ``scale: auto`` on an image without nuclei) yields an all-zero ``thresholded``: the device is
still called for regions, raw intensities and boundaries, with intensity thresholds of +infinity, which no pixel exceeds.

Divergences from the reference, all on inputs it crashes on or leaves to chance: images are processed in sorted order; a
per-image failure (missing mask, unreadable file, 4-channel image under a ``color_sensitivity`` of fewer than three entries - two entries cannot
broadcast over three probes in the reference either (:85) -, 16-bit TIFF - ``cv2.imread``'s internal 16-to-8 conversion cannot be pinned without
OpenCV -) is reported, skipped and turns the exit code to 1 while the other images' outputs are still written;
configuration errors exit with code 2; ``use_min_cut: True`` is one of them when the handle in use has no ``min_cut`` method (the
library's own ``Handle`` has it; the max_flow_binary_mask splitter needs its device call); integer CSV columns are always written as integers (pandas promotes them to
float when it concatenates an image without nuclei with others); in a folder that mixes 3- and 4-channel images the CSV has the aqua
columns as soon as one processed image had four channels, always after red's, and the rows of the 3-channel images leave those four
fields empty (the reference cannot run such a folder at all - three entries do not broadcast over a 3-channel image's two probes,
which here take the first two -; ``pd.concat`` puts the columns in order of first appearance, so that a leading 3-channel image moves the aqua columns
to the end, and would promote the aqua integer columns to float beside the missing values).  Kept as in the reference: with ``scale: auto`` the scale
of the FIRST image is used for every later image (:228 overwrites the variable).

A side effect on the process: ``main`` calls ``keep_freed_memory`` (glibc's ``mallopt``), so that the multi-megabyte arrays of one
image are recycled for the next instead of going back to the kernel between the device calls; ``ECSEG_MALLOC_DEFAULT=1`` switches
that off.
"""
import contextlib
import datetime
import math
import os
import shutil
import subprocess
import sys

import numpy as np

from .interseg import ImageError

DEFAULT_PARAMS = {
    'normal_threshold': 15,
    'color_sensitivity': [70, 70],
    'line_thickness': 2,
    'min_cc_size': 7,
    'gaussian_sigma': 3,
    'kernel_size': [7, 7],
    'target_median_nuclei_size': 2500,
    'cell_size_threshold_coeff': 1.25,
    'flow_limit': 60,
}
PARAMS_FILE = os.path.join('src', 'stat_fish_params.yaml')
PROBE_NAMES = ('green', 'red')                   # the probes every image has; a fourth channel adds THIRD_PROBE (:191-193)
THIRD_PROBE = 'aqua'
AQUA_BGR = (54, 137, 233)                        # aqua_rgb = [233, 137, 54] (:163) as merge_channels applies it, reversed
MAX_KERNEL = 63                # ECSEG_FISH_SPOT_MAX_KERNEL
MAX_LINE = 16                  # ECSEG_FISH_SPOT_MAX_LINE
MAX_DIST = 32                  # ECSEG_MIN_CUT_MAX_DIST


# the parameters of nuclei_segment in src/stat_fish_params.yaml, read only with the config key nuset_weights; scale_ratio: the
# reference's file says 0.3; the built-in default stays 1 (no rescale), any value in (0, 1] is taken from the file
NUSET_DEFAULT_PARAMS = {'min_score': 0.95, 'nms_threshold': 0.01, 'scale_ratio': 1}


class ConfigError(Exception):
    pass


def csv_columns(n_probe=2):
    """Column order of src/stat_fish.py:277-288; with ``n_probe=3`` the four aqua columns stand after red's (:280-284)."""
    cols = ['image_name', 'nucleus_center']
    for name in (PROBE_NAMES + (THIRD_PROBE,))[:n_probe]:
        cols += ['#_FISH_pixels (%s)' % name, '#_FISH_foci (%s)' % name, 'Avg fish intensity (%s)' % name,
                 'Max fish intensity (%s)' % name]
    return cols + ['#_DAPI_pixels', '#_FISH_pixels (green and red)', '#_FISH_foci (green and red)']


def sampled_gaussian_kernel(kernel_shape, sigma):
    """src/stat_fish.py:28-38: the normal density sampled at the distances from the kernel's centre, normalised to sum 1."""
    import scipy.stats
    shape = np.array(kernel_shape)
    centers = (shape / 2) - 0.5
    axis_y, axis_x = [np.arange(size) - center for size, center in zip(shape, centers)]
    grid = np.linalg.norm(np.dstack(np.meshgrid(axis_x, axis_y)), axis=2).astype(np.float64)
    gaussian = scipy.stats.norm.pdf(grid, scale=sigma)
    return gaussian / gaussian.sum()


def gaussian_proj_kernel(kernel_shape, sigma):
    """src/stat_fish.py:41-55 without the two trailing axes: the Gaussian kernel minus its projection on the constant kernel,
    scaled to unit norm.  A 1 x 1 kernel gives 0 / 0 = NaN (the device then finds no normal centre)."""
    g = sampled_gaussian_kernel(kernel_shape, sigma)
    c = np.ones(kernel_shape)
    c = c / np.linalg.norm(c)
    proj = np.dot(g.flatten(), c.flatten()) * c
    perp = g - proj
    with np.errstate(divide='ignore', invalid='ignore'):
        perp = perp / np.linalg.norm(perp)
    return perp


def derived_parameters(scale, params):
    """src/stat_fish.py:232-240 -> (gaussian_stdev, min_cc_size, kernel shape); three NaNs for a NaN scale."""
    if isinstance(scale, float) and math.isnan(scale):
        return float('nan'), float('nan'), float('nan')
    stdev = params['gaussian_sigma'] / scale
    min_cc = int(params['min_cc_size'] // (scale * scale))
    shape = [int(dim // scale) if (dim // scale % 2) else int(dim // scale) + 1 for dim in params['kernel_size']]
    return stdev, min_cc, shape


def lsq_name(img_name, params, stdev, min_cc):
    """src/stat_fish.py:291-292."""
    abbreviation = '_'.join('%s%s' % (letter, format(x, '.1f')) for letter, x in zip(['g', 'r', 'aq'], params['color_sensitivity']))
    return '%s_lsq_n%s_std%s_s%s_%s.tif' % (img_name, params['normal_threshold'], format(stdev, '.2f'), min_cc, abbreviation)


def with_segmentation(img, boundaries, green):
    """src/stat_fish.py:296, ``np.minimum(I + [b, -b, b], 255).astype(np.uint8)`` in BGR: on boundary pixels blue and red become
    255 and green becomes I - 255 wrapped to uint8, i.e. (I + 1) & 255.  ``green``: the index of the green channel."""
    out = np.array(img, np.uint8, copy=True)
    on = np.asarray(boundaries) != 0
    for c in range(3):
        out[..., c][on] = (out[..., c][on] + np.uint8(1)) if c == green else np.uint8(255)
    return out


def get_scale(areas, target_median_nuclei_size):
    """src/stat_fish.py:127-132; NaN without regions."""
    if not len(areas):
        return float('nan')
    return float(np.sqrt(target_median_nuclei_size / np.median(areas)))


def rows_from_records(img_name, records, n_probe=2):
    """CSV rows of one image from the records of ecseg_fish_spots (src/stat_fish.py:249-288), laid out as ``csv_columns(n_probe)``."""
    rows = []
    for r in np.asarray(records, np.int64).reshape(-1, 24).tolist():
        row = [img_name, '%d_%d' % (r[2] // r[1], r[3] // r[1])]
        for j in range(n_probe):
            pixels, foci, total, count, peak = r[4 + 5 * j:9 + 5 * j]
            row += [pixels, foci, (total / count) if count else 0.0, peak]
        rows.append(row + [r[1], r[19], r[20]])
    return rows


def widen_rows(rows):
    """Rows laid out as ``csv_columns(2)`` -> as ``csv_columns(3)``, the four aqua fields empty; rows that have them pass."""
    at, wide = 2 + 4 * len(PROBE_NAMES), len(csv_columns(3))
    return [r if len(r) == wide else r[:at] + [''] * 4 + r[at:] for r in rows]


def keep_freed_memory():
    """Tells glibc's allocator to keep what the process frees (``mallopt``: no trimming of the heap top, no ``mmap`` below 32 MiB, 256
    MiB of top padding) -> True when that was done.  Every image allocates and frees a dozen arrays of 1.4 - 6 MB around its device
    calls; with the default policy they come from and go back to the kernel each time, and unmapping memory the GPU runtime has just
    copied from or to makes the driver take the process's queues off the GPU and put them back about 10 ms later, which the next device
    call waits for (DESIGN.md 5.9 has the measurements).  With the arrays recycled inside the process that does not happen, and
    the page faults of fresh memory go as well.  The cost is that the process keeps its peak of freed memory (about 100 MB at 1040 x
    1392).  ``ECSEG_MALLOC_DEFAULT=1`` in the environment leaves the allocator alone; so does a C library without ``mallopt``."""
    import ctypes
    if os.environ.get('ECSEG_MALLOC_DEFAULT', '0') not in ('', '0'):
        return False
    try:
        mallopt = ctypes.CDLL(None).mallopt
    except (OSError, AttributeError):
        return False
    M_TRIM_THRESHOLD, M_TOP_PAD, M_MMAP_THRESHOLD = -1, -2, -3
    ok = [mallopt(M_TRIM_THRESHOLD, 2 ** 31 - 1), mallopt(M_TOP_PAD, 256 << 20), mallopt(M_MMAP_THRESHOLD, 32 << 20)]
    return all(v == 1 for v in ok)


def merge_aqua(bgr, aqua):
    """``merge_channels`` (:110-115) on the uint8 image as :295 calls it, in integers: ``coeff * aqua`` is a Python int times a uint8
    array and wraps modulo 256 before ``/ 255``, so a channel gains 1 where ``(coeff * aqua) & 255 == 255`` and nothing elsewhere,
    saturating at 255.  ``bgr``: the three (H, W) uint8 planes blue, green, red -> the three merged planes."""
    q = np.asarray(aqua).astype(np.int32)
    return [np.minimum(np.asarray(a).astype(np.int32) + (((k * q) & 255) == 255), 255).astype(np.uint8) for a, k in zip(bgr, AQUA_BGR)]


def render(img, channels, thresholded, boundaries):
    """The three colour files of :295-300,306-308 in numpy, what ``Handle.fish_render`` computes on the device: (H, W, C) uint8 image
    with ``channels`` = its (blue, green, red[, aqua]) indices, the (H, W, C - 1) masks and the (H, W) boundaries -> the RGB rasters
    (_original, _original_with_segmentation, _lsq_).  The _lsq_ merge runs on an int array in the reference and does not wrap:
    ``min(255, x + coeff * mask / 255)``."""
    bgr = [img[..., c] for c in channels[:3]]
    lsq = [boundaries, thresholded[..., 0], thresholded[..., 1]]
    if len(channels) > 3:
        bgr = merge_aqua(bgr, img[..., channels[3]])
        m = thresholded[..., 2].astype(np.int32)
        lsq = [np.minimum(x.astype(np.int32) + k * m // 255, 255).astype(np.uint8) for x, k in zip(lsq, AQUA_BGR)]
    original = np.stack(bgr[::-1], axis=-1)                  # the writers store RGB; cv2 writes its BGR arrays as RGB
    return original, with_segmentation(original, boundaries, 1), np.stack(lsq[::-1], axis=-1)


def read_image(path, handle, max_probes=2, tiff_read_on_device=False, pre=None, tiff_read_deflate=False):
    """-> ((H, W, C) uint8 image, its (blue, green, red[, aqua]) channel indices) (src/stat_fish.py:206-212).  C is 3, or 4 for a
    four-channel ``.npy`` when ``max_probes`` (the entries of ``color_sensitivity``) is at least 3.  ``tiff_read_on_device``: a TIFF's
    strips are decoded by ``handle.tiff_decode`` (``image_io.imread(path, handle=handle)``).  ``pre``: what ``image_io.imread_many``
    returned for the file, an array or the exception, when it was read ahead with its chunk (config key ``tiff_read_batch``).
    ``tiff_read_deflate`` (the config key, with ``tiff_read_on_device``): Deflate files count for the device reader too
    (``image_io.imread(path, handle=handle, deflate=True)``)."""
    from . import image_io
    try:
        if isinstance(pre, Exception):
            raise pre
        if pre is not None:
            I = pre
        elif tiff_read_on_device and tiff_read_deflate:
            I = image_io.imread(path, handle=handle, deflate=True)
        else:
            I = image_io.imread(path, handle=handle if tiff_read_on_device else None)
    except Exception as e:
        raise ImageError('cannot be read (%s)' % e)
    is_npy = path.lower().endswith('.npy')
    if is_npy:
        if I.ndim == 3 and I.shape[2] == 4 and I.dtype in (np.uint8, np.uint16) and max_probes >= 3:
            if I.dtype == np.uint16:
                I = handle.u16_to_u8(np.ascontiguousarray(I))
            return np.ascontiguousarray(I), (0, 1, 2, 3)
        if I.ndim != 3 or I.shape[2] != 3 or I.dtype not in (np.uint8, np.uint16):
            raise ImageError("isn't an (H, W, 3) uint8 / uint16 array (shape %s, %s); a fourth channel needs a third "
                             "color_sensitivity entry, which the reference cannot take either" % (I.shape, I.dtype))
        if I.dtype == np.uint16:
            I = handle.u16_to_u8(np.ascontiguousarray(I))
        return np.ascontiguousarray(I), (0, 1, 2)
    if I.dtype != np.uint8:
        raise ImageError('is a %s TIFF: only 8-bit TIFFs are read (the 16-to-8-bit conversion inside cv2.imread is not reproduced); '
                         'convert it, or store it as a uint16 .npy' % I.dtype)
    if I.ndim == 2:
        I = np.repeat(I[..., None], 3, axis=2)               # cv2.imread turns a gray file into three equal channels
    elif I.shape[2] == 1:
        I = np.repeat(I, 3, axis=2)
    elif I.shape[2] < 3:
        raise ImageError('has %d samples per pixel' % I.shape[2])
    elif I.shape[2] > 3:
        I = I[..., :3]                                       # cv2.imread drops the samples beyond three
    return np.ascontiguousarray(I), (2, 1, 0)


def read_mask(path, handle=None, pre=None, tiff_read_deflate=False):
    """``handle``: the mask's strips are decoded by ``handle.tiff_decode`` (config key ``tiff_read_on_device``).  ``pre``: as
    ``read_image``'s, and so is ``tiff_read_deflate``."""
    from . import image_io
    if not os.path.exists(path):
        raise ImageError('has no nucleus mask %s' % path)
    try:
        if isinstance(pre, Exception):
            raise pre
        if pre is not None:
            m = pre
        elif handle is not None and tiff_read_deflate:
            m = image_io.imread(path, handle=handle, deflate=True)
        else:
            m = image_io.imread(path, handle=handle)
    except Exception as e:
        raise ImageError('nucleus mask %s cannot be read (%s)' % (path, e))
    if m.ndim == 3 and m.shape[2] == 1:
        m = m[..., 0]
    if m.ndim != 2 or m.dtype != np.uint8:
        raise ImageError('nucleus mask %s is not an 8-bit single-sample image (shape %s, %s)' % (path, m.shape, m.dtype))
    return (m != 0).astype(np.uint8) * np.uint8(255)


def process_image(path, mask_path, out_root, params, scale, handle, stats=None, use_min_cut=False, segment=None, tiff_on_device=False,
                  tiff_read_on_device=False, pre_read=None, pending=None, tiff_read_deflate=False, min_cut_regions_on_device=False):
    """One image of src/stat_fish.py:199-308 -> (CSV rows, the scale that was used); the rows of a four-channel image carry the aqua
    fields of ``csv_columns(3)``, and ``stats['probes']`` becomes 3 once such an image was seen (it may have no nucleus and no row).  The three colour files come from ``handle.fish_render`` when the handle has it, else from
    ``render``, which writes the same bytes.  ``use_min_cut`` (:221-224): the label map comes
    from the min-cut splitter, already numbered 1..n (its cells need not be connected, which ecseg_fish_spots allows).  ``segment``
    (config key ``nuset_weights``): the mask is ``segment(blue channel)`` (:212-214) instead of the file ``mask_path``.
    ``tiff_on_device`` (the config key of that name): every TIFF of the image is LZW-encoded on the device - the colour files by
    ``handle.fish_render_tiff``, which renders them there too, the mask and the min-cut picture by ``handle.tiff_encode`` - and
    reaches the disk as the file image these return; the bytes are those of the host writers.  ``tiff_read_on_device`` (the config key
    of that name): the image and the mask are read with ``handle.tiff_decode`` where the device reader takes the file; the samples are
    those of the host readers; ``tiff_read_deflate`` (the config key of that name): Deflate files count for it too.  ``pre_read`` (config key ``tiff_read_batch``): ``(image, mask)`` as ``image_io.imread_many`` returned them
    for ``path`` and ``mask_path`` - an array, the exception, or None for "read it here" - when the files were read ahead with their chunk.
    ``pending`` (config key ``tiff_write_batch`` above 1, with ``tiff_on_device``): a list; instead of rendering and writing its TIFF
    files the image appends its pending TIFF work to it - the render inputs, the mask, the optional min-cut picture, the file names
    and its CSV rows - and returns no rows: ``main`` writes the files of k such images through one ``handle.fish_render_tiff_many``
    call and adds the rows once they are on disk.  The ``.npy`` file is written here as always.  A pending image holds its image,
    thresholded masks, boundaries and mask until then, 3 + 2 + 1 + 1 bytes per pixel: about 10.1 MB at 1040 x 1392 x 3 (8.7 MB without
    the mask; another 4.3 MB with the min-cut picture).  ``min_cut_regions_on_device`` (the config key of that name, with
    ``use_min_cut``): the splitter's labelling, selection and centres come from one ``handle.min_cut_regions`` call; same labels."""
    import time
    from . import image_io
    t0 = time.perf_counter()
    img_name = os.path.basename(path)[:-4]
    pre_image, pre_mask = pre_read if pre_read is not None else (None, None)
    I, channels = read_image(path, handle, len(params['color_sensitivity']), tiff_read_on_device, pre_image, tiff_read_deflate)
    blue = channels[0]
    mask = read_mask(mask_path, handle if tiff_read_on_device else None, pre_mask, tiff_read_deflate) if segment is None else segment(I[:, :, blue])
    imheight, imwidth = mask.shape
    I = np.ascontiguousarray(I[:imheight, :imwidth])
    mask = np.ascontiguousarray(mask[:I.shape[0], :I.shape[1]])
    if mask.size == 0:
        raise ImageError('is empty')
    t1 = time.perf_counter()
    probes = list(channels[1:])                              # green, red[, aqua]
    line = params['line_thickness']
    visualization = None
    try:
        if use_min_cut:
            from .min_cut import binary_seg_to_instance_min_cut
            labels, visualization = binary_seg_to_instance_min_cut(mask, params['flow_limit'], params['cell_size_threshold_coeff'], handle=handle,
                                                                   regions_on_device=min_cut_regions_on_device)
        else:
            labels = handle.ccl_labels(mask, 8)
        off = ([[0.0]], float('inf'), [float('inf')] * len(probes), 1)     # a call for the regions alone
        if scale == 'auto':
            rec, _, _ = handle.fish_spots(labels, I, probes, off[0], off[1], off[2], off[3], line)
            scale = get_scale(rec[:, 1], params['target_median_nuclei_size'])
        stdev, min_cc, shape = derived_parameters(scale, params)
        if isinstance(stdev, float) and math.isnan(stdev):
            rec, thr, bnd = handle.fish_spots(labels, I, probes, off[0], off[1], off[2], off[3], line)
        else:
            if shape[0] != shape[1] or shape[0] > MAX_KERNEL or shape[0] < 1:
                raise ImageError('needs a %s Gaussian kernel: the device takes square kernels up to %d x %d' % (shape, MAX_KERNEL, MAX_KERNEL))
            weights = gaussian_proj_kernel(shape, stdev)
            rec, thr, bnd = handle.fish_spots(labels, I, probes, weights, params['normal_threshold'], params['color_sensitivity'][:len(probes)],
                                              min_cc, line)
    except Exception as e:
        if getattr(e, 'code', None) == -1:
            raise ImageError(str(e))
        raise
    t2 = time.perf_counter()
    lut = np.zeros(labels.size + 1, np.int32)                 # label value -> dense rank (1 .. n), what skimage numbers them
    lut[rec[:, 0]] = np.arange(1, len(rec) + 1, dtype=np.int32)
    ranks = lut[labels]
    annotated_path = os.path.join(out_root, img_name)
    os.makedirs(annotated_path, exist_ok=True)
    if tiff_on_device and pending is not None:               # tiff_write_batch: the TIFF work is handed back, main() writes it with its chunk
        image_io.write_npy_int64(os.path.join(annotated_path, img_name + '__segmentation_min_cut.npy'), ranks)
        names = [img_name + '_original.tif', img_name + '_original_with_segmentation.tif', lsq_name(img_name, params, stdev, min_cc),
                 img_name + '_segmentation.tif', img_name + '_segmentation_corrected_min_cut.tif']
        picture = None if visualization is None else np.ascontiguousarray(visualization[..., ::-1])
        pending.append(dict(path=path, folder=annotated_path, names=names, item=(I, channels, thr, bnd, mask, picture),
                            rows=rows_from_records(img_name, rec, len(probes)), nuclei=len(rec), probes=len(probes)))
        if stats is not None:                                # (nuclei and probes count once the files are on disk: main() adds them)
            for key, v in (('read', t1 - t0), ('device', t2 - t1), ('write', time.perf_counter() - t2)):
                stats[key] = stats.get(key, 0.0) + v
        return [], scale
    if tiff_on_device:                                       # three file images instead of three rasters
        original, segmented, lsq = handle.fish_render_tiff(I, channels, thr, bnd)
    else:
        original, segmented, lsq = (handle.fish_render if hasattr(handle, 'fish_render') else render)(I, channels, thr, bnd)
    tiffs = [(img_name + '_segmentation.tif', mask), (img_name + '_original_with_segmentation.tif', segmented),
             (img_name + '_original.tif', original), (lsq_name(img_name, params, stdev, min_cc), lsq)]
    if visualization is not None:                            # (:304-305) cv2 writes its (r, g, b) array as if it were BGR: the file holds (b, g, r)
        tiffs.append((img_name + '_segmentation_corrected_min_cut.tif', np.ascontiguousarray(visualization[..., ::-1])))
    image_io.write_npy_int64(os.path.join(annotated_path, img_name + '__segmentation_min_cut.npy'), ranks)
    for name, what in tiffs:
        out = os.path.join(annotated_path, name)
        if tiff_on_device:
            image_io.write_file_image(out, what if isinstance(what, bytes) else handle.tiff_encode(what))
        elif what.ndim == 2:
            image_io.write_tiff_gray8(out, what)
        else:
            image_io.write_tiff_rgb8(out, what)
    if stats is not None:
        for key, v in (('read', t1 - t0), ('device', t2 - t1), ('write', time.perf_counter() - t2)):
            stats[key] = stats.get(key, 0.0) + v
        stats['nuclei'] = stats.get('nuclei', 0) + len(rec)
        stats['probes'] = max(stats.get('probes', len(PROBE_NAMES)), len(probes))
    return rows_from_records(img_name, rec, len(probes)), scale


def prepare_image(path, mask_path, out_root, params, scale, handle, stats=None, use_min_cut=False, segment=None, tiff_read_on_device=False,
                  pre_read=None, tiff_read_deflate=False, min_cut_regions_on_device=False):
    """The front half of ``process_image`` for ``stat_fish.batch`` above 1 -> (the image's share of a chunk, the scale that was used):
    the image and its mask are read (or segmented), the min-cut splitter runs when it is on, and the image's own parameters are worked
    out - with ``scale: auto`` from the areas of a regions-only ``fish_spots`` call, as ``process_image`` does.  Nothing is labelled,
    measured, rendered or written here: ``main`` hands the ``item`` of k images to one ``handle.stat_fish_many`` call.  Arguments and
    failures (``ImageError``) are ``process_image``'s.  A pending image holds its image, its mask (or label map) and the optional
    min-cut picture until its chunk runs: 3 + 1 bytes per pixel, 5.8 MB at 1040 x 1392 x 3 (4 more bytes per pixel with
    ``use_min_cut``, whose label map is int32, and 3 more for its picture)."""
    import time
    t0 = time.perf_counter()
    img_name = os.path.basename(path)[:-4]
    pre_image, pre_mask = pre_read if pre_read is not None else (None, None)
    I, channels = read_image(path, handle, len(params['color_sensitivity']), tiff_read_on_device, pre_image, tiff_read_deflate)
    mask = read_mask(mask_path, handle if tiff_read_on_device else None, pre_mask, tiff_read_deflate) if segment is None else segment(I[:, :, channels[0]])
    imheight, imwidth = mask.shape
    I = np.ascontiguousarray(I[:imheight, :imwidth])
    mask = np.ascontiguousarray(mask[:I.shape[0], :I.shape[1]])
    if mask.size == 0:
        raise ImageError('is empty')
    t1 = time.perf_counter()
    probes = list(channels[1:])
    labels = visualization = None
    off = ([[0.0]], float('inf'), [float('inf')] * len(probes), 1)
    try:
        if use_min_cut:
            from .min_cut import binary_seg_to_instance_min_cut
            labels, visualization = binary_seg_to_instance_min_cut(mask, params['flow_limit'], params['cell_size_threshold_coeff'], handle=handle,
                                                                   regions_on_device=min_cut_regions_on_device)
        if scale == 'auto':                                  # the areas come first: the weights depend on them
            rec, _, _ = handle.fish_spots(labels if use_min_cut else handle.ccl_labels(mask, 8), I, probes, off[0], off[1], off[2], off[3],
                                          params['line_thickness'])
            scale = get_scale(rec[:, 1], params['target_median_nuclei_size'])
    except Exception as e:
        if getattr(e, 'code', None) == -1:
            raise ImageError(str(e))
        raise
    stdev, min_cc, shape = derived_parameters(scale, params)
    if isinstance(stdev, float) and math.isnan(stdev):
        weights, normal, ithr, min_cc_used = off
    else:
        if shape[0] != shape[1] or shape[0] > MAX_KERNEL or shape[0] < 1:
            raise ImageError('needs a %s Gaussian kernel: the device takes square kernels up to %d x %d' % (shape, MAX_KERNEL, MAX_KERNEL))
        weights, normal, ithr, min_cc_used = gaussian_proj_kernel(shape, stdev), params['normal_threshold'], params['color_sensitivity'][:len(probes)], min_cc
    item = dict(img=I, channels=channels, weights=weights, normal_threshold=normal, intensity_thresholds=ithr, min_cc_size=min_cc_used)
    if use_min_cut:
        item.update(labels=labels, mask_file=mask)
        if visualization is not None:
            item['picture'] = np.ascontiguousarray(visualization[..., ::-1])
    else:
        item.update(mask=mask, mask_file=True)
    names = [img_name + '_original.tif', img_name + '_original_with_segmentation.tif', lsq_name(img_name, params, stdev, min_cc),
             img_name + '_segmentation.tif', img_name + '_segmentation_corrected_min_cut.tif']
    if stats is not None:
        for key, v in (('read', t1 - t0), ('device', time.perf_counter() - t1)):
            stats[key] = stats.get(key, 0.0) + v
    return dict(path=path, name=img_name, folder=os.path.join(out_root, img_name), names=names, item=item, probes=len(probes)), scale


def load_params():
    """DEFAULT_PARAMS overridden by a src/stat_fish_params.yaml in the working directory -> (params, path of that file or None)."""
    import yaml
    params = {k: (list(v) if isinstance(v, list) else v) for k, v in DEFAULT_PARAMS.items()}
    source = None
    if os.path.isfile(PARAMS_FILE):
        with open(PARAMS_FILE) as f:
            user = yaml.safe_load(f) or {}
        if not isinstance(user, dict):
            raise ConfigError('%s is not a mapping' % PARAMS_FILE)
        params.update({k: v for k, v in user.items() if k in DEFAULT_PARAMS})
        source = PARAMS_FILE

    def number(v):
        return isinstance(v, (int, float)) and not isinstance(v, bool)
    for key in ('normal_threshold', 'gaussian_sigma', 'min_cc_size', 'target_median_nuclei_size'):
        if not number(params[key]):
            raise ConfigError('%s must be a number' % key)
    cs = params['color_sensitivity']
    if not isinstance(cs, list) or len(cs) < len(PROBE_NAMES) or not all(number(v) for v in cs):
        raise ConfigError('color_sensitivity must be a list of at least %d numbers' % len(PROBE_NAMES))
    ks = params['kernel_size']
    if not isinstance(ks, list) or len(ks) != 2 or not all(number(v) and v > 0 for v in ks):
        raise ConfigError('kernel_size must be a list of two positive numbers')
    if not number(params['cell_size_threshold_coeff']) or not params['cell_size_threshold_coeff'] >= 0:
        raise ConfigError('cell_size_threshold_coeff must be a non-negative number')
    fl = params['flow_limit']
    if not number(fl) or not fl >= 0 or math.isinf(fl) or not 1 <= (-1 + int(math.sqrt(1 + 2 * fl))) // 2 <= MAX_DIST:
        raise ConfigError('flow_limit must give a distance (-1 + int(sqrt(1 + 2 * flow_limit))) // 2 between 1 and %d (flow_limit 4 .. 2243)'
                          % MAX_DIST)
    lt = params['line_thickness']
    if isinstance(lt, bool) or not isinstance(lt, int) or not 1 <= lt <= MAX_LINE:
        raise ConfigError('line_thickness must be an integer between 1 and %d' % MAX_LINE)
    return params, source


def load_nuset_segmenter(var, handle):
    """The config key ``nuset_weights`` ([whole.npz, foreground.npz], or one path for both passes; optional ``nuset_base``, default
    64) -> ``segment(blue)`` = ``NuSeT.segment`` with ``min_score`` / ``nms_threshold`` / ``scale_ratio`` of src/stat_fish_params.yaml and
    ``nuclei_size_T`` of the config.  ``scale_ratio`` other than 1 must lie in (0, 1) and needs a handle with ``rescale_down`` and
    ``rescale_mask_up``; an image smaller than 16 x 16 after scaling is reported as that image's failure.  Every other problem is a
    ConfigError."""
    import yaml
    from . import nuset
    paths = var['nuset_weights']
    paths = [paths] if isinstance(paths, str) else paths
    if not isinstance(paths, list) or len(paths) not in (1, 2) or not all(isinstance(p, str) for p in paths):
        raise ConfigError('nuset_weights must be one .npz path or a list of two (whole-image and foreground checkpoint)')
    prm = dict(NUSET_DEFAULT_PARAMS)
    if os.path.isfile(PARAMS_FILE):
        with open(PARAMS_FILE) as f:
            user = yaml.safe_load(f) or {}
        if isinstance(user, dict):
            prm.update({k: v for k, v in user.items() if k in prm})
    for k, v in prm.items():
        if isinstance(v, bool) or not isinstance(v, (int, float)) or math.isnan(v):
            raise ConfigError('%s must be a number' % k)
    if prm['scale_ratio'] != 1:
        if not 0 < prm['scale_ratio'] <= 1 or math.isinf(prm['scale_ratio']):
            raise ConfigError('scale_ratio: %s with nuset_weights: only values in (0, 1] are built (above 1 the second rescale of '
                              'nuclei_segment Gaussian-filters the 0 / 1 uint8 mask into almost nothing)' % prm['scale_ratio'])
        if handle is not None and not all(hasattr(handle, m) for m in ('rescale_down', 'rescale_mask_up')):
            raise ConfigError('scale_ratio: %s with nuset_weights needs the rescale step of nuclei_segment (rescale_down, rescale_mask_up), '
                              'which the handle in use does not have; only scale_ratio: 1 works on it' % prm['scale_ratio'])
    size_t = var['nuclei_size_T']
    if isinstance(size_t, bool) or not isinstance(size_t, int) or size_t < 0:
        raise ConfigError('nuclei_size_T must be a non-negative integer')
    base = var.get('nuset_base', 64)
    if isinstance(base, bool) or not isinstance(base, int) or base < 1:
        raise ConfigError('nuset_base must be a positive integer')
    if handle is not None and not all(hasattr(handle, m) for m in ('marker_watershed', 'clean_nuclei', 'nuset_forward', 'rpn_proposals_last')):
        raise ConfigError('nuset_weights needs NuSeT\'s device calls (nuset_forward, rpn_proposals_last, marker_watershed, clean_nuclei), which '
                          'the handle in use does not have')
    weights = []
    for p in paths:
        try:
            weights.append(nuset.load_weights_npz(p, base))
        except Exception as e:
            raise ConfigError('nuset_weights: %s cannot be used (%s)' % (p, e))
    state = {}

    def segment(blue, handle):
        if 'nets' not in state:
            state['nets'] = [nuset.NuSeT(w, base, handle=handle) for w in weights]
        nets = state['nets']
        second = nets[-1] if len(nets) > 1 else None
        if prm['scale_ratio'] == 1:
            return nets[0].segment(blue, prm['min_score'], prm['nms_threshold'], size_t, second=second)
        try:
            return nets[0].segment(blue, prm['min_score'], prm['nms_threshold'], size_t, second=second, scale_ratio=prm['scale_ratio'])
        except ValueError as e:                              # e.g. smaller than 16 x 16 after scaling: this image only
            raise ImageError(str(e))

    def segment_many(blues, handle):
        """``[segment(b, handle) for b in blues]`` through ``NuSeT.segment_many`` (config key ``nuset_batch``); what ``segment`` would
        raise for one image stands in its place, as the exception ``segment`` raises."""
        if 'nets' not in state:
            state['nets'] = [nuset.NuSeT(w, base, handle=handle) for w in weights]
        nets = state['nets']
        out = nets[0].segment_many(blues, prm['min_score'], prm['nms_threshold'], size_t, second=nets[-1] if len(nets) > 1 else None,
                                   scale_ratio=prm['scale_ratio'])
        return [ImageError(str(m)) if isinstance(m, ValueError) and prm['scale_ratio'] != 1 else m for m in out]
    segment.many = segment_many
    return segment


def current_commit():
    """src/stat_fish.py:186: the last word of ``git log -1 | head -1``; empty without git."""
    try:
        out = subprocess.run('git log -1 | head -1', shell=True, capture_output=True).stdout.decode()
    except OSError:
        return ''
    return out.strip().split(' ')[-1]


def main(argv=None, handle=None):
    """``make stat_fish``.  Like the reference's ``main`` it takes everything from section ``stat_fish`` of ``config.yaml`` in
    the working directory; ``argv`` is accepted for the shim's sake and not read.  ``handle`` is an injection point for tests and
    tools (anything with ``Handle.ccl_labels``, ``fish_spots`` and ``u16_to_u8``, and ``min_cut`` for ``use_min_cut: True``; ``fish_render``
    is used when it is there, ``tiff_encode`` and ``fish_render_tiff`` are needed for ``tiff_on_device: true``, ``tiff_decode`` for
    ``tiff_read_on_device: true``, ``tiff_decode_many`` too for ``tiff_read_batch`` above 1, ``tiff_encode_many`` and
    ``fish_render_tiff_many`` for ``tiff_write_batch`` above 1); without it the call opens a handle on device 0 and closes it at the end.

    ``tiff_write_batch: k`` (with ``tiff_on_device: true``; default 1): the TIFF files of k images are rendered and encoded by one
    ``handle.fish_render_tiff_many`` call - ``process_image`` hands its TIFF work back (its docstring says what an image holds until
    then) and the files are written every k such images and at the end.  The files, their names, the CSV and the messages are those of
    k = 1.  An image's CSV rows are added once its files are on disk; where such a call or a write fails, every image of that chunk is
    reported as not processed (exit code 1, no rows), the other chunks are unaffected, and an image that failed earlier is in no chunk.

    ``batch: k`` (with ``tiff_on_device: true``; default 1; above 1 ``tiff_write_batch`` is ignored): the images are read and prepared
    one by one (``prepare_image``) and k of them are labelled, measured, rendered and encoded by one ``handle.stat_fish_many`` call,
    which returns the dense ranks (the ``.npy``), the records and the file images.  Files, names, CSV, messages and exit code are those
    of k = 1; a chunk whose call fails reports each of its images, by the rule above."""
    import yaml
    from . import csvio
    from .utils import get_imgs
    try:
        with open('config.yaml') as infile:
            var = (yaml.safe_load(infile) or {}).get('stat_fish')
        if not isinstance(var, dict):
            raise ConfigError('config.yaml has no stat_fish section')
        for key in ('inpath', 'scale', 'use_min_cut', 'nuclei_size_T'):       # nuclei_size_T belongs to nuclei_segment: accepted, unused
            if key not in var:
                raise ConfigError('config.yaml: stat_fish has no key %s' % key)
        inpath = str(var['inpath'])
        if not os.path.isdir(inpath):
            raise ConfigError('Input folder does not exist. Exiting...')
        use_min_cut = bool(var['use_min_cut'])
        if use_min_cut and handle is not None and not hasattr(handle, 'min_cut'):
            raise ConfigError('use_min_cut: True needs the min-cut splitter (src/max_flow_binary_mask.py), whose device call the handle in use '
                              'does not have: set use_min_cut: False in config.yaml')
        regions_on_device = var.get('min_cut_regions_on_device', False)
        if not isinstance(regions_on_device, bool):
            raise ConfigError('min_cut_regions_on_device must be true or false (true, with use_min_cut: the labelling, the selection and the '
                              'centres of the min-cut splitter come from one device call)')
        regions_on_device = regions_on_device and use_min_cut        # ignored without the splitter
        if regions_on_device and handle is not None and not hasattr(handle, 'min_cut_regions'):
            raise ConfigError('min_cut_regions_on_device: true needs the device call min_cut_regions, which the handle in use does not have; '
                              'only min_cut_regions_on_device: false works on it')
        scale = var['scale']
        if scale != 'auto' and (isinstance(scale, bool) or not isinstance(scale, (int, float)) or not scale > 0 or math.isinf(scale)):
            raise ConfigError('scale must be a positive number or "auto"')
        masks = str(var['masks']) if var.get('masks') is not None else os.path.join(inpath, 'nuclei_masks')
        segmenter = load_nuset_segmenter(var, handle) if var.get('nuset_weights') is not None else None
        batch = var.get('nuset_batch', 1) if segmenter is not None else 1
        if isinstance(batch, bool) or not isinstance(batch, int) or batch < 1:
            raise ConfigError('nuset_batch must be a positive integer (how many images share one marker-watershed call; 1: one by one)')
        if batch > 1 and handle is not None and not hasattr(handle, 'marker_watershed_batch'):
            raise ConfigError('nuset_batch: %d needs the batched marker watershed (marker_watershed_batch), which the handle in use does not '
                              'have; only nuset_batch: 1 works on it' % batch)
        tiff_on_device = var.get('tiff_on_device', False)
        if not isinstance(tiff_on_device, bool):
            raise ConfigError('tiff_on_device must be true or false (true: the LZW strips of every TIFF are encoded on the device)')
        if tiff_on_device and handle is not None and not all(hasattr(handle, m) for m in ('tiff_encode', 'fish_render_tiff')):
            raise ConfigError('tiff_on_device: true needs the device TIFF encoder (tiff_encode, fish_render_tiff), which the handle in use '
                              'does not have; only tiff_on_device: false works on it')
        tiff_read_on_device = var.get('tiff_read_on_device', False)
        if not isinstance(tiff_read_on_device, bool):
            raise ConfigError('tiff_read_on_device must be true or false (true: the strips of every input TIFF are decoded on the device)')
        if tiff_read_on_device and handle is not None and not hasattr(handle, 'tiff_decode'):
            raise ConfigError('tiff_read_on_device: true needs the device TIFF reader (tiff_decode), which the handle in use '
                              'does not have; only tiff_read_on_device: false works on it')
        read_batch = var.get('tiff_read_batch', 1)
        if isinstance(read_batch, bool) or not isinstance(read_batch, int) or read_batch < 1:
            raise ConfigError('tiff_read_batch must be a positive integer (how many images, with their masks, are read in one call of the '
                              'device TIFF reader; 1: one by one)')
        if not tiff_read_on_device:
            read_batch = 1                                   # the key belongs to the device reader
        if read_batch > 1 and handle is not None and not hasattr(handle, 'tiff_decode_many'):
            raise ConfigError('tiff_read_batch: %d needs the batched device TIFF reader (tiff_decode_many), which the handle in use does not '
                              'have; only tiff_read_batch: 1 works on it' % read_batch)
        read_deflate = var.get('tiff_read_deflate', False)
        if not isinstance(read_deflate, bool):
            raise ConfigError('tiff_read_deflate must be true or false (true, with tiff_read_on_device: Deflate input TIFFs count for the device reader too)')
        if not tiff_read_on_device:
            read_deflate = False                             # the key belongs to the device reader
        read_tiled = var.get('tiff_read_tiled', False)
        if not isinstance(read_tiled, bool):
            raise ConfigError('tiff_read_tiled must be true or false (true, with tiff_read_on_device: tiled input TIFFs count for the device reader too)')
        if not tiff_read_on_device:
            read_tiled = False                               # the key belongs to the device reader
        if read_tiled and handle is not None and not hasattr(handle, 'set_option'):
            raise ConfigError('tiff_read_tiled: true needs a handle with options (set_option), which the handle in use does not have; only '
                              'tiff_read_tiled: false works on it')
        read_packbits = var.get('tiff_read_packbits', False)
        if not isinstance(read_packbits, bool):
            raise ConfigError('tiff_read_packbits must be true or false (true, with tiff_read_on_device: PackBits input TIFFs count for the device reader too)')
        if not tiff_read_on_device:
            read_packbits = False                            # the key belongs to the device reader
        if read_packbits and handle is not None and not hasattr(handle, 'set_option'):
            raise ConfigError('tiff_read_packbits: true needs a handle with options (set_option), which the handle in use does not have; only '
                              'tiff_read_packbits: false works on it')
        write_batch = var.get('tiff_write_batch', 1)
        if isinstance(write_batch, bool) or not isinstance(write_batch, int) or write_batch < 1:
            raise ConfigError('tiff_write_batch must be a positive integer (how many images have their TIFF files encoded in one call of the '
                              'device TIFF encoder; 1: one by one)')
        if not tiff_on_device:
            write_batch = 1                                  # the key belongs to the device encoder
        fish_batch = var.get('batch', 1)
        if isinstance(fish_batch, bool) or not isinstance(fish_batch, int) or fish_batch < 1:
            raise ConfigError('batch must be a positive integer (how many images are labelled, measured, rendered and encoded in one device '
                              'call; 1: one by one)')
        if not tiff_on_device:
            fish_batch = 1                                   # the key belongs to the device encoder: the chunk's files are encoded in its call
        if fish_batch > 1:
            write_batch = 1                                  # ... and there is nothing left for tiff_write_batch to batch
            if handle is not None and not hasattr(handle, 'stat_fish_many'):
                raise ConfigError('batch: %d needs the batched stat_fish call (stat_fish_many), which the handle in use does not have; only '
                                  'batch: 1 works on it' % fish_batch)
        if write_batch > 1 and handle is not None and not all(hasattr(handle, m) for m in ('tiff_encode_many', 'fish_render_tiff_many')):
            raise ConfigError('tiff_write_batch: %d needs the batched device TIFF encoder (tiff_encode_many, fish_render_tiff_many), which the '
                              'handle in use does not have; only tiff_write_batch: 1 works on it' % write_batch)
        if segmenter is None and not os.path.isdir(masks):
            raise ConfigError('The folder of nucleus masks %s does not exist (config key masks): it holds one 8-bit <name>.tif per '
                              'image, non-zero = nucleus' % masks)
        params, params_source = load_params()
        image_paths = get_imgs(inpath)
        if not image_paths:
            raise ConfigError('No .tif / .npy images in the input folder. Exiting...')    # the reference crashes in pd.concat
    except ConfigError as e:
        print(e)
        sys.exit(2)

    output_folder = 'tmp_' + datetime.datetime.now().strftime('%m-%d_%H:%M:%S')
    out_root = os.path.join(inpath, output_folder)
    os.makedirs(out_root, exist_ok=True)
    shutil.copyfile('config.yaml', os.path.join(out_root, 'config_%s.yaml' % current_commit()))
    if params_source:
        shutil.copyfile(params_source, os.path.join(out_root, 'stat_fish_params.yaml'))
    else:
        with open(os.path.join(out_root, 'stat_fish_params.yaml'), 'w') as f:
            yaml.safe_dump(params, f)

    own = handle is None
    if own:
        from ._lib import Handle
        handle = Handle(0)
    keep_freed_memory()
    from ._lib import tiff_options
    options = contextlib.ExitStack()                         # image_io.imread / imread_many read the two options off the handle
    options.enter_context(tiff_options(handle, tiled=read_tiled or None, packbits=read_packbits or None))
    rows, failed, seen = [], [], {}
    mask_of = lambda p: os.path.join(masks, os.path.basename(p)[:-4] + '.tif')
    ahead = {}                                               # tiff_read_batch: image path -> (image, mask) read with its chunk, until the image is done

    def read_ahead(k):                                       # image k opens a chunk of read_batch images: their files, and their masks where those are files, in one call
        if read_batch == 1 or k % read_batch:
            return
        import time
        from . import image_io
        chunk = image_paths[k:k + read_batch]
        files = chunk + ([mask_of(p) for p in chunk if os.path.exists(mask_of(p))] if segmenter is None else [])
        t0 = time.perf_counter()
        got = dict(zip(files, image_io.imread_many(files, handle=handle, deflate=True) if read_deflate else image_io.imread_many(files, handle=handle)))
        seen['read'] = seen.get('read', 0.0) + time.perf_counter() - t0
        for p in chunk:
            ahead[p] = (got[p], got.get(mask_of(p)) if segmenter is None else None)

    def handed_in(mask):                                     # the `segment` hook of process_image for a mask computed with its chunk
        def segment(blue):
            if isinstance(mask, Exception):
                raise mask
            return mask
        return segment
    pending = [] if write_batch > 1 else None                # tiff_write_batch: the TIFF work of the images whose files are not on disk yet

    def flush():                                             # their TIFF files through one call, then their rows; a failure is every such image's
        if not pending:
            return
        import time
        from . import image_io
        t0 = time.perf_counter()
        chunk = list(pending)
        del pending[:]
        try:
            for w, files in zip(chunk, handle.fish_render_tiff_many([w['item'] for w in chunk])):
                for name, data in zip(w['names'], files):
                    if data is not None:
                        image_io.write_file_image(os.path.join(w['folder'], name), data)
        except Exception as e:
            if getattr(e, 'code', None) != -1 and not isinstance(e, OSError):
                raise
            for w in chunk:
                print(w['path'], '-', 'its TIFF files could not be written (%s)' % e)
                failed.append((w['path'], 'its TIFF files could not be written (%s)' % e))
            return
        finally:
            seen['write'] = seen.get('write', 0.0) + time.perf_counter() - t0
        for w in chunk:
            rows.extend(w['rows'])
            seen['nuclei'] = seen.get('nuclei', 0) + w['nuclei']
            seen['probes'] = max(seen.get('probes', len(PROBE_NAMES)), w['probes'])
    held = []                                                # stat_fish.batch: the images prepared for the next stat_fish_many call

    def run_chunk():                                         # one device call for the held images, then their files and rows; a failed call is every such image's
        if not held:
            return
        import time
        from . import image_io
        t0 = time.perf_counter()
        chunk = list(held)
        del held[:]
        try:
            results = handle.stat_fish_many([w['item'] for w in chunk], params['line_thickness'])
            t1 = time.perf_counter()
            seen['device'] = seen.get('device', 0.0) + t1 - t0
            for w, res in zip(chunk, results):
                if isinstance(res, Exception):               # the binding refused this image alone
                    print(w['path'], '-', res)
                    failed.append((w['path'], str(res)))
                    continue
                ranks, rec, files = res
                os.makedirs(w['folder'], exist_ok=True)
                image_io.write_npy_int64(os.path.join(w['folder'], w['name'] + '__segmentation_min_cut.npy'), ranks)
                for name, data in zip(w['names'], files):
                    if data is not None:
                        image_io.write_file_image(os.path.join(w['folder'], name), data)
                w['rows'], w['nuclei'] = rows_from_records(w['name'], rec, w['probes']), len(rec)
            seen['write'] = seen.get('write', 0.0) + time.perf_counter() - t1
        except Exception as e:
            if getattr(e, 'code', None) != -1 and not isinstance(e, OSError):
                raise
            for w in chunk:
                if 'rows' in w:
                    del w['rows']
                if not any(w['path'] == f[0] for f in failed):
                    print(w['path'], '-', 'its chunk could not be processed (%s)' % e)
                    failed.append((w['path'], 'its chunk could not be processed (%s)' % e))
            return
        for w in chunk:
            if 'rows' in w:
                rows.extend(w['rows'])
                seen['nuclei'] = seen.get('nuclei', 0) + w['nuclei']
                seen['probes'] = max(seen.get('probes', len(PROBE_NAMES)), w['probes'])
    try:
        for at in range(0, len(image_paths), batch):
            chunk = image_paths[at:at + batch]
            hooks = {}
            if segmenter is not None and batch == 1:
                hooks[chunk[0]] = lambda blue: segmenter(blue, handle)
            elif segmenter is not None:                      # nuset_batch: the chunk's blue channels (and nothing else of them) are held at once
                blues = []
                for k, p in enumerate(chunk, at):
                    try:
                        read_ahead(k)
                        I, channels = read_image(p, handle, len(params['color_sensitivity']), tiff_read_on_device, ahead.get(p, (None, None))[0], read_deflate)
                        blues.append((p, np.ascontiguousarray(I[:, :, channels[0]])))
                    except ImageError as e:
                        hooks[p] = handed_in(e)              # (process_image meets and reports it at the image's turn)
                    I = None
                for (p, _), m in zip(blues, segmenter.many([b for _, b in blues], handle)):
                    hooks[p] = handed_in(m)
                blues = None
            for k, p in enumerate(chunk, at):
                print("Processing image: ", p)
                try:
                    if p not in ahead:
                        read_ahead(k)
                    if fish_batch > 1:
                        work, scale = prepare_image(p, mask_of(p), out_root, params, scale, handle, stats=seen, use_min_cut=use_min_cut,
                                                    segment=hooks.get(p), tiff_read_on_device=tiff_read_on_device, pre_read=ahead.pop(p, None),
                                                    tiff_read_deflate=read_deflate, min_cut_regions_on_device=regions_on_device)
                        held.append(work)
                        if len(held) >= fish_batch:
                            run_chunk()
                        continue
                    img_rows, scale = process_image(p, mask_of(p), out_root, params, scale, handle,
                                                     stats=seen, use_min_cut=use_min_cut, segment=hooks.get(p), tiff_on_device=tiff_on_device,
                                                     tiff_read_on_device=tiff_read_on_device, pre_read=ahead.pop(p, None), pending=pending,
                                                     tiff_read_deflate=read_deflate, min_cut_regions_on_device=regions_on_device)
                    rows += img_rows
                except ImageError as e:
                    print(p, '-', e)
                    failed.append((p, str(e)))
                if pending is not None and len(pending) >= write_batch:
                    flush()
        flush()
        run_chunk()
    finally:
        options.close()                                      # a handle that was handed in goes back as it came
        if own:
            handle.close()
    with open(os.path.join(out_root, 'stat_fish_lsq.csv'), 'w') as f:
        n_probe = seen.get('probes', len(PROBE_NAMES))
        f.write(csvio.csv_text(csv_columns(n_probe), widen_rows(rows) if n_probe == 3 else rows))

    annotated = os.path.join(inpath, 'annotated')
    if os.path.isdir(annotated):
        old = annotated + '_' + str(datetime.datetime.now())[5:-10].replace(' ', '-')
        k, target = 1, old
        while os.path.exists(target):                        # a second run within the minute: the reference's rename fails here
            k += 1
            target = '%s_%d' % (old, k)
        os.rename(annotated, target)
    os.rename(out_root, annotated)
    failed.sort(key=lambda f: image_paths.index(f[0]))      # (folder order also where a flush of tiff_write_batch reported its images late)
    if failed:
        print("%d image(s) were NOT processed and are missing from the CSV:" % len(failed))
        for p, why in failed:
            print("  ", p, "-", why)
        sys.exit(1)             # the reference would have crashed on the first such image


if __name__ == "__main__":
    main(sys.argv[1:])
