#!/usr/bin/env python3
"""``make fish_distance_calculation``: the normalised distance between the FISH probe and the centromere probe of every
nucleus (reference src/fish_distance_calculation.py), from the ``annotated/`` folder stat_fish leaves behind.

Per image the per-nucleus integers come from one device call (``Handle.fish_distances`` -> ecseg_fish_distances,
csrc/fishdist_kernels.hip); the host applies the reference's gate and spot limit and takes the two square roots:
``sqrt(min squared distance) / sqrt(area)`` in float64 is bit-identical to the reference's
``np.linalg.norm(...).min() / np.sqrt(area)`` because sqrt is monotone and correctly rounded, so the minimum of the roots
is the root of the (exact, integer) minimum.

Divergences from the reference, all on inputs it crashes on or leaves to chance: images are processed in sorted order
(the reference: directory order) and of several ``<name>_lsq*.tif`` the first in sorted order is read; a per-image
failure is reported, skipped and turns the exit code to 1 while the CSV is still written; configuration errors exit
with code 2 and a message.

Optional config keys: ``batch: k`` (default 1) takes the sorted images k at a time: their files are read and prepared on
``io_threads`` reader threads (default: the host's CPU budget, as ``meta_overlay`` takes the key) and ONE device call,
``Handle.fish_distances_many`` -> ecseg_fish_distances_batch, measures the chunk.  The printed lines and their order, the CSV, the
failed images and the exit code are those of ``batch: 1``; an image that fails, fails alone.
"""
import glob
import math
import os
import sys
import time

import numpy as np

from .interseg import ImageError

COLOR_TO_INDEX = {'red': 0, 'green': 1, 'blue': 2}
CSV_COLUMNS = ['normalized_distance']


def distances_from_records(records, max_centromeric_spots):
    """The values of get_distances_img (src/fish_distance_calculation.py:19-45) from the records of ecseg_fish_distances:
    a cell counts when both gate bits are set (:21) and it has at most ``max_centromeric_spots`` FISH spots (:31); its value
    is inf without FISH pixels (:42), else sqrt(min squared distance) / sqrt(area) (:39).  FISH pixels without any centromere
    pixel - where the reference dies in ``.min()`` of an empty array - raise ImageError."""
    out = []
    for r in np.asarray(records, np.int64).reshape(-1, 8).tolist():
        if r[2] != 3 or r[5] > max_centromeric_spots:
            continue
        if r[3] == 0:
            out.append(float('inf'))
        elif r[4] == 0:
            raise ImageError('nucleus %d has FISH pixels but no centromere pixel (the reference fails here too)' % r[0])
        else:
            out.append(math.sqrt(r[6]) / math.sqrt(r[1]))
    return out


def prepare_image(lsq, segmentation, presets):
    """What get_distances_img does before the device call: the checks, the renumbering by rank of a map whose labels exceed H * W and
    the int32 cast -> (labels int32 (H, W), lsq uint8 (H, W, C)), both contiguous, or None for an empty map (no value)."""
    centromere_probe_index, fish_probe_index, max_centromeric_spots = presets
    seg = np.asarray(segmentation)
    lsq = np.asarray(lsq)
    if seg.ndim != 2 or seg.dtype.kind not in 'iu':
        raise ImageError('segmentation is not a 2-D integer label map (shape %s, %s)' % (seg.shape, seg.dtype))
    if lsq.ndim != 3 or lsq.dtype != np.uint8:
        raise ImageError("lsq image isn't an 8-bit multi-channel image (shape %s, %s)" % (lsq.shape, lsq.dtype))
    need = max(centromere_probe_index, fish_probe_index, 1) + 1
    if lsq.shape[2] < need:
        raise ImageError('lsq image has %d channel(s), %d are needed' % (lsq.shape[2], need))
    if lsq.shape[:2] != seg.shape:
        raise ImageError('lsq image (%d x %d) and segmentation (%d x %d) differ in size' % (lsq.shape[:2] + seg.shape))
    if seg.size == 0:
        return None
    if int(seg.max()) > seg.size:
        # ranks keep the ascending order regionprops walks in; the device call takes labels 1 .. H * W
        values, inverse = np.unique(seg, return_inverse=True)
        rank = np.cumsum(values > 0)
        seg = np.where(values > 0, rank, 0)[inverse.reshape(seg.shape)]
    return np.ascontiguousarray(np.where(seg > 0, seg, 0), np.int32), np.ascontiguousarray(lsq)


def get_distances_img(lsq, segmentation, presets, handle):
    """src/fish_distance_calculation.py:16-46 for one image; presets = (centromere_probe_index, fish_probe_index,
    max_centromeric_spots); ``handle``: a ``_lib.Handle`` (or anything with its ``fish_distances``)."""
    centromere_probe_index, fish_probe_index, max_centromeric_spots = presets
    prepared = prepare_image(lsq, segmentation, presets)
    if prepared is None:
        return []
    try:
        rec = handle.fish_distances(prepared[0], prepared[1], fish_probe_index, centromere_probe_index)
    except Exception as e:
        if getattr(e, 'code', None) == -1:
            raise ImageError(str(e))
        raise
    return distances_from_records(rec, max_centromeric_spots)


def load_image(root_directory, img_path):
    """(lsq, segmentation) of one ``<inpath>/<name>.tif`` (src/fish_distance_calculation.py:51-60)."""
    from . import image_io
    img_name = os.path.basename(img_path)[:-4]
    img_directory = os.path.join(root_directory, 'annotated', img_name)
    if not os.path.isdir(img_directory):
        raise ImageError('has no folder annotated/%s (run stat_fish first)' % img_name)
    segmentation_path = os.path.join(img_directory, img_name + '__segmentation_min_cut.npy')
    lsq_paths = sorted(glob.glob(os.path.join(glob.escape(img_directory), glob.escape(img_name) + '_lsq*.tif')))
    if not os.path.exists(segmentation_path):
        raise ImageError('has no segmentation %s (run stat_fish first)' % segmentation_path)
    try:
        segmentation = np.load(segmentation_path, allow_pickle=False)
    except Exception as e:
        raise ImageError('segmentation %s cannot be read (%s)' % (segmentation_path, e))
    if not lsq_paths:
        raise ImageError('has no %s_lsq*.tif in annotated/%s (run stat_fish first)' % (img_name, img_name))
    try:
        lsq = image_io.imread(lsq_paths[0])
    except Exception as e:
        raise ImageError('lsq image %s cannot be read (%s)' % (lsq_paths[0], e))
    return lsq, segmentation


def _add(stats, key, t0):
    if stats is not None:
        stats[key] = stats.get(key, 0.0) + time.perf_counter() - t0


def get_distances_path(root_directory, handle, *presets, stats=None):
    """-> (distances of all images in sorted image order, [(path, why)] of the images that failed).  ``stats`` (tools): a dict that
    gathers the seconds spent reading (``read_s``), in the device call with what prepares it (``device_s``) and on the rows (``rows_s``)."""
    distances, failed = [], []
    for img_path in sorted(glob.glob(os.path.join(glob.escape(root_directory), '*.tif'))):
        print("Processing image: ", img_path)
        try:
            t0 = time.perf_counter()
            lsq, segmentation = load_image(root_directory, img_path)
            _add(stats, 'read_s', t0)
            t0 = time.perf_counter()
            distances += get_distances_img(lsq, segmentation, presets, handle)
            _add(stats, 'device_s', t0)
        except ImageError as e:
            print(img_path, '-', e)
            failed.append((img_path, str(e)))
    return distances, failed


def _chunk_records(handle, good, fish_probe_index, centromere_probe_index):
    """``fish_distances_many`` over the prepared images of one chunk -> per image its records or the exception it fails with alone.  A
    call that is refused as a whole (code -1) is taken apart: every image then goes alone and keeps its own verdict."""
    def call(items):
        return handle.fish_distances_many([p[0] for p in items], [p[1] for p in items], fish_probe_index, centromere_probe_index)
    try:
        return call(good)
    except Exception as e:
        if getattr(e, 'code', None) != -1:
            raise
        if len(good) == 1:
            return [e]
    out = []
    for p in good:
        try:
            out += call([p])
        except Exception as e:
            if getattr(e, 'code', None) != -1:
                raise
            out.append(e)
    return out


def get_distances_path_batched(root_directory, handle, batch, io_threads, *presets, stats=None):
    """``get_distances_path`` with the sorted images taken ``batch`` at a time: ``load_image`` and ``prepare_image`` run on
    ``io_threads`` reader threads, one chunk ahead of the device; ``handle.fish_distances_many`` measures a chunk in one call;
    ``distances_from_records`` runs per image.  Lines, values, failures and their order are ``get_distances_path``'s."""
    import concurrent.futures as cf
    centromere_probe_index, fish_probe_index, max_centromeric_spots = presets
    paths = sorted(glob.glob(os.path.join(glob.escape(root_directory), '*.tif')))
    chunks = [paths[i:i + batch] for i in range(0, len(paths), batch)]
    distances, failed = [], []

    def read(img_path):
        try:
            lsq, segmentation = load_image(root_directory, img_path)
            return prepare_image(lsq, segmentation, presets)
        except ImageError as e:
            return e

    with cf.ThreadPoolExecutor(io_threads) as readers:
        ahead = [[readers.submit(read, p) for p in c] for c in chunks[:2]]
        for k, chunk in enumerate(chunks):
            t0 = time.perf_counter()
            prepared = [f.result() for f in ahead.pop(0)]
            _add(stats, 'read_s', t0)                          # (what the device waited for: the reads run ahead of it)
            if k + 2 < len(chunks):
                ahead.append([readers.submit(read, p) for p in chunks[k + 2]])
            t0 = time.perf_counter()
            good = [p for p in prepared if isinstance(p, tuple)]
            answers = iter(_chunk_records(handle, good, fish_probe_index, centromere_probe_index) if good else [])
            _add(stats, 'device_s', t0)
            t0 = time.perf_counter()
            for img_path, p in zip(chunk, prepared):
                print("Processing image: ", img_path)
                try:
                    if isinstance(p, ImageError):
                        raise p
                    if p is None:                            # an empty map: no value
                        continue
                    rec = next(answers)
                    if isinstance(rec, Exception):
                        raise ImageError(str(rec))
                    distances += distances_from_records(rec, max_centromeric_spots)
                except ImageError as e:
                    print(img_path, '-', e)
                    failed.append((img_path, str(e)))
            _add(stats, 'rows_s', t0)
    return distances, failed


def _batch_key(var, handle):
    """The validated ``batch`` and ``io_threads`` keys; a configuration error prints its message and exits with code 2."""
    batch = var.get('batch', 1)
    if isinstance(batch, bool) or not isinstance(batch, int) or batch < 1:
        print("batch must be a positive integer (how many images share one device call; 1: one by one). Please update the config.yaml "
              "file accordingly.")
        sys.exit(2)
    if batch > 1 and handle is not None and not hasattr(handle, 'fish_distances_many'):
        print("batch: %d needs the batched distance call (fish_distances_many), which the handle in use does not have; only batch: 1 "
              "works on it." % batch)
        sys.exit(2)
    io_threads = var.get('io_threads')
    if batch > 1 and not io_threads:
        from .utils import default_io_threads
        io_threads = default_io_threads(1)
    return batch, io_threads


def main(argv=None, handle=None, stats=None):
    """``make fish_distance_calculation``.  Like the reference's ``main`` it takes everything from section
    ``fish_distance_calculation`` of ``config.yaml`` in the working directory; ``argv`` is accepted for the shim's sake and not
    read.  ``handle`` is an injection point for tests and tools (anything with ``Handle.fish_distances``, and with
    ``Handle.fish_distances_many`` for ``batch`` above 1); without it the call opens a handle on device 0 and closes it at the end.
    ``stats``: see ``get_distances_path``."""
    import yaml
    from . import csvio
    with open('config.yaml') as infile:
        var = yaml.safe_load(infile)['fish_distance_calculation']
    directory = var['inpath']
    if not os.path.isdir(str(directory)):
        print("Input folder does not exist. Exiting...")
        sys.exit(2)
    if not os.path.isdir(os.path.join(directory, 'annotated')):
        print("Input folder has no annotated/ folder: run stat_fish first. Exiting...")
        sys.exit(2)
    colors = {}
    for key in ('centromere_probe_color', 'fish_probe_color'):
        colors[key] = str(var[key]).lower()
        if colors[key] not in COLOR_TO_INDEX:
            print("%s can only be \"red\", \"green\" or \"blue\". Please update the config.yaml file accordingly." % key)
            sys.exit(2)
    max_centromeric_spots = var['max_centromeric_spots']
    if isinstance(max_centromeric_spots, bool) or not isinstance(max_centromeric_spots, int):
        print("max_centromeric_spots must be an integer. Please update the config.yaml file accordingly.")
        sys.exit(2)
    batch, io_threads = _batch_key(var, handle)
    own = handle is None
    if own:
        from ._lib import Handle
        handle = Handle(0)
    presets = (COLOR_TO_INDEX[colors['centromere_probe_color']], COLOR_TO_INDEX[colors['fish_probe_color']], max_centromeric_spots)
    try:
        if batch > 1:
            distances, failed = get_distances_path_batched(directory, handle, batch, io_threads, *presets, stats=stats)
        else:
            distances, failed = get_distances_path(directory, handle, *presets, stats=stats)
    finally:
        if own:
            handle.close()
    with open(os.path.join(directory, 'centromere_distances.csv'), 'w') as f:
        f.write(csvio.csv_text(CSV_COLUMNS, [[d] for d in distances]))
    if failed:
        print("%d image(s) were NOT processed and are missing from the CSV:" % len(failed))
        for p, why in failed:
            print("  ", p, "-", why)
        sys.exit(1)             # the reference would have crashed on the first such image


if __name__ == "__main__":
    main(sys.argv[1:])
