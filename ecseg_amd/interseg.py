"""``make interseg`` on MI355X: drop-in for the reference's ``src/interseg.py`` (config section, checks, exit codes and
``interphase_prediction_<color>.csv``).  Per image, the nuclei of ``annotated/<name>/<name>_segmentation.tif`` (what
``make stat_fish`` / NuSeT leaves, out of scope here) become region records and 256 x 256 crops on the device
(``Handle.nuclei_regions`` / ``Handle.nucleus_crops``, csrc/interseg_kernels.hip); the two Keras classifiers
``interseg_models/interseg`` (3 classes: No-amp / EC-amp / HSR-amp) and ``interseg_models/ecseg_c`` (focal amplification,
one sigmoid unit) run batched through the same plan interpreter and HIP kernels as the metaseg U-Net, and the per-nucleus
decision logic of src/interseg.py:131-190 is applied to their outputs (``classify_crops``).  One key of its own:
``classify_on_device`` (false; true: one ``Handle.classify_nucleus_crops`` call per image builds the crops, writes both classifiers'
inputs from them on the device and runs the plans - no crop crosses the bus; the same CSV).  With it, ``batch: k`` (1): the sorted
images go k at a time, their files read side by side on host threads and their nuclei through ONE ``Handle.interseg_many`` call
(``process_chunk``); the same CSV, messages and exit code.
"""
import csv
import os
import re
import sys

import numpy as np

ECSEG_I_MODEL = 'interseg'
ECSEG_C_MODEL = 'ecseg_c'

# src/interseg.py:72-90
ECSEG_I_LABEL_MAP = {0: 'No-amp', 1: 'EC-amp', 2: 'HSR-amp'}
ECSEG_C_LABEL_MAP = {0: 'No-amp', 1: 'Focal-amp'}
INTERSEG_LABEL_MAP = {
    ('No-amp', 'No-amp'): 'No-amp', ('No-amp', 'EC-amp'): 'No-amp', ('No-amp', 'HSR-amp'): 'No-amp',
    ('Focal-amp', 'No-amp'): 'No-amp', ('Focal-amp', 'EC-amp'): 'EC-amp', ('Focal-amp', 'HSR-amp'): 'HSR-amp',
}
EMPTY = 'No_Prediction (Segmentation_Empty)'
FAILED_QUALITY = 'No_Prediction (Failed Centromeric Quality Score)'
LOW_CENT = 'No_Prediction (Low_CENT_Brightness)'


def preprocess_ecseg_c(batch_x):
    """src/utils.py:166-173 for one (H, W, 3) image: per-channel max normalisation (FISH channels 0/1, DAPI channel 2),
    quantised to 1/255 steps: ``round(x / norm * 255) / 255`` (tf.math.round = half to even) in float32."""
    x = np.asarray(batch_x, np.float32)
    norm = x.reshape(-1, x.shape[-1]).max(axis=0).astype(np.float32)          # concat([fish_norm (2), dapi_norm (1)])
    with np.errstate(divide='ignore', invalid='ignore'):
        return (np.rint((x / norm) * np.float32(255)) / np.float32(255)).astype(np.float32)


def classify_crops(ecseg_i_model, crops, ecseg_c_model=None, centromeric_quality_score_pass=True, from_patches=False,
                   channel_max=None):
    """``crops``: (N, 256, 256, 3) uint8, channel 0 = target FISH, 1 = centromeric probe, 2 = DAPI (the order built at
    src/interseg.py:118).  Returns one dict per crop with the reference's columns: ecSeg-i probabilities and label, the
    ecSeg-c probabilities and label (when a centromeric-probe model is given) and the merged interSeg label
    (src/interseg.py:153-190).  ``from_patches``: crops come from the tiling of a nucleus larger than 256 px, where the
    reference skips all-zero tiles (src/interseg.py:199-210).  All crops go through the device in one batch; the
    reference calls ``model.predict`` crop by crop, which gives the same numbers (no layer depends on the batch).
    ``from_patches`` may also be a per-crop boolean array; ``channel_max`` (N, 3): the crops' per-channel maxima when the
    caller has them already (``Handle.nucleus_crops``)."""
    crops = np.ascontiguousarray(crops, np.uint8)
    if crops.ndim != 4 or crops.shape[1:] != (256, 256, 3):
        raise ValueError('crops must be (N, 256, 256, 3) uint8')
    n = len(crops)
    has_c = ecseg_c_model is not None
    from_patches = np.broadcast_to(np.asarray(from_patches, bool), (n,))
    cmax = np.asarray(channel_max).reshape(n, 3) if channel_max is not None else None
    if cmax is not None:
        empty = from_patches & (cmax.max(axis=1) == 0) if n else np.zeros(0, bool)
    else:
        empty = np.array([from_patches[k] and not crops[k].any() for k in range(n)], bool)
    live = np.flatnonzero(~empty)
    pred_i, pred_c, ran_c = np.zeros((n, 3), np.float32), np.zeros(n, np.float32), np.zeros(n, bool)
    if len(live):
        pred_i[live] = ecseg_i_model.predict(crops[live][..., 0])              # (n, 3): src/interseg.py:155
        ran_c[live] = [has_c and centromeric_quality_score_pass and
                       (cmax[k, 1] if cmax is not None else crops[k][..., 1].max()) > 10 for k in live]
        if ran_c.any():
            xc = np.stack([preprocess_ecseg_c(crops[k]) for k in np.flatnonzero(ran_c)])
            pred_c[ran_c] = ecseg_c_model.predict(xc).reshape(-1)               # (n,): src/interseg.py:168
    return rows_from_predictions(has_c, centromeric_quality_score_pass, ~empty, pred_i, ran_c, pred_c)


def rows_from_predictions(has_c, centromeric_quality_score_pass, ran_i, pred_i, ran_c, pred_c):
    """The rows of ``classify_crops`` from what the classifiers gave, wherever they ran (the host path above,
    ``Handle.classify_nucleus_crops``): ``ran_i`` (N) bool and ``pred_i`` (N, 3) float32 of ecSeg-i - a crop it did not run for is
    an empty tile of an oversized nucleus; ``ran_c`` (N) bool and ``pred_c`` (N) float32 of ecSeg-c.  ``has_c``: there is a
    centromeric-probe model, so the rows carry its columns."""
    ran_i, ran_c = np.asarray(ran_i, bool), np.asarray(ran_c, bool)
    rows = [dict() for _ in range(len(ran_i))]
    for k, r in enumerate(rows):
        if not ran_i[k]:
            r.update({'interSeg_label': EMPTY, 'ecSeg-i_label': EMPTY, 'pred_no_amp': EMPTY, 'pred_ec': EMPTY, 'pred_hsr': EMPTY})
            if has_c:
                r.update({'ecSeg-c_label': EMPTY, 'pred_no_focal_amp': EMPTY, 'pred_focal_amp': EMPTY})
            continue
        # np.float32 scalars, as the reference keeps them (src/interseg.py:156-158,169-170): a CSV written from these
        # rows prints 0.3, not float64(float32(0.3)) = 0.30000001192092896
        r['pred_no_amp'], r['pred_ec'], r['pred_hsr'] = (np.float32(v) for v in pred_i[k])
        i_label = ECSEG_I_LABEL_MAP[int(np.argmax(pred_i[k]))]
        r['ecSeg-i_label'] = i_label
        if ran_c[k]:
            v = np.float32(pred_c[k])
            r['pred_no_focal_amp'], r['pred_focal_amp'] = np.float32(1) - v, v        # float32 complement
            c_label = ECSEG_C_LABEL_MAP[int(v > 0.5)]
            r['ecSeg-c_label'] = c_label
            r['interSeg_label'] = INTERSEG_LABEL_MAP[(c_label, i_label)]
        else:
            if has_c and not centromeric_quality_score_pass:
                r['ecSeg-c_label'] = r['pred_no_focal_amp'] = r['pred_focal_amp'] = FAILED_QUALITY
            elif has_c:
                r['ecSeg-c_label'] = r['pred_no_focal_amp'] = r['pred_focal_amp'] = LOW_CENT
            r['interSeg_label'] = i_label
    return rows


# ---- the file-level driver (src/interseg.py:48-258) ----------------------------------------------------------------------
LOW_TRGT = 'No_Prediction (Low_TRGT_brightness)'
CROP_BATCH = 64                   # crops per classifier call
_NUMBER = re.compile(r'^[+-]?(\d+\.?\d*|\.\d+)([eE][+-]?\d+)?$')


def crop_windows(h, w):
    """(dy, dx, th, tw) of the crops of a nucleus whose bbox is h x w (src/interseg.py:152-154,190-194 and im2patches_overlap
    :27-46): the whole bbox when it is <= 256 in both dimensions; else 256-stride tiles, not overlapping, a partial tile
    dropped unless the whole dimension is < 256 (then the tile spans it)."""
    if h <= 256 and w <= 256:
        return [(0, 0, h, w)]
    rows = [(0, h)] if h < 256 else [(256 * i, 256) for i in range(h // 256)]
    cols = [(0, w)] if w < 256 else [(256 * j, 256) for j in range(w // 256)]
    return [(dy, dx, th, tw) for dy, th in rows for dx, tw in cols]


def region_rows(records):
    """Region records of ``Handle.nuclei_regions`` -> (nucleus_center strings, low-brightness flags, crop descriptors
    (N, 5) int32 (region, y0, x0, h, w), per-crop from_patches flags, region of every crop)."""
    rec = np.asarray(records, np.int64).reshape(-1, 8)
    area = rec[:, 0]
    centers = ['%d_%d' % (sr // a, sc // a) for a, sr, sc in zip(area.tolist(), rec[:, 5].tolist(), rec[:, 6].tolist())]
    low = 4 * rec[:, 7] < 51 * area                                   # sum / area < 12.75 (src/interseg.py:134), exactly
    desc, tiled, owner = [], [], []
    for k in np.flatnonzero(~low):
        y0, x0, y1, x1 = (int(v) for v in rec[k, 1:5])
        wins = crop_windows(y1 - y0, x1 - x0)
        for dy, dx, th, tw in wins:
            desc.append((k, y0 + dy, x0 + dx, th, tw))
            tiled.append(not (y1 - y0 <= 256 and x1 - x0 <= 256))
            owner.append(k)
    return centers, low, np.array(desc, np.int32).reshape(-1, 5), np.array(tiled, bool), np.array(owner, np.int64)


def kurtosis(x):
    """scipy.stats.kurtosis(x) (Fisher, biased, nan_policy='propagate') of the scipy the reference pins (1.7): NaN for an
    empty column or one holding NaN, -3 for a constant one."""
    a = np.asarray(x, np.float64).reshape(-1)
    if a.size == 0 or np.isnan(a).any():
        return float('nan')
    d = a - a.mean()
    s = d ** 2
    m2 = s.mean()
    m4 = (s ** 2).mean()
    if m2 <= (np.finfo(np.float64).resolution * a.mean()) ** 2:
        return -3.0
    return float(m4 / m2 ** 2.0 - 3.0)


def read_stat_fish(path):
    """annotated/stat_fish_lsq.csv as ``pd.read_csv(path, keep_default_na=False, na_values=['_'])`` reads it, reduced to what
    the quality score needs: {column: list of cells} (cells are str; '_' is pandas' NaN)."""
    with open(path, newline='') as f:
        rows = list(csv.reader(f))
    if not rows:
        raise ValueError('%s is empty' % path)
    head, body = rows[0], rows[1:]
    return {c: [r[j] if j < len(r) else '' for r in body] for j, c in enumerate(head)}


def quality_score(table, image_name, other_color):
    """Centromeric quality score of one image (src/interseg.py:108-111): the kurtosis of its ``Avg fish intensity
    (<other color>)`` cells; inf when the table has no rows.  As in pandas, an ``image_name`` column whose every cell is a
    number (or '_') is read as numbers: no image name matches it and the score is NaN (fails)."""
    names = table.get('image_name')
    col = table.get('Avg fish intensity (%s)' % other_color)
    if names is None or col is None:
        raise ValueError("stat_fish_lsq.csv has no 'image_name' / 'Avg fish intensity (%s)' column" % other_color)
    if not names:
        return float('inf')
    if all(c == '_' or _NUMBER.match(c) for c in names):
        return float('nan')

    def num(c):
        return float(c) if _NUMBER.match(c) else float('nan')       # '_' (and cells pandas would keep as text) -> NaN
    return kurtosis([num(c) for n, c in zip(names, col) if n == image_name])


class ImageError(Exception):
    pass


def _load_image(p, seg_path):
    from . import image_io
    if not os.path.exists(p):
        raise ImageError('cannot be read')
    try:
        I = image_io.imread(p)
    except Exception as e:
        raise ImageError('cannot be read (%s)' % e)
    if I.ndim < 3 or I.shape[2] < 3:
        raise ImageError("isn't an RGB image (shape %s): interSeg needs the FISH channels" % (I.shape,))
    if not os.path.exists(seg_path):
        raise ImageError('has no segmentation %s (run stat_fish first)' % seg_path)
    try:
        seg = image_io.imread(seg_path)
    except Exception as e:
        raise ImageError('segmentation %s cannot be read (%s)' % (seg_path, e))
    if seg.ndim == 3 and seg.shape[2] == 1:
        seg = seg[..., 0]
    if seg.ndim != 2:
        raise ImageError('segmentation %s is not a single-channel image (shape %s)' % (seg_path, seg.shape))
    if seg.shape[0] > I.shape[0] or seg.shape[1] > I.shape[1]:
        raise ImageError('segmentation %s (%d x %d) is larger than the image (%d x %d)' % ((seg_path,) + seg.shape[:2] + I.shape[:2]))
    return I, seg


def _stem_and_segmentation(p):
    path_split = os.path.split(p)
    stem = path_split[1][:-4]
    return stem, os.path.join(path_split[0], 'annotated', stem, stem + '_segmentation.tif')


def _device_inputs(I, seg, seg_path, handle):
    """What ``_load_image`` read, as the device calls take it: both uint8, C-contiguous."""
    from . import image_tools
    I = np.ascontiguousarray(image_tools.u16_to_u8(I, handle=handle))
    seg = np.ascontiguousarray(seg)
    if seg.dtype != np.uint8:                                       # a 16-bit / bool mask: the device call takes uint8
        if len(np.unique(seg[seg != 0])) > 1:
            raise ImageError('segmentation %s holds several non-zero values: only 0 / non-zero nucleus masks are supported' % seg_path)
        seg = (seg != 0).astype(np.uint8) * np.uint8(255)
    return I, seg


def _csv_rows(stem, centers, low, owner, crop_rows, has_c):
    """The CSV rows of one image from its regions' centres and gate flags and its crops' rows (``owner``: the region of every crop)."""
    by_region = {}
    for k, r in zip(owner.tolist(), crop_rows):
        by_region.setdefault(k, []).append(r)
    rows = []
    for k in range(len(centers)):
        if low[k]:
            rows.append([stem, centers[k], LOW_TRGT] + ([LOW_TRGT] if has_c else []) + [LOW_TRGT])
            continue
        for r in by_region.get(k, []):
            rows.append([stem, centers[k], r['interSeg_label']] + ([r['ecSeg-c_label']] if has_c else []) + [r['ecSeg-i_label']])
    return rows


def process_image(p, handle, ecseg_i_model, ecseg_c_model, fish_index, quality_pass, stats=None, classify_on_device=False):
    """CSV rows of one image (src/interseg.py:105-235): [name, nucleus_center, interSeg_label, (ecSeg-c_label,) ecSeg-i_label].
    ``classify_on_device`` (the config key): one ``handle.classify_nucleus_crops`` call takes the crop descriptors and returns the
    classifiers' outputs - the crops never reach the host; the same rows."""
    import time
    stem, seg_path = _stem_and_segmentation(p)
    t0 = time.perf_counter()
    I, seg = _device_inputs(*_load_image(p, seg_path), seg_path, handle)
    t1 = time.perf_counter()
    has_c = ecseg_c_model is not None
    crop_rows = []
    try:
        rec = handle.nuclei_regions(seg, I, fish_index)
        centers, low, desc, tiled, owner = region_rows(rec)
        order = (fish_index, 1 - fish_index, 2)
        if classify_on_device:
            t2 = time.perf_counter()
            if len(desc):
                _, pred_i, ran_i, pred_c, ran_c = handle.classify_nucleus_crops(desc, order, tiled, has_c and quality_pass, ecseg_i_model,
                                                                               ecseg_c_model)
                crop_rows = rows_from_predictions(has_c, quality_pass, ran_i, pred_i, ran_c, pred_c)
        else:
            crops, cmax = handle.nucleus_crops(desc, order) if len(desc) else (np.zeros((0, 256, 256, 3), np.uint8), np.zeros((0, 3), np.int32))
            t2 = time.perf_counter()
    except Exception as e:
        if getattr(e, 'code', None) == -1:
            raise ImageError(str(e))
        raise
    if not classify_on_device:
        for b0 in range(0, len(desc), CROP_BATCH):
            sl = slice(b0, b0 + CROP_BATCH)
            crop_rows += classify_crops(ecseg_i_model, crops[sl], ecseg_c_model, quality_pass, from_patches=tiled[sl], channel_max=cmax[sl])
    t3 = time.perf_counter()
    rows = _csv_rows(stem, centers, low, owner, crop_rows, has_c)
    if stats is not None:
        for key, v in (('read', t1 - t0), ('device_crops', t2 - t1), ('classifiers', t3 - t2), ('rows', time.perf_counter() - t3)):
            stats[key] = stats.get(key, 0.0) + v
        stats['crops'] = stats.get('crops', 0) + len(desc)
        stats['nuclei'] = stats.get('nuclei', 0) + len(centers)
    return rows


def process_chunk(paths, quality, handle, ecseg_i_model, ecseg_c_model, fish_index, pool, stats=None):
    """``process_image`` for the images of one chunk (config key ``batch``, with ``classify_on_device``): the files are read side by
    side on ``pool``, then ONE ``handle.interseg_many`` call takes every image that could be read.  ``quality``: per image its
    ``quality_pass`` flag, or the ``ImageError`` the quality score raised.  Returns per image its CSV rows or its ``ImageError``: what
    fails one image leaves the others alone."""
    import time
    has_c = ecseg_c_model is not None
    names = [_stem_and_segmentation(p) for p in paths]
    t0 = time.perf_counter()

    def load(k):
        if isinstance(quality[k], ImageError):
            return quality[k]
        try:
            return _load_image(paths[k], names[k][1])
        except ImageError as e:
            return e
    out = list(pool.map(load, range(len(paths))))
    live = []
    for k, item in enumerate(out):
        if not isinstance(item, ImageError):
            try:
                live.append((k,) + _device_inputs(item[0], item[1], names[k][1], handle))
            except ImageError as e:
                out[k] = e
    t1 = time.perf_counter()
    results = handle.interseg_many([I for _, I, _ in live], [seg for _, _, seg in live], fish_index, [bool(quality[k]) for k, _, _ in live],
                                   ecseg_i_model, ecseg_c_model) if live else []
    t2 = time.perf_counter()
    for (k, _, _), res in zip(live, results):
        if isinstance(res, Exception):
            if getattr(res, 'code', None) != -1:
                raise res
            out[k] = ImageError(str(res))
            continue
        rec, (owner, pred_i, ran_i, pred_c, ran_c) = res
        centers, low = region_rows(rec)[:2]
        crop_rows = rows_from_predictions(has_c, bool(quality[k]), ran_i, pred_i, ran_c, pred_c)
        out[k] = _csv_rows(names[k][0], centers, low, np.asarray(owner, np.int64), crop_rows, has_c)
        if stats is not None:
            stats['crops'] = stats.get('crops', 0) + len(owner)
            stats['nuclei'] = stats.get('nuclei', 0) + len(centers)
    if stats is not None:
        for key, v in (('read', t1 - t0), ('device', t2 - t1), ('rows', time.perf_counter() - t2)):
            stats[key] = stats.get(key, 0.0) + v
    return out


def csv_columns(has_centromeric_probe):
    return ['image_name', 'nucleus_center', 'interSeg_label'] + (['ecSeg-c_label'] if has_centromeric_probe else []) + ['ecSeg-i_label']


def main(argv=None):
    import yaml
    from . import csvio
    from .utils import get_imgs, load_model
    config = open("config.yaml")
    var = yaml.load(config, Loader=yaml.FullLoader)['interseg']
    inpath = var['inpath']
    fish_color = str(var['FISH_color']).lower()
    has_centromeric_probe = bool(var['has_centromeric_probe'])

    if not os.path.isdir(os.path.join(inpath)):
        print("Input folder does not exist. Exiting...")
        sys.exit(2)
    else:
        if (fish_color != 'green') & (fish_color != 'red'):
            print("FISH_color can only be \"green\" or \"red\". Please update the config.yaml file accordingly.")
            sys.exit(2)
    classify_on_device = var.get('classify_on_device', False)
    if not isinstance(classify_on_device, bool):
        print("interseg.classify_on_device must be true or false (true: the nucleus crops go through the classifiers without leaving the device). Exiting...")
        sys.exit(2)
    batch = var.get('batch', 1)
    if isinstance(batch, bool) or not isinstance(batch, int) or batch < 1:
        print("interseg.batch must be a positive integer (how many images share one device call, with classify_on_device: true; 1: one by one). Exiting...")
        sys.exit(2)
    if not classify_on_device:
        batch = 1                                            # (as tiff_read_batch without its parent key)
    fish_index = 1 if fish_color == 'green' else 0
    os.makedirs(os.path.join(inpath, 'annotated'), exist_ok=True)

    image_paths = get_imgs(inpath)
    if not image_paths:
        # the reference crashes here (pd.concat of nothing, src/interseg.py:256)
        print("No .tif / .npy images in the input folder. Exiting...")
        sys.exit(2)

    ecseg_i_model = load_model(ECSEG_I_MODEL)
    ecseg_c_model = load_model(ECSEG_C_MODEL) if has_centromeric_probe else None
    handle = ecseg_i_model.handle
    if classify_on_device and not hasattr(handle, 'classify_nucleus_crops'):
        print("interseg.classify_on_device: true needs the device classifier path (classify_nucleus_crops), which the handle in use does not have. Exiting...")
        sys.exit(2)
    if batch > 1 and not hasattr(handle, 'interseg_many'):
        print("interseg.batch: %d needs the batched device path (interseg_many), which the handle in use does not have; only batch: 1 works on it. Exiting..." % batch)
        sys.exit(2)
    table, table_error = None, None
    if has_centromeric_probe:
        # the reference reads the table even without a centromeric probe, where it is never used (src/interseg.py:101)
        try:
            table = read_stat_fish(os.path.join(inpath, 'annotated', 'stat_fish_lsq.csv'))
        except (OSError, ValueError) as e:
            table_error = 'annotated/stat_fish_lsq.csv cannot be read (%s): run stat_fish first' % e

    def quality_of(p):
        if not has_centromeric_probe:
            return True
        if table_error:
            raise ImageError(table_error)
        try:
            return bool(quality_score(table, os.path.split(p)[1][:-4], ['red', 'green'][1 - fish_index]) <= 3)
        except ValueError as e:
            raise ImageError(str(e))

    rows, failed = [], []
    if batch == 1:
        for p in image_paths:
            print("Processing image: ", p)
            try:
                rows += process_image(p, handle, ecseg_i_model, ecseg_c_model, fish_index, quality_of(p), classify_on_device=classify_on_device)
            except ImageError as e:
                print(p, '-', e)
                failed.append((p, str(e)))
    else:
        from concurrent.futures import ThreadPoolExecutor
        from .utils import default_io_threads
        with ThreadPoolExecutor(default_io_threads()) as pool:
            for c0 in range(0, len(image_paths), batch):
                chunk = image_paths[c0:c0 + batch]
                quality = []
                for p in chunk:
                    try:
                        quality.append(quality_of(p))
                    except ImageError as e:
                        quality.append(e)
                results = process_chunk(chunk, quality, handle, ecseg_i_model, ecseg_c_model, fish_index, pool)
                for p, res in zip(chunk, results):               # the lines of batch: 1, in its order
                    print("Processing image: ", p)
                    if isinstance(res, ImageError):
                        print(p, '-', res)
                        failed.append((p, str(res)))
                    else:
                        rows += res
    with open(os.path.join(inpath, 'interphase_prediction_%s.csv' % fish_color), 'w') as f:
        f.write(csvio.csv_text(csv_columns(has_centromeric_probe), rows))
    if failed:
        print("%d image(s) were NOT processed and are missing from the CSV:" % len(failed))
        for p, why in failed:
            print("  ", p, "-", why)
        sys.exit(1)             # the reference would have crashed on the first such image


if __name__ == "__main__":
    main(sys.argv[1:])
