#!/opt/conda/bin/python3.9
"""Golden vectors of the interSeg file-level driver (``make interseg``), taken from the libraries the reference runs on.

Run (build container only, never on the GPU box):

    /opt/conda/bin/python3.9 tools/make_golden_interseg.py

Scenes are synthetic 0 / 255 nucleus masks with RGB images.  For every scene the tool records what
``skimage.measure.label(seg, connectivity=None)`` + ``regionprops`` give (region order, area, bbox, centroid strings, the
channel sums of the brightness gate), the crop windows of each region (whole bbox when it is <= 256 in both dimensions,
else the 256-stride tiles with partial tiles dropped unless the whole dimension is < 256), and the crops themselves as
``skimage.transform.resize(I * mask, (256, 256), preserve_range=True).astype('uint8')`` computes them (scikit-image 0.18.3).
It also records ``scipy.stats.kurtosis`` of columns read by ``pandas.read_csv(keep_default_na=False, na_values=['_'])``
(the centromeric quality score).  Only data is stored.

  interseg_scene_small.npz   seg / image / region records / windows / crops of the small-nucleus corner cases
  interseg_scene_large.npz   the same for bboxes of 256 and larger (tiles, dropped remainders, an all-zero tile)
  interseg_kurtosis.json     stat_fish_lsq.csv texts, image names, kurtosis values and pass / fail
"""
import io
import json
import os
import warnings

import numpy as np
import pandas as pd
from scipy.stats import kurtosis
from skimage import measure
from skimage.transform import resize

warnings.filterwarnings('ignore')
OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', 'tests', 'golden')


def windows(h, w):
    """(dy, dx, th, tw, tiled) of the crops of a bbox h x w."""
    if h <= 256 and w <= 256:
        return [(0, 0, h, w, 0)]
    rows = [(0, h)] if h < 256 else [(256 * i, 256) for i in range(h // 256)]
    cols = [(0, w)] if w < 256 else [(256 * j, 256) for j in range(w // 256)]
    return [(dy, dx, th, tw, 1) for dy, th in rows for dx, tw in cols]


def record(seg, img):
    H, W = seg.shape
    I = img[:H, :W]
    lab = measure.label(seg, connectivity=None)
    regs, wins, crops = [], [], []
    for k, r in enumerate(measure.regionprops(lab)):
        mask = lab == r.label
        cy, cx = r.centroid
        y0, x0, y1, x1 = r.bbox
        regs.append([r.area, y0, x0, y1, x1, int(I[..., 0][mask].sum()), int(I[..., 1][mask].sum()),
                     int(float(np.sum((I * mask[..., None])[..., 0])) / np.sum(mask) < 12.75)])
        centers = str(int(cy)) + '_' + str(int(cx))
        regs[-1].append(centers)
        temp = (I * mask[..., None])[y0:y1, x0:x1]
        for dy, dx, th, tw, tiled in windows(y1 - y0, x1 - x0):
            wins.append([k, y0 + dy, x0 + dx, th, tw, tiled])
            crops.append(resize(temp[dy:dy + th, dx:dx + tw], (256, 256), preserve_range=True).astype('uint8'))
    return lab, regs, wins, crops


def save(name, seg, img):
    lab, regs, wins, crops = record(seg, img)
    np.savez_compressed(os.path.join(OUT, name), seg=seg, image=img,
                        records=np.array([r[:8] for r in regs], np.int64).reshape(-1, 8),
                        centers=np.array([r[8] for r in regs]), windows=np.array(wins, np.int32).reshape(-1, 6),
                        crops=np.array(crops, np.uint8).reshape(-1, 256, 256, 3))
    print(name, 'regions', len(regs), 'crops', len(crops), os.path.getsize(os.path.join(OUT, name)), 'bytes')


def scene_small():
    rng = np.random.default_rng(7)
    H, W = 150, 200                                  # the image is larger than the mask (src/interseg.py:116-117)
    seg = np.zeros((H, W), np.uint8)
    img = pattern(H + 6, W + 9)
    img[15:40, 25:35] = rng.integers(0, 256, (25, 10, 3))          # noise under the 1-pixel-wide nucleus
    img[85:115, 105:135] = rng.integers(0, 256, (30, 30, 3))       # and under the inner nucleus of the ring
    img[100:140, 150:195] = 255                      # saturated block
    seg[0:3, 0:4] = 255                              # top-left border
    seg[10, 20] = 255                                # 1 pixel
    seg[15:40, 30] = 255                             # 1 pixel wide (w = 1)
    seg[50, 10:40] = 255                             # h = 1
    seg[60:62, 10:50] = 255                          # h = 2
    seg[70:100, 60:62] = 255                         # w = 2
    seg[20:26, 50:56] = 255; seg[26:30, 56:62] = 255  # joined only diagonally: one region
    seg[40:46, 80:86] = 255; seg[47:50, 87:90] = 255  # 1 px gap on the diagonal: two regions
    yy, xx = np.ogrid[:H, :W]
    ring = ((yy - 100) ** 2 + (xx - 120) ** 2 <= 25 ** 2) & ((yy - 100) ** 2 + (xx - 120) ** 2 >= 15 ** 2)
    seg[ring] = 255
    seg[96:104, 116:124] = 255                       # a second nucleus inside the ring's bbox
    seg[110:135, 160:190] = 255                      # inside the saturated block
    seg[H - 5:H, W - 7:W] = 255                      # bottom-right border
    seg[0:4, W - 3:W] = 255                          # top-right border
    # exact brightness gate: mean channel 0 == 12.75 (passes) and just below (fails)
    seg[130:132, 20:22] = 255; img[130:132, 20:22, 0] = [[12, 13], [13, 13]]
    seg[136:138, 20:22] = 255; img[136:138, 20:22, 0] = [[12, 13], [13, 12]]
    return seg, img


def pattern(H, W):
    yy, xx = np.mgrid[:H, :W]
    img = np.stack([((yy // 7) * 29 + (xx // 11) * 13) % 256, ((yy // 5) * 7 + (xx // 6) * 41) % 256,
                    ((yy // 9 + xx // 13) * 37) % 256], -1).astype(np.uint8)
    return img


def scene_large():
    H, W = 560, 1180
    seg = np.zeros((H, W), np.uint8)
    img = pattern(H, W)
    img[300:420, 600:900] = 255                      # saturated block under the cols-only nucleus
    img[40:60, 40:300, 0] = 0                        # dark band
    seg[0:256, 0:540] = 255                          # L-shape: bbox 530 x 540 -> 2 x 2 tiles, the last one all zero,
    seg[0:530, 0:256] = 255                          #   remainders 18 rows / 28 columns dropped
    seg[300:500, 300:500] = 255                      # another nucleus in the empty quadrant of the L's bbox
    seg[10:310, 580:700] = 255                       # rows only: 300 x 120 -> one 256 x 120 tile
    yy, xx = np.ogrid[:H, :W]
    seg[((yy - 380) / 50.0) ** 2 + ((xx - 750) / 150.0) ** 2 <= 1.0] = 255      # cols only: ~101 x 301
    seg[10:266, 900:1156] = 255                      # bbox exactly 256 x 256
    seg[10:20, 900:910] = 0
    seg[300:556, 1100:1180] = 255                    # 256 x 80 on the right border
    return seg, img


def kurtosis_cases():
    rng = np.random.default_rng(3)
    cases = []

    def table(names, green, red=None):
        df = pd.DataFrame({'image_name': names, 'Avg fish intensity (red)': red if red is not None else ['1.5'] * len(names),
                           'Avg fish intensity (green)': green})
        return df.to_csv(index=False)

    vals = [('%.3f' % v) for v in rng.gamma(2.0, 10.0, 12)]
    cases.append((table(['img_a'] * 6 + ['img_b'] * 6, vals), ['img_a', 'img_b', 'img_c']))
    heavy = ['1'] * 9 + ['200']                                    # kurtosis > 3: fails
    cases.append((table(['s1'] * 10 + ['s2'] * 3, heavy + ['4', '5', '6']), ['s1', 's2']))
    cases.append((table(['c'] * 4, ['7'] * 4), ['c']))             # constant column
    cases.append((table(['n'] * 3, ['1', '_', '3']), ['n']))        # '_' -> NaN
    cases.append((table(['001', '002', '002'], ['1', '2', '3']), ['001', '002']))   # numeric names: read as int, nothing matches
    cases.append(('image_name,Avg fish intensity (red),Avg fish intensity (green)\n', ['x']))   # empty table
    out = []
    for text, names in cases:
        df = pd.read_csv(io.StringIO(text), keep_default_na=False, na_values=['_'])
        for color in ('red', 'green'):
            for name in names:
                sel = df[df['image_name'] == name]
                score = kurtosis(sel['Avg fish intensity (%s)' % color]) if len(df) else float('inf')
                out.append({'csv': text, 'image': name, 'column': color, 'score': None if np.isnan(score) else float(score),
                            'pass': bool(score <= 3)})
    with open(os.path.join(OUT, 'interseg_kurtosis.json'), 'w') as f:
        json.dump(out, f, indent=0)
    print('interseg_kurtosis.json', len(out), 'cases')


if __name__ == '__main__':
    os.makedirs(OUT, exist_ok=True)
    save('interseg_scene_small.npz', *scene_small())
    save('interseg_scene_large.npz', *scene_large())
    kurtosis_cases()
