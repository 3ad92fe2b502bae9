"""Cases of NuSeT's two ``rescale`` calls (reference src/utils.py:136,157-162), shared by tools/make_golden_rescale.py (which runs
scikit-image / scipy on them), tests/test_rescale.py (restatement == golden) and tests/test_gpu_rescale.py (device == restatement ==
golden).  Plain numpy only: the golden tool imports this file under an old interpreter.

A down case is a dict: name, image (uint8 H x W), scale (the ``scale_ratio`` s).  An up case: name, mask (``clean_image``'s uint8
0 / 1), scale (1 / s, computed as the reference writes it) and sizes (the NUCLEI_SIZE_T values)."""
import numpy as np


def scene(h, w, seed):
    """A seeded DAPI-like image: noise floor plus Gaussian blobs, scaled to stay below 250.  It is noisy everywhere and never
    saturates: on a flat (or exactly linear) stretch a Gaussian pass lands on an integer give or take the last bit of a weight, and
    that bit of ``exp`` differs between numpy releases (tools/make_golden_rescale.py refuses such a case)."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[:h, :w]
    img = np.zeros((h, w))
    for _ in range(max(3, h * w // 700)):
        cy, cx, r = rng.uniform(0, h), rng.uniform(0, w), rng.uniform(2, 9)
        img += rng.uniform(60, 260) * np.exp(-((yy - cy) ** 2 + (xx - cx) ** 2) / (2 * r * r))
    img *= min(1.0, 180.0 / img.max())
    return np.clip(img + rng.normal(30.0, 8.0, (h, w)), 1, 255).astype(np.uint8)


def blobs(h, w, seed, n=None):
    """A seeded 0 / 1 mask of discs and a few single pixels."""
    rng = np.random.default_rng(seed)
    yy, xx = np.ogrid[:h, :w]
    m = np.zeros((h, w), np.uint8)
    for _ in range(n if n is not None else max(2, h * w // 900)):
        cy, cx, r = int(rng.integers(0, h)), int(rng.integers(0, w)), int(rng.integers(1, 9))
        m[(yy - cy) ** 2 + (xx - cx) ** 2 <= r * r] = 1
    for _ in range(3):
        m[int(rng.integers(0, h)), int(rng.integers(0, w))] = 1
    return m


def _down(name, image, scale):
    return dict(name=name, image=np.ascontiguousarray(image, np.uint8), scale=float(scale))


def _up(name, mask, scale, sizes=(0,)):
    return dict(name=name, mask=np.ascontiguousarray(mask, np.uint8), scale=float(scale), sizes=tuple(int(s) for s in sizes))


def down_cases():
    out = [_down('scene_64x80_s0.3', scene(64, 80, 1), 0.3),            # radius 5, the mirror at all four borders
           _down('scene_53x47_s0.3', scene(53, 47, 2), 0.3),            # odd extents, f_y != f_x
           _down('scene_40x40_s0.5', scene(40, 40, 3), 0.5),
           _down('scene_30x30_s0.7', scene(30, 30, 4), 0.7),            # radius 1
           _down('scene_37x61_s0.25', scene(37, 61, 5), 0.25)]
    for v in (0, 200, 255):
        out.append(_down('constant_%d_s0.7' % v, np.full((30, 30), v, np.uint8), 0.7))     # truncation: 200 comes out as 198
        out.append(_down('constant_%d_s0.25' % v, np.full((40, 36), v, np.uint8), 0.25))   # radius 6
    yy, xx = np.mgrid[:40, :44]
    out.append(_down('checkerboard_s0.25', ((yy + xx) % 2) * 255, 0.25))
    out.append(_down('checkerboard_s0.5', ((yy + xx) % 2) * 255, 0.5))
    out.append(_down('ramp_s0.25', (yy * 3 + xx * 2) % 256, 0.25))
    out.append(_down('ramp_s0.7', (yy * 3 + xx * 2) % 256, 0.7))
    out.append(_down('scene_203x331_s0.3', scene(203, 331, 6), 0.3))    # several workgroup tiles, ragged edges
    return out


def up_cases():
    up3, up2 = 1 / 0.3, 1 / 0.5
    out = [_up('blobs_16x32', blobs(16, 32, 11), up3, (0, 30)),
           _up('blobs_32x48', blobs(32, 48, 12), up3, (0, 30, 200)),
           _up('blobs_48x32_half', blobs(48, 32, 13), up2, (0, 10, 100)),
           _up('blobs_304x416', blobs(304, 416, 14, 90), up3, (0, 400))]
    m = np.zeros((16, 32), np.uint8); m[1, 3:20] = 1; m[2:12, 1] = 1     # row 1 / column 1 but not row 0 / column 0: the mirrored -1 shows
    out.append(_up('row1_col1', m, up3, (0, 5)))
    m = np.zeros((16, 32), np.uint8); m[7, 13] = 1                       # vmax < 1 / 255
    out.append(_up('lone_pixel', m, up3, (0, 3)))
    out.append(_up('all_zero', np.zeros((16, 32), np.uint8), up3, (0, 5)))
    out.append(_up('all_one', np.ones((16, 32), np.uint8), up3, (0, 5)))
    m = np.zeros((32, 48), np.uint8); m[6:12, 8:14] = 1; m[12:18, 14:20] = 1
    out.append(_up('diagonal_blobs', m, up3, (0, 700, 1500)))
    out.append(_up('diagonal_blobs_half', m, up2, (0, 200, 500)))
    m = np.zeros((32, 48), np.uint8); m[10:14, 20:26] = 1; m[24:26, 5:8] = 1
    import rescale_ref                                                   # plain numpy too; the golden tool checks it on this very case
    area = int((rescale_ref.rescale_mask_up(m, up3, 0)[70:, :35] != 0).sum())         # the smaller component, up-scaled
    out.append(_up('size_at_area', m, up3, (0, area, area + 1)))         # equal to its area: kept; one above: removed
    return out


def random_down(seed, max_extent=160):
    rng = np.random.default_rng(5000 + seed)
    s = float(rng.choice([0.2, 0.25, 0.3, 0.4, 0.5, 0.6, 0.7, 0.8, 0.9]))
    lo = int(np.ceil(4 / s)) + 4
    h, w = (int(v) for v in rng.integers(lo, max(lo + 1, max_extent + 1), 2))
    kind = int(rng.integers(0, 4))
    img = scene(h, w, 7000 + seed) if kind else rng.integers(0, 256, (h, w)).astype(np.uint8)
    return _down('random_down_%d' % seed, img, s)


def random_up(seed, max_extent=96):
    rng = np.random.default_rng(6000 + seed)
    s = float(rng.choice([0.2, 0.25, 0.3, 0.4, 0.5, 0.6, 0.7, 0.8, 0.9]))
    h, w = (int(v) for v in rng.integers(2, max_extent + 1, 2))
    m = blobs(h, w, 8000 + seed)
    if rng.random() < 0.15:
        m = 1 - m
    return _up('random_up_%d' % seed, m, 1 / s, (0, int(rng.integers(1, 80)), int(rng.integers(80, 900))))


SEEDS = range(12)
