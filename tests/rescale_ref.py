"""numpy restatement of the two ``rescale`` calls of NuSeT's ``nuclei_segment`` (reference src/utils.py:136 and :157-162) as
scikit-image 0.18.3 / scipy 1.7.1 compute them, without either library: tools/make_golden_rescale.py ties it to their own outputs
(tests/golden/nuset_rescale.npz), tests/test_gpu_rescale.py ties the device to it bit for bit.  Plain numpy only: the golden tool
imports this file under an old interpreter.

Down, ``rescale(image_u8, s, anti_aliasing=True)``: ``scipy.ndimage.gaussian_filter`` on the uint8 array (axis 0, then axis 1, each
writing uint8 by truncation, mode 'mirror', scipy's symmetric-kernel order of additions), / 255, then the bilinear ``warp`` on the
exact map ``y = f * (r + 0.5) - 0.5``.  Up, ``rescale(cleaned_u8, 1 / s)``: the same bilinear without a filter, the min-max scaling
with its truncation, ``> 0 -> 255`` and ``remove_small_objects`` (4-connected)."""
import numpy as np


def out_extent(shape, scale):
    """``np.round(scale * shape)`` (half to even) -> (out_h, out_w) as ints."""
    out = np.round(scale * np.asarray(shape))
    return int(out[0]), int(out[1])


def gaussian_weights(f):
    """The 2 r + 1 float64 weights of ``gaussian_filter1d`` at ``sigma = max(0, (f - 1) / 2)``; [1.0] (r = 0) where scipy copies."""
    sigma = max(0.0, (float(f) - 1) / 2)
    if not sigma > 1e-15:
        return np.ones(1, np.float64)
    radius = int(4.0 * sigma + 0.5)
    sigma2 = sigma * sigma
    x = np.arange(-radius, radius + 1)
    phi = np.exp(-0.5 / sigma2 * x ** 2)
    return phi / phi.sum()


def mirror(i, n):
    """Indices mirrored without repeating the edge sample (-1 -> 1, n -> n - 2); one reflection, then clamped."""
    i = np.where(i < 0, -i, i)
    i = np.where(i >= n, 2 * (n - 1) - i, i)
    return np.clip(i, 0, n - 1)


def filter_axis(a, w, axis):
    """One truncating uint8 pass of scipy's symmetric correlate1d along ``axis``."""
    r = len(w) // 2
    if r == 0:
        return a.copy()
    a = np.moveaxis(a, axis, 0)
    n = a.shape[0]
    if r >= n:
        raise ValueError('the radius %d needs more than one reflection of %d samples' % (r, n))
    line = a.astype(np.float64)
    i = np.arange(n)
    tmp = line * w[r]
    for j in range(-r, 0):
        tmp = tmp + (line[mirror(i + j, n)] + line[mirror(i - j, n)]) * w[r + j]
    return np.moveaxis(tmp.astype(np.uint8), 0, axis)         # values in [0, 255]: the cast truncates


def bilinear(p, out_h, out_w):
    """Order-1 ``warp`` of the float64 image ``p`` to (out_h, out_w), mode 'reflect', on the exact coordinate map."""
    H, W = p.shape
    fy, fx = np.float64(H) / np.float64(out_h), np.float64(W) / np.float64(out_w)
    y = fy * (np.arange(out_h) + 0.5) - 0.5
    x = fx * (np.arange(out_w) + 0.5) - 0.5
    y0f, x0f = np.floor(y), np.floor(x)
    dy, dx = (y - y0f)[:, None], (x - x0f)[None, :]
    y0, y1 = mirror(y0f.astype(np.int64), H), mirror(np.ceil(y).astype(np.int64), H)
    x0, x1 = mirror(x0f.astype(np.int64), W), mirror(np.ceil(x).astype(np.int64), W)
    top = (1 - dx) * p[y0][:, x0] + dx * p[y0][:, x1]
    bottom = (1 - dx) * p[y1][:, x0] + dx * p[y1][:, x1]
    return (1 - dy) * top + dy * bottom


def rescale_down(image, scale):
    """uint8 (H, W) -> (float64 (out_h, out_w), the filtered uint8 (H, W))."""
    a = np.asarray(image)
    if a.dtype != np.uint8 or a.ndim != 2:
        raise ValueError('rescale_down takes one (H, W) uint8 image')
    out_h, out_w = out_extent(a.shape, scale)
    filtered = filter_axis(a, gaussian_weights(a.shape[0] / out_h), 0)
    filtered = filter_axis(filtered, gaussian_weights(a.shape[1] / out_w), 1)
    return bilinear(filtered.astype(np.float64) / 255, out_h, out_w), filtered


def label4(b):
    """4-connected components of a bool image in raster order of their first pixel -> (int32 labels, count): run-based union-find."""
    H, W = b.shape
    lab = np.zeros((H, W), np.int32)
    parent = [0]

    def find(i):
        while parent[i] != i:
            parent[i] = parent[parent[i]]
            i = parent[i]
        return i
    prev = []
    for y in range(H):
        row = np.concatenate(([0], b[y].astype(np.int8), [0]))
        d = np.diff(row)
        runs = []
        for s, e in zip(np.nonzero(d == 1)[0], np.nonzero(d == -1)[0]):
            k = len(parent)
            parent.append(k)
            for ps, pe, pk in prev:
                if ps < e and s < pe:
                    a, c = find(pk), find(k)
                    if a != c:
                        parent[max(a, c)] = min(a, c)
            runs.append((s, e, k))
            lab[y, s:e] = k
        prev = runs
    root = np.array([find(i) for i in range(len(parent))], np.int32)
    _, dense = np.unique(root, return_inverse=True)
    return dense.astype(np.int32)[lab], int(dense.max())


def mask_up_values(cleaned, scale):
    """The float64 image the reference thresholds: ``rescale(cleaned_u8, scale)`` -> (v, ((v - vmin) / (vmax - vmin)) * 255)."""
    c = np.asarray(cleaned)
    if c.dtype != np.uint8 or c.ndim != 2:
        raise ValueError('rescale_mask_up takes one (H, W) uint8 image')
    v = bilinear(c.astype(np.float64) / 255, *out_extent(c.shape, scale))
    with np.errstate(all='ignore'):
        return v, ((v - v.min()) / (v.max() - v.min())) * 255


def rescale_mask_up(cleaned, scale, nuclei_size_T):
    """uint8 (H, W) -> the final uint8 0 / 255 mask of src/utils.py:157-162."""
    _, t = mask_up_values(cleaned, scale)
    on = t >= 1                                               # uint8(t) > 0; NaN (an image of one value): False
    if nuclei_size_T > 0:
        lab, _ = label4(on)
        sizes = np.bincount(lab.ravel())
        small = sizes < nuclei_size_T
        small[0] = False
        on = on & ~small[lab]
    return on.astype(np.uint8) * np.uint8(255)
