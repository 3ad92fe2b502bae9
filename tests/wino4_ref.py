"""Float64 truth, per-output error scale and float32 replay of the F(4x4, 3x3) Winograd kernels (ecseg_amd/csrc/wino4r_kernel.hip,
wino4_kernel.hip, wino4s_kernel.hip) for tests/test_wino4_ref.py (CPU) and tests/test_gpu_wino4_accuracy.py (device).  numpy only.
TEST INFRASTRUCTURE ONLY.

The kernels compute, per 4 x 4 output tile and output channel o,

    Y = A^T [ sum_c U[c, o] . V[c] ] A + bias,       U = G g G^T (float64 on the host, rounded ONCE to float32),  V = B^T d B,

with the interpolation points {0, +-a, +-b, inf} of ecseg_amd/csrc/common.h (``points()`` reads them from the header).

* ``truth``   a float64 direct 3 x 3 'same' correlation + bias, then the tail (linear / relu, 2 x 2 max-pool, 1 x 1 softmax head).
* ``scale``   Q = |A^T| ( sum_c (|G| |g| |G^T|) . (|B^T| |d| |B|) ) |A|, the magnitude every rounding on the kernels' path is relative to:
              an operation that rounds a partial result r commits at most u |r|, u = 2^-24, and every partial result of the transforms
              and of the channel sum is bounded by the same expression with absolute values, so each rounding costs an output at most
              u Q (first order) - however disparate the channels are, where a per-layer max norm says nothing.
* ``replay``  the kernels' float32 arithmetic in their own operation order (moved here from tools/wino_points.py, which imports it).
* ``hard_count``  how many roundings lie on the path of one output.

Everything works on the tiles that can be non-zero (``Tiles``): a tile whose 6 x 6 x Cin inputs are all zero has V = 0, an output channel
whose filter slice is all zero has U = 0, and then every step of the kernel adds exact zeros: the output is act(bias) bit for bit.
"""
import os
import re

import numpy as np
from numpy.lib.stride_tricks import as_strided

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U32 = 2.0 ** -24


def points():
    """(a, b) of ecseg_amd/csrc/common.h (ECSEG_W4_PA, ECSEG_W4_PB)."""
    with open(os.path.join(ROOT, 'ecseg_amd', 'csrc', 'common.h')) as f:
        src = f.read()
    a = re.search(r'#define\s+ECSEG_W4_PA\s+([0-9.eE+-]+)', src)
    b = re.search(r'#define\s+ECSEG_W4_PB\s+([0-9.eE+-]+)', src)
    assert a and b, 'common.h no longer defines the F(4x4) points'
    return float(a.group(1)), float(b.group(1))


def matrices(a=None, b=None):
    """-> (BT 6 x 6, G 6 x 3, AT 4 x 6) in float64: the rows wino4_consts.inc and filter_layout.hip (winograd4_filter) state."""
    if a is None:
        a, b = points()
    a2, b2 = a * a, b * b
    BT = np.array([[a2 * b2, 0, -(a2 + b2), 0, 1, 0],
                   [0, -a * b2, -b2, a, 1, 0],
                   [0, a * b2, -b2, -a, 1, 0],
                   [0, -a2 * b, -a2, b, 1, 0],
                   [0, a2 * b, -a2, -b, 1, 0],
                   [0, a2 * b2, 0, -(a2 + b2), 0, 1]])
    na, nb = 2 * a2 * (a2 - b2), 2 * b2 * (b2 - a2)
    G = np.array([[1 / (a2 * b2), 0, 0],
                  [1 / na, a / na, a2 / na],
                  [1 / na, -a / na, a2 / na],
                  [1 / nb, b / nb, b2 / nb],
                  [1 / nb, -b / nb, b2 / nb],
                  [0, 0, 1]])
    AT = np.array([[1, 1, 1, 1, 1, 0],
                   [0, a, -a, b, -b, 0],
                   [0, a2, a2, b2, b2, 0],
                   [0, a2 * a, -a2 * a, b2 * b, -b2 * b, 1]])
    return BT, G, AT


# ---- float32 arithmetic on float32-valued float64 arrays -------------------------------------------------------------------------------
def f32(x):
    return np.asarray(x, np.float64).astype(np.float32).astype(np.float64)


def fma(a, b, c):
    """float32 fma: the product of two float32 is exact in float64, one rounding of the sum to 53 bits and one to 24 (double rounding at
    2^-29 relative: negligible for error statistics)."""
    return f32(a * b + c)


def bf16_trunc(x):
    """The high 16 bits of a float32 (the truncation the split kernel and wino4s_filter_kernel use), as float64."""
    bits = np.asarray(x, np.float64).astype(np.float32).view(np.uint32) & np.uint32(0xffff0000)
    return bits.view(np.float32).astype(np.float64)


def split3(x):
    """x = x1 + x2 + x3 exactly, 8 significant bits each: x1 = hi16(x), x2 = hi16(x - x1), x3 = x - x1 - x2 (both differences exact)."""
    x1 = bf16_trunc(x)
    r = f32(x - x1)
    x2 = bf16_trunc(r)
    return x1, x2, bf16_trunc(f32(r - x2))


# ---- tiles -----------------------------------------------------------------------------------------------------------------------------
class Tiles:
    """The 6 x 6 input tiles of a layer (x NHWC float32, 'same' zero halo; H and W multiples of 4) that hold a non-zero, and the output
    channels whose filter slice holds one.  ``d`` (T, 6, 6, Cin) float64, ``w`` (3, 3, Cin, K) float64, ``idx`` (T, 3) = (n, ty, tx)."""

    def __init__(self, x, w, everything=False):
        x, w = np.asarray(x), np.asarray(w)
        assert x.dtype == np.float32 and w.dtype == np.float32 and w.shape[:3] == (3, 3, x.shape[3])
        n, h, wd, c = x.shape
        assert h % 4 == 0 and wd % 4 == 0
        self.shape, self.cin, self.cout = (n, h, wd), c, w.shape[3]
        xp = np.zeros((n, h + 2, wd + 2, c), np.float32)
        xp[:, 1:-1, 1:-1] = x
        nz = np.ascontiguousarray((xp != 0).any(axis=-1))
        s = nz.strides
        self.active = as_strided(nz, (n, h // 4, wd // 4, 6, 6), (s[0], 4 * s[1], 4 * s[2], s[1], s[2])).any(axis=(3, 4))
        if everything:                                            # (the tests of the skipping itself)
            self.active = np.ones_like(self.active)
        self.idx = np.argwhere(self.active)
        s = xp.strides
        win = as_strided(xp, (n, h // 4, wd // 4, 6, 6, c), (s[0], 4 * s[1], 4 * s[2], s[1], s[2], s[3]))
        self.d = win[self.idx[:, 0], self.idx[:, 1], self.idx[:, 2]].astype(np.float64)
        self.chans = np.arange(w.shape[3]) if everything else np.flatnonzero((w != 0).any(axis=(0, 1, 2)))
        self.w = w.astype(np.float64)[..., self.chans]

    def _six(self, a):
        n, h, wd = self.shape
        return a.reshape(n, h // 4, 4, wd // 4, 4, self.cout)

    def scatter(self, vals, fill):
        """vals (T, 4, 4, K) -> (N, H, W, Cout) float64, ``fill`` (Cout,) everywhere else."""
        out = np.empty(self.shape + (self.cout,), np.float64)
        out[...] = np.asarray(fill, np.float64)
        six = self._six(out)
        i = self.idx
        blk = six[i[:, 0], i[:, 1], :, i[:, 2], :, :]
        blk[..., self.chans] = vals
        six[i[:, 0], i[:, 1], :, i[:, 2], :, :] = blk
        return out

    def gather(self, full):
        """(N, H, W, Cout) -> its values at the active tiles and channels, (T, 4, 4, K)."""
        i = self.idx
        return self._six(np.asarray(full))[i[:, 0], i[:, 1], :, i[:, 2], :, :][..., self.chans]

    def rest_equals(self, full, fill):
        """Every output outside the active tiles and channels equals ``fill`` (Cout,) bit for bit (as float32 values; -0.0 == 0.0)."""
        ok = np.asarray(full) == np.asarray(fill, np.float32)
        six = self._six(ok)
        i = self.idx
        blk = six[i[:, 0], i[:, 1], :, i[:, 2], :, :]
        blk[..., self.chans] = True
        six[i[:, 0], i[:, 1], :, i[:, 2], :, :] = blk
        return bool(ok.all())


def truth_tiles(t, bias=None):
    """Float64 direct correlation of the active tiles -> (T, 4, 4, K), bias added."""
    y = np.zeros((len(t.idx), 4, 4, len(t.chans)))
    for ky in range(3):
        for kx in range(3):
            y += t.d[:, ky:ky + 4, kx:kx + 4, :] @ t.w[ky, kx]
    if bias is not None:
        y += np.asarray(bias, np.float64)[t.chans]
    return y


def scale_tiles(t):
    """Q of the active tiles -> (T, 4, 4, K), float64."""
    BT, G, AT = (np.abs(m) for m in matrices())
    av = np.einsum('ij,tjkc,lk->tilc', BT, np.abs(t.d), BT, optimize=True)
    au = np.einsum('ij,jkco,lk->ilco', G, np.abs(t.w), G, optimize=True)
    p = np.empty((len(t.idx), 6, 6, len(t.chans)))
    for i in range(6):
        for l in range(6):
            p[:, i, l, :] = av[:, i, l, :] @ au[i, l]
    return np.einsum('yi,tilo,xl->tyxo', AT, p, AT, optimize=True)


# ---- the replay ------------------------------------------------------------------------------------------------------------------------
def input_transform(d, a, b):
    """V = B^T d B of tiles d (T, 6, 6, C) as the kernels form it: the row transform t[xi] = c0 d[r0] + c1 d[r1] + c2 d[r2] + d[r3] as ONE
    fma chain per row, innermost term first (row_pass of wino4r / wino4s, transform of wino4_kernel.hip), the column transform with the
    shared even / odd parts of the +- points (mfma_stage / point).  -> (T, xi, nu, C)."""
    a2, b2 = a * a, b * b
    rows = [(0, 2, 4, None, a2 * b2, -(a2 + b2), None), (1, 2, 3, 4, -a * b2, -b2, a), (1, 2, 3, 4, a * b2, -b2, -a),
            (1, 2, 3, 4, -a2 * b, -a2, b), (1, 2, 3, 4, a2 * b, -a2, -b), (1, 3, 5, None, a2 * b2, -(a2 + b2), None)]
    t = []
    for r0, r1, r2, r3, c0, c1, c2 in rows:                         # t[xi]: (T, 6 columns, C)
        if r3 is None:
            t.append(fma(c0, d[:, r0], fma(c1, d[:, r1], d[:, r2])))
        else:
            t.append(fma(c0, d[:, r0], fma(c1, d[:, r1], fma(c2, d[:, r2], d[:, r3]))))
    t = np.stack(t, axis=1)                                          # (T, xi, j, C)
    u = [t[:, :, j] for j in range(6)]
    ea, oa = fma(-b2, u[2], u[4]), fma(-b2, u[1], u[3])
    eb, ob = fma(-a2, u[2], u[4]), fma(-a2, u[1], u[3])
    return np.stack([fma(a2 * b2, u[0], fma(-(a2 + b2), u[2], u[4])), fma(a, oa, ea), fma(-a, oa, ea), fma(b, ob, eb), fma(-b, ob, eb),
                     fma(a2 * b2, u[1], fma(-(a2 + b2), u[3], u[5]))], axis=2)


def filter_transform(g, a, b):
    """U = G g G^T of filters g (3, 3, C, K): float64, ONE rounding to float32 (winograd4_filter) -> (xi, nu, C, K)."""
    G = matrices(a, b)[1]
    return f32(np.einsum('ik,klco,jl->ijco', G, np.asarray(g, np.float64), G, optimize=True))


def fold(m, a, b):
    """Six planes -> four, the output transform of the fp32 kernels (write_R, wino4_combine.inc): s12, d12, s34, d34 first."""
    a2, b2 = a * a, b * b
    s12, d12, s34, d34 = f32(m[1] + m[2]), f32(m[1] - m[2]), f32(m[3] + m[4]), f32(m[3] - m[4])
    r0 = f32(f32(m[0] + s12) + s34)
    r1 = fma(a, d12, f32(b * d34))
    r2 = fma(a2, s12, f32(b2 * s34))
    r3 = f32(fma(a2 * a, d12, f32(b2 * b * d34)) + m[5])
    return [r0, r1, r2, r3]


def fold_halves(m, a, b):
    """The first fold of conv_wino4s_kernel: a wave holds HALF a row - (m0, m+a, m-a) or (minf, m+b, m-b) - half 0 writes the exchange
    image, half 1 adds onto it."""
    a2, b2 = a * a, b * b
    sa, da, sb, db = f32(m[1] + m[2]), f32(m[1] - m[2]), f32(m[3] + m[4]), f32(m[3] - m[4])
    r0 = f32(f32(m[0] + sa) + sb)
    r1 = f32(f32(a * da) + f32(b * db))
    r2 = f32(f32(a2 * sa) + f32(b2 * sb))
    r3 = f32(f32(a2 * a * da) + fma(b2 * b, db, m[5]))
    return [r0, r1, r2, r3]


def channel_sum(V, U, mode):
    """M[t, xi, nu, k] = sum_c V[t, xi, nu, c] U[xi, nu, c, k].

    fp32    one float32 fma per input channel, in channel order (v_mfma_f32_32x32x2_f32: every product enters the accumulator on its own).
    bf16x3  wino4s_kernel.hip: both operands split exactly into three bf16 pieces by truncation (``split3``); per 8-channel group (Cin % 8
            == 4: the missing channels are zeros) THREE v_mfma_f32_32x32x16_bf16, each over 8 channels x 2 piece products, in this order:
                [v3|v1] x [u1|u3] = v3 u1 + v1 u3,     [v1|v2] x [u2|u1] = v1 u2 + v2 u1,     [v2|v1] x [u2|u1] = v2 u2 + v1 u1
            (smallest first; v2 u3, v3 u2, v3 u3 are dropped).  A product of two bf16 is exact in float32; an MFMA's 16 products are
            summed here without rounding and added to the float32 accumulator with one rounding."""
    T, C, K = V.shape[0], V.shape[3], U.shape[3]
    M = np.zeros((T, 6, 6, K))
    if mode == 'fp32':
        for c in range(C):
            M = fma(V[:, :, :, c, None], U[None, :, :, c, :], M)
        return M
    assert mode == 'bf16x3', mode
    v1, v2, v3 = split3(V)
    u1, u2, u3 = split3(U)
    dot = lambda p, q, s: np.einsum('tijc,ijck->tijk', p[..., s], q[:, :, s, :], optimize=True)
    for g0 in range(0, C, 8):
        s = slice(g0, min(g0 + 8, C))
        M = f32(M + (dot(v3, u1, s) + dot(v1, u3, s)))
        M = f32(M + (dot(v1, u2, s) + dot(v2, u1, s)))
        M = f32(M + (dot(v2, u2, s) + dot(v1, u1, s)))
    return M


def output_transform(M, a, b, mode):
    """(T, xi, nu, K) -> (T, 4, 4, K): R = M A row by row (the wave's own fold), then Y = A^T R (the combine step)."""
    first = fold_halves if mode == 'bf16x3' else fold
    R = np.stack(first([M[:, :, j] for j in range(6)], a, b), axis=2)          # (T, xi, 4, K)
    return np.stack(fold([R[:, j] for j in range(6)], a, b), axis=1)           # (T, 4, 4, K)


def replay_tiles(t, bias=None, mode='fp32', V=None):
    """The kernels' float32 result on the active tiles -> (T, 4, 4, K) (before the activation).  ``V``: a transformed input from an
    earlier call on the same data."""
    a, b = points()
    if V is None:
        V = input_transform(t.d, a, b)
    y = output_transform(channel_sum(V, filter_transform(t.w, a, b), mode), a, b, mode)
    if bias is not None:
        y = f32(y + np.asarray(bias, np.float64)[t.chans])
    return y


def kernel_order_error(a, b, cin, cout=16, tiles=64, seed=0):
    """tools/wino_points.py's experiment: relative rms error of the fp32 replay on ``tiles`` seeded 6 x 6 tiles of ReLU-like data against He-normal
    filters, for the symmetric point set {0, +-a, +-b, inf}."""
    rng = np.random.default_rng(seed)
    d = f32(np.maximum(rng.normal(0, 1, (tiles, cin, 6, 6)), 0))
    g = f32(rng.normal(0, np.sqrt(2.0 / (9 * cin)), (cout, cin, 3, 3)))
    truth = np.zeros((tiles, cout, 4, 4))
    for ky in range(3):
        for kx in range(3):
            truth += np.einsum('tcyx,oc->toyx', d[:, :, ky:ky + 4, kx:kx + 4], g[:, :, ky, kx])
    V = input_transform(d.transpose(0, 2, 3, 1), a, b)
    Y = output_transform(channel_sum(V, filter_transform(g.transpose(2, 3, 1, 0), a, b), 'fp32'), a, b, 'fp32')
    Y = np.ascontiguousarray(Y.transpose(0, 3, 1, 2))               # (tiles, cout, 4, 4), as truth
    scale = np.sqrt((truth ** 2).mean())
    return float(np.sqrt(((Y - truth) ** 2).mean()) / scale)


# ---- tails -----------------------------------------------------------------------------------------------------------------------------
def _spec(act):
    """An activation as (name, alpha): a plain name, or (name, alpha) with LeakyReLU's slope, ELU's alpha or ReLU's max_value."""
    return (act, None) if isinstance(act, str) else (act[0], act[1])


def act64(y, act):
    """The activation in float64, each in the form that does not cancel.  ``act``: a name (linear, relu, sigmoid, tanh, elu, swish) or
    (name, alpha) for leaky_relu / elu / relu_clip."""
    name, alpha = _spec(act)
    y = np.asarray(y, np.float64)
    with np.errstate(over='ignore', under='ignore'):
        if name == 'linear':
            return y
        if name == 'relu':
            return np.maximum(y, 0)
        if name == 'relu_clip':
            return np.clip(y, 0.0, alpha)
        if name == 'leaky_relu':
            return np.where(y > 0, y, alpha * y)
        if name in ('sigmoid', 'swish'):
            e = np.exp(-np.abs(y))
            s = np.where(y >= 0, 1.0 / (1.0 + e), e / (1.0 + e))
            return s if name == 'sigmoid' else y * s
        if name == 'tanh':
            return np.tanh(y)
        if name == 'elu':
            return np.where(y > 0, y, (1.0 if alpha is None else alpha) * np.expm1(np.minimum(y, 0.0)))
    raise AssertionError('no activation %r' % (act,))


FLT_MIN, DENORMAL = 2.0 ** -126, 2.0 ** -149
SECOND = 1.0 + 2.0 ** -10          # the products of errors that a first-order count leaves out (as in tests/test_gpu_layers.py)


def act_lip(act):
    """The largest |act'| anywhere: what an error of the argument is multiplied by at most."""
    name, alpha = _spec(act)
    if name in ('linear', 'relu', 'relu_clip', 'tanh'):
        return 1.0
    if name == 'sigmoid':
        return 0.25
    if name == 'elu':
        return max(1.0, 1.0 if alpha is None else abs(alpha))     # alpha e^v for v <= 0
    if name == 'leaky_relu':
        return max(1.0, abs(alpha))
    raise AssertionError('no Lipschitz constant for %r' % (act,))


def act_own(v, act, expm1=False):
    """-> (bound, exact): the error of the convolution kernels' own float32 evaluation of act at the float32 argument v, as an absolute
    bound per element (derived in tests/test_gpu_conv_tails.py from OCML's documented ceilings, as tests/test_gpu_layers.py's table is);
    ``exact``: the result is one of the inputs or a constant (the select class: bound 0).  ``expm1``: the element-wise kernels' ELU
    (dwconv_kernel, apply_act_ext: alpha * expm1f(v)) instead of the convolution kernels' alpha * (expf(v) - 1.f)."""
    name, alpha = _spec(act)
    v = np.asarray(v, np.float64)
    want = np.abs(act64(v, act))
    if name in ('linear', 'relu', 'relu_clip'):
        return np.zeros_like(v), True
    if name == 'leaky_relu':
        return U32 * want + DENORMAL, False
    if name in ('sigmoid', 'swish'):
        floor = FLT_MIN
        if name == 'swish':
            floor = np.where(-v > np.log(float(np.finfo(np.float32).max)), np.abs(v) / float(np.finfo(np.float32).max), FLT_MIN)
        return 8 * U32 * want * SECOND + floor, False
    if name == 'tanh':
        return 10 * U32 * want * SECOND + FLT_MIN, False
    if name == 'elu':
        a = 1.0 if alpha is None else abs(alpha)
        if expm1:
            return 7 * U32 * want * SECOND + FLT_MIN, False
        ev = np.exp(np.minimum(v, 0.0))
        return np.where(v > 0, 0.0, a * U32 * (6 * ev + 2 * np.abs(ev - 1.0)) * SECOND + FLT_MIN), False
    raise AssertionError('no bound for %r' % (act,))


def act32(y, act):
    """The convolution kernels' float32 evaluation of act on float32 values, as float64 arrays of float32 values (the replay's tail): the
    float64 function rounded once, except ELU, which follows the kernels' alpha * (expf(v) - 1.f)."""
    name, alpha = _spec(act)
    y = f32(y)
    if name == 'elu':
        a = 1.0 if alpha is None else alpha
        with np.errstate(under='ignore'):
            return np.where(y > 0, y, f32(a * f32(f32(np.exp(np.minimum(y, 0.0))) - 1.0)))
    return f32(act64(y, act))


def pool2(y, how=np.max):
    n, h, w, c = y.shape
    return how(y.reshape(n, h // 2, 2, w // 2, 2, c), axis=(2, 4))


def softmax64(l):
    e = np.exp(l - l.max(axis=-1, keepdims=True))
    return e / e.sum(axis=-1, keepdims=True)


def head_replay(y, hw, hb, act='softmax'):
    """The fused 1 x 1 head (wino4_combine.inc, wino4_head.inc) in float32: per pass of 32 channels a lane adds the products of its
    channel quad onto its partial logits, a butterfly over the eight lanes of a pixel, the bias, then softmax over the k <= 4 classes with
    float32 exp, or the head's activation (``act32``)."""
    hw, hb = np.asarray(hw, np.float64).reshape(-1, np.asarray(hw).shape[-1]), np.asarray(hb, np.float64)
    cout, k = hw.shape
    assert cout == 64 and 1 <= k <= 4
    part = [np.zeros(y.shape[:-1] + (k,)) for _ in range(8)]
    for p in range(2):
        for q in range(8):
            c0 = 32 * p + 4 * q
            acc = f32(y[..., c0, None] * hw[c0])
            for e in range(1, 4):
                acc = fma(y[..., c0 + e, None], hw[c0 + e], acc)
            part[q] = f32(part[q] + acc)
    for step in (1, 2, 4):
        part = [f32(part[q] + part[q ^ step]) for q in range(8)]
    l = f32(part[0] + hb)
    if _spec(act)[0] != 'softmax':
        return act32(l, act)
    e = f32(np.exp(f32(l - l.max(axis=-1, keepdims=True))))
    s = e[..., 0]
    for c in range(1, k):
        s = f32(s + e[..., c])
    return f32(e / s[..., None])


HEAD_OWN = 12          # roundings on a product's way through the head: multiply, 3 adds of the quad, 2 accumulations, 3 butterfly adds, bias, + 2
SOFTMAX_OWN = 16       # exp (<= 4 ulp allowed), three adds, the divide, numerator and denominator


def truth(x, w, b=None, act='linear', tail=None, head=None):
    """Float64 direct 3 x 3 'same' correlation of x (N, H, W, Cin) with w (3, 3, Cin, Cout) + bias, the activation, then ``tail``: None,
    'pool' (2 x 2 max-pool) or 'head' (``head`` = (weights (Cout, k) or (1, 1, Cout, k), bias): 1 x 1 convolution + softmax)."""
    t = Tiles(x, w)
    fill = np.zeros(t.cout) if b is None else np.asarray(b, np.float64)
    y = act64(t.scatter(truth_tiles(t, b), fill), act)
    if tail == 'pool':
        return pool2(y)
    if tail == 'head':
        hw, hb = head
        hw = np.asarray(hw, np.float64).reshape(t.cout, -1)
        return softmax64(y @ hw + np.asarray(hb, np.float64))
    assert tail is None, tail
    return y


def scale(x, w):
    """Q at every output of the layer, (N, H, W, Cout) float64."""
    t = Tiles(x, w)
    return t.scatter(scale_tiles(t), np.zeros(t.cout))


def pool_scale(q):
    """A pooled output moves by at most the largest move of its four inputs."""
    return pool2(q)


def head_scale(q, y, head, act='softmax', feat_own=None):
    """-> (S, own) of the head's outputs, both (N, H, W, k), k <= 4 classes.  Per class S_k = sum_o |h_ok| Q_o, the convolution's scale
    carried through the 1 x 1 layer, and own_k = HEAD_OWN u (sum_o |h_ok| |y_o| + |hb_k|), the head's own roundings on the logit, plus
    sum_o |h_ok| feat_own_o where the features carry an error of their own (``feat_own``: the convolution's activation).

    softmax   is 1-Lipschitz in the max norm, so every class moves by at most the largest move of a logit: S and own are the maxima over the
              classes, and own gains SOFTMAX_OWN u + 2 u (max l - min l) for the softmax itself (outputs <= 1; the float32 difference
              l - max carries u |l - max| into the exponent).  One class: the output is e^0 / e^0 = 1 whatever the logit.
    other     S_k and own_k times the head activation's Lipschitz constant (``act_lip``), plus its own bound at the logit (``act_own``).
              SECOND on the L own term: the device evaluates the activation at its own logit, not at l, and act_own is at most 10 u times
              a function of slope <= L, so it moves by at most 10 u L own."""
    hw, hb = head
    hw, hb = np.abs(np.asarray(hw, np.float64).reshape(q.shape[-1], -1)), np.asarray(hb, np.float64)
    k = hw.shape[1]
    S = q @ hw
    l = y @ np.asarray(head[0], np.float64).reshape(q.shape[-1], -1) + hb
    own = HEAD_OWN * U32 * (np.abs(y) @ hw + np.abs(hb))
    if feat_own is not None:
        own = own + feat_own @ hw
    if _spec(act)[0] == 'softmax':
        S, own = S.max(axis=-1, keepdims=True), own.max(axis=-1, keepdims=True)
        own = own + U32 * (SOFTMAX_OWN + 2 * (l.max(axis=-1, keepdims=True) - l.min(axis=-1, keepdims=True)))
        return np.repeat(S, k, axis=-1), np.repeat(own, k, axis=-1)
    L = act_lip(act)
    return L * S, L * own * SECOND + act_own(l, act)[0]


def replay(x, w, b=None, mode='fp32', act='linear', tail=None, head=None):
    """The float32 replay of a whole NHWC layer: 4 x 4 tiling, zero halo, bias, activation and tail -> float64 array of float32 values.
    (Cin % 8 == 4: the kernels pad the last group with zero channels, which add exact zeros - nothing to replay.)"""
    t = Tiles(x, w)
    fill = np.zeros(t.cout) if b is None else f32(b)
    y = act64(t.scatter(replay_tiles(t, b, mode), fill), act)
    if tail == 'pool':
        return pool2(y)
    if tail == 'head':
        return head_replay(y, *head)
    assert tail is None, tail
    return y


def hard_count(cin, mode):
    """First-order count of the roundings on the path of ONE output, each bounded by u Q (u = 2^-24), read off the kernel sources:

    3   row transform: t = fma(c0, d0, fma(c1, d1, fma(c2, d2, d3))) - a term passes through at most three roundings (row_pass);
    2   column transform: e = fma(-k, t2, t4), o = fma(-k, t1, t3), V = fma(+-r, o, e), or fma(KP, t0, fma(KS, t2, t4)): at most two;
        together |V^ - V| <= 5 u |B^T| |d| |B|;
    1   U = G g G^T is formed in float64 and rounded once: |U^ - U| <= u |G| |g| |G^T|;
    Cin8  = Cin rounded up to 8, the channel sum: n float32 accumulations in ANY order (sequential, split-K halves, MFMA internals)
        put at most n roundings behind a product, each relative to a partial sum <= sum |V| |U|;
    4   the wave's own fold R = M A: s = m1 + m2 | d = m1 - m2, then at most two more (r0 = (m0 + s12) + s34, r3 = fma(a3, d12, fma(b3,
        d34, m5))), and one for the add that joins the two partial images (split-K in conv_wino4_kernel, half rows in conv_wino4s_kernel);
    4   the combine step Y = A^T R without contraction: s | d, the multiply, two adds (y3 = a3 d12 + b3 d34 + q5);
    1   the bias.  Its own rounding is relative to |y + b| and is the ``u |truth|`` term of the bound; this unit covers the gap between
        this first-order count and (1 + u)^n - 1 (n u < 2^-15 here).

    bf16x3 adds 3: the dropped piece products v2 u3 + v3 u2 + v3 u3, documented in wino4s_kernel.hip as <= 3 x 2^-24 |V U| (that figure
    holds for pieces of 2^-8 and 2^-16 relative size; with the kernel's truncating split |v2| < 2^-7 |v| and |v3| < 2^-15 |v|, so the
    worst case of the three is 2^-21 |V U| = 8 u, reached only when every piece of every channel sits at its maximum).  The six kept
    products are exact in float32; the three MFMAs of a group are charged the group's 8 units of Cin8.
    """
    assert mode in ('fp32', 'bf16x3'), mode
    cin8 = -(-cin // 8) * 8
    return 3 + 2 + 1 + cin8 + 4 + 4 + 1 + (3 if mode == 'bf16x3' else 0)
