"""The cases of tests/test_wino4_ref.py (CPU) and tests/test_gpu_wino4_accuracy.py (device): single F(4x4) layers at the smallest shapes that
reach every arm of conv_wino4r_kernel, conv_wino4_kernel and conv_wino4s_kernel - tools/wino4_layer_digests.py's LAYERS plus one deep channel
sum - and the seeded data families they run on.  TEST INFRASTRUCTURE ONLY.

    odd_regions   3 x 16 x 16, 8 -> 64      an odd region count          cout96    2 x 32 x 32, 64 -> 96    Cout % 64 == 32
    tail4         2 x 32 x 48, 12 -> 64     the Cin % 8 == 4 tail        split_k   2 x 32 x 32, 64 -> 32    conv_wino4_kernel (and wino4_split = 0)
    pool          2 x 32 x 32, 24 -> 64     + fused 2 x 2 max-pool       head      2 x 32 x 32, 16 -> 64    + fused 4-class softmax head
    deep          2 x 16 x 16, 256 -> 64    a long channel sum

A case (``build``) is a dict: ``name``, ``cfg`` / ``weights`` / ``x`` for keras_plan.build_plan and forward_patches, ``layer`` = (input of the
layer under test, filter, bias or None, activation), ``tail`` (None / 'pool' / 'head') and ``head`` (weights, bias), ``bits`` (the fusion bits
expected in the launch profile), and for the delta families ``tap`` = (r, q, ci, co).  ``evaluate`` holds a result - the device's or the
replay's - against float64 truth.
"""
import zlib

import numpy as np

from ecseg_amd import keras_plan
from tests import conv_exact_cases as cx
from tests import wino4_ref as ref
from tools import wino4_layer_digests as wd

SHAPES = dict(wd.LAYERS, deep=(2, 16, 16, 256, 64, None))
PLAIN = tuple(k for k, v in SHAPES.items() if v[5] is None)
FAMILIES = ('dense', 'disparate', 'delta_input', 'delta_filter', 'view')
TILE, REGION = 4, 16
BATCH = 128                              # images per forward_patches call (delta_input has hundreds)


def options(shape):
    """The library options a case runs under: winograd 2 and 3; the lone 32-channel block also unsplit."""
    out = [dict(winograd=2, wino4_split=1), dict(winograd=3, wino4_split=1)]
    if SHAPES[shape][4] == 32:
        out += [dict(winograd=2, wino4_split=0), dict(winograd=3, wino4_split=0)]
    return [dict(cx.LIBRARY_DEFAULTS, **o) for o in out]


def mode_of(shape, opts):
    """The arithmetic a case runs under ``opts``: where Cout % 64 != 0, winograd = 3 falls back to the fp32 kernels."""
    return 'bf16x3' if (opts['winograd'] >= 3 and SHAPES[shape][4] % 64 == 0) else 'fp32'


def kind_of(shape, opts):
    return 5 if mode_of(shape, opts) == 'bf16x3' else 2


def opts_id(o):
    return 'winograd%d_split%d' % (o['winograd'], o['wino4_split'])


def _rng(*key):
    return np.random.default_rng(zlib.crc32('/'.join(str(k) for k in key).encode()))


def _f32(a):
    return np.ascontiguousarray(a, np.float32)


def _single(name, shape, x, w, b, act, **more):
    n, H, W, cin, cout, tail = SHAPES[shape]
    layers = [cx._in(H, W, cin), cx.conv_layer('op', 'in', cout, 3, act=act, bias=b is not None)]
    return dict(name=name, shape=shape, cfg=cx._F(layers, 'op'), weights={'op': [w] + ([b] if b is not None else [])}, x=x,
                layer=(x, w, b, act), tail=None, head=None, bits=0, **more)


def dense_data(shape, key='dense'):
    n, H, W, cin, cout, tail = SHAPES[shape]
    rng = _rng(key, shape)
    return (_f32(rng.normal(size=(n, H, W, cin))), _f32(rng.normal(size=(3, 3, cin, cout)) / np.sqrt(9 * cin)), _f32(rng.normal(size=cout)))


def dense(shape, act):
    x, w, b = dense_data(shape)
    return _single('%s/dense/%s' % (shape, act), shape, x, w, b, act)


def disparate(shape, act):
    """Dense data with channel c of x scaled by 2^k_c and its filter slice by 2^-k_c, k_c in -10 .. 10 (exact scalings: the truth keeps its
    size, the intermediate magnitudes - and Q - do not care, a per-layer max norm of x or w is off by up to 2^10)."""
    x, w, b = dense_data(shape, 'disparate')
    k = _rng('disparate_k', shape).integers(-10, 11, size=x.shape[3]).astype(np.float64)
    x = _f32(x * 2.0 ** k)
    w = _f32(w * 2.0 ** -k[None, None, :, None])
    return _single('%s/disparate/%s' % (shape, act), shape, x, w, b, act)


def seam_lines(n):
    """Both sides of every 4-pixel tile seam of an axis of n pixels (every 16-pixel region seam is one of them)."""
    return sorted({v for t in range(TILE, n, TILE) for v in (t - 1, t)})


def delta_positions(H, W):
    """conv_exact_cases.impulse_positions' construction with 4 x 4 tiles and 16 x 16 regions: every corner, pixels of every edge and both
    sides of every seam, in all combinations.  (The patch seam - the last rows of one image next to the first rows of the next in memory -
    is reached by the edge positions: neighbouring images carry their impulses on the facing edges.)"""
    assert H % REGION == 0 and W % REGION == 0
    ys = sorted({0, 1, H - 1} | set(seam_lines(H)))
    xs = sorted({0, 1, (W - 1) // 2, W - 1} | set(seam_lines(W)))
    return [(y, x) for y in ys for x in xs]


def delta_channels(cin):
    """All 8 slots of the first 8-channel group and every channel of the last group (the 4-channel tail where Cin % 8 == 4)."""
    last = (cin - 1) // 8 * 8
    return sorted(set(range(8)) | set(range(last, cin)))


def full_significands(rng, shape, lo=-6, hi=6):
    """float32 with all 24 significand bits in use (odd significands), magnitudes 2^lo .. 2^hi, both signs."""
    mant = (rng.integers(2 ** 23, 2 ** 24, size=shape) | 1).astype(np.float64)
    v = mant * 2.0 ** (rng.integers(lo, hi, size=shape) - 23.0) * rng.choice([-1.0, 1.0], size=shape)
    out = v.astype(np.float32)
    assert np.array_equal(out.astype(np.float64), v)
    return out


def delta_input(shape):
    """One image per position: a single 1.0 (image i in channel ``delta_channels``[i % len]), full-significand weights, no bias, linear."""
    n, H, W, cin, cout, tail = SHAPES[shape]
    pos, chs = delta_positions(H, W), delta_channels(cin)
    assert len(pos) >= len(chs)
    x = np.zeros((len(pos), H, W, cin), np.float32)
    for i, (y, xx) in enumerate(pos):
        x[i, y, xx, chs[i % len(chs)]] = 1.0
    w = full_significands(_rng('delta_input', shape), (3, 3, cin, cout))
    return _single('%s/delta_input' % shape, shape, x, w, None, 'linear', positions=pos)


def delta_filter_pairs(shape):
    """conv_exact_cases.delta_filter_cases' construction: one pair per tap, the (ci, co) pair moving along, then one pair for every 4-channel
    group of Cin and every 32-channel block of Cout (both halves of every 64-block, the lone 32-block) that the taps have not reached."""
    n, H, W, cin, cout, tail = SHAPES[shape]
    ci_list = [cx._group_pick(g, cin) for g, _ in cx.channel_groups(cin)]
    co_list = [b + (5 * (b // 32) + 3) % 32 for b in range(0, cout, 32)]
    pairs = [(r, q, ci_list[t % len(ci_list)], co_list[(t // 2) % len(co_list)]) for t, (r, q) in enumerate((r, q) for r in range(3) for q in range(3))]
    ci_seen, co_seen = {p[2] for p in pairs}, {p[3] for p in pairs}
    pairs += [(2, 2, ci, co_list[-1]) for ci in ci_list if ci not in ci_seen]
    pairs += [(2, 2, ci_list[-1], co) for co in co_list if co not in co_seen]
    return pairs


def delta_filter(shape):
    """-> one case per pair: tap (r, q) of (ci, co) is 1.0, every other weight 0; dense data; an arbitrary bias, 0 on ``co``; linear."""
    n, H, W, cin, cout, tail = SHAPES[shape]
    x = dense_data(shape, 'delta_filter')[0]
    rng = _rng('delta_filter_bias', shape)
    out = []
    for r, q, ci, co in delta_filter_pairs(shape):
        w = np.zeros((3, 3, cin, cout), np.float32)
        w[r, q, ci, co] = 1.0
        b = full_significands(rng, (cout,), -3, 3)
        b[co] = 0.0
        out.append(_single('%s/delta_filter/tap%d_%d_ci%d_co%d' % (shape, r, q, ci, co), shape, x, w, b, 'linear', tap=(r, q, ci, co)))
    return out


def view(shape, act='linear'):
    """conv_exact_cases.concat_case's graph - three convolutions whose outputs are the members of a Concatenate and are written straight into
    its buffer - with the layer under test reading the LAST member: a channel view at offset 8 of a buffer of Cin + 8 channels.  The three
    are 1 x 1 convolutions with 0 / 1 weights and no bias, so each output is one product x * 1.0 plus exact zeros on any kernel: member 'c' is
    the input with its channels rotated by one, and the layer under test sees exactly known data."""
    n, H, W, cin, cout, tail = SHAPES[shape]
    x, w, b = dense_data(shape, 'view')
    layers, weights = [cx._in(H, W, cin)], {}
    for nm, co in zip('abc', (4, 4, cin)):
        layers.append(cx.conv_layer(nm, 'in', co, 1, act='linear', bias=False))
        sel = np.zeros((1, 1, cin, co), np.float32)
        for o in range(co):
            sel[0, 0, (o + 1) % cin, o] = 1.0
        weights[nm] = [sel]
    layers.append(cx._L('Concatenate', 'cat', ['a', 'b', 'c'], axis=-1))
    layers.append(cx.conv_layer('op', 'c', cout, 3, act=act, bias=True))
    weights['op'] = [w, b]
    x_in = np.ascontiguousarray(np.roll(x, -1, axis=3))             # channel o of 'c' = channel (o + 1) % Cin of x
    return dict(name='%s/view/%s' % (shape, act), shape=shape, cfg=cx._F(layers, 'op'), weights=weights, x=x, layer=(x_in, w, b, act), tail=None,
                head=None, bits=0, in_view=True)


def tail_case(shape):
    """'pool' and 'head' as tools/wino4_layer_digests.py builds them (same seeds), with ReLU: every value the tail sees is >= 0."""
    n, H, W, cin, cout, tail = SHAPES[shape]
    cfg, w, x = wd.layer_model(shape, 'relu')
    head = (w['h'][0].reshape(cout, -1), w['h'][1]) if tail == 'head' else None
    return dict(name='%s/dense/relu' % shape, shape=shape, cfg=cfg, weights=w, x=x, layer=(x, w['c'][0], w['c'][1], 'relu'), tail=tail, head=head,
                bits=0x100 if tail == 'pool' else 0x200)


def build(shape, family):
    """-> the list of cases of one (shape, family)."""
    if SHAPES[shape][5] is not None:
        assert family == 'dense'
        return [tail_case(shape)]
    if family in ('dense', 'disparate'):
        return [{'dense': dense, 'disparate': disparate}[family](shape, act) for act in ('linear', 'relu')]
    if family == 'delta_input':
        return [delta_input(shape)]
    if family == 'delta_filter':
        return delta_filter(shape)
    assert family == 'view', family
    return [view(shape)]


def all_groups():
    return [(s, f) for s in PLAIN for f in FAMILIES] + [(s, 'dense') for s in SHAPES if s not in PLAIN]


def plan_of(case):
    return keras_plan.build_plan(case['cfg'], case['weights'], fuse=True)


def layer_under_test(plan):
    """conv_exact_cases.conv_paths' record of the LAST 3 x 3 convolution of the plan."""
    recs = [d for d in cx.conv_paths(plan) if plan.ops[d['op']]['kh'] == 3]
    return recs[-1]


# ---- a result against the truth -----------------------------------------------------------------------------------------------------------
class Reference:
    """Truth, scale and replays of one case, formed once.  Plain cases stay on the active tiles and channels (``ref.Tiles``); the inactive
    outputs must equal act(bias) bit for bit.  Pool and head cases are dense: whole arrays."""

    def __init__(self, case, V_cache=None):
        x, w, b, act = case['layer']
        self.case, self.act, self.b = case, act, b
        self.t = t = ref.Tiles(x, w)
        self.fill = ref.act64(np.zeros(t.cout) if b is None else b.astype(np.float64), act)
        self.V_cache = V_cache if V_cache is not None else {}
        y, q = ref.truth_tiles(t, b), ref.scale_tiles(t)
        self.own = 0.0
        if case['tail'] is None:
            self.truth, self.S = ref.act64(y, act), q
        else:
            assert t.active.all() and len(t.chans) == t.cout
            yf, qf = ref.act64(t.scatter(y, self.fill), act), t.scatter(q, 0.0)
            if case['tail'] == 'pool':
                self.truth, self.S = ref.pool2(yf), ref.pool_scale(qf)
            else:
                self.truth = ref.softmax64(yf @ case['head'][0].astype(np.float64) + case['head'][1].astype(np.float64))
                self.S, self.own = ref.head_scale(qf, yf, case['head'])
        self._replay = {}

    def count(self, mode):
        return ref.hard_count(self.t.cin, mode)

    def bound(self, mode):
        """|result - truth| <= hard_count u Q + u |truth| (+ the head's own roundings) at every output."""
        return self.count(mode) * ref.U32 * self.S + ref.U32 * np.abs(self.truth) + self.own

    def select(self, full):
        """A whole output array -> (the values ``truth`` is stated on, whether every other output equals act(bias) bit for bit)."""
        if self.case['tail'] is not None:
            return np.asarray(full, np.float64), True
        return self.t.gather(full).astype(np.float64), self.t.rest_equals(full, self.fill)

    def replay(self, mode):
        if mode not in self._replay:
            if 'V' not in self.V_cache:
                self.V_cache['V'] = ref.input_transform(self.t.d, *ref.points())
            y = ref.act64(ref.replay_tiles(self.t, self.b, mode, V=self.V_cache['V']), self.act)
            if self.case['tail'] is not None:
                yf = self.t.scatter(y, self.fill)
                y = ref.pool2(yf) if self.case['tail'] == 'pool' else ref.head_replay(yf, *self.case['head'])
            self._replay[mode] = y
        return self._replay[mode]

    def measure(self, vals, mode):
        """vals: ``select``ed values -> dict(rho_max, rho_rms, over = outputs beyond the hard bound, worst = the largest error / bound,
        n = outputs with Q > 0).  rho = |vals - truth| / (u Q) over the outputs with Q > 0; where Q == 0 the hard bound itself asks for
        |error| <= u |truth|."""
        err = np.abs(vals - self.truth)
        bound = self.bound(mode)
        pos = self.S > 0
        rho = err[pos] / (ref.U32 * self.S[pos])
        with np.errstate(divide='ignore', invalid='ignore'):
            ratio = np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), np.where(err > 0, np.inf, 0.0))
        return dict(rho_max=float(rho.max()) if rho.size else 0.0, rho_rms=float(np.sqrt((rho ** 2).mean())) if rho.size else 0.0,
                    over=int((err > bound).sum()), worst=float(ratio.max()), n=int(pos.sum()))


def references(shape, family):
    """-> [(case, Reference)] of a group; the cases of delta_filter share their data, hence one transformed input."""
    cache = {}
    return [(c, Reference(c, cache if family == 'delta_filter' else None)) for c in build(shape, family)]
