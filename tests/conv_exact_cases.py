"""The cases of tests/test_conv_exact.py (CPU) and tests/test_gpu_conv_exact.py (device): inputs on which a convolution path must
equal tests/conv_exact_ref.py bit for bit.  TEST INFRASTRUCTURE ONLY.

A case is a dict: ``name``, ``group``, ``cls`` ('lattice' / 'impulse' / 'identity'), ``cfg``, ``weights``, ``x`` (uint8 or float32 NHWC:
the two entry points of ``forward_patches``), ``opts`` (the library options it runs under, OPTION_DEFAULTS where it says nothing),
``path`` (the path label of ``conv_paths`` that the layer under test must take), ``kind`` (the launch-profile kind of that layer,
or None where the profile does not report the kernel), ``bits`` (the fusion bits 0x100 / 0x200 / 0x400 expected on that record).

* lattice: integer inputs, weights and biases (weights multiples of 4 on the F(2x2) kernels) - ``lattice_groups``, ``random_case``;
* impulse: a delta input against arbitrary float32 weights, a delta filter against arbitrary float32 data - ``impulse_families``;
* identity: ordinary float data on the F(4x4) kernels - ``identity_cases``.

``conv_paths(plan)`` restates which kernel ``ecseg_model_load`` (ecseg_amd/csrc/model_load.hip) gives every convolution op of a plan, and
``profile_kinds(plan, opts)`` what ``run_plan_op`` (ecseg_amd/csrc/plan_run.hip) then records per launch, so that no case silently tests another
path: the CPU test asserts the labels, the device test the recorded kinds.
"""
import zlib

import numpy as np

from ecseg_amd import keras_plan

OPTION_DEFAULTS = dict(winograd=0, wino_resident=1, wino16=1, wino4_split=1, fuse_first=1)
LIBRARY_DEFAULTS = dict(winograd=2, wino_resident=1, wino16=1, wino4_split=1, fuse_first=1)
RANDOM_SEEDS = range(42)

CIN_LIST = (1, 3, 4, 5, 8, 12, 16, 20, 32, 40)
COUT_LIST = (1, 2, 3, 4, 5, 7, 8, 16, 20, 32, 48, 64)

# every path the device test must see: label of conv_paths -> what takes it
PATHS = ('mfma', 'tap', 'wino', 'wino_res', 'wino16', 'first', 'small_cin', 'head', 'head_fused', 'pool_fused', 'first_fused', 'generic',
         'generic_dil', 'grouped', 'dw', 'convt_gemm', 'convt_phase', 'convt_subpixel', 'convt_generic', 'convt_split', 'dense', 'concat_view')


def _L(cls, name, inbound, **cfg):
    return {'class_name': cls, 'name': name, 'config': dict(cfg, name=name),
            'inbound_nodes': [[[i, 0, 0, {}] for i in inbound]] if inbound else []}


def _F(layers, out):
    return {'class_name': 'Functional', 'config': {'name': 'm', 'layers': layers, 'input_layers': [['in', 0, 0]], 'output_layers': [[out, 0, 0]]}}


def _in(h, w, c):
    return _L('InputLayer', 'in', [], batch_input_shape=[None, h, w, c])


def _rng(name):
    return np.random.default_rng(zlib.crc32(name.encode()))


def _f32(a):
    return np.ascontiguousarray(a, np.float32)


def conv_layer(name, src, cout, k, s=1, padding='same', act='linear', bias=True, dil=1, groups=1, cls='Conv2D'):
    k2 = [k, k] if isinstance(k, int) else list(k)
    s2 = [s, s] if isinstance(s, int) else list(s)
    d2 = [dil, dil] if isinstance(dil, int) else list(dil)
    kw = dict(kernel_size=k2, strides=s2, padding=padding, activation=act, use_bias=bias)
    if cls == 'Conv2D':
        kw.update(filters=cout, dilation_rate=d2, groups=groups)
    elif cls == 'Conv2DTranspose':
        kw.update(filters=cout)
    elif cls == 'DepthwiseConv2D':
        kw.update(depth_multiplier=cout, dilation_rate=d2)
    elif cls == 'SeparableConv2D':
        kw.update(filters=cout[1], depth_multiplier=cout[0], dilation_rate=d2)
    return _L(cls, name, [src], **kw)


def int_weights(rng, shape, wmax, step=1):
    return _f32(rng.integers(-(wmax // step), wmax // step + 1, size=shape) * step)


def int_input(rng, shape, as_u8, xmax=255):
    if as_u8:
        return rng.integers(0, xmax + 1, size=shape).astype(np.uint8)
    return _f32(rng.integers(-xmax, xmax + 1, size=shape))


def _case(name, group, cls, layers, weights, x, path, opts=None, kind=None, bits=0, **more):
    return dict(name=name, group=group, cls=cls, cfg=_F(layers, layers[-1]['config']['name']), weights=weights, x=x, path=path,
                opts=dict(OPTION_DEFAULTS, **(opts or {})), kind=kind, bits=bits, **more)


# ---- which kernel a plan's convolution ops take (ecseg_amd/csrc/model_load.hip, ecseg_amd/csrc/plan_run.hip) --------------------------------
def _ntile(cout):
    return 128 if cout % 128 == 0 else 64 if (cout % 64 == 0 or cout > 64) else 32


def conv_paths(plan):
    """-> one dict per OP_CONV / OP_CONVT / OP_DWCONV op, in plan order: op (index), path, and the filter images the op carries
    (wino, wino16, wino4, split1)."""
    out = []
    for idx, o in enumerate(plan.ops):
        if o['op'] not in (keras_plan.OP_CONV, keras_plan.OP_CONVT, keras_plan.OP_DWCONV):
            continue
        ti, to = plan.tensors[o['in0']], plan.tensors[o['out']]
        cin, cout, k, s = ti['c'], to['c'], o['kh'], o['stride']
        d = dict(op=idx, path=None, wino=False, wino16=False, wino4=False, split1=False, cin=cin, cout=cout, h=to['h'], w=to['w'],
                 in_view=ti['c_stride'] != ti['c'], out_view=to['c_stride'] != to['c'], out_offset=to['c_offset'])
        in_al = ti['c_stride'] % 4 == 0 and ti['c_offset'] % 4 == 0 and cin % 4 == 0
        out_al = to['c_stride'] % 4 == 0 and to['c_offset'] % 4 == 0
        if o['op'] == keras_plan.OP_DWCONV:
            d['path'] = 'dw'
        elif o['op'] == keras_plan.OP_CONV:
            dil = max(o.get('dilation', 1), 1)
            square = o['kh'] == o['kw']
            taps_ok = square and k in (1, 2, 3)
            tap_ok = in_al and cin >= 8 and cout >= 8
            if o['mode'] & 0xffff:
                d['path'] = 'generic_dil'
            elif dil > 1 and not (k == 1 and o['kw'] == 1):
                d['path'] = 'tap' if tap_ok else 'generic_dil'
            elif s != 1:
                d['path'] = 'mfma' if (s == 2 and taps_ok and in_al and cin >= 8) else 'tap' if tap_ok else 'generic'
            elif cin <= 4 and cout % 4 == 0 and out_al:
                d['path'] = 'first' if (cin == 1 and o['kh'] == 3 and o['kw'] == 3) else 'small_cin'
            elif k == 1 and o['kw'] == 1 and cout <= 8 and in_al:
                d['path'] = 'head'
            elif taps_ok and in_al and cin >= 8 and (cout >= 16 or (k >= 2 and cin >= 16)):
                d['path'] = 'mfma'
                if k == 3 and o['pad_top'] == 1 and o['pad_left'] == 1 and (to['h'], to['w']) == (ti['h'], ti['w']) and cout >= 16 and cout % 4 == 0 and out_al:
                    d['wino'] = True
                    d['wino16'] = cin in (16, 32) and cout in (16, 32) and to['h'] >= 16 and to['w'] >= 32
                    d['wino4'] = cin >= 8 and cout % 32 == 0 and (cout != 32 or cin >= 64) and to['h'] % 16 == 0 and to['w'] % 16 == 0
            elif tap_ok and not taps_ok:
                d['path'] = 'tap'
            else:
                d['path'] = 'generic'
        else:
            square = o['kh'] == o['kw']
            if square and k == s and in_al and cin >= 8 and cout >= 16 and o['pad_top'] == 0 and o['pad_left'] == 0:
                d['path'] = 'convt_gemm'
                bn = 16 if (cout <= 16 and k == 2) else _ntile(cout)
                coutp = -(-cout // bn) * bn
                d['split1'] = k == 2 and coutp % 32 == 0 and cin >= 16
            elif square and k in (3, 4) and s == 2 and in_al and cin >= 8:
                d['path'] = 'convt_phase' if (cout >= 32 and o['pad_top'] <= 1 and o['pad_left'] <= 1) else 'convt_subpixel'
            else:
                d['path'] = 'convt_generic'
        out.append(d)
    return out


def profile_kinds(plan, opts):
    """-> [(op index, kernel kind)] of the launches that the profile records (the matrix-core paths), fusion bits left out: 0 direct,
    1 F(2x2), 2 F(4x4), 3 filter-resident F(2x2), 4 wino16, 5 F(4x4) bf16x3, 6 one-tap bf16x3 GEMM."""
    W = opts['winograd']
    out = []
    for d in conv_paths(plan):
        if d['path'] in ('tap', 'convt_phase', 'convt_subpixel'):
            out.append((d['op'], 0))
        elif d['path'] == 'convt_gemm':
            out.append((d['op'], 6 if (W >= 3 and d['split1']) else 0))
        elif d['path'] == 'mfma':
            if W >= 2 and d['wino4']:
                kind = 5 if (W >= 3 and d['cout'] % 64 == 0) else 2
            elif W and d['wino'] and d['h'] >= 4 and d['w'] >= 8:
                if opts['wino16'] and d['wino16']:
                    kind = 4
                elif opts['wino_resident'] and d['cout'] <= 32 and d['cin'] <= 32:
                    kind = 3
                else:
                    kind = 1
            else:
                kind = 0
            out.append((d['op'], kind))
    return out


def plan_labels(plan, opts):
    """-> the set of PATHS labels that a plan run under ``opts`` exhibits."""
    paths = conv_paths(plan)
    kinds = dict(profile_kinds(plan, opts))
    labels = set()
    for i, d in enumerate(paths):
        k = kinds.get(d['op'])
        labels.add({1: 'wino', 3: 'wino_res', 4: 'wino16', 6: 'convt_split'}.get(k, d['path']))
        if d['in_view'] and d['out_view']:
            labels.add('grouped')
        o = plan.ops[d['op']]
        ti = plan.tensors[o['in0']]
        if o['op'] == keras_plan.OP_CONV and (ti['h'], ti['w'], o['kh']) == (1, 1, 1) and plan.output_rank == 2:
            labels.add('dense')
        nxt = plan.ops[d['op'] + 1] if d['op'] + 1 < len(plan.ops) else None
        if nxt is not None and nxt['in0'] == o['out']:
            if k in (1, 3, 4) and nxt['op'] == keras_plan.OP_MAXPOOL and (nxt['kh'], nxt['kw'], nxt['stride'], nxt['mode']) == (2, 2, 2, 0):
                labels.add('pool_fused')
            if k == 4 and i + 1 < len(paths) and paths[i + 1]['op'] == d['op'] + 1 and paths[i + 1]['path'] == 'head' and paths[i + 1]['cout'] <= 4:
                labels.add('head_fused')
            if d['path'] == 'first' and opts['fuse_first'] and kinds.get(d['op'] + 1) == 4 and d['cout'] in (16, 32) and d['w'] % 4 == 0:
                labels.add('first_fused')
    # convolutions that write the model output's own buffer as views at offsets 4 and 6, reading a compact tensor (a grouped
    # convolution's members read slices): the members of a Concatenate that is the output
    out_buf = plan.tensors[plan.output_tensor]['buffer']
    members = [d for d in paths if d['out_view'] and not d['in_view'] and plan.tensors[plan.ops[d['op']]['out']]['buffer'] == out_buf]
    if {4, 6} <= {d['out_offset'] for d in members} and plan.tensors[plan.output_tensor]['c_stride'] == plan.tensors[plan.output_tensor]['c']:
        labels.add('concat_view')
    return labels


# ---- Part A: the lattice -------------------------------------------------------------------------------------------------
def single(name, group, path, H, W, cin, cout, k, s=1, padding='same', act='linear', bias=True, N=1, u8=True, dil=1, groups=1, cls='Conv2D',
           opts=None, kind=None, wmax=3, step=1, xmax=255, bmax=50):
    """InputLayer + one layer with integer data."""
    rng = _rng(name)
    k2 = (k, k) if isinstance(k, int) else tuple(k)
    if cls == 'Conv2D':
        shapes = [k2 + (cin // groups, cout)]
        nb = cout
    elif cls == 'Conv2DTranspose':
        shapes = [k2 + (cout, cin)]
        nb = cout
    elif cls == 'DepthwiseConv2D':
        shapes = [k2 + (cin, cout)]
        nb = cin * cout
    else:
        shapes = [k2 + (cin, cout[0]), (1, 1, cin * cout[0], cout[1])]
        nb = cout[1]
    ws = [int_weights(rng, shp, wmax, step) for shp in shapes]
    if bias:
        ws.append(int_weights(rng, (nb,), bmax))
    x = int_input(rng, (N, H, W, cin), u8, xmax)
    layers = [_in(H, W, cin), conv_layer('op', 'in', cout, k, s, padding, act, bias, dil, groups, cls)]
    return _case(name, group, 'lattice', layers, {'op': ws}, x, path, opts, kind)


def _flags(q):
    """act, bias, batch and input type from a counter: every combination comes up."""
    return dict(act=('linear', 'relu')[q % 2], bias=bool((q // 2) % 2 == 0), N=(1, 3)[(q // 3) % 2], u8=bool((q // 5) % 2 == 0))


EXT_H = (1, 7, 8, 9, 17)            # the direct kernel's tile is 8 x 16 pixels (4 x 32 from 32 columns on)
EXT_W = (1, 15, 16, 17, 33)


def mfma_cases():
    """conv_mfma_kernel under winograd = 0: k = 1, 2, 3, 5 x stride 1, 2, 3 x 'same' / 'valid' (5 x 5 and stride 3 on its tap-by-tap
    form), then Cout = 1 .. 8 (a mostly empty 32-column tile), then the wide 4 x 32 tile."""
    out, q = [], 0
    for k in (1, 2, 3, 5):
        for s in (1, 2, 3):
            for padding in ('same', 'valid'):
                H, W = EXT_H[q % 5], EXT_W[(q // 2 + 1) % 5]
                if padding == 'valid':
                    H, W = max(H, k), max(W, k)
                cin, cout = (8, 12, 16, 20, 32, 40)[q % 6], (16, 20, 32, 48, 64)[q % 5]
                path = 'mfma' if (k <= 3 and s <= 2) else 'tap'
                out.append(single('mfma_k%d_s%d_%s_%dx%d_%dto%d' % (k, s, padding, H, W, cin, cout), 'mfma', path, H, W, cin, cout, k, s, padding,
                                  kind=0, **_flags(q)))
                q += 1
    for cout in (1, 2, 3, 4, 5, 7, 8):
        H, W = EXT_H[1 + q % 4], EXT_W[1 + (q + 2) % 4]
        out.append(single('mfma_few_%dx%d_16to%d' % (H, W, cout), 'mfma', 'mfma', H, W, 16, cout, 3, kind=0, **_flags(q)))
        q += 1
    for (H, W) in ((3, 31), (4, 32), (5, 33), (9, 65)):
        out.append(single('mfma_wide_%dx%d' % (H, W), 'mfma', 'mfma', H, W, (8, 20)[q % 2], (16, 48)[q % 2], (3, 2)[q % 2], kind=0, **_flags(q)))
        q += 1
    out.append(single('mfma_s2_same_odd_9x17', 'mfma', 'mfma', 9, 17, 16, 16, 3, 2, kind=0, N=3))      # asymmetric 'same' padding on both axes
    out.append(single('mfma_s2_same_odd_k2_7x33', 'mfma', 'mfma', 7, 33, 8, 32, 2, 2, kind=0, u8=False))
    return out


WINO_OPTS = {'wino': dict(winograd=1, wino_resident=0, wino16=0), 'wino_res': dict(winograd=1, wino_resident=1, wino16=0),
             'wino16': dict(winograd=1, wino_resident=1, wino16=1)}
WINO_KIND = {'wino': 1, 'wino_res': 3, 'wino16': 4}


def wino_case(path, H, W, cin, cout, q, tag='', **more):
    name = '%s_%dx%d_%dto%d%s' % (path, H, W, cin, cout, tag)
    return single(name, 'wino', path, H, W, cin, cout, 3, opts=WINO_OPTS[path], kind=WINO_KIND[path], wmax=8, step=4, **dict(_flags(q), **more))


def wino_cases():
    """The three F(2x2) kernels under winograd = 1.  conv_wino_kernel: 8 x 16 pixel tiles (16 rows at 64 output channels);
    conv_wino_res_kernel: the same tiles, a workgroup walks ``tpw`` of a tile row (more than one only in a launch of >= 2048
    workgroups: the 128 x 1377 case walks 2, its last segment holds one partial tile); conv_wino16_kernel: 16 x 32 blocks, a workgroup
    walks up to 8 (16 x 289: 8 + 2 blocks, the last partial)."""
    out, q = [], 0
    for (H, W) in ((4, 8), (7, 15), (8, 16), (9, 17), (17, 33), (15, 31)):
        cin, cout = (8, 12, 16, 20, 32, 40)[q % 6], (16, 20, 32, 48, 64, 64)[q % 6]
        out.append(wino_case('wino', H, W, cin, cout, q))
        q += 1
    for (H, W) in ((4, 8), (7, 15), (8, 16), (9, 17), (17, 33)):
        cin, cout = (8, 12, 16, 20, 32)[q % 5], (16, 20, 32, 28, 16)[q % 5]
        out.append(wino_case('wino_res', H, W, cin, cout, q))
        q += 1
    out.append(wino_case('wino_res', 128, 1377, 8, 16, 0, '_walk', N=3))
    for (H, W), (cin, cout) in (((16, 32), (16, 16)), ((17, 33), (16, 32)), ((15 + 16, 31 + 32), (32, 16)), ((33, 65), (32, 32)),
                                ((16, 289), (16, 16))):
        out.append(wino_case('wino16', H, W, cin, cout, q))
        q += 1
    return out


def direct_cases():
    """conv_first_kernel (Cin = 1, 3 x 3: a thread owns 8 rows), conv_small_cin_kernel (Cin <= 4 and Cout % 4 == 0; Cin = 5 is past its
    rule and takes conv_generic_kernel, as every Cout that is no multiple of 4 does), conv_head_kernel (1 x 1, Cout <= 8; 4 / 8 / 16 lanes
    per pixel from Cin = 16 / 32 / 64) and conv_generic_kernel (dilated, per-axis strides and rates)."""
    out, q = [], 0
    for (H, W), cout in (((1, 1), 4), ((7, 15), 16), ((8, 16), 8), ((9, 17), 32), ((17, 5), 64)):
        out.append(single('first_%dx%d_1to%d' % (H, W, cout), 'direct', 'first', H, W, 1, cout, 3, **_flags(q)))
        q += 1
    out.append(single('first_valid_9x17_1to4', 'direct', 'first', 9, 17, 1, 4, 3, padding='valid', N=3))
    for cin, cout, k, padding, (H, W) in ((3, 4, 3, 'same', (7, 15)), (3, 8, 2, 'valid', (8, 16)), (4, 20, 1, 'same', (1, 17)), (3, 48, 5, 'same', (9, 5)),
                                          (1, 4, 5, 'same', (3, 3)), (3, 4, (1, 3), 'valid', (2, 9))):
        out.append(single('smallcin_k%s_%s_%dx%d_%dto%d' % (k, padding, H, W, cin, cout), 'direct', 'small_cin', H, W, cin, cout, k, padding=padding, **_flags(q)))
        q += 1
    for cin, cout, k, (H, W) in ((5, 4, 3, (7, 15)), (5, 3, 3, (9, 17)), (3, 5, 3, (8, 16)), (1, 1, 3, (17, 33)), (5, 7, 2, (1, 1)), (3, 2, 3, (3, 2))):
        out.append(single('generic_k%d_%dx%d_%dto%d' % (k, H, W, cin, cout), 'direct', 'generic', H, W, cin, cout, k, **_flags(q)))
        q += 1
    out.append(single('generic_s3_7x15_5to3', 'direct', 'generic', 7, 15, 5, 3, 3, 3, **_flags(q)))
    for cin, cout, (H, W) in ((8, 1, (1, 1)), (12, 2, (7, 15)), (16, 3, (8, 16)), (20, 4, (9, 17)), (32, 5, (17, 33)), (40, 7, (3, 5)), (64, 8, (5, 13))):
        out.append(single('head_%dx%d_%dto%d' % (H, W, cin, cout), 'direct', 'head', H, W, cin, cout, 1, **_flags(q)))
        q += 1
    for name, cin, cout, k, s, dil, padding, (H, W) in (('dil2', 5, 3, 3, 1, 2, 'same', (7, 15)), ('dil2_valid', 3, 4, 3, 1, 2, 'valid', (9, 17)),
                                                        ('dil2_tap', 8, 16, 3, 1, 2, 'same', (9, 17)), ('stride_2x1', 8, 16, 3, (2, 1), 1, 'same', (9, 17)),
                                                        ('stride_1x3', 3, 5, 2, (1, 3), 1, 'valid', (8, 16)), ('dil_1x2', 16, 4, 3, 1, (1, 2), 'same', (7, 15)),
                                                        ('dil_3x1', 5, 8, (2, 3), 1, (3, 1), 'same', (9, 7))):
        path = 'tap' if name == 'dil2_tap' else 'generic_dil'
        out.append(single('generic_%s_%dx%d_%dto%d' % (name, H, W, cin, cout), 'direct', path, H, W, cin, cout, k, s, padding, dil=dil,
                          kind=0 if path == 'tap' else None, **_flags(q)))
        q += 1
    return out


def grouped_cases():
    """Grouped Conv2D (a convolution per group on a channel slice of the input, written into its slice of the output), the three depthwise
    forms and SeparableConv2D."""
    out, q = [], 0
    for cin, cout, groups, k, s, (H, W) in ((16, 32, 2, 3, 1, (9, 17)), (12, 6, 3, 3, 1, (7, 15)), (24, 48, 3, 1, 1, (8, 16)), (32, 32, 2, 3, 2, (9, 17)),
                                            (8, 8, 2, 2, 1, (5, 5))):
        out.append(single('grouped_g%d_k%d_s%d_%dx%d_%dto%d' % (groups, k, s, H, W, cin, cout), 'grouped', 'grouped', H, W, cin, cout, k, s, groups=groups,
                          **_flags(q)))
        q += 1
    for cin, mult, k, s, dil, padding, (H, W) in ((5, 1, 3, 1, 1, 'same', (7, 15)), (8, 2, 3, 2, 1, 'same', (9, 17)), (3, 2, 5, 1, 1, 'valid', (8, 16)),
                                                  (4, 1, 3, 1, 2, 'same', (17, 33)), (16, 1, 2, 3, 1, 'valid', (8, 9)), (1, 1, 3, 1, 1, 'same', (1, 1))):
        nm = 'dw_m%d_k%d_s%d_d%d_%s_%dx%d_c%d' % (mult, k, s, dil, padding, H, W, cin)
        out.append(single(nm, 'grouped', 'dw', H, W, cin, mult, k, s, padding, dil=dil, cls='DepthwiseConv2D', **_flags(q)))
        q += 1
    for cin, mult, (H, W) in ((5, 1, (7, 15)), (8, 2, (9, 17)), (4, 3, (1, 5))):
        out.append(single('dw_groups_m%d_%dx%d_c%d' % (mult, H, W, cin), 'grouped', 'dw', H, W, cin, cin * mult, 3, groups=cin, **_flags(q)))
        q += 1
    for cin, mult, cout, k, s, (H, W) in ((5, 1, 3, 3, 1, (7, 15)), (8, 2, 16, 3, 2, (9, 17)), (16, 1, 4, 5, 1, (8, 16))):
        out.append(single('separable_m%d_k%d_s%d_%dx%d_%dto%d' % (mult, k, s, H, W, cin, cout), 'grouped', 'dw', H, W, cin, (mult, cout), k, s,
                          cls='SeparableConv2D', **_flags(q)))
        q += 1
    return out


def transpose_cases():
    """Conv2DTranspose: k = 2 / stride 2 as a GEMM with a scatter epilogue (and as the bf16x3 GEMM under winograd = 3, where integers
    of at most 8 bits are their own first bf16 piece); k = 3, 4 / stride 2 phase by phase (Cout >= 32) or as one 2 x 2-tap sub-pixel
    convolution (fewer); everything else on convt_generic_kernel."""
    out, q = [], 0
    for cin, cout, (H, W) in ((8, 16, (1, 1)), (12, 20, (7, 15)), (16, 32, (8, 16)), (20, 48, (9, 17)), (32, 64, (4, 33)), (40, 16, (5, 31))):
        out.append(single('convt_k2_%dx%d_%dto%d' % (H, W, cin, cout), 'transpose', 'convt_gemm', H, W, cin, cout, 2, 2, cls='Conv2DTranspose', kind=0, **_flags(q)))
        q += 1
    for cin, cout, (H, W) in ((16, 32, (8, 16)), (20, 48, (9, 17)), (32, 64, (4, 33)), (16, 32, (7, 15))):
        # weights and inputs of at most 8 bits: |w| <= 127, x uint8 or |x| <= 255
        out.append(single('convt_split_%dx%d_%dto%d' % (H, W, cin, cout), 'transpose', 'convt_split', H, W, cin, cout, 2, 2, cls='Conv2DTranspose',
                          opts=dict(winograd=3), kind=6, wmax=127, **_flags(q)))
        q += 1
    for k in (3, 4):
        for padding in ('same', 'valid'):
            for cin, cout, (H, W) in ((8, 32, (7, 15)), (16, 48, (9, 17)), (12, 16, (8, 16)), (20, 3, (1, 1))):
                path = 'convt_phase' if cout >= 32 else 'convt_subpixel'
                out.append(single('convt_k%d_%s_%dx%d_%dto%d' % (k, padding, H, W, cin, cout), 'transpose', path, H, W, cin, cout, k, 2, padding,
                                  cls='Conv2DTranspose', kind=0, **_flags(q)))
                q += 1
    for cin, cout, k, s, padding, (H, W) in ((3, 5, 3, 2, 'same', (7, 15)), (8, 16, 3, 3, 'valid', (5, 9)), (8, 16, 5, 2, 'same', (8, 16)), (5, 4, 2, 2, 'valid', (9, 3)),
                                             (8, 16, 4, 4, 'same', (3, 5)), (8, 4, 3, 1, 'same', (7, 9))):
        path = 'convt_gemm' if (k == s and cin >= 8) else 'convt_generic'
        out.append(single('convt_generic_k%d_s%d_%s_%dx%d_%dto%d' % (k, s, padding, H, W, cin, cout), 'transpose', path, H, W, cin, cout, k, s, padding,
                          cls='Conv2DTranspose', kind=0 if path == 'convt_gemm' else None, **_flags(q)))
        q += 1
    return out


def fusion_case(what, H, W, c, q, tag=''):
    """A second layer that the first one's launch takes over: 'pool' - 3 x 3 convolution + MaxPooling2D(2 x 2) (0x100); 'head' - 3 x 3
    convolution on conv_wino16_kernel + 1 x 1 convolution to 3 classes (0x200); 'first' - Conv2D(1 -> c) computed into the halo of the
    c -> c convolution behind it (0x400).  Inputs of at most 6 (4 for 'first') bits keep the second layer's sums below 2^24."""
    name = 'fused_%s_%dx%d_c%d%s' % (what, H, W, c, tag)
    rng = _rng(name)
    f = _flags(q)
    opts = dict(WINO_OPTS['wino16'])
    if what == 'first':
        x = int_input(rng, (f['N'], H, W, 1), True, 15)
        layers = [_in(H, W, 1), conv_layer('c1', 'in', c, 3, act='relu'), conv_layer('op', 'c1', c, 3, act=f['act'], bias=f['bias'])]
        weights = {'c1': [int_weights(rng, (3, 3, 1, c), 1), int_weights(rng, (c,), 3)],
                   'op': [int_weights(rng, (3, 3, c, c), 8, 4)] + ([int_weights(rng, (c,), 50)] if f['bias'] else [])}
        return _case(name, 'fusion', 'lattice', layers, weights, x, 'first_fused', opts, 4, 0x400)
    cin = c if what == 'head' else (8, 16, 32)[q % 3]
    x = int_input(rng, (f['N'], H, W, cin), f['u8'], 63)
    layers = [_in(H, W, cin), conv_layer('c1', 'in', c, 3, act='relu')]
    weights = {'c1': [int_weights(rng, (3, 3, cin, c), 8, 4), int_weights(rng, (c,), 50)]}
    if what == 'pool':
        layers.append(_L('MaxPooling2D', 'op', ['c1'], pool_size=[2, 2], strides=[2, 2], padding='valid'))
        if tag == '_res':
            opts = dict(WINO_OPTS['wino_res'])
        kind = 4 if (opts['wino16'] and cin in (16, 32) and c in (16, 32) and H >= 16 and W >= 32) else 3
        return _case(name, 'fusion', 'lattice', layers, weights, x, 'pool_fused', opts, kind, 0x100)
    layers.append(conv_layer('op', 'c1', 3, 1, act=f['act'], bias=f['bias']))
    weights['op'] = [int_weights(rng, (1, 1, c, 3), 3)] + ([int_weights(rng, (3,), 50)] if f['bias'] else [])
    return _case(name, 'fusion', 'lattice', layers, weights, x, 'head_fused', opts, 4, 0x200)


def dense_case(H, W, c, units, q, tag=''):
    name = 'dense_%dx%dx%d_to%d%s' % (H, W, c, units, tag)
    rng = _rng(name)
    f = _flags(q)
    feats = H * W * c
    layers = [_in(H, W, c), _L('Flatten', 'flat', ['in']), _L('Dense', 'op', ['flat'], units=units, activation=f['act'], use_bias=f['bias'])]
    weights = {'op': [int_weights(rng, (feats, units), 3)] + ([int_weights(rng, (units,), 50)] if f['bias'] else [])}
    return _case(name, 'fusion', 'lattice', layers, weights, int_input(rng, (f['N'], H, W, c), f['u8']), 'dense')


def concat_case(cin, k, H, W, q, tag=''):
    """Three convolutions with 4, 2 and 3 (Cin >= 16: 16) output channels whose outputs are the members of a Concatenate: they write
    straight into the concatenated buffer, at channel offsets 0, 4 and 6."""
    name = 'concat_k%d_%dx%d_c%d%s' % (k, H, W, cin, tag)
    rng = _rng(name)
    f = _flags(q)
    couts = (4, 2, 16 if cin >= 16 else 3)
    layers, weights = [_in(H, W, cin)], {}
    for nm, co in zip('abc', couts):
        layers.append(conv_layer(nm, 'in', co, k, act=f['act'], bias=f['bias']))
        weights[nm] = [int_weights(rng, (k, k, cin, co), 3)] + ([int_weights(rng, (co,), 50)] if f['bias'] else [])
    layers.append(_L('Concatenate', 'op', ['a', 'b', 'c'], axis=-1))
    return _case(name, 'fusion', 'lattice', layers, weights, int_input(rng, (f['N'], H, W, cin), f['u8']), 'concat_view')


def fusion_cases():
    out = [fusion_case('pool', 16, 32, 16, 0), fusion_case('pool', 18, 34, 32, 1), fusion_case('pool', 8, 16, 20, 2, '_res'), fusion_case('pool', 10, 18, 16, 4, '_res'),
           fusion_case('head', 16, 32, 16, 0), fusion_case('head', 17, 33, 32, 3), fusion_case('head', 33, 65, 16, 5),
           fusion_case('first', 16, 32, 16, 0), fusion_case('first', 17, 36, 32, 1), fusion_case('first', 33, 68, 16, 3),
           dense_case(3, 4, 4, 16, 0), dense_case(1, 1, 8, 32, 1), dense_case(2, 3, 5, 10, 2), dense_case(4, 4, 4, 5, 3),
           concat_case(3, 3, 7, 15, 0), concat_case(16, 3, 9, 17, 1), concat_case(5, 1, 8, 16, 2), concat_case(20, 2, 17, 33, 3)]
    return out


LATTICE_GROUPS = ('mfma', 'wino', 'direct', 'grouped', 'transpose', 'fusion')


def lattice_cases(group):
    if group == 'random':
        return [random_case(s) for s in RANDOM_SEEDS]
    return {'mfma': mfma_cases, 'wino': wino_cases, 'direct': direct_cases, 'grouped': grouped_cases, 'transpose': transpose_cases,
            'fusion': fusion_cases}[group]()


RANDOM_FAMILIES = ('mfma', 'mfma_s2', 'tap', 'wino', 'wino_res', 'wino16', 'first', 'small_cin', 'generic', 'head', 'generic_dil', 'grouped', 'dw',
                   'separable', 'convt_gemm', 'convt_split', 'convt_phase', 'convt_subpixel', 'convt_generic', 'pool', 'head_fused', 'first_fused', 'dense', 'concat')


def random_case(seed):
    """Seed -> a family (in turn, so that the committed range holds every family) with extents, channel counts, batch, activation, bias and
    input type drawn from the lists above."""
    rng = np.random.default_rng(1000 + seed)
    pick = lambda seq: seq[int(rng.integers(0, len(seq)))]
    fam = RANDOM_FAMILIES[seed % len(RANDOM_FAMILIES)]
    q = int(rng.integers(0, 20))
    f = _flags(q)
    H, W = pick((7, 8, 9, 17)), pick((15, 16, 17, 33))
    tag = 'random%02d_%s' % (seed, fam)
    big_in, big_out = pick((8, 12, 16, 20, 32, 40)), pick((16, 20, 32, 48, 64))
    if fam == 'mfma':
        c = single(tag, 'random', 'mfma', H, W, big_in, big_out, pick((1, 2, 3)), padding=pick(('same', 'valid')), kind=0, **f)
    elif fam == 'mfma_s2':
        c = single(tag, 'random', 'mfma', H, W, big_in, pick(COUT_LIST), pick((1, 2, 3)), 2, pick(('same', 'valid')), kind=0, **f)
    elif fam == 'tap':
        k, s = pick(((5, 1), (5, 2), (3, 3), (2, 3)))
        c = single(tag, 'random', 'tap', H, W, big_in, pick((8, 16, 20, 32)), k, s, pick(('same', 'valid')), kind=0, **f)
    elif fam in ('wino', 'wino_res'):
        c = single(tag, 'random', fam, H, W, pick((8, 12, 16, 20, 32)), pick((16, 20, 32)) if fam == 'wino_res' else big_out, 3, opts=WINO_OPTS[fam],
                   kind=WINO_KIND[fam], wmax=8, step=4, **f)
    elif fam == 'wino16':
        c = single(tag, 'random', fam, pick((16, 17, 33)), pick((32, 33, 65)), pick((16, 32)), pick((16, 32)), 3, opts=WINO_OPTS[fam], kind=4, wmax=8, step=4, **f)
    elif fam == 'first':
        c = single(tag, 'random', 'first', H, W, 1, pick((4, 8, 16, 20, 32)), 3, padding=pick(('same', 'valid')), **f)
    elif fam == 'small_cin':
        c = single(tag, 'random', 'small_cin', H, W, pick((3, 4)), pick((4, 8, 16, 20)), pick((1, 2, 3, 5)), padding=pick(('same', 'valid')), **f)
    elif fam == 'generic':
        c = single(tag, 'random', 'generic', H, W, pick((1, 3, 5)), pick((1, 2, 3, 5, 7)), pick((2, 3, 5)), pick((1, 2, 3)), pick(('same', 'valid')), **f)
    elif fam == 'head':
        c = single(tag, 'random', 'head', H, W, big_in, pick((1, 2, 3, 4, 5, 7, 8)), 1, **f)
    elif fam == 'generic_dil':
        s, dil = pick(((1, 2), (1, 3), ((2, 1), 1), ((1, 2), 1), (1, (2, 1)), (1, (1, 3))))
        c = single(tag, 'random', 'generic_dil', H, W, pick((3, 5, 8)), pick((3, 4, 5)), 3, s, pick(('same', 'valid')), dil=dil, **f)
    elif fam == 'grouped':
        g = pick((2, 4))
        c = single(tag, 'random', 'grouped', H, W, g * pick((3, 4, 8)), g * pick((2, 4, 16)), pick((1, 2, 3)), pick((1, 2)), groups=g, **f)
    elif fam == 'dw':
        c = single(tag, 'random', 'dw', H, W, pick(CIN_LIST), pick((1, 2)), pick((2, 3, 5)), pick((1, 2)), pick(('same', 'valid')), cls='DepthwiseConv2D', **f)
    elif fam == 'separable':
        c = single(tag, 'random', 'dw', H, W, pick(CIN_LIST), (pick((1, 2)), pick(COUT_LIST)), 3, pick((1, 2)), pick(('same', 'valid')), cls='SeparableConv2D', **f)
    elif fam == 'convt_gemm':
        c = single(tag, 'random', 'convt_gemm', H, W, big_in, big_out, 2, 2, pick(('same', 'valid')), cls='Conv2DTranspose', kind=0, **f)
    elif fam == 'convt_split':
        c = single(tag, 'random', 'convt_split', H, W, pick((16, 20, 32, 40)), pick((32, 48, 64)), 2, 2, cls='Conv2DTranspose', opts=dict(winograd=3), kind=6,
                   wmax=127, **f)
    elif fam in ('convt_phase', 'convt_subpixel'):
        c = single(tag, 'random', fam, H, W, big_in, pick((32, 48, 64) if fam == 'convt_phase' else (1, 3, 16, 20)), pick((3, 4)), 2, pick(('same', 'valid')),
                   cls='Conv2DTranspose', kind=0, **f)
    elif fam == 'convt_generic':
        k = pick((2, 3, 4))
        c = single(tag, 'random', 'convt_generic', H, W, pick((1, 3, 5)), pick((1, 3, 4, 16)), k, pick((1, 2, 3)[:k]), pick(('same', 'valid')),
                   cls='Conv2DTranspose', **f)       # (stride <= kernel: the float64 oracle has no gaps between the taps to fill)
    elif fam == 'pool':
        c = fusion_case('pool', pick((16, 18, 34)), pick((32, 34, 66)), pick((16, 32)), q, '_' + tag)
    elif fam == 'head_fused':
        c = fusion_case('head', pick((16, 17, 33)), pick((32, 33, 65)), pick((16, 32)), q, '_' + tag)
    elif fam == 'first_fused':
        c = fusion_case('first', pick((16, 17, 33)), pick((32, 36, 68)), pick((16, 32)), q, '_' + tag)
    elif fam == 'dense':
        c = dense_case(pick((1, 2, 3)), pick((1, 3, 4)), pick((4, 5, 8)), pick((5, 10, 16, 32)), q, '_' + tag)
    else:
        c = concat_case(pick((3, 5, 16, 20)), pick((1, 2, 3)), H, W, q, '_' + tag)
    return dict(c, name=tag, group='random')


def all_lattice_cases():
    return [c for g in LATTICE_GROUPS + ('random',) for c in lattice_cases(g)]


# ---- Part B: impulses ----------------------------------------------------------------------------------------------------
def wide_floats(rng, shape):
    """Finite float32 with all 24 significand bits in use (an odd significand), magnitudes 1e-20 .. 1e20, both signs."""
    mant = (rng.integers(2 ** 23, 2 ** 24, size=shape) | 1).astype(np.float64)
    v = mant * 2.0 ** (rng.integers(-66, 66, size=shape) - 23.0) * rng.choice([-1.0, 1.0], size=shape)
    out = v.astype(np.float32)
    assert np.array_equal(out.astype(np.float64), v)
    return out


# family -> (layer class, kernel, stride, dilation, padding, Cin, Cout or multiplier, (H, W), options, path, profile kind).  The extents put
# at least one seam of the family's tile (IMPULSE_TILES) inside the output on both axes: stride-2 layers get 17 x 33 inputs (9 x 17 outputs).
IMPULSE_FAMILIES = {
    'mfma': ('Conv2D', 3, 1, 1, 'same', 16, 16, (9, 17), None, 'mfma', 0),
    'mfma_s2': ('Conv2D', 3, 2, 1, 'same', 12, 20, (17, 33), None, 'mfma', 0),
    'mfma_k2_valid': ('Conv2D', 2, 1, 1, 'valid', 8, 48, (9, 34), None, 'mfma', 0),
    'tap_k5': ('Conv2D', 5, 1, 1, 'same', 8, 8, (9, 17), None, 'tap', 0),
    'first': ('Conv2D', 3, 1, 1, 'same', 1, 8, (9, 17), None, 'first', None),
    'small_cin': ('Conv2D', 3, 1, 1, 'same', 3, 8, (9, 17), None, 'small_cin', None),
    'head': ('Conv2D', 1, 1, 1, 'same', 16, 3, (9, 17), None, 'head', None),
    'generic': ('Conv2D', 3, 1, 1, 'same', 5, 3, (9, 17), None, 'generic', None),
    'generic_dil': ('Conv2D', 3, 1, 2, 'same', 5, 3, (9, 17), None, 'generic_dil', None),
    'dw': ('DepthwiseConv2D', 3, 1, 1, 'same', 8, 2, (9, 17), None, 'dw', None),
    'dw_vec': ('DepthwiseConv2D', 3, 1, 1, 'same', 8, 1, (9, 17), None, 'dw', None),
    'dw_s2': ('DepthwiseConv2D', 3, 2, 1, 'same', 8, 1, (17, 33), None, 'dw', None),
    'convt_gemm': ('Conv2DTranspose', 2, 2, 1, 'same', 8, 16, (9, 17), None, 'convt_gemm', 0),
    'convt_phase_k3': ('Conv2DTranspose', 3, 2, 1, 'same', 8, 32, (9, 17), None, 'convt_phase', 0),
    'convt_phase_k4': ('Conv2DTranspose', 4, 2, 1, 'valid', 12, 32, (9, 17), None, 'convt_phase', 0),
    'convt_subpixel': ('Conv2DTranspose', 3, 2, 1, 'valid', 8, 16, (9, 17), None, 'convt_subpixel', 0),
    'convt_generic': ('Conv2DTranspose', 3, 2, 1, 'same', 3, 5, (9, 17), None, 'convt_generic', None),
    'convt_split': ('Conv2DTranspose', 2, 2, 1, 'same', 20, 32, (9, 17), dict(winograd=3), 'convt_split', 6),
}


# Output pixels per workgroup tile (rows, columns), and whether the tiles walk the layer's INPUT extent (the transposed kernels).  Direct
# MFMA kernel: 8 x 16, 4 x 32 from 32 output columns on; dwconv_kernel (multiplier 1, channels % 4 == 0): 8 x 8; conv_first_kernel: a thread
# owns 8 rows; the per-pixel kernels (small_cin, head, generic, the other depthwise and transposed forms) have no tile: 8 x 16 stands in.
IMPULSE_TILES = {'mfma_k2_valid': (4, 32), 'dw_vec': (8, 8), 'dw_s2': (8, 8)}


def _impulse_layer(fam, bias):
    cls, k, s, dil, padding, cin, cout, (H, W), opts, path, kind = IMPULSE_FAMILIES[fam]
    return [_in(H, W, cin), conv_layer('op', 'in', cout, k, s, padding, 'linear', bias, dil, cls=cls)]


def _kernel_shape(fam):
    cls, k, s, dil, padding, cin, cout, hw, opts, path, kind = IMPULSE_FAMILIES[fam]
    return {'Conv2D': (k, k, cin, cout), 'Conv2DTranspose': (k, k, cout, cin), 'DepthwiseConv2D': (k, k, cin, cout)}[cls]


def impulse_seams(fam):
    """-> (rows, columns) of the INPUT at which an impulse lands on either side of a tile seam of the family's kernel: for a forward
    convolution with stride s the input pixels s t - s .. s t + s - 1 around every seam t of the output tiling (they reach outputs on both
    sides of it); for a transposed one, whose tiles walk the input, the pixels t - 1 and t."""
    cls, k, s, dil, padding, cin, cout, (H, W), opts, path, kind = IMPULSE_FAMILIES[fam]
    th, tw = IMPULSE_TILES.get(fam, (8, 16))
    if cls == 'Conv2DTranspose':
        s, oh, ow = 1, H, W
    elif padding == 'same':
        oh, ow = -(-H // s), -(-W // s)
    else:
        oh, ow = (H - ((k - 1) * dil + 1)) // s + 1, (W - ((k - 1) * dil + 1)) // s + 1
    rows = sorted({y for t in range(th, oh, th) for y in range(s * t - s, s * t + s) if 0 <= y < H})
    cols = sorted({x for t in range(tw, ow, tw) for x in range(s * t - s, s * t + s) if 0 <= x < W})
    return rows, cols


def impulse_positions(fam):
    """Every corner, pixels of every edge, and both sides of every tile seam (``impulse_seams``), in all combinations."""
    H, W = IMPULSE_FAMILIES[fam][7]
    rows, cols = impulse_seams(fam)
    ys = sorted({0, 1, H - 1} | set(rows))
    xs = sorted({0, 1, (W - 1) // 2, W - 1} | set(cols))
    return [(y, x) for y in ys for x in xs]


def delta_input_case(fam):
    """One image per impulse position: image i is 0 except x[pos_i, channel i % Cin] = 1 (every input channel comes up: there are more
    positions than channels); arbitrary weights, no bias."""
    cls, k, s, dil, padding, cin, cout, (H, W), opts, path, kind = IMPULSE_FAMILIES[fam]
    name = 'delta_input_' + fam
    rng = _rng(name)
    pos = impulse_positions(fam)
    assert len(pos) >= cin
    x = np.zeros((len(pos), H, W, cin), np.float32)
    for i, (y, xx) in enumerate(pos):
        x[i, y, xx, i % cin] = 1.0
    weights = {'op': [wide_floats(rng, _kernel_shape(fam))]}
    return _case(name, 'impulse', 'impulse', _impulse_layer(fam, False), weights, x, path, opts, kind)


def channel_groups(n):
    """The 4-channel groups of n channels as (first, last + 1); every 8-channel group holds one."""
    return [(g, min(g + 4, n)) for g in range(0, n, 4)]


def _group_pick(g, n):
    """One channel of the 4-channel group that starts at g: its position in the group moves with the group."""
    return min(g + (g // 4) % 4, n - 1)


def delta_filter_cases(fam):
    """The tap (r, q) of one (cin, cout) pair is 1, every other weight 0; the bias of that output channel is 0, the others arbitrary; the
    data arbitrary.  One case per tap (the pair moving along), then, on the last tap, one case for every 4-channel group of Cin and of Cout
    that the taps have not reached: the union covers every tap and every 4- and 8-channel group of both sides (asserted in
    tests/test_conv_exact.py).  ``tap`` = (r, q, ci, co, output channel)."""
    cls, k, s, dil, padding, cin, cout, (H, W), opts, path, kind = IMPULSE_FAMILIES[fam]
    shape = _kernel_shape(fam)
    rng = _rng('delta_filter_' + fam)
    x = wide_floats(rng, (2, H, W, cin))
    n_out = cin * cout if cls == 'DepthwiseConv2D' else cout
    co_dim = shape[3] if cls != 'Conv2DTranspose' else shape[2]
    ci_list = [_group_pick(g, cin) for g, _ in channel_groups(cin)]
    co_list = [_group_pick(g, co_dim) for g, _ in channel_groups(co_dim)]
    pairs = [(r, q, ci_list[t % len(ci_list)], co_list[(t // 2) % len(co_list)]) for t, (r, q) in enumerate((r, q) for r in range(k) for q in range(k))]
    ci_seen, co_seen = {p[2] for p in pairs}, {p[3] for p in pairs}
    pairs += [(k - 1, k - 1, ci, co_list[-1]) for ci in ci_list if ci not in ci_seen]
    pairs += [(k - 1, k - 1, ci_list[-1], co) for co in co_list if co not in co_seen]
    out = []
    for r, q, ci, co in pairs:
        w = np.zeros(shape, np.float32)
        if cls == 'Conv2DTranspose':
            w[r, q, co, ci] = 1.0
            oc = co
        else:
            w[r, q, ci, co] = 1.0
            oc = ci * cout + co if cls == 'DepthwiseConv2D' else co
        b = wide_floats(rng, (n_out,))
        b[oc] = 0.0
        out.append(_case('delta_filter_%s_tap%d_%d_ci%d_co%d' % (fam, r, q, ci, co), 'impulse', 'impulse', _impulse_layer(fam, True),
                         {'op': [w, b]}, x, path, opts, kind, tap=(r, q, ci, co, oc)))
    return out


def impulse_cases(fam):
    return [delta_input_case(fam)] + delta_filter_cases(fam)


# ---- Part C: identities of the F(4x4) kernels ----------------------------------------------------------------------------
# (name, Cin, Cout, (H, W), N): Cin % 8 == 4, Cout % 64 == 32, an odd number of 16 x 16 regions (a workgroup takes two: pairs then span
# two patches), one and several K groups
IDENTITY_SHAPES = (('w4_12to96', 12, 96, (16, 48), 3), ('w4_12to64', 12, 64, (16, 48), 3), ('w4_20to64', 20, 64, (48, 16), 3), ('w4_20to96', 20, 96, (16, 16), 5),
                   ('w4_68to32', 68, 32, (16, 48), 3), ('w4_16to128', 16, 128, (32, 48), 2))
IDENTITY_OPTS = (dict(winograd=2, wino4_split=1), dict(winograd=2, wino4_split=0), dict(winograd=3, wino4_split=1), dict(winograd=3, wino4_split=0))


def identity_case(name, cin, cout, hw, n, pad_to=None):
    """A 3 x 3 'same' ReLU convolution on ordinary float data; ``pad_to``: the same layer with input channels and filter slices cin ..
    pad_to - 1 added, all zero."""
    rng = _rng('identity_' + name)
    H, W = hw
    x = _f32(rng.normal(size=(n, H, W, cin)))
    w = _f32(rng.normal(size=(3, 3, cin, cout)) / np.sqrt(9 * cin))
    b = _f32(rng.normal(size=cout))
    c = pad_to or cin
    if pad_to:
        x = np.concatenate([x, np.zeros((n, H, W, pad_to - cin), np.float32)], axis=-1)
        w = np.concatenate([w, np.zeros((3, 3, pad_to - cin, cout), np.float32)], axis=2)
    layers = [_in(H, W, c), conv_layer('op', 'in', cout, 3, act='relu')]
    return _case(name + ('_padded%d' % pad_to if pad_to else ''), 'identity', 'identity', layers, {'op': [w, b]}, np.ascontiguousarray(x), 'mfma')


def identity_cases():
    return [identity_case(*s) for s in IDENTITY_SHAPES]


# Cin -> the zero-padded Cin it must equal.  4 against 8 is left out BY DESIGN: ecseg_amd/csrc/model_load.hip gives a Cin <= 4 layer to
# conv_small_cin_kernel ("cin <= 4 && cout % 4 == 0") and builds an F(4x4) filter image only from 8 input channels on ("cin >= 8"),
# so the 4-channel layer never reaches an F(4x4) kernel and is another summation altogether.
IDENTITY_PADS = {12: 16, 20: 24, 68: 72}
