"""Host-side logic that needs no GPU: the C ABI exports what include/ecseg_hip.h declares, the HDF5 reader, the
Keras -> plan lowering, the sharding / record all-gather (gloo, world_size 2)."""
import json
import os
import re
import socket
import sys

import numpy as np
import pytest

from ecseg_amd import dist as edist
from ecseg_amd import hdf5_min, keras_plan, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_library_exports_every_declared_symbol():
    from ecseg_amd._lib import EXPORTS, load_library
    header = open(os.path.join(ROOT, 'include', 'ecseg_hip.h')).read()
    declared = set(re.findall(r'\b(ecseg_[a-z0-9_]+)\s*\(', header))
    assert declared, 'no prototypes found'
    lib = load_library()
    for name in sorted(declared):
        assert hasattr(lib, name), 'libecseg_hip.so does not export %s' % name
    assert declared == set(EXPORTS)
    assert lib.ecseg_abi_version() == 6


def test_missing_gpu_fails_loudly():
    """No silent CPU fallback: without a HIP device the product raises."""
    import torch
    if torch.cuda.is_available():
        pytest.skip('GPU present')
    from ecseg_amd._lib import EcsegError, Handle
    with pytest.raises(EcsegError):
        Handle(0)


def test_product_does_not_import_oracle():
    pkg = os.path.join(ROOT, 'ecseg_amd')
    for dirpath, _, files in os.walk(pkg):
        for f in files:
            if f.endswith(('.py', '.hip', '.h', '.cpp')):
                text = open(os.path.join(dirpath, f)).read()
                assert not re.search(r'^\s*(from|import)\s+oracle\b', text, re.M), f


def test_hdf5_reader_on_keras_fixture(golden_dir):
    cfg, weights = hdf5_min.load_keras_h5(os.path.join(golden_dir, 'keras_tiny.h5'))
    exp = np.load(os.path.join(golden_dir, 'keras_tiny_expected.npz'))
    assert json.loads(cfg) == json.loads(str(exp['model_config']))
    f = hdf5_min.File(os.path.join(golden_dir, 'keras_tiny.h5'))
    assert f.attrs['keras_version'] == '2.8.0' and f.attrs['backend'] == 'tensorflow'
    n = 0
    for lname in hdf5_min._attr_list(f['model_weights'].attrs, 'layer_names'):
        for wn in hdf5_min._attr_list(f['model_weights'][lname].attrs, 'weight_names'):
            key = wn.replace('/', '__').replace(':', '_')
            got = f['model_weights'][lname][wn].read()
            assert got.dtype == np.float32 and np.array_equal(got, exp[key]), wn
            n += 1
    assert n == 18
    assert [a.shape for a in weights['conv2d_transpose']] == [(2, 2, 4, 8), (4,)]
    with pytest.raises(hdf5_min.Hdf5Error):
        hdf5_min.File(__file__)


def _check_plan(plan):
    """Every op reads tensors that are still intact: no op writes a buffer that holds a tensor needed later."""
    last_read = {}
    for k, o in enumerate(plan.ops):
        for t in (o['in0'], o['in1']):
            if t >= 0:
                last_read[t] = k
    last_read[plan.output_tensor] = len(plan.ops)
    written_at = {plan.input_tensor: -1}
    for k, o in enumerate(plan.ops):
        written_at.setdefault(o['out'], k)
    for k, o in enumerate(plan.ops):
        out = plan.tensors[o['out']]
        lo, hi = out['c_offset'], out['c_offset'] + out['c']
        for t, w in written_at.items():
            if t == o['out'] or w >= k or last_read.get(t, -1) < k:
                continue
            tt = plan.tensors[t]
            if tt['buffer'] != out['buffer']:
                continue
            same_layout = tt['c_stride'] == out['c_stride'] and (tt['h'], tt['w']) == (out['h'], out['w'])
            disjoint = same_layout and (tt['c_offset'] + tt['c'] <= lo or hi <= tt['c_offset'])
            assert disjoint, 'op %d overwrites live tensor %d' % (k, t)
    for t in plan.tensors:
        assert t['h'] * t['w'] * t['c_stride'] <= plan.buffer_floats[t['buffer']]


@pytest.mark.parametrize('base,up,bn', [(64, 'transpose', False), (16, 'upsample', True), (16, 'upsample', False), (32, 'transpose', True)])
def test_plan_of_canonical_unet(base, up, bn):
    cfg = synth.unet_config(base=base, up=up, batchnorm=bn)
    w = synth.unet_weights(cfg)
    for fuse in (False, True):
        plan = keras_plan.build_plan(cfg, w, fuse=fuse)
        _check_plan(plan)
        ti, to = plan.tensors[plan.input_tensor], plan.tensors[plan.output_tensor]
        assert (ti['h'], ti['w'], ti['c']) == (256, 256, 1) and (to['h'], to['w'], to['c']) == (256, 256, 4)
        if fuse:
            assert all(o['op'] not in (keras_plan.OP_AFFINE, keras_plan.OP_ACT) for o in plan.ops)
            assert all(o['op'] != keras_plan.OP_COPY for o in plan.ops)     # concatenation is free
            if up == 'upsample':
                # round 6: UpSampling2D(2) + Conv2D(2x2, 'same') = ONE 3x3 / stride-2 transposed convolution with pre-summed taps, cropped by one
                assert all(o['op'] != keras_plan.OP_UPSAMPLE for o in plan.ops)
                ct = [o for o in plan.ops if o['op'] == keras_plan.OP_CONVT]
                assert len(ct) == 4 and all((o['kh'], o['kw'], o['stride'], o['pad_top'], o['pad_left']) == (3, 3, 2, 1, 1) for o in ct)
                k2 = w[[l['config']['name'] for l in cfg['config']['layers'] if l['class_name'] == 'Conv2D' and l['config']['kernel_size'] == [2, 2]][0]][0]
                k3 = plan.weights[ct[0]['w0']].reshape(3, 3, k2.shape[3], k2.shape[2])
                if not bn:                                                   # (a folded BatchNorm scales the taps)
                    assert np.allclose(k3[1, 1], k2.sum((0, 1)).T, atol=1e-6) and np.allclose(k3[0, 0], k2[1, 1].T) and np.allclose(k3[2, 1], (k2[0, 0] + k2[0, 1]).T, atol=1e-6)
        elif up == 'upsample':
            assert sum(1 for o in plan.ops if o['op'] == keras_plan.OP_UPSAMPLE) == 4
        # window lanes (csrc/plan_run.hip run_plan) address the model input and output in plain window order while every other
        # tensor is packed into a lane's private slice of its buffer: the two must have buffers of their own
        for io in (plan.input_tensor, plan.output_tensor):
            b = plan.tensors[io]['buffer']
            assert [k for k, t in enumerate(plan.tensors) if t['buffer'] == b] == [io]
    if base == 64 and up == 'transpose':
        assert abs(plan.flops_per_patch() / 1e9 - 96.2) < 0.1
        assert sum(plan.buffer_floats) * 4 < 90e6                           # liveness re-use: < 90 MB per patch


def test_plan_unrolls_shared_layers_into_calls():
    """Round 6 (VERDICT r05 missing #4): a layer called twice (two inbound nodes) becomes two ops on ONE weight index, in dependency order
    (the second call is listed before the layers that feed it); a reference to a call that does not exist is a clean PlanError."""
    from tests.test_oracle_layers import _shared_model
    rng = np.random.default_rng(3)
    c = 8
    cfg = _shared_model(32, 32, c)
    w = {'sc': [rng.normal(size=(3, 3, c, c)).astype(np.float32), rng.normal(size=c).astype(np.float32)],
         'sbn': [np.ones(c, np.float32), np.zeros(c, np.float32), np.zeros(c, np.float32), np.ones(c, np.float32)]}
    for fuse in (False, True):
        plan = keras_plan.build_plan(cfg, w, fuse=fuse)
        _check_plan(plan)
        convs = [o for o in plan.ops if o['op'] == keras_plan.OP_CONV]
        assert len(convs) == 2
        # shared weights: one copy in the plan (no BatchNorm is folded into either call: both feed the Add as well)
        assert convs[0]['w0'] == convs[1]['w0'] and convs[0]['w1'] == convs[1]['w1']
    bad = json.loads(json.dumps(cfg))
    bad['config']['layers'][4]['inbound_nodes'] = [[['sc', 0, 0, {}], ['sc', 2, 0, {}]]]
    with pytest.raises(keras_plan.PlanError, match='call 2'):
        keras_plan.build_plan(bad, w)


def test_plan_rejects_what_it_cannot_lower():
    cfg = synth.unet_config(base=16, depth=1)
    w = synth.unet_weights(cfg)
    bad = json.loads(json.dumps(cfg))
    bad['config']['layers'][1]['class_name'] = 'ConvLSTM2D'
    with pytest.raises(keras_plan.PlanError):
        keras_plan.build_plan(bad, w)
    bad = json.loads(json.dumps(cfg))
    bad['config']['layers'][1]['config']['strides'] = [2, 1]              # strides > 1 together with a dilation rate > 1 (on any axes)
    bad['config']['layers'][1]['config']['dilation_rate'] = [1, 2]
    with pytest.raises(keras_plan.PlanError, match='Keras rejects'):
        keras_plan.build_plan(bad, w)
    bad = json.loads(json.dumps(cfg))
    bad['config']['layers'][1]['config']['strides'] = [1, 300]            # the horizontal stride travels in 8 bits of `mode`
    with pytest.raises(keras_plan.PlanError, match='out of range'):
        keras_plan.build_plan(bad, w)
    bad = json.loads(json.dumps(cfg))
    bad['config']['layers'][1]['config']['groups'] = 3                    # 3 groups do not divide 1 -> 16 channels
    with pytest.raises(keras_plan.PlanError):
        keras_plan.build_plan(bad, w)
    with pytest.raises(keras_plan.PlanError):
        keras_plan.build_plan(cfg, w, output=1)                           # the model has one output


def test_plan_lowers_anisotropic_convolutions():
    """Round 6: per-axis strides / dilation rates of a plain Conv2D lower to a CONV op whose `mode` carries the
    horizontal values (include/ecseg_hip.h); 'same' padding and the output extent follow each axis' own stride and dilated kernel extent.
    DepthwiseConv2D / grouped convolutions with per-axis values still end in PlanError."""
    def one(cls='Conv2D', **kw):
        layers = [dict(class_name='InputLayer', name='in', inbound_nodes=[], config=dict(name='in', batch_input_shape=[None, 20, 30, 8])),
                  dict(class_name=cls, name='c', inbound_nodes=[[['in', 0, 0, {}]]],
                       config=dict(name='c', kernel_size=[3, 3], padding='same', activation='linear', use_bias=True, **kw))]
        return {'class_name': 'Functional', 'config': {'name': 'm', 'layers': layers, 'input_layers': [['in', 0, 0]], 'output_layers': [['c', 0, 0]]}}
    w = {'c': [np.zeros((3, 3, 8, 16), np.float32), np.zeros(16, np.float32)]}
    plan = keras_plan.build_plan(one(filters=16, strides=[2, 1]), w)
    (op,) = [o for o in plan.ops if o['op'] == keras_plan.OP_CONV]
    assert (op['stride'], op['dilation'], op['mode'], op['pad_top'], op['pad_left']) == (2, 1, 1, 0, 1)      # 20 rows, stride 2: pads (0, 1)
    to = plan.tensors[op['out']]
    assert (to['h'], to['w'], to['c']) == (10, 30, 16)
    plan = keras_plan.build_plan(one(filters=16, strides=[1, 3]), w)
    (op,) = [o for o in plan.ops if o['op'] == keras_plan.OP_CONV]
    assert (op['stride'], op['mode']) == (1, 3) and (plan.tensors[op['out']]['h'], plan.tensors[op['out']]['w']) == (20, 10)
    plan = keras_plan.build_plan(one(filters=16, dilation_rate=[2, 3]), w)
    (op,) = [o for o in plan.ops if o['op'] == keras_plan.OP_CONV]
    assert (op['stride'], op['dilation'], op['mode'], op['pad_top'], op['pad_left']) == (1, 2, 3 << 8, 2, 3)
    plan = keras_plan.build_plan(one(filters=16, strides=[2, 2], dilation_rate=[1, 1]), w)                    # isotropic: mode stays 0
    assert [o['mode'] for o in plan.ops if o['op'] == keras_plan.OP_CONV] == [0]
    with pytest.raises(keras_plan.PlanError, match='anisotropic'):
        keras_plan.build_plan(one('DepthwiseConv2D', strides=[2, 1], depth_multiplier=1), {'c': [np.zeros((3, 3, 8, 1), np.float32), np.zeros(8, np.float32)]})
    with pytest.raises(keras_plan.PlanError, match='anisotropic'):
        keras_plan.build_plan(one(filters=16, strides=[2, 1], groups=2), {'c': [np.zeros((3, 3, 4, 16), np.float32), np.zeros(16, np.float32)]})


def test_loader_corner_graphs_lower_and_their_channels_first_twins_agree():
    """The generator of `tools/fuzz_layers.py --loader` on the CPU: 24 random chains of per-axis convolutions, shared layers, pools and
    BatchNorm lower to plans (anisotropic CONV ops carry their `mode` word, a shared layer becomes one op per call on ONE weight index), and
    the oracle evaluates the channels_first twin natively to the transposed result of the channels_last graph."""
    from oracle import unet
    from tools.fuzz_layers import channels_first_twin, random_graph_r6
    seen = {'aniso': 0, 'shared': 0, 'cf': 0}
    for seed in range(24):
        rng = np.random.default_rng(5 * 10 ** 6 + seed)
        cfg, w, (h, ww, c), cf = random_graph_r6(rng)
        plan = keras_plan.build_plan(cfg, w)
        convs = [o for o in plan.ops if o['op'] == keras_plan.OP_CONV]
        seen['aniso'] += any(o['mode'] for o in convs)
        for L in cfg['config']['layers']:
            if len(L['inbound_nodes']) == 2:                       # a layer called twice: two ops, one kernel
                seen['shared'] += 1
                k = w[L['name']][0]
                twins = [o for o in convs if plan.weights[o['w0']].size == k.size and np.array_equal(np.ravel(plan.weights[o['w0']]), k.ravel())]
                assert len(twins) >= 2 and len({o['w0'] for o in twins}) == 1, (seed, L['name'])
        if cf and seed % 2 == 0:                                   # (the oracle pass is the slow part: every second twin)
            seen['cf'] += 1
            x = rng.integers(0, 256, size=(1, h, ww, c), dtype=np.uint8).astype(np.float32)
            want = unet.forward(cfg, w, x)
            twin = channels_first_twin(cfg)
            assert keras_plan.build_plan(twin, w).channels_first
            got = unet.forward(twin, w, np.ascontiguousarray(np.moveaxis(x, -1, 1)))
            assert np.abs(np.moveaxis(got, 1, -1) - want).max() <= 2e-4 * max(1.0, float(np.abs(want).max())), seed
    assert seen['aniso'] >= 5 and seen['shared'] >= 5 and seen['cf'] >= 2, seen


def test_plan_lowers_round5_vocabulary(golden_dir):
    """dilation_rate, groups, DepthwiseConv2D / SeparableConv2D, Multiply, PReLU, Normalization,
    LayerNormalization, nested sub-models and several outputs lower to a plan (they ended in PlanError before); the h5py-written
    MobileNet-style fixture (nested backbone whose group mixes the variables of all its layers, trainable ones first) loads
    through hdf5_min into the same plan as its in-memory definition."""
    from ecseg_amd import keras_plan as kp
    cfg_txt, w = hdf5_min.load_keras_h5(os.path.join(golden_dir, 'mobilenet_synth.h5'))
    assert isinstance(w['backbone'], kp.NamedWeights) and w['backbone'].names[0] == 'stem/kernel:0'
    assert w['backbone'].names[-1].endswith('moving_variance:0')            # the frozen statistics come last
    plan = kp.build_plan(cfg_txt, w)
    cfg0, w0 = synth.mobilenet_classifier(31)
    plan0 = kp.build_plan(cfg0, w0)
    assert plan.ops == plan0.ops and all(np.array_equal(a, b) for a, b in zip(plan.weights, plan0.weights))
    ops = [o['op'] for o in plan.ops]
    assert kp.OP_DWCONV in ops and kp.OP_PRELU in ops and kp.OP_LAYERNORM in ops and plan.output_rank == 2
    assert any(o['op'] == kp.OP_ADD and o['mode'] == 1 for o in plan.ops)                     # the squeeze-and-excite Multiply
    assert any(o['op'] == kp.OP_CONV and o['dilation'] == 2 for o in plan.ops)                # the dilated 3x3
    assert any(o['op'] == kp.OP_MAXPOOL and o['pad_top'] == 0 and o['kh'] == 3 for o in plan.ops)   # 'same' 3x3 / 2 pooling of 24 rows: pad (0, 1)
    assert 'backbone/b2_se_mul' in plan.layer_tensor and 'backbone' not in plan.layer_tensor  # inlined, prefixed names
    # BatchNormalization folded into the depthwise kernels, ReLU6 fused: DWCONV carries bias + RELU_CLIP(6)
    dws = [o for o in plan.ops if o['op'] == kp.OP_DWCONV]
    assert dws[0]['act'] == kp.ACT['relu_clip'] and dws[0]['alpha'] == 6.0 and dws[0]['w1'] >= 0
    # the grouped convolution: four CONV ops on 8-channel slices of one buffer, writing 8-channel slices of the output
    grp = [o for o in plan.ops if o['op'] == kp.OP_CONV and plan.tensors[o['in0']]['c'] == 8 and o['kh'] == 3]
    assert len(grp) == 4
    assert sorted(plan.tensors[o['in0']]['c_offset'] for o in grp) == [0, 8, 16, 24]
    assert sorted(plan.tensors[o['out']]['c_offset'] for o in grp) == [0, 8, 16, 24]
    assert len({plan.tensors[o['out']]['buffer'] for o in grp}) == 1 and all(plan.tensors[o['out']]['c_stride'] == 32 for o in grp)
    # the separable convolution's swish is not one of the convolution kernels' activations: linear conv + ACT pass
    k = [i for i, o in enumerate(plan.ops) if o['op'] == kp.OP_ACT and o['act'] == kp.ACT['swish']]
    assert len(k) == 1 and plan.ops[k[0] - 1]['op'] == kp.OP_CONV and plan.ops[k[0] - 1]['act'] == 0 and plan.ops[k[0]]['in0'] == plan.ops[k[0]]['out']
    # several outputs: either can be the plan's
    two = json.loads(json.dumps(cfg0))
    two['config']['output_layers'].append(['gap', 0, 0])
    assert kp.build_plan(two, w0).output_tensor == plan0.output_tensor
    p1 = kp.build_plan(two, w0, output=1)
    p1n = kp.build_plan(two, w0, output='gap')
    assert p1.output_tensor == p1n.output_tensor == p1.layer_tensor['gap'] and p1.tensors[p1.output_tensor]['c'] == 32
    # a top-level Sequential whose first layer is a nested model
    seq = {'class_name': 'Sequential', 'config': {'name': 's', 'layers': [
        dict(cfg0['config']['layers'][2], inbound_nodes=[]),
        {'class_name': 'GlobalMaxPooling2D', 'config': {'name': 'gmp'}}]}}
    ps = kp.build_plan(seq, {'backbone': w0['backbone']})
    assert ps.output_rank == 2 and ps.tensors[ps.output_tensor]['c'] == 32
    # Normalization from config statistics and from adapted weights give the same affine op
    norm = lambda **c: {'class_name': 'Sequential', 'config': {'name': 'n', 'layers': [
        {'class_name': 'Normalization', 'config': dict(c, name='norm', batch_input_shape=[None, 8, 8, 3])}]}}
    pa = kp.build_plan(norm(axis=[-1], mean=[1.0, 2.0, 3.0], variance=[4.0, 9.0, 16.0]), {})
    pb = kp.build_plan(norm(axis=[-1], mean=None, variance=None), {'norm': [np.array([1., 2., 3.], np.float32), np.array([4., 9., 16.], np.float32), np.array(7)]})
    assert np.allclose(pa.weights[0], [0.5, 1 / 3, 0.25]) and np.allclose(pa.weights[1], [-0.5, -2 / 3, -0.75])
    assert all(np.array_equal(a, b) for a, b in zip(pa.weights, pb.weights))


def test_shard_bounds_and_records():
    for n, world in [(4096, 8), (10, 4), (3, 8), (0, 2), (7, 1)]:
        seen = []
        per0 = None
        for r in range(world):
            a, b, per = edist.shard_bounds(n, r, world)
            per0 = per if per0 is None else per0
            assert per == per0 and b - a <= per
            seen += list(range(a, b))
        assert seen == list(range(n))
    rec = edist.make_records(5, 3, 4, n_ec=[7, 8, 9])
    assert rec.shape == (4, 16) and rec.nbytes == 4 * 128
    assert list(rec[:, 0]) == [5, 6, 7, -1] and list(rec[:3, 2]) == [7, 8, 9]


def _free_port():
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, world, port, n_images, q):
    os.environ.update(RANK=str(rank), WORLD_SIZE=str(world), MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port),
                      LOCAL_RANK=str(rank))
    import torch
    r, w = edist.init_process_group('gloo')
    a, b, per = edist.shard_bounds(n_images, r, w)
    n_ec = [1000 + i for i in range(a, b)]                       # stands in for this rank's device results
    rec = torch.from_numpy(edist.make_records(a, b - a, per, n_ec=n_ec))
    out = edist.compact_records(edist.allgather_records(rec))
    q.put((rank, out[:, edist.F_INDEX].tolist(), out[:, edist.F_NEC].tolist()))
    torch.distributed.barrier()
    torch.distributed.destroy_process_group()


@pytest.mark.parametrize('n_images', [7, 8])
def test_allgather_records_gloo_world2(n_images):
    import torch.multiprocessing as mp
    ctx = mp.get_context('spawn')
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, n_images, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = [q.get(timeout=120) for _ in procs]
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    for rank, idx, nec in res:
        assert idx == list(range(n_images))
        assert nec == [1000 + i for i in range(n_images)]


def _expected_fields(i):
    """What image i's device results are in the configs[3] rehearsal: a deterministic function of the global index."""
    return (i * 7919) % 20011, [(i * (k + 3) + k) % 9973 for k in range(12)], (3 if i % 997 == 5 else 0), (i * 31) % 1009


def _worker_configs3(rank, world, port, sizes, folder, q):
    os.environ.update(RANK=str(rank), WORLD_SIZE=str(world), MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port), LOCAL_RANK=str(rank))
    import torch
    from ecseg_amd import metaseg
    r, w = edist.init_process_group('gloo')
    digest = []
    for n_images in sizes:
        a, b, per = edist.shard_bounds(n_images, r, w)
        f = [_expected_fields(i) for i in range(a, b)]
        rec = edist.make_records(a, b - a, per, n_ec=[x[0] for x in f], overlay=[x[1] for x in f], status=[x[2] for x in f],
                                 tie_risk=[x[3] for x in f])
        assert rec.shape == (per, edist.RECORD_INT64) and (rec[b - a:, edist.F_INDEX] == -1).all()
        out = edist.compact_records(edist.allgather_records(torch.from_numpy(rec)))
        paths = [os.path.join(folder, 'img%05d.tif' % i) for i in range(n_images)]
        sub = os.path.join(folder, 'n%d' % n_images)
        if r == 0:
            os.makedirs(sub, exist_ok=True)
        failed = metaseg.finish(sub, paths, out, r, log=lambda *a_: None)
        digest.append((n_images, per, out.shape, bool((out[:, edist.F_INDEX] == np.arange(n_images)).all()),
                       int(out[:, edist.F_NEC].sum()), int(out[:, edist.F_OVERLAY:edist.F_OVERLAY + 12].sum()), int(out[:, edist.F_TIE].sum()), len(failed)))
        torch.distributed.barrier()
    q.put((rank, digest))
    torch.distributed.barrier()
    torch.distributed.destroy_process_group()


def test_configs3_4096_records_over_8_gloo_ranks(tmp_path):
    """BASELINE.json configs[3] on paper (no 8-GPU node has ever run it: VERDICT r04 item 8): 4096 images sharded over 8 ranks
    as contiguous blocks of 512, one all-gather of the 128-byte records, every rank ends up with all 4096 rows in
    sorted-path order and rank 0 writes ec_quantification.csv (src/metaseg.py:44-46,56-57) - through shard_bounds /
    make_records / allgather_records / compact_records / metaseg.finish with the job's real sizes; and 4090 images, where the
    last shard is padded (6 rows of index -1)."""
    import torch.multiprocessing as mp
    world, sizes = 8, (4096, 4090)
    ctx = mp.get_context('spawn')
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker_configs3, args=(r, world, port, sizes, str(tmp_path), q)) for r in range(world)]
    for p in procs:
        p.start()
    res = sorted(q.get(timeout=300) for _ in procs)
    for p in procs:
        p.join(timeout=120)
        assert p.exitcode == 0
    assert [r for r, _ in res] == list(range(world))
    for n_images in sizes:
        exp = [_expected_fields(i) for i in range(n_images)]
        want = (n_images, 512, (n_images, edist.RECORD_INT64), True, sum(x[0] for x in exp), sum(sum(x[1]) for x in exp),
                sum(x[3] for x in exp), sum(1 for x in exp if x[2]))
        for rank, digest in res:
            got = [d for d in digest if d[0] == n_images][0]
            assert tuple(got) == want, (rank, got, want)
        text = open(os.path.join(str(tmp_path), 'n%d' % n_images, 'ec_quantification.csv')).read()
        rows = text.strip().split('\n')
        ok = [i for i in range(n_images) if not exp[i][2]]
        assert rows[0] == 'image name,# of ec' and len(rows) == 1 + len(ok)      # (the reference's column name: src/metaseg.py:40)
        assert rows[1:] == ['img%05d.tif,%d' % (i, exp[i][0]) for i in ok]
    assert edist.shard_bounds(4096, 7, 8) == (3584, 4096, 512) and edist.shard_bounds(4090, 7, 8) == (3584, 4090, 512)


@pytest.mark.parametrize('n_convs', [2, 3, 4, 5])
def test_fusable_head_never_shares_a_buffer_with_the_fused_convs_input(n_convs):
    """the 1x1 head may be finished by the output stage of the 3x3 convolution in front of it; workgroups
    then write head pixels while others still read that convolution's input halo, so the two must not share a buffer
    (same rule as the fused 2x2 max-pool).  Plain conv stacks used to re-use the freed input buffer for the head."""
    cfg = synth.conv_stack_config(n_convs)
    plan = keras_plan.build_plan(cfg, synth.unet_weights(cfg))
    head, conv = plan.ops[-1], plan.ops[-2]
    assert head['kh'] == 1 and conv['kh'] == 3 and head['in0'] == conv['out']
    bufs = [plan.tensors[t]['buffer'] for t in (conv['in0'], conv['out'], head['out'])]
    assert len(set(bufs)) == 3, bufs
    for base in (16, 64):                                   # ... and the canonical U-Nets keep the property
        p = keras_plan.build_plan(synth.unet_config(base=base), synth.unet_weights(synth.unet_config(base=base)))
        head, conv = p.ops[-1], p.ops[-2]
        assert len({p.tensors[t]['buffer'] for t in (conv['in0'], conv['out'], head['out'])}) == 3


def test_bench_refuses_more_ranks_than_gpus():
    """`bench.py --gpus N` starts its own ranks; with fewer than N devices visible it must fail loudly (never run one
    rank and report it as N)."""
    import subprocess
    import torch
    if torch.cuda.device_count() >= 2:
        pytest.skip('2 GPUs present')
    env = {k: v for k, v in os.environ.items() if k not in ('RANK', 'WORLD_SIZE', 'LOCAL_RANK')}
    out = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '2', '--steps', '1'], env=env,
                         capture_output=True, text=True, timeout=300)
    assert out.returncode != 0
    assert 'HIP device' in (out.stderr + out.stdout)


@pytest.mark.parametrize('kind', ['interseg', 'ecseg_c'])
def test_plan_of_classifier_graphs(kind, golden_dir):
    """interSeg classifier call shapes (src/interseg.py:96-98): the fixtures written by h5py load through hdf5_min and
    lower to a plan whose output is (N, K)."""
    cfg, w = hdf5_min.load_keras_h5(os.path.join(golden_dir, '%s_synth.h5' % kind))
    ref_cfg = synth.classifier_config(kind)
    assert (json.loads(cfg) if isinstance(cfg, (str, bytes)) else cfg) == ref_cfg
    plan = keras_plan.build_plan(cfg, w)
    to, ti = plan.tensors[plan.output_tensor], plan.tensors[plan.input_tensor]
    assert plan.output_rank == 2 and (to['h'], to['w']) == (1, 1) and to['c'] == (3 if kind == 'interseg' else 1)
    assert (ti['h'], ti['w'], ti['c']) == ((256, 256, 1) if kind == 'interseg' else (256, 256, 3))
    ops = [o['op'] for o in plan.ops]
    assert keras_plan.OP_GLOBALPOOL in ops if kind == 'interseg' else keras_plan.OP_GLOBALPOOL not in ops
    assert any(o['op'] == keras_plan.OP_CONV and o['stride'] == 2 for o in plan.ops)


def test_shipped_library_has_no_diagnostic_kernels():
    """VERDICT r02 #8, r06 "next round" 6: the shipped library holds exactly the F(4x4) kernels it launches - ONE conv_wino4_kernel (split-K
    for a lone 32-channel output block, no template), conv_wino4r_kernel / conv_wino4s_kernel with and without the fused head - and
    wino4_kernel.hip contains no timing-only ablation, cycle stamp or variant hook at all."""
    import re
    import shutil
    import subprocess
    from ecseg_amd._lib import LIB_PATH
    nm = shutil.which('nm') or '/opt/rocm/lib/llvm/bin/llvm-nm'
    out = subprocess.run([nm, '-C', LIB_PATH], capture_output=True, text=True, check=True).stdout
    w4 = sorted(set(re.findall(r' (?:void )?ecseg::(conv_wino4_kernel[^(]*)\(', out)))
    assert w4 == ['conv_wino4_kernel'], w4
    for name in ('conv_wino4r_kernel', 'conv_wino4s_kernel'):
        inst = sorted(set(re.findall(r' ecseg::%s<([^>]*)>\(' % name, out)))
        assert inst == ['false', 'true'], (name, inst)
    src = open(os.path.join(ROOT, 'ecseg_amd', 'csrc', 'wino4_kernel.hip')).read()
    for word in ('ABL', 'STAMP', 'W4_VARIANT', 's_memtime'):
        assert word not in src, word


def test_set_option_no_longer_knows_wino4_rowpass():
    """The superseded non-split conv_wino4_kernel path went together with the option that selected it: ecseg_set_option has no
    "wino4_rowpass" key any more (it fails like any unknown key) and no source of the library names the option.  The same holds for
    "post_graph" (meta_inference replayed from a captured HIP graph: measured +-0 %, retired with its graph cache)."""
    csrc = os.path.join(ROOT, 'ecseg_amd', 'csrc')
    api = open(os.path.join(csrc, 'api.hip')).read()          # (the handle's options live with its life cycle)
    body = api.split('int ecseg_set_option(', 1)[1].split('\n}\n', 1)[0]
    assert '"wino4_split"' in body and 'unknown option or bad value' in body        # (the function this test means to read)
    for retired in ('rowpass', 'post_graph'):
        assert retired not in body
        for f in sorted(f for f in os.listdir(csrc) if f.endswith(('.hip', '.h', '.inc', '.cpp'))):
            assert retired not in open(os.path.join(csrc, f), errors='replace').read(), (retired, f)


def test_no_kernel_of_the_shipped_library_spills_registers():
    """`conv_wino16_kernel<1,1,1,HEAD,*>` spilled 4 / 12 VGPRs to scratch and nothing in the suite looked.  Every
    kernel of every code object inside libecseg_hip.so must report .vgpr_spill_count 0 and no private segment (scratch memory) in
    its metadata notes.  (Scalar registers that overflow are parked in lanes of a vector register - v_writelane, no memory traffic;
    ccl_local_kernel and some wide conv_wino16 variants do that - and are not counted here.)"""
    import shutil
    import struct
    import subprocess
    import tempfile
    from ecseg_amd._lib import LIB_PATH
    readelf = '/opt/rocm/lib/llvm/bin/llvm-readelf'
    if not os.path.exists(readelf) or not shutil.which('objcopy'):
        pytest.skip('no llvm-readelf / objcopy')
    with tempfile.TemporaryDirectory() as d:
        fat = os.path.join(d, 'fat.bin')
        subprocess.run(['objcopy', '-O', 'binary', '--only-section=.hip_fatbin', LIB_PATH, fat], check=True)
        blob = open(fat, 'rb').read()
        kernels = {}
        for m in re.finditer(b'\x7fELF\x02\x01', blob):           # the gfx950 code objects (ELF64, little endian) of the fat binary
            i = m.start()
            shoff = struct.unpack_from('<Q', blob, i + 0x28)[0]
            shentsize, shnum = struct.unpack_from('<HH', blob, i + 0x3a)
            co = os.path.join(d, 'co.elf')
            with open(co, 'wb') as f:
                f.write(blob[i:i + shoff + shentsize * shnum])
            notes = subprocess.run([readelf, '--notes', co], capture_output=True, text=True, check=True).stdout
            for blk in notes.split('- .agpr_count:')[1:]:
                get = lambda k: re.search(r'\.%s:\s+(\S+)' % k, blk).group(1)
                kernels[get('name')] = (int(get('vgpr_spill_count')), int(get('private_segment_fixed_size')))
    assert len(kernels) > 100, len(kernels)
    assert any('conv_wino4s_kernel' in k for k in kernels) and any('conv_wino16_kernel' in k for k in kernels)
    bad = {k: v for k, v in kernels.items() if v != (0, 0)}
    assert not bad, bad


def test_native_launcher_stops_the_peers_of_a_failed_rank(tmp_path):
    """a rank that dies before the record all-gather must not leave its peers (blocked in RCCL) and the parent
    hanging: the supervisor polls ALL children, terminates the others on the first non-zero exit, removes the rendezvous
    directory and returns that exit code."""
    import time
    from ecseg_amd import metaseg
    marker = tmp_path / 'rdzv_seen'
    script = ("import os, sys, time\n"
              "open(%r, 'a').write(os.path.dirname(os.environ['ECSEG_RDZV']) + '\\n')\n"
              "assert len(bytes.fromhex(os.environ['ECSEG_RDZV_NONCE'])) == 16 and os.environ['ECSEG_DIST'] == 'native'\n"
              "if os.environ['RANK'] == '1':\n    time.sleep(0.5); sys.exit(3)\n"
              "time.sleep(120)\n" % str(marker))
    t0 = time.time()
    code = metaseg._supervise_native(3, dict(os.environ), argv=[sys.executable, '-c', script])
    assert code == 3
    assert time.time() - t0 < 30, 'the surviving ranks were waited for'
    dirs = set(marker.read_text().split())
    assert len(dirs) == 1 and not os.path.exists(dirs.pop()), 'rendezvous directory left behind'
    # all ranks succeed: exit code 0
    assert metaseg._supervise_native(2, dict(os.environ), argv=[sys.executable, '-c', 'pass']) == 0


def test_rendezvous_rejects_a_stale_file_of_another_job(tmp_path, monkeypatch):
    """a 128-byte id left at a user-supplied ECSEG_RDZV by a crashed job is not this job's: readers check the
    job nonce in front of the id; the writer replaces the file atomically without following a planted symlink."""
    import threading
    path = str(tmp_path / 'id')
    mine, other = os.urandom(16), os.urandom(16)
    edist.write_rendezvous(path, b'S' * 128, other)                   # stale file of a crashed job
    with pytest.raises(TimeoutError):
        edist.read_rendezvous(path, 128, timeout=0.3, poll=0.05, nonce=mine)
    t = threading.Timer(0.2, edist.write_rendezvous, (path, b'N' * 128, mine))
    t.start()
    assert edist.read_rendezvous(path, 128, timeout=10, poll=0.02, nonce=mine) == b'N' * 128
    t.join()
    assert os.stat(path).st_mode & 0o777 == 0o600
    # a symlink planted at the temporary name is not followed
    victim = tmp_path / 'victim'
    victim.write_bytes(b'keep')
    os.symlink(str(victim), '%s.tmp%d' % (path, os.getpid()))
    edist.write_rendezvous(path, b'M' * 128, mine)
    assert victim.read_bytes() == b'keep'
    monkeypatch.setenv('ECSEG_RDZV_NONCE', mine.hex())
    assert edist.job_nonce() == mine
    # the launcher of a polling rank has gone: stop polling
    with pytest.raises(RuntimeError):
        edist.read_rendezvous(str(tmp_path / 'never'), 128, timeout=10, poll=0.02, nonce=mine, alive=lambda: False)


def test_host_cpu_budget_and_io_thread_default(monkeypatch):
    """The I/O thread pools of the file pipelines are sized by the CPUs this process may really use (affinity capped by the cgroup
    quota), shared between the ranks of the node: 4 ranks x 32 threads inside a 16-CPU quota ran at half the rate of one rank
    (tools/host_scaling.py, EXPERIMENTS.md 6)."""
    from ecseg_amd import utils
    n = utils.host_cpu_budget()
    assert 1 <= n <= (os.cpu_count() or 1)
    monkeypatch.setattr(utils, 'host_cpu_budget', lambda: 16)
    assert utils.default_io_threads(1) == 32 and utils.default_io_threads(4) == 8 and utils.default_io_threads(8) == 4
    monkeypatch.setattr(utils, 'host_cpu_budget', lambda: 2)
    assert utils.default_io_threads(8) == 2                      # never fewer than two
    monkeypatch.setattr(utils, 'host_cpu_budget', lambda: 256)
    assert utils.default_io_threads(1) == 32                     # capped


def test_host_allocator_tuning_is_optional_and_idempotent(monkeypatch):
    from ecseg_amd import utils
    monkeypatch.setattr(utils, '_allocator_tuned', False)
    monkeypatch.setenv('ECSEG_HOST_MALLOC', 'default')
    assert utils.tune_host_allocator() is False and utils._allocator_tuned is False      # opt-out: allocator left alone
    monkeypatch.delenv('ECSEG_HOST_MALLOC')
    first = utils.tune_host_allocator()
    assert isinstance(first, bool) and utils._allocator_tuned is True
    assert utils.tune_host_allocator() is False                                           # once per process
    a = np.ones((1040, 1392), np.int64)                                                    # the allocator still works
    assert int(a.sum()) == 1040 * 1392


def test_integration_stub_structs_match_the_binding():
    """INTEGRATION.md B shows the ctypes stub a reference maintainer would paste into src/utils.py.  Its struct layouts and its
    ABI check must be the ones of the shipped binding (round 5 found the stub one field behind the header)."""
    import ctypes as C
    from ecseg_amd import _lib
    text = open(os.path.join(ROOT, 'INTEGRATION.md')).read()
    stub = text[text.index('class _Tensor(ctypes.Structure)'):text.index('def load_model(model_name):')]
    ns = {'ctypes': C}
    exec(stub, ns)                                        # the two class definitions, nothing else
    for mine, theirs in ((ns['_Tensor'], _lib.TensorDesc), (ns['_Op'], _lib.OpDesc)):
        assert [(n, t) for n, t in mine._fields_] == [(n, t) for n, t in theirs._fields_]
        assert C.sizeof(mine) == C.sizeof(theirs)
    assert '_lib.ecseg_abi_version() == %d' % _lib.ABI_VERSION in text
    # every library call the document makes exists
    for name in set(re.findall(r'_lib\.(ecseg_[a-z0-9_]+)', text)):
        assert name in _lib.EXPORTS, name
