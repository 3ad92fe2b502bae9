"""Device time of NuSeT's network stage per image: the three-output plan with its argmax (ecseg_nuset_forward) and the proposal
layer (ecseg_rpn_proposals_last), at 304 x 416 (the default ``scale_ratio`` 0.3 of a 1040 x 1392 image, cropped to multiples of 16)
and at 1040 x 1392, with seeded base-64 weights, against the numpy restatement of the proposal layer (tests/nuset_ref.py) on one
core.  Prints one JSON line per size.

    python tools/time_nuset.py [--base 64] [--reps 5] [--sizes 304x416,1040x1392]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..')
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import nuset_ref as ref                                  # noqa: E402
from ecseg_amd import _lib, nuset, synth                 # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--base', type=int, default=64)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--sizes', default='304x416,1040x1392')
    ap.add_argument('--nms-threshold', type=float, default=0.1)
    args = ap.parse_args()
    h = _lib.Handle(0)
    weights = nuset.synth_weights(nuset.nuset_config(16, 16, args.base), seed=0)
    net = nuset.NuSeT(weights, base=args.base, handle=h)
    for size in args.sizes.split(','):
        H, W = (int(v) for v in size.split('x'))
        img = synth.dapi_image(3, 1040, 1392)[:H, :W] if H <= 1040 and W <= 1392 else synth.dapi_image(3, H, W)
        x = nuset.whole_image_norm(img)
        t0 = time.perf_counter()
        mask = net.mask(x)                                   # loads the plan, warms up
        load_s = time.perf_counter() - t0
        base_size = nuset.anchor_size(mask, h) or 16.0
        anchors = nuset.reference_anchors(base_size)
        plan_ms, prop_ms, wall_ms = [], [], []
        for _ in range(args.reps):
            t0 = time.perf_counter()
            mask = net.mask(x)
            plan_ms.append(h.timings()['unet'])
            scores, props, idx = h.rpn_proposals_last(anchors, nuset.STRIDE, H, W, args.nms_threshold)
            prop_ms.append(h.timings()['count'])
            wall_ms.append((time.perf_counter() - t0) * 1e3)
        cls, bbox = (h.read_tensor(net.plan.layer_tensor[n], 1)[0] for n in nuset.RPN_LAYERS[1:])
        t0 = time.perf_counter()
        want = ref.proposals(cls, bbox, anchors, nuset.STRIDE, H, W, args.nms_threshold)
        numpy_ms = (time.perf_counter() - t0) * 1e3
        print(json.dumps(dict(size=[H, W], base=args.base, device=h.device_name, candidates=int(cls.size // 2), kept=int(want['kept']),
                              n_out=int(len(idx)), foreground=float(mask.mean()), anchor_base_size=base_size,
                              plan_ms=float(np.median(plan_ms)), proposals_ms=float(np.median(prop_ms)), wall_ms=float(np.median(wall_ms)),
                              numpy_proposals_ms=numpy_ms, same_selection_as_numpy=bool(np.array_equal(idx, want['indices'])),
                              plan_load_s=load_s, gflop_per_image=h.flops_per_patch() / 1e9)), flush=True)
    h.close()


if __name__ == '__main__':
    main()
