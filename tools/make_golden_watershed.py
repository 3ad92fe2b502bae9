#!/opt/conda/bin/python3.9
"""Golden vectors of NuSeT's ``_watershed``, ``clean_image`` and final threshold, taken from the reference's own functions on the
libraries they run on (scikit-image 0.18.3).  Build container only, never on the GPU box:

    tools/make_golden_watershed.py --reference <checkout of the reference>            writes tests/golden/nuset_watershed.npz
    tools/make_golden_watershed.py --reference <...> --campaign 4000                   compares, stores nothing

It imports ``src/model_layers/marker_watershed.py`` and ``src/nuset_utils/normalization.py`` with a stub ``tensorflow`` module (they
import it for the ``py_func`` wrapper only) and ``np.bool = bool`` (``clean_image`` uses the alias numpy 1.24 dropped), runs them
on the cases of tests/watershed_cases.py and stores, per case k: mask_k, scores_k, proposals_k, min_score_k, sizes_k, the outputs
ws_k (``_watershed``) and clean_k (``clean_image`` of it) as uint8, and final_k_<T> (src/utils.py:159-162) per NUCLEI_SIZE_T.  Only
data is stored.

``--campaign N`` runs N seeded random cases through the reference's functions AND through tests/watershed_ref.py and reports every
difference; it also counts the cases on which the restatement's FIFO variant of the flood (``flood_fifo``) differs."""
import argparse
import heapq
import os
import sys
import time
import types
import warnings

import numpy as np

warnings.filterwarnings('ignore')
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, '..', 'tests'))
import watershed_cases as wc                                       # noqa: E402
import watershed_ref as wr                                         # noqa: E402


FIFO_ONLY = []                                                     # cases on which only the FIFO variant of the flood differs


def flood_fifo(mask, markers_rw, d2):
    """``watershed_ref.flood`` with one FIFO per value, markers in raster order, in place of the heap: NOT exact (the campaign counts
    how often), kept to keep that fact measured."""
    m = (np.asarray(mask) != 0).copy()
    H, W = m.shape
    out = (markers_rw * m).astype(np.int64)
    fifo = {}
    keys = []                                            # heap of the values that have a FIFO
    def push(v, item):
        q = fifo.get(v)
        if q is None:
            q = fifo[v] = [0, []]
            heapq.heappush(keys, v)
        q[1].append(item)
    for r, c in zip(*np.nonzero(out)):
        push(-int(d2[r, c]), (int(r), int(c), int(r), int(c)))
    while keys:
        v = keys[0]
        q = fifo[v]
        if q[0] == len(q[1]):
            heapq.heappop(keys)
            del fifo[v]
            continue
        r, c, sr, sc = q[1][q[0]]
        q[0] += 1
        if out[r, c] and (r, c) != (sr, sc):
            continue
        first = 0
        line = False
        for dy, dx in wr.NEIGHBOURS:
            y, x = r + dy, c + dx
            if 0 <= y < H and 0 <= x < W and m[y, x] and out[y, x]:
                if first == 0:
                    first = out[y, x]
                elif out[y, x] != first:
                    line = True
                    break
        if line:
            m[r, c] = False                              # a line pixel leaves the mask; a marker pixel keeps its label
            continue
        out[r, c] = out[sr, sc]
        for dy, dx in wr.NEIGHBOURS:
            y, x = r + dy, c + dx
            if 0 <= y < H and 0 <= x < W and m[y, x] and not out[y, x]:
                push(-int(d2[y, x]), (y, x, sr, sc))
    return out


def load_reference(root):
    sys.modules['tensorflow'] = types.ModuleType('tensorflow')
    if not hasattr(np, 'bool'):
        np.bool = bool
    sys.path.insert(0, os.path.join(root, 'src'))
    from model_layers.marker_watershed import _watershed
    from nuset_utils.normalization import clean_image
    from skimage import morphology

    def final(mw, t):                                              # src/utils.py:159-162, verbatim arithmetic
        with np.errstate(all='ignore'):
            i8 = (((mw - mw.min()) / (mw.max() - mw.min())) * 255).astype(np.uint8)
        i8[i8 > 0] = 255
        i8 = morphology.remove_small_objects(i8.astype('bool'), t).astype('int') * 255
        return i8.astype('uint8')
    return _watershed, clean_image, final


def run_reference(fns, case):
    _watershed, clean_image, final = fns
    with np.errstate(all='ignore'):
        ws = _watershed(case['scores'].copy(), case['proposals'].copy(), case['mask'].astype(np.int32), case['min_score'])
        cl = clean_image(ws)
    return ws, cl, {t: final(cl, t) for t in case['sizes']}


def compare(fns, case):
    """-> list of the stages on which the restatement differs from the reference."""
    ws, cl, fin = run_reference(fns, case)
    bad = []
    mine = wr.watershed(case['scores'], case['proposals'], case['mask'], case['min_score'])
    if not np.array_equal(mine, ws):
        bad.append('watershed(%d px)' % int((mine != ws).sum()))
    fifo = wr.watershed(case['scores'], case['proposals'], case['mask'], case['min_score'], flood_fn=flood_fifo)
    if not np.array_equal(fifo, ws):
        FIFO_ONLY.append(case['name'])
    mc, _ = wr.clean_image(ws)
    if not np.array_equal(mc, cl):
        bad.append('clean_image')
    for t, f in fin.items():
        if not np.array_equal(wr.final_mask(cl, t), f):
            bad.append('final_%d' % t)
    return bad


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reference', default=os.environ.get('NUSET_REFERENCE', ''), help='checkout of the reference project')
    ap.add_argument('--campaign', type=int, default=0)
    ap.add_argument('--first-seed', type=int, default=100000)
    ap.add_argument('--max-extent', type=int, default=128)
    a = ap.parse_args()
    fns = load_reference(a.reference)
    if a.campaign:
        t0, failures = time.time(), []
        for seed in range(a.first_seed, a.first_seed + a.campaign):
            bad = compare(fns, wc.random_case(seed, a.max_extent))
            if bad:
                failures.append(seed)
                print('seed %d: %s' % (seed, ', '.join(bad)), flush=True)
        print('campaign: %d cases, %d with a difference, %.0f s; flood_fifo differs on %d: %s'
              % (a.campaign, len(failures), time.time() - t0, len(FIFO_ONLY), ' '.join(FIFO_ONLY)))
        return 1 if failures else 0
    data, names = {}, []
    for k, case in enumerate(wc.all_cases()):
        ws, cl, fin = run_reference(fns, case)
        assert ws.min() >= 0 and ws.max() <= 1 and cl.max() <= 1
        names.append(case['name'])
        data['mask_%d' % k] = case['mask']
        data['scores_%d' % k] = case['scores']
        data['proposals_%d' % k] = case['proposals']
        data['min_score_%d' % k] = np.float64(case['min_score'])
        data['sizes_%d' % k] = np.asarray(case['sizes'], np.int64)
        data['ws_%d' % k] = ws.astype(np.uint8)
        data['clean_%d' % k] = cl.astype(np.uint8)
        for t, f in fin.items():
            data['final_%d_%d' % (k, t)] = f
        bad = compare(fns, case)
        print('%-32s %3d x %3d  ws %6d  clean %6d  %s' % (case['name'], case['mask'].shape[0], case['mask'].shape[1], int(ws.sum()),
                                                         int(cl.sum()), ', '.join(bad) or 'restatement equal'))
    data['names'] = np.array(names)
    out = os.path.join(HERE, '..', 'tests', 'golden', 'nuset_watershed.npz')
    np.savez_compressed(out, **data)
    print('%s: %d cases, %d bytes' % (os.path.normpath(out), len(names), os.path.getsize(out)))
    return 0


if __name__ == '__main__':
    sys.exit(main())
