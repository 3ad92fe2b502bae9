"""A numpy restatement of NuSeT's proposal layer (reference src/model_layers/rpn_proposal.py with src/nuset_utils/bbox_transform_tf.py
and generate_anchors.py), written from the TensorFlow semantics that the contract of ecseg_rpn_proposals in include/ecseg_hip.h
lists.  Not a test module, and never the product's Python.

``proposals(..., dtype=np.float32)`` is the device's arithmetic: every TensorFlow op rounds to float32, exp is the correctly rounded
float32 exponential (float32 of the float64 one).  ``dtype=np.float64`` is the adjudicator: the same float32 inputs and float32
anchors, every operation after that in double precision.  A case is fit for an exact comparison when both select the same
candidates - no decision of the float32 run hangs on a rounding.

``min_gap`` of a run: over the pair decisions its NMS made (a selected box against every later candidate still alive), the smallest
|IoU - nms_threshold| - bound, where ``bound`` (``iou_bound``) is how far coordinate errors of ``coord_tol`` can move that IoU."""
import numpy as np


def coord_tol(im_h, im_w):
    """What float32 may move a coordinate by: a few ulp of exp and of the half-dozen float32 operations behind a corner, at the
    largest coordinate (the tolerance of the device comparison)."""
    return 4.0 * float(np.spacing(np.float32(max(im_h, im_w))))


def _exp(x, dtype):
    return np.exp(x.astype(np.float64)).astype(dtype)


def all_anchors(ref_anchors, stride, fh, fw):
    """generate_anchors: float32(ref[a] + (x, y, x, y) * stride), the sum in float64; index (y * fw + x) * A + a."""
    ref = np.asarray(ref_anchors, np.float64)
    sx, sy = np.meshgrid(np.arange(fw, dtype=np.float64) * stride, np.arange(fh, dtype=np.float64) * stride)
    shifts = np.stack([sx.reshape(-1), sy.reshape(-1), sx.reshape(-1), sy.reshape(-1)], axis=1)
    return (ref[None] + shifts[:, None]).reshape(-1, 4).astype(np.float32)


def scores_of(cls_score, dtype=np.float32):
    c = np.asarray(cls_score, np.float32).reshape(-1, 2).astype(dtype)
    with np.errstate(invalid='ignore'):
        m = np.maximum(c[:, 0], c[:, 1])
        e0, e1 = _exp(c[:, 0] - m, dtype), _exp(c[:, 1] - m, dtype)
        return e1 / (e0 + e1)


def decode(anchors, deltas, dtype=np.float32):
    """bbox_transform_tf.py:41-66, operation by operation."""
    a = np.asarray(anchors, np.float32).astype(dtype)
    d = np.asarray(deltas, np.float32).reshape(-1, 4).astype(dtype)
    one, half = dtype(1.0), dtype(0.5)
    with np.errstate(invalid='ignore', over='ignore'):
        w = a[:, 2] - a[:, 0] + one
        h = a[:, 3] - a[:, 1] + one
        urx = a[:, 0] + half * w
        ury = a[:, 1] + half * h
        px = d[:, 0] * w + urx
        py = d[:, 1] * h + ury
        pw = _exp(d[:, 2], dtype) * w
        ph = _exp(d[:, 3], dtype) * h
        return np.stack([px - half * pw, py - half * ph, px + half * pw - one, py + half * ph - one], axis=1)


def iou_row(b, others):
    """tf.image.non_max_suppression's IoU of box ``b`` with each of ``others`` ((x1, y1, x2, y2); corners normalised; a box of
    area <= 0 has IoU 0 with everything), in the dtype of the boxes."""
    zero = b.dtype.type(0)
    bx0, bx1, by0, by1 = min(b[0], b[2]), max(b[0], b[2]), min(b[1], b[3]), max(b[1], b[3])
    ox0, ox1 = np.minimum(others[:, 0], others[:, 2]), np.maximum(others[:, 0], others[:, 2])
    oy0, oy1 = np.minimum(others[:, 1], others[:, 3]), np.maximum(others[:, 1], others[:, 3])
    ab = (by1 - by0) * (bx1 - bx0)
    ao = (oy1 - oy0) * (ox1 - ox0)
    ih = np.maximum(np.minimum(by1, oy1) - np.maximum(by0, oy0), zero)
    iw = np.maximum(np.minimum(bx1, ox1) - np.maximum(bx0, ox0), zero)
    inter = ih * iw
    with np.errstate(invalid='ignore', divide='ignore'):
        iou = inter / (ab + ao - inter)
    return np.where((ab > 0) & (ao > 0), iou, zero), ih, iw, ab, ao


def iou_bound(b, others, iou, ih, iw, ab, ao, tol):
    """How far the IoU of two boxes can move when each of their corners moves by at most ``tol``: an extent changes by 2 tol, so
    the intersection changes by d_i <= 2 tol (ih + iw) + 4 tol^2 and each area by 2 tol (w + h) + 4 tol^2; with U = a + b - i,
    |d IoU| <= (d_i + IoU d_U) / (U - d_U), d_U <= d_a + d_b + d_i.  The float32 roundings of the IoU's own six operations add at
    most 6 x 2^-24 IoU.  A pair that does not touch even after such a move (gap > 2 tol) has bound 0: its IoU is 0 either way."""
    b = np.asarray(b, np.float64)
    o = np.asarray(others, np.float64)
    iou, ih, iw, ab, ao = (np.asarray(v, np.float64) for v in (iou, ih, iw, ab, ao))
    wb, hb = abs(b[2] - b[0]), abs(b[3] - b[1])
    wo, ho = np.abs(o[:, 2] - o[:, 0]), np.abs(o[:, 3] - o[:, 1])
    d_i = 2 * tol * (ih + iw) + 4 * tol * tol
    d_u = 2 * tol * (wb + hb) + 2 * tol * (wo + ho) + 8 * tol * tol + d_i
    u = ab + ao - ih * iw
    with np.errstate(invalid='ignore', divide='ignore'):
        bound = (d_i + iou * d_u) / np.maximum(u - d_u, 1e-300) + 6 * 2.0 ** -24 * iou
    # separated by more than the corners can move: IoU stays 0
    gx = np.maximum(np.minimum(o[:, 0], o[:, 2]) - max(b[0], b[2]), min(b[0], b[2]) - np.maximum(o[:, 0], o[:, 2]))
    gy = np.maximum(np.minimum(o[:, 1], o[:, 3]) - max(b[1], b[3]), min(b[1], b[3]) - np.maximum(o[:, 1], o[:, 3]))
    apart = (np.maximum(gx, gy) > 2 * tol) | (ab <= 0) | (ao <= 0)
    return np.where(apart, 0.0, np.where(u - d_u > 0, bound, np.inf))


def proposals(cls_score, bbox_pred, ref_anchors, stride, im_h, im_w, nms_threshold, pre_nms_top_n=6000, post_nms_top_n=800,
              dtype=np.float32, gaps=True):
    """-> dict(scores, proposals, indices: of the selected candidates, in selection order; all_scores, all_boxes: of every
    candidate; kept: how many passed the filter; order: the top-k candidate indices; min_gap).  ``gaps=False`` leaves ``min_gap``
    out (None): the selection is the same and costs half as much, for a caller that already knows the case to be decided."""
    dtype = np.dtype(dtype).type
    cls_score = np.asarray(cls_score, np.float32)
    fh, fw = cls_score.shape[:2]
    anchors = all_anchors(ref_anchors, stride, fh, fw)
    sc = scores_of(cls_score, dtype)
    bx = decode(anchors, bbox_pred, dtype)
    zero = dtype(0)
    with np.errstate(invalid='ignore'):
        keep = (np.maximum(bx[:, 2] - bx[:, 0], zero) * np.maximum(bx[:, 3] - bx[:, 1], zero) > 0) & (sc >= 0)
    cand = np.flatnonzero(keep)
    # tf.nn.top_k: descending, equal values in ascending index order (a stable sort of the negated scores)
    order = cand[np.argsort(-sc[cand], kind='stable')][:min(int(pre_nms_top_n), len(cand))]
    b = bx[order]
    thr = dtype(np.float32(nms_threshold))
    tol = coord_tol(im_h, im_w)
    alive = np.ones(len(order), bool)
    sel, min_gap = [], np.inf
    for i in range(len(order)):
        if not alive[i]:
            continue
        sel.append(i)
        if len(sel) == int(post_nms_top_n):
            break
        rest = np.flatnonzero(alive[i + 1:]) + i + 1
        if len(rest) == 0:
            continue
        iou, ih, iw, ab, ao = iou_row(b[i], b[rest])
        if gaps:
            bound = iou_bound(b[i], b[rest], iou, ih, iw, ab, ao, tol)
            min_gap = min(min_gap, float(np.min(np.abs(iou.astype(np.float64) - float(thr)) - bound)))
        alive[rest[iou > thr]] = False
    sel = np.asarray(sel, np.int64)
    out = b[sel] if len(sel) else np.zeros((0, 4), dtype)
    wmax, hmax = dtype(np.float32(im_w) - np.float32(1)), dtype(np.float32(im_h) - np.float32(1))
    clipped = np.stack([np.maximum(np.minimum(out[:, 0], wmax), zero), np.maximum(np.minimum(out[:, 1], hmax), zero),
                        np.maximum(np.minimum(out[:, 2], wmax), zero), np.maximum(np.minimum(out[:, 3], hmax), zero)], axis=1)
    idx = order[sel] if len(sel) else np.zeros(0, np.int64)
    return dict(scores=sc[idx], proposals=clipped, indices=idx.astype(np.int32), all_scores=sc, all_boxes=bx, kept=len(cand),
                order=order, min_gap=min_gap if gaps else None)


def run_case(c, dtype=np.float32, gaps=True):
    """``proposals`` on a case dict of tests/nuset_cases.py."""
    return proposals(c['cls'], c['bbox'], c['ref'], c['stride'], c['im_h'], c['im_w'], c['thr'], c['pre'], c['post'], dtype=dtype, gaps=gaps)


def judge(c):
    """What makes a case fit for an exact comparison with the device: the float32 run (the device's arithmetic) and the float64
    adjudicator agree on the order of the kept candidates, scores that differ in float64 differ in float32 (ties are ties in both:
    equal inputs), both select the same candidates, and no pair decision of either run comes closer to the threshold than
    coordinate errors of ``coord_tol`` can move an IoU.  -> (None when all of that holds, else the first condition that fails as
    a string; the float32 run)."""
    a, b = run_case(c, np.float32), run_case(c, np.float64)
    return _first_failure(c, a, b), a


def undecided(c):
    """None when case ``c`` is decided alike in float32 and float64 (``judge``), else the reason it is not."""
    return judge(c)[0]


def _first_failure(c, a, b):
    if a['all_scores'].dtype != np.float32 or b['all_scores'].dtype != np.float64:
        return 'the runs are not float32 and float64'
    if a['kept'] != b['kept']:
        return 'kept %d in float32, %d in float64' % (a['kept'], b['kept'])
    if not np.array_equal(a['order'], b['order']):
        return 'the top-k order differs at %d places' % int((a['order'] != b['order']).sum())
    sa, sb = a['all_scores'][a['order']], b['all_scores'][b['order']]
    if not np.array_equal(sa[:-1] == sa[1:], sb[:-1] == sb[1:]):
        return 'scores tie in one precision only'
    if not np.array_equal(a['indices'], b['indices']):
        return 'the selections differ'
    if not (a['min_gap'] > 0 and b['min_gap'] > 0):
        return 'IoU gap %.3g (float32), %.3g (float64)' % (a['min_gap'], b['min_gap'])
    if len(a['scores']):
        err = float(np.abs(a['proposals'].astype(np.float64) - b['proposals']).max())
        if not err <= coord_tol(c['im_h'], c['im_w']):
            return 'coordinates differ by %.3g' % err
        if not np.abs(a['scores'].astype(np.float64) - b['scores']).max() < 1e-6:
            return 'scores differ by 1e-6 or more'
    return None


def case_mismatches(gpu, c, want, raw=False):
    """One device call (``gpu``: a ``_lib.Handle``) on case ``c`` against the restatement's run ``want``, by the assertions of
    tests/test_gpu_nuset.py ``test_proposals_from_given_tensors``; shared by that module and tools/fuzz_nuset.py -> (differences as strings, largest coordinate error, coordinates that are not
    bit-equal[, the device's (scores, proposals, indices)])."""
    scores, props, idx = gpu.rpn_proposals(c['cls'], c['bbox'], c['ref'], c['stride'], c['im_h'], c['im_w'], c['thr'], c['pre'], c['post'])
    bad, err, unequal = [], 0.0, 0
    if (scores.dtype, props.dtype, idx.dtype) != (np.float32, np.float32, np.int32):
        bad.append('dtypes %s %s %s' % (scores.dtype, props.dtype, idx.dtype))
    if not (len(scores) == len(props) == len(idx)) or props.shape != (len(idx), 4):
        bad.append('shapes %s %s %s' % (scores.shape, props.shape, idx.shape))
    elif idx.tolist() != want['indices'].tolist():
        n = min(len(idx), len(want['indices']))
        first = int(np.argmax(idx[:n] != want['indices'][:n])) if (idx[:n] != want['indices'][:n]).any() else n
        bad.append('%d indices, %d expected, the first difference at %d' % (len(idx), len(want['indices']), first))
    else:
        if not np.array_equal(scores, want['scores']):
            bad.append('%d scores differ' % int((scores != want['scores']).sum()))
        if len(idx):
            err = float(np.abs(props.astype(np.float64) - want['proposals'].astype(np.float64)).max())
            unequal = int((props != want['proposals']).sum())
            tol = 4 * float(np.spacing(np.float32(max(c['im_h'], c['im_w']))))
            if not err <= tol:
                bad.append('coordinate error %g above %g' % (err, tol))
            if not np.all(np.diff(scores) <= 0):
                bad.append('scores increase')
            if not (props[:, [0, 2]].min() >= 0 and props[:, [0, 2]].max() <= c['im_w'] - 1 and props[:, [1, 3]].min() >= 0
                    and props[:, [1, 3]].max() <= c['im_h'] - 1):
                bad.append('a proposal outside the image')
    return (bad, err, unequal, (scores, props, idx)) if raw else (bad, err, unequal)
