"""NuSeT's network stage (reference src/utils.py:35-103, ``load_nuset``): everything ``sess.run([pred_masks, scores, proposals])``
computes - the U-Net's argmax mask, the RPN head on its pool-4 feature map and the proposal layer (decode, filter, top-k, NMS,
clip) - on the device, behind one three-output plan.  The ``py_func`` half that follows it in the reference is here too, at
``resize_scale == 1`` (``NuSeT.segment``): the marker list of ``marker_watershed`` on the host (``watershed_markers``), the watershed
(``Handle.marker_watershed``) and ``clean_image`` with the final threshold (``Handle.clean_nuclei``) on the device.  At
``0 < resize_scale < 1`` the two ``rescale`` calls around them run on the device too (``Handle.rescale_down``,
``Handle.rescale_mask_up``), as scikit-image 0.18.3 computes them; ``resize_scale > 1`` is not built.

Host side, as in the reference: ``whole_image_norm`` / ``foreground_norm`` (src/nuset_utils/normalization.py), ``anchor_size``
(src/model_layers/anchor_size.py, from the region records of ``ecseg_nuclei_regions``) and ``reference_anchors``
(src/nuset_utils/anchors.py) in float64."""
import numpy as np

from . import _lib, keras_plan, synth

STRIDE = 16                                            # src/utils.py:64
SCALES = (0.5, 1.0, 2.0)                               # :59
RATIOS = (0.125, 0.25, 0.5, 1.0, 2.0, 4.0, 8.0)        # :60
N_ANCHORS = len(SCALES) * len(RATIOS)
PRE_NMS_TOP_N, POST_NMS_TOP_N = 6000, 800              # src/model_layers/rpn_proposal.py:19,25
RPN_LAYERS = ('rpn_conv/3x3', 'rpn_cls_score', 'rpn_bbox_pred')
# layer of ``nuset_config`` -> variable scope of the reference's checkpoints (TF1 numbers unnamed layers in creation order)
CHECKPOINT_SCOPE = dict([('conv%d-%d' % (lv, k), 'model_U-Net/conv%d-%d' % (lv, k)) for lv in range(1, 6) for k in range(1, 5)
                         if k <= 2 or lv <= 4] +
                        [('up4', 'model_U-Net/conv2d_transpose'), ('up3', 'model_U-Net/conv2d_transpose_1'),
                         ('up2', 'model_U-Net/conv2d_transpose_2'), ('up1', 'model_U-Net/conv2d_transpose_3'),
                         ('final', 'model_U-Net/final')] + [(n, 'model_RPN/' + n) for n in RPN_LAYERS])


def nuset_config(h, w, base=64):
    """Keras functional ``model_config`` of NuSeT's network with three outputs: ``final`` (the U-Net's 2-channel logits,
    src/model_layers/models.py:5-136), ``rpn_cls_score`` (2 x 21 channels) and ``rpn_bbox_pred`` (4 x 21) of the RPN head on the
    pool-4 output (src/model_layers/model_RPN.py: ``rpn_conv/3x3`` 3x3 'same' with bias and NO activation, then the two 1x1
    convolutions).  The U-Net is ``synth.nuset_unet_config`` at ``h`` x ``w``, except that only the first up-sampler is followed by a
    ReLU, as in models.py:78-124.  ``h`` and ``w`` must be multiples of 16 (``nuclei_segment`` crops to that, src/utils.py:138-141);
    ``base`` = 64 is the reference's width, smaller ones are for tests."""
    h, w, base = int(h), int(w), int(base)
    if h <= 0 or w <= 0 or h % 16 or w % 16:
        raise ValueError('nuset_config: the image extent must be a positive multiple of 16, got %d x %d' % (h, w))
    if base < 1:
        raise ValueError('nuset_config: base must be positive')
    cfg = synth.nuset_unet_config(base=base, hw=h)
    layers = cfg['config']['layers']
    for L in layers:
        if L['class_name'] == 'InputLayer':
            L['config']['batch_input_shape'] = [None, h, w, 1]
        elif L['name'] in ('up3', 'up2', 'up1'):
            L['config']['activation'] = 'linear'

    def conv(name, x, filters, k):
        layers.append({'class_name': 'Conv2D', 'name': name, 'inbound_nodes': [[[x, 0, 0, {}]]],
                       'config': dict(name=name, filters=filters, kernel_size=[k, k], strides=[1, 1], padding='same' if k == 3 else 'valid',
                                      activation='linear', use_bias=True, dilation_rate=[1, 1], groups=1)})
        return name

    rpn = conv(RPN_LAYERS[0], 'pool4', 8 * base, 3)            # 512 channels at base 64
    conv(RPN_LAYERS[1], rpn, 2 * N_ANCHORS, 1)
    conv(RPN_LAYERS[2], rpn, 4 * N_ANCHORS, 1)
    cfg['config']['name'] = 'nuset'
    cfg['config']['output_layers'] = [['final', 0, 0], [RPN_LAYERS[1], 0, 0], [RPN_LAYERS[2], 0, 0]]
    return cfg


def weight_shapes(config):
    """{layer name: [kernel shape, bias shape]} (no bias shape where the layer has none) in layer order."""
    shapes, cin = {}, {}
    for L in config['config']['layers']:
        cls, lc, name = L['class_name'], L['config'], L['config']['name']
        if cls == 'InputLayer':
            cin[name] = lc['batch_input_shape'][3]
            continue
        srcs = [r[0] for r in L['inbound_nodes'][0]]
        c = sum(cin[s] for s in srcs) if cls == 'Concatenate' else cin[srcs[0]]
        if cls in ('Conv2D', 'Conv2DTranspose'):
            kh, kw = lc['kernel_size']
            f = lc['filters']
            shapes[name] = [(kh, kw, c, f) if cls == 'Conv2D' else (kh, kw, f, c)] + ([(f,)] if lc.get('use_bias', True) else [])
            c = f
        cin[name] = c
    return shapes


def synth_weights(config, seed=0):
    """Seeded weights for ``nuset_config`` (tests and timing), like ``synth.unet_weights``: He-normal kernels on a normalised input;
    the RPN's two 1x1 heads are scaled down so that scores spread over (0, 1) and the decoded boxes stay near their anchors."""
    weights = synth.unet_weights(config, seed=seed, input_scale=1.0)
    for name, shp in weight_shapes(config).items():
        weights[name] = weights[name][:len(shp)]
    weights[RPN_LAYERS[1]][0] = weights[RPN_LAYERS[1]][0] * np.float32(0.5)
    weights[RPN_LAYERS[2]][0] = weights[RPN_LAYERS[2]][0] * np.float32(0.05)
    return weights


def load_weights_npz(path, base=64):
    """Weights of ``nuset_config(., ., base)`` from an ``.npz`` keyed by the checkpoint's variable names
    (``model_U-Net/conv1-1/kernel``, ``.../bias``, ``model_U-Net/conv2d_transpose{,_1,_2,_3}/{kernel,bias}``,
    ``model_U-Net/final/kernel``, ``model_RPN/rpn_conv/3x3/{kernel,bias}``, ``model_RPN/rpn_cls_score/...``,
    ``model_RPN/rpn_bbox_pred/...``; INTEGRATION.md has the TensorFlow lines that write one) -> {layer name: [kernel, bias]} in
    plan order, float32.  A missing or mis-shaped entry raises ``ValueError`` naming its key.  TF1 checkpoints are not read here."""
    out = {}
    with np.load(path) as z:
        for name, shp in weight_shapes(nuset_config(16, 16, base)).items():
            arrs = []
            for part, want in zip(('kernel', 'bias'), shp):
                key = '%s/%s' % (CHECKPOINT_SCOPE[name], part)
                if key not in z.files:
                    raise ValueError('%s: no entry %r' % (path, key))
                a = z[key]
                if tuple(a.shape) != tuple(want):
                    raise ValueError('%s: entry %r has shape %s, expected %s' % (path, key, tuple(a.shape), tuple(want)))
                arrs.append(np.ascontiguousarray(a, np.float32))
            out[name] = arrs
    return out


# ---- host pipeline ------------------------------------------------------------------------------------------------------------
def whole_image_norm(image):
    """(image - mean) / std over the whole image (normalization.py:7-8), float64 arithmetic -> float32."""
    a = np.asarray(image, np.float64)
    with np.errstate(divide='ignore', invalid='ignore'):
        return ((a - a.mean()) / a.std()).astype(np.float32)


def foreground_norm(image, mask):
    """(image - median) / (std + 1e-5) with the statistics of the non-zero pixels of image * mask (normalization.py:10-23) ->
    float32, or None when there is no such pixel (the reference returns a NaN image then)."""
    a = np.asarray(image, np.float64)
    fg = a * np.asarray(mask, np.float64)
    nz = fg[fg != 0]
    if nz.size == 0:
        return None
    return ((a - np.median(nz)) / (nz.std() + 1e-5)).astype(np.float32)


def anchor_size(mask, handle):
    """Median over the 8-connected regions of ``mask`` of max(bounding-box height, width) (anchor_size.py:10-32), float64, from the
    region records of ``handle.nuclei_regions``; None when the mask has no region."""
    m = (np.asarray(mask) != 0).astype(np.uint8)
    rec = handle.nuclei_regions(m, m[..., None], 0)
    if len(rec) == 0:
        return None
    return float(np.median(np.maximum(rec[:, 3] - rec[:, 1], rec[:, 4] - rec[:, 2])))


def reference_anchors(base_size):
    """generate_anchors_reference (src/nuset_utils/anchors.py) in float64: (21, 4) (x1, y1, x2, y2) centred on 0, anchor index =
    ratio index * 3 + scale index."""
    scales, ratios = np.meshgrid(np.asarray(SCALES, np.float64), np.asarray(RATIOS, np.float64))
    scales, sq = scales.reshape(-1), np.sqrt(ratios.reshape(-1))
    heights = scales * sq * np.float64(base_size)
    widths = scales / sq * np.float64(base_size)
    return np.stack([0 - (widths - 1) / 2, 0 - (heights - 1) / 2, 0 + (widths - 1) / 2, 0 + (heights - 1) / 2], axis=-1)


EDGE_LEN, MIN_REGION_AREA = 20, 10                     # src/model_layers/marker_watershed.py:16,65


def _round_half_even(v):
    return int(round(float(v)))                        # Python's round, as the reference calls it


def watershed_markers(scores, proposals, mask, min_score, handle):
    """The host part of ``_watershed`` (marker_watershed.py:22-80): the ordered marker list as int32 (rows, cols, labels), a later
    entry overwriting an earlier one on the same pixel, or None for the two branches that leave the mask as it is (no score, or none
    above ``min_score``).  Kept proposals ascending by score; centre = round-half-even of the float32 mean of the box's ends, the ROW
    from ``bbox[1]`` and ``bbox[3]``; a marker only where the 20-pixel edge mask is 0; a negative centre wraps as numpy's index does
    (-21 and below can land inside), one past the image raises IndexError as the reference does (the proposal layer clips its boxes
    to the image, so neither happens behind it).  Then one marker at the centre of the clipped bounding box of
    every 8-connected region of at least 10 pixels (the records of ``handle.nuclei_regions``, in skimage's order) whose box holds
    no marker yet, possibly on a background pixel."""
    scores = np.asarray(scores, np.float32).reshape(-1)
    proposals = np.asarray(proposals, np.float32).reshape(-1, 4)
    m = (np.asarray(mask) != 0).astype(np.uint8)
    if m.ndim != 2 or len(scores) != len(proposals):
        raise ValueError('watershed_markers takes n scores, (n, 4) proposals and one (H, W) mask')
    H, W = m.shape
    if scores.size == 0 or not scores.max() > min_score:
        return None
    top = scores > min_score
    proposals = proposals[top][scores[top].argsort()]
    placed = np.zeros((H, W), bool)
    rows, cols = [], []
    for b in proposals:
        r = _round_half_even((b[3] + b[1]) / np.float32(2))
        c = _round_half_even((b[2] + b[0]) / np.float32(2))
        if not (-H <= r < H and -W <= c < W):
            raise IndexError('watershed_markers: centre (%d, %d) lies outside the %d x %d image' % (r, c, H, W))
        r, c = r % H, c % W
        if EDGE_LEN <= r < H - EDGE_LEN and EDGE_LEN <= c < W - EDGE_LEN:
            rows.append(r); cols.append(c)
            placed[r, c] = True
    for area, r0, c0, r1, c1 in np.asarray(handle.nuclei_regions(m, m[..., None], 0))[:, :5]:
        if area < MIN_REGION_AREA:
            continue
        r0, r1, c0, c1 = (int(min(v, lim - 1)) for v, lim in ((r0, H), (r1, H), (c0, W), (c1, W)))
        if not placed[r0:r1, c0:c1].any():
            r, c = _round_half_even((r0 + r1) / 2), _round_half_even((c0 + c1) / 2)
            rows.append(r); cols.append(c)
            placed[r, c] = True
    return np.asarray(rows, np.int32), np.asarray(cols, np.int32), np.arange(1, len(rows) + 1, dtype=np.int32)


def _empty():
    return np.zeros(0, np.float32), np.zeros((0, 4), np.float32)


class NuSeT:
    """The network half of ``load_nuset`` on one handle.  ``weights``: {layer name: [kernel, bias]} (``load_weights_npz`` /
    ``synth_weights``); one ``NuSeT`` per checkpoint - the reference keeps two sessions, whole-image-normalised and
    foreground-normalised (src/utils.py:92-102), and ``nuclei_masks`` takes the second one as ``second``."""

    def __init__(self, weights, base=64, handle=None, device=0):
        if handle is None:
            handle = _lib.Handle(device)
        self.handle, self.weights, self.base = handle, weights, int(base)
        self.plan = None

    def _load(self, h, w):
        """The three-output plan at ``h`` x ``w``: re-built and re-loaded when the extent (or the handle's model) changed."""
        ti = self.plan.tensors[self.plan.input_tensor] if self.plan is not None else None
        if ti is None or (ti['h'], ti['w']) != (h, w) or self.handle.plan is not self.plan:
            self.plan = keras_plan.build_plan(nuset_config(h, w, self.base), self.weights, keep=RPN_LAYERS[1:])
            self.handle.load_plan(self.plan)
        return self.plan.layer_tensor[RPN_LAYERS[1]], self.plan.layer_tensor[RPN_LAYERS[2]]

    def mask(self, image_norm):
        """(H, W) normalised image -> uint8 (H, W) argmax mask; the RPN tensors stay on the handle."""
        x = np.ascontiguousarray(image_norm, np.float32)
        if x.ndim != 2:
            raise ValueError('NuSeT takes one (H, W) image')
        cls_t, bbox_t = self._load(*x.shape)
        return self.handle.nuset_forward(x, cls_t, bbox_t)

    def run(self, image_norm, nms_threshold=0.1, pre_nms_top_n=PRE_NMS_TOP_N, post_nms_top_n=POST_NMS_TOP_N):
        """``sess.run([pred_masks, scores, proposals])``: -> (mask uint8 (H, W), scores float32 (n,) descending, proposals float32
        (n, 4) as (x1, y1, x2, y2)).  A mask without a region has no anchor size: no proposals."""
        m = self.mask(image_norm)
        base_size = anchor_size(m, self.handle)
        if base_size is None:
            return (m,) + _empty()
        scores, proposals, _ = self.handle.rpn_proposals_last(reference_anchors(base_size), STRIDE, m.shape[0], m.shape[1], nms_threshold,
                                                              pre_nms_top_n, post_nms_top_n)
        return m, scores, proposals

    def nuclei_masks(self, image, min_score=0.85, nms_threshold=0.1, second=None):
        """The two passes of ``nuclei_segment`` between its ``rescale`` and the watershed (src/utils.py:138-152): crop to multiples of
        16, whole-image norm -> mask -> foreground norm -> ``run`` of ``second`` (the foreground-normalised checkpoint's ``NuSeT``;
        default: this one).  -> (mask, scores, proposals) of the second pass, the proposals being those the watershed takes its
        markers from: ``scores > min_score`` (src/model_layers/marker_watershed.py:22-26).  A first mask without a foreground pixel
        gives an all-zero mask and no proposals."""
        a = np.asarray(image)
        if a.ndim != 2:
            raise ValueError('nuclei_masks takes one (H, W) image')
        H, W = a.shape[0] // 16 * 16, a.shape[1] // 16 * 16
        if H == 0 or W == 0:
            raise ValueError('nuclei_masks: the image is smaller than 16 x 16')
        a = a[:H, :W]
        m1 = self.mask(whole_image_norm(a))
        fg = foreground_norm(a, m1)
        if fg is None:
            return (np.zeros((H, W), np.uint8),) + _empty()
        m, scores, proposals = (second or self).run(fg, nms_threshold)
        top = scores > min_score
        return m, scores[top], proposals[top]

    def segment(self, image, min_score=0.95, nms_threshold=0.01, nuclei_size_T=0, second=None, scale_ratio=1):
        """``nuclei_segment`` (src/utils.py:134-163): ``nuclei_masks``, the markers, the marker watershed, ``clean_image`` and the final
        threshold -> uint8 0 / 255 mask of the cropped extent (multiples of 16).  ``scale_ratio`` (``resize_scale``) below 1: the uint8
        image is shrunk first (``Handle.rescale_down``, :136), everything up to ``clean_image`` runs on the small float64 image, and the
        cleaned mask is scaled back up before the threshold (``Handle.rescale_mask_up``, :157-162) -> a mask of
        ``round(cropped small extent / scale_ratio)``, within a few pixels of the image's extent.  A scaled image below 16 x 16, or a
        ``scale_ratio`` outside (0, 1], raises ``ValueError``."""
        m, mk = self._segment_head(image, min_score, nms_threshold, second, scale_ratio)
        ws = m if mk is None else self.handle.marker_watershed(m, *mk)
        return self._segment_tail(ws, nuclei_size_T, scale_ratio)

    @staticmethod
    def _check_scale(scale_ratio):
        if scale_ratio != 1 and not 0 < scale_ratio < 1:
            raise ValueError('segment: scale_ratio must lie in (0, 1], got %r (above 1 the reference\'s second rescale Gaussian-filters the '
                             '0 / 1 uint8 mask into almost nothing: not built)' % (scale_ratio,))

    def _segment_head(self, image, min_score, nms_threshold, second, scale_ratio):
        """``segment`` up to the watershed: -> (mask, the marker list of ``watershed_markers`` or None)."""
        self._check_scale(scale_ratio)
        if scale_ratio != 1:
            image = np.asarray(image)
            if image.ndim != 2:
                raise ValueError('segment takes one (H, W) image')
            if min(_lib.rescale_extent(image.shape, scale_ratio)) < 16:
                raise ValueError('segment: the image scaled by %s is smaller than 16 x 16' % (scale_ratio,))
            image = self.handle.rescale_down(image, scale_ratio)[0]
        m, scores, proposals = self.nuclei_masks(image, min_score, nms_threshold, second)
        return m, watershed_markers(scores, proposals, m, min_score, self.handle)

    def _segment_tail(self, ws, nuclei_size_T, scale_ratio):
        """``segment`` behind the watershed: ``clean_image``, the rescale back up and the final threshold."""
        if scale_ratio == 1:
            return self.handle.clean_nuclei(ws, nuclei_size_T)[0]
        cleaned = self.handle.clean_nuclei(ws, 0, want_cleaned=True)[2]
        return self.handle.rescale_mask_up(cleaned, 1 / scale_ratio, nuclei_size_T)

    def segment_many(self, images, min_score=0.95, nms_threshold=0.01, nuclei_size_T=0, second=None, scale_ratio=1):
        """``[segment(im, ...) for im in images]``, byte for byte, with the marker watersheds of all images in ONE device call
        (``Handle.marker_watershed_batch``: the flood is one serial wave per image, and the waves of different images run side by
        side).  Everything else runs image after image as in ``segment``: the rescale, the network and the marker list first, the
        clean-up and the rescale back up after the batch; the plan is re-loaded when the extent changes, so images of one extent
        are best kept together.  A ``ValueError`` that ``segment`` would raise for one image (one below 16 x 16 after scaling) is
        RETURNED in that image's place and the others are not disturbed; a ``scale_ratio`` outside (0, 1] raises at once."""
        self._check_scale(scale_ratio)
        heads = []
        for image in images:
            try:
                heads.append(self._segment_head(image, min_score, nms_threshold, second, scale_ratio))
            except ValueError as e:
                heads.append(e)
        good = [k for k, v in enumerate(heads) if not isinstance(v, ValueError)]
        flooded = self.handle.marker_watershed_batch([heads[k][0] for k in good], [heads[k][1] for k in good])
        out = list(heads)
        for k, ws in zip(good, flooded):
            out[k] = self._segment_tail(ws, nuclei_size_T, scale_ratio)
        return out
