// NuSeT's drivers: the network stage and the proposal layer (nuset_kernels.hip), the marker watershed for one image and for a batch
// and the clean-up behind it (watershed_kernels.hip), and the two rescale calls (rescale_kernels.hip).
#include "driver_util.h"

using namespace ecseg;

// cls / bbox: on the device already (null: upload the host tensors first)
static int rpn_driver(ecseg_ctx* h, const float* d_cls, int cls_cs, const float* d_bbox, int bbox_cs, const float* cls_host,
                      const float* bbox_host, int fh, int fw, int A, const double* ref_anchors, int stride, int im_h, int im_w,
                      float nms_threshold, int pre, int post, int32_t* n_out, float* scores, float* proposals, int32_t* indices) {
    if (n_out) *n_out = 0;
    if (!n_out || !scores || !proposals || !indices || !ref_anchors || fh <= 0 || fw <= 0 || A <= 0 || im_h <= 0 || im_w <= 0)
        return fail(h, ECSEG_E_INVALID, "rpn_proposals: bad arguments");
    if ((long long)fh * fw * A > ECSEG_RPN_MAX_CANDIDATES)
        return fail(h, ECSEG_E_INVALID, "rpn_proposals: more than " + std::to_string(ECSEG_RPN_MAX_CANDIDATES) + " candidates");
    if (pre < 1 || pre > ECSEG_RPN_MAX_PRE_NMS)
        return fail(h, ECSEG_E_INVALID, "rpn_proposals: pre_nms_top_n must be between 1 and " + std::to_string(ECSEG_RPN_MAX_PRE_NMS));
    if (post < 1 || stride < 1 || (long long)stride * std::max(fh, fw) >= (1ll << 31))       // (an anchor coordinate, not a pixel count)
        return fail(h, ECSEG_E_INVALID, "rpn_proposals: post_nms_top_n and stride must be positive");
    USE_DEVICE(h);
    const size_t N = (size_t)fh * fw * A, K = std::min<size_t>((size_t)pre, N), no = std::min<size_t>((size_t)post, K);
    int rc;
    RpnBufs b{};
    if ((rc = lay_out(h, h->call_arena, [&](Carver& c) { b = rpn_bufs(c, fh, fw, A, rpn_sort_len((int)N), pre, post, !d_cls); }))) return rc;
    hipStream_t s = h->stream;
    clear_timings(h);
    if (!d_cls) {
        const size_t px = (size_t)fh * fw;
        HIP_TRY(h, hipMemcpyAsync(b.cls, cls_host, px * 2 * A * sizeof(float), hipMemcpyHostToDevice, s));
        HIP_TRY(h, hipMemcpyAsync(b.bbox, bbox_host, px * 4 * A * sizeof(float), hipMemcpyHostToDevice, s));
        d_cls = b.cls; cls_cs = 2 * A; d_bbox = b.bbox; bbox_cs = 4 * A;
    }
    HIP_TRY(h, hipMemcpyAsync(b.ref, ref_anchors, (size_t)A * 4 * sizeof(double), hipMemcpyHostToDevice, s));
    TIMED(h, s, 0, 1, HIP_TRY(h, run_rpn_proposals(d_cls, cls_cs, d_bbox, bbox_cs, b.ref, fh, fw, A, stride, im_h, im_w, nms_threshold, pre, (int)no, b, s)));
    int32_t misc[2];
    HIP_TRY(h, hipMemcpyAsync(misc, b.misc, sizeof(misc), hipMemcpyDeviceToHost, s));
    WAIT_SET(h, s, 0, 1);                      // (ref_anchors is read by the copy above: it lives until here)
    const int n = misc[0];
    if (n < 0 || (size_t)n > no) return fail(h, ECSEG_E_HIP, "rpn_proposals: the device reported an impossible count");
    *n_out = n;
    if (n > 0) {
        HIP_TRY(h, hipMemcpyAsync(scores, b.out_scores, (size_t)n * sizeof(float), hipMemcpyDeviceToHost, s));
        HIP_TRY(h, hipMemcpyAsync(proposals, b.out_boxes, (size_t)n * 4 * sizeof(float), hipMemcpyDeviceToHost, s));
        HIP_TRY(h, hipMemcpyAsync(indices, b.out_idx, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost, s));
        HIP_TRY(h, hipStreamSynchronize(s));
    }
    return ECSEG_OK;
}

// What a batch of the marker watershed needs, from its table (n x 5: offset, H, W, first marker, markers) and the foreground count of
// every image: the device table with the heap slices laid end to end, the packed bytes up to the end of the last image, the list
// entries in use, the heap elements and the largest image.  Empty string, or what is wrong with image `i`.
struct WsBatchPlan { std::vector<WsImage> tab; size_t span = 0, n_markers = 0, heap_total = 0; int max_px = 0, max_w = 0, max_markers = 0; };
static std::string ws_batch_plan(const int64_t* images, int n_images, const long long* foreground, WsBatchPlan& pl) {
    pl = WsBatchPlan();
    pl.tab.resize((size_t)n_images);
    long long end = 0;
    for (int i = 0; i < n_images; ++i) {
        const int64_t* d = images + 5 * (size_t)i;
        const std::string who = "image " + std::to_string(i);
        const long long off = d[0], H = d[1], W = d[2], first = d[3], n = d[4], fg = foreground[i];
        if (H < 1 || W < 1 || H > ECSEG_WATERSHED_MAX_EXTENT || W > ECSEG_WATERSHED_MAX_EXTENT)
            return who + ": an extent outside 1 .. " + std::to_string(ECSEG_WATERSHED_MAX_EXTENT);
        if (off < end) return who + " overlaps the one in front";
        if (off > (1ll << 62)) return who + ": offset out of range";
        end = off + H * W;
        if (first < 0 || n < 0 || first >= (1ll << 31) || n >= (1ll << 31)) return who + ": a negative or oversized marker range";
        if (fg < 0 || fg > H * W) return who + ": a foreground count outside its pixel count";
        if (5 * fg + 1 >= (1ll << 31)) return who + " holds too many foreground pixels for one heap";
        WsImage& w = pl.tab[(size_t)i];
        w.off = off; w.heap_off = (long long)pl.heap_total; w.H = (int)H; w.W = (int)W; w.first_marker = (int)first; w.n_markers = (int)n;
        w.heap_cap = (int)(5 * fg + 1); w.pad = 0;
        pl.heap_total += (size_t)w.heap_cap;
        pl.n_markers = std::max(pl.n_markers, (size_t)(first + n));
        pl.max_px = std::max(pl.max_px, (int)(H * W)); pl.max_w = std::max(pl.max_w, (int)W); pl.max_markers = std::max(pl.max_markers, (int)n);
    }
    pl.span = (size_t)end;
    return std::string();
}

// The stage products of a marker watershed that the *_stages_debug entries hand back, as host pointers (each may be null: not copied):
// rw, filled, d2 and lab of WatershedBufs / WatershedBatchBufs, `count` elements each.  The plain entries pass four nulls.
struct WsStages { int32_t* rw; uint8_t* filled; int32_t* d2; int32_t* lab; };
static hipError_t ws_read_stages(const WsStages& st, const int32_t* rw, const uint8_t* filled, const int32_t* d2, const int32_t* lab, size_t count,
                                 hipStream_t s) {
    hipError_t e = hipSuccess;
    if (st.rw && (e = hipMemcpyAsync(st.rw, rw, count * sizeof(int32_t), hipMemcpyDeviceToHost, s)) != hipSuccess) return e;
    if (st.filled && (e = hipMemcpyAsync(st.filled, filled, count, hipMemcpyDeviceToHost, s)) != hipSuccess) return e;
    if (st.d2 && (e = hipMemcpyAsync(st.d2, d2, count * sizeof(int32_t), hipMemcpyDeviceToHost, s)) != hipSuccess) return e;
    if (st.lab && (e = hipMemcpyAsync(st.lab, lab, count * sizeof(int32_t), hipMemcpyDeviceToHost, s)) != hipSuccess) return e;
    return e;
}

// ecseg_marker_watershed and ecseg_marker_watershed_stages_debug: one driver, the second with somewhere to put the stage products
static int marker_watershed_driver(ecseg_ctx* h, const uint8_t* mask, int H, int W, const int32_t* marker_rows, const int32_t* marker_cols,
                                   const int32_t* marker_labels, long long n_markers, uint8_t* out, const WsStages& st) {
    DRIVER_OPEN(h);
    if (!mask || !out || H <= 0 || W <= 0) return fail(h, ECSEG_E_INVALID, "marker_watershed: bad arguments");
    if (H > ECSEG_WATERSHED_MAX_EXTENT || W > ECSEG_WATERSHED_MAX_EXTENT)
        return fail(h, ECSEG_E_INVALID, "marker_watershed: an extent above " + std::to_string(ECSEG_WATERSHED_MAX_EXTENT));
    if (n_markers < 0 || n_markers >= (1ll << 31) || (n_markers > 0 && (!marker_rows || !marker_cols || !marker_labels)))
        return fail(h, ECSEG_E_INVALID, "marker_watershed: n_markers must be between 0 and 2^31 - 1, with the three lists");
    const int n = (int)n_markers;
    for (int i = 0; i < n; ++i) {
        if (marker_rows[i] < 0 || marker_rows[i] >= H || marker_cols[i] < 0 || marker_cols[i] >= W)
            return fail(h, ECSEG_E_INVALID, "marker_watershed: marker " + std::to_string(i) + " lies outside the image");
        if (marker_labels[i] < 1) return fail(h, ECSEG_E_INVALID, "marker_watershed: marker " + std::to_string(i) + " has a label below 1");
    }
    const size_t px = (size_t)H * W;
    size_t fg = 0;
    for (size_t p = 0; p < px; ++p) fg += mask[p] != 0;
    if (5 * fg + 1 >= (1ull << 31)) return fail(h, ECSEG_E_INVALID, "marker_watershed: the mask holds too many pixels for one heap");
    const int cap = (int)(5 * fg + 1);
    USE_DEVICE(h);
    int rc;
    WatershedBufs b{};
    if ((rc = lay_out(h, h->call_arena, [&](Carver& c) { b = watershed_bufs(c, H, W, n, cap); }))) return rc;
    hipStream_t s = h->stream;
    clear_timings(h);
    HIP_TRY(h, hipMemcpyAsync(b.mask, mask, px, hipMemcpyHostToDevice, s));
    if (n > 0) {
        HIP_TRY(h, hipMemcpyAsync(b.rows, marker_rows, (size_t)n * sizeof(int32_t), hipMemcpyHostToDevice, s));
        HIP_TRY(h, hipMemcpyAsync(b.cols, marker_cols, (size_t)n * sizeof(int32_t), hipMemcpyHostToDevice, s));
        HIP_TRY(h, hipMemcpyAsync(b.labels, marker_labels, (size_t)n * sizeof(int32_t), hipMemcpyHostToDevice, s));
    }
    TIMED(h, s, 0, 1, HIP_TRY(h, run_marker_watershed(b.mask, H, W, b.rows, b.cols, b.labels, n, cap, b, s)));
    int32_t misc[4] = {0, 0, 0, 0};
    HIP_TRY(h, hipMemcpyAsync(out, b.out, px, hipMemcpyDeviceToHost, s));
    HIP_TRY(h, ws_read_stages(st, b.rw, b.filled, b.d2, b.lab, px, s));
    HIP_TRY(h, hipMemcpyAsync(misc, b.misc, sizeof(misc), hipMemcpyDeviceToHost, s));
    WAIT_SET(h, s, 0, 1);
    if (misc[1]) return fail(h, ECSEG_E_HIP, "marker_watershed: the heap overflowed its bound");
    return ECSEG_OK;
}

// ecseg_marker_watershed_batch and ecseg_marker_watershed_batch_stages_debug, in the same way
static int marker_watershed_batch_driver(ecseg_ctx* h, const uint8_t* masks, long long mask_bytes, const int64_t* images, int n_images,
                                         const int32_t* marker_rows, const int32_t* marker_cols, const int32_t* marker_labels,
                                         long long n_markers, uint8_t* out, const WsStages& st) {
    DRIVER_OPEN(h);
    const std::string me = "marker_watershed_batch: ";
    if (n_images < 0 || n_images > ECSEG_WATERSHED_BATCH_MAX_IMAGES)
        return fail(h, ECSEG_E_INVALID, me + "n_images must be between 0 and " + std::to_string(ECSEG_WATERSHED_BATCH_MAX_IMAGES));
    if (mask_bytes < 0 || n_markers < 0 || n_markers >= (1ll << 31) || (n_images > 0 && (!masks || !images || !out)) ||
        (n_markers > 0 && (!marker_rows || !marker_cols || !marker_labels)))
        return fail(h, ECSEG_E_INVALID, me + "bad arguments");
    clear_timings(h);                                        // (before the images are checked, where ecseg_marker_watershed clears behind its checks)
    if (n_images == 0) return ECSEG_OK;
    std::vector<long long> fg((size_t)n_images, 0);
    WsBatchPlan pl;
    std::string bad = ws_batch_plan(images, n_images, fg.data(), pl);         // the geometry first: nothing is read through a bad offset
    if (!bad.empty()) return fail(h, ECSEG_E_INVALID, me + bad);
    if ((long long)pl.span > mask_bytes) {
        int i = 0;
        while (pl.tab[(size_t)i].off + (long long)pl.tab[(size_t)i].H * pl.tab[(size_t)i].W <= mask_bytes) ++i;
        return fail(h, ECSEG_E_INVALID, me + "image " + std::to_string(i) + " leaves the " + std::to_string(mask_bytes) + " bytes of masks");
    }
    for (int i = 0; i < n_images; ++i) {
        const WsImage& w = pl.tab[(size_t)i];
        if ((long long)w.first_marker + w.n_markers > n_markers)
            return fail(h, ECSEG_E_INVALID, me + "image " + std::to_string(i) + ": its marker range leaves the " + std::to_string(n_markers) + " entries of the lists");
        for (long long k = w.first_marker; k < (long long)w.first_marker + w.n_markers; ++k) {
            const std::string who = me + "image " + std::to_string(i) + ": marker " + std::to_string(k);
            if (marker_rows[k] < 0 || marker_rows[k] >= w.H || marker_cols[k] < 0 || marker_cols[k] >= w.W)
                return fail(h, ECSEG_E_INVALID, who + " lies outside the image");
            if (marker_labels[k] < 1) return fail(h, ECSEG_E_INVALID, who + " has a label below 1");
        }
        const uint8_t* m = masks + w.off;
        const size_t px = (size_t)w.H * w.W;
        size_t n = 0;
        for (size_t p = 0; p < px; ++p) n += m[p] != 0;
        fg[(size_t)i] = (long long)n;
    }
    bad = ws_batch_plan(images, n_images, fg.data(), pl);                     // now with the heaps
    if (!bad.empty()) return fail(h, ECSEG_E_INVALID, me + bad);
    USE_DEVICE(h);
    int rc;
    WatershedBatchBufs b{};
    if ((rc = lay_out(h, h->call_arena, [&](Carver& c) { b = watershed_batch_bufs(c, pl.span, n_images, pl.n_markers, pl.heap_total); })))
        return rc;
    hipStream_t s = h->stream;
    const size_t nm = pl.n_markers, ni = (size_t)n_images;
    HIP_TRY(h, hipMemcpyAsync(b.mask, masks, pl.span, hipMemcpyHostToDevice, s));
    HIP_TRY(h, hipMemcpyAsync(b.tab, pl.tab.data(), ni * sizeof(WsImage), hipMemcpyHostToDevice, s));
    if (nm > 0) {
        HIP_TRY(h, hipMemcpyAsync(b.rows, marker_rows, nm * sizeof(int32_t), hipMemcpyHostToDevice, s));
        HIP_TRY(h, hipMemcpyAsync(b.cols, marker_cols, nm * sizeof(int32_t), hipMemcpyHostToDevice, s));
        HIP_TRY(h, hipMemcpyAsync(b.labels, marker_labels, nm * sizeof(int32_t), hipMemcpyHostToDevice, s));
    }
    TIMED(h, s, 0, 1, HIP_TRY(h, run_marker_watershed_batch(n_images, pl.span, pl.max_px, pl.max_w, pl.max_markers, b, s)));
    std::vector<int32_t> misc(ni * 4, 0);
    HIP_TRY(h, hipMemcpyAsync(out, b.out, pl.span, hipMemcpyDeviceToHost, s));
    HIP_TRY(h, ws_read_stages(st, b.rw, b.filled, b.d2, b.lab, pl.span, s));
    HIP_TRY(h, hipMemcpyAsync(misc.data(), b.misc, misc.size() * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    HIP_TRY(h, hipStreamSynchronize(s));                     // (pl.tab and misc are read and written by the copies above: they live until here)
    std::fill(out + pl.span, out + mask_bytes, (uint8_t)0);  // behind the last image
    timed_set(h, 0, 1);
    for (int i = 0; i < n_images; ++i)
        if (misc[(size_t)i * 4 + 1]) return fail(h, ECSEG_E_HIP, me + "the heap of image " + std::to_string(i) + " overflowed its bound");
    return ECSEG_OK;
}

extern "C" {

// ---- NuSeT's network stage (src/utils.py:35-103) ---------------------------------------------------------------------------
int ecseg_nuset_forward(ecseg_ctx* h, const float* x, int H, int W, int cls_tensor, int bbox_tensor, uint8_t* mask) {
    if (h) drop_sent_ahead(h);                               // (not DRIVER_OPEN: check_model refuses a null handle itself)
    int rc = check_model(h);
    if (rc) return rc;
    h->nuset_cls_t = h->nuset_bbox_t = -1;
    if (!x || !mask || H <= 0 || W <= 0) return fail(h, ECSEG_E_INVALID, "nuset_forward: bad arguments");
    const int nt = (int)h->tensors.size();
    if (cls_tensor < 0 || cls_tensor >= nt || bbox_tensor < 0 || bbox_tensor >= nt || cls_tensor == bbox_tensor)
        return fail(h, ECSEG_E_INVALID, "nuset_forward: bad RPN tensor index");
    const ecseg_tensor_desc& ti = h->tensors[h->input_tensor];
    const ecseg_tensor_desc& to = h->tensors[h->output_tensor];
    const ecseg_tensor_desc& tc = h->tensors[cls_tensor];
    const ecseg_tensor_desc& tb = h->tensors[bbox_tensor];
    if (ti.h != H || ti.w != W || ti.c != 1 || ti.c_stride != 1 || ti.c_offset != 0)
        return fail(h, ECSEG_E_INVALID, "nuset_forward: the loaded plan takes (" + std::to_string(ti.h) + ", " + std::to_string(ti.w) + ", " +
                                            std::to_string(ti.c) + ") inputs, not a (" + std::to_string(H) + ", " + std::to_string(W) + ") image");
    if (to.h != H || to.w != W || to.c != 2) return fail(h, ECSEG_E_INVALID, "nuset_forward: the plan's output is not (H, W, 2) logits");
    if (tc.c < 2 || tc.c % 2 || tb.c != 2 * tc.c || tb.h != tc.h || tb.w != tc.w)
        return fail(h, ECSEG_E_INVALID, "nuset_forward: the RPN tensors are not (fh, fw, 2A) and (fh, fw, 4A)");
    for (const ecseg_tensor_desc& t : h->tensors)
        if (&t != &tc && &t != &tb && (t.buffer == tc.buffer || t.buffer == tb.buffer))
            return fail(h, ECSEG_E_INVALID, "nuset_forward: an RPN tensor shares its buffer with another tensor (build the plan with keep=)");
    USE_DEVICE(h);
    const size_t px = (size_t)H * W;
    if ((rc = ensure_patches(h, 1))) return rc;
    NusetMaskBufs b{};
    if ((rc = lay_out(h, h->call_arena, [&](Carver& c) { b = nuset_mask_bufs(c, H, W); }))) return rc;
    hipStream_t s = h->stream;
    clear_timings(h);
    prof_begin(h);
    HIP_TRY(h, hipMemcpyAsync(view_of(h, h->input_tensor).p, x, px * sizeof(float), hipMemcpyHostToDevice, s));
    TIMED(h, s, 0, 1,
          if ((rc = run_plan(h, 1))) return rc;
          HIP_TRY(h, launch_argmax2(view_of(h, h->output_tensor), b.mask, s)));
    HIP_TRY(h, hipMemcpyAsync(mask, b.mask, px, hipMemcpyDeviceToHost, s));
    HIP_TRY(h, hipStreamSynchronize(s));
    prof_end(h);
    timed_set(h, 0, 1, ECSEG_T_UNET);
    h->nuset_cls_t = cls_tensor; h->nuset_bbox_t = bbox_tensor;
    return ECSEG_OK;
}

int ecseg_rpn_proposals(ecseg_ctx* h, const float* cls_score, const float* bbox_pred, int fh, int fw, int A, const double* ref_anchors,
                        int stride, int im_h, int im_w, float nms_threshold, int pre_nms_top_n, int post_nms_top_n, int32_t* n_out,
                        float* scores, float* proposals, int32_t* indices) {
    DRIVER_OPEN(h);
    if (!cls_score || !bbox_pred) return fail(h, ECSEG_E_INVALID, "rpn_proposals: bad arguments");
    return rpn_driver(h, nullptr, 0, nullptr, 0, cls_score, bbox_pred, fh, fw, A, ref_anchors, stride, im_h, im_w, nms_threshold,
                      pre_nms_top_n, post_nms_top_n, n_out, scores, proposals, indices);
}

int ecseg_rpn_proposals_last(ecseg_ctx* h, int A, const double* ref_anchors, int stride, int im_h, int im_w, float nms_threshold,
                             int pre_nms_top_n, int post_nms_top_n, int32_t* n_out, float* scores, float* proposals, int32_t* indices) {
    if (h) drop_sent_ahead(h);                               // (as ecseg_nuset_forward)
    int rc = check_model(h);
    if (rc) return rc;
    if (h->nuset_cls_t < 0 || h->cap_patches < 1)
        return fail(h, ECSEG_E_INVALID, "rpn_proposals_last: no RPN tensors on the handle (call ecseg_nuset_forward first)");
    const TView c = view_of(h, h->nuset_cls_t), b = view_of(h, h->nuset_bbox_t);
    if (c.c != 2 * A) return fail(h, ECSEG_E_INVALID, "rpn_proposals_last: the RPN tensors hold " + std::to_string(c.c / 2) + " anchors per position");
    return rpn_driver(h, c.p, c.cs, b.p, b.cs, nullptr, nullptr, c.h, c.w, A, ref_anchors, stride, im_h, im_w, nms_threshold, pre_nms_top_n,
                      post_nms_top_n, n_out, scores, proposals, indices);
}

// ---- NuSeT's marker watershed (src/model_layers/marker_watershed.py:82-91) ----------------------------------------------------
int ecseg_marker_watershed(ecseg_ctx* h, const uint8_t* mask, int H, int W, const int32_t* marker_rows, const int32_t* marker_cols,
                           const int32_t* marker_labels, long long n_markers, uint8_t* out) {
    return marker_watershed_driver(h, mask, H, W, marker_rows, marker_cols, marker_labels, n_markers, out, WsStages{});
}

int ecseg_marker_watershed_stages_debug(ecseg_ctx* h, const uint8_t* mask, int H, int W, const int32_t* marker_rows, const int32_t* marker_cols,
                                        const int32_t* marker_labels, long long n_markers, uint8_t* out, int32_t* rw, uint8_t* filled,
                                        int32_t* d2, int32_t* lab) {
    return marker_watershed_driver(h, mask, H, W, marker_rows, marker_cols, marker_labels, n_markers, out, WsStages{rw, filled, d2, lab});
}

// ---- the same over a batch of images, one flood wave per image -----------------------------------------------------------------
long long ecseg_marker_watershed_batch_bytes(const int64_t* images, int n_images, const long long* foreground) {
    if (n_images == 0) return 0;
    if (n_images < 0 || n_images > ECSEG_WATERSHED_BATCH_MAX_IMAGES || !images || !foreground) return -1;
    WsBatchPlan pl;
    if (!ws_batch_plan(images, n_images, foreground, pl).empty()) return -1;
    Carver c;
    (void)watershed_batch_bufs(c, pl.span, n_images, pl.n_markers, pl.heap_total);
    return (long long)c.used;
}

int ecseg_marker_watershed_batch(ecseg_ctx* h, const uint8_t* masks, long long mask_bytes, const int64_t* images, int n_images,
                                 const int32_t* marker_rows, const int32_t* marker_cols, const int32_t* marker_labels, long long n_markers,
                                 uint8_t* out) {
    return marker_watershed_batch_driver(h, masks, mask_bytes, images, n_images, marker_rows, marker_cols, marker_labels, n_markers, out,
                                         WsStages{});
}

int ecseg_marker_watershed_batch_stages_debug(ecseg_ctx* h, const uint8_t* masks, long long mask_bytes, const int64_t* images, int n_images,
                                              const int32_t* marker_rows, const int32_t* marker_cols, const int32_t* marker_labels,
                                              long long n_markers, uint8_t* out, int32_t* rw, uint8_t* filled, int32_t* d2, int32_t* lab) {
    return marker_watershed_batch_driver(h, masks, mask_bytes, images, n_images, marker_rows, marker_cols, marker_labels, n_markers, out,
                                         WsStages{rw, filled, d2, lab});
}

// ---- NuSeT's clean-up behind the marker watershed (src/nuset_utils/normalization.py:25-37, src/utils.py:159-162) -----------------
int ecseg_clean_nuclei(ecseg_ctx* h, const uint8_t* mask, int H, int W, int nuclei_size_t, uint8_t* out, uint8_t* cleaned, double* mean_area) {
    DRIVER_OPEN(h);
    if (!mask || !out || H <= 0 || W <= 0) return fail(h, ECSEG_E_INVALID, "clean_nuclei: bad arguments");
    if (!px_below_2_31(H, W)) return fail(h, ECSEG_E_INVALID, "clean_nuclei: the image must hold fewer than 2^31 pixels");
    if (nuclei_size_t < 0) return fail(h, ECSEG_E_INVALID, "clean_nuclei: nuclei_size_T must not be negative");
    USE_DEVICE(h);
    const size_t px = (size_t)H * W;
    int rc;
    CleanBufs b{};
    if ((rc = lay_out(h, h->call_arena, [&](Carver& c) { b = clean_bufs(c, H, W); }))) return rc;
    hipStream_t s = h->stream;
    clear_timings(h);
    HIP_TRY(h, hipMemcpyAsync(b.mask, mask, px, hipMemcpyHostToDevice, s));
    TIMED(h, s, 0, 1, HIP_TRY(h, run_clean_nuclei(b.mask, H, W, nuclei_size_t, b, s)));
    double dbl[2] = {0.0, 0.0};
    HIP_TRY(h, hipMemcpyAsync(out, b.out, px, hipMemcpyDeviceToHost, s));
    if (cleaned) HIP_TRY(h, hipMemcpyAsync(cleaned, b.cleaned, px, hipMemcpyDeviceToHost, s));
    HIP_TRY(h, hipMemcpyAsync(dbl, b.dbl, sizeof(dbl), hipMemcpyDeviceToHost, s));
    HIP_TRY(h, hipStreamSynchronize(s));
    if (mean_area) *mean_area = dbl[0];
    timed_set(h, 0, 1);
    return ECSEG_OK;
}

// ---- NuSeT's two rescale calls (src/utils.py:136,157-162) ----------------------------------------------------------------------
int ecseg_rescale_down(ecseg_ctx* h, const uint8_t* img, int H, int W, int out_h, int out_w, const double* wy, int ry, const double* wx,
                       int rx, uint8_t* filtered, double* out) {
    DRIVER_OPEN(h);
    if (!img || !out || H <= 0 || W <= 0 || out_h <= 0 || out_w <= 0) return fail(h, ECSEG_E_INVALID, "rescale_down: bad arguments");
    if (!px_below_2_31(H, W)) return fail(h, ECSEG_E_INVALID, "rescale_down: the image must hold fewer than 2^31 pixels");
    if (out_h > H || out_w > W) return fail(h, ECSEG_E_INVALID, "rescale_down: the output extent exceeds the input's");
    if (ry < 0 || rx < 0 || ry > ECSEG_RESCALE_MAX_RADIUS || rx > ECSEG_RESCALE_MAX_RADIUS)
        return fail(h, ECSEG_E_INVALID, "rescale_down: a filter radius outside 0 .. " + std::to_string(ECSEG_RESCALE_MAX_RADIUS));
    if (ry >= H || rx >= W) return fail(h, ECSEG_E_INVALID, "rescale_down: a filter radius reaches across the whole image");
    if ((ry > 0 && !wy) || (rx > 0 && !wx)) return fail(h, ECSEG_E_INVALID, "rescale_down: no weights for a radius above 0");
    USE_DEVICE(h);
    const size_t px = (size_t)H * W, opx = (size_t)out_h * out_w;
    int rc;
    RescaleDownBufs b{};
    if ((rc = lay_out(h, h->call_arena, [&](Carver& c) { b = rescale_down_bufs(c, H, W, out_h, out_w); }))) return rc;
    hipStream_t s = h->stream;
    clear_timings(h);
    HIP_TRY(h, hipMemcpyAsync(b.img, img, px, hipMemcpyHostToDevice, s));
    if (ry > 0) HIP_TRY(h, hipMemcpyAsync(b.wy, wy, (size_t)(2 * ry + 1) * sizeof(double), hipMemcpyHostToDevice, s));
    if (rx > 0) HIP_TRY(h, hipMemcpyAsync(b.wx, wx, (size_t)(2 * rx + 1) * sizeof(double), hipMemcpyHostToDevice, s));
    TIMED(h, s, 0, 1, HIP_TRY(h, run_rescale_down(b.img, H, W, out_h, out_w, b.wy, ry, b.wx, rx, b.tmp, b.filtered, b.v, s)));
    HIP_TRY(h, hipMemcpyAsync(out, b.v, opx * sizeof(double), hipMemcpyDeviceToHost, s));
    if (filtered) HIP_TRY(h, hipMemcpyAsync(filtered, b.filtered, px, hipMemcpyDeviceToHost, s));
    WAIT_SET(h, s, 0, 1);
    return ECSEG_OK;
}

int ecseg_rescale_mask_up(ecseg_ctx* h, const uint8_t* cleaned, int H, int W, int out_h, int out_w, int nuclei_size_t, uint8_t* out) {
    DRIVER_OPEN(h);
    if (!cleaned || !out || H <= 0 || W <= 0 || out_h <= 0 || out_w <= 0) return fail(h, ECSEG_E_INVALID, "rescale_mask_up: bad arguments");
    if (!px_below_2_31(out_h, out_w)) return fail(h, ECSEG_E_INVALID, "rescale_mask_up: the output must hold fewer than 2^31 pixels");
    if (nuclei_size_t < 0) return fail(h, ECSEG_E_INVALID, "rescale_mask_up: nuclei_size_T must not be negative");
    if (out_h < H || out_w < W) return fail(h, ECSEG_E_INVALID, "rescale_mask_up: the output extent is below the input's");
    USE_DEVICE(h);
    const size_t px = (size_t)H * W, opx = (size_t)out_h * out_w;
    int rc;
    RescaleUpBufs b{};
    if ((rc = lay_out(h, h->call_arena, [&](Carver& c) { b = rescale_up_bufs(c, H, W, out_h, out_w); }))) return rc;
    hipStream_t s = h->stream;
    clear_timings(h);
    HIP_TRY(h, hipMemcpyAsync(b.cleaned, cleaned, px, hipMemcpyHostToDevice, s));
    TIMED(h, s, 0, 1, HIP_TRY(h, run_rescale_mask_up(b.cleaned, H, W, out_h, out_w, nuclei_size_t, b, s)));
    HIP_TRY(h, hipMemcpyAsync(out, b.out, opx, hipMemcpyDeviceToHost, s));
    WAIT_SET(h, s, 0, 1);
    return ECSEG_OK;
}

}  // extern "C"
