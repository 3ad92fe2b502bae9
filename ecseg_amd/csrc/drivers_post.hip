// The one-call drivers of the clean-up and counting kernels (ccl_kernels.hip, meta_inference_kernels.hip, overlay_kernels.hip, stitch_preprocess_kernels.hip): each uploads its inputs, runs its kernels on the main
// stream and downloads the results (u16_to_u8, stitch_argmax, the stitch / preprocess / Otsu stages for the tests, meta_inference, the counts, one labelling pass alone, overlay).
#include "driver_util.h"

using namespace ecseg;

extern "C" {

int ecseg_u16_to_u8(ecseg_ctx* h, const uint16_t* in, long long count, uint8_t* out) {
    DRIVER_OPEN(h);
    if (count < 0 || (count > 0 && (!in || !out))) return fail(h, ECSEG_E_INVALID, "u16_to_u8: bad arguments");
    if (count == 0) return ECSEG_OK;
    USE_DEVICE(h);
    int rc;
    if ((rc = h->d_aux8.ensure(h, (size_t)count * 2))) return rc;
    if ((rc = h->d_gray.ensure(h, (size_t)count))) return rc;
    hipStream_t s = h->stream;
    HIP_TRY(h, hipMemcpyAsync(h->d_aux8, in, (size_t)count * 2, hipMemcpyHostToDevice, s));
    HIP_TRY(h, launch_u16_to_u8(reinterpret_cast<const uint16_t*>(h->d_aux8.p), h->d_gray, (size_t)count, s));
    HIP_TRY(h, hipMemcpyAsync(out, h->d_gray, (size_t)count, hipMemcpyDeviceToHost, s));
    HIP_TRY(h, hipStreamSynchronize(s));
    return ECSEG_OK;                                         // (untimed, as ecseg_stitch_argmax: stage_ms keeps the call before's)
}

int ecseg_stitch_argmax(ecseg_ctx* h, const float* probs, int n_img, int H, int W, uint8_t* labels_raw) {
    DRIVER_OPEN(h);
    if (n_img < 0 || (n_img > 0 && (!probs || !labels_raw))) return fail(h, ECSEG_E_INVALID, "stitch_argmax: bad arguments");
    if (n_img == 0) return ECSEG_OK;
    USE_DEVICE(h);
    StitchPlan* sp = nullptr;
    int rc;
    if ((rc = get_stitch(h, H, W, &sp))) return rc;
    const size_t px = (size_t)H * W, nfl = (size_t)n_img * sp->n_pos * 65536 * 4;
    if ((rc = h->d_probs_in.ensure(h, nfl))) return rc;
    if ((rc = h->d_raw.ensure(h, px * n_img))) return rc;
    hipStream_t s = h->stream;
    HIP_TRY(h, hipMemcpyAsync(h->d_probs_in, probs, nfl * sizeof(float), hipMemcpyHostToDevice, s));
    HIP_TRY(h, launch_stitch_argmax(h->d_probs_in, 4, sp->map_dev, n_img, sp->n_pos, H, W, h->d_raw, s));
    HIP_TRY(h, hipMemcpyAsync(labels_raw, h->d_raw, px * n_img, hipMemcpyDeviceToHost, s));
    HIP_TRY(h, hipStreamSynchronize(s));
    return ECSEG_OK;
}

// Test-only: launch_stitch_argmax with its tie counters and launch_stitch_probs over the WHOLE batch, one launch each (segment_dev
// stitches launch group by launch group), patches with any channel stride; every output may be null.
int ecseg_stitch_stages_debug(ecseg_ctx* h, const float* probs, int chan_stride, int n_img, int H, int W, uint8_t* labels, int32_t* tie_risk,
                              float* probs_out) {
    DRIVER_OPEN(h);
    if (n_img < 0 || chan_stride < 4 || (n_img > 0 && !probs)) return fail(h, ECSEG_E_INVALID, "stitch_stages: bad arguments");
    if (n_img == 0) return ECSEG_OK;
    USE_DEVICE(h);
    StitchPlan* sp = nullptr;
    int rc;
    if ((rc = get_stitch(h, H, W, &sp))) return rc;
    const size_t px = (size_t)H * W, nfl = (size_t)n_img * sp->n_pos * 65536 * chan_stride;
    if ((rc = h->d_probs_in.ensure(h, nfl))) return rc;
    if ((rc = h->d_raw.ensure(h, px * n_img))) return rc;
    if ((rc = h->d_tie.ensure(h, (size_t)n_img))) return rc;
    if ((rc = h->d_tie_sh.ensure(h, (size_t)n_img * G_SHARDS * G_STRIDE))) return rc;
    if (probs_out && (rc = h->d_sprobs.ensure(h, px * n_img * 4))) return rc;
    hipStream_t s = h->stream;
    HIP_TRY(h, hipMemcpyAsync(h->d_probs_in, probs, nfl * sizeof(float), hipMemcpyHostToDevice, s));
    HIP_TRY(h, launch_stitch_argmax(h->d_probs_in, chan_stride, sp->map_dev, n_img, sp->n_pos, H, W, h->d_raw, s, h->d_tie, h->d_tie_sh));
    if (probs_out) HIP_TRY(h, launch_stitch_probs(h->d_probs_in, chan_stride, sp->map_dev, n_img, sp->n_pos, H, W, h->d_sprobs, s));
    if (labels) HIP_TRY(h, hipMemcpyAsync(labels, h->d_raw, px * n_img, hipMemcpyDeviceToHost, s));
    if (tie_risk) HIP_TRY(h, hipMemcpyAsync(tie_risk, h->d_tie, (size_t)n_img * 4, hipMemcpyDeviceToHost, s));
    if (probs_out) HIP_TRY(h, hipMemcpyAsync(probs_out, h->d_sprobs, px * n_img * 4 * sizeof(float), hipMemcpyDeviceToHost, s));
    HIP_TRY(h, hipStreamSynchronize(s));
    return ECSEG_OK;                                         // (untimed: stage_ms keeps the call before's)
}

// Test-only: run_preprocess as ecseg_preprocess runs it, with the histograms and Otsu's thresholds it leaves on the way; every output
// may be null.
int ecseg_preprocess_stages_debug(ecseg_ctx* h, const void* img, int n_img, int H, int W, int C, int bps, uint32_t* hist, int32_t* threshold,
                                  int32_t* inverted, uint8_t* gray) {
    DRIVER_OPEN(h);
    if (n_img < 0 || H <= 0 || W <= 0 || (C != 1 && C != 3 && C != 4) || (bps != 1 && bps != 2) || (n_img > 0 && !img))
        return fail(h, ECSEG_E_INVALID, "preprocess_stages: bad arguments");
    if (n_img == 0) return ECSEG_OK;
    USE_DEVICE(h);
    const size_t px = (size_t)H * W, tot = px * n_img, in_bytes = tot * C * bps;
    int rc;
    if ((rc = h->d_aux8.ensure(h, in_bytes))) return rc;
    if ((rc = h->d_gray.ensure(h, tot))) return rc;
    if ((rc = h->d_i32.ensure(h, (size_t)2 * n_img))) return rc;       // the inverted flags, then the thresholds
    if ((rc = h->d_hist.ensure(h, (size_t)n_img * 256))) return rc;
    hipStream_t s = h->stream;
    HIP_TRY(h, hipMemcpyAsync(h->d_aux8, img, in_bytes, hipMemcpyHostToDevice, s));
    HIP_TRY(h, run_preprocess(h->d_aux8, n_img, H, W, C, bps, h->d_gray, h->d_i32, h->d_hist, s, h->d_i32 + n_img));
    if (hist) HIP_TRY(h, hipMemcpyAsync(hist, h->d_hist, (size_t)n_img * 256 * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    if (threshold) HIP_TRY(h, hipMemcpyAsync(threshold, h->d_i32 + n_img, (size_t)n_img * 4, hipMemcpyDeviceToHost, s));
    if (inverted) HIP_TRY(h, hipMemcpyAsync(inverted, h->d_i32, (size_t)n_img * 4, hipMemcpyDeviceToHost, s));
    if (gray) HIP_TRY(h, hipMemcpyAsync(gray, h->d_gray, tot, hipMemcpyDeviceToHost, s));
    HIP_TRY(h, hipStreamSynchronize(s));
    return ECSEG_OK;                                         // (untimed)
}

// Test-only: otsu_decide_kernel alone on the caller's histograms, each with its own pixel count (which must be its sum).
int ecseg_otsu_debug(ecseg_ctx* h, const uint32_t* hist, int n_img, const int64_t* px, int32_t* threshold, int32_t* inverted) {
    DRIVER_OPEN(h);
    if (n_img < 0 || (n_img > 0 && (!hist || !px))) return fail(h, ECSEG_E_INVALID, "otsu_debug: bad arguments");
    for (int i = 0; i < n_img; ++i) {
        unsigned long long sum = 0;
        for (int b = 0; b < 256; ++b) sum += hist[(size_t)i * 256 + b];
        if (px[i] < 1 || px[i] > 0x7fffffffll || (unsigned long long)px[i] != sum)
            return fail(h, ECSEG_E_INVALID, "otsu_debug: px of histogram " + std::to_string(i) + " is not its sum, or outside 1 .. 2^31 - 1");
    }
    if (n_img == 0) return ECSEG_OK;
    USE_DEVICE(h);
    int rc;
    if ((rc = h->d_hist.ensure(h, (size_t)n_img * 256))) return rc;
    if ((rc = h->d_i64.ensure(h, (size_t)n_img))) return rc;
    if ((rc = h->d_i32.ensure(h, (size_t)2 * n_img))) return rc;       // the inverted flags, then the thresholds
    static_assert(sizeof(long long) == sizeof(int64_t), "px goes up as it is");
    hipStream_t s = h->stream;
    HIP_TRY(h, hipMemcpyAsync(h->d_hist, hist, (size_t)n_img * 256 * sizeof(uint32_t), hipMemcpyHostToDevice, s));
    HIP_TRY(h, hipMemcpyAsync(h->d_i64, px, (size_t)n_img * 8, hipMemcpyHostToDevice, s));
    HIP_TRY(h, launch_otsu_decide(h->d_hist, n_img, h->d_i64, h->d_i32, h->d_i32 + n_img, s));
    if (threshold) HIP_TRY(h, hipMemcpyAsync(threshold, h->d_i32 + n_img, (size_t)n_img * 4, hipMemcpyDeviceToHost, s));
    if (inverted) HIP_TRY(h, hipMemcpyAsync(inverted, h->d_i32, (size_t)n_img * 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(h, hipStreamSynchronize(s));
    return ECSEG_OK;                                         // (untimed)
}

int ecseg_meta_inference_dev(ecseg_ctx* h, const uint8_t* in, int n_img, int H, int W, uint8_t* out, int32_t* n_ec) {
    DRIVER_OPEN(h);
    if (n_img < 0 || H <= 0 || W <= 0 || (n_img > 0 && (!in || !out))) return fail(h, ECSEG_E_INVALID, "meta_inference: bad arguments");
    if (n_img == 0) return ECSEG_OK;
    if (!px_below_2_31(H, W)) return fail(h, ECSEG_E_INVALID, "image too large");
    USE_DEVICE(h);
    const size_t px = (size_t)H * W;
    int rc;
    if ((rc = ensure_post(h, std::min(n_img, h->post_chunk), px))) return rc;
    hipStream_t s = h->stream;
    if (out != in) HIP_TRY(h, hipMemcpyAsync(out, in, px * n_img, hipMemcpyDeviceToDevice, s));
    TIMED(h, s, 0, 1,
          for (int i0 = 0; i0 < n_img; i0 += h->post_chunk) {
              const int ni = std::min(h->post_chunk, n_img - i0);
              HIP_TRY(h, run_meta_inference(h->ws, out + (size_t)i0 * px, ni, H, W, n_ec ? n_ec + i0 : nullptr, s, 1, 6));
          });
    HIP_TRY(h, hipStreamSynchronize(s));
    clear_timings(h);                                        // (behind the wait, where every other driver clears before its upload: a failed call keeps the timings of the one before)
    timed_set(h, 0, 1, ECSEG_T_POST);
    return ECSEG_OK;
}

int ecseg_meta_inference(ecseg_ctx* h, const uint8_t* in, int n_img, int H, int W, uint8_t* out, int32_t* n_ec) {
    DRIVER_OPEN(h);
    if (n_img < 0 || H <= 0 || W <= 0 || (n_img > 0 && (!in || !out))) return fail(h, ECSEG_E_INVALID, "meta_inference: bad arguments");
    if (n_img == 0) return ECSEG_OK;
    USE_DEVICE(h);
    const size_t tot = (size_t)H * W * n_img;
    int rc;
    if ((rc = h->d_post.ensure(h, tot))) return rc;
    if ((rc = h->d_i32.ensure(h, (size_t)n_img))) return rc;
    HIP_TRY(h, hipMemcpyAsync(h->d_post, in, tot, hipMemcpyHostToDevice, h->stream));
    if ((rc = ecseg_meta_inference_dev(h, h->d_post, n_img, H, W, h->d_post, h->d_i32))) return rc;
    HIP_TRY(h, hipMemcpyAsync(out, h->d_post, tot, hipMemcpyDeviceToHost, h->stream));
    if (n_ec) HIP_TRY(h, hipMemcpyAsync(n_ec, h->d_i32, (size_t)n_img * 4, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    return ECSEG_OK;
}

// Test-only: stages first..last of the clean-up alone (run_meta_inference with a partial range), uploaded and chunked as
// ecseg_meta_inference does it; kill_out (may be null): the nucleus test's per-pixel decision when the range holds stage 4.
int ecseg_meta_inference_stages_debug(ecseg_ctx* h, const uint8_t* in, int n_img, int H, int W, int first, int last, uint8_t* out,
                                      uint8_t* kill_out) {
    DRIVER_OPEN(h);
    if (n_img < 0 || H <= 0 || W <= 0 || (n_img > 0 && (!in || !out))) return fail(h, ECSEG_E_INVALID, "meta_inference_stages: bad arguments");
    if (first < 1 || last > 6 || first > last) return fail(h, ECSEG_E_INVALID, "meta_inference_stages: stages are 1..6, first <= last");
    if (n_img == 0) return ECSEG_OK;
    if (!px_below_2_31(H, W)) return fail(h, ECSEG_E_INVALID, "image too large");
    USE_DEVICE(h);
    const size_t px = (size_t)H * W, tot = px * n_img;
    const int chunk = std::min(n_img, h->post_chunk);
    const bool kill = kill_out && first <= 4 && last >= 4;
    int rc;
    if ((rc = h->d_post.ensure(h, tot))) return rc;
    if ((rc = ensure_post(h, chunk, px))) return rc;
    if (kill && (rc = h->d_gray.ensure(h, px * chunk))) return rc;
    hipStream_t s = h->stream;
    HIP_TRY(h, hipMemcpyAsync(h->d_post, in, tot, hipMemcpyHostToDevice, s));
    for (int i0 = 0; i0 < n_img; i0 += chunk) {              // (untimed: stage_ms keeps the call before's)
        const int ni = std::min(chunk, n_img - i0);
        const hipError_t e = run_meta_inference(h->ws, h->d_post.p + (size_t)i0 * px, ni, H, W, nullptr, s, first, last,
                                                kill ? h->d_gray.p : nullptr);
        if (e != hipSuccess) return fail_hip(h, e, "meta_inference_stages kernels");
        if (kill) HIP_TRY(h, hipMemcpyAsync(kill_out + (size_t)i0 * px, h->d_gray, px * ni, hipMemcpyDeviceToHost, s));
    }
    HIP_TRY(h, hipMemcpyAsync(out, h->d_post, tot, hipMemcpyDeviceToHost, s));
    HIP_TRY(h, hipStreamSynchronize(s));
    return ECSEG_OK;
}

enum CountKind { COUNT_CC, COUNT_COLOC, COUNT_HSR, COUNT_LABELS };

// shared driver of the mask-counting entry points: uploads one or two mask stacks, chunks over images
static int count_driver(ecseg_ctx* h, const uint8_t* a, const uint8_t* b, int n_img, int H, int W, CountKind kind, int arg,
                        int32_t* n_out, int64_t* px_out, int32_t* labels_out) {
    DRIVER_OPEN(h);
    if (n_img < 0 || H <= 0 || W <= 0 || (n_img > 0 && !a)) return fail(h, ECSEG_E_INVALID, "count: bad arguments");
    if (n_img == 0) return ECSEG_OK;
    if (!px_below_2_31(H, W)) return fail(h, ECSEG_E_INVALID, "image too large");
    USE_DEVICE(h);
    const size_t px = (size_t)H * W;
    const int chunk = h->post_chunk;
    int rc;
    if ((rc = ensure_post(h, std::min(n_img, chunk), px))) return rc;
    if ((rc = h->d_gray.ensure(h, px * std::min(n_img, chunk)))) return rc;
    if (b && (rc = h->d_aux8.ensure(h, px * std::min(n_img, chunk)))) return rc;
    if ((rc = h->d_i32.ensure(h, labels_out ? px * std::min(n_img, chunk) : (size_t)chunk))) return rc;
    if ((rc = h->d_i64.ensure(h, (size_t)chunk))) return rc;
    hipStream_t s = h->stream;
    clear_timings(h);
    for (int i0 = 0; i0 < n_img; i0 += chunk) {
        const int ni = std::min(chunk, n_img - i0);
        HIP_TRY(h, hipMemcpyAsync(h->d_gray, a + (size_t)i0 * px, px * ni, hipMemcpyHostToDevice, s));
        if (b) HIP_TRY(h, hipMemcpyAsync(h->d_aux8, b + (size_t)i0 * px, px * ni, hipMemcpyHostToDevice, s));
        hipError_t e = hipSuccess;
        TIMED(h, s, 0, 1,
              if (kind == COUNT_CC) e = run_count_cc(h->ws, h->d_gray, ni, H, W, h->d_i32, h->d_i64, s);
              else if (kind == COUNT_COLOC) e = run_count_coloc(h->ws, h->d_gray, h->d_aux8, ni, H, W, h->d_i32, s);
              else if (kind == COUNT_HSR) e = run_count_hsr(h->ws, h->d_gray, h->d_aux8, ni, H, W, arg, h->d_i32, s);
              else e = run_ccl_labels(h->ws, h->d_gray, ni, H, W, arg, h->d_i32, s);
              if (e != hipSuccess) return fail_hip(h, e, "count kernels"));
        if (labels_out) HIP_TRY(h, hipMemcpyAsync(labels_out + (size_t)i0 * px, h->d_i32, px * ni * 4, hipMemcpyDeviceToHost, s));
        else if (n_out) HIP_TRY(h, hipMemcpyAsync(n_out + i0, h->d_i32, (size_t)ni * 4, hipMemcpyDeviceToHost, s));
        if (px_out) HIP_TRY(h, hipMemcpyAsync(px_out + i0, h->d_i64, (size_t)ni * 8, hipMemcpyDeviceToHost, s));
        WAIT_ADD(h, s, 0, 1);
    }
    return ECSEG_OK;
}

int ecseg_count_cc(ecseg_ctx* h, const uint8_t* mask, int n_img, int H, int W, int32_t* n_out, int64_t* px_out) {
    return count_driver(h, mask, nullptr, n_img, H, W, COUNT_CC, 0, n_out, px_out, nullptr);
}
int ecseg_ccl_labels(ecseg_ctx* h, const uint8_t* mask, int n_img, int H, int W, int connectivity, int32_t* labels_out) {
    if (h && connectivity != 4 && connectivity != 8) return fail(h, ECSEG_E_INVALID, "connectivity must be 4 or 8");
    if (h && n_img > 0 && !labels_out) return fail(h, ECSEG_E_INVALID, "labels_out is NULL");
    return count_driver(h, mask, nullptr, n_img, H, W, COUNT_LABELS, connectivity, nullptr, nullptr, labels_out);
}
int ecseg_count_colocalization(ecseg_ctx* h, const uint8_t* ob1, const uint8_t* ob2, int n_img, int H, int W, int32_t* n_out) {
    if (h && n_img > 0 && !ob2) return fail(h, ECSEG_E_INVALID, "ob2 is NULL");
    return count_driver(h, ob1, ob2, n_img, H, W, COUNT_COLOC, 0, n_out, nullptr, nullptr);
}
int ecseg_count_hsr(ecseg_ctx* h, const uint8_t* chrom, const uint8_t* fish, int n_img, int H, int W, int thr, int32_t* n_out) {
    if (h && n_img > 0 && !fish) return fail(h, ECSEG_E_INVALID, "fish is NULL");
    return count_driver(h, chrom, fish, n_img, H, W, COUNT_HSR, thr, n_out, nullptr, nullptr);
}

// Test-only: one labelling pass alone (run_ccl_pass_debug), uploaded and chunked as count_driver does it, every export brought back.
int ecseg_ccl_pass_debug(ecseg_ctx* h, const uint8_t* key_img, const uint8_t* aux_img, int n_img, int H, int W,
                         const ecseg_ccl_pass_desc* pass, const ecseg_ccl_pass_out* out) {
    DRIVER_OPEN(h);
    if (n_img < 0 || H <= 0 || W <= 0 || !pass || (n_img > 0 && (!key_img || !out))) return fail(h, ECSEG_E_INVALID, "ccl_pass_debug: bad arguments");
    if (n_img == 0) return ECSEG_OK;
    if (!out->root || !out->area || !out->sumy || !out->sumx || !out->flag || !out->counters || !out->list1 || !out->list2 || !out->tile_any)
        return fail(h, ECSEG_E_INVALID, "ccl_pass_debug: every output is required");
    if (pass->conn != 4 && pass->conn != 8) return fail(h, ECSEG_E_INVALID, "connectivity must be 4 or 8");
    if (pass->aux_mode == 3 && !aux_img) return fail(h, ECSEG_E_INVALID, "ccl_pass_debug: aux_mode 3 needs aux_img");
    if (pass->n_queries < 0 || pass->n_queries > 5) return fail(h, ECSEG_E_INVALID, "ccl_pass_debug: at most 5 flag queries");
    if ((pass->need & 8) && pass->conn != 8) return fail(h, ECSEG_E_INVALID, "ccl_pass_debug: the root lists are sized for 8-connected components");
    if (pass->n_queries > 0 && pass->count_only) return fail(h, ECSEG_E_INVALID, "ccl_pass_debug: a count_only pass writes no flag words to query");
    if (!px_below_2_31(H, W)) return fail(h, ECSEG_E_INVALID, "image too large");
    USE_DEVICE(h);
    const size_t px = (size_t)H * W, cap = ccl_list_cap(H, W);
    const size_t tiles = (size_t)((H + 31) / 32) * (size_t)((W + 63) / 64);
    const int chunk = std::min(n_img, h->post_chunk);
    int rc;
    CclPassExport b{};
    if ((rc = ensure_post(h, chunk, px))) return rc;
    if ((rc = h->d_gray.ensure(h, px * chunk))) return rc;
    if (aux_img && (rc = h->d_aux8.ensure(h, px * chunk))) return rc;
    if ((rc = lay_out(h, h->call_arena, [&](Carver& c) { b = ccl_pass_export_bufs(c, chunk, px, cap); }))) return rc;
    CclPassDesc d{};
    d.lut = pass->lut; d.conn = pass->conn; d.stat = pass->stat; d.aux_mode = pass->aux_mode; d.aux_c = pass->aux_c; d.need = pass->need;
    d.count_only = pass->count_only != 0; d.sparse = pass->sparse != 0; d.allow_full = pass->allow_full != 0;
    d.n_q = pass->n_queries;
    for (int k = 0; k < 5; ++k) { d.q_key[k] = pass->query_key[k]; d.q_need[k] = pass->query_need[k]; }
    hipStream_t s = h->stream;
    for (int i0 = 0; i0 < n_img; i0 += chunk) {              // (untimed: stage_ms keeps the call before's)
        const int ni = std::min(chunk, n_img - i0);
        const size_t o = (size_t)i0 * px, nb = px * ni;
        HIP_TRY(h, hipMemcpyAsync(h->d_gray, key_img + o, nb, hipMemcpyHostToDevice, s));
        if (aux_img) HIP_TRY(h, hipMemcpyAsync(h->d_aux8, aux_img + o, nb, hipMemcpyHostToDevice, s));
        const hipError_t e = run_ccl_pass_debug(h->ws, h->d_gray, aux_img ? h->d_aux8.p : nullptr, ni, H, W, d, b, s);
        if (e != hipSuccess) return fail_hip(h, e, "ccl_pass_debug kernels");
        HIP_TRY(h, hipMemcpyAsync(out->root + o, b.root, nb * 4, hipMemcpyDeviceToHost, s));
        HIP_TRY(h, hipMemcpyAsync(out->area + o, b.area, nb * 4, hipMemcpyDeviceToHost, s));
        HIP_TRY(h, hipMemcpyAsync(out->sumy + o, b.sumy, nb * 8, hipMemcpyDeviceToHost, s));
        HIP_TRY(h, hipMemcpyAsync(out->sumx + o, b.sumx, nb * 8, hipMemcpyDeviceToHost, s));
        HIP_TRY(h, hipMemcpyAsync(out->flag + o, b.flag, nb * 4, hipMemcpyDeviceToHost, s));
        HIP_TRY(h, hipMemcpyAsync(out->counters + (size_t)i0 * CCL_DEBUG_COUNTERS, b.counters, (size_t)ni * CCL_DEBUG_COUNTERS * 4, hipMemcpyDeviceToHost, s));
        HIP_TRY(h, hipMemcpyAsync(out->list1 + (size_t)i0 * cap, b.list1, (size_t)ni * cap * 4, hipMemcpyDeviceToHost, s));
        HIP_TRY(h, hipMemcpyAsync(out->list2 + (size_t)i0 * cap, b.list2, (size_t)ni * cap * 4, hipMemcpyDeviceToHost, s));
        HIP_TRY(h, hipMemcpyAsync(out->tile_any + (size_t)i0 * tiles, h->ws.tile_any, (size_t)ni * tiles, hipMemcpyDeviceToHost, s));
        HIP_TRY(h, hipStreamSynchronize(s));
    }
    return ECSEG_OK;
}

// Test-only: every scratch arena of ctx.h filled with `byte` over its whole capacity (not the last layout's extent), between two waits
// for every stream of the handle.  Nothing grows or is freed.  The slots that are meant to outlive their call are withdrawn the way
// their owners do it, so that no later call reads the fill as state:
//   keep_arena  iseg (ecseg_nuclei_regions -> ecseg_nucleus_crops, ecseg_classify_nucleus_crops): iseg_n = -1, "no region map";
//   pre_arena   the decode-ahead's file images, tables and status words (pre_file_status): DRIVER_OPEN drops what was sent ahead
//               (pre_tiffs.files = null, without which no call takes the rasters; pre_plan and pre_read_ms keep their values unread);
//   post_arena  ws: only its layout outlives a call, never its contents; dropped, so the next ensure_post lays it out for its own need.
// call_arena, count_arena and ecseg_fish_distances_batch's own buffer carry nothing: the cell index a FISH driver leaves in call_arena is rebuilt by the call that comes back.
int ecseg_scratch_fill_debug(ecseg_ctx* h, int byte) {
    DRIVER_OPEN(h);
    if (byte < 0 || byte > 255) return fail(h, ECSEG_E_INVALID, "scratch_fill_debug: byte must be 0 .. 255");
    USE_DEVICE(h);
    auto wait_all = [&]() -> hipError_t {
        hipError_t e;
        if ((e = hipStreamSynchronize(h->stream)) != hipSuccess) return e;
        if ((e = hipStreamSynchronize(h->stream2)) != hipSuccess) return e;
        if (h->stream_in && (e = hipStreamSynchronize(h->stream_in)) != hipSuccess) return e;
        for (hipStream_t ls : h->lane_streams) if ((e = hipStreamSynchronize(ls)) != hipSuccess) return e;
        return hipSuccess;
    };
    HIP_TRY(h, wait_all());
    h->iseg_n = -1; h->iseg = RegionMapBufs{};
    h->pre_file_status = nullptr;
    h->ws = PostWorkspace{};
    for (DevBuf<uint8_t>* a : {&h->post_arena, &h->call_arena, &h->count_arena, &h->keep_arena, &h->pre_arena, &h->fishdist_batch_buf})
        if (a->p && a->cap) HIP_TRY(h, hipMemsetAsync(a->p, byte, a->cap, h->stream));
    HIP_TRY(h, wait_all());
    return ECSEG_OK;                                         // (untimed: stage_ms keeps the call before's)
}

int ecseg_overlay(ecseg_ctx* h, const uint8_t* labels, const uint8_t* rgb, int n_img, int H, int W, int C, int sens, int hsr_thr,
                  int64_t* out) {
    DRIVER_OPEN(h);
    if (n_img < 0 || H <= 0 || W <= 0 || C < 2 || (n_img > 0 && (!labels || !rgb || !out)))
        return fail(h, ECSEG_E_INVALID, "overlay: bad arguments");
    if (n_img == 0) return ECSEG_OK;
    if (!px_below_2_31(H, W)) return fail(h, ECSEG_E_INVALID, "image too large");
    USE_DEVICE(h);
    const size_t px = (size_t)H * W;
    const int chunk = h->post_chunk;
    int rc;
    if ((rc = ensure_post(h, std::min(n_img, chunk), px))) return rc;
    if ((rc = h->d_gray.ensure(h, px * std::min(n_img, chunk)))) return rc;
    if ((rc = h->d_aux8.ensure(h, px * C * std::min(n_img, chunk)))) return rc;
    if ((rc = h->d_i64.ensure(h, (size_t)chunk * 12))) return rc;
    hipStream_t s = h->stream;
    clear_timings(h);
    for (int i0 = 0; i0 < n_img; i0 += chunk) {
        const int ni = std::min(chunk, n_img - i0);
        HIP_TRY(h, hipMemcpyAsync(h->d_gray, labels + (size_t)i0 * px, px * ni, hipMemcpyHostToDevice, s));
        HIP_TRY(h, hipMemcpyAsync(h->d_aux8, rgb + (size_t)i0 * px * C, px * C * ni, hipMemcpyHostToDevice, s));
        TIMED(h, s, 0, 1, HIP_TRY(h, run_overlay(h->ws, h->d_gray, h->d_aux8, ni, H, W, C, sens, hsr_thr, h->d_i64, s)));
        HIP_TRY(h, hipMemcpyAsync(out + (size_t)i0 * 12, h->d_i64, (size_t)ni * 12 * 8, hipMemcpyDeviceToHost, s));
        WAIT_ADD(h, s, 0, 1);
    }
    return ECSEG_OK;
}

// ecseg_overlay's rows and the red / green PNGs of meta_overlay from one upload: the 8-bit image (u16_to_u8 of 16-bit samples, on the
// device) is counted and then coded channel by channel where it lies (png_gray_encode, drivers_files.hip) and never comes back.
int ecseg_overlay_files(ecseg_ctx* h, const uint8_t* labels, const void* img, int n_img, int H, int W, int C, int bytes_per_sample, int sens,
                        int hsr_thr, int64_t* out, uint8_t* const* red_files, uint8_t* const* green_files, long long file_cap, long long* red_bytes,
                        long long* green_bytes) {
    DRIVER_OPEN(h);
    if (n_img < 0 || n_img >= 65536 || H <= 0 || W <= 0 || C < 2 || C > 256 || (bytes_per_sample != 1 && bytes_per_sample != 2) || file_cap < 1 ||
        ((size_t)W + 1) * (size_t)H >= 0x7fffffffull ||
        (n_img > 0 && (!labels || !img || !out || !red_files || !green_files || !red_bytes || !green_bytes)))
        return fail(h, ECSEG_E_INVALID, "overlay_files: bad arguments");
    for (int i = 0; i < n_img; ++i) if (!red_files[i] || !green_files[i]) return fail(h, ECSEG_E_INVALID, "overlay_files: a null file buffer");
    clear_timings(h);
    h->file_ms[0] = h->file_ms[1] = 0.f;
    if (n_img == 0) return ECSEG_OK;
    for (int i = 0; i < n_img; ++i) red_bytes[i] = green_bytes[i] = 0;
    if (!px_below_2_31(H, W)) return fail(h, ECSEG_E_INVALID, "image too large");
    USE_DEVICE(h);
    const size_t px = (size_t)H * W, bps = (size_t)bytes_per_sample;
    const int chunk = std::min(h->post_chunk, n_img);
    int rc;
    if ((rc = ensure_post(h, chunk, px))) return rc;
    if ((rc = h->d_gray.ensure(h, px * chunk))) return rc;
    if ((rc = h->d_aux8.ensure(h, px * C * bps * chunk))) return rc;
    if ((rc = h->d_i64.ensure(h, (size_t)chunk * 12))) return rc;
    uint8_t* i8 = nullptr;
    GrayEncodeBufs b{};
    if ((rc = lay_out(h, h->call_arena, [&](Carver& c) {
            i8 = c.take<uint8_t>(bps == 2 ? px * C * chunk : 0);
            b = gray_encode_bufs(c, H, W, C, chunk, 2 * chunk, false);
        }))) return rc;
    if (bps == 1) i8 = h->d_aux8.p;
    hipStream_t s = h->stream;
    std::vector<uint8_t*> files((size_t)2 * chunk);
    std::vector<long long> bytes((size_t)2 * chunk);
    for (int i0 = 0; i0 < n_img; i0 += chunk) {
        const int ni = std::min(chunk, n_img - i0);
        HIP_TRY(h, hipMemcpyAsync(h->d_gray, labels + (size_t)i0 * px, px * ni, hipMemcpyHostToDevice, s));
        HIP_TRY(h, hipMemcpyAsync(h->d_aux8, static_cast<const uint8_t*>(img) + (size_t)i0 * px * C * bps, px * C * bps * ni, hipMemcpyHostToDevice, s));
        if (bps == 2) HIP_TRY(h, launch_u16_to_u8(reinterpret_cast<const uint16_t*>(h->d_aux8.p), i8, px * C * ni, s));
        TIMED(h, s, 0, 1, HIP_TRY(h, run_overlay(h->ws, h->d_gray, i8, ni, H, W, C, sens, hsr_thr, h->d_i64, s)));
        HIP_TRY(h, hipMemcpyAsync(out + (size_t)i0 * 12, h->d_i64, (size_t)ni * 12 * 8, hipMemcpyDeviceToHost, s));
        for (int i = 0; i < ni; ++i) { files[2 * (size_t)i] = red_files[i0 + i]; files[2 * (size_t)i + 1] = green_files[i0 + i]; }
        const GraySource src{i8, px * C, (uint32_t)W, (uint32_t)C, (uint32_t)(((size_t)W + 1) * (size_t)H), 2u, 0u | (1u << 8), 1u};
        float ms = 0.f;
        if ((rc = png_gray_encode(h, "overlay_files", src, 2 * ni, H, W, b, files.data(), file_cap, bytes.data(), &ms))) return rc;   // (waits for the stream)
        for (int i = 0; i < ni; ++i) { red_bytes[i0 + i] = bytes[2 * (size_t)i]; green_bytes[i0 + i] = bytes[2 * (size_t)i + 1]; }
        timed_add(h, 0, 1);
        h->file_ms[1] += ms;
        h->stage_ms[ECSEG_T_COUNT] += ms;
    }
    return ECSEG_OK;
}

}  // extern "C"
