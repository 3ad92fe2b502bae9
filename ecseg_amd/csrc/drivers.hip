// The one-call drivers: each uploads its inputs, runs one family of kernels on the main stream and downloads the results
// (u16_to_u8, stitch_argmax, meta_inference, the counts, overlay, the interSeg regions / crops, the FISH distances, the FISH spots and their three colour files, TIFF files encoded and decoded on the device, the min-cut tasks, NuSeT's mask and proposals, its marker watershed for one image and for a batch, clean-up and rescale).
#include <cstring>

#include "ctx.h"

#include "png_label_code.h"
#include "tiff_parse.h"

using namespace ecseg;

// The strips of n_files rasters are encoded and packed (run_tiff_encode is done or on a stream that the main stream's end waits
// for): brings the tables over, puts head and tail around every file's strips and copies the strips into the caller's buffers.
int ecseg::tiff_collect(ecseg_ctx* h, const char* who, int n_files, int H, int W, int spp, const TiffEncodeBufs& b, uint8_t* const* files,
                        long long file_cap, long long* file_bytes, bool strict) {
    hipStream_t s = h->stream;
    const size_t ns = (size_t)b.nstrips;
    std::vector<uint32_t> cnt(ns * n_files);
    std::vector<unsigned long long> off((ns + 1) * n_files);
    HIP_TRY(h, hipMemcpyAsync(cnt.data(), b.cnt, cnt.size() * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    HIP_TRY(h, hipMemcpyAsync(off.data(), b.off, off.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
    HIP_TRY(h, hipStreamSynchronize(s));
    std::vector<std::vector<uint8_t>> head(n_files), tail(n_files);
    std::vector<uint32_t> offs(ns);
    for (int f = 0; f < n_files; ++f) {
        const unsigned long long* o = off.data() + (ns + 1) * f;
        const uint32_t* m = cnt.data() + ns * f;
        for (size_t k = 0; k < ns; ++k) {
            if (8 + o[k] + m[k] + 1 >= 0xffffffffull) return fail(h, ECSEG_E_INVALID, std::string(who) + ": the file would pass 4 GiB (classic TIFF has 32-bit offsets)");
            offs[k] = (uint32_t)(8 + o[k]);
        }
        tiff_frame(H, W, spp, b.rps, offs.data(), m, b.nstrips, (size_t)(8 + o[ns]), &head[f], &tail[f]);
        const unsigned long long total = 8 + o[ns] + tail[f].size();
        if (total > (unsigned long long)file_cap && strict)
            return fail(h, ECSEG_E_INVALID, std::string(who) + ": a file of " + std::to_string(total) + " bytes does not fit the capacity of " +
                                                std::to_string(file_cap) + " (ecseg_tiff_encode_bound says what always does)");
        file_bytes[f] = total > (unsigned long long)file_cap ? -(long long)total : (long long)total;
    }
    for (int f = 0; f < n_files; ++f) {
        if (file_bytes[f] < 0) continue;
        const size_t data = (size_t)off[(ns + 1) * f + ns];
        std::memcpy(files[f], head[f].data(), 8);
        HIP_TRY(h, hipMemcpyAsync(files[f] + 8, b.packed + b.file_stride * f, data, hipMemcpyDeviceToHost, s));
        std::memcpy(files[f] + 8 + data, tail[f].data(), tail[f].size());
    }
    HIP_TRY(h, hipStreamSynchronize(s));
    return ECSEG_OK;
}

int ecseg::png_encode_files(ecseg_ctx* h, const char* who, const uint8_t* d_labels, int n, int H, int W, const PngEncodeBufs& b,
                            uint8_t* const* files, long long file_cap, long long* file_bytes, float* ms) {
    hipStream_t s = h->stream;
    const size_t px = (size_t)H * W;
    HIP_TRY(h, hipEventRecord(h->ev_files[2], s));
    HIP_TRY(h, run_png_count(d_labels, px, n, H, W, b, s));
    HIP_TRY(h, hipEventRecord(h->ev_files[3], s));
    std::vector<uint32_t> counts((size_t)n * PNG_NCOUNT);
    HIP_TRY(h, hipMemcpyAsync(counts.data(), b.counts, counts.size() * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    HIP_TRY(h, hipStreamSynchronize(s));
    // the code of every image and with it the exact size of its stream: the stream buffer holds just that, in whole dwords
    std::vector<PngDevCode> codes((size_t)n);
    std::vector<size_t> zb((size_t)n);
    size_t words = 0;
    for (int i = 0; i < n; ++i) {
        const uint32_t* c = counts.data() + (size_t)i * PNG_NCOUNT;
        LabelPngCode k;
        label_png_code(c, c + 4, (uint32_t)H, LABEL_PNG_PALETTE, &k);
        zb[i] = label_png_stream_bytes(k, c, c + 4, (uint32_t)H);
        if (zb[i] >= 0x7fffffffull) return fail(h, ECSEG_E_INVALID, std::string(who) + ": a stream of 2 GiB or more does not fit a PNG chunk");
        PngDevCode& d = codes[i];
        std::memset(&d, 0, sizeof d);
        for (int q = 0; q < 4; ++q) { d.cbits[q] = k.cbits[q]; d.cn[q] = (uint32_t)k.cn[q]; }
        for (int m = 0; m <= 64; ++m) { d.mbits[m] = k.mbits[m]; d.mn[m] = (uint32_t)k.mn[m]; }
        std::memcpy(d.head, k.head, sizeof d.head);
        d.head_bits = k.head_bits; d.filt = k.filt; d.filt_n = (uint32_t)k.filt_n; d.eob = k.eob; d.eob_n = (uint32_t)k.eob_n;
        d.z_off = words; d.z_words = (uint32_t)((zb[i] + 3) / 4);
        words += d.z_words;
    }
    int rc;
    if ((rc = h->count_arena.ensure(h, words * 4, "hipMalloc(png streams)"))) return rc;
    uint32_t* z = reinterpret_cast<uint32_t*>(h->count_arena.p);
    HIP_TRY(h, hipMemcpyAsync(b.codes, codes.data(), codes.size() * sizeof(PngDevCode), hipMemcpyHostToDevice, s));
    HIP_TRY(h, hipEventRecord(h->ev_files[4], s));
    HIP_TRY(h, run_png_emit(d_labels, px, n, H, W, b, z, words * 4, s));
    HIP_TRY(h, hipEventRecord(h->ev_files[5], s));
    std::vector<unsigned long long> dz((size_t)n);
    HIP_TRY(h, hipMemcpyAsync(dz.data(), b.z_bytes, dz.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
    for (int i = 0; i < n; ++i) {
        const size_t total = label_png_file_bytes(zb[i]);
        file_bytes[i] = total > (unsigned long long)file_cap ? -(long long)total : (long long)total;
        if (file_bytes[i] > 0)
            HIP_TRY(h, hipMemcpyAsync(files[i] + LABEL_PNG_Z_OFFSET, z + codes[i].z_off, zb[i], hipMemcpyDeviceToHost, s));
    }
    HIP_TRY(h, hipStreamSynchronize(s));
    for (int i = 0; i < n; ++i) {
        if (dz[i] != zb[i])
            return fail(h, ECSEG_E_HIP, std::string(who) + ": image " + std::to_string(i) + ": the device wrote a stream of " + std::to_string(dz[i]) +
                                            " bytes where the counts give " + std::to_string(zb[i]));
        if (file_bytes[i] > 0) label_png_frame(files[i], zb[i], H, W);
    }
    *ms = stage_elapsed(h->ev_files[2], h->ev_files[3]) + stage_elapsed(h->ev_files[4], h->ev_files[5]);
    return ECSEG_OK;
}

extern "C" {

int ecseg_u16_to_u8(ecseg_ctx* h, const uint16_t* in, long long count, uint8_t* out) {
    if (!h) return ECSEG_E_INVALID;
    drop_sent_ahead(h);
    if (count < 0 || (count > 0 && (!in || !out))) return fail(h, ECSEG_E_INVALID, "u16_to_u8: bad arguments");
    if (count == 0) return ECSEG_OK;
    HIP_TRY(h, hipSetDevice(h->device));
    int rc;
    if ((rc = h->d_aux8.ensure(h, (size_t)count * 2))) return rc;
    if ((rc = h->d_gray.ensure(h, (size_t)count))) return rc;
    hipStream_t s = h->stream;
    HIP_TRY(h, hipMemcpyAsync(h->d_aux8, in, (size_t)count * 2, hipMemcpyHostToDevice, s));
    HIP_TRY(h, launch_u16_to_u8(reinterpret_cast<const uint16_t*>(h->d_aux8.p), h->d_gray, (size_t)count, s));
    HIP_TRY(h, hipMemcpyAsync(out, h->d_gray, (size_t)count, hipMemcpyDeviceToHost, s));
    HIP_TRY(h, hipStreamSynchronize(s));
    return ECSEG_OK;
}

int ecseg_stitch_argmax(ecseg_ctx* h, const float* probs, int n_img, int H, int W, uint8_t* labels_raw) {
    if (!h) return ECSEG_E_INVALID;
    drop_sent_ahead(h);
    if (n_img < 0 || (n_img > 0 && (!probs || !labels_raw))) return fail(h, ECSEG_E_INVALID, "stitch_argmax: bad arguments");
    if (n_img == 0) return ECSEG_OK;
    HIP_TRY(h, hipSetDevice(h->device));
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

int ecseg_meta_inference_dev(ecseg_ctx* h, const uint8_t* in, int n_img, int H, int W, uint8_t* out, int32_t* n_ec) {
    if (!h) return ECSEG_E_INVALID;
    drop_sent_ahead(h);
    if (n_img < 0 || H <= 0 || W <= 0 || (n_img > 0 && (!in || !out))) return fail(h, ECSEG_E_INVALID, "meta_inference: bad arguments");
    if (n_img == 0) return ECSEG_OK;
    if ((long long)H * W >= (1ll << 31)) return fail(h, ECSEG_E_INVALID, "image too large");
    HIP_TRY(h, hipSetDevice(h->device));
    const size_t px = (size_t)H * W;
    int rc;
    if ((rc = ensure_post(h, std::min(n_img, h->post_chunk), px))) return rc;
    hipStream_t s = h->stream;
    if (out != in) HIP_TRY(h, hipMemcpyAsync(out, in, px * n_img, hipMemcpyDeviceToDevice, s));
    HIP_TRY(h, hipEventRecord(h->ev[0], s));
    for (int i0 = 0; i0 < n_img; i0 += h->post_chunk) {
        const int ni = std::min(h->post_chunk, n_img - i0);
        HIP_TRY(h, run_meta_inference(h->ws, out + (size_t)i0 * px, ni, H, W, n_ec ? n_ec + i0 : nullptr, s));
    }
    HIP_TRY(h, hipEventRecord(h->ev[1], s));
    HIP_TRY(h, hipStreamSynchronize(s));
    for (float& v : h->stage_ms) v = 0.f;
    h->stage_ms[ECSEG_T_POST] = stage_elapsed(h->ev[0], h->ev[1]);
    return ECSEG_OK;
}

int ecseg_meta_inference(ecseg_ctx* h, const uint8_t* in, int n_img, int H, int W, uint8_t* out, int32_t* n_ec) {
    if (!h) return ECSEG_E_INVALID;
    drop_sent_ahead(h);
    if (n_img < 0 || H <= 0 || W <= 0 || (n_img > 0 && (!in || !out))) return fail(h, ECSEG_E_INVALID, "meta_inference: bad arguments");
    if (n_img == 0) return ECSEG_OK;
    HIP_TRY(h, hipSetDevice(h->device));
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

// shared driver of the mask-counting entry points: uploads one or two mask stacks, chunks over images
static int count_driver(ecseg_ctx* h, const uint8_t* a, const uint8_t* b, int n_img, int H, int W, int kind, int arg,
                        int32_t* n_out, int64_t* px_out, int32_t* labels_out) {
    if (!h) return ECSEG_E_INVALID;
    drop_sent_ahead(h);
    if (n_img < 0 || H <= 0 || W <= 0 || (n_img > 0 && !a)) return fail(h, ECSEG_E_INVALID, "count: bad arguments");
    if (n_img == 0) return ECSEG_OK;
    if ((long long)H * W >= (1ll << 31)) return fail(h, ECSEG_E_INVALID, "image too large");
    HIP_TRY(h, hipSetDevice(h->device));
    const size_t px = (size_t)H * W;
    const int chunk = h->post_chunk;
    int rc;
    if ((rc = ensure_post(h, std::min(n_img, chunk), px))) return rc;
    if ((rc = h->d_gray.ensure(h, px * std::min(n_img, chunk)))) return rc;
    if (b && (rc = h->d_aux8.ensure(h, px * std::min(n_img, chunk)))) return rc;
    if ((rc = h->d_i32.ensure(h, labels_out ? px * std::min(n_img, chunk) : (size_t)chunk))) return rc;
    if ((rc = h->d_i64.ensure(h, (size_t)chunk))) return rc;
    hipStream_t s = h->stream;
    for (float& v : h->stage_ms) v = 0.f;
    for (int i0 = 0; i0 < n_img; i0 += chunk) {
        const int ni = std::min(chunk, n_img - i0);
        HIP_TRY(h, hipMemcpyAsync(h->d_gray, a + (size_t)i0 * px, px * ni, hipMemcpyHostToDevice, s));
        if (b) HIP_TRY(h, hipMemcpyAsync(h->d_aux8, b + (size_t)i0 * px, px * ni, hipMemcpyHostToDevice, s));
        hipError_t e = hipSuccess;
        HIP_TRY(h, hipEventRecord(h->ev[0], s));
        if (kind == 0) e = run_count_cc(h->ws, h->d_gray, ni, H, W, h->d_i32, h->d_i64, s);
        else if (kind == 1) e = run_count_coloc(h->ws, h->d_gray, h->d_aux8, ni, H, W, h->d_i32, s);
        else if (kind == 2) e = run_count_hsr(h->ws, h->d_gray, h->d_aux8, ni, H, W, arg, h->d_i32, s);
        else e = run_ccl_labels(h->ws, h->d_gray, ni, H, W, arg, h->d_i32, s);
        if (e != hipSuccess) return fail_hip(h, e, "count kernels");
        HIP_TRY(h, hipEventRecord(h->ev[1], s));
        if (labels_out) HIP_TRY(h, hipMemcpyAsync(labels_out + (size_t)i0 * px, h->d_i32, px * ni * 4, hipMemcpyDeviceToHost, s));
        else if (n_out) HIP_TRY(h, hipMemcpyAsync(n_out + i0, h->d_i32, (size_t)ni * 4, hipMemcpyDeviceToHost, s));
        if (px_out) HIP_TRY(h, hipMemcpyAsync(px_out + i0, h->d_i64, (size_t)ni * 8, hipMemcpyDeviceToHost, s));
        HIP_TRY(h, hipStreamSynchronize(s));
        h->stage_ms[ECSEG_T_COUNT] += stage_elapsed(h->ev[0], h->ev[1]);
    }
    return ECSEG_OK;
}

int ecseg_count_cc(ecseg_ctx* h, const uint8_t* mask, int n_img, int H, int W, int32_t* n_out, int64_t* px_out) {
    return count_driver(h, mask, nullptr, n_img, H, W, 0, 0, n_out, px_out, nullptr);
}
int ecseg_ccl_labels(ecseg_ctx* h, const uint8_t* mask, int n_img, int H, int W, int connectivity, int32_t* labels_out) {
    if (h && connectivity != 4 && connectivity != 8) return fail(h, ECSEG_E_INVALID, "connectivity must be 4 or 8");
    if (h && n_img > 0 && !labels_out) return fail(h, ECSEG_E_INVALID, "labels_out is NULL");
    return count_driver(h, mask, nullptr, n_img, H, W, 3, connectivity, nullptr, nullptr, labels_out);
}
// Test-only: one labelling pass alone (run_ccl_pass_debug), uploaded and chunked as count_driver does it, every export brought back.
int ecseg_ccl_pass_debug(ecseg_ctx* h, const uint8_t* key_img, const uint8_t* aux_img, int n_img, int H, int W,
                         const ecseg_ccl_pass_desc* pass, const ecseg_ccl_pass_out* out) {
    if (!h) return ECSEG_E_INVALID;
    drop_sent_ahead(h);
    if (n_img < 0 || H <= 0 || W <= 0 || !pass || (n_img > 0 && (!key_img || !out))) return fail(h, ECSEG_E_INVALID, "ccl_pass_debug: bad arguments");
    if (n_img == 0) return ECSEG_OK;
    if (!out->root || !out->area || !out->sumy || !out->sumx || !out->flag || !out->counters || !out->list1 || !out->list2 || !out->tile_any)
        return fail(h, ECSEG_E_INVALID, "ccl_pass_debug: every output is required");
    if (pass->conn != 4 && pass->conn != 8) return fail(h, ECSEG_E_INVALID, "connectivity must be 4 or 8");
    if (pass->aux_mode == 3 && !aux_img) return fail(h, ECSEG_E_INVALID, "ccl_pass_debug: aux_mode 3 needs aux_img");
    if (pass->n_queries < 0 || pass->n_queries > 5) return fail(h, ECSEG_E_INVALID, "ccl_pass_debug: at most 5 flag queries");
    if ((pass->need & 8) && pass->conn != 8) return fail(h, ECSEG_E_INVALID, "ccl_pass_debug: the root lists are sized for 8-connected components");
    if (pass->n_queries > 0 && pass->count_only) return fail(h, ECSEG_E_INVALID, "ccl_pass_debug: a count_only pass writes no flag words to query");
    if ((long long)H * W >= (1ll << 31)) return fail(h, ECSEG_E_INVALID, "image too large");
    HIP_TRY(h, hipSetDevice(h->device));
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
    for (int i0 = 0; i0 < n_img; i0 += chunk) {
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
int ecseg_count_colocalization(ecseg_ctx* h, const uint8_t* ob1, const uint8_t* ob2, int n_img, int H, int W, int32_t* n_out) {
    if (h && n_img > 0 && !ob2) return fail(h, ECSEG_E_INVALID, "ob2 is NULL");
    return count_driver(h, ob1, ob2, n_img, H, W, 1, 0, n_out, nullptr, nullptr);
}
int ecseg_count_hsr(ecseg_ctx* h, const uint8_t* chrom, const uint8_t* fish, int n_img, int H, int W, int thr, int32_t* n_out) {
    if (h && n_img > 0 && !fish) return fail(h, ECSEG_E_INVALID, "fish is NULL");
    return count_driver(h, chrom, fish, n_img, H, W, 2, thr, n_out, nullptr, nullptr);
}

int ecseg_overlay(ecseg_ctx* h, const uint8_t* labels, const uint8_t* rgb, int n_img, int H, int W, int C, int sens, int hsr_thr,
                  int64_t* out) {
    if (!h) return ECSEG_E_INVALID;
    drop_sent_ahead(h);
    if (n_img < 0 || H <= 0 || W <= 0 || C < 2 || (n_img > 0 && (!labels || !rgb || !out)))
        return fail(h, ECSEG_E_INVALID, "overlay: bad arguments");
    if (n_img == 0) return ECSEG_OK;
    if ((long long)H * W >= (1ll << 31)) return fail(h, ECSEG_E_INVALID, "image too large");
    HIP_TRY(h, hipSetDevice(h->device));
    const size_t px = (size_t)H * W;
    const int chunk = h->post_chunk;
    int rc;
    if ((rc = ensure_post(h, std::min(n_img, chunk), px))) return rc;
    if ((rc = h->d_gray.ensure(h, px * std::min(n_img, chunk)))) return rc;
    if ((rc = h->d_aux8.ensure(h, px * C * std::min(n_img, chunk)))) return rc;
    if ((rc = h->d_i64.ensure(h, (size_t)chunk * 12))) return rc;
    hipStream_t s = h->stream;
    for (float& v : h->stage_ms) v = 0.f;
    for (int i0 = 0; i0 < n_img; i0 += chunk) {
        const int ni = std::min(chunk, n_img - i0);
        HIP_TRY(h, hipMemcpyAsync(h->d_gray, labels + (size_t)i0 * px, px * ni, hipMemcpyHostToDevice, s));
        HIP_TRY(h, hipMemcpyAsync(h->d_aux8, rgb + (size_t)i0 * px * C, px * C * ni, hipMemcpyHostToDevice, s));
        HIP_TRY(h, hipEventRecord(h->ev[0], s));             // the kernels alone (inputs resident): ecseg_get_timings()[ECSEG_T_COUNT]
        HIP_TRY(h, run_overlay(h->ws, h->d_gray, h->d_aux8, ni, H, W, C, sens, hsr_thr, h->d_i64, s));
        HIP_TRY(h, hipEventRecord(h->ev[1], s));
        HIP_TRY(h, hipMemcpyAsync(out + (size_t)i0 * 12, h->d_i64, (size_t)ni * 12 * 8, hipMemcpyDeviceToHost, s));
        HIP_TRY(h, hipStreamSynchronize(s));
        h->stage_ms[ECSEG_T_COUNT] += stage_elapsed(h->ev[0], h->ev[1]);
    }
    return ECSEG_OK;
}

// ---- interSeg driver (src/interseg.py:113-235) ----------------------------------------------------------------------
int ecseg_nuclei_regions(ecseg_ctx* h, const uint8_t* seg, int H, int W, const uint8_t* img, int img_h, int img_w, int C,
                         int channel0, int capacity, int64_t* records, int32_t* n_regions) {
    if (!h) return ECSEG_E_INVALID;
    drop_sent_ahead(h);
    h->iseg_n = -1;
    if (!seg || !img || !n_regions || H <= 0 || W <= 0 || img_h < H || img_w < W || C < 1 || channel0 < 0 || channel0 >= C ||
        capacity < 0 || (capacity > 0 && !records))
        return fail(h, ECSEG_E_INVALID, "nuclei_regions: bad arguments (the segmentation must not be larger than the image)");
    if ((long long)H * W >= (1ll << 31) || (long long)H * img_w * C >= (1ll << 40)) return fail(h, ECSEG_E_INVALID, "image too large");
    HIP_TRY(h, hipSetDevice(h->device));
    const size_t px = (size_t)H * W, img_bytes = (size_t)H * img_w * C;
    int rc;
    RegionBufs b{};
    if ((rc = ensure_post(h, 1, px))) return rc;
    if ((rc = h->d_gray.ensure(h, px))) return rc;
    if ((rc = lay_out(h, h->keep_arena, [&](Carver& c) { h->iseg = region_map_bufs(c, H, W, img_w, C); }))) return rc;
    if ((rc = lay_out(h, h->call_arena, [&](Carver& c) { b = region_bufs(c, H, W, capacity); }))) return rc;
    hipStream_t s = h->stream;
    for (float& v : h->stage_ms) v = 0.f;
    HIP_TRY(h, hipMemcpyAsync(h->d_gray, seg, px, hipMemcpyHostToDevice, s));
    HIP_TRY(h, hipMemcpyAsync(h->iseg.img, img, img_bytes, hipMemcpyHostToDevice, s));   // the first H rows: I[:imheight, :imwidth]
    HIP_TRY(h, hipEventRecord(h->ev[0], s));
    HIP_TRY(h, run_ccl_labels(h->ws, h->d_gray, 1, H, W, 8, h->iseg.lab, s));
    HIP_TRY(h, run_nuclei_regions(h->d_gray, h->iseg.img, H, W, img_w, C, channel0, h->iseg.lab, b, s));
    HIP_TRY(h, hipEventRecord(h->ev[1], s));
    int32_t misc[4];
    HIP_TRY(h, hipMemcpyAsync(misc, b.misc, sizeof(misc), hipMemcpyDeviceToHost, s));
    HIP_TRY(h, hipStreamSynchronize(s));
    h->stage_ms[ECSEG_T_COUNT] = stage_elapsed(h->ev[0], h->ev[1]);
    const int n = misc[0], vmax = misc[1], vmin = 255 - misc[2];
    if (n > 0 && vmin != vmax)
        return fail(h, ECSEG_E_INVALID, "segmentation holds the non-zero values " + std::to_string(vmin) + " .. " + std::to_string(vmax) +
                                            ": only 0 / non-zero nucleus masks are supported, not instance-id maps");
    *n_regions = n;
    if (n <= capacity && n > 0) {
        HIP_TRY(h, hipMemcpyAsync(records, b.rec, (size_t)n * 8 * sizeof(int64_t), hipMemcpyDeviceToHost, s));
        HIP_TRY(h, hipStreamSynchronize(s));
    }
    h->iseg_H = H; h->iseg_W = W; h->iseg_img_w = img_w; h->iseg_C = C; h->iseg_n = n;
    return ECSEG_OK;
}

int ecseg_nucleus_crops(ecseg_ctx* h, const int32_t* crops, int n_crops, const int32_t* channel_order, uint8_t* out,
                        int32_t* channel_max) {
    if (!h) return ECSEG_E_INVALID;
    drop_sent_ahead(h);
    if (n_crops < 0 || (n_crops > 0 && (!crops || !channel_order || !out || !channel_max)))
        return fail(h, ECSEG_E_INVALID, "nucleus_crops: bad arguments");
    if (n_crops == 0) return ECSEG_OK;
    if (h->iseg_n < 0) return fail(h, ECSEG_E_INVALID, "nucleus_crops: no region map on the handle (call ecseg_nuclei_regions first)");
    int order[3];
    for (int c = 0; c < 3; ++c) {
        order[c] = channel_order[c];
        if (order[c] < 0 || order[c] >= h->iseg_C) return fail(h, ECSEG_E_INVALID, "nucleus_crops: channel_order out of range");
    }
    for (int k = 0; k < n_crops; ++k) {
        const int32_t* d = crops + (size_t)k * 5;
        if (d[0] < 0 || d[0] >= h->iseg_n || d[1] < 0 || d[2] < 0 || d[3] < 1 || d[3] > 256 || d[4] < 1 || d[4] > 256 ||
            d[1] > h->iseg_H - d[3] || d[2] > h->iseg_W - d[4])
            return fail(h, ECSEG_E_INVALID, "nucleus_crops: crop " + std::to_string(k) + " is not a 1..256 x 1..256 window of a region");
    }
    HIP_TRY(h, hipSetDevice(h->device));
    const int chunk = 256;                                   // 48 MiB of crops per launch
    const size_t crop_bytes = (size_t)256 * 256 * 3;
    const int nc = std::min(n_crops, chunk);
    int rc;
    CropBufs b{};
    if ((rc = lay_out(h, h->call_arena, [&](Carver& c) { b = crop_bufs(c, nc); }))) return rc;
    hipStream_t s = h->stream;
    for (float& v : h->stage_ms) v = 0.f;
    for (int k0 = 0; k0 < n_crops; k0 += chunk) {
        const int k = std::min(chunk, n_crops - k0);
        HIP_TRY(h, hipMemcpyAsync(b.desc, crops + (size_t)k0 * 5, (size_t)k * 5 * sizeof(int32_t), hipMemcpyHostToDevice, s));
        HIP_TRY(h, hipEventRecord(h->ev[0], s));
        HIP_TRY(h, run_nucleus_crops(h->iseg.lab, h->iseg.img, h->iseg_W, h->iseg_img_w, h->iseg_C, b.desc, k, order, b.crops, b.max, s));
        HIP_TRY(h, hipEventRecord(h->ev[1], s));
        HIP_TRY(h, hipMemcpyAsync(out + (size_t)k0 * crop_bytes, b.crops, (size_t)k * crop_bytes, hipMemcpyDeviceToHost, s));
        HIP_TRY(h, hipMemcpyAsync(channel_max + (size_t)k0 * 3, b.max, (size_t)k * 3 * sizeof(int32_t), hipMemcpyDeviceToHost, s));
        HIP_TRY(h, hipStreamSynchronize(s));
        h->stage_ms[ECSEG_T_COUNT] += stage_elapsed(h->ev[0], h->ev[1]);
    }
    return ECSEG_OK;
}

// The opening phase of ecseg_fish_distances and ecseg_fish_spots: the label map and the image on the device, the dense cell index
// (stage_ms[ECSEG_T_COUNT] = its device time) and the number of cells.  `who` prefixes the refusal of a label above H * W.  `b`
// lies in the call arena: what the caller sizes by the cell count goes to the count arena.
static int open_dense_cells(ecseg_ctx* h, const char* who, const int32_t* labels, int H, int W, const uint8_t* img, int C, CellIndexBufs& b,
                            int32_t* n_cells) {
    const size_t px = (size_t)H * W;
    if (int rc = lay_out(h, h->call_arena, [&](Carver& c) { b = cell_index_bufs(c, H, W, C); })) return rc;
    hipStream_t s = h->stream;
    for (float& v : h->stage_ms) v = 0.f;
    HIP_TRY(h, hipMemcpyAsync(b.lab, labels, px * sizeof(int32_t), hipMemcpyHostToDevice, s));
    HIP_TRY(h, hipMemcpyAsync(b.img, img, px * C, hipMemcpyHostToDevice, s));
    HIP_TRY(h, hipEventRecord(h->ev[0], s));
    HIP_TRY(h, run_dense_cells(b.lab, H, W, b, s));
    HIP_TRY(h, hipEventRecord(h->ev[1], s));
    int32_t misc[4];
    HIP_TRY(h, hipMemcpyAsync(misc, b.misc, sizeof(misc), hipMemcpyDeviceToHost, s));
    HIP_TRY(h, hipStreamSynchronize(s));
    h->stage_ms[ECSEG_T_COUNT] = stage_elapsed(h->ev[0], h->ev[1]);
    if (misc[3])
        return fail(h, ECSEG_E_INVALID, std::string(who) + ": the label map holds a label larger than H * W = " + std::to_string(px) +
                                            " (renumber the labels by rank first)");
    *n_cells = misc[0];
    return ECSEG_OK;
}

// ---- fish_distance_calculation (src/fish_distance_calculation.py:16-46) ---------------------------------------------------
int ecseg_fish_distances(ecseg_ctx* h, const int32_t* labels, int H, int W, const uint8_t* lsq, int C, int fish_channel,
                         int centromere_channel, int capacity, int64_t* records, int32_t* n_cells) {
    if (!h) return ECSEG_E_INVALID;
    drop_sent_ahead(h);
    if (n_cells) *n_cells = 0;
    if (!labels || !lsq || !n_cells || H <= 0 || W <= 0 || capacity < 0 || (capacity > 0 && !records))
        return fail(h, ECSEG_E_INVALID, "fish_distances: bad arguments");
    if (C < 2) return fail(h, ECSEG_E_INVALID, "fish_distances: the lsq image needs at least 2 channels (the gate reads channels 0 and 1)");
    if (fish_channel < 0 || fish_channel >= C || centromere_channel < 0 || centromere_channel >= C)
        return fail(h, ECSEG_E_INVALID, "fish_distances: channel out of range (the lsq image has " + std::to_string(C) + " channels)");
    if ((long long)H * W >= (1ll << 31) || (long long)H * W * C >= (1ll << 40))
        return fail(h, ECSEG_E_INVALID, "fish_distances: image too large (H * W must be below 2^31, H * W * C below 2^40)");
    HIP_TRY(h, hipSetDevice(h->device));
    int rc;
    CellIndexBufs cells{};
    if ((rc = open_dense_cells(h, "fish_distances", labels, H, W, lsq, C, cells, n_cells))) return rc;
    const int n = *n_cells;
    if (n == 0 || n > capacity) return ECSEG_OK;             // the cell count alone: the caller comes back with a larger buffer
    // the rest is sized by the number of cells, which is known only now
    FishDistBufs b{};
    if ((rc = lay_out(h, h->count_arena, [&](Carver& c) { b = fishdist_bufs(c, cells, H, W, n, fishdist_slices(n)); }))) return rc;
    hipStream_t s = h->stream;
    HIP_TRY(h, hipEventRecord(h->ev[2], s));
    HIP_TRY(h, run_fishdist_records(cells.lab, cells.img, H, W, C, fish_channel, centromere_channel, n, b, s));
    HIP_TRY(h, hipEventRecord(h->ev[3], s));
    HIP_TRY(h, hipMemcpyAsync(records, b.rec, (size_t)n * 8 * sizeof(int64_t), hipMemcpyDeviceToHost, s));
    HIP_TRY(h, hipStreamSynchronize(s));
    h->stage_ms[ECSEG_T_COUNT] += stage_elapsed(h->ev[2], h->ev[3]);
    return ECSEG_OK;
}

// ---- stat_fish behind nuclei_segment (src/stat_fish.py:73-107,134-142,226-300) --------------------------------------------------
int ecseg_fish_spots(ecseg_ctx* h, const int32_t* labels, int H, int W, const uint8_t* img, int C, const int32_t* probe_channels,
                     int n_probe, const double* weights, int K, double normal_threshold, const double* intensity_thresholds,
                     int min_cc_size, int line_thickness, int capacity, uint8_t* thresholded, uint8_t* boundaries,
                     int64_t* records, int32_t* n_cells) {
    if (!h) return ECSEG_E_INVALID;
    drop_sent_ahead(h);
    if (n_cells) *n_cells = 0;
    if (!labels || !img || !probe_channels || !weights || !intensity_thresholds || !thresholded || !boundaries || !n_cells || H <= 0 ||
        W <= 0 || C < 1 || capacity < 0 || (capacity > 0 && !records))
        return fail(h, ECSEG_E_INVALID, "fish_spots: bad arguments");
    if (n_probe < 1 || n_probe > 3) return fail(h, ECSEG_E_INVALID, "fish_spots: n_probe must be 1, 2 or 3");
    int ch[3] = {0, 0, 0};
    double ithr[3] = {0.0, 0.0, 0.0};
    for (int j = 0; j < n_probe; ++j) {
        ch[j] = probe_channels[j];
        ithr[j] = intensity_thresholds[j];
        if (ch[j] < 0 || ch[j] >= C)
            return fail(h, ECSEG_E_INVALID, "fish_spots: probe channel out of range (the image has " + std::to_string(C) + " channels)");
    }
    if (K < 1 || K > ECSEG_FISH_SPOT_MAX_KERNEL || K % 2 == 0)
        return fail(h, ECSEG_E_INVALID, "fish_spots: the kernel side must be odd and between 1 and " + std::to_string(ECSEG_FISH_SPOT_MAX_KERNEL));
    if (line_thickness < 1 || line_thickness > ECSEG_FISH_SPOT_MAX_LINE)
        return fail(h, ECSEG_E_INVALID, "fish_spots: line_thickness must be between 1 and " + std::to_string(ECSEG_FISH_SPOT_MAX_LINE));
    if ((long long)H * W >= (1ll << 31) || (long long)H * W * C >= (1ll << 40))
        return fail(h, ECSEG_E_INVALID, "fish_spots: image too large (H * W must be below 2^31, H * W * C below 2^40)");
    HIP_TRY(h, hipSetDevice(h->device));
    const size_t px = (size_t)H * W, np = (size_t)n_probe;
    int rc;
    CellIndexBufs cells{};
    if ((rc = open_dense_cells(h, "fish_spots", labels, H, W, img, C, cells, n_cells))) return rc;
    const int n = *n_cells;
    if (n > capacity) return ECSEG_OK;                       // the cell count alone: the caller comes back with a larger buffer
    if (n == 0) {                                            // no cell: nothing is thresholded and no rank differs from 0
        std::fill(thresholded, thresholded + px * np, (uint8_t)0);
        std::fill(boundaries, boundaries + px, (uint8_t)0);
        return ECSEG_OK;
    }
    FishSpotBufs b{};
    if ((rc = lay_out(h, h->count_arena, [&](Carver& c) { b = fishspot_bufs(c, cells, H, W, n_probe, K, n); }))) return rc;
    hipStream_t s = h->stream;
    HIP_TRY(h, hipMemcpyAsync(b.w, weights, (size_t)K * K * sizeof(double), hipMemcpyHostToDevice, s));
    HIP_TRY(h, hipEventRecord(h->ev[2], s));
    HIP_TRY(h, run_fishspot(cells.lab, cells.img, H, W, C, n_probe, ch, b.w, K, normal_threshold, ithr, min_cc_size, line_thickness, n, b, s));
    HIP_TRY(h, hipEventRecord(h->ev[3], s));
    HIP_TRY(h, hipMemcpyAsync(thresholded, b.thr, px * np, hipMemcpyDeviceToHost, s));
    HIP_TRY(h, hipMemcpyAsync(boundaries, b.bnd, px, hipMemcpyDeviceToHost, s));
    HIP_TRY(h, hipMemcpyAsync(records, b.rec, (size_t)n * ECSEG_FISH_SPOT_INT64 * sizeof(int64_t), hipMemcpyDeviceToHost, s));
    HIP_TRY(h, hipStreamSynchronize(s));
    h->stage_ms[ECSEG_T_COUNT] += stage_elapsed(h->ev[2], h->ev[3]);
    return ECSEG_OK;
}

// ---- stat_fish's three colour files (src/stat_fish.py:110-115,295-300) ------------------------------------------------------------
// the argument rules the two entry points share; ch: the validated channel indices
static int fish_render_check(ecseg_ctx* h, const uint8_t* img, int H, int W, int C, const int32_t* channels, const uint8_t* thresholded,
                             int n_probe, const uint8_t* boundaries, int ch[4]) {
    if (!img || !channels || !thresholded || !boundaries || H <= 0 || W <= 0) return fail(h, ECSEG_E_INVALID, "fish_render: bad arguments");
    if (C < 3 || C > 4) return fail(h, ECSEG_E_INVALID, "fish_render: the image must have 3 or 4 channels, not " + std::to_string(C));
    if (n_probe != C - 1)
        return fail(h, ECSEG_E_INVALID, "fish_render: n_probe must be C - 1 = " + std::to_string(C - 1) + " (one mask per FISH channel)");
    for (int j = 0; j < 4; ++j) ch[j] = 0;
    for (int j = 0; j < C; ++j) {
        ch[j] = channels[j];
        if (ch[j] < 0 || ch[j] >= C)
            return fail(h, ECSEG_E_INVALID, "fish_render: channel index out of range (the image has " + std::to_string(C) + " channels)");
    }
    if ((long long)H * W >= (1ll << 31)) return fail(h, ECSEG_E_INVALID, "fish_render: image too large (H * W must be below 2^31)");
    return ECSEG_OK;
}

int ecseg_fish_render(ecseg_ctx* h, const uint8_t* img, int H, int W, int C, const int32_t* channels, const uint8_t* thresholded,
                      int n_probe, const uint8_t* boundaries, uint8_t* original, uint8_t* with_segmentation, uint8_t* lsq) {
    if (!h) return ECSEG_E_INVALID;
    drop_sent_ahead(h);
    if (!original || !with_segmentation || !lsq) return fail(h, ECSEG_E_INVALID, "fish_render: bad arguments");
    int ch[4], rc;
    if ((rc = fish_render_check(h, img, H, W, C, channels, thresholded, n_probe, boundaries, ch))) return rc;
    HIP_TRY(h, hipSetDevice(h->device));
    const size_t px = (size_t)H * W;
    FishRenderBufs b{};
    if ((rc = lay_out(h, h->call_arena, [&](Carver& c) { b = fish_render_bufs(c, H, W, C); }))) return rc;
    hipStream_t s = h->stream;
    for (float& v : h->stage_ms) v = 0.f;
    HIP_TRY(h, hipMemcpyAsync(b.img, img, px * C, hipMemcpyHostToDevice, s));
    HIP_TRY(h, hipMemcpyAsync(b.thr, thresholded, px * n_probe, hipMemcpyHostToDevice, s));
    HIP_TRY(h, hipMemcpyAsync(b.bnd, boundaries, px, hipMemcpyHostToDevice, s));
    HIP_TRY(h, hipEventRecord(h->ev[0], s));
    HIP_TRY(h, run_fish_render(H, W, C, ch, b, s));
    HIP_TRY(h, hipEventRecord(h->ev[1], s));
    HIP_TRY(h, hipMemcpyAsync(original, b.orig, px * 3, hipMemcpyDeviceToHost, s));
    HIP_TRY(h, hipMemcpyAsync(with_segmentation, b.seg, px * 3, hipMemcpyDeviceToHost, s));
    HIP_TRY(h, hipMemcpyAsync(lsq, b.lsq, px * 3, hipMemcpyDeviceToHost, s));
    HIP_TRY(h, hipStreamSynchronize(s));
    h->stage_ms[ECSEG_T_COUNT] = stage_elapsed(h->ev[0], h->ev[1]);
    return ECSEG_OK;
}

// ---- TIFF files encoded on the device (tiff_kernels.hip; the host writer is tiff_write_u8, host_io.cpp) -----------------------------
static bool tiff_args_ok(int H, int W, int spp) {            // what tiff_write_u8 accepts
    return H > 0 && W > 0 && (spp == 1 || spp == 3) && (long long)W * spp < (1ll << 30);
}

long long ecseg_tiff_encode_bound(int H, int W, int spp) {
    if (!tiff_args_ok(H, W, spp)) return -1;
    const int rps = tiff_rows_per_strip(H, W, spp), nstrips = (H + rps - 1) / rps;
    return (long long)(8 + (size_t)nstrips * (tiff_strip_bound((size_t)rps * W * spp) + 1) + tiff_tail_bound(nstrips, spp));
}

int ecseg_tiff_encode(ecseg_ctx* h, const uint8_t* img, int H, int W, int spp, int invert, uint8_t* out, long long out_cap, long long* out_bytes) {
    if (!h) return ECSEG_E_INVALID;
    drop_sent_ahead(h);
    if (!img || !out || !out_bytes || out_cap < 0 || !tiff_args_ok(H, W, spp)) return fail(h, ECSEG_E_INVALID, "tiff_encode: bad arguments");
    *out_bytes = 0;
    const int rps = tiff_rows_per_strip(H, W, spp);
    if ((H + rps - 1) / rps >= (1 << 26)) return fail(h, ECSEG_E_INVALID, "tiff_encode: 2^26 strips or more (such a file would pass 4 GiB)");
    HIP_TRY(h, hipSetDevice(h->device));
    int rc;
    TiffEncodeBufs b{};
    if ((rc = lay_out(h, h->call_arena, [&](Carver& c) { b = tiff_encode_bufs(c, H, W, spp, 1, true); }))) return rc;
    hipStream_t s = h->stream;
    for (float& v : h->stage_ms) v = 0.f;
    HIP_TRY(h, hipMemcpyAsync(b.img, img, (size_t)H * W * spp, hipMemcpyHostToDevice, s));
    HIP_TRY(h, hipEventRecord(h->ev[0], s));
    HIP_TRY(h, run_tiff_encode(TiffSources{{b.img, nullptr, nullptr}, 0}, 1, H, W, spp, invert, b, s));
    HIP_TRY(h, hipEventRecord(h->ev[1], s));
    if ((rc = tiff_collect(h, "tiff_encode", 1, H, W, spp, b, &out, out_cap, out_bytes, true))) return rc;
    h->stage_ms[ECSEG_T_COUNT] = stage_elapsed(h->ev[0], h->ev[1]);
    return ECSEG_OK;
}

int ecseg_fish_render_tiff(ecseg_ctx* h, const uint8_t* img, int H, int W, int C, const int32_t* channels, const uint8_t* thresholded,
                           int n_probe, const uint8_t* boundaries, uint8_t* const* files, long long file_cap, long long* file_bytes,
                           uint8_t* original, uint8_t* with_segmentation, uint8_t* lsq) {
    if (!h) return ECSEG_E_INVALID;
    drop_sent_ahead(h);
    if (!files || !files[0] || !files[1] || !files[2] || !file_bytes || file_cap < 0) return fail(h, ECSEG_E_INVALID, "fish_render_tiff: bad arguments");
    int ch[4], rc;
    if ((rc = fish_render_check(h, img, H, W, C, channels, thresholded, n_probe, boundaries, ch))) return rc;
    if (!tiff_args_ok(H, W, 3)) return fail(h, ECSEG_E_INVALID, "fish_render_tiff: the TIFF writer takes lines below 2^30 bytes");
    file_bytes[0] = file_bytes[1] = file_bytes[2] = 0;
    HIP_TRY(h, hipSetDevice(h->device));
    const size_t px = (size_t)H * W;
    FishRenderBufs b{};
    TiffEncodeBufs t{};
    if ((rc = lay_out(h, h->call_arena, [&](Carver& c) { b = fish_render_bufs(c, H, W, C); t = tiff_encode_bufs(c, H, W, 3, 3, false); }))) return rc;
    hipStream_t s = h->stream;
    for (float& v : h->stage_ms) v = 0.f;
    HIP_TRY(h, hipMemcpyAsync(b.img, img, px * C, hipMemcpyHostToDevice, s));
    HIP_TRY(h, hipMemcpyAsync(b.thr, thresholded, px * n_probe, hipMemcpyHostToDevice, s));
    HIP_TRY(h, hipMemcpyAsync(b.bnd, boundaries, px, hipMemcpyHostToDevice, s));
    HIP_TRY(h, hipEventRecord(h->ev[0], s));
    HIP_TRY(h, run_fish_render(H, W, C, ch, b, s));
    HIP_TRY(h, run_tiff_encode(TiffSources{{b.orig, b.seg, b.lsq}, 0}, 3, H, W, 3, 0, t, s));
    HIP_TRY(h, hipEventRecord(h->ev[1], s));
    if (original) HIP_TRY(h, hipMemcpyAsync(original, b.orig, px * 3, hipMemcpyDeviceToHost, s));
    if (with_segmentation) HIP_TRY(h, hipMemcpyAsync(with_segmentation, b.seg, px * 3, hipMemcpyDeviceToHost, s));
    if (lsq) HIP_TRY(h, hipMemcpyAsync(lsq, b.lsq, px * 3, hipMemcpyDeviceToHost, s));
    if ((rc = tiff_collect(h, "fish_render_tiff", 3, H, W, 3, t, files, file_cap, file_bytes, true))) return rc;
    h->stage_ms[ECSEG_T_COUNT] = stage_elapsed(h->ev[0], h->ev[1]);
    return ECSEG_OK;
}

// ---- TIFF files decoded on the device (tiff_decode_kernels.hip; the host reader is ecseg_tiff_read, host_io.cpp) -------------------
int ecseg_tiff_decode_routes(const uint8_t* file, long long n_bytes) {
    TiffInfo t;
    return file && n_bytes >= 0 && parse_tiff(file, (size_t)n_bytes, &t) == ECSEG_OK && tiff_goes_to_device(t) ? 1 : 0;
}

// The strips of a parsed file that is to be decoded lie in the file: ECSEG_OK, or ECSEG_E_INVALID and which one does not.
static int tiff_strips_in_file(const TiffInfo& t, size_t n, std::string& why) {
    const size_t nstrips = ((size_t)t.H + t.rps - 1) / t.rps, n_table = std::min(t.off.size(), nstrips);
    for (size_t k = 0; k < n_table; ++k)
        if (t.off[k] > n) { why = "strip " + std::to_string(k) + " starts behind the end of the file"; return ECSEG_E_INVALID; }
    return ECSEG_OK;
}

// What ecseg_tiff_decode makes of a file before any device work, for itself and for every file of a batch: the tags in t, *parsed
// (the file has a shape), and ECSEG_OK or the status with its reason.  with_strips: the file is to be decoded, not only measured.
static int tiff_decode_verdict(const uint8_t* file, size_t n, bool with_strips, TiffInfo& t, bool* parsed, std::string& why) {
    t = TiffInfo();
    int rc = parse_tiff(file, n, &t);
    *parsed = rc == ECSEG_OK;
    if (rc != ECSEG_OK) {
        why = rc == ECSEG_E_UNSUPPORTED ? "a layout the native readers leave to the Python reader" : "not a TIFF file, or a corrupt one";
        return rc;
    }
    const unsigned long long bpp = t.bits / 8, line = (unsigned long long)t.W * t.spp * bpp, total = line * t.H;
    if (t.comp != 1 && t.comp != 5) { why = "Deflate strips are decoded by the host reader"; return ECSEG_E_UNSUPPORTED; }
    if ((unsigned long long)t.rps * line >= (1ull << 31) || total >= (1ull << 40)) {
        why = "strips of 2 GiB or more, or an image of 1 TiB or more";
        return ECSEG_E_UNSUPPORTED;
    }
    return with_strips ? tiff_strips_in_file(t, n, why) : ECSEG_OK;
}

int ecseg_tiff_decode(ecseg_ctx* h, const uint8_t* file, long long n_bytes, void* dst, long long dst_bytes, int* H, int* W, int* samples_per_pixel,
                      int* bits_per_sample) {
    if (!h) return ECSEG_E_INVALID;
    drop_sent_ahead(h);
    if (!file || n_bytes < 0 || !H || !W || !samples_per_pixel || !bits_per_sample || (dst && dst_bytes < 0))
        return fail(h, ECSEG_E_INVALID, "tiff_decode: bad arguments");
    for (float& v : h->stage_ms) v = 0.f;
    TiffInfo t;
    std::string why;
    const size_t n = (size_t)n_bytes;
    bool parsed = false;
    int rc = tiff_decode_verdict(file, n, false, t, &parsed, why);
    if (parsed) { *H = (int)t.H; *W = (int)t.W; *samples_per_pixel = (int)t.spp; *bits_per_sample = (int)t.bits; }
    if (rc != ECSEG_OK) return fail(h, rc, "tiff_decode: " + why);
    const unsigned long long bpp = t.bits / 8, line = (unsigned long long)t.W * t.spp * bpp, total = line * t.H;
    if (!dst) return ECSEG_OK;
    if ((unsigned long long)dst_bytes < total) return fail(h, ECSEG_E_INVALID, "tiff_decode: the destination holds fewer bytes than the image");
    if ((rc = tiff_strips_in_file(t, n, why)) != ECSEG_OK) return fail(h, rc, "tiff_decode: " + why);
    const size_t nstrips = ((size_t)t.H + t.rps - 1) / t.rps, n_table = std::min(t.off.size(), nstrips);
    HIP_TRY(h, hipSetDevice(h->device));
    TiffDecodeBufs b{};
    if ((rc = lay_out(h, h->call_arena, [&](Carver& c) { b = tiff_decode_bufs(c, n, (int)n_table, (size_t)total, (int)nstrips); }))) return rc;
    hipStream_t s = h->stream;
    HIP_TRY(h, hipMemcpyAsync(b.file, file, n, hipMemcpyHostToDevice, s));
    HIP_TRY(h, hipMemcpyAsync(b.offs, t.off.data(), n_table * sizeof(uint32_t), hipMemcpyHostToDevice, s));
    HIP_TRY(h, hipMemcpyAsync(b.cnts, t.cnt.data(), n_table * sizeof(uint32_t), hipMemcpyHostToDevice, s));
    HIP_TRY(h, hipEventRecord(h->ev[0], s));
    HIP_TRY(h, run_tiff_decode(b, (unsigned long long)n, (int)t.H, (int)t.W, (int)t.spp, (int)bpp, (int)t.rps, t.comp == 5, bpp == 2 && !t.le, t.pred == 2, s));
    HIP_TRY(h, hipEventRecord(h->ev[1], s));
    std::vector<uint32_t> status(nstrips);
    HIP_TRY(h, hipMemcpyAsync(status.data(), b.status, nstrips * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    HIP_TRY(h, hipStreamSynchronize(s));
    h->stage_ms[ECSEG_T_COUNT] = stage_elapsed(h->ev[0], h->ev[1]);
    for (size_t k = 0; k < nstrips; ++k)
        if (status[k]) return fail(h, ECSEG_E_INVALID, "tiff_decode: strip " + std::to_string(k) + " holds a corrupt LZW stream");
    HIP_TRY(h, hipMemcpyAsync(dst, b.raster, (size_t)total, hipMemcpyDeviceToHost, s));
    HIP_TRY(h, hipStreamSynchronize(s));
    return ECSEG_OK;
}

// ---- the same over a batch of files: every strip of every file is a wave of one launch ----------------------------------------------
// The files of a batch as ecseg_tiff_decode judges each alone: info[i] and status[i] (with_strips as there), and the rows of the
// layout for the files that are ECSEG_OK (dst_offsets may be null: the rasters back to back, 16-bit ones on even offsets).  Empty
// string, or which argument is wrong.
static std::string tiff_batch_plan(const uint8_t* files, long long files_bytes, const int64_t* ranges, int n_files, const int64_t* dst_offsets,
                                   bool with_strips, std::vector<TiffInfo>& info, std::vector<int>& status, std::vector<TdFileIn>& in) {
    info.assign((size_t)n_files, TiffInfo()); status.assign((size_t)n_files, ECSEG_OK); in.assign((size_t)n_files, TdFileIn());
    long long end = 0;
    for (int i = 0; i < n_files; ++i) {                      // the geometry first: nothing is read through a bad range
        const long long off = ranges[2 * (size_t)i], nb = ranges[2 * (size_t)i + 1];
        if (nb < 0 || off < end || off > files_bytes || nb > files_bytes - off)
            return "file " + std::to_string(i) + ": its range overlaps the one in front or leaves the " + std::to_string(files_bytes) + " bytes of files";
        end = off + nb;
    }
    unsigned long long packed = 0;
    std::string why;
    for (int i = 0; i < n_files; ++i) {
        const size_t off = (size_t)ranges[2 * (size_t)i], nb = (size_t)ranges[2 * (size_t)i + 1];
        TiffInfo& t = info[(size_t)i];
        bool parsed = false;
        status[(size_t)i] = tiff_decode_verdict(files + off, nb, with_strips, t, &parsed, why);
        if (!parsed) t.H = t.W = 0;                          // (no shape to report)
        if (status[(size_t)i] != ECSEG_OK) continue;
        TdFileIn& f = in[(size_t)i];
        const size_t nstrips = ((size_t)t.H + t.rps - 1) / t.rps;
        f.in_batch = true; f.src_off = off; f.n_bytes = nb;
        f.n_table = (uint32_t)std::min(t.off.size(), nstrips); f.H = t.H; f.W = t.W; f.spp = t.spp; f.bps = t.bits / 8; f.rps = t.rps;
        f.lzw = t.comp == 5; f.swap = f.bps == 2 && !t.le; f.predictor = t.pred == 2;
        if (dst_offsets) {
            if (dst_offsets[i] < 0) return "file " + std::to_string(i) + ": a negative destination offset";
            f.dst_off = (uint64_t)dst_offsets[i];
        } else {
            packed += packed & (f.bps - 1);
            f.dst_off = packed;
            packed += (unsigned long long)f.W * f.spp * f.bps * f.H;
        }
    }
    return std::string();
}

int ecseg_tiff_decode_batch_counts(const uint8_t* file, long long n_bytes) {
    TiffInfo t;
    std::string why;
    bool parsed = false;
    return file && n_bytes >= 0 && tiff_decode_verdict(file, (size_t)n_bytes, true, t, &parsed, why) == ECSEG_OK && tiff_batch_counts(t) ? 1 : 0;
}

int ecseg_tiff_decode_batch_routes(const uint8_t* files, long long files_bytes, const int64_t* file_ranges, int n_files) {
    if (n_files <= 0 || !files || !file_ranges || files_bytes < 0) return 0;
    std::vector<TiffInfo> info; std::vector<int> status; std::vector<TdFileIn> in;
    if (!tiff_batch_plan(files, files_bytes, file_ranges, n_files, nullptr, true, info, status, in).empty()) return 0;
    std::vector<const TiffInfo*> ok;
    for (int i = 0; i < n_files; ++i) if (status[(size_t)i] == ECSEG_OK) ok.push_back(&info[(size_t)i]);
    return tiff_batch_goes_to_device(ok.data(), ok.size()) ? 1 : 0;
}

long long ecseg_tiff_decode_batch_bytes(const uint8_t* files, long long files_bytes, const int64_t* file_ranges, int n_files) {
    if (n_files == 0) return 0;
    if (n_files < 0 || !files || !file_ranges || files_bytes < 0) return -1;
    std::vector<TiffInfo> info; std::vector<int> status; std::vector<TdFileIn> in;
    if (!tiff_batch_plan(files, files_bytes, file_ranges, n_files, nullptr, true, info, status, in).empty()) return -1;
    TdBatchLayout L;
    if (!td_batch_layout(in, L).empty()) return -1;
    Carver c;
    (void)tiff_decode_batch_bufs(c, L);
    return (long long)c.used;
}

int ecseg_tiff_decode_batch(ecseg_ctx* h, const uint8_t* files, long long files_bytes, const int64_t* file_ranges, int n_files, void* dst,
                            long long dst_bytes, const int64_t* dst_offsets, int32_t* shapes, int32_t* status) {
    if (!h) return ECSEG_E_INVALID;
    drop_sent_ahead(h);
    const std::string me = "tiff_decode_batch: ";
    if (n_files < 0 || files_bytes < 0 || (n_files > 0 && (!files || !file_ranges || !shapes || !status)) ||
        (dst && (dst_bytes < 0 || (n_files > 0 && !dst_offsets))))
        return fail(h, ECSEG_E_INVALID, me + "bad arguments");
    for (float& v : h->stage_ms) v = 0.f;
    if (n_files == 0) return ECSEG_OK;
    const size_t nf = (size_t)n_files;
    std::vector<TiffInfo> info; std::vector<int> verdict; std::vector<TdFileIn> in;
    std::string bad = tiff_batch_plan(files, files_bytes, file_ranges, n_files, dst ? dst_offsets : nullptr, dst != nullptr, info, verdict, in);
    if (!bad.empty()) return fail(h, ECSEG_E_INVALID, me + bad);
    if (dst) {                                               // every raster inside the destination and clear of the others
        std::vector<std::pair<uint64_t, uint64_t>> spans;   // (offset, end) of the files that are decoded
        for (size_t i = 0; i < nf; ++i) {
            if (!in[i].in_batch) continue;
            const uint64_t total = (uint64_t)in[i].W * in[i].spp * in[i].bps * in[i].H;
            if (in[i].dst_off > (uint64_t)dst_bytes || total > (uint64_t)dst_bytes - in[i].dst_off)
                return fail(h, ECSEG_E_INVALID, me + "file " + std::to_string(i) + ": its raster leaves the " + std::to_string(dst_bytes) + " bytes of the destination");
            spans.emplace_back(in[i].dst_off, in[i].dst_off + total);
        }
        std::sort(spans.begin(), spans.end());
        for (size_t k = 1; k < spans.size(); ++k)
            if (spans[k].first < spans[k - 1].second) return fail(h, ECSEG_E_INVALID, me + "two rasters overlap in the destination");
    }
    TdBatchLayout L;
    if (dst && !(bad = td_batch_layout(in, L)).empty()) return fail(h, ECSEG_E_INVALID, me + bad);
    for (size_t i = 0; i < nf; ++i) {
        const TiffInfo& t = info[i];
        int32_t* q = shapes + 4 * i;
        q[0] = (int32_t)t.H; q[1] = (int32_t)t.W; q[2] = t.H ? (int32_t)t.spp : 0; q[3] = t.H ? (int32_t)t.bits : 0;
        status[i] = verdict[i];
    }
    if (!dst || L.n_strips == 0) return ECSEG_OK;
    HIP_TRY(h, hipSetDevice(h->device));
    int rc;
    TiffDecodeBatchBufs b{};
    if ((rc = lay_out(h, h->call_arena, [&](Carver& c) { b = tiff_decode_batch_bufs(c, L); }))) return rc;
    std::vector<uint32_t> tables((size_t)L.table_words);
    for (size_t i = 0; i < nf; ++i) {
        const TdFile& f = L.tab[i];
        std::copy(info[i].off.begin(), info[i].off.begin() + f.n_table, tables.begin() + (size_t)f.table_off);
        std::copy(info[i].cnt.begin(), info[i].cnt.begin() + f.n_table, tables.begin() + (size_t)f.table_off + f.n_table);
    }
    hipStream_t s = h->stream;
    HIP_TRY(h, hipMemcpyAsync(b.files, files + L.src_base, (size_t)L.src_span, hipMemcpyHostToDevice, s));
    HIP_TRY(h, hipMemcpyAsync(b.tab, L.tab.data(), nf * sizeof(TdFile), hipMemcpyHostToDevice, s));
    if (!tables.empty()) HIP_TRY(h, hipMemcpyAsync(b.tables, tables.data(), tables.size() * sizeof(uint32_t), hipMemcpyHostToDevice, s));
    HIP_TRY(h, hipEventRecord(h->ev[0], s));
    HIP_TRY(h, run_tiff_decode_batch(b, L, s));
    HIP_TRY(h, hipEventRecord(h->ev[1], s));
    std::vector<uint32_t> corrupt(nf, 0);
    HIP_TRY(h, hipMemcpyAsync(corrupt.data(), b.file_status, nf * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    HIP_TRY(h, hipStreamSynchronize(s));                     // (L.tab and tables are read by the copies above: they live until here)
    h->stage_ms[ECSEG_T_COUNT] = stage_elapsed(h->ev[0], h->ev[1]);
    // the rasters of the clean files, a run without a gap in one copy: all of them at once where the caller packed them
    std::vector<std::pair<uint64_t, uint64_t>> runs;
    for (size_t i = 0; i < nf; ++i) {
        if (!L.tab[i].in_batch) continue;
        if (corrupt[i]) { status[i] = ECSEG_E_INVALID; continue; }
        runs.emplace_back(L.tab[i].raster_off, L.tab[i].raster_off + td_file_raster_bytes(L.tab[i]));
    }
    std::sort(runs.begin(), runs.end());
    for (size_t k = 0; k < runs.size();) {
        size_t e = k + 1;
        uint64_t end = runs[k].second;
        while (e < runs.size() && runs[e].first == end) end = runs[e++].second;
        HIP_TRY(h, hipMemcpyAsync(static_cast<uint8_t*>(dst) + L.dst_base + runs[k].first, b.rasters + runs[k].first, (size_t)(end - runs[k].first),
                                  hipMemcpyDeviceToHost, s));
        k = e;
    }
    HIP_TRY(h, hipStreamSynchronize(s));
    return ECSEG_OK;
}

// ---- label PNG files encoded on the device (png_kernels.hip; the host writer is ecseg_png_write_labels, host_io.cpp) ---------------
int ecseg_png_labels_encode(ecseg_ctx* h, const uint8_t* labels, int n_img, int H, int W, uint8_t* const* files, long long file_cap,
                            long long* file_bytes) {
    if (!h) return ECSEG_E_INVALID;
    drop_sent_ahead(h);
    if (n_img < 0 || n_img >= 65536 || H <= 0 || W <= 0 || W >= (1 << 30) || file_cap < 1 || (n_img > 0 && (!labels || !files || !file_bytes)))
        return fail(h, ECSEG_E_INVALID, "png_labels_encode: bad arguments");
    for (int i = 0; i < n_img; ++i) if (!files[i]) return fail(h, ECSEG_E_INVALID, "png_labels_encode: a null file buffer");
    for (float& v : h->stage_ms) v = 0.f;
    if (n_img == 0) return ECSEG_OK;
    for (int i = 0; i < n_img; ++i) file_bytes[i] = 0;
    HIP_TRY(h, hipSetDevice(h->device));
    int rc;
    PngEncodeBufs b{};
    if ((rc = lay_out(h, h->call_arena, [&](Carver& c) { b = png_encode_bufs(c, H, W, n_img, true); }))) return rc;
    HIP_TRY(h, hipMemcpyAsync(b.labels, labels, (size_t)n_img * H * W, hipMemcpyHostToDevice, h->stream));
    return png_encode_files(h, "png_labels_encode", b.labels, n_img, H, W, b, files, file_cap, file_bytes, &h->stage_ms[ECSEG_T_COUNT]);
}

// ---- the min-cut splitter's max-flow tasks (src/max_flow_binary_mask.py:59-116) ------------------------------------------------
int ecseg_min_cut(ecseg_ctx* h, const uint8_t* masks, long long mask_bytes, const int32_t* tasks, int n_tasks, int dist, uint8_t* side,
                  int32_t* flow) {
    if (!h) return ECSEG_E_INVALID;
    drop_sent_ahead(h);
    if (n_tasks < 0 || mask_bytes < 0 || (n_tasks > 0 && (!masks || !tasks || !side || !flow)))
        return fail(h, ECSEG_E_INVALID, "min_cut: bad arguments");
    if (dist < 1 || dist > ECSEG_MIN_CUT_MAX_DIST)
        return fail(h, ECSEG_E_INVALID, "min_cut: dist must be between 1 and " + std::to_string(ECSEG_MIN_CUT_MAX_DIST));
    if (mask_bytes > ECSEG_MIN_CUT_MAX_BYTES)
        return fail(h, ECSEG_E_INVALID, "min_cut: more than " + std::to_string(ECSEG_MIN_CUT_MAX_BYTES) + " bytes of windows in one call");
    for (float& v : h->stage_ms) v = 0.f;
    if (n_tasks == 0) return ECSEG_OK;
    std::vector<long long> soff((size_t)n_tasks, -1);
    long long end = 0;
    size_t scratch = 0;
    int n_global = 0;
    for (int i = 0; i < n_tasks; ++i) {
        const int32_t* t = tasks + 8 * (size_t)i;
        const std::string who = "min_cut: task " + std::to_string(i);
        const long long off = t[0], th = t[1], tw = t[2];
        if (th < 1 || tw < 1 || th * tw > ECSEG_MIN_CUT_MAX_PIXELS)
            return fail(h, ECSEG_E_INVALID, who + ": the window must hold between 1 and " + std::to_string(ECSEG_MIN_CUT_MAX_PIXELS) + " pixels");
        if (off < end || off + th * tw > mask_bytes)
            return fail(h, ECSEG_E_INVALID, who + ": the window overlaps the one in front or leaves the buffer");
        end = off + th * tw;
        if (t[3] < 0 || t[3] >= th || t[4] < 0 || t[4] >= tw || t[5] < 0 || t[5] >= th || t[6] < 0 || t[6] >= tw)
            return fail(h, ECSEG_E_INVALID, who + ": source or sink outside the window");
        if (t[3] == t[5] && t[4] == t[6]) return fail(h, ECSEG_E_INVALID, who + ": source and sink are the same pixel");
        if (!masks[off + t[3] * tw + t[4]] || !masks[off + t[5] * tw + t[6]])
            return fail(h, ECSEG_E_INVALID, who + ": source or sink on a zero pixel");
        if (th * tw > h->min_cut_lds_pixels) {
            soff[(size_t)i] = (long long)scratch;
            ++n_global;
            scratch += mincut_scratch_bytes((int)th, (int)tw);
        }
    }
    HIP_TRY(h, hipSetDevice(h->device));
    const size_t nb = (size_t)mask_bytes, nt = (size_t)n_tasks;
    int rc;
    MinCutBufs b{};
    if ((rc = lay_out(h, h->call_arena, [&](Carver& c) { b = mincut_bufs(c, nb, n_tasks, scratch); }))) return rc;
    hipStream_t s = h->stream;
    HIP_TRY(h, hipMemcpyAsync(b.mask, masks, nb, hipMemcpyHostToDevice, s));
    HIP_TRY(h, hipMemcpyAsync(b.desc, tasks, nt * 8 * sizeof(int32_t), hipMemcpyHostToDevice, s));
    HIP_TRY(h, hipMemcpyAsync(b.soff, soff.data(), nt * sizeof(long long), hipMemcpyHostToDevice, s));
    HIP_TRY(h, hipMemsetAsync(b.side, 0, nb, s));
    HIP_TRY(h, hipEventRecord(h->ev[0], s));
    HIP_TRY(h, run_mincut(b.mask, b.desc, b.soff, n_tasks, n_global, dist, b.scratch, b.side, b.flow, s));
    HIP_TRY(h, hipEventRecord(h->ev[1], s));
    HIP_TRY(h, hipMemcpyAsync(side, b.side, nb, hipMemcpyDeviceToHost, s));
    HIP_TRY(h, hipMemcpyAsync(flow, b.flow, nt * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    HIP_TRY(h, hipStreamSynchronize(s));                     // (soff is read by the copy above: it lives until here)
    h->stage_ms[ECSEG_T_COUNT] = stage_elapsed(h->ev[0], h->ev[1]);
    return ECSEG_OK;
}

// ---- NuSeT's network stage (src/utils.py:35-103) ---------------------------------------------------------------------------
int ecseg_nuset_forward(ecseg_ctx* h, const float* x, int H, int W, int cls_tensor, int bbox_tensor, uint8_t* mask) {
    if (h) drop_sent_ahead(h);
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
    HIP_TRY(h, hipSetDevice(h->device));
    const size_t px = (size_t)H * W;
    if ((rc = ensure_patches(h, 1))) return rc;
    NusetMaskBufs b{};
    if ((rc = lay_out(h, h->call_arena, [&](Carver& c) { b = nuset_mask_bufs(c, H, W); }))) return rc;
    hipStream_t s = h->stream;
    for (float& v : h->stage_ms) v = 0.f;
    prof_begin(h);
    HIP_TRY(h, hipMemcpyAsync(view_of(h, h->input_tensor).p, x, px * sizeof(float), hipMemcpyHostToDevice, s));
    HIP_TRY(h, hipEventRecord(h->ev[0], s));
    if ((rc = run_plan(h, 1))) return rc;
    HIP_TRY(h, launch_argmax2(view_of(h, h->output_tensor), b.mask, s));
    HIP_TRY(h, hipEventRecord(h->ev[1], s));
    HIP_TRY(h, hipMemcpyAsync(mask, b.mask, px, hipMemcpyDeviceToHost, s));
    HIP_TRY(h, hipStreamSynchronize(s));
    prof_end(h);
    h->stage_ms[ECSEG_T_UNET] = stage_elapsed(h->ev[0], h->ev[1]);
    h->nuset_cls_t = cls_tensor; h->nuset_bbox_t = bbox_tensor;
    return ECSEG_OK;
}

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
    if (post < 1 || stride < 1 || (long long)stride * std::max(fh, fw) >= (1ll << 31))
        return fail(h, ECSEG_E_INVALID, "rpn_proposals: post_nms_top_n and stride must be positive");
    HIP_TRY(h, hipSetDevice(h->device));
    const size_t N = (size_t)fh * fw * A, K = std::min<size_t>((size_t)pre, N), no = std::min<size_t>((size_t)post, K);
    int rc;
    RpnBufs b{};
    if ((rc = lay_out(h, h->call_arena, [&](Carver& c) { b = rpn_bufs(c, fh, fw, A, rpn_sort_len((int)N), pre, post, !d_cls); }))) return rc;
    hipStream_t s = h->stream;
    for (float& v : h->stage_ms) v = 0.f;
    if (!d_cls) {
        const size_t px = (size_t)fh * fw;
        HIP_TRY(h, hipMemcpyAsync(b.cls, cls_host, px * 2 * A * sizeof(float), hipMemcpyHostToDevice, s));
        HIP_TRY(h, hipMemcpyAsync(b.bbox, bbox_host, px * 4 * A * sizeof(float), hipMemcpyHostToDevice, s));
        d_cls = b.cls; cls_cs = 2 * A; d_bbox = b.bbox; bbox_cs = 4 * A;
    }
    HIP_TRY(h, hipMemcpyAsync(b.ref, ref_anchors, (size_t)A * 4 * sizeof(double), hipMemcpyHostToDevice, s));
    HIP_TRY(h, hipEventRecord(h->ev[0], s));
    HIP_TRY(h, run_rpn_proposals(d_cls, cls_cs, d_bbox, bbox_cs, b.ref, fh, fw, A, stride, im_h, im_w, nms_threshold, pre, (int)no, b, s));
    HIP_TRY(h, hipEventRecord(h->ev[1], s));
    int32_t misc[2];
    HIP_TRY(h, hipMemcpyAsync(misc, b.misc, sizeof(misc), hipMemcpyDeviceToHost, s));
    HIP_TRY(h, hipStreamSynchronize(s));                      // (ref_anchors is read by the copy above: it lives until here)
    h->stage_ms[ECSEG_T_COUNT] = stage_elapsed(h->ev[0], h->ev[1]);
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

int ecseg_rpn_proposals(ecseg_ctx* h, const float* cls_score, const float* bbox_pred, int fh, int fw, int A, const double* ref_anchors,
                        int stride, int im_h, int im_w, float nms_threshold, int pre_nms_top_n, int post_nms_top_n, int32_t* n_out,
                        float* scores, float* proposals, int32_t* indices) {
    if (!h) return ECSEG_E_INVALID;
    drop_sent_ahead(h);
    if (!cls_score || !bbox_pred) return fail(h, ECSEG_E_INVALID, "rpn_proposals: bad arguments");
    return rpn_driver(h, nullptr, 0, nullptr, 0, cls_score, bbox_pred, fh, fw, A, ref_anchors, stride, im_h, im_w, nms_threshold,
                      pre_nms_top_n, post_nms_top_n, n_out, scores, proposals, indices);
}

int ecseg_rpn_proposals_last(ecseg_ctx* h, int A, const double* ref_anchors, int stride, int im_h, int im_w, float nms_threshold,
                             int pre_nms_top_n, int post_nms_top_n, int32_t* n_out, float* scores, float* proposals, int32_t* indices) {
    if (h) drop_sent_ahead(h);
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
    if (!h) return ECSEG_E_INVALID;
    drop_sent_ahead(h);
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
    HIP_TRY(h, hipSetDevice(h->device));
    int rc;
    WatershedBufs b{};
    if ((rc = lay_out(h, h->call_arena, [&](Carver& c) { b = watershed_bufs(c, H, W, n, cap); }))) return rc;
    hipStream_t s = h->stream;
    for (float& v : h->stage_ms) v = 0.f;
    HIP_TRY(h, hipMemcpyAsync(b.mask, mask, px, hipMemcpyHostToDevice, s));
    if (n > 0) {
        HIP_TRY(h, hipMemcpyAsync(b.rows, marker_rows, (size_t)n * sizeof(int32_t), hipMemcpyHostToDevice, s));
        HIP_TRY(h, hipMemcpyAsync(b.cols, marker_cols, (size_t)n * sizeof(int32_t), hipMemcpyHostToDevice, s));
        HIP_TRY(h, hipMemcpyAsync(b.labels, marker_labels, (size_t)n * sizeof(int32_t), hipMemcpyHostToDevice, s));
    }
    HIP_TRY(h, hipEventRecord(h->ev[0], s));
    HIP_TRY(h, run_marker_watershed(b.mask, H, W, b.rows, b.cols, b.labels, n, cap, b, s));
    HIP_TRY(h, hipEventRecord(h->ev[1], s));
    int32_t misc[4] = {0, 0, 0, 0};
    HIP_TRY(h, hipMemcpyAsync(out, b.out, px, hipMemcpyDeviceToHost, s));
    HIP_TRY(h, hipMemcpyAsync(misc, b.misc, sizeof(misc), hipMemcpyDeviceToHost, s));
    HIP_TRY(h, hipStreamSynchronize(s));
    h->stage_ms[ECSEG_T_COUNT] = stage_elapsed(h->ev[0], h->ev[1]);
    if (misc[1]) return fail(h, ECSEG_E_HIP, "marker_watershed: the heap overflowed its bound");
    return ECSEG_OK;
}

// ---- the same over a batch of images, one flood wave per image -----------------------------------------------------------------
// What a batch needs, from its table (n x 5: offset, H, W, first marker, markers) and the foreground count of every image: the device
// table with the heap slices laid end to end, the packed bytes up to the end of the last image, the list entries in use, the heap
// elements and the largest image.  Empty string, or what is wrong with image `i`.
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
    if (!h) return ECSEG_E_INVALID;
    drop_sent_ahead(h);
    const std::string me = "marker_watershed_batch: ";
    if (n_images < 0 || n_images > ECSEG_WATERSHED_BATCH_MAX_IMAGES)
        return fail(h, ECSEG_E_INVALID, me + "n_images must be between 0 and " + std::to_string(ECSEG_WATERSHED_BATCH_MAX_IMAGES));
    if (mask_bytes < 0 || n_markers < 0 || n_markers >= (1ll << 31) || (n_images > 0 && (!masks || !images || !out)) ||
        (n_markers > 0 && (!marker_rows || !marker_cols || !marker_labels)))
        return fail(h, ECSEG_E_INVALID, me + "bad arguments");
    for (float& v : h->stage_ms) v = 0.f;
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
    HIP_TRY(h, hipSetDevice(h->device));
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
    HIP_TRY(h, hipEventRecord(h->ev[0], s));
    HIP_TRY(h, run_marker_watershed_batch(n_images, pl.span, pl.max_px, pl.max_w, pl.max_markers, b, s));
    HIP_TRY(h, hipEventRecord(h->ev[1], s));
    std::vector<int32_t> misc(ni * 4, 0);
    HIP_TRY(h, hipMemcpyAsync(out, b.out, pl.span, hipMemcpyDeviceToHost, s));
    HIP_TRY(h, hipMemcpyAsync(misc.data(), b.misc, misc.size() * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    HIP_TRY(h, hipStreamSynchronize(s));                     // (pl.tab and misc are read and written by the copies above: they live until here)
    std::fill(out + pl.span, out + mask_bytes, (uint8_t)0);  // behind the last image
    h->stage_ms[ECSEG_T_COUNT] = stage_elapsed(h->ev[0], h->ev[1]);
    for (int i = 0; i < n_images; ++i)
        if (misc[(size_t)i * 4 + 1]) return fail(h, ECSEG_E_HIP, me + "the heap of image " + std::to_string(i) + " overflowed its bound");
    return ECSEG_OK;
}

// ---- NuSeT's clean-up behind the marker watershed (src/nuset_utils/normalization.py:25-37, src/utils.py:159-162) -----------------
int ecseg_clean_nuclei(ecseg_ctx* h, const uint8_t* mask, int H, int W, int nuclei_size_t, uint8_t* out, uint8_t* cleaned, double* mean_area) {
    if (!h) return ECSEG_E_INVALID;
    drop_sent_ahead(h);
    if (!mask || !out || H <= 0 || W <= 0) return fail(h, ECSEG_E_INVALID, "clean_nuclei: bad arguments");
    if ((long long)H * W >= (1ll << 31)) return fail(h, ECSEG_E_INVALID, "clean_nuclei: the image must hold fewer than 2^31 pixels");
    if (nuclei_size_t < 0) return fail(h, ECSEG_E_INVALID, "clean_nuclei: nuclei_size_T must not be negative");
    HIP_TRY(h, hipSetDevice(h->device));
    const size_t px = (size_t)H * W;
    int rc;
    CleanBufs b{};
    if ((rc = lay_out(h, h->call_arena, [&](Carver& c) { b = clean_bufs(c, H, W); }))) return rc;
    hipStream_t s = h->stream;
    for (float& v : h->stage_ms) v = 0.f;
    HIP_TRY(h, hipMemcpyAsync(b.mask, mask, px, hipMemcpyHostToDevice, s));
    HIP_TRY(h, hipEventRecord(h->ev[0], s));
    HIP_TRY(h, run_clean_nuclei(b.mask, H, W, nuclei_size_t, b, s));
    HIP_TRY(h, hipEventRecord(h->ev[1], s));
    double dbl[2] = {0.0, 0.0};
    HIP_TRY(h, hipMemcpyAsync(out, b.out, px, hipMemcpyDeviceToHost, s));
    if (cleaned) HIP_TRY(h, hipMemcpyAsync(cleaned, b.cleaned, px, hipMemcpyDeviceToHost, s));
    HIP_TRY(h, hipMemcpyAsync(dbl, b.dbl, sizeof(dbl), hipMemcpyDeviceToHost, s));
    HIP_TRY(h, hipStreamSynchronize(s));
    if (mean_area) *mean_area = dbl[0];
    h->stage_ms[ECSEG_T_COUNT] = stage_elapsed(h->ev[0], h->ev[1]);
    return ECSEG_OK;
}

// ---- NuSeT's two rescale calls (src/utils.py:136,157-162) ----------------------------------------------------------------------
int ecseg_rescale_down(ecseg_ctx* h, const uint8_t* img, int H, int W, int out_h, int out_w, const double* wy, int ry, const double* wx,
                       int rx, uint8_t* filtered, double* out) {
    if (!h) return ECSEG_E_INVALID;
    drop_sent_ahead(h);
    if (!img || !out || H <= 0 || W <= 0 || out_h <= 0 || out_w <= 0) return fail(h, ECSEG_E_INVALID, "rescale_down: bad arguments");
    if ((long long)H * W >= (1ll << 31)) return fail(h, ECSEG_E_INVALID, "rescale_down: the image must hold fewer than 2^31 pixels");
    if (out_h > H || out_w > W) return fail(h, ECSEG_E_INVALID, "rescale_down: the output extent exceeds the input's");
    if (ry < 0 || rx < 0 || ry > ECSEG_RESCALE_MAX_RADIUS || rx > ECSEG_RESCALE_MAX_RADIUS)
        return fail(h, ECSEG_E_INVALID, "rescale_down: a filter radius outside 0 .. " + std::to_string(ECSEG_RESCALE_MAX_RADIUS));
    if (ry >= H || rx >= W) return fail(h, ECSEG_E_INVALID, "rescale_down: a filter radius reaches across the whole image");
    if ((ry > 0 && !wy) || (rx > 0 && !wx)) return fail(h, ECSEG_E_INVALID, "rescale_down: no weights for a radius above 0");
    HIP_TRY(h, hipSetDevice(h->device));
    const size_t px = (size_t)H * W, opx = (size_t)out_h * out_w;
    int rc;
    RescaleDownBufs b{};
    if ((rc = lay_out(h, h->call_arena, [&](Carver& c) { b = rescale_down_bufs(c, H, W, out_h, out_w); }))) return rc;
    hipStream_t s = h->stream;
    for (float& v : h->stage_ms) v = 0.f;
    HIP_TRY(h, hipMemcpyAsync(b.img, img, px, hipMemcpyHostToDevice, s));
    if (ry > 0) HIP_TRY(h, hipMemcpyAsync(b.wy, wy, (size_t)(2 * ry + 1) * sizeof(double), hipMemcpyHostToDevice, s));
    if (rx > 0) HIP_TRY(h, hipMemcpyAsync(b.wx, wx, (size_t)(2 * rx + 1) * sizeof(double), hipMemcpyHostToDevice, s));
    HIP_TRY(h, hipEventRecord(h->ev[0], s));
    HIP_TRY(h, run_rescale_down(b.img, H, W, out_h, out_w, b.wy, ry, b.wx, rx, b.tmp, b.filtered, b.v, s));
    HIP_TRY(h, hipEventRecord(h->ev[1], s));
    HIP_TRY(h, hipMemcpyAsync(out, b.v, opx * sizeof(double), hipMemcpyDeviceToHost, s));
    if (filtered) HIP_TRY(h, hipMemcpyAsync(filtered, b.filtered, px, hipMemcpyDeviceToHost, s));
    HIP_TRY(h, hipStreamSynchronize(s));
    h->stage_ms[ECSEG_T_COUNT] = stage_elapsed(h->ev[0], h->ev[1]);
    return ECSEG_OK;
}

int ecseg_rescale_mask_up(ecseg_ctx* h, const uint8_t* cleaned, int H, int W, int out_h, int out_w, int nuclei_size_t, uint8_t* out) {
    if (!h) return ECSEG_E_INVALID;
    drop_sent_ahead(h);
    if (!cleaned || !out || H <= 0 || W <= 0 || out_h <= 0 || out_w <= 0) return fail(h, ECSEG_E_INVALID, "rescale_mask_up: bad arguments");
    if ((long long)out_h * out_w >= (1ll << 31)) return fail(h, ECSEG_E_INVALID, "rescale_mask_up: the output must hold fewer than 2^31 pixels");
    if (nuclei_size_t < 0) return fail(h, ECSEG_E_INVALID, "rescale_mask_up: nuclei_size_T must not be negative");
    if (out_h < H || out_w < W) return fail(h, ECSEG_E_INVALID, "rescale_mask_up: the output extent is below the input's");
    HIP_TRY(h, hipSetDevice(h->device));
    const size_t px = (size_t)H * W, opx = (size_t)out_h * out_w;
    int rc;
    RescaleUpBufs b{};
    if ((rc = lay_out(h, h->call_arena, [&](Carver& c) { b = rescale_up_bufs(c, H, W, out_h, out_w); }))) return rc;
    hipStream_t s = h->stream;
    for (float& v : h->stage_ms) v = 0.f;
    HIP_TRY(h, hipMemcpyAsync(b.cleaned, cleaned, px, hipMemcpyHostToDevice, s));
    HIP_TRY(h, hipEventRecord(h->ev[0], s));
    HIP_TRY(h, run_rescale_mask_up(b.cleaned, H, W, out_h, out_w, nuclei_size_t, b, s));
    HIP_TRY(h, hipEventRecord(h->ev[1], s));
    HIP_TRY(h, hipMemcpyAsync(out, b.out, opx, hipMemcpyDeviceToHost, s));
    HIP_TRY(h, hipStreamSynchronize(s));
    h->stage_ms[ECSEG_T_COUNT] = stage_elapsed(h->ev[0], h->ev[1]);
    return ECSEG_OK;
}

}  // extern "C"
