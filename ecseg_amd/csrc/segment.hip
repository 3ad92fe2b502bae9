// The image pipeline: stitch geometry per image size, the clean-up workspace, segment_dev (tile -> U-Net -> stitch / argmax ->
// meta_inference -> count, group by group) and the entry points around it, ecseg_meta_segment with its send-ahead buffer and
// ecseg_meta_segment_tiffs, whose input files decode on the device into that buffer, included.
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include "ctx.h"

namespace ecseg {

namespace {

// ---- tiling / stitch geometry (reference src/image_tools.py:148-252), computed once per image size ----
std::vector<int> window_starts(int dim) {
    const int cropped = dim - 50, spw = 206;
    std::vector<int> s;
    for (int e = 0; e < cropped / spw; ++e) s.push_back(spw * e);
    if (cropped % spw) s.push_back(cropped - spw);
    return s;
}

}  // namespace

int get_stitch(ecseg_ctx* h, int H, int W, StitchPlan** out) {
    auto key = std::make_pair(H, W);
    auto it = h->stitch.find(key);
    if (it != h->stitch.end()) { *out = &it->second; return ECSEG_OK; }
    if (H < 256 || W < 256) return fail(h, ECSEG_E_INVALID, "image smaller than one 256x256 window");
    if ((long long)H * W >= (1ll << 31)) return fail(h, ECSEG_E_INVALID, "image too large");
    const std::vector<int> Lh = window_starts(H), Lw = window_starts(W);
    std::vector<int32_t> pos;
    for (int w : Lw) for (int hh : Lh) { pos.push_back(hh); pos.push_back(w); }   // meshgrid order: columns outer
    const int n = (int)pos.size() / 2;
    if (n >= 32768) return fail(h, ECSEG_E_INVALID, "too many patches per image");
    const int h_l = Lh.back(), w_l = Lw.back();
    const int Hc = h_l + 256, Wc = w_l + 256;    // == H, W
    std::vector<int32_t> map((size_t)Hc * Wc, -1);
    auto put = [&](int i, int dr0, int dr1, int dc0, int dc1, int sr0, int sc0) {
        for (int r = dr0; r < dr1; ++r)
            for (int c = dc0; c < dc1; ++c)
                map[(size_t)r * Wc + c] = (i << 16) | ((sr0 + r - dr0) << 8) | (sc0 + c - dc0);
    };
    const int o = 25, lo = 25, hi = 231;
    for (int i = 0; i < n; ++i) {
        const int ph = pos[2 * i], pw = pos[2 * i + 1];
        if (ph == 0) {
            if (pw == 0) { put(i, 0, o, 0, o, 0, 0); put(i, lo, hi, 0, o, lo, 0); put(i, 0, o, lo, hi, 0, lo); }
            else { if (pw == w_l) put(i, 0, o, Wc - o, Wc, 0, hi); put(i, 0, o, pw + lo, pw + hi, 0, lo); }
        }
        if (pw == 0 && ph != 0) put(i, ph + lo, ph + hi, 0, o, lo, 0);
        if (ph == h_l) {
            if (pw == w_l) {
                put(i, Hc - o, Hc, Wc - o, Wc, hi, hi);
                put(i, h_l + lo, Hc - o, Wc - o, Wc, lo, hi);
                put(i, Hc - o, Hc, w_l + lo, Wc - o, hi, lo);
            } else {
                if (pw == 0) put(i, Hc - o, Hc, 0, o, hi, 0);
                put(i, Hc - o, Hc, pw + lo, pw + hi, hi, lo);
            }
        }
        if (pw == w_l && pw != h_l) put(i, ph + lo, ph + hi, Wc - o, Wc, lo, hi);   // sic: column start vs h_l (:242)
    }
    for (int i = 0; i < n; ++i) put(i, pos[2 * i] + lo, pos[2 * i] + hi, pos[2 * i + 1] + lo, pos[2 * i + 1] + hi, lo, lo);
    StitchPlan sp;                                           // (owns its device memory: an early return below leaks nothing)
    sp.n_pos = n;
    sp.box.assign((size_t)n * 4, 0);
    for (int i = 0; i < n; ++i) { sp.box[4 * i] = 256; sp.box[4 * i + 1] = -1; sp.box[4 * i + 2] = 256; sp.box[4 * i + 3] = -1; }
    for (int32_t v : map) {
        if (v < 0) continue;
        const int i = v >> 16, y = (v >> 8) & 255, x = v & 255;
        sp.box[4 * i] = std::min(sp.box[4 * i], y); sp.box[4 * i + 1] = std::max(sp.box[4 * i + 1], y);
        sp.box[4 * i + 2] = std::min(sp.box[4 * i + 2], x); sp.box[4 * i + 3] = std::max(sp.box[4 * i + 3], x);
    }
    HIP_TRY(h, hipMalloc(reinterpret_cast<void**>(&sp.pos_dev.p), pos.size() * sizeof(int32_t)));
    HIP_TRY(h, hipMalloc(reinterpret_cast<void**>(&sp.map_dev.p), map.size() * sizeof(int32_t)));
    HIP_TRY(h, hipMemcpy(sp.pos_dev, pos.data(), pos.size() * sizeof(int32_t), hipMemcpyHostToDevice));
    HIP_TRY(h, hipMemcpy(sp.map_dev, map.data(), map.size() * sizeof(int32_t), hipMemcpyHostToDevice));
    auto ins = h->stitch.emplace(key, std::move(sp));
    *out = &ins.first->second;
    return ECSEG_OK;
}

int ensure_post(ecseg_ctx* h, int n_img, size_t px) {
    PostWorkspace& w = h->ws;
    if (n_img <= w.cap_img && px <= w.cap_px && w.L) return ECSEG_OK;
    const int ni = std::max(n_img, w.cap_img);
    const size_t np = std::max(px, w.cap_px);
    const int rc = lay_out(h, h->post_arena, [&](Carver& c) { w = post_workspace(c, ni, np); }, "hipMalloc(post workspace)");
    if (rc) w = PostWorkspace{};
    return rc;
}

namespace {

bool debug_calls() { static const bool on = getenv("ECSEG_DEBUG_CALLS") != nullptr; return on; }

double dbg_now() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

// Wait for everything enqueued on a stream (the long waits: a whole launch group).  "blocking_wait" 1 (default): record an
// event created with hipEventBlockingSync and sleep on it - beside the device's blocking-sync flag (ecseg_create) this also
// keeps the runtime's helper thread off the CPU (0.31 -> 0.13 cores busy per waiting call).
hipError_t wait_stream(ecseg_ctx* h, hipStream_t s) {
    if (!h->blocking_wait) return hipStreamSynchronize(s);
    hipError_t e = hipSuccess;
    if (!h->ev_block && (e = hipEventCreateWithFlags(&h->ev_block, hipEventBlockingSync | hipEventDisableTiming)) != hipSuccess) return e;
    if ((e = hipEventRecord(h->ev_block, s)) != hipSuccess) return e;
    return hipEventSynchronize(h->ev_block);
}

// Device-resident pipeline: gray (n_img, H, W) -> raw labels, post labels, counts.  All pointers are device pointers.
// probs_host (optional): the stitched float32 probabilities of every image, copied out group by group.
int segment_dev(ecseg_ctx* h, const uint8_t* gray, int n_img, int H, int W, uint8_t* raw, uint8_t* post, int32_t* n_ec,
                float* probs_host = nullptr) {
    const double tq00 = dbg_now();
    int rc = check_model(h);
    if (rc) return rc;
    if ((rc = h->d_tie.ensure(h, (size_t)n_img))) return rc;
    const ecseg_tensor_desc& ti = h->tensors[h->input_tensor];
    const ecseg_tensor_desc& to = h->tensors[h->output_tensor];
    if (ti.h != 256 || ti.w != 256 || ti.c != 1 || ti.c_stride != 1)
        return fail(h, ECSEG_E_INVALID, "segment: model input must be (256, 256, 1)");
    if (to.h != 256 || to.w != 256 || to.c != 4)
        return fail(h, ECSEG_E_INVALID, "segment: model output must be (256, 256, 4)");
    StitchPlan* sp = nullptr;
    if ((rc = get_stitch(h, H, W, &sp))) return rc;
    const size_t px = (size_t)H * W;
    hipStream_t s = h->stream, s2 = h->overlap_post ? h->stream2 : h->stream;
    // images per U-Net launch: images_per_group is calibrated for 35-window images (1040 x 1392); larger images have more
    // windows each, so the group shrinks to keep the activation memory (~82 MB per window for a base-64 U-Net) bounded
    const int wpg = windows_per_group(h);
    const int grp = std::max(1, std::min(wpg / 35, std::max(1, wpg / sp->n_pos)));
    if ((rc = ensure_patches(h, std::min(grp, n_img) * sp->n_pos))) return rc;
    if ((rc = ensure_post(h, std::min(n_img, grp), px))) return rc;
    if ((rc = h->d_tie_sh.ensure(h, (size_t)std::min(grp, n_img) * G_SHARDS * G_STRIDE))) return rc;
    if (probs_host && (rc = h->d_sprobs.ensure(h, (size_t)std::min(grp, n_img) * px * 4))) return rc;
    for (float& v : h->stage_ms) v = 0.f;
    prof_begin(h);
    // Per group: tile -> U-Net -> stitch/argmax on the main stream; the group's clean-up + count then runs on the second
    // stream while the main stream already computes the next group's U-Net (MFMA-bound convs and latency-bound
    // integer kernels co-exist well).  6 events per group: tile start, unet start, tail start, tail end, post start/end.
    // events come from a pool owned by the handle (freed in ecseg_destroy): nothing to leak on an early return, and no
    // event creation inside the timed loop
    const size_t ngrp = ((size_t)n_img + grp - 1) / grp;
    while (h->grp_events.size() < 6 * ngrp) {
        hipEvent_t e;
        HIP_TRY(h, hipEventCreate(&e));
        h->grp_events.push_back(e);
    }
    const std::vector<hipEvent_t>& evs = h->grp_events;
    size_t used = 0;
    const double tq0 = dbg_now();
    for (int i0 = 0; i0 < n_img; i0 += grp) {
        const int ni = std::min(grp, n_img - i0);
        const hipEvent_t* e6 = &evs[used];
        used += 6;
        HIP_TRY(h, hipEventRecord(e6[0], s));
        HIP_TRY(h, launch_tile_patches(gray + (size_t)i0 * px, ni, H, W, sp->pos_dev, sp->n_pos,
                                       view_of(h, h->input_tensor).p, s));
        HIP_TRY(h, hipEventRecord(e6[1], s));
        {
            // small batches: 2+ window lanes on their own streams (see run_plan); lane 0 stays on the main stream
            const int nw = ni * sp->n_pos;
            int lanes = h->unet_lanes > 0 ? h->unet_lanes : (nw <= h->lane_auto_windows ? 2 : 1);
            if (h->profile_kernels || !h->lanes_ok) lanes = 1;     // (per-launch events are taken on the main stream)
            if (ni > 1) lanes = std::min(lanes, ni);         // whole images per lane
            lanes = std::max(1, std::min(lanes, std::min(nw, 8)));
            while ((int)h->lane_streams.size() < lanes - 1) {
                hipStream_t ls;
                HIP_TRY(h, hipStreamCreateWithFlags(&ls, hipStreamNonBlocking));
                h->lane_streams.push_back(ls);
            }
            while ((int)h->lane_events.size() < lanes - 1) {     // (its own loop: a failed creation leaves the two lists consistent)
                hipEvent_t le;
                HIP_TRY(h, hipEventCreateWithFlags(&le, hipEventDisableTiming));
                h->lane_events.push_back(le);
            }
            if (lanes == 1) {
                if ((rc = run_plan(h, nw, sp))) return rc;
            } else {
                const int unit = ni > 1 ? sp->n_pos : 1, units = nw / unit;
                std::vector<LaneSpec> specs;
                int u0 = 0;
                for (int l = 0; l < lanes; ++l) {
                    const int u1 = (int)((long long)units * (l + 1) / lanes);
                    hipStream_t ls = l == 0 ? s : h->lane_streams[l - 1];
                    if (l > 0) HIP_TRY(h, hipStreamWaitEvent(ls, e6[1], 0));
                    specs.push_back({u0 * unit, (u1 - u0) * unit, ls});
                    u0 = u1;
                }
                if ((rc = run_plan(h, nw, sp, &specs))) return rc;
                for (int l = 1; l < lanes; ++l) {
                    HIP_TRY(h, hipEventRecord(h->lane_events[l - 1], h->lane_streams[l - 1]));
                    HIP_TRY(h, hipStreamWaitEvent(s, h->lane_events[l - 1], 0));
                }
            }
        }
        HIP_TRY(h, hipEventRecord(e6[2], s));
        const TView pv = view_of(h, h->output_tensor);
        HIP_TRY(h, launch_stitch_argmax(pv.p, pv.cs, sp->map_dev, ni, sp->n_pos, H, W, raw + (size_t)i0 * px, s, h->d_tie + i0, h->d_tie_sh));
        HIP_TRY(h, hipEventRecord(e6[3], s));
        if (probs_host) {                                  // (diagnostic output: outside the stage timers)
            HIP_TRY(h, launch_stitch_probs(pv.p, pv.cs, sp->map_dev, ni, sp->n_pos, H, W, h->d_sprobs, s));
            HIP_TRY(h, hipMemcpyAsync(probs_host + (size_t)i0 * px * 4, h->d_sprobs, (size_t)ni * px * 4 * sizeof(float), hipMemcpyDeviceToHost, s));
        }
        if (s2 != s) HIP_TRY(h, hipStreamWaitEvent(s2, e6[3], 0));
        HIP_TRY(h, hipEventRecord(e6[4], s2));
        if (post != raw)
            HIP_TRY(h, hipMemcpyAsync(post + (size_t)i0 * px, raw + (size_t)i0 * px, px * ni, hipMemcpyDeviceToDevice, s2));
        HIP_TRY(h, run_meta_inference(h->ws, post + (size_t)i0 * px, ni, H, W, n_ec ? n_ec + i0 : nullptr, s2, 1, 6));
        HIP_TRY(h, hipEventRecord(e6[5], s2));
    }
    const double tq1 = dbg_now();
    HIP_TRY(h, wait_stream(h, s));
    if (s2 != s) HIP_TRY(h, wait_stream(h, s2));
    const double tq2 = dbg_now();
    // ECSEG_DEBUG_CALLS: host-side timeline of the call on stderr (a `make metaseg` whose device calls take longer than their
    // kernels: is the host late with the launches, or is the wait long - e.g. a throttled CPU quota - ?)
    if (debug_calls()) fprintf(stderr, "[segment_dev] setup %.2f enqueue %.2f wait %.2f ms\n", tq0 - tq00, tq1 - tq0, tq2 - tq1);
    for (size_t k = 0; k + 5 < used; k += 6) {
        h->stage_ms[ECSEG_T_TILE] += stage_elapsed(evs[k], evs[k + 1]);
        h->stage_ms[ECSEG_T_UNET] += stage_elapsed(evs[k + 1], evs[k + 2]);
        h->stage_ms[ECSEG_T_TAIL] += stage_elapsed(evs[k + 2], evs[k + 3]);
        h->stage_ms[ECSEG_T_POST] += stage_elapsed(evs[k + 4], evs[k + 5]);
    }
    prof_end(h);
    return ECSEG_OK;
}

}  // namespace

}  // namespace ecseg

using namespace ecseg;

extern "C" {

int ecseg_segment_images_dev(ecseg_ctx* h, const uint8_t* gray, int n_img, int H, int W, uint8_t* raw, uint8_t* post, int32_t* n_ec) {
    if (!h) return ECSEG_E_INVALID;
    drop_sent_ahead(h);
    if (n_img < 0 || (n_img > 0 && (!gray || !post))) return fail(h, ECSEG_E_INVALID, "segment: bad arguments");
    if (n_img == 0) return ECSEG_OK;
    HIP_TRY(h, hipSetDevice(h->device));
    const size_t px = (size_t)H * W;
    int rc;
    uint8_t* raw_buf = raw;
    if (!raw_buf) {
        if ((rc = h->d_raw.ensure(h, px * n_img))) return rc;
        raw_buf = h->d_raw;
    }
    return segment_dev(h, gray, n_img, H, W, raw_buf, post, n_ec);
}

int ecseg_segment_images(ecseg_ctx* h, const uint8_t* gray, int n_img, int H, int W, uint8_t* raw, uint8_t* post, int32_t* n_ec) {
    return ecseg_segment_images_ex(h, gray, n_img, H, W, raw, post, n_ec, nullptr, nullptr);
}

int ecseg_segment_images_ex(ecseg_ctx* h, const uint8_t* gray, int n_img, int H, int W, uint8_t* raw, uint8_t* post, int32_t* n_ec,
                            int32_t* tie_risk, float* probs) {
    if (!h) return ECSEG_E_INVALID;
    drop_sent_ahead(h);
    if (n_img < 0 || (n_img > 0 && (!gray || !post))) return fail(h, ECSEG_E_INVALID, "segment: bad arguments");
    if (n_img == 0) return ECSEG_OK;
    int rc = check_model(h);
    if (rc) return rc;
    HIP_TRY(h, hipSetDevice(h->device));
    const size_t px = (size_t)H * W, tot = px * n_img;
    if ((rc = h->d_gray.ensure(h, tot))) return rc;
    if ((rc = h->d_raw.ensure(h, tot))) return rc;
    if ((rc = h->d_post.ensure(h, tot))) return rc;
    if ((rc = h->d_i32.ensure(h, (size_t)n_img))) return rc;
    HIP_TRY(h, hipMemcpyAsync(h->d_gray, gray, tot, hipMemcpyHostToDevice, h->stream));
    if ((rc = segment_dev(h, h->d_gray, n_img, H, W, h->d_raw, h->d_post, h->d_i32, probs))) return rc;
    if (raw) HIP_TRY(h, hipMemcpyAsync(raw, h->d_raw, tot, hipMemcpyDeviceToHost, h->stream));
    if (tie_risk) HIP_TRY(h, hipMemcpyAsync(tie_risk, h->d_tie, (size_t)n_img * 4, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipMemcpyAsync(post, h->d_post, tot, hipMemcpyDeviceToHost, h->stream));
    if (n_ec) HIP_TRY(h, hipMemcpyAsync(n_ec, h->d_i32, (size_t)n_img * 4, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    return ECSEG_OK;
}

int ecseg_preprocess(ecseg_ctx* h, const void* img, int n_img, int H, int W, int C, int bps, uint8_t* gray_out, int32_t* inverted_out) {
    if (!h) return ECSEG_E_INVALID;
    drop_sent_ahead(h);
    if (n_img < 0 || H <= 0 || W <= 0 || (C != 1 && C != 3 && C != 4) || (bps != 1 && bps != 2) || (n_img > 0 && (!img || !gray_out)))
        return fail(h, ECSEG_E_INVALID, "preprocess: bad arguments");
    if (n_img == 0) return ECSEG_OK;
    HIP_TRY(h, hipSetDevice(h->device));
    const size_t px = (size_t)H * W, tot = px * n_img, in_bytes = tot * C * bps;
    int rc;
    if ((rc = h->d_aux8.ensure(h, in_bytes))) return rc;
    if ((rc = h->d_gray.ensure(h, tot))) return rc;
    if ((rc = h->d_i32.ensure(h, (size_t)n_img))) return rc;
    if ((rc = h->d_hist.ensure(h, (size_t)n_img * 256))) return rc;
    hipStream_t s = h->stream;
    HIP_TRY(h, hipMemcpyAsync(h->d_aux8, img, in_bytes, hipMemcpyHostToDevice, s));
    HIP_TRY(h, hipEventRecord(h->ev[0], s));                 // the kernels alone (inputs resident): ecseg_get_timings()[ECSEG_T_COUNT]
    HIP_TRY(h, run_preprocess(h->d_aux8, n_img, H, W, C, bps, h->d_gray, h->d_i32, h->d_hist, s));
    HIP_TRY(h, hipEventRecord(h->ev[1], s));
    HIP_TRY(h, hipMemcpyAsync(gray_out, h->d_gray, tot, hipMemcpyDeviceToHost, s));
    if (inverted_out) HIP_TRY(h, hipMemcpyAsync(inverted_out, h->d_i32, (size_t)n_img * 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(h, hipStreamSynchronize(s));
    for (float& v : h->stage_ms) v = 0.f;
    h->stage_ms[ECSEG_T_COUNT] = stage_elapsed(h->ev[0], h->ev[1]);
    return ECSEG_OK;
}

// meta_segment of a batch in ONE call (src/utils.py:105-124 minus the file I/O, + src/metaseg.py:46): the raw images go up
// once, the pre-processed images never leave the device between meta_preprocess and the U-Net (the two-call sequence
// ecseg_preprocess + ecseg_segment_images_ex downloads them, synchronises and uploads them again), and their copy back
// to the host (dapi/<name> is written from it) travels on the second stream under the U-Net.
// files (ecseg_meta_segment_files): the two file images per image, the dapi strips encoded on the second stream beside the copy
// of gray_out, the label PNGs behind the clean-up
struct MetaFiles { uint8_t* const* dapi; long long dapi_cap; long long* dapi_bytes; uint8_t* const* png; long long png_cap; long long* png_bytes; };
// tiffs (ecseg_meta_segment_tiffs): the input is the files themselves.  Their strips decode on the device straight into the input
// slots (raster i at i * H * W * C * bps of d_aux8, or of d_pre for the call after: ecseg_prefetch_tiffs), and the host never sees a sample.
struct MetaTiffs { const uint8_t* files; long long files_bytes; const int64_t* ranges; int32_t* status; };

// What the host makes of the files of one such call: every file judged as ecseg_tiff_decode judges it alone on this handle (its
// tiff_kinds), a file of another shape than the call's refused, the rest laid out on the slots.  ECSEG_OK, or the
// argument error.
static int tiffs_plan(ecseg_ctx* h, const uint8_t* files, long long files_bytes, const int64_t* ranges, int n, int H, int W, int C, int bps, TiffsPlan& p) {
    const std::string me = "meta_segment_tiffs: ";
    std::vector<TiffInfo> info; std::vector<TdFileIn> in;
    std::string bad = tiff_batch_plan(files, files_bytes, ranges, n, nullptr, true, info, p.verdict, in, h->tiff_kinds);
    if (!bad.empty()) return fail(h, ECSEG_E_INVALID, me + bad);
    const uint64_t slot = (uint64_t)H * W * C * bps;
    for (size_t i = 0; i < (size_t)n; ++i) {
        TdFileIn& f = in[i];
        if (!f.in_batch) continue;
        if (f.H != (uint32_t)H || f.W != (uint32_t)W || f.spp != (uint32_t)C || f.bps != (uint32_t)bps) {     // (a raster of another size must not reach the slots)
            f = TdFileIn();
            p.verdict[i] = ECSEG_E_INVALID;
            continue;
        }
        f.dst_off = i * slot;
    }
    if (!(bad = td_batch_layout(in, p.L)).empty()) return fail(h, ECSEG_E_INVALID, me + bad);
    tiff_plan_tables(info, p);
    return ECSEG_OK;
}

// The stream and the event of what is sent ahead (images or files), made when the first call sends something.
static int ensure_stream_in(ecseg_ctx* h) {
    if (!h->stream_in) HIP_TRY(h, hipStreamCreateWithFlags(&h->stream_in, hipStreamNonBlocking));
    if (!h->ev_pre) HIP_TRY(h, hipEventCreateWithFlags(&h->ev_pre, hipEventDisableTiming));
    return ECSEG_OK;
}

static int meta_segment_run(ecseg_ctx* h, const void* img, int n_img, int H, int W, int C, int bps, uint8_t* gray_out, uint8_t* post,
                            int32_t* n_ec, int32_t* tie_risk, const MetaFiles* files, const MetaTiffs* tiffs = nullptr) {
    int rc = check_model(h);
    if (rc) return rc;
    const size_t px = (size_t)H * W, tot = px * n_img, slot = px * C * bps, in_bytes = tot * C * bps;
    // what was named or sent ahead for the other kind of input is for nobody
    if (tiffs) { h->next_host = nullptr; h->next_bytes = 0; h->pre_host = nullptr; h->pre_bytes = 0; }
    else { h->next_tiffs.files = nullptr; h->pre_tiffs.files = nullptr; }
    TiffsKey me;
    TiffsPlan plan;
    bool ahead = false;                                    // this call's rasters lie decoded in d_pre
    if (tiffs) {
        me.files = tiffs->files; me.bytes = tiffs->files_bytes; me.n = n_img; me.H = H; me.W = W; me.C = C; me.bps = bps;
        me.ranges.assign(tiffs->ranges, tiffs->ranges + 2 * (size_t)n_img);
        me.opts = h->tiff_kinds;                     // (a set decoded ahead under other options is not this call's: withdrawn below)
        if (h->next_tiffs.same_set(me)) h->next_tiffs.files = nullptr;     // (registered for a call that never came: it names THIS call's files)
        ahead = h->pre_tiffs.same(me) && h->d_pre && h->pre_file_status;
        h->pre_tiffs.files = nullptr;                      // (files decoded ahead are for the very next call or for nobody)
        h->read_ms = 0.f;
        if (!ahead && (rc = tiffs_plan(h, tiffs->files, tiffs->files_bytes, tiffs->ranges, n_img, H, W, C, bps, plan))) return rc;
    }
    const TiffsPlan& my_plan = ahead ? h->pre_plan : plan;
    HIP_TRY(h, hipSetDevice(h->device));
    if ((rc = h->d_aux8.ensure(h, in_bytes))) return rc;
    TiffEncodeBufs tb{};
    PngEncodeBufs pb{};
    TiffDecodeBatchBufs db{};
    if ((files || (tiffs && !ahead)) && (rc = lay_out(h, h->call_arena, [&](Carver& c) {
            if (files) { tb = tiff_encode_bufs(c, H, W, 1, n_img, false); pb = png_encode_bufs(c, H, W, n_img, false); }
            if (tiffs && !ahead) db = tiff_decode_batch_bufs(c, plan.L, h->d_aux8);
        })))
        return rc;
    if ((rc = h->d_gray.ensure(h, tot))) return rc;
    if ((rc = h->d_raw.ensure(h, tot))) return rc;
    if ((rc = h->d_post.ensure(h, tot))) return rc;
    if ((rc = h->d_i32.ensure(h, (size_t)2 * n_img))) return rc;       // counts, then the inverted flags
    if ((rc = h->d_hist.ensure(h, (size_t)n_img * 256))) return rc;
    hipStream_t s = h->stream, sc = h->stream2;
    const double t0 = dbg_now();
    std::vector<int> st;                                   // tiffs: the status of every file
    if (!tiffs && h->next_host == img) { h->next_host = nullptr; h->next_bytes = 0; }     // (registered for a call that never came: it names THIS call's images)
    if (tiffs) {
        const uint32_t* d_status = db.file_status;
        if (ahead) {
            // decoded ahead (ecseg_prefetch_tiffs) while the call before this one computed: the two input buffers change places, and
            // the status words the decode left in pre_arena are read here, behind ev_pre
            HIP_TRY(h, hipStreamWaitEvent(s, h->ev_pre, 0));
            h->d_aux8.swap(h->d_pre);
            d_status = h->pre_file_status;
            h->read_ms = h->pre_read_ms;
        } else if ((rc = tiff_batch_launch(h, tiffs->files, plan, db, s, h->ev_read[0], h->ev_read[1]))) {
            return rc;
        }
        std::vector<uint32_t> corrupt((size_t)n_img, 0);
        HIP_TRY(h, hipMemcpyAsync(corrupt.data(), d_status, (size_t)n_img * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
        HIP_TRY(h, hipStreamSynchronize(s));               // (plan and the caller's files are read by the copies above: until here)
        if (!ahead) h->read_ms = stage_elapsed(h->ev_read[0], h->ev_read[1]);
        st = my_plan.verdict;
        for (int i = 0; i < n_img; ++i) {
            if (st[(size_t)i] == ECSEG_OK && corrupt[(size_t)i]) st[(size_t)i] = ECSEG_E_INVALID;
            tiffs->status[i] = st[(size_t)i];
            // an image that did not decode is the all-zero image: nothing an earlier call left in the slot reaches an output
            if (st[(size_t)i] != ECSEG_OK) HIP_TRY(h, hipMemsetAsync(h->d_aux8 + (size_t)i * slot, 0, slot, s));
        }
    } else if (h->pre_host == img && h->pre_bytes == in_bytes && h->d_pre) {
        // these images were sent ahead (ecseg_prefetch_input) while the call before this one computed: the two input buffers
        // change places (the one given up last held the images of the call before, whose pre-processing is long over)
        HIP_TRY(h, hipStreamWaitEvent(s, h->ev_pre, 0));
        h->d_aux8.swap(h->d_pre);
        h->pre_host = nullptr; h->pre_bytes = 0;
    } else {
        h->pre_host = nullptr; h->pre_bytes = 0;           // (images sent ahead are for the very next call or for nobody)
        HIP_TRY(h, hipMemcpyAsync(h->d_aux8, img, in_bytes, hipMemcpyHostToDevice, s));
    }
    const double t1 = dbg_now();
    HIP_TRY(h, run_preprocess(h->d_aux8, n_img, H, W, C, bps, h->d_gray, h->d_i32 + n_img, h->d_hist, s));
    if (gray_out || files) {
        HIP_TRY(h, hipEventRecord(h->ev[2], s));
        HIP_TRY(h, hipStreamWaitEvent(sc, h->ev[2], 0));
    }
    if (files) {                                           // dapi/<name>.tif holds cv2.bitwise_not of the pre-processed image
        HIP_TRY(h, hipEventRecord(h->ev_files[0], sc));
        HIP_TRY(h, run_tiff_encode(TiffSources{{h->d_gray, nullptr, nullptr}, px}, n_img, H, W, 1, 1, tb, sc));
        HIP_TRY(h, hipEventRecord(h->ev_files[1], sc));
    }
    if (gray_out) HIP_TRY(h, hipMemcpyAsync(gray_out, h->d_gray, tot, hipMemcpyDeviceToHost, sc));
    if (h->next_host) {                                    // the next call's images, registered by ecseg_prefetch_input
        const void* nx = h->next_host; const size_t nb = h->next_bytes;
        h->next_host = nullptr; h->next_bytes = 0;
        h->pre_host = nullptr; h->pre_bytes = 0;
        if ((rc = ensure_stream_in(h))) return rc;
        if ((rc = h->d_pre.ensure(h, nb))) return rc;
        HIP_TRY(h, hipMemcpyAsync(h->d_pre, nx, nb, hipMemcpyHostToDevice, h->stream_in));
        HIP_TRY(h, hipEventRecord(h->ev_pre, h->stream_in));
        h->pre_host = nx; h->pre_bytes = nb;
    }
    bool sent_tiffs = false;
    if (tiffs && h->next_tiffs.files) {                    // the next call's files, registered by ecseg_prefetch_tiffs: uploaded and decoded on
        TiffsKey nx;                                       // stream_in into the spare input buffer, under this call's kernels
        std::swap(nx, h->next_tiffs);
        h->next_tiffs.files = nullptr;
        // a set with an argument error is not decoded ahead: the call it was named for reports it
        if (tiffs_plan(h, nx.files, nx.bytes, nx.ranges.data(), nx.n, nx.H, nx.W, nx.C, nx.bps, h->pre_plan) == ECSEG_OK) {
            if ((rc = ensure_stream_in(h))) return rc;
            if ((rc = h->d_pre.ensure(h, (size_t)nx.n * nx.H * nx.W * nx.C * nx.bps))) return rc;
            TiffDecodeBatchBufs ab{};
            if ((rc = lay_out(h, h->pre_arena, [&](Carver& c) { ab = tiff_decode_batch_bufs(c, h->pre_plan.L, h->d_pre); }, "hipMalloc(decode-ahead)"))) return rc;
            if ((rc = tiff_batch_launch(h, nx.files, h->pre_plan, ab, h->stream_in, h->ev_read[2], h->ev_read[3]))) return rc;
            HIP_TRY(h, hipEventRecord(h->ev_pre, h->stream_in));
            h->pre_file_status = ab.file_status;
            nx.opts = h->tiff_kinds;                 // (what pre_plan was made under)
            std::swap(h->pre_tiffs, nx);
            sent_tiffs = true;
        } else {
            h->err.clear();
        }
    }
    const double t2 = dbg_now();
    if ((rc = segment_dev(h, h->d_gray, n_img, H, W, h->d_raw, h->d_post, h->d_i32))) return rc;
    const double t3 = dbg_now();
    HIP_TRY(h, hipMemcpyAsync(post, h->d_post, tot, hipMemcpyDeviceToHost, s));
    if (tie_risk) HIP_TRY(h, hipMemcpyAsync(tie_risk, h->d_tie, (size_t)n_img * 4, hipMemcpyDeviceToHost, s));
    if (n_ec) HIP_TRY(h, hipMemcpyAsync(n_ec, h->d_i32, (size_t)n_img * 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(h, wait_stream(h, s));
    const double t4 = dbg_now();
    HIP_TRY(h, wait_stream(h, sc));
    if (h->pre_host) HIP_TRY(h, wait_stream(h, h->stream_in));     // (long done: the caller's buffer is not read after this call)
    if (sent_tiffs) {                                      // (the same; pre_plan's tables have been copied, the status words stay on the device)
        HIP_TRY(h, wait_stream(h, h->stream_in));
        h->pre_read_ms = stage_elapsed(h->ev_read[2], h->ev_read[3]);
    }
    if (files) {                                           // (both streams are idle: the tables, then the files that fit)
        if ((rc = tiff_collect(h, "meta_segment_files", n_img, H, W, 1, tb, files->dapi, files->dapi_cap, files->dapi_bytes, false))) return rc;
        h->file_ms[0] = stage_elapsed(h->ev_files[0], h->ev_files[1]);
        if ((rc = png_encode_files(h, "meta_segment_files", h->d_post, n_img, H, W, pb, files->png, files->png_cap, files->png_bytes, &h->file_ms[1])))
            return rc;
    }
    for (size_t i = 0; i < st.size(); ++i) {               // a file that did not decode has no count and no files
        if (st[i] == ECSEG_OK) continue;
        if (n_ec) n_ec[i] = -1;
        if (files) files->dapi_bytes[i] = files->png_bytes[i] = 0;
    }
    const double t5 = dbg_now();
    if (debug_calls()) fprintf(stderr, "[meta_segment n=%d] upload enqueue %.2f preprocess + gray copy enqueue %.2f segment_dev %.2f (stage timers %.2f) labels down %.2f gray wait %.2f total %.2f ms\n",
                     n_img, t1 - t0, t2 - t1, t3 - t2, h->stage_ms[0] + h->stage_ms[1] + h->stage_ms[2] + h->stage_ms[3], t4 - t3, t5 - t4, t5 - t0);
    return ECSEG_OK;
}

int ecseg_meta_segment(ecseg_ctx* h, const void* img, int n_img, int H, int W, int C, int bps, uint8_t* gray_out, uint8_t* post,
                       int32_t* n_ec, int32_t* tie_risk) {
    if (!h) return ECSEG_E_INVALID;
    if (n_img < 0 || H <= 0 || W <= 0 || (C != 1 && C != 3 && C != 4) || (bps != 1 && bps != 2) || (n_img > 0 && (!img || !post)))
        return fail(h, ECSEG_E_INVALID, "meta_segment: bad arguments");
    if (n_img == 0) return ECSEG_OK;
    return meta_segment_run(h, img, n_img, H, W, C, bps, gray_out, post, n_ec, tie_risk, nullptr);
}

int ecseg_meta_segment_files(ecseg_ctx* h, const void* img, int n_img, int H, int W, int C, int bps, uint8_t* const* dapi_files,
                             long long dapi_cap, long long* dapi_bytes, uint8_t* const* png_files, long long png_cap, long long* png_bytes,
                             uint8_t* gray_out, uint8_t* labels_post, int32_t* n_ec, int32_t* tie_risk) {
    if (!h) return ECSEG_E_INVALID;
    if (n_img < 0 || H <= 0 || W <= 0 || (C != 1 && C != 3 && C != 4) || (bps != 1 && bps != 2) || (n_img > 0 && (!img || !labels_post)))
        return fail(h, ECSEG_E_INVALID, "meta_segment_files: bad arguments");
    if (!dapi_files || !dapi_bytes || !png_files || !png_bytes || dapi_cap < 1 || png_cap < 1)
        return fail(h, ECSEG_E_INVALID, "meta_segment_files: a null file table or a capacity below 1");
    for (int i = 0; i < n_img; ++i)
        if (!dapi_files[i] || !png_files[i]) return fail(h, ECSEG_E_INVALID, "meta_segment_files: a null file buffer");
    if (n_img >= 65536 || W >= (1 << 30)) return fail(h, ECSEG_E_INVALID, "meta_segment_files: 65536 images or more, or lines of 2^30 pixels or more");
    h->file_ms[0] = h->file_ms[1] = 0.f;
    if (n_img == 0) return ECSEG_OK;
    const int rps = tiff_rows_per_strip(H, W, 1);
    if ((H + rps - 1) / rps >= (1 << 26)) return fail(h, ECSEG_E_INVALID, "meta_segment_files: 2^26 strips or more (such a file would pass 4 GiB)");
    const MetaFiles files{dapi_files, dapi_cap, dapi_bytes, png_files, png_cap, png_bytes};
    return meta_segment_run(h, img, n_img, H, W, C, bps, gray_out, labels_post, n_ec, tie_risk, &files);
}

// ecseg_meta_segment with the files themselves as its input: what both entry points refuse before any work
static int tiffs_args(ecseg_ctx* h, const char* who, const uint8_t* files, long long files_bytes, const int64_t* file_ranges, int n_files, int H, int W,
                      int C, int bps, bool outputs) {
    if (n_files < 0 || files_bytes < 0 || H <= 0 || W <= 0 || (C != 1 && C != 3 && C != 4) || (bps != 1 && bps != 2) ||
        (n_files > 0 && (!files || !file_ranges || !outputs)))
        return fail(h, ECSEG_E_INVALID, std::string(who) + ": bad arguments");
    if (n_files >= 65536) return fail(h, ECSEG_E_INVALID, std::string(who) + ": 65536 images or more");
    return ECSEG_OK;
}

int ecseg_meta_segment_tiffs(ecseg_ctx* h, const uint8_t* files, long long files_bytes, const int64_t* file_ranges, int n_files, int H, int W, int C,
                             int bps, int32_t* status, uint8_t* gray_out, uint8_t* labels_post, int32_t* n_ec, int32_t* tie_risk) {
    if (!h) return ECSEG_E_INVALID;
    if (int rc = tiffs_args(h, "meta_segment_tiffs", files, files_bytes, file_ranges, n_files, H, W, C, bps, status && labels_post)) {
        drop_sent_ahead(h);
        return rc;
    }
    if (n_files == 0) { drop_sent_ahead(h); return ECSEG_OK; }
    const MetaTiffs tiffs{files, files_bytes, file_ranges, status};
    return meta_segment_run(h, nullptr, n_files, H, W, C, bps, gray_out, labels_post, n_ec, tie_risk, nullptr, &tiffs);
}

int ecseg_meta_segment_tiffs_files(ecseg_ctx* h, const uint8_t* files, long long files_bytes, const int64_t* file_ranges, int n_files, int H, int W,
                                   int C, int bps, int32_t* status, uint8_t* const* dapi_files, long long dapi_cap, long long* dapi_bytes,
                                   uint8_t* const* png_files, long long png_cap, long long* png_bytes, uint8_t* gray_out, uint8_t* labels_post,
                                   int32_t* n_ec, int32_t* tie_risk) {
    if (!h) return ECSEG_E_INVALID;
    const char* who = "meta_segment_tiffs_files";
    int rc = tiffs_args(h, who, files, files_bytes, file_ranges, n_files, H, W, C, bps, status && labels_post);
    if (!rc && (!dapi_files || !dapi_bytes || !png_files || !png_bytes || dapi_cap < 1 || png_cap < 1))
        rc = fail(h, ECSEG_E_INVALID, std::string(who) + ": a null file table or a capacity below 1");
    for (int i = 0; !rc && i < n_files; ++i)
        if (!dapi_files[i] || !png_files[i]) rc = fail(h, ECSEG_E_INVALID, std::string(who) + ": a null file buffer");
    if (!rc && W >= (1 << 30)) rc = fail(h, ECSEG_E_INVALID, std::string(who) + ": lines of 2^30 pixels or more");
    const int rps = rc ? 1 : tiff_rows_per_strip(H, W, 1);
    if (!rc && (H + rps - 1) / rps >= (1 << 26)) rc = fail(h, ECSEG_E_INVALID, std::string(who) + ": 2^26 strips or more (such a file would pass 4 GiB)");
    if (rc || n_files == 0) { drop_sent_ahead(h); if (!rc) h->file_ms[0] = h->file_ms[1] = 0.f; return rc; }
    h->file_ms[0] = h->file_ms[1] = 0.f;
    const MetaFiles out{dapi_files, dapi_cap, dapi_bytes, png_files, png_cap, png_bytes};
    const MetaTiffs tiffs{files, files_bytes, file_ranges, status};
    return meta_segment_run(h, nullptr, n_files, H, W, C, bps, gray_out, labels_post, n_ec, tie_risk, &out, &tiffs);
}

int ecseg_get_read_timings(ecseg_ctx* h, float* ms_out) {
    if (!h || !ms_out) return ECSEG_E_INVALID;
    ms_out[0] = h->read_ms;
    return ECSEG_OK;
}

// Names the files of the ecseg_meta_segment_tiffs call AFTER the coming one, as that call will pass them (page-locked memory, unchanged
// until then).  The coming ecseg_meta_segment_tiffs call uploads them on the input stream and decodes them there into the spare input
// buffer, under its own kernels, with scratch of its own (pre_arena: the status words are read by the call that takes the rasters); the
// call after it recognises them by (pointer, bytes, ranges, n, shape) and the handle's three tiff_*_on_device options as they stood
// when the set was planned, waits, swaps the buffers and skips upload and decode.  Any other call withdraws them, and so does a
// change of those options.  files == null or n_files == 0 withdraws.
int ecseg_prefetch_tiffs(ecseg_ctx* h, const uint8_t* files, long long files_bytes, const int64_t* file_ranges, int n_files, int H, int W, int C,
                         int bytes_per_sample) {
    if (!h) return ECSEG_E_INVALID;
    h->next_tiffs = TiffsKey();
    if (!files || !file_ranges || n_files <= 0) return ECSEG_OK;
    if (tiffs_args(h, "prefetch_tiffs", files, files_bytes, file_ranges, n_files, H, W, C, bytes_per_sample, true))
        return ECSEG_E_INVALID;
    TiffsKey& k = h->next_tiffs;
    k.files = files; k.bytes = files_bytes; k.n = n_files; k.H = H; k.W = W; k.C = C; k.bps = bytes_per_sample;
    k.ranges.assign(file_ranges, file_ranges + 2 * (size_t)n_files);
    return ECSEG_OK;
}

int ecseg_get_file_timings(ecseg_ctx* h, float* ms_out) {
    if (!h || !ms_out) return ECSEG_E_INVALID;
    ms_out[0] = h->file_ms[0]; ms_out[1] = h->file_ms[1];
    return ECSEG_OK;
}

// Names the raw images of the call AFTER the coming ecseg_meta_segment call (same n_img x H x W x C x bytes_per_sample layout,
// `bytes` in total, page-locked memory: from pageable memory the copy would be staged by the calling thread inside the
// coming call and delay its kernels).  The coming call sends them ahead on a stream of their own, under its kernels (2.4 ms
// for 32 RGB images), into the spare input buffer; the call after it recognises its images by (pointer, size) and skips its
// own upload (so the images must not change in between).  A call with other images uploads as always and drops what was sent
// ahead.  The memory is read during the coming call only.
int ecseg_prefetch_input(ecseg_ctx* h, const void* img, size_t bytes) {
    if (!h) return ECSEG_E_INVALID;
    h->next_host = (img && bytes) ? img : nullptr;
    h->next_bytes = h->next_host ? bytes : 0;
    return ECSEG_OK;
}

}  // extern "C"
