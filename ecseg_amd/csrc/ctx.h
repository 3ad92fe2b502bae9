// Internal header of the library's host side: the handle (ecseg_ctx), the device memory it owns and what the host-side files
// (api, filter_layout, model_load, plan_run, segment, drivers_*) share.  No kernel includes this.
#pragma once
#include <algorithm>
#include <array>
#include <map>
#include <string>
#include <utility>
#include <vector>

#include "common.h"
#include "tiff_parse.h"

namespace ecseg {

// h == null: the error of a failed ecseg_create
int fail(ecseg_ctx* h, int code, const std::string& msg);
int fail_hip(ecseg_ctx* h, hipError_t e, const char* what);
#define HIP_TRY(h, call) do { hipError_t _e = (call); if (_e != hipSuccess) return fail_hip((h), _e, #call); } while (0)

// Device buffer that frees itself: `cap` elements at `p`, allocated to exactly the size asked for when that is more than it holds
// (no growth factor: allocation sizes and moments are the caller's).  Reads as the pointer it owns.
template <typename T>
struct DevBuf {
    T* p = nullptr;
    size_t cap = 0;
    DevBuf() = default;
    DevBuf(DevBuf&& o) noexcept { swap(o); }
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    ~DevBuf() { if (p) (void)hipFree(p); }
    void swap(DevBuf& o) { std::swap(p, o.p); std::swap(cap, o.cap); }
    operator T*() const { return p; }
    int ensure(ecseg_ctx* h, size_t need_elems, const char* what = "hipMalloc") {
        if (need_elems <= cap && p) return ECSEG_OK;
        if (p) { hipError_t e = hipFree(p); p = nullptr; cap = 0; if (e != hipSuccess) return fail_hip(h, e, "hipFree"); }
        if (need_elems == 0) need_elems = 1;
        hipError_t e = hipMalloc(reinterpret_cast<void**>(&p), need_elems * sizeof(T));
        if (e != hipSuccess) { p = nullptr; return fail(h, ECSEG_E_NOMEM, std::string(what) + ": " + hipGetErrorString(e)); }
        cap = need_elems;
        return ECSEG_OK;
    }
};

struct OpRt {                 // run-time form of one plan operator
    ecseg_op_desc d;
    int path;                 // which kernel family
    float* wt = nullptr;      // device weights in the layout the chosen kernel wants
    float* wt_wino = nullptr; // Winograd-transformed filter (16 points) when the op is eligible
    float* wt_wino4 = nullptr; // F(4x4,3x3) filter image (36 points, per-wave stage layout of wino4r_kernel.hip / wino4_kernel.hip)
    float* wt_wino16 = nullptr; // F(2x2,3x3) filter image of wino16_kernel.hip (Cin, Cout in {16, 32})
    void* wt_split1 = nullptr; // bf16x3 image of convs_kernel.hip (one-tap GEMM: the 2x2 / stride-2 up-convolutions), made from `wt` when "winograd" = 3 is asked for
    int s1_cin = 0, s1_np = 0; // its K and column count (0: not eligible)
    void* wt_wino4s = nullptr; // bf16x3 stage image of wino4s_kernel.hip, made on the device from wt_wino4 when "winograd" = 3 is asked for
    int w4_cin = 0, w4_cout = 0; // the layer wt_wino4 was made for
    int coutp_wino = 0;
    float* bias = nullptr;
    float* head_w4 = nullptr; // PATH_HEAD with <= 4 classes: [cin][4] / [4] zero-padded copies for the fused output stage
    float* head_b4 = nullptr;
    // demand-driven cropping: which part of this op's OUTPUT somebody reads, as a recipe applied to the stitch's per-window
    // bounding box: 'd' = grow by one pixel (a 3x3 convolution behind), 'h' = halve (a 2x2 / stride-2 up-convolution
    // behind); crop_ok = false: everything is needed (or unknown)
    bool crop_ok = false;
    std::string crop_code;
    float* scale = nullptr;   // AFFINE
    float* shift = nullptr;
    int cin_chunks = 0, coutp = 0;
    int subpixel = 0;         // CONVT kh x kw / stride 2 with k in {3, 4} as a 2x2-tap convolution over the input (relayout_convt_subpixel)
    // round 6: the same layers with >= 32 output channels run PHASE BY PHASE instead - output rows y = 2 j + c come from the kernel rows
    // kh = c + crop (mod 2) at input offsets (c + crop - kh) / 2: four forward convolutions of 1 or 2 taps per axis on the input extent
    // (9 instead of 16 tap x phase products at k = 3, no zero blocks staged or multiplied, no overhanging tile row), each with a
    // strided scatter store.  ph_wt[c_y * 2 + c_x] != null: that path; ph_R / ph_S / ph_pt / ph_pl: taps and leading pad of each phase
    float* ph_wt[4] = {nullptr, nullptr, nullptr, nullptr};
    int ph_R[4] = {0, 0, 0, 0}, ph_S[4] = {0, 0, 0, 0}, ph_pt[4] = {0, 0, 0, 0}, ph_pl[4] = {0, 0, 0, 0};
    double flops = 0.0;       // algorithmic 2*MAC per patch
};
enum { PATH_MFMA = 1, PATH_SMALL_CIN = 2, PATH_HEAD = 3, PATH_GENERIC = 4, PATH_OTHER = 5, PATH_TAP = 6 /* conv_mfma_tap_kernel: any taps / stride / dilation */ };

struct CropLut {                  // size: extent (pixels) of the tensors it applies to; start[w]: first entry of window w (entries are window-major)
    DevBuf<int32_t> dev; int len = 0; int size = 0; std::vector<int> start;
};
struct StitchPlan {
    int n_pos = 0;
    DevBuf<int32_t> pos_dev;      // (n_pos, 2) window origins (row, col), reference order
    DevBuf<int32_t> map_dev;      // (H*W) source map
    // demand-driven cropping: per window the bounding box (y0, y1, x0, x1) of the pixels the stitch reads, and the region
    // lists built from it on first use, keyed by the op's crop recipe (OpRt::crop_code)
    std::vector<int> box;
    std::map<std::string, CropLut> luts;
    std::map<std::string, DevBuf<int32_t>> boxes;   // per recipe: device (n_pos, 4) need boxes (get_crop_box)
};

// Window lanes (round 4): windows [w0, w0 + cnt) of a batch on stream `s` (run_plan)
struct LaneSpec { int w0, cnt; hipStream_t s; };

// Every device allocation of the handle that outlives a call, apart from the model's (free_model).  A base of ecseg_ctx, so
// that the code says h->d_gray; ecseg_destroy moves it out and lets it die BEFORE the streams go.  A buffer added here is
// released with the rest: there is no list of names to keep.
struct DevMem {
    std::map<std::pair<int, int>, StitchPlan> stitch;      // per image size (get_stitch)
    DevBuf<uint8_t> d_gray, d_raw, d_post;
    DevBuf<int32_t> d_tie;        // per-image tie-risk counts of the last segment call
    DevBuf<int32_t> d_tie_sh;     // their replicated counters (one launch group)
    DevBuf<float> d_sprobs;       // stitched probabilities of one launch group (ecseg_segment_images_ex)
    DevBuf<uint8_t> d_aux8;       // second uint8 input (masks, rgb)
    DevBuf<uint8_t> d_pre;        // ecseg_prefetch_input: the raw images of the NEXT ecseg_meta_segment call, uploaded on their own stream while this call computes
    DevBuf<uint8_t> d_u8in;       // uint8 patches of forward_patches
    DevBuf<int32_t> d_i32;        // small int outputs
    DevBuf<long long> d_i64;
    DevBuf<float> d_probs_in;
    DevBuf<uint32_t> d_hist;
    // The drivers' scratch: each call lays its buffers out in an arena with the layout functions of common.h (lay_out below) and relies
    // on nothing an earlier call left there.  An arena grows to the largest need it has met and never shrinks.
    DevBuf<uint8_t> post_arena;   // the clean-up workspace `ws` (ensure_post)
    DevBuf<uint8_t> call_arena;   // everything a driver can size before its first launch
    DevBuf<uint8_t> count_arena;  // the FISH drivers: what is sized by the cell count, read back while call_arena is in use
    DevBuf<uint8_t> keep_arena;   // `iseg`, left by ecseg_nuclei_regions for ecseg_nucleus_crops: no other driver touches it
    DevBuf<uint8_t> fishdist_batch_buf;   // ecseg_fish_distances_batch alone: carved by the driver itself in two parts (fishdist_batch.h), grow-only
    DevBuf<uint8_t> pre_arena;    // ecseg_prefetch_tiffs: the decode-ahead's file images, tables and status words; they outlive the call that launched it, which call_arena does not
};

// A batch of TIFF files that decode into the input slots of one ecseg_meta_segment_tiffs call (segment.hip): the key the call after
// recognises them by, what the host made of every file, and the layout with raster i at i * H * W * C * bytes_per_sample.
struct TiffsKey {
    const uint8_t* files = nullptr; long long bytes = 0; int n = 0, H = 0, W = 0, C = 0, bps = 0;
    unsigned opts = 0;               // h->tiff_kinds when the set was planned: which kinds of file the handle took then
    std::vector<int64_t> ranges;
    bool same_set(const TiffsKey& o) const {
        return files && files == o.files && bytes == o.bytes && n == o.n && H == o.H && W == o.W && C == o.C && bps == o.bps && ranges == o.ranges;
    }
    bool same(const TiffsKey& o) const { return same_set(o) && opts == o.opts; }       // a set planned under other options is another set
};
struct TiffsPlan {
    std::vector<int> verdict;        // per file: ecseg_tiff_decode's status before any device work, or ECSEG_E_INVALID for another shape
    TdBatchLayout L;
    std::vector<uint32_t> tables;    // the strip tables as the device takes them
};

}  // namespace ecseg

struct ecseg_ctx : ecseg::DevMem {
    int device = 0;
    hipStream_t stream = nullptr;
    hipStream_t stream2 = nullptr;   // post-processing of group g overlaps the U-Net of group g+1
    std::vector<hipStream_t> lane_streams;   // window lanes of small batches (run_plan)
    std::vector<hipEvent_t> lane_events;
    int unet_lanes = 0;              // 0: automatic (2 lanes up to lane_auto_windows windows per group, else 1)
    int lane_auto_windows = 70;
    bool lanes_ok = false;           // the input's and the output's buffers hold nothing of another per-window size (run_plan)
    std::string err;
    char devname[256] = {0};

    bool has_model = false;
    std::vector<ecseg_tensor_desc> tensors;
    std::vector<ecseg::OpRt> ops;
    int n_buffers = 0;
    std::vector<size_t> buf_floats;       // floats per patch of every buffer
    std::vector<float*> bufs;
    int cap_patches = 0;
    std::vector<float*> dev_allocs;       // weight allocations (freed on reload / destroy)
    float* zero_page = nullptr;           // 1 KiB: 64 bytes of zeros + diagnostics scratch
    int input_tensor = -1, output_tensor = -1;
    std::vector<int> consumers;   // per tensor: number of operators reading it
    double flops_per_patch = 0.0, mfma_flops_per_patch = 0.0;

    // image pipeline
    int images_per_group = 0;    // images (of 35 windows) per U-Net launch; 0 = automatic: ~48 GB of activations (windows_per_group)
    const void* pre_host = nullptr; size_t pre_bytes = 0;  // what d_pre holds (host pointer + size are the key); nullptr: nothing
    const void* next_host = nullptr; size_t next_bytes = 0;   // registered by ecseg_prefetch_input for the coming call to send ahead
    hipStream_t stream_in = nullptr;
    hipEvent_t ev_pre = nullptr;
    ecseg::TiffsKey next_tiffs;      // registered by ecseg_prefetch_tiffs for the coming call to decode ahead
    ecseg::TiffsKey pre_tiffs;       // what d_pre holds decoded (files == nullptr: nothing), with pre_plan and the status words at pre_file_status
    ecseg::TiffsPlan pre_plan;
    uint32_t* pre_file_status = nullptr;   // in pre_arena: read by the call that takes the rasters, after ev_pre
    // ECSEG_TIFF_* bits, set and cleared by the options tiff_deflate_on_device / tiff_tiled_on_device / tiff_packbits_on_device: ecseg_tiff_decode,
    // ecseg_tiff_decode_batch and ecseg_meta_segment_tiffs take Deflate strips (tiffb_inflate_kernel) / tiled files (tiffb_untile_kernel) /
    // PackBits files (tiffb_packbits_kernel); a kind whose bit is clear is ECSEG_E_UNSUPPORTED
    unsigned tiff_kinds = 0;
    int min_cut_lds_pixels = ECSEG_MIN_CUT_LDS_PIXELS;   // windows above this many pixels keep their state in global memory (tests lower it)
    int min_cut_centers_lds_pixels = ECSEG_MIN_CUT_CENTERS_LDS_PIXELS;   // ecseg_min_cut_regions: crops above this many pixels keep their state in global memory (tests lower it)
    ecseg::PostWorkspace ws{};       // carved from post_arena
    ecseg::RegionMapBufs iseg{};     // carved from keep_arena
    int iseg_H = 0, iseg_W = 0, iseg_img_w = 0, iseg_C = 0, iseg_n = -1;   // iseg_n < 0: no region map on the handle
    int nuset_cls_t = -1, nuset_bbox_t = -1;   // the RPN tensors the last ecseg_nuset_forward left in the plan's buffers (-1: none)
    int post_chunk = 64;
    int overlap_post = 0;
    int blocking_wait = 1;    // the long waits (a whole launch group) sleep on a blocking event instead of spinning on the stream
    hipEvent_t ev_block = nullptr;
    int fuse_pool = 1;        // 2x2 max-pool written by the producing F(4x4) convolution's output stage
    int crop = 1;             // segment path: skip output regions of the last full-resolution convolutions that the stitch never reads
    int crop_mask = 1;        // cropped plan: Winograd kernels read zeros outside the receptive field of the needed outputs (0: A/B measurements only - results then depend on stale buffer contents in the last bits)
    int fuse_head = 1;        // 1x1 head (<= 4 classes) computed by the output stage of the last F(4x4) convolution
    int use_winograd = 2;     // 0 direct, 1 Winograd F(2x2,3x3), 2 F(4x4,3x3) where eligible (else F(2x2)), 3: F(4x4) with 3-way bf16 split operands on the bf16 matrix pipe where eligible (else as 2)
    int wino4_split = 1;      // F(4x4) layers with exactly 32 output channels: split-K over the channel-half waves (conv_wino4_kernel); 0: a zero-padded 64-channel block on conv_wino4r_kernel
    int wino16 = 1;           // F(2x2) layers with 16 / 32 input and output channels: conv_wino16_kernel (16x16x4 MFMA, register output stage)
    int wino_resident = 1;    // F(2x2) layers with <= 32 input and output channels: filter-resident kernel (conv_wino_res_kernel)
    int fuse_first = 1;       // the network's first layer (3x3, 1 -> 16 channels) computed into the halo of the 16 -> 16 convolution behind it (conv_wino16_kernel FIRST)

    // timing
    hipEvent_t ev[ECSEG_T_N + 1] = {};
    float stage_ms[ECSEG_T_N] = {};
    hipEvent_t ev_files[6] = {};     // the device file coders: [0, 1] the batched dapi strips, [2, 3] the PNG count, [4, 5] the PNG emit
    float file_ms[2] = {};           // device time of the last ecseg_meta_segment_files call's dapi encode and PNG kernels
    hipEvent_t ev_read[4] = {};      // the TIFF decode kernels: [0, 1] of the call itself, [2, 3] of the decode-ahead on stream_in
    float read_ms = 0.f, pre_read_ms = 0.f;   // device time of the decode that served the last ecseg_meta_segment_tiffs call / of the decode-ahead in d_pre
    bool profile_kernels = false;
    std::vector<hipEvent_t> prof_events;   // pairs
    std::vector<hipEvent_t> grp_events;    // 6 per image group of segment_dev
    size_t prof_used = 0;
    double prof_flops = 0.0, prof_exec_flops = 0.0;
    struct ProfRec { int op; int kind; double flops, exec_flops; float ms; };   // kind: 0 direct, 1 F(2x2), 2 F(4x4), 3 filter-resident F(2x2), 4 F(2x2) on 16x16x4 MFMAs (wino16), 5 F(4x4) with bf16x3 split operands (wino4s; exec_flops = the fp32-equivalent products, each issued as 6 bf16 products), 6 one-tap GEMM with bf16x3 split operands (convs_kernel)
    std::vector<ProfRec> prof_recs;        // one per profiled launch of the last segment / forward call
    double last_conv_ms = 0.0; long long last_conv_launches = 0; double last_conv_flops = 0.0, last_conv_exec_flops = 0.0;
};

namespace ecseg {

inline TView view_of(const ecseg_ctx* h, int t) {
    const ecseg_tensor_desc& d = h->tensors[t];
    TView v;
    v.p = h->bufs[d.buffer] + d.c_offset;
    v.h = d.h; v.w = d.w; v.c = d.c; v.cs = d.c_stride;
    return v;
}

inline float stage_elapsed(hipEvent_t a, hipEvent_t b) {
    float t = 0.f;
    return hipEventElapsedTime(&t, a, b) == hipSuccess ? t : 0.f;
}

// Measure, ensure, place: runs `layout` (which fills the caller's *Bufs through the layout functions of common.h) on a measuring
// Carver, grows `arena` to that size if it holds less, and runs it again on the arena.  When the allocation fails the *Bufs are
// left holding the measuring pass's bare offsets: a caller that keeps them on the handle (ws, iseg) marks them invalid itself.
template <typename F>
int lay_out(ecseg_ctx* h, DevBuf<uint8_t>& arena, F&& layout, const char* what = "hipMalloc") {
    Carver measure, place;
    layout(measure);
    if (int rc = arena.ensure(h, measure.used, what)) return rc;
    layout(place = Carver(arena.p));
    return ECSEG_OK;
}

// Images named or sent ahead by ecseg_prefetch_input belong to the very next ecseg_meta_segment call: any other call on the handle
// in between withdraws them (the hit is keyed by host pointer + size, and a registration that outlived its call could
// meet a recycled page-locked buffer of the same shape holding OTHER pixels).
inline void drop_sent_ahead(ecseg_ctx* h) {
    h->next_host = nullptr; h->next_bytes = 0;
    h->pre_host = nullptr; h->pre_bytes = 0;
    h->next_tiffs.files = nullptr; h->pre_tiffs.files = nullptr;     // (ecseg_prefetch_tiffs: the same rule)
}

// api.hip
int check_model(ecseg_ctx* h);

// drivers_files.hip: the file coders' tails, shared with ecseg_meta_segment_files (segment.hip) and ecseg_fish_render_tiff
// (drivers_fish.hip).  Both bring the tables over, wait, and copy every file that fits file_cap into files[i] (file_bytes[i]: its
// length); a file that does not fit is not produced.
// tiff_collect, strict: that is an error and nothing is written; else file_bytes[i] = -(the bytes it needs) and the call goes on.
inline bool tiff_args_ok(int H, int W, int spp) {            // what tiff_write_u8 (host_io.cpp) and with it the device encoder accepts
    return H > 0 && W > 0 && (spp == 1 || spp == 3) && (long long)W * spp < (1ll << 30);
}
int tiff_collect(ecseg_ctx* h, const char* who, int n_files, int H, int W, int spp, const TiffEncodeBufs& b, uint8_t* const* files,
                 long long file_cap, long long* file_bytes, bool strict);
// The batched encoder's two ends, shared by ecseg_tiff_encode_batch and ecseg_fish_render_tiff_batch (drivers_fish.hip): the table
// rows ([n][5]: byte offset, H, W, spp, invert) checked and turned into the layout's input, and - behind run_tiff_encode_batch - the
// file images, back to back in out, with out_ranges[f] = (offset, bytes); too small an out_cap is ECSEG_E_INVALID with nothing written.
std::string tiff_encode_batch_plan(const int64_t* files, int n_files, long long raster_bytes, std::vector<TeFileIn>& in);
int tiff_batch_collect(ecseg_ctx* h, const char* who, const TeBatchLayout& L, const TiffEncodeBatchBufs& b, uint8_t* out, long long out_cap,
                       int64_t* out_ranges);
// The label PNGs of n images that lie on the device (image i at d_labels + i * H * W), on the main stream: count, code build on the
// host, emit into count_arena, frame.  *ms: device time of the kernels.
int png_encode_files(ecseg_ctx* h, const char* who, const uint8_t* d_labels, int n, int H, int W, const PngEncodeBufs& b,
                     uint8_t* const* files, long long file_cap, long long* file_bytes, float* ms);

// The gray PNGs (ecseg_png_write_channel's files) of n_planes planes of images that lie on the device, on the main stream: count, code
// build and capacity verdict on the host, emit of the files that fit, frame.  files / file_bytes: per plane.  *ms: as above.
int png_gray_encode(ecseg_ctx* h, const char* who, const GraySource& src, int n_planes, int H, int W, const GrayEncodeBufs& b,
                    uint8_t* const* files, long long file_cap, long long* file_bytes, float* ms);

// The files of a batch as ecseg_tiff_decode judges each alone: info[i] and status[i] (with_strips: the file is to be decoded, not only
// measured), and the rows of the layout for the files that are ECSEG_OK (dst_offsets may be null: the rasters back to back, 16-bit
// ones on even offsets).  kinds (ECSEG_TIFF_*, a handle's tiff_kinds): the Deflate, tiled and PackBits files whose bit is set are taken,
// the others are ECSEG_E_UNSUPPORTED.
// Empty string, or which argument is wrong.
std::string tiff_batch_plan(const uint8_t* files, long long files_bytes, const int64_t* ranges, int n_files, const int64_t* dst_offsets,
                            bool with_strips, std::vector<TiffInfo>& info, std::vector<int>& status, std::vector<TdFileIn>& in, unsigned kinds);
// The rest of the way, one statement for ecseg_tiff_decode (a batch of one), ecseg_tiff_decode_batch and ecseg_meta_segment_tiffs:
// p.tables from the files' parsed tags and p.L; then, with the buffers of tiff_decode_batch_bufs(p.L), the upload of the file span,
// the table and the tables and the decode on stream s, the kernels between events e0 and e1.  p and the caller's files are read until
// s has been waited for; the status words (b.file_status) are the caller's to read.
void tiff_plan_tables(const std::vector<TiffInfo>& info, TiffsPlan& p);
int tiff_batch_launch(ecseg_ctx* h, const uint8_t* files, const TiffsPlan& p, const TiffDecodeBatchBufs& b, hipStream_t s, hipEvent_t e0, hipEvent_t e1);

// filter_layout.hip: host arrays to host arrays
std::vector<float> relayout_conv(const float* w, int R, int S, int cin, int cout, int chunks, int np);
std::vector<float> relayout_wino16(const std::vector<float>& u, int cin, int cout);
std::vector<float> winograd_filter(const float* w, int cin, int cout);
std::vector<float> winograd4_filter(const float* w, int cin, int cout);
std::vector<float> relayout_convt(const float* w, int kT, int cin, int cout, int chunks, int coutp);
std::vector<float> relayout_convt_subpixel(const float* w, int k, int cin, int cout, int chunks, int coutp);
struct PhaseFilter { std::vector<float> hwio; int R, S, pt, pl; };    // taps and leading pad of one output phase's forward convolution
std::array<PhaseFilter, 4> convt_phase_filters(const float* w, int k, int cin, int cout, int crop_top, int crop_left);

// model_load.hip
void free_model(ecseg_ctx* h);
int ensure_split_images(ecseg_ctx* h);

// plan_run.hip
int ensure_patches(ecseg_ctx* h, int n);
int windows_per_group(const ecseg_ctx* h);
int run_plan(ecseg_ctx* h, int n_all, StitchPlan* crop = nullptr, const std::vector<LaneSpec>* lanes = nullptr);
int run_plan_to_host(ecseg_ctx* h, int ni, float* out);   // run_plan on a filled input tensor + the outputs' copy, stream not waited for
void prof_begin(ecseg_ctx* h);
void prof_end(ecseg_ctx* h);    // stream must be idle

// segment.hip
int get_stitch(ecseg_ctx* h, int H, int W, StitchPlan** out);
int ensure_post(ecseg_ctx* h, int n_img, size_t px);

}  // namespace ecseg
