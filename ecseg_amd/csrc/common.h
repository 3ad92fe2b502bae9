// Shared declarations of libecseg_hip (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/ecseg_hip.h"
#include "scratch.h"
#include "iseg_batch.h"
#include "fish_batch.h"
#include "fishdist_batch.h"
#include "mincut_regions.h"
#include "tiff_decode_batch.h"
#include "tiff_encode_batch.h"
#include "tiff_frame.h"

namespace ecseg {

// NHWC float32 view into a device buffer: consecutive pixels are `cs` floats apart, `p` points at the view's first
// channel of pixel (n=0, y=0, x=0).
struct TView {
    float* p;
    int h, w, c, cs;
};

struct ConvParams {
    TView in, out;
    const float* wt;    // re-laid-out kernel (see relayout_* in filter_layout.hip)
    const float* bias;  // may be null
    int n;              // patches in the batch
    int R, S;           // taps
    int pad_top, pad_left;
    int act;
    float alpha;
    int cin_chunks;     // ceil(Cin / 8)
    int coutp;          // Cout padded to a multiple of the N tile
    // transposed-conv mode (R = S = 1 in the GEMM, kT x kT stride-kT scatter in the epilogue)
    int convt;          // 0 | 1 | 2 (2: ONE output phase per launch - N = coutp, the phase in phase_a / phase_b)
    int kT, crop_top, crop_left;
    int convt_ext;      // transposed mode: tiles walk the input extent + convt_ext (sub-pixel form of k x k / stride 2: 1)
    int phase_a, phase_b;   // transposed mode with ONE output phase per launch (N = coutp): the launch writes output (kT i + phase_a - crop_top, kT j + phase_b - crop_left)
    int tap_zero_mask;  // sub-pixel form (R = S = 2, kT = 2): bit (tap * 4 + phase) set = that (tap, output phase) block of the filter is all zero
                        // (7 of 16 at k = 3: the phases have 4, 2, 2 and 1 taps): conv_mfma_kernel skips its MFMAs.  0: multiply everything
    int stride;         // forward convolution: output stride (0 / 1: dense; 2: conv_mfma gathers a strided halo)
    const float* zero;  // >= 16 bytes of zeros in device memory (LDS-DMA source for padding / out-of-image pixels)
    TView pool;         // pool.p != null: also write MaxPooling2D(2x2, stride 2) of the activated output (conv_wino4 only)
    // fused 1x1 head (conv_wino4 only, Cout == 64): head_w != null: logits = act(out) . head_w[64][4] + head_b[4] (classes
    // padded to 4), head_act (softmax | linear ...) over head_k classes, written to head_out; the 64-channel output itself
    // is not written when head_only != 0
    const float* head_w; const float* head_b; TView head_out; int head_k, head_act, head_only;
    // demand-driven cropping (conv_wino4 only): lut != null: only the 16x16 regions listed are computed, the same list
    // for every image of `per_image` consecutive patches; entry = patch-in-image << 16 | (y origin / 4) << 8 | (x origin / 4)
    const int32_t* lut; int lut_len, per_image;
    // Winograd kernels of a cropped plan: in_box != null: (y0, y1, x0, x1), inclusive, per window of an image - the receptive
    // field of the outputs a later stage reads; input pixels outside it are read as ZERO.  A Winograd tile mixes its whole
    // 6x6 (4x4) input tile into every output: pixels outside an output's 3x3 support cancel only up to rounding, and
    // outside the box a cropped producer has left whatever the buffer held before - the results would depend (in the last
    // bits) on the history of the buffer.  Window of patch i: (i + box_first) % per_image.
    const int32_t* in_box; int box_first;
    // conv_mfma (transposed convolutions): the same list idea over its TH x TW tiles of the INPUT extent; force_tw = 16 | 32
    // selects the tile shape the list was built for (0: the launcher's own choice)
    int force_tw;
    // conv_wino (F(2x2)): 1: layers with <= 32 input and <= 32 output channels take the filter-resident kernel
    int resident;
    // conv_wino4: 1: a layer with exactly 32 output channels splits the input channels of every 8-channel group between the
    // two channel-half waves of a transform row instead of multiplying zero padding
    int w4_split;
    // conv_wino16 (16 -> 16 channels), round 5: first_w != null: p.in is the network's 1-channel INPUT and this launch also computes
    // the layer in front - Conv2D 3x3 'same', 1 -> 16 channels, kernel first_w[9][16] (HWIO), bias first_b (may be null),
    // activation first_act - on the matrix cores, straight into its own halo buffer: the 16-channel tensor between the two
    // layers never exists in memory
    const float* first_w; const float* first_b; int first_act; float first_alpha;
    // filter image strides in floats: [tap][chunk][half][N padded][4] with padded chunk / tap pitches (power-of-two
    // pitches put the 16 transform points of a K-chunk on the same L2 channel and set)
    long wt_chunk_stride, wt_tap_stride;
};

// Winograd F(4x4,3x3) interpolation points {0, +-W4_PA, +-W4_PB, inf}, shared by the host filter transform (filter_layout.hip:
// winograd4_filter) and the kernels' input / output transforms (wino4_consts.inc).  The textbook set is {0, +-1, +-2, inf};
// the rounding error of the result is dominated by the float32 channel sum of the transformed products on the matrix cores,
// whose magnitude the points set: tools/wino_points.py replays the kernel's arithmetic on the CPU and measures, against a
// float64 convolution, 4.4x the error of a sequential float32 direct convolution for {1, 2} and 2.0x for {5/8, 3/2} (the
// best pair on a 1/16 grid; both dyadic, so every constant of B^T and A^T stays exact in float32) - at the same number of
// VALU instructions (the +-1 rows' additions become fmas).
// (-DECSEG_W4_PA=1 -DECSEG_W4_PB=2 rebuilds the textbook kernel for A/B measurements: tools/build_variants.sh points12)
#ifndef ECSEG_W4_PA
#define ECSEG_W4_PA 0.625
#define ECSEG_W4_PB 1.5
#endif
constexpr double W4_PA = ECSEG_W4_PA, W4_PB = ECSEG_W4_PB;

// pitches used by relayout_* (filter_layout.hip) and the kernels
inline long wt_chunk_pitch(int np_total) { return (long)2 * np_total * 4 + 32; }
inline long wt_tap_pitch(int np_total, int chunks) { return wt_chunk_pitch(np_total) * chunks + 96; }

// Blocks of 256 threads for a grid-stride kernel over `total` work items: never 0, capped at 65536 * 16
inline unsigned grid_for(size_t total) {
    size_t b = (total + 255) / 256;
    if (b > 65536 * 16) b = 65536 * 16;
    return (unsigned)(b ? b : 1);
}

// ---- conv_mfma_kernel.hip: implicit-GEMM convolutions on the fp32 matrix cores ---------------------------------
hipError_t launch_conv_mfma(const ConvParams& p, hipStream_t s);
bool       conv_mfma_supported(const ConvParams& p);
int        conv_mfma_ntile(int cout);   // N tile (32 | 64 | 128) used for a given Cout
// Conv2D with any taps / stride / dilation on the matrix cores; p.wt = relayout_conv image, p.coutp padded to conv_mfma_ntile()
hipError_t launch_conv_mfma_tap(const ConvParams& p, int dilation, hipStream_t s);
bool       conv_mfma_tap_supported(const ConvParams& p);

// ---- wino2_kernel.hip: Winograd F(2x2,3x3) for 3x3 / stride 1 / pad 1 convolutions; p.wt = 16 transformed taps, p.coutp padded
// ---- to conv_wino_ntile() --------------------------------------------------------------------------------------
hipError_t launch_conv_wino(const ConvParams& p, hipStream_t s);
int        conv_wino_ntile(int cout);

// ---- the other matrix-core convolutions, one file each -----------------------------------------------------------
// Winograd F(2x2,3x3) for 16 / 32 input and output channels on 16x16x4 MFMAs (wino16_kernel.hip); p.wt = image written by
// relayout_wino16 (filter_layout.hip)
hipError_t launch_conv_wino16(const ConvParams& p, hipStream_t s);
bool       conv_wino16_supported(const ConvParams& p);
bool       conv_wino16_first_supported(const ConvParams& p);   // with ConvParams::first_w: the network's first layer computed into the halo
// Winograd F(4x4,3x3), split-K kernel for a lone 32-channel output block (wino4_kernel.hip: out.c == 32, no fused head; anything else is
// hipErrorInvalidValue); p.wt = image written by winograd4_filter (filter_layout.hip)
hipError_t launch_conv_wino4(const ConvParams& p, hipStream_t s);
// eligibility rules shared by the three F(4x4) kernels
bool       conv_wino4_supported(const ConvParams& p);
bool       conv_wino4_span_ok(const ConvParams& p, int windows);   // the halo's buffer descriptor reaches `windows` consecutive windows
// F(4x4,3x3) on the fp32 matrix cores with the row transform done once per workgroup (wino4r_kernel.hip, round 6): every fp32 F(4x4) layer but
// the lone 32-channel blocks that launch_conv_wino4 takes; p.wt as there
hipError_t launch_conv_wino4r(const ConvParams& p, hipStream_t s);
bool       conv_wino4r_supported(const ConvParams& p);
// F(4x4,3x3) with 3-way bf16 split operands on the bf16 matrix pipe (wino4s_kernel.hip, round 6); p.wt = the stage image written
// on the device by launch_wino4s_filter from the fp32 image of winograd4_filter (wino4s_image_bytes bytes)
hipError_t launch_conv_wino4s(const ConvParams& p, hipStream_t s);
bool       conv_wino4s_supported(const ConvParams& p);
size_t     wino4s_image_bytes(int cin, int cout);
hipError_t launch_wino4s_filter(const float* wt_wino4, void* dst, int cin, int cout, hipStream_t s);
// One-tap GEMM (2x2 / stride-2 transposed convolutions, 1x1 convolutions) with 3-way bf16 split operands (convs_kernel.hip, round 6);
// p.wt = the split image launch_convs_filter writes from the fp32 one-tap image (np = kT * kT * coutp columns; convs_image_bytes bytes)
hipError_t launch_convs(const ConvParams& p, hipStream_t s);
bool       convs_supported(const ConvParams& p);
size_t     convs_image_bytes(int cin, int np);
hipError_t launch_convs_filter(const float* wt_fp32, void* dst, int cin, int np, hipStream_t s);

// ---- conv_direct_kernels.hip: convolutions off the matrix cores ------------------------------------------------------
hipError_t launch_conv_small_cin(const TView& in, const TView& out, const float* w_hwio, const float* bias, int n,
                                 int R, int S, int pad_top, int pad_left, int act, float alpha, hipStream_t s);
hipError_t launch_conv_head(const TView& in, const TView& out, const float* w_io, const float* bias, int n, int act,
                            float alpha, hipStream_t s);
// scalar kernel: vertical / horizontal stride and dilation rate may differ (dilation rates below 1 count as 1)
hipError_t launch_conv_generic(const TView& in, const TView& out, const float* w_hwio, const float* bias, int n, int R, int S,
                               int stride, int stride_x, int dilation, int dilation_x, int pad_top, int pad_left, int act, float alpha,
                               hipStream_t s);
hipError_t launch_convt_generic(const TView& in, const TView& out, const float* w_hwoi, const float* bias, int n,
                                int R, int S, int stride, int crop_top, int crop_left, int act, float alpha,
                                hipStream_t s);
// DepthwiseConv2D: kernel (kh, kw, cin, mult), output channel = input channel * mult + j
hipError_t launch_dwconv(const TView& in, const TView& out, const float* w, const float* bias, int n, int kh, int kw, int stride,
                         int dilation, int pad_top, int pad_left, int mult, int act, float alpha, hipStream_t s);

// ---- layer_kernels.hip: everything that is not a convolution -----------------------------------------------------
hipError_t launch_maxpool(const TView& in, const TView& out, int n, int kh, int kw, int stride, int mode, hipStream_t s);
hipError_t launch_pool_pad(const TView& in, const TView& out, int n, int kh, int kw, int stride, int pad_top, int pad_left, int mode,
                           hipStream_t s);
hipError_t launch_global_pool(const TView& in, const TView& out, int n, int mode, hipStream_t s);
hipError_t launch_upsample(const TView& in, const TView& out, int n, int factor, int mode, hipStream_t s);
hipError_t launch_affine(const TView& in, const TView& out, const float* scale, const float* shift, int n, int act,
                         float alpha, hipStream_t s);
// y = act(a (+) b), mode = ECSEG_BIN_*, extents of 1 broadcast
hipError_t launch_binary(const TView& a, const TView& b, const TView& out, int n, int mode, int act, float alpha, hipStream_t s);
hipError_t launch_prelu(const TView& in, const TView& out, const float* slope, int n, int per_element, hipStream_t s);
hipError_t launch_layernorm(const TView& in, const TView& out, const float* gamma, const float* beta, int n, float eps, hipStream_t s);
hipError_t launch_copy(const TView& in, const TView& out, int n, int off_y, int off_x, hipStream_t s);
hipError_t launch_softmax(const TView& in, const TView& out, int n, hipStream_t s);
hipError_t launch_u8_to_f32(const uint8_t* in, float* out, size_t count, hipStream_t s);
// im2patches_overlap on the device: (n_img, H, W) uint8 -> (n_img * n_pos, 256, 256, 1) float32
hipError_t launch_tile_patches(const uint8_t* gray, int n_img, int H, int W, const int32_t* pos_yx, int n_pos,
                               float* out, hipStream_t s);

// ---- post-processing launchers: stitch_preprocess_kernels.hip (launch_stitch_*, launch_u16_to_u8, run_preprocess),
// ---- meta_inference_kernels.hip (run_meta_inference), ccl_kernels.hip (run_count_cc, run_ccl_labels, run_ccl_pass_debug),
// ---- overlay_kernels.hip (run_count_coloc, run_count_hsr, run_overlay); the labelling engine they share: ccl.h -------------
// stitch + img_as_ubyte + argmax; src_map: (H*W) int32 = (patch << 16) | (y << 8) | x, or -1 when never written
// tie_risk (may be null): per image, the pixels whose two largest quantised values differ by at most 1; tie_shards: scratch of
// n_img * G_SHARDS * G_STRIDE ints (replicated counters, one 128-B line each)
hipError_t launch_stitch_argmax(const float* probs, int prob_cs, const int32_t* src_map, int n_img, int n_pos,
                                int H, int W, uint8_t* labels, hipStream_t s, int32_t* tie_risk = nullptr, int32_t* tie_shards = nullptr);
// the stitched probabilities themselves: float32 (n_img, H, W, 4); never-written canvas pixels are 0
hipError_t launch_stitch_probs(const float* probs, int prob_cs, const int32_t* src_map, int n_img, int n_pos,
                               int H, int W, float* out, hipStream_t s);

struct PostWorkspace {
    // all sized for `cap_img` images of `cap_px` pixels
    int32_t* L;          // union-find parents / final root index per pixel
    uint32_t* area;      // per-root slots (indexed like L)
    unsigned long long* sumy;
    unsigned long long* sumx;
    uint32_t* flag;      // per-root bit flags
    uint8_t* tmpA;       // scratch label images
    uint8_t* tmpB;
    int32_t* list;       // per image: compacted root lists for the nucleus-in-metaphase test
    int32_t* g;          // G_SLOTS x cap_img blocks of per-image counters (G_STRIDE ints x G_SHARDS replicas each)
    uint8_t* tile_any;   // per image and 64 x 32 labelling tile: the tile holds a keyed pixel (written by ccl_local)
    uint32_t* own_bits;  // per image and tile: 2048 bits, bit = the pixel is the root of a tile component ("owner"; ccl_local -> ccl_resolve)
    double* binned;      // per image and axis: the chromosome centroids' coordinates grouped by integer bin (nucleus test)
    int32_t* binstart;   // per image and axis: first entry of every bin in `binned` (NUCLEUS_BIN_EXTENT + 2 ints)
    size_t binned_cap;   // entries per image and axis in `binned`
    int cap_img;
    size_t cap_px;
};
enum { G_STRIDE = 32, G_SHARDS = 16 };
enum { G_SLOTS = 6 };                  // counter blocks in PostWorkspace::g: one per labelling of run_meta_inference that produces counters (zeroed by ONE memset)
enum { NUCLEUS_BIN_EXTENT = 32768 };   // largest image extent for which the nucleus test runs on binned coordinates (LDS histogram)
inline PostWorkspace post_workspace(Carver& c, int n_img, size_t px) {
    PostWorkspace w{};
    const size_t ni = (size_t)n_img, tot = ni * px;
    // Root lists of the nucleus-in-metaphase test: run_meta_inference uses px/4 + (H+W)/2 + 4 entries per image
    // (>= ceil(H/2)*ceil(W/2), the most 8-connected components an image can hold); (H+W)/2 <= px/2 + 1, and every
    // entry costs 4 B (nucleus root) + 16 B (chromosome centroid).
    const size_t list_cap = px / 4 + px / 2 + 8;
    w.L = c.take<int32_t>(tot); w.area = c.take<uint32_t>(tot); w.sumy = c.take<unsigned long long>(tot); w.sumx = c.take<unsigned long long>(tot);
    w.flag = c.take<uint32_t>(tot); w.tmpA = c.take<uint8_t>(tot); w.tmpB = c.take<uint8_t>(tot);
    w.list = reinterpret_cast<int32_t*>(c.take<uint8_t>(ni * list_cap * 20 + 256)); w.g = c.take<int32_t>((size_t)G_SLOTS * ni * G_STRIDE * G_SHARDS);
    w.tile_any = c.take<uint8_t>(ni * (px / 16 + 2));          // (W/64 + 1)(H/32 + 1) <= px/16 + 1 tiles per image
    // owner bits: 256 B per 64 x 32 tile; ceil(W/64) ceil(H/32) <= px/2048 + W/64 + H/32 + 1 <= px/31 + 3 tiles for any H x W = px
    w.own_bits = c.take<uint32_t>(ni * (px / 31 + 4) * 64);
    w.binned_cap = list_cap < ((size_t)1 << 20) ? list_cap : (size_t)1 << 20;
    w.binned = c.take<double>(ni * 2 * w.binned_cap); w.binstart = c.take<int32_t>(ni * 2 * (NUCLEUS_BIN_EXTENT + 2));
    w.cap_img = n_img; w.cap_px = px;
    return w;
}

// meta_inference on n_img uint8 label images, in place; n_ec receives count_cc(img==3)[0] per image (when last == 6).
// first..last: the stages to run, 1..6 in production (the whole schedule); a partial range is test-only, as is kill_dev
// (n_img * H * W bytes, written when the range holds stage 4: 1 where the nucleus test erases the pixel).
hipError_t run_meta_inference(PostWorkspace& ws, uint8_t* img, int n_img, int H, int W, int32_t* n_ec_dev,
                              hipStream_t s, int first, int last, uint8_t* kill_dev = nullptr);
hipError_t run_count_cc(PostWorkspace& ws, const uint8_t* mask, int n_img, int H, int W, int32_t* n_dev,
                        long long* px_dev, hipStream_t s);
hipError_t run_ccl_labels(PostWorkspace& ws, const uint8_t* mask, int n_img, int H, int W, int conn,
                          int32_t* labels_dev, hipStream_t s);
// Test-only: ONE labelling pass (the CclPass of ccl.h, field by field) alone, with everything it produced exported.
// q_key / q_need: up to 5 queries of count_flagged_owner_roots_kernel (roots with key == q_key, 0 = any, whose flag word holds all
// bits of q_need), answered in counters 9 .. 13.
struct CclPassDesc {
    uint32_t lut;
    int conn, stat, aux_mode, aux_c, need;
    bool count_only, sparse, allow_full;
    int n_q, q_key[5];
    uint32_t q_need[5];
};
enum { CCL_DEBUG_COUNTERS = 16 };      // per image: NCOMP[1..3], NPX[1..3], LAST_ROOT, NLIST1, NLIST2, CNT0..4, two spare
// entries per image in each root list of a NEED_LISTS pass (run_meta_inference's formula: >= ceil(H/2) ceil(W/2), the most
// 8-connected components an image can hold)
inline size_t ccl_list_cap(int H, int W) { return (size_t)H * W / 4 + (size_t)(H + W) / 2 + 4; }
// root: per pixel, -1 unkeyed, else the component's root (pixel index in the image) read as consumers do, pixel -> owner -> root
// (-2: a parent out of range); count_only passes: the pixel's own index where count_roots_kernel counts it, else -1.
// area / sumy / sumx / flag: the root's slots at root pixels, 0 elsewhere.  list1 / list2: (n_img, ccl_list_cap) entries, -1 beyond
// the counts.
struct CclPassExport {
    int32_t* root; uint32_t* area; unsigned long long* sumy; unsigned long long* sumx; uint32_t* flag;
    int32_t* counters; int32_t* list1; int32_t* list2;
};
inline CclPassExport ccl_pass_export_bufs(Carver& c, int n_img, size_t px, size_t list_cap) {
    CclPassExport b;
    const size_t tot = (size_t)n_img * px;
    b.root = c.take<int32_t>(tot); b.area = c.take<uint32_t>(tot); b.sumy = c.take<unsigned long long>(tot);
    b.sumx = c.take<unsigned long long>(tot); b.flag = c.take<uint32_t>(tot);
    b.counters = c.take<int32_t>((size_t)n_img * CCL_DEBUG_COUNTERS);
    b.list1 = c.take<int32_t>((size_t)n_img * list_cap); b.list2 = c.take<int32_t>((size_t)n_img * list_cap);
    return b;
}
hipError_t run_ccl_pass_debug(PostWorkspace& ws, const uint8_t* key_img, const uint8_t* aux_img, int n_img, int H, int W,
                              const CclPassDesc& d, const CclPassExport& out, hipStream_t s);
hipError_t run_count_coloc(PostWorkspace& ws, const uint8_t* ob1, const uint8_t* ob2, int n_img, int H, int W,
                           int32_t* n_dev, hipStream_t s);
hipError_t run_count_hsr(PostWorkspace& ws, const uint8_t* chrom, const uint8_t* fish, int n_img, int H, int W,
                         int thr, int32_t* n_dev, hipStream_t s);
// labels: the driver's device copy; label bytes above 3 are folded to 0 in it (they are no class of the reference)
hipError_t run_overlay(PostWorkspace& ws, uint8_t* labels, const uint8_t* rgb, int n_img, int H, int W, int C,
                       int sens, int hsr_thr, long long* out_dev, hipStream_t s);
hipError_t launch_u16_to_u8(const uint16_t* in, uint8_t* out, size_t count, hipStream_t s);
// hist_ws: n_img * 256 counters, left holding the histograms; threshold (may be null): Otsu's threshold per image
hipError_t run_preprocess(const void* img, int n_img, int H, int W, int C, int bps, uint8_t* gray, int32_t* inverted,
                          uint32_t* hist_ws, hipStream_t s, int32_t* threshold = nullptr);
// Otsu and the "> 50 % white" decision alone on given histograms (n_img, 256); px_img (required): the sum of each; threshold may be null
hipError_t launch_otsu_decide(const uint32_t* hist, int n_img, const long long* px_img, int32_t* inverted, int32_t* threshold, hipStream_t s);

// ---- launchers implemented in interseg_kernels.hip (the file-level driver of src/interseg.py) ------------------------------
// What ecseg_nuclei_regions leaves for ecseg_nucleus_crops: the region label map (H, W) and the first H rows of the image.
struct RegionMapBufs { int32_t* lab; uint8_t* img; };
inline RegionMapBufs region_map_bufs(Carver& c, int H, int W, int img_w, int C) {
    RegionMapBufs b;
    b.lab = c.take<int32_t>((size_t)H * W); b.img = c.take<uint8_t>((size_t)H * img_w * C);
    return b;
}
// Device buffers of run_nuclei_regions: the per-pixel index rid with its scan blocks blk, the counters misc, and `cap` regions'
// worth of accumulators acc, bounding boxes bb and records rec.
struct RegionBufs { int32_t* rid; int32_t* blk; int32_t* misc; unsigned long long* acc; int32_t* bb; int64_t* rec; int cap; };
inline RegionBufs region_bufs(Carver& c, int H, int W, int cap) {
    const size_t px = (size_t)H * W, n = (size_t)cap;
    RegionBufs b;
    b.rid = c.take<int32_t>(px); b.blk = c.take<int32_t>((px + 1023) / 1024); b.misc = c.take<int32_t>(4); b.acc = c.take<unsigned long long>(n * 4);
    b.bb = c.take<int32_t>(n * 4); b.rec = c.take<int64_t>(n * 8);
    b.cap = cap;
    return b;
}
// Device buffers of run_nucleus_crops for n crops: the descriptors, the 256 x 256 x 3 crops and the channel maxima.
struct CropBufs { int32_t* desc; uint8_t* crops; int32_t* max; };
inline CropBufs crop_bufs(Carver& c, int n) {
    CropBufs b;
    b.desc = c.take<int32_t>((size_t)n * 5); b.crops = c.take<uint8_t>((size_t)n * 256 * 256 * 3); b.max = c.take<int32_t>((size_t)n * 3);
    return b;
}
// labels: in, run_ccl_labels' 8-connected labels of seg != 0 (one image); out, 1 + region index (skimage's order), 0 background.
// img: (>= H, img_w, C) uint8, channel ch0 summed per region.  misc[0] = number of regions, misc[1] = largest non-zero value of
// seg, misc[2] = 255 - smallest; rec: the first min(cap, misc[0]) region records (see ecseg_nuclei_regions).
hipError_t run_nuclei_regions(const uint8_t* seg, const uint8_t* img, int H, int W, int img_w, int C, int ch0, int32_t* labels,
                              const RegionBufs& b, hipStream_t s);
// desc: n crops (region, y0, x0, h, w), 1 <= h, w <= 256, inside the H x W label map -> out (n, 256, 256, 3) uint8 with channels
// order[0..2] of img, chmax (n, 3) int32
hipError_t run_nucleus_crops(const int32_t* labels, const uint8_t* img, int W, int img_w, int C, const int32_t* desc, int n,
                             const int order[3], uint8_t* out, int32_t* chmax, hipStream_t s);

// ---- launcher implemented in iseg_classify_kernels.hip (the classifiers' inputs; arithmetic and selection rules in iseg_classify.h) ----
// Device buffers of ecseg_classify_nucleus_crops for chunks of n crops: run_nucleus_crops' own and the two lists of chosen crops.
struct ClassifyBufs { CropBufs crop; int32_t* sel_i; int32_t* sel_c; };
inline ClassifyBufs classify_bufs(Carver& c, int n) {
    ClassifyBufs b;
    b.crop = crop_bufs(c, n); b.sel_i = c.take<int32_t>((size_t)n); b.sel_c = c.take<int32_t>((size_t)n);
    return b;
}
// Device buffers of ecseg_interseg_batch for one group of n images padded to Hm x Wm (iseg_batch.h, whose iseg_batch_bytes restates
// this layout's size): the group's bytes of the packed buffer, the table and the plan; mask, label map and region index of every
// padded pixel with the scan blocks; the counters misc (4) and imisc (n, 4); cap records' accumulators, boxes and records; one
// classifier chunk with the batch's own descriptors.
struct IsegBatchBufs {
    uint8_t* packed; IsegImage* tab; int32_t* plan; uint8_t* mask; int32_t* lab; int32_t* rid; int32_t* blk; int32_t* misc; int32_t* imisc;
    unsigned long long* acc; int32_t* bb; int64_t* rec; int32_t* desc; ClassifyBufs cls; int cap;
};
inline IsegBatchBufs iseg_batch_bufs(Carver& c, int n, int Hm, int Wm, size_t span, int cap) {
    const size_t px = (size_t)n * Hm * Wm, r = (size_t)cap;
    IsegBatchBufs b;
    b.packed = c.take<uint8_t>(span); b.tab = c.take<IsegImage>((size_t)n); b.plan = c.take<int32_t>((size_t)n * ISEG_PLAN);
    b.mask = c.take<uint8_t>(px); b.lab = c.take<int32_t>(px); b.rid = c.take<int32_t>(px); b.blk = c.take<int32_t>((px + 1023) / 1024);
    b.misc = c.take<int32_t>(4); b.imisc = c.take<int32_t>((size_t)n * 4);
    b.acc = c.take<unsigned long long>(r * 4); b.bb = c.take<int32_t>(r * 4); b.rec = c.take<int64_t>(r * 8);
    b.desc = c.take<int32_t>((size_t)ISEG_CHUNK * ISEG_DESC); b.cls = classify_bufs(c, ISEG_CHUNK);
    b.cap = cap;
    return b;
}
// The opening of a chunk of masks of different extents, shared by ecseg_interseg_batch and ecseg_stat_fish_batch: mask (n, Hm, Wm) =
// the segmentation of tab[i] (seg_off, h, w; bytes of `packed`) in the top left corner, background elsewhere; lab = its 8-connected
// labels (run_ccl_labels: 1 + the raster index, in the padded plane, of the component's first pixel).  n * Hm * Wm < 2^31.
hipError_t run_pad_label_masks(const uint8_t* packed, const IsegImage* tab, int n, int Hm, int Wm, uint8_t* mask, int32_t* lab, PostWorkspace& ws,
                               hipStream_t s);
// The group's tab and packed bytes are on the device: pads and labels the masks, numbers the regions per image, hands the cap records
// out (plan, misc[3] = records taken) and writes them; imisc[i][1..2]: image i's value range, as misc[1..2] of run_nuclei_regions.
hipError_t run_iseg_batch_regions(int n, int Hm, int Wm, int ch0, const IsegBatchBufs& b, PostWorkspace& ws, hipStream_t s);
// b.desc: n <= ISEG_CHUNK crops (image, region, y0, x0, h, w) -> b.cls.crop.crops / max, as run_nucleus_crops
hipError_t run_iseg_batch_crops(int Hm, int Wm, const IsegBatchBufs& b, int n, const int order[3], hipStream_t s);
// crops: (k, 256, 256, 3) uint8 with chmax (k, 3); sel_i / sel_c: n_i / n_c crop indices in [0, k), in any order, repeats allowed.
// out_i (n_i, 256, 256, 1) float32 = (float) of channel 0 of crop sel_i[j]; out_c (n_c, 256, 256, 3) float32 = preprocess_ecseg_c of
// crop sel_c[j] (iseg_c_value with the crop's own maxima).  Both 16-byte aligned; either list may be empty (its pointers unused).
hipError_t run_iseg_classifier_inputs(const uint8_t* crops, const int32_t* chmax, const int32_t* sel_i, int n_i, const int32_t* sel_c,
                                      int n_c, float* out_i, float* out_c, hipStream_t s);

// ---- launchers implemented in fishdist_kernels.hip (src/fish_distance_calculation.py:16-46) ---------------------------------
// The dense cell index of one H x W label map, shared with fishspot_kernels.hip: rid, its scan blocks blk and the counters misc,
// with the label map lab and the C-channel image img they belong to.
struct CellIndexBufs { int32_t* rid; int32_t* blk; int32_t* misc; int32_t* lab; uint8_t* img; };
inline CellIndexBufs cell_index_bufs(Carver& c, int H, int W, int C) {
    const size_t px = (size_t)H * W;
    CellIndexBufs b;
    b.lab = c.take<int32_t>(px); b.img = c.take<uint8_t>(px * C); b.rid = c.take<int32_t>(px); b.blk = c.take<int32_t>((px + 1023) / 1024);
    b.misc = c.take<int32_t>(4);
    return b;
}
// labels: (H, W) int32 instance labels, <= 0 background.  Leaves rid[label - 1] = dense ascending cell index of every label that
// occurs, misc[0] = number of cells, misc[3] = 1 when some label exceeds H * W (rid then misses it: do not go on).
hipError_t run_dense_cells(const int32_t* labels, int H, int W, const CellIndexBufs& b, hipStream_t s);
// Device buffers of run_fishdist_records: rid, blk and misc as run_dense_cells left them, the per-pixel par, flist and clist,
// and - sized by the number of cells n - acc, val, off, cur and rec, and the per-slice pbest and proots.
struct FishDistBufs { int32_t* rid; int32_t* par; int32_t* blk; int32_t* misc; int2* flist; int2* clist; unsigned* acc; int32_t* val;
                      int32_t* off; int32_t* cur; int64_t* rec; unsigned long long* pbest; int32_t* proots; };
int fishdist_slices(int n);   // workgroups per cell of the distance search for n cells
// slices: fishdist_slices(n)
inline FishDistBufs fishdist_bufs(Carver& c, const CellIndexBufs& cells, int H, int W, int n, int slices) {
    const size_t px = (size_t)H * W, nn = (size_t)n;
    FishDistBufs b;
    b.rid = cells.rid; b.blk = cells.blk; b.misc = cells.misc;
    b.par = c.take<int32_t>(px); b.flist = c.take<int2>(px); b.clist = c.take<int2>(px); b.acc = c.take<unsigned>(nn * 4);
    b.val = c.take<int32_t>(nn); b.off = c.take<int32_t>(nn * 2); b.cur = c.take<int32_t>(nn * 2); b.rec = c.take<int64_t>(nn * 8);
    b.pbest = c.take<unsigned long long>(nn * slices); b.proots = c.take<int32_t>(nn * slices);
    return b;
}
// After run_dense_cells with n = misc[0] > 0 and misc[3] == 0: relabels `labels` in place to cell + 1 and writes the n records
// of ecseg_fish_distances to rec.  lsq: (H, W, C) uint8; fi / ci: FISH and centromere channel.
hipError_t run_fishdist_records(int32_t* labels, const uint8_t* lsq, int H, int W, int C, int fi, int ci, int n, const FishDistBufs& b,
                                hipStream_t s);

// A chunk of images (ecseg_fish_distances_batch; layout, table and buffers in fishdist_batch.h).  b.lab holds the label maps and b.lsq
// the rasters where the table has them, b.tab the rows.  run_fishdist_batch_open builds the dense cell index of every image with one
// scan and leaves b.plan ((n + 1, 2) int32: per image its first cell and 1 = a label above H * W, such an image holding no cell; the
// last pair: the chunk's cells).  run_fishdist_batch_records, once the caller has carved c for those cells (partials = cells *
// fishdist_slices(cells)), relabels b.lab in place and writes the records of all images back to back to c.rec.
hipError_t run_fishdist_batch_open(const FdbLayout& L, const FdbPixelBufs& b, hipStream_t s);
hipError_t run_fishdist_batch_records(const FdbLayout& L, const FdbPixelBufs& b, const FdbCellBufs& c, int cells, int fi, int ci, hipStream_t s);

// ---- launcher implemented in fishspot_kernels.hip (src/stat_fish.py:73-107,134-142,226-300) ---------------------------------
// Device buffers of one H x W image with np probes: rid as run_dense_cells left it, mx, the outputs thr (one plane per probe) and
// bnd, par and sz (4 planes each: probes 0..2, the pair), the K x K filter weights w and - sized by the number of cells n - acc,
// cnt, val and rec.
struct FishSpotBufs { int32_t* rid; int32_t* mx; uint8_t* thr; uint8_t* bnd; int32_t* par; int32_t* sz; unsigned long long* acc;
                      unsigned* cnt; int32_t* val; int64_t* rec; double* w; };
inline FishSpotBufs fishspot_bufs(Carver& c, const CellIndexBufs& cells, int H, int W, int np, int K, int n) {
    const size_t px = (size_t)H * W, nn = (size_t)n;
    FishSpotBufs b;
    b.rid = cells.rid;
    b.mx = c.take<int32_t>(4); b.w = c.take<double>((size_t)K * K); b.thr = c.take<uint8_t>(px * np); b.bnd = c.take<uint8_t>(px);
    b.par = c.take<int32_t>(px * 4); b.sz = c.take<int32_t>(px * 4); b.acc = c.take<unsigned long long>(nn * 12); b.cnt = c.take<unsigned>(nn * 8);
    b.val = c.take<int32_t>(nn); b.rec = c.take<int64_t>(nn * ECSEG_FISH_SPOT_INT64);
    return b;
}
// After run_dense_cells with n = misc[0] > 0 and misc[3] == 0: relabels `labels` in place to cell + 1 and writes thr, bnd and the
// n records of ecseg_fish_spots.  img: (H, W, C) uint8; ch: the np probe channels; wts: K x K float64 on the device.
hipError_t run_fishspot(int32_t* labels, const uint8_t* img, int H, int W, int C, int np, const int ch[3], const double* wts, int K,
                        double normal_thr, const double ithr[3], int min_cc, int line_t, int n, const FishSpotBufs& b, hipStream_t s);

// A chunk of images (ecseg_stat_fish_batch; layout, table and buffers in fish_batch.h).  b.work holds the rasters, b.tab the rows,
// b.ptab the padded images' rows, b.w the weights, and the given label maps lie in b.lab.  run_fishspot_batch_open labels the masks,
// builds the dense cell index of every image with one scan and leaves per image its cells and first record in the rows and in b.plan
// ((n + 1, 2) int32: cells, 1 = a label above H * W; the last pair: the chunk's cells).  run_fishspot_batch, once the caller has
// read the plan and laid out c for `cells`: run_fishspot for every image, one launch per stage; b.lab becomes the ranks.
hipError_t run_fishspot_batch_open(const FsBatchLayout& L, const FsBatchBufs& b, PostWorkspace& ws, hipStream_t s);
hipError_t run_fishspot_batch(const FsBatchLayout& L, const FsBatchBufs& b, const FsBatchCellBufs& c, int cells, int max_cells, int line_t,
                              hipStream_t s);

// Device buffers of ecseg_fish_render for one H x W image of C channels: the inputs img (C bytes per pixel), thr (C - 1) and bnd
// (1), and the three (H, W, 3) outputs orig, seg and lsq.
struct FishRenderBufs { uint8_t* img; uint8_t* thr; uint8_t* bnd; uint8_t* orig; uint8_t* seg; uint8_t* lsq; };
inline FishRenderBufs fish_render_bufs(Carver& c, int H, int W, int C) {
    const size_t px = (size_t)H * W;
    FishRenderBufs b;
    b.img = c.take<uint8_t>(px * C); b.thr = c.take<uint8_t>(px * (C - 1)); b.bnd = c.take<uint8_t>(px);
    b.orig = c.take<uint8_t>(px * 3); b.seg = c.take<uint8_t>(px * 3); b.lsq = c.take<uint8_t>(px * 3);
    return b;
}
// The three colour files of stat_fish (:110-115,295-300) from b.img, b.thr and b.bnd into b.orig, b.seg and b.lsq, RGB.  C: 3 or
// 4; ch: the image's blue, green, red and (C = 4) aqua channel, each inside 0 .. C - 1.
hipError_t run_fish_render(int H, int W, int C, const int ch[4], const FishRenderBufs& b, hipStream_t s);

// ---- launcher implemented in tiff_kernels.hip (the LZW strips of tiff_write_u8, host_io.cpp) -----------------------------------
// Device buffers of one encode of n_files H x W rasters of spp samples (one extent, so one strip plan: strips of rps rows,
// nstrips per file).  img: the upload of ecseg_tiff_encode (zero bytes when the rasters are on the device already); slots: per
// (file, strip) slot_stride bytes = the host's bound 2 * strip bytes + 64, rounded up to 16; cnt: the encoded length of every
// strip; off: per file nstrips + 1 offsets of the packed strips, counted from the first strip, the last one their total; packed:
// per file file_stride bytes, room for every strip at its bound.
struct TiffEncodeBufs { uint8_t* img; uint8_t* slots; uint32_t* cnt; unsigned long long* off; uint8_t* packed;
                        size_t slot_stride, file_stride; int rps, nstrips; };
inline TiffEncodeBufs tiff_encode_bufs(Carver& c, int H, int W, int spp, int n_files, bool upload) {
    const size_t line = (size_t)W * spp;
    TiffEncodeBufs b;
    b.rps = tiff_rows_per_strip(H, W, spp);
    b.nstrips = (H + b.rps - 1) / b.rps;
    b.slot_stride = (tiff_strip_bound((size_t)b.rps * line) + 15) / 16 * 16;
    b.file_stride = (size_t)b.nstrips * b.slot_stride;
    const size_t nf = (size_t)n_files;
    b.img = c.take<uint8_t>(upload ? (size_t)H * line * nf : 0); b.slots = c.take<uint8_t>(nf * b.file_stride);
    b.cnt = c.take<uint32_t>(nf * b.nstrips); b.off = c.take<unsigned long long>(nf * ((size_t)b.nstrips + 1));
    b.packed = c.take<uint8_t>(nf * b.file_stride);
    return b;
}
// Encodes n_files rasters that lie on the device: the strips (horizontal predictor, `invert`, LZW) into b.slots and b.cnt, the
// scan into b.off, the gather into b.packed.  nstrips must be below 2^26.  The rasters: stride == 0: img[0 .. n_files - 1], at
// most three of them; stride > 0: a batch, raster f at img[0] + f * stride (n_files below 65536: grid dimension y is the file).
struct TiffSources { const uint8_t* img[3]; size_t stride; };
hipError_t run_tiff_encode(const TiffSources& src, int n_files, int H, int W, int spp, int invert, const TiffEncodeBufs& b, hipStream_t s);
// Encodes a batch of rasters laid out by te_batch_layout (tiff_encode_batch.h), in one launch per kernel: the strips of all files
// into b.slots and b.cnt, per file its strip offsets into b.off, where every file image starts into b.base, and the strips into
// b.packed at base[f] + 8 + off, the gaps for heads and tails left as they are.  b.tab is in place and b.src holds the rasters.
hipError_t run_tiff_encode_batch(const TiffEncodeBatchBufs& b, const TeBatchLayout& L, hipStream_t s);

// ---- launcher implemented in tiff_decode_kernels.hip (the strips of ecseg_tiff_read, host_io.cpp) -------------------------------
// Decodes a batch of files laid out by td_batch_layout (tiff_decode_batch.h; a lone file is a batch of one), in one launch per kernel:
// every strip of every file (LZW or uncompressed, a strip holds less than 2^31 bytes) into b.rasters and b.strip_status (0, or 1:
// corrupt), the row pass - 16-bit samples swapped, the horizontal predictor undone - once per sample size that needs it, then
// b.file_status (0, or 1: some strip of the file is corrupt).  b.tab, b.files and b.tables are in place.
hipError_t run_tiff_decode_batch(const TiffDecodeBatchBufs& b, const TdBatchLayout& L, hipStream_t s);

// ---- launchers implemented in png_kernels.hip (the label PNG of ecseg_png_write_labels, host_io.cpp) ------------------------------
// The token counts of one image, as deflate_labels' pass 1 takes them: [0..3] runs per colour, [4 + m] matches of 4 m bytes for
// m = 1..64 (m = 64 with the whole-64 parts of long runs; m = 0 counts the runs without a remainder match and is not used).
constexpr int PNG_NCOUNT = 4 + 65;
// One image's code on the device (LabelPngCode, png_label_code.h, in dwords): cbits / cn per colour, mbits / mn per match of 4 m
// bytes, head the first head_bits bits of the stream as little-endian dwords (1540 at most), the codes of the filter byte and
// of the end of the block; z_off / z_words: where in the stream buffer the image's stream lies (in dwords) and the dwords it owns.
struct PngDevCode {
    unsigned long long cbits[4];
    unsigned long long z_off;
    uint32_t cn[4], mbits[65], mn[65], head[64];
    uint32_t head_bits, filt, filt_n, eob, eob_n, z_words;
};
static_assert(sizeof(PngDevCode) % 8 == 0, "copied to LDS dword by dword, laid out as an array");
// Device buffers of one encode of n H x W label images: labels (the upload of ecseg_png_labels_encode; zero bytes when the labels
// are on the device already), the counts, per scan line its Adler terms, its bits and its bit offset in the stream, per image its
// code and the stream's length as the device found it.
struct PngEncodeBufs { uint8_t* labels; uint32_t* counts; uint32_t* row_a; uint32_t* row_b; unsigned long long* row_bits;
                       unsigned long long* row_off; PngDevCode* codes; unsigned long long* z_bytes; };
inline PngEncodeBufs png_encode_bufs(Carver& c, int H, int W, int n, bool upload) {
    const size_t rows = (size_t)n * H;
    PngEncodeBufs b;
    b.labels = c.take<uint8_t>(upload ? rows * W : 0); b.counts = c.take<uint32_t>((size_t)n * PNG_NCOUNT);
    b.row_a = c.take<uint32_t>(rows); b.row_b = c.take<uint32_t>(rows);
    b.row_bits = c.take<unsigned long long>(rows); b.row_off = c.take<unsigned long long>(rows);
    b.codes = c.take<PngDevCode>((size_t)n); b.z_bytes = c.take<unsigned long long>((size_t)n);
    return b;
}
// labels: n images of H x W, image i at labels + i * img_stride, on the device.  run_png_count clears and fills b.counts, b.row_a
// and b.row_b; run_png_emit, with b.codes in place, clears z (z_bytes bytes, a multiple of 4) and writes every stream and b.z_bytes.
// n below 65536 (grid dimension y is the image), W below 2^30.
hipError_t run_png_count(const uint8_t* labels, size_t img_stride, int n, int H, int W, const PngEncodeBufs& b, hipStream_t s);
hipError_t run_png_emit(const uint8_t* labels, size_t img_stride, int n, int H, int W, const PngEncodeBufs& b, uint32_t* z, size_t z_bytes,
                        hipStream_t s);

// ---- launchers implemented in png_gray_kernels.hip (the gray PNG of ecseg_png_write_channel, host_io.cpp) ------------------------
// A plane is one (image, channel) pair; plane p is channel (chans >> 8 (p % n_ch)) & 255 of image p / n_ch.  Its filtered stream has
// n = H (W + 1) bytes (below 2^31) and is walked in spans of PGRAY_SPAN bytes, a wave each.  The counts of one plane: the 286
// literal / length symbols as deflate_gray_sub's first scan takes them (the end of the block not counted), [286]: runs with a match.
constexpr int PGRAY_NCOUNT = 287;
constexpr uint32_t PGRAY_SPAN = 1024;
struct GraySource { const uint8_t* px; size_t img_stride; uint32_t W, C, n, n_ch, chans, invert; };
// One plane's code on the device (GrayPngCode, png_gray_code.h): lit[b] = code | length << 16; match[L] = bits | length << 24 for a
// match of L = 3..258 bytes; head the first head_bits bits of the stream as little-endian dwords (1525 at most); z_off / z_words:
// where in the stream buffer the plane's stream lies (in dwords) and the dwords it owns - none for a file that does not fit.
struct GrayDevCode {
    unsigned long long z_off;
    uint32_t lit[256], match[260], head[64];
    uint32_t head_bits, eob, eob_n, z_words;
};
static_assert(sizeof(GrayDevCode) % 8 == 0, "copied to LDS dword by dword, laid out as an array");
// Device buffers of one encode of n_planes planes of n_img H x W x C images: px (the upload of ecseg_png_channel_encode; zero bytes
// when the pixels are on the device already), the counts, per span the start of the run that reaches into it, its Adler terms, its
// bits and its bit offset, per plane its code and the stream's length as the device found it, and the streams: z_stride bytes per
// plane, sized as the host writer sizes its own buffer (2 n + 4096), the streams packed from its front by their exact sizes.
struct GrayEncodeBufs { uint8_t* px; uint32_t* counts; uint32_t* span_carry; uint32_t* span_a; uint32_t* span_b; unsigned long long* span_bits;
                        unsigned long long* span_off; GrayDevCode* codes; unsigned long long* z_bytes; uint32_t* z; uint32_t n_spans; size_t z_stride; };
inline GrayEncodeBufs gray_encode_bufs(Carver& c, int H, int W, int C, int n_img, int n_planes, bool upload) {
    const size_t n = (size_t)H * ((size_t)W + 1), np = (size_t)n_planes;
    GrayEncodeBufs b;
    b.n_spans = (uint32_t)((n + PGRAY_SPAN - 1) / PGRAY_SPAN);
    b.z_stride = (2 * n + 4096 + 3) / 4 * 4;
    const size_t spans = np * b.n_spans;
    b.px = c.take<uint8_t>(upload ? (size_t)n_img * H * W * C : 0); b.counts = c.take<uint32_t>(np * PGRAY_NCOUNT);
    b.span_carry = c.take<uint32_t>(spans); b.span_a = c.take<uint32_t>(spans); b.span_b = c.take<uint32_t>(spans);
    b.span_bits = c.take<unsigned long long>(spans); b.span_off = c.take<unsigned long long>(spans);
    b.codes = c.take<GrayDevCode>(np); b.z_bytes = c.take<unsigned long long>(np); b.z = c.take<uint32_t>(np * (b.z_stride / 4));
    return b;
}
// run_pgray_count clears and fills b.counts, b.span_carry, b.span_a and b.span_b; run_pgray_emit, with b.codes in place, clears the
// first z_bytes bytes of b.z (a multiple of 4) and writes every stream that has dwords, and b.z_bytes.  n_planes below 65536 (grid
// dimension y is the plane).
hipError_t run_pgray_count(const GraySource& src, int n_planes, const GrayEncodeBufs& b, hipStream_t s);
hipError_t run_pgray_emit(const GraySource& src, int n_planes, const GrayEncodeBufs& b, size_t z_bytes, hipStream_t s);

// ---- launcher implemented in mincut_kernels.hip (src/max_flow_binary_mask.py:59-116) -----------------------------------------
// n_tasks tasks of ecseg_min_cut, one workgroup each.  desc: (n_tasks, 8) int32 as the entry point takes them, validated by the
// caller; soff: per task the byte offset of its mincut_scratch_bytes(h, w) bytes in `scratch` (16-byte aligned), or < 0 for a
// window of at most ECSEG_MIN_CUT_LDS_PIXELS pixels whose state stays in LDS.  side: as masks, written over every window.
size_t mincut_scratch_bytes(int h, int w);
// Device buffers of one ecseg_min_cut call: the packed windows and their sides (mask_bytes each), the task table desc with the
// offsets soff and the flows, and scratch_bytes = the sum of mincut_scratch_bytes over the windows too large for LDS.
struct MinCutBufs { uint8_t* mask; uint8_t* side; int32_t* desc; long long* soff; int32_t* flow; uint8_t* scratch; };
inline MinCutBufs mincut_bufs(Carver& c, size_t mask_bytes, int n_tasks, size_t scratch_bytes) {
    MinCutBufs b;
    b.mask = c.take<uint8_t>(mask_bytes); b.side = c.take<uint8_t>(mask_bytes); b.desc = c.take<int32_t>((size_t)n_tasks * 8);
    b.soff = c.take<long long>((size_t)n_tasks); b.flow = c.take<int32_t>((size_t)n_tasks); b.scratch = c.take<uint8_t>(scratch_bytes);
    return b;
}
// n_global: how many tasks have soff >= 0 (a kernel without tasks is not launched).
hipError_t run_mincut(const uint8_t* masks, const int32_t* desc, const long long* soff, int n_tasks, int n_global, int d, uint8_t* scratch,
                      uint8_t* side, int32_t* flow, hipStream_t s);

// ---- launchers implemented in mincut_centers_kernels.hip (src/max_flow_binary_mask.py:143-216; layout: mincut_regions.h) ------
// (the device buffers McrOpenBufs and McrRegionBufs are laid out in mincut_regions.h)
// b.mask on the device, H * W < 2^31 -> b.lab = run_ccl_labels' 4-connected labels, b.rid[p] = roots in front of pixel p,
// b.misc[0] = the number of labels.
hipError_t run_mcr_label(PostWorkspace& ws, int H, int W, const McrOpenBufs& b, hipStream_t s);
// n = b.misc[0] > 0 -> b.lab renumbered 1..n in raster order of first pixels; stats (n, 5): area, first and last row, first and last column
hipError_t run_mcr_stats(int H, int W, int n, const McrOpenBufs& b, int32_t* stats, hipStream_t s);
// b.regions (label, r0, c0, h, w, window offset) and b.slot in place -> b.windows, b.comp (numbered 1.. per region), b.counts,
// b.first, *b.total and the centre records; n_lds: how many regions mcr_in_lds admits (a kernel without regions is not launched).
hipError_t run_mcr_centers(const int32_t* labels, int W, int n_regions, int n_lds, int min_rad, int lds_pixels, const McrRegionBufs& b,
                           hipStream_t s);

// ---- launchers implemented in nuset_kernels.hip (src/utils.py:53, src/model_layers/rpn_proposal.py) ---------------------------
// mask (h * w uint8) = argmax over the 2 channels of `logits`, a tie giving 0.
hipError_t launch_argmax2(const TView& logits, uint8_t* mask, hipStream_t s);
struct NusetMaskBufs { uint8_t* mask; };
inline NusetMaskBufs nuset_mask_bufs(Carver& c, int H, int W) { return NusetMaskBufs{c.take<uint8_t>((size_t)H * W)}; }
// Device buffers of one proposal call over N = fh * fw * A candidates: boxes, scores, the sort keys, the suppression matrix mat
// over the K = min(pre_nms_top_n, N) best, misc (n_out, kept candidates), the outputs (min(post_nms_top_n, K) entries each), the
// A reference anchors ref and, where the host gives them, the RPN tensors cls and bbox.
struct RpnBufs { float4* boxes; float* scores; unsigned long long* keys; unsigned long long* mat; int32_t* misc; float* out_scores;
                 float4* out_boxes; int32_t* out_idx; double* ref; float* cls; float* bbox; };
int rpn_sort_len(int N);      // N padded to the power of two the sort works on
// sort_len: rpn_sort_len(fh * fw * A); upload: the RPN tensors come from the host (else cls and bbox are empty slots)
inline RpnBufs rpn_bufs(Carver& c, int fh, int fw, int A, int sort_len, int pre, int post, bool upload) {
    const size_t px = (size_t)fh * fw, N = px * A, K = (size_t)pre < N ? (size_t)pre : N, no = (size_t)post < K ? (size_t)post : K;
    RpnBufs b;
    b.ref = c.take<double>((size_t)A * 4); b.boxes = c.take<float4>(N); b.scores = c.take<float>(N);
    b.keys = c.take<unsigned long long>((size_t)sort_len); b.mat = c.take<unsigned long long>(K * ((K + 63) / 64)); b.misc = c.take<int32_t>(2);
    b.out_scores = c.take<float>(no); b.out_boxes = c.take<float4>(no); b.out_idx = c.take<int32_t>(no);
    b.cls = c.take<float>(upload ? px * 2 * A : 0); b.bbox = c.take<float>(upload ? px * 4 * A : 0);
    return b;
}
// cls / bbox: (fh, fw, 2A) / (fh, fw, 4A) float32 on the device, consecutive pixels cls_cs / bbox_cs floats apart; ref: A x 4
// float64 on the device.  The arguments are validated by the caller (ecseg_rpn_proposals).
hipError_t run_rpn_proposals(const float* cls, int cls_cs, const float* bbox, int bbox_cs, const double* ref, int fh, int fw, int A, int stride,
                             int im_h, int im_w, float nms_threshold, int pre, int post, const RpnBufs& b, hipStream_t s);

// ---- launcher implemented in watershed_kernels.hip (src/nuset_utils/normalization.py:25-37, src/utils.py:159-162) ------------
// Device buffers of one H x W image: the input mask, par and sz, tmp, cleaned and out, misc (cells, pixels, the value flags of
// `cleaned`, 0) and dbl (mean_area, mean_area / 5).
struct CleanBufs { int32_t* par; int32_t* sz; uint8_t* tmp; uint8_t* cleaned; uint8_t* out; int32_t* misc; double* dbl; uint8_t* mask; };
inline CleanBufs clean_bufs(Carver& c, int H, int W) {
    const size_t px = (size_t)H * W;
    CleanBufs b;
    b.mask = c.take<uint8_t>(px); b.tmp = c.take<uint8_t>(px); b.cleaned = c.take<uint8_t>(px); b.out = c.take<uint8_t>(px);
    b.par = c.take<int32_t>(px); b.sz = c.take<int32_t>(px); b.misc = c.take<int32_t>(4); b.dbl = c.take<double>(2);
    return b;
}
// mask: (H, W) uint8 on the device, H * W < 2^31 -> cleaned (clean_image, 0 / 1), out (the final mask, 0 / 255), dbl[0] = mean_area.
hipError_t run_clean_nuclei(const uint8_t* mask, int H, int W, int nuclei_size_t, const CleanBufs& b, hipStream_t s);

// Device buffers of run_marker_watershed for one H x W image: the input mask, the per-pixel idx, rw, g, d2, lab, par, sz, work,
// filled and out, misc ([0] `filled` holds a zero, [1] heap overflow), the heap (heap_cap keys and payloads) and the n_markers
// markers' rows, cols and labels.
struct WatershedBufs { int32_t* idx; int32_t* rw; int32_t* g; int32_t* d2; int32_t* lab; int32_t* par; int32_t* sz; uint8_t* work;
                       uint8_t* filled; uint8_t* out; int32_t* misc; unsigned long long* heap_k; int2* heap_p; uint8_t* mask;
                       int32_t* rows; int32_t* cols; int32_t* labels; };
inline WatershedBufs watershed_bufs(Carver& c, int H, int W, int n_markers, int heap_cap) {
    const size_t px = (size_t)H * W;
    WatershedBufs b;
    b.mask = c.take<uint8_t>(px); b.out = c.take<uint8_t>(px); b.par = c.take<int32_t>(px); b.sz = c.take<int32_t>(px); b.misc = c.take<int32_t>(4);
    b.idx = c.take<int32_t>(px); b.rw = c.take<int32_t>(px); b.g = c.take<int32_t>(px); b.d2 = c.take<int32_t>(px); b.lab = c.take<int32_t>(px);
    b.work = c.take<uint8_t>(px); b.filled = c.take<uint8_t>(px); b.rows = c.take<int32_t>((size_t)n_markers);
    b.cols = c.take<int32_t>((size_t)n_markers); b.labels = c.take<int32_t>((size_t)n_markers);
    b.heap_k = c.take<unsigned long long>((size_t)heap_cap); b.heap_p = c.take<int2>((size_t)heap_cap);
    return b;
}
// mask (H, W) uint8 and the n ordered markers (validated by the caller) on the device -> out = mask * (flooded label != 0).
// heap_cap >= 5 * (non-zero mask pixels) + 1: every marker pixel once, at most four pushes per expanded pixel.
hipError_t run_marker_watershed(const uint8_t* mask, int H, int W, const int32_t* rows, const int32_t* cols, const int32_t* labels, int n,
                                int heap_cap, const WatershedBufs& b, hipStream_t s);

// One image of a batched marker watershed, as the device reads it: its H x W bytes start `off` bytes into the packed masks (and its
// per-pixel int32 values `off` elements into theirs), its n_markers markers at entry first_marker of the lists, its heap of heap_cap
// elements at element heap_off of the batch's keys and payloads.
struct WsImage { long long off; long long heap_off; int H, W, first_marker, n_markers, heap_cap, pad; };
// Device buffers of run_marker_watershed_batch over n_images images inside `span` packed bytes: what WatershedBufs holds per pixel,
// `span` elements each and every image's part at its own offset; misc with 4 words per image ([0] `filled` holds a zero, [1] heap
// overflow); the table; the first n_markers entries of the lists; heap_total = the sum of the heap capacities.  The heaps are typed
// arrays indexed by element, so a slice starts on a multiple of 8 bytes wherever its image's bytes start.
struct WatershedBatchBufs { uint8_t* mask; uint8_t* out; uint8_t* work; uint8_t* filled; int32_t* idx; int32_t* rw; int32_t* g; int32_t* d2;
                            int32_t* lab; int32_t* par; int32_t* sz; int32_t* misc; WsImage* tab; int32_t* rows; int32_t* cols; int32_t* labels;
                            unsigned long long* heap_k; int2* heap_p; };
inline WatershedBatchBufs watershed_batch_bufs(Carver& c, size_t span, int n_images, size_t n_markers, size_t heap_total) {
    WatershedBatchBufs b;
    b.mask = c.take<uint8_t>(span); b.out = c.take<uint8_t>(span); b.work = c.take<uint8_t>(span); b.filled = c.take<uint8_t>(span);
    b.idx = c.take<int32_t>(span); b.rw = c.take<int32_t>(span); b.g = c.take<int32_t>(span); b.d2 = c.take<int32_t>(span);
    b.lab = c.take<int32_t>(span); b.par = c.take<int32_t>(span); b.sz = c.take<int32_t>(span); b.misc = c.take<int32_t>((size_t)n_images * 4);
    b.tab = c.take<WsImage>((size_t)n_images); b.rows = c.take<int32_t>(n_markers); b.cols = c.take<int32_t>(n_markers);
    b.labels = c.take<int32_t>(n_markers); b.heap_k = c.take<unsigned long long>(heap_total); b.heap_p = c.take<int2>(heap_total);
    return b;
}
// b.mask, b.tab and the lists filled and validated by the caller; max_px / max_w / max_markers: the largest pixel count, width and
// marker count of one image (they size the grids) -> b.out = per image what run_marker_watershed gives it, 0 outside every image.
hipError_t run_marker_watershed_batch(int n_images, size_t span, int max_px, int max_w, int max_markers, const WatershedBatchBufs& b,
                                      hipStream_t s);

// ---- launchers implemented in rescale_kernels.hip (src/utils.py:136,157-162 on scikit-image 0.18 / scipy 1.7) ------------------
// img (H, W) uint8 on the device -> filtered (H, W) uint8 (the two truncating Gaussian passes; tmp: H*W uint8 between them) and out
// (oh, ow) float64 (the bilinear warp of filtered / 255).  wy / wx: 2 r + 1 float64 weights on the device, r = 0: that axis is
// copied.  Validated by the caller: oh <= H, ow <= W, ry < H, rx < W, radii <= ECSEG_RESCALE_MAX_RADIUS.
hipError_t run_rescale_down(const uint8_t* img, int H, int W, int oh, int ow, const double* wy, int ry, const double* wx, int rx,
                            uint8_t* tmp, uint8_t* filtered, double* out, hipStream_t s);
// Device buffers of one down-scaling of an H x W image to oh x ow: run_rescale_down's arguments, wy and wx with room for the
// largest radius.
struct RescaleDownBufs { uint8_t* img; uint8_t* tmp; uint8_t* filtered; double* v; double* wy; double* wx; };
inline RescaleDownBufs rescale_down_bufs(Carver& c, int H, int W, int oh, int ow) {
    const size_t px = (size_t)H * W;
    RescaleDownBufs b;
    b.img = c.take<uint8_t>(px); b.tmp = c.take<uint8_t>(px); b.filtered = c.take<uint8_t>(px); b.v = c.take<double>((size_t)oh * ow);
    b.wy = c.take<double>(2 * ECSEG_RESCALE_MAX_RADIUS + 1); b.wx = c.take<double>(2 * ECSEG_RESCALE_MAX_RADIUS + 1);
    return b;
}
// Device buffers of one up-scaling of an H x W mask to oh x ow: the input `cleaned`, the warped values v, mm (~min and max of v as
// bit patterns), par and sz and out (the final 0 / 255 mask).
struct RescaleUpBufs { double* v; unsigned long long* mm; int32_t* par; int32_t* sz; uint8_t* out; uint8_t* cleaned; };
inline RescaleUpBufs rescale_up_bufs(Carver& c, int H, int W, int oh, int ow) {
    const size_t opx = (size_t)oh * ow;
    RescaleUpBufs b;
    b.cleaned = c.take<uint8_t>((size_t)H * W); b.out = c.take<uint8_t>(opx); b.par = c.take<int32_t>(opx); b.sz = c.take<int32_t>(opx);
    b.v = c.take<double>(opx); b.mm = c.take<unsigned long long>(2);
    return b;
}
// cleaned (H, W) uint8 on the device, oh >= H, ow >= W, oh * ow < 2^31.
hipError_t run_rescale_mask_up(const uint8_t* cleaned, int H, int W, int oh, int ow, int nuclei_size_t, const RescaleUpBufs& b, hipStream_t s);

}  // namespace ecseg
