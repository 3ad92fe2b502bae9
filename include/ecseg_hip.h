/*
 * ecseg_hip.h - C ABI of libecseg_hip.so: the MI355X (gfx950) implementation of ecSeg's metaseg hot path.
 *
 * The reference (UCRajkumar/ecSeg) is pure Python and has no FFI of its own; the boundary it exposes is three
 * Python call shapes plus a file contract.  Each entry point below names the reference
 * interface it stands in for (file:line relative to the reference repository).  The ctypes binding that a
 * maintainer would add on the reference side is shown in INTEGRATION.md.
 *
 * Conventions
 *   - plain C: opaque handle, plain pointers and sizes, no C++/torch types;
 *   - every call returns 0 on success or a negative ECSEG_E_* code; the text of the last failure is available
 *     from ecseg_last_error(); nothing throws across the ABI;
 *   - the caller owns host memory, the handle owns device memory and its HIP stream;
 *   - one handle per GPU; a handle is not thread-safe, different handles may be driven from different threads;
 *   - all calls are synchronous with respect to the host (results are complete on return);
 *   - "_dev" variants take DEVICE pointers (e.g. torch tensors' data_ptr) and run on the handle's stream without
 *     host copies; they still return only after the stream has drained unless stated otherwise.
 *   - images are row-major (H, W[, C]); label images are uint8 with values 0..3
 *     (0 background, 1 nucleus, 2 chromosome, 3 ecDNA: src/utils.py:128-131).
 */
#ifndef ECSEG_HIP_H
#define ECSEG_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 2 (round 3): ecseg_get_conv_launch_profile kinds 3 / 4 and fusion bits, images_per_group 0 = automatic, op code 9
 * (GLOBALPOOL), MAXPOOL honours `mode`, CONV accepts stride != 1, ecseg_npy_write_i64 / ecseg_png_write* /
 * ecseg_tiff_* / ecseg_allgather_records added.  ecseg_amd/_lib.py refuses a library whose version differs from the one it was written for. */
/* 3 (round 4): ecseg_segment_images_ex (per-image tie-risk counts, stitched probabilities). */
/* 4 (round 5): ecseg_op_desc gains `dilation`; op codes 10-12 (DWCONV, PRELU, LAYERNORM); ADD takes `mode` (add / multiply / subtract /
 * maximum / minimum) and broadcasts extents of 1; MAXPOOL honours pad_top / pad_left ('same' pooling); activation codes 7-14;
 * ECSEG_COMM_TIMEOUT_S bounds ecseg_comm_create / ecseg_allgather_records*. */
/* 5 (round 5): ecseg_meta_segment (pre-process + segment in one call), ecseg_prefetch_input, ecseg_host_alloc / ecseg_host_free
 * (page-locked host buffers); ecseg_create sets the device's scheduling flag to hipDeviceScheduleBlockingSync (see there). */
/* (round 6, still 5 - additions a round-5 caller never triggers: option "winograd" = 3 (the round's second option, which selected the superseded F(4x4) kernel path, went with that path: the key fails as unknown); ecseg_get_conv_launch_profile kinds 5 / 6
 * (the split kernels); CONV ops read their so far unused `mode` word as the horizontal stride / dilation rate (0 = as before); CONVT kernels larger than
 * their stride run phase by phase.) */
/* (still 5 - additive: ecseg_nuclei_regions and ecseg_nucleus_crops, the file-level interSeg driver; nothing existing changed.) */
/* (still 5 - additive: ecseg_fish_distances, the per-nucleus records of fish_distance_calculation; nothing existing changed.) */
/* (still 5 - additive: ecseg_fish_spots, the per-nucleus records, masks and boundaries of stat_fish, and ecseg_tiff_write_rgb8; ecseg_npy_write_i32_as_i64
 * beside ecseg_npy_write_i64; nothing existing changed.) */
/* (still 5 - additive: ecseg_fish_render, the three colour files of stat_fish for 3- and 4-channel images; nothing existing changed.) */
/* (still 5 - additive: ecseg_tiff_encode_bound, ecseg_tiff_encode and ecseg_fish_render_tiff, stat_fish's LZW TIFF files encoded on the
 * device; nothing existing changed.) */
/* (still 5 - additive: ecseg_png_labels_encode, ecseg_meta_segment_files with ecseg_get_file_timings, and ecseg_png_labels_stream_size:
 * `make metaseg`'s dapi TIFFs and label PNGs encoded on the device; nothing existing changed.) */
/* (still 5 - additive: ecseg_tiff_decode and ecseg_tiff_decode_routes, stat_fish's input TIFFs decoded on the device; nothing existing
 * changed.) */
/* (still 5 - additive: ecseg_tiff_decode_batch, ecseg_tiff_decode_batch_bytes, ecseg_tiff_decode_batch_routes and
 * ecseg_tiff_decode_batch_counts, many TIFF files decoded in one device call, a wave per strip of any file; nothing existing changed.) */
/* (still 5 - additive: ecseg_meta_segment_tiffs, ecseg_meta_segment_tiffs_files, ecseg_prefetch_tiffs and ecseg_get_read_timings,
 * `make metaseg`'s input TIFFs decoded on the device into the U-Net's batch; nothing existing changed.) */
/* (still 5 - additive: ecseg_ccl_pass_debug, one connected-component labelling pass alone with everything it produced read back, for
 * the tests of the labelling kernels; nothing existing changed.) */
/* (still 5 - additive: ecseg_meta_inference_stages_debug, a range of the six clean-up stages of meta_inference alone on given images, for
 * the tests of the kernels between the labelling passes; nothing existing changed.) */
/* (still 5 - additive: ecseg_png_channel_encode, ecseg_png_channel_bound and ecseg_overlay_files, `make meta_overlay`'s red and green
 * PNGs encoded on the device; nothing existing changed.) */
/* (still 5 - additive: ecseg_tiff_encode_batch, ecseg_tiff_encode_batch_bytes and ecseg_fish_render_tiff_batch, the TIFF files of many
 * stat_fish images encoded in one device call, a wave per strip of any file; nothing existing changed.) */
/* (still 5 - additive: ecseg_classify_nucleus_crops and ecseg_iseg_classifier_inputs_debug, interSeg's crops through both classifiers
 * without a host round trip; nothing existing changed.) */
/* (still 5 - additive: ecseg_marker_watershed_stages_debug and ecseg_marker_watershed_batch_stages_debug, the marker watershed with its
 * stage products (rw, filled, d2, lab) read back, for the tests of its kernels; nothing existing changed.) */
/* (still 5 - additive: option "tiff_deflate_on_device" with ecseg_tiff_decode_routes_ex, ecseg_tiff_decode_batch_routes_ex,
 * ecseg_tiff_decode_batch_counts_ex and ecseg_tiff_decode_batch_bytes_ex, Deflate strips decoded on the device behind an option that
 * is off by default; nothing existing changed.) */
/* (still 5 - additive: option "tiff_tiled_on_device" with ecseg_tiff_decode_routes_ex2, ecseg_tiff_decode_batch_routes_ex2,
 * ecseg_tiff_decode_batch_counts_ex2 and ecseg_tiff_decode_batch_bytes_ex2, tiled TIFF files decoded on the device behind an option
 * that is off by default; nothing existing changed.) */
/* (still 5 - additive: option "tiff_packbits_on_device" with ecseg_tiff_decode_routes_ex3, ecseg_tiff_decode_batch_routes_ex3,
 * ecseg_tiff_decode_batch_counts_ex3 and ecseg_tiff_decode_batch_bytes_ex3, PackBits files decoded on the device behind an option that
 * is off by default; ecseg_meta_segment_tiffs, ecseg_meta_segment_tiffs_files and ecseg_prefetch_tiffs read the three tiff_*_on_device
 * options of their handle; with every option at its default nothing changed.) */
/* (still 5 - additive: ecseg_interseg_batch, the regions, crops and classifiers of many interSeg images in one call; nothing existing
 * changed.  The number stays where every additive entry above left it: a caller of version 5 runs unchanged.) */
/* (still 5 - additive: ecseg_stitch_stages_debug, ecseg_preprocess_stages_debug and ecseg_otsu_debug, the stitch with its tie-risk count
 * over a whole batch in one launch, meta_preprocess with its histograms and thresholds, and Otsu alone on given histograms, for the
 * tests of csrc/stitch_preprocess_kernels.hip; nothing existing changed.) */
/* (still 5 - additive: ecseg_stat_fish_batch and ecseg_stat_fish_batch_bytes, the labelling, spot statistics, colour files and TIFF
 * encode of many stat_fish images in one call; nothing existing changed.) */
/* (still 5 - additive: ecseg_scratch_fill_debug, every scratch arena of the handle filled with one byte, for the tests that hold each
 * driver to its answer whatever an earlier call left there; nothing existing changed.) */
/* (still 5 - additive: ecseg_fish_distances_batch, the per-nucleus records of fish_distance_calculation for many images in one call;
 * nothing existing changed.) */
/* 6: the kinds word.  ecseg_tiff_decode_routes, ecseg_tiff_decode_batch_routes, ecseg_tiff_decode_batch_counts and
 * ecseg_tiff_decode_batch_bytes take a last argument `unsigned kinds` (ECSEG_TIFF_DEFLATE | ECSEG_TIFF_TILED | ECSEG_TIFF_PACKBITS; 0: the
 * answers they gave without it) and replace their twelve copies with the suffixes _ex (deflate), _ex2 (deflate, tiled) and _ex3
 * (deflate, tiled, packbits), which are gone: _exN(..., d, t, p) is now (..., d * ECSEG_TIFF_DEFLATE | t * ECSEG_TIFF_TILED |
 * p * ECSEG_TIFF_PACKBITS).  The three tiff_*_on_device options and every other entry point are as they were. */
#define ECSEG_ABI_VERSION 6

#define ECSEG_OK             0
#define ECSEG_E_INVALID     -1   /* bad argument / shape / plan */
#define ECSEG_E_HIP         -2   /* a HIP runtime call failed */
#define ECSEG_E_NOMODEL     -3   /* a model-dependent call before ecseg_model_load */
#define ECSEG_E_NOMEM       -4
#define ECSEG_E_UNSUPPORTED -5
#define ECSEG_E_IO          -6   /* a file could not be opened / read / written (host I/O entry points) */

typedef struct ecseg_ctx ecseg_ctx;

/* ---- lifetime ------------------------------------------------------------------------------------------- */
int         ecseg_abi_version(void);
/* SIDE EFFECT ON THE PROCESS: ecseg_create sets hipDeviceScheduleBlockingSync on the device - a device-wide, process-wide
 * setting: every HIP user of the process (torch tensors of an embedding application too) then SLEEPS while it waits for the GPU
 * instead of spinning (same wall time, one core less per waiting call).  ECSEG_SPIN_WAIT=1 in the environment leaves the runtime's
 * default alone - at your own risk: under the default mode hipFree was seen to hang for ever in ecseg_destroy after several
 * handles had been created and closed in one process (csrc/api.hip: ecseg_create).  ECSEG_DEBUG_CALLS=1 prints a host-side
 * timeline of every ecseg_meta_segment call on stderr. */
int         ecseg_create(ecseg_ctx** out, int device_id);
void        ecseg_destroy(ecseg_ctx* h);
const char* ecseg_last_error(ecseg_ctx* h);        /* h may be NULL: error of the last failed ecseg_create */
int         ecseg_device_name(ecseg_ctx* h, char* buf, int buflen);
/* The HIP stream all work of this handle is launched on (hipStream_t as void*), for event timing by the caller. */
void*       ecseg_stream(ecseg_ctx* h);

/* ---- model plan: replaces tf.keras.models.load_model (src/utils.py:27-33) -------------------------------- */
/* Kernel-level operators of the U-Net plan.  The host (ecseg_amd/keras_plan.py) lowers the Keras model_config
 * found in metaseg.h5 to this list; tensors are NHWC float32 "views" into device buffers so that Concatenate
 * costs nothing (producers write straight into the concatenated buffer). */
enum {
    ECSEG_OP_CONV      = 1,  /* Conv2D kh x kw, stride s, dilation d, zero padding (pad_top, pad_left), bias, activation; a Dense
                                layer is the 1x1 case on a (1, 1, features) tensor; a grouped convolution is one CONV per group
                                on channel views */
    ECSEG_OP_CONVT     = 2,  /* Conv2DTranspose kh x kw, stride s, crop (pad_top, pad_left), bias, activation */
    ECSEG_OP_MAXPOOL   = 3,  /* MaxPooling2D (mode 0) / AveragePooling2D (mode 1) kh x kw stride s; 'same': (pad_top, pad_left) window
                                positions before the input (the maximum / the average runs over the pixels inside the input) */
    ECSEG_OP_UPSAMPLE  = 4,  /* UpSampling2D x s, mode: 0 nearest, 1 bilinear (half-pixel centres) */
    ECSEG_OP_AFFINE    = 5,  /* y = act(x * scale[c] + shift[c]): BatchNormalization (inference), Rescaling */
    ECSEG_OP_ACT       = 6,  /* y = act(x) */
    ECSEG_OP_ADD       = 7,  /* y = act(a (+) b), (+) = `mode` (ECSEG_BIN_*: Add / Multiply / Subtract / Maximum / Minimum); an extent of
                                1 in either input (h, w or c) is broadcast - the squeeze-and-excite x * s(1, 1, c) */
    ECSEG_OP_COPY      = 8,  /* y = x (materialise a view, ZeroPadding2D / Cropping2D via offsets) */
    ECSEG_OP_GLOBALPOOL = 9, /* GlobalMaxPooling2D (mode 0) / GlobalAveragePooling2D (mode 1): (h, w, c) -> (1, 1, c) */
    ECSEG_OP_DWCONV    = 10, /* DepthwiseConv2D kh x kw, stride s, dilation, zero padding (pad_top, pad_left), depth multiplier
                                `mode` (>= 1; output channel = input channel * mode + j), kernel (kh, kw, cin, mode), bias,
                                activation; SeparableConv2D = DWCONV followed by a 1x1 CONV */
    ECSEG_OP_PRELU     = 11, /* y = x > 0 ? x : a * x; w0 = a: mode 0 one slope per channel (shared_axes [1, 2]), mode 1 one per
                                (y, x, channel) of the patch */
    ECSEG_OP_LAYERNORM = 12  /* LayerNormalization over the channel axis of every pixel: (x - mean) / sqrt(var + alpha) * w0[c] +
                                w1[c] (alpha = epsilon; w0 / w1 = -1: no scale / no centre) */
};
/* RELU_CLIP: min(max(x, 0), alpha) (ReLU(max_value) - relu6); ELU: x > 0 ? x : alpha (exp(x) - 1); HARD_SIGMOID: Keras' clip(0.2 x +
 * 0.5, 0, 1); GELU: the exact erf form (Keras' default approximate=False) */
enum { ECSEG_ACT_LINEAR = 0, ECSEG_ACT_RELU = 1, ECSEG_ACT_SOFTMAX = 2, ECSEG_ACT_SIGMOID = 3,
       ECSEG_ACT_LEAKY = 4, ECSEG_ACT_TANH = 5, ECSEG_ACT_ELU = 6, ECSEG_ACT_RELU_CLIP = 7, ECSEG_ACT_SWISH = 8,
       ECSEG_ACT_HARD_SIGMOID = 9, ECSEG_ACT_SOFTPLUS = 10, ECSEG_ACT_SELU = 11, ECSEG_ACT_GELU = 12, ECSEG_ACT_EXP = 13,
       ECSEG_ACT_SOFTSIGN = 14 };
/* ECSEG_OP_ADD `mode` */
enum { ECSEG_BIN_ADD = 0, ECSEG_BIN_MUL = 1, ECSEG_BIN_SUB = 2, ECSEG_BIN_MAX = 3, ECSEG_BIN_MIN = 4 };

typedef struct ecseg_tensor_desc {
    int32_t buffer;     /* index of the device buffer this view lives in */
    int32_t h, w, c;    /* per-patch logical shape */
    int32_t c_stride;   /* floats between consecutive pixels in the buffer (>= c_offset + c) */
    int32_t c_offset;   /* first channel of the view inside a pixel */
} ecseg_tensor_desc;

typedef struct ecseg_op_desc {
    int32_t op;
    int32_t in0, in1;           /* tensor indices (in1 = -1 when unused) */
    int32_t out;
    int32_t kh, kw, stride;
    int32_t pad_top, pad_left;  /* CONV: zero padding before; CONVT: rows/cols cropped from the full output;
                                   COPY: offset of the input inside the output (>0) or crop (<0) */
    int32_t act;
    int32_t mode;               /* UPSAMPLE interpolation; MAXPOOL / GLOBALPOOL: 0 max, 1 average; ADD: ECSEG_BIN_*; DWCONV: depth
                                   multiplier; PRELU: 0 per channel, 1 per element; CONV (round 6): per-axis strides / dilation
                                   rates - bits 0-7 the HORIZONTAL stride, bits 8-15 the HORIZONTAL dilation rate where they differ
                                   from the vertical ones in `stride` / `dilation` (0: the same; such layers run on the scalar
                                   kernel, any taps / channels) */
    int32_t w0, w1;             /* weight array indices: CONV/CONVT kernel + bias (-1 none); AFFINE scale + shift */
    float   alpha;              /* LEAKY slope / RELU_CLIP maximum / ELU alpha; LAYERNORM epsilon */
    int32_t dilation;           /* CONV / DWCONV: dilation_rate (0 or 1: none) */
} ecseg_op_desc;

/* weights[i] is a host float32 array of weight_len[i] elements, Keras layout
 * (Conv2D kernel HWIO; Conv2DTranspose kernel (kh, kw, out, in)).  The library re-lays kernels out for its MFMA
 * kernels once, on the device.  input_tensor must be (256, 256, 1)-shaped per patch for the segment calls. */
int ecseg_model_load(ecseg_ctx* h,
                     const ecseg_tensor_desc* tensors, int n_tensors, int n_buffers,
                     const ecseg_op_desc* ops, int n_ops,
                     const float* const* weights, const int64_t* weight_len, int n_weights,
                     int input_tensor, int output_tensor);
int ecseg_model_flops_per_patch(ecseg_ctx* h, double* flops);   /* algorithmic 2*MAC count of the loaded plan */

/* ---- model.predict_on_batch(uint8[N,256,256,C]) -> float32[N,256,256,K] (src/utils.py:115) --------------- */
int ecseg_forward_patches(ecseg_ctx* h, const uint8_t* patches_nhwc, int n, float* out_nhwc);
/* Same with float32 inputs (N, H, W, C): the interSeg classifier ecseg_c is fed normalised floats
 * (preprocess_ecseg_c, src/utils.py:166-173; src/interseg.py:167-168). */
int ecseg_forward_patches_f32(ecseg_ctx* h, const float* patches_nhwc, int n, float* out_nhwc);
/* Debug/parity: copy any plan tensor (compact NHWC float32) after the last forward of n patches. */
int ecseg_read_tensor(ecseg_ctx* h, int tensor, int n, float* out_nhwc);

/* ---- meta_segment minus file I/O (src/utils.py:111-119) + count_cc(I==3)[0] (src/metaseg.py:46) ---------- */
/* gray: n_img pre-processed uint8 images (H, W) (the output of meta_preprocess).  Steps on the device:
 * im2patches_overlap (src/image_tools.py:148-186) -> U-Net -> patches2im_overlap (:188-252) -> img_as_ubyte ->
 * argmax (src/utils.py:117-118) -> meta_inference (src/image_tools.py:15-84) -> count_cc(I==3)[0].
 * labels_raw (optional, may be NULL) receives the argmax labels, labels_post the post-processed labels,
 * n_ec one int32 per image. */
int ecseg_segment_images(ecseg_ctx* h, const uint8_t* gray, int n_img, int H, int W,
                         uint8_t* labels_raw, uint8_t* labels_post, int32_t* n_ec);
int ecseg_segment_images_dev(ecseg_ctx* h, const uint8_t* gray_dev, int n_img, int H, int W,
                             uint8_t* labels_raw_dev, uint8_t* labels_post_dev, int32_t* n_ec_dev);
/* ecseg_segment_images with two optional extra outputs (either may be NULL):
 *   tie_risk  one int32 per image: the number of pixels whose two largest uint8-quantised probabilities (the values
 *             np.argmax sees, src/utils.py:117-118) differ by at most 1 - the pixels whose label a last-bit difference between
 *             two float32 evaluations of the network (this library, TensorFlow, a CPU port) can flip; an upper bound on the
 *             raw-label disagreement of such evaluations for this image;
 *   probs     float32 (n_img, H, W, 4): the stitched probabilities themselves (patches2im_overlap, src/utils.py:116; never-
 *             written canvas pixels are 0), for comparison with the reference's own stitched output. */
int ecseg_segment_images_ex(ecseg_ctx* h, const uint8_t* gray, int n_img, int H, int W,
                            uint8_t* labels_raw, uint8_t* labels_post, int32_t* n_ec, int32_t* tie_risk, float* probs);
/* Upper bound on images (of 35 windows) per internal U-Net launch group.  Default and n == 0: automatic - as many as fit
 * ~48 GB of activations, between 16 and 64 (16 for the canonical base-64 U-Net, 32 for base 32, 64 for base 16). */
int ecseg_set_images_per_group(ecseg_ctx* h, int n);
/* Tuning knobs: "overlap_post" (1: clean-up + count of group g run on a second stream beside the U-Net of group g+1;
 * 0 (default): everything on one stream - measured equal, the MFMA convs already fill the chip), "post_chunk"
 * (images per post-processing launch set), "images_per_group", "winograd" (3x3 / stride-1 / 'same'
 * convolutions: 2 (default) Winograd F(4x4,3x3) where the layer allows it (extents % 16, Cin % 4 and >= 8, Cout % 32), else
 * F(2x2,3x3); 1: F(2x2,3x3); 0: the direct implicit-GEMM kernel; all three are fp32 MFMA kernels; 3 (round 6): as 2, with the F(4x4) layers of whole
 * 64-channel output blocks and the 2x2 / stride-2 up-convolutions on the BF16 matrix pipe - both operands split exactly into three bf16 pieces, six of the
 * nine piece products, float32 accumulation: float32-accurate; the split filter images are made on the device when the option is set), "fuse_first" (1 (default): the network's first layer - Conv2D 3x3 'same', 1 -> 16 channels - is computed
 * by the 16 -> 16 conv_wino16_kernel convolution behind it, on the matrix cores, straight into that kernel's halo buffer; the 16-channel tensor
 * between the two never exists in memory; 0: conv_first_kernel writes it), "wino16" (1 (default):
 * F(2x2,3x3) layers with 16 or 32 input and output channels and extents >= 16 x 32 take conv_wino16_kernel - 16x16x4 MFMAs,
 * register output stage; 0: the 32-wide F(2x2) kernels), "wino_resident" (1 (default): the remaining F(2x2) layers with <= 32
 * input and <= 32 output channels keep their filter in registers and walk a tile row; 0: the streaming F(2x2) kernel - the
 * results of the two are identical), "wino4_split" (1 (default): an F(4x4) layer with exactly 32 output channels splits the 8 input
 * channels of a group between the two channel-half waves of a transform row; 0: the upper waves multiply the zero padding
 * of the 64-channel block), "fuse_pool" (1
 * (default): a MaxPooling2D(2x2, stride 2) that directly follows a Winograd (F(4x4) or F(2x2)) convolution is written by that
 * convolution's output stage; 0: separate max-pool kernel), "fuse_head" (1 (default): a 1x1 convolution with <= 4 output channels that
 * is the only reader of a 64-channel F(4x4) convolution (or of a 16 / 32-channel conv_wino16_kernel convolution) is computed by
 * that convolution's output stage and the feature tensor is never written; 0: separate head kernel), "crop" (1 (default): in ecseg_segment_images the last
 * full-resolution convolutions (F(4x4): 16x16 regions; conv_wino16_kernel: 16x32 blocks; 2x2 up-convolutions: input tiles)
 * compute only the parts of every window that the stitch (or the halo of the convolutions behind them) reads - 72 % of them
 * at 1040x1392, and their Winograd tiles read zeros outside the receptive field of those parts ("crop_mask", 1 (default)), so the result
 * is a pure function of the image: independent of batch position, window lanes and of what ran before; it agrees with whole windows
 * (0) to float32 rounding, i.e. labels can differ at near-ties of the quantised probabilities), "unet_lanes" (0 (default): automatic -
 * a launch group of <= 70 windows (one or two 1040x1392 images) runs its U-Net as two window lanes on their own streams, which fills
 * the half-empty last round of workgroups of the deep layers (one image: 11.3 -> 10.4 ms); 1..8: that many lanes; results are
 * bit-identical for every value), "blocking_wait" (1 (default): the wait for a launch group sleeps on an event created
 * with hipEventBlockingSync; 0: hipStreamSynchronize), "min_cut_lds_pixels" (0 .. ECSEG_MIN_CUT_LDS_PIXELS (default): windows of
 * ecseg_min_cut with more pixels than this keep their state in global memory instead of LDS; the results do not depend on it),
 * "min_cut_centers_lds_pixels" (0 .. ECSEG_MIN_CUT_CENTERS_LDS_PIXELS (default): the same for the crops of ecseg_min_cut_regions),
 * "tiff_deflate_on_device" (0 (default): ecseg_tiff_decode and ecseg_tiff_decode_batch leave Deflate files to the host,
 * ECSEG_E_UNSUPPORTED; 1: they decode them on the device - see "TIFF files decoded on the device" below), "tiff_tiled_on_device"
 * (0 (default): the two leave tiled files to the Python reader, ECSEG_E_UNSUPPORTED without a shape; 1: they decode them on the
 * device - the same section), "tiff_packbits_on_device" (0 (default): the two leave PackBits files to the Python reader,
 * ECSEG_E_UNSUPPORTED without a shape; 1: they decode them on the device - the same section). */
int ecseg_set_option(ecseg_ctx* h, const char* key, int value);

/* ---- meta_preprocess (src/image_tools.py:86-101) ---------------------------------------------------------- */
/* img: n_img images (H, W, C) of uint8 (bytes_per_sample 1) or uint16 (2), C in {1,3,4}.  u16 -> u8 as
 * cv2.convertScaleAbs(alpha=255/65535); channel 2 when C > 1; Otsu; inverted when more than half is white.
 * gray_out: (n_img, H, W) uint8; inverted_out (optional) one flag per image. */
int ecseg_preprocess(ecseg_ctx* h, const void* img, int n_img, int H, int W, int C, int bytes_per_sample,
                     uint8_t* gray_out, int32_t* inverted_out);

/* ---- meta_segment of a batch in one call (src/utils.py:105-124 minus imread / imwrite, + src/metaseg.py:46) ---------- */
/* img as for ecseg_preprocess.  pre_process (src/utils.py:112) -> patches -> U-Net -> stitch -> argmax -> meta_inference ->
 * count_cc(I==3)[0] without the pre-processed images leaving the device in between: what `make metaseg` calls per batch.
 * gray_out (optional): the pre-processed images (src/utils.py:122-123 writes dapi/<name> from them), copied back under
 * the U-Net; labels_post, n_ec, tie_risk (optional) as for ecseg_segment_images_ex.  Results are identical to
 * ecseg_preprocess followed by ecseg_segment_images_ex. */
int ecseg_meta_segment(ecseg_ctx* h, const void* img, int n_img, int H, int W, int C, int bytes_per_sample,
                       uint8_t* gray_out, uint8_t* labels_post, int32_t* n_ec, int32_t* tie_risk);

/* Names the raw images of the ecseg_meta_segment call AFTER the coming one (page-locked memory, same layout, `bytes` in total):
 * the coming call uploads them on a stream of their own under its kernels, the call after it recognises them by (pointer, size)
 * and skips its own upload - the host <-> device copies of batch k + 1 overlap the kernels of batch k on ONE handle.  The
 * images must not change between the two calls; a call with other images uploads as always and drops what was sent ahead.
 * Results are those of calls without it. */
int ecseg_prefetch_input(ecseg_ctx* h, const void* img, size_t bytes);

/* ---- page-locked host buffers ------------------------------------------------------------------------------ */
/* Host pointers handed to any entry point may be ordinary (pageable) memory.  Buffers from ecseg_host_alloc make the
 * host <-> device copies DMA transfers (about 2x the pageable rate, and the gray_out copy of ecseg_meta_segment then really
 * overlaps the U-Net).  Free with ecseg_host_free before ecseg_destroy.  Unlike every other entry point these two may be called
 * from another thread while the handle is inside a call (they use only its device number); a failure is reported by the
 * return code alone (ECSEG_E_NOMEM / ECSEG_E_HIP), not through ecseg_last_error. */
int ecseg_host_alloc(ecseg_ctx* h, size_t bytes, void** out);
int ecseg_host_free(ecseg_ctx* h, void* p);

/* u16_to_u8 alone (src/image_tools.py:98-101, used by split_FISH_channels :142): count uint16 samples ->
 * uint8 with cv2.convertScaleAbs(alpha = 255/65535) rounding. */
int ecseg_u16_to_u8(ecseg_ctx* h, const uint16_t* in, long long count, uint8_t* out);

/* ---- stitched probabilities -> labels only (src/utils.py:116-118), for parity of the tail in isolation ---- */
/* probs: (n_img * n_patches, 256, 256, 4) float32 patch predictions in reference patch order. */
int ecseg_stitch_argmax(ecseg_ctx* h, const float* probs, int n_img, int H, int W, uint8_t* labels_raw);
/* Test-only: the stitch kernels over the whole batch, one launch each (the pipeline stitches one launch group at a time, so only here
 * does a thread's grid-stride walk reach a second image once n_img * H * W passes 16384 workgroups of 256 pixels).  probs:
 * (n_img * n_patches, 256, 256, chan_stride) float32, chan_stride >= 4, channels 4 .. chan_stride - 1 never read.  Every output may
 * be NULL: labels (n_img, H, W) uint8, the quantised first-maximum argmax; tie_risk (n_img) int32, as ecseg_segment_images_ex counts
 * it (written pixels whose two largest quantised values differ by at most 1); probs_out (n_img, H, W, 4) float32, the stitched
 * probabilities, 0 where the stitch writes nothing.  ECSEG_E_INVALID: chan_stride < 4, a NULL probs, an image below 256 x 256. */
int ecseg_stitch_stages_debug(ecseg_ctx* h, const float* probs, int chan_stride, int n_img, int H, int W, uint8_t* labels, int32_t* tie_risk,
                              float* probs_out);
/* Test-only: ecseg_preprocess with what it leaves on the way.  img, n_img, H, W, C, bytes_per_sample as there.  Every output may be
 * NULL: hist (n_img, 256) uint32, the histogram of the 8-bit image before the inversion; threshold (n_img) int32, Otsu's threshold;
 * inverted (n_img) int32; gray (n_img, H, W) uint8 as ecseg_preprocess returns it. */
int ecseg_preprocess_stages_debug(ecseg_ctx* h, const void* img, int n_img, int H, int W, int C, int bytes_per_sample, uint32_t* hist,
                                  int32_t* threshold, int32_t* inverted, uint8_t* gray);
/* Test-only: the Otsu kernel of ecseg_preprocess alone on given histograms.  hist: (n_img, 256) uint32; px: (n_img) int64, the pixel
 * count of each image - it must be the sum of its histogram and lie in 1 .. 2^31 - 1, anything else is ECSEG_E_INVALID.  threshold,
 * inverted (n_img) int32, either may be NULL: Otsu's threshold and the "more than half of the pixels lie above it" flag. */
int ecseg_otsu_debug(ecseg_ctx* h, const uint32_t* hist, int n_img, const int64_t* px, int32_t* threshold, int32_t* inverted);

/* ---- meta_inference(I) (src/image_tools.py:15-84) + count_cc(I==3)[0] on given label images -------------- */
int ecseg_meta_inference(ecseg_ctx* h, const uint8_t* labels_in, int n_img, int H, int W,
                         uint8_t* labels_out, int32_t* n_ec);
int ecseg_meta_inference_dev(ecseg_ctx* h, const uint8_t* labels_in_dev, int n_img, int H, int W,
                             uint8_t* labels_out_dev, int32_t* n_ec_dev);
/* Test-only: stages first..last of meta_inference alone.  labels_in is the input of stage `first`, labels_out the image after stage
 * `last`: 1 fill_holes(1), 2 fill_holes(2), 3 size_thresh + ec_band_removal (:41-64), 4 the nucleus-in-metaphase test (:66-81),
 * 5 merge_comp(1), 6 merge_comp(2) + the final ecDNA dilation (:83).  1..6 is ecseg_meta_inference without the count.  kill_out (may
 * be NULL; (n_img, H, W), written when the range holds stage 4): 1 at the pixels of the nuclei the test erases, 0 elsewhere.
 * ECSEG_E_INVALID: a range outside 1..6 or first > last. */
int ecseg_meta_inference_stages_debug(ecseg_ctx* h, const uint8_t* labels_in, int n_img, int H, int W, int first, int last,
                                      uint8_t* labels_out, uint8_t* kill_out);

/* ---- counting (src/image_tools.py:103-134) ---------------------------------------------------------------- */
/* masks are uint8 (non-zero = True), (n_img, H, W). */
/* count_cc (:114-119): n_out = number of 8-connected components; px_out = total pixels, or -1 where the
 * reference returns float 0.0 (no component, or a mask without any background pixel). */
int ecseg_count_cc(ecseg_ctx* h, const uint8_t* mask, int n_img, int H, int W, int32_t* n_out, int64_t* px_out);
/* Connected-component labels themselves: 0 background, else 1 + raster index of the component's first pixel
 * (connectivity 4 or 8); used by the parity tests of the union-find kernels. */
int ecseg_ccl_labels(ecseg_ctx* h, const uint8_t* mask, int n_img, int H, int W, int connectivity,
                     int32_t* labels_out);
/* Test-only: ONE labelling pass of the post-processing (struct CclPass of csrc/ccl.h, field by field) run alone, and
 * everything it produced read back whole.  lut: key of a pixel = byte (value & 3) of it, or value != 0 when it is 0xffffffff;
 * conn 4 | 8; stat bit 0 area, bit 1 coordinate sums; aux_mode 0 none, 1 image border, 2 value == aux_c, 3 bits 0-4 of aux_img;
 * need bit 0 components per key, 1 pixels per key, 2 last root + 1, 3 the two root lists; n_queries <= 5 flag queries (roots with
 * key == query_key, 0 = any, whose flag word holds all bits of query_need).
 * ECSEG_E_INVALID: conn not 4 / 8, aux_mode 3 without aux_img, lists with conn 4 (their capacity bounds 8-connected components only),
 * queries after a count_only pass (it writes no flag words). */
typedef struct ecseg_ccl_pass_desc {
    uint32_t lut;
    int32_t conn, stat, aux_mode, aux_c, need, count_only, sparse, allow_full;
    int32_t n_queries, query_key[5];
    uint32_t query_need[5];
} ecseg_ccl_pass_desc;
/* All of them required, (n_img, H, W) unless said otherwise.  root: -1 where the key is 0, else the pixel index (in the image) of the
 * component's root = its first pixel in raster order; after a count_only pass the pixel's own index where it was counted as a
 * root, else -1.  area / sumy / sumx / flag: the component's at its root pixel, 0 elsewhere.  counters: (n_img, 16) components
 * per key 1..3, pixels per key 1..3, last root + 1, entries of list1 / list2, the 5 query answers, 2 spare.  list1 / list2:
 * (n_img, H*W/4 + (H+W)/2 + 4) roots of value 1 / 2 in no particular order, -1 beyond their counts.  tile_any: (n_img,
 * ceil(H/32), ceil(W/64)) 0 no keyed pixel, 1 some, 2 a full tile treated as one node. */
typedef struct ecseg_ccl_pass_out {
    int32_t* root; uint32_t* area; uint64_t* sumy; uint64_t* sumx; uint32_t* flag;
    int32_t* counters; int32_t* list1; int32_t* list2; uint8_t* tile_any;
} ecseg_ccl_pass_out;
int ecseg_ccl_pass_debug(ecseg_ctx* h, const uint8_t* key_img, const uint8_t* aux_img, int n_img, int H, int W,
                         const ecseg_ccl_pass_desc* pass, const ecseg_ccl_pass_out* out);
/* Test-only: waits for the handle's streams, fills the whole present capacity of every scratch arena of the drivers with `byte`
 * (0 .. 255) and waits again.  No arena grows, shrinks or is freed.  What a call leaves in an arena for a later one is withdrawn as
 * its owner withdraws it: the region map of ecseg_nuclei_regions (ecseg_nucleus_crops then fails with "no region map on the
 * handle"), whatever was sent or decoded ahead for the next ecseg_meta_segment call, and the layout of the clean-up workspace, which
 * the next call that needs it makes anew.  Every driver must answer afterwards as on a fresh handle. */
int ecseg_scratch_fill_debug(ecseg_ctx* h, int byte);
/* count_colocalization (:126-134) */
int ecseg_count_colocalization(ecseg_ctx* h, const uint8_t* ob1, const uint8_t* ob2, int n_img, int H, int W,
                               int32_t* n_out);
/* count_HSR (:103-112) */
int ecseg_count_hsr(ecseg_ctx* h, const uint8_t* chrom, const uint8_t* fish, int n_img, int H, int W,
                    int size_threshold, int32_t* n_out);

/* ---- meta_overlay row (src/meta_overlay.py:59-95, src/image_tools.py:136-146) ----------------------------- */
/* labels: (n_img, H, W) uint8 post-processed labels (what read_seg loads, src/utils.py:125-132): 1 nucleus, 2 chromosome,
 * 3 ecDNA; every other byte, those above 3 included, is background, as with the reference's labels == 1 / 2 / 3;
 * rgb: (n_img, H, W, C>=2) uint8, channel 0 red, channel 1 green; sensitivity: color_sensitivity.
 * out: n_img rows of 12 int64, in final CSV column order (src/meta_overlay.py:98-100):
 *   [0,1]  count_cc(ec)                 (n, px)   px = -1 stands for the reference's float 0.0
 *   [2,3]  count_cc(green & ~nuclei & ~chrom)
 *   [4,5]  count_cc(red   & ~nuclei & ~chrom)
 *   [6]    coloc(ec, green')   [7] coloc(ec, red')   [8] coloc(green' & ~chrom, red' & ~chrom)
 *   [9]    coloc(ec, red' & green')   [10] HSR(red)   [11] HSR(green)          (x' = x & ~nuclei) */
int ecseg_overlay(ecseg_ctx* h, const uint8_t* labels, const uint8_t* rgb, int n_img, int H, int W, int C,
                  int sensitivity, int hsr_size_threshold, int64_t* out);

/* ---- interSeg: nuclei and their crops (src/interseg.py:113-235, im2patches_overlap :27-46) --------------------------- */
/* Replaces measure.label(seg, connectivity=None) + measure.regionprops + the brightness gate (src/interseg.py:121-134) for
 * ONE image.  seg: (H, W) uint8 nucleus mask (what stat_fish writes as annotated/<name>/<name>_segmentation.tif, 0 / 255);
 * img: (img_h, img_w, C) uint8 with img_h >= H, img_w >= W - only I[:H, :W] is read (src/interseg.py:116-117).
 * Regions are the 8-connected components of seg != 0 in skimage's order (raster order of their first pixel); a seg holding
 * two different non-zero values (an instance-id map, which skimage would label by value) is refused with ECSEG_E_INVALID.
 * *n_regions = the number of regions; records (capacity x 8 int64) receive, when n_regions <= capacity, per region:
 *   [0] area  [1] min row  [2] min col  [3] max row + 1  [4] max col + 1   (regionprops' area and bbox)
 *   [5] sum of rows  [6] sum of columns  (centroid = sum / area; nucleus_center = floor of both)
 *   [7] sum of channel `channel0` of img inside the region (the gate of :134 is 4 * [7] < 51 * [0]).
 * When n_regions > capacity nothing is written: call again with a buffer of n_regions records.  The region label map and
 * I[:H] stay on the handle for ecseg_nucleus_crops until the next ecseg_nuclei_regions call. */
int ecseg_nuclei_regions(ecseg_ctx* h, const uint8_t* seg, int H, int W, const uint8_t* img, int img_h, int img_w, int C,
                         int channel0, int capacity, int64_t* records, int32_t* n_regions);
/* The crops of src/interseg.py:131-133,150-152 (whole bbox) and :190-194 / :27-46 (256-stride tiles of a larger bbox):
 * crops: n_crops x (region, y0, x0, h, w) int32, 1 <= h, w <= 256, inside the last ecseg_nuclei_regions image.  Crop k =
 * the window with every pixel outside region `region` zeroed, channels channel_order[0..2] of img (the (fish, 1 - fish, 2)
 * reorder of :119), resized to 256 x 256 like resize(.., (256, 256), preserve_range=True).astype('uint8') with the exact
 * affine map (scale h / 256; bilinear, 'reflect' inside the window; integer arithmetic, truncated).
 * out: (n_crops, 256, 256, 3) uint8; channel_max: (n_crops, 3) int32, the maximum of every output channel (the empty-tile
 * test of :199 and the centromere gate of :160). */
int ecseg_nucleus_crops(ecseg_ctx* h, const int32_t* crops, int n_crops, const int32_t* channel_order, uint8_t* out,
                        int32_t* channel_max);
/* The crops of ecseg_nucleus_crops through the two classifiers without leaving the device (src/interseg.py:153-170,199-210).
 * h: the handle that holds the region map; model_i: the handle with the ecSeg-i plan ((256, 256, 1) -> 3 values; may be h itself);
 * model_c: the handle with the ecSeg-c plan ((256, 256, 3) -> 1 value), or NULL.  All on one device.  crops, n_crops, channel_order:
 * as ecseg_nucleus_crops, with its checks and its chunks of 256 crops; from_patches: one byte per crop, non-zero for a tile of a
 * nucleus larger than 256 px; centromeric: non-zero when ecSeg-c applies to this image (a centromeric probe and a passed quality
 * score).  Per chunk the maxima come back (the call's one wait per chunk before the models run), and the host chooses: ecSeg-i
 * runs for every crop but a from_patches crop whose three maxima are 0; ecSeg-c for a crop ecSeg-i runs for when centromeric is
 * set, model_c is given and channel_max[1] > 10.  One kernel then writes (float)channel 0 of the chosen crops into the ecSeg-i
 * plan's input and round(x / max_c * 255) / 255 (float32, half to even, x / 0 = NaN) of every channel into the ecSeg-c plan's
 * (src/utils.py:166-173), and each plan runs on its own handle's stream in runs of at most that handle's windows per group.
 * channel_max (n_crops, 3) int32; pred_i (n_crops, 3) float32 and ran_i (n_crops) bytes; pred_c (n_crops) float32 (may be NULL
 * without model_c) and ran_c (n_crops) bytes: ran_* is 1 where that model ran, and the rows of pred_* where it did not are left as
 * they were.  crops_out: NULL, or (n_crops, 256, 256, 3) uint8 filled as ecseg_nucleus_crops fills `out`.
 * Device time (ecseg_get_timings): on h, ECSEG_T_COUNT the crop kernels and ECSEG_T_TILE the input kernel; on each model handle,
 * ECSEG_T_UNET its plan runs (h's own when it is model_i).  ECSEG_E_INVALID: the argument errors of ecseg_nucleus_crops, a model
 * handle without a plan or with one of another shape (the message names the model), handles on different devices. */
int ecseg_classify_nucleus_crops(ecseg_ctx* h, ecseg_ctx* model_i, ecseg_ctx* model_c, const int32_t* crops, int n_crops,
                                 const int32_t* channel_order, const uint8_t* from_patches, int centromeric, int32_t* channel_max,
                                 float* pred_i, uint8_t* ran_i, float* pred_c, uint8_t* ran_c, uint8_t* crops_out);
/* For the tests of the input kernel alone: crops (k, 256, 256, 3) uint8 and channel_max (k, 3) as given, 1 <= k <= 256; sel_i / sel_c:
 * n_i / n_c <= 256 crop indices in [0, k), any order, repeats allowed -> out_i (n_i, 256, 256) float32, out_c (n_c, 256, 256, 3)
 * float32, what ecseg_classify_nucleus_crops would write into the two plans' inputs.  Device time in ECSEG_T_TILE. */
int ecseg_iseg_classifier_inputs_debug(ecseg_ctx* h, const uint8_t* crops, int k, const int32_t* channel_max, const int32_t* sel_i,
                                       int n_i, const int32_t* sel_c, int n_c, float* out_i, float* out_c);
/* ecseg_nuclei_regions, the crop windows of src/interseg.py:150-154,190-194 and ecseg_classify_nucleus_crops for n_images images in
 * ONE call: per image exactly the records and the classifier outputs those calls give for it alone.
 * packed: packed_bytes bytes holding, per image, the uint8 image (H, W, C), C >= 3, and its uint8 segmentation (h, w), h <= H,
 * w <= W (16-bit images are converted by the caller, as for ecseg_nuclei_regions).  images: n_images x 8 int64 rows
 * (image offset, H, W, C, segmentation offset, h, w, run_c).  The 2 n_images rasters lie in the order image 0, segmentation 0,
 * image 1, ...: each starts at or after the end of the one in front (ecseg_marker_watershed_batch's rule: back to back, gaps allowed,
 * no overlap).  run_c: 1 where ecSeg-c applies to that image (a passed quality score); ignored when model_c is NULL.  fish_index 0 / 1:
 * the channel the gate sums, and the crops' channels are (fish_index, 1 - fish_index, 2).  h, model_i, model_c: as
 * ecseg_classify_nucleus_crops; the region map ecseg_nuclei_regions left on h is not touched.
 * out: n_images x 8 int32 rows
 *   [0] status: ECSEG_ISEG_OK; ECSEG_ISEG_INSTANCE_IDS - two different non-zero values, [5] the smallest and [6] the largest (the
 *       refusal of ecseg_nuclei_regions, for this image only); ECSEG_ISEG_RECORDS_OVERFLOW / ECSEG_ISEG_CROPS_OVERFLOW - its
 *       records / crops do not fit what is left of record_capacity / crop_capacity
 *   [1] its regions   [2] its first record in `records`, -1 unless OK or CROPS_OVERFLOW   [3] its crops, -1 where they were not
 *   counted   [4] its first crop in the per-crop arrays, -1 unless OK   [7] 0.
 * Capacities are handed out in image order and nothing is ever truncated: an image whose regions do not fit takes no record and
 * the images behind it go on (one whose regions fit takes their room whatever its status becomes); the same for the crops of the
 * images that are OK so far.  Call again for the reported images with [1] / [3] entries of room.
 * records (record_capacity x 8 int64): the layout of ecseg_nuclei_regions, region indices restart at 0 per image.  Per crop, in
 * image order, then region order, then window order (crop_capacity entries each): crop_region (its region), channel_max (x 3),
 * ran_i, pred_i (x 3), ran_c, pred_c (may be NULL without model_c) as ecseg_classify_nucleus_crops writes them.  The classifier
 * chunks of 256 crops are filled across image boundaries.
 * One synchronous call, scratch from the call arena: the masks are padded to the largest (h, w) of the call and labelled as one
 * same-shape batch, 9 bytes per padded pixel besides the rasters and one chunk of crops; above 8 GiB, or 2^31 padded pixels, the
 * call runs consecutive images in several groups (the classifier chunks are then filled per group).  Device time as
 * ecseg_classify_nucleus_crops, the labelling and statistics in ECSEG_T_COUNT too.  ECSEG_E_INVALID: a null pointer that is
 * needed, n_images outside 0 .. ECSEG_INTERSEG_BATCH_MAX_IMAGES, a negative capacity, fish_index not 0 / 1, a row with an extent
 * < 1, C outside 3 .. 256, a segmentation larger than its image, 2^31 pixels or more, run_c not 0 / 1, a raster that overlaps the
 * one in front or leaves packed (the message names the image), and the model errors of ecseg_classify_nucleus_crops. */
#define ECSEG_INTERSEG_BATCH_MAX_IMAGES 1024
#define ECSEG_ISEG_OK               0
#define ECSEG_ISEG_INSTANCE_IDS     1
#define ECSEG_ISEG_RECORDS_OVERFLOW 2
#define ECSEG_ISEG_CROPS_OVERFLOW   3
int ecseg_interseg_batch(ecseg_ctx* h, ecseg_ctx* model_i, ecseg_ctx* model_c, const uint8_t* packed, long long packed_bytes,
                         const int64_t* images, int n_images, int fish_index, int record_capacity, int crop_capacity, int32_t* out,
                         int64_t* records, int32_t* crop_region, int32_t* channel_max, float* pred_i, uint8_t* ran_i, float* pred_c,
                         uint8_t* ran_c);

/* ---- fish_distance_calculation: per-nucleus FISH - centromere distances (src/fish_distance_calculation.py:16-46) --------- */
/* Replaces, for ONE image, the loop over regionprops(segmentation) (:19), the gate on lsq channels 0 and 1 (:21), the spot
 * count measure.label(fish_probe).max() (:30-32) and the pixel loop np.linalg.norm(centromere_coords - fish_coord).min()
 * (:34-45).  labels: (H, W) int32 instance labels (what stat_fish saves as <name>__segmentation_min_cut.npy), values <= 0
 * are background, a label's pixels need not be connected; a label larger than H * W is refused with ECSEG_E_INVALID
 * (renumber by rank).  lsq: (H, W, C) uint8, C >= 2 (annotated/<name>/<name>_lsq*.tif: 0 red, 1 green, 2 boundaries).
 * *n_cells = the number of different labels > 0; records (capacity x 8 int64) receive, when n_cells <= capacity, per label
 * in ascending label order:
 *   [0] label  [1] area  [2] gate bits: 1 = channel 0 non-zero somewhere in the cell, 2 = channel 1 (the gate of :21 is [2] == 3)
 *   [3] FISH pixels (lsq[..., fish_channel] != 0 inside the cell)  [4] centromere pixels (centromere_channel)
 *   [5] 8-connected components of the FISH pixels, joined only through pixels of this cell (the spot limit of :31 is [5] > max)
 *   [6] min over FISH pixels f and centromere pixels c of the cell of |f - c|^2, exact; -1 when either set is empty
 *   [7] 0 (reserved).
 * The value of :39 is sqrt([6]) / sqrt([1]) in float64.  When n_cells > capacity nothing is written: call again with a buffer
 * of n_cells records.  One image per call, synchronous; the call keeps buffers of its own (a region map left on the handle by
 * ecseg_nuclei_regions stays valid); device time of the kernels in ECSEG_T_COUNT.  ECSEG_E_INVALID: C < 2, a channel outside
 * 0 .. C - 1, H * W >= 2^31, H * W * C >= 2^40.  The distance search is brute force (FISH x centromere pixels per cell). */
int ecseg_fish_distances(ecseg_ctx* h, const int32_t* labels, int H, int W, const uint8_t* lsq, int C, int fish_channel,
                         int centromere_channel, int capacity, int64_t* records, int32_t* n_cells);

/* The same for n_images images in ONE call (config key fish_distance_calculation.batch).  Image i has shapes[3 i ..] = H, W, C of its
 * own, labels[i] ((H, W) int32) and lsqs[i] ((H, W, C) uint8) as ecseg_fish_distances takes them; fish_channel and centromere_channel
 * apply to every image.  On the device the images' pixels lie back to back on one pixel axis (csrc/fishdist_batch.h): one scan numbers
 * the cells of the whole chunk, ascending by (image, label) - the same label value in two images is two cells - and no connected
 * component, list or distance reaches across the seam between two images.
 *   n_cells[i]: the different labels > 0 of image i.  records: 8 int64 per cell as ecseg_fish_distances writes them, the images back to
 * back in call order.  status[i]: ECSEG_OK, or ECSEG_E_INVALID for an image holding a label above its H * W: that image has n_cells[i]
 * = 0 and no record and disturbs no other image (the call itself returns ECSEG_OK).  record_capacity: room of `records` in cells, for
 * the whole chunk; when the chunk holds more, the call returns ECSEG_OK with every n_cells[i] and status[i] set and nothing else
 * written (ecseg_fish_distances' rule): come back with a larger buffer.  Every field is a sum, an OR, a minimum or a root count, so no
 * byte depends on the order of the atomics: the records equal those of n_images single calls, and two calls give identical bytes.
 *   ECSEG_E_INVALID, the message naming the image ("image i: ..."): what the single call refuses (no pointer, H or W below 1, C < 2, a
 * channel outside 0 .. C - 1, H * W >= 2^31, H * W * C >= 2^40); also more than ECSEG_FISH_DISTANCES_BATCH_MAX_IMAGES images, a chunk
 * of 2^31 pixels or more, or of 2^40 lsq bytes or more.  n_images == 0 is ECSEG_OK and does nothing.  One synchronous call; a chunk
 * whose scratch would pass 8 GiB runs its consecutive images in several groups.  The scratch is one grow-only buffer of the driver's
 * own on the handle (none of the arenas; a region map left by ecseg_nuclei_regions stays valid), freed with the handle; device time
 * of all kernels in ECSEG_T_COUNT. */
#define ECSEG_FISH_DISTANCES_BATCH_MAX_IMAGES 8192
int ecseg_fish_distances_batch(ecseg_ctx* h, int n_images, const int32_t* const* labels, const uint8_t* const* lsqs,
                               const int32_t* shapes /* [n][3] H, W, C */, int fish_channel, int centromere_channel, int record_capacity,
                               int64_t* records, int32_t* n_cells, int32_t* status);

/* ---- stat_fish behind nuclei_segment: per-nucleus FISH spot statistics (src/stat_fish.py:73-107,134-142,226-300) ----------- */
/* Replaces, for ONE image, get_thresholded (:73-88, the two TensorFlow convolutions included), the loop over
 * regionprops(labeled_segmented_cells) with count_blobs and intensity_metrics (:134-142,249-275; src/image_tools.py:121-124) and
 * get_boundaries (:91-107).  labels: (H, W) int32 instance labels as for ecseg_fish_distances (<= 0 background, <= H * W, need
 * not be connected; cells = the labels that occur, ascending).  img: (H, W, C) uint8.  probe_channels: n_probe (1..3) channel
 * indices into img, the reference's green then red (then aqua).  weights: K x K float64, K odd, 1 <= K <=
 * ECSEG_FISH_SPOT_MAX_KERNEL - the projected Gaussian kernel of :28-55, computed by the caller (its bits are the host's).
 *   Peak filter: per probe, coefficient = the zero-padded "SAME" correlation of the channel with weights, accumulated in float64
 *     in row-major tap order; centre = coefficient > normal_threshold, or pixel == the channel's maximum over the whole image
 *     when that maximum is non-zero; thresholded = centre && pixel > intensity_thresholds[probe] && label > 0.  NaN weights (K = 1
 *     gives 0 / 0) yield no normal centre.  An intensity threshold of +infinity switches a probe's mask off altogether (the
 *     reference's NaN-scale branch, :238-240).
 *   Spots: per cell and probe the 4-connected components (scipy.ndimage.label's default) of thresholded, joined only through
 *     pixels of the same cell; components of fewer than min_cc_size pixels are cleared from thresholded (:140 does so in place).
 *   Boundaries: with R = the dense rank of the labels (cell index + 1, 0 background) and t = line_thickness (1 ..
 *     ECSEG_FISH_SPOT_MAX_LINE), a pixel is 255 when sum R[y][x-t+1 .. x] != sum R[y][x+1 .. x+t] or the same along y, taps
 *     outside the image counting 0 (TensorFlow's "SAME" for the even kernel: t - 1 before, t after); the sums are 64-bit.
 * Outputs, written when n_cells <= capacity: thresholded (H, W, n_probe) uint8 0 / 255, cleaned; boundaries (H, W) uint8 0 / 255;
 * records (capacity x ECSEG_FISH_SPOT_INT64 int64), per cell in ascending label order:
 *   [0] label  [1] area  [2] sum of rows  [3] sum of columns   (nucleus centre = floor([2] / [1]), floor([3] / [1]))
 *   per probe j at 4 + 5 j: [+0] pixels of the kept spots  [+1] kept spots (foci)  [+2] sum and [+3] count of the non-zero raw
 *     pixels of the channel inside the cell (mean = sum / count, 0 without any)  [+4] their maximum      (0 for j >= n_probe)
 *   [19] pixels and [20] components of (cleaned mask 0 AND cleaned mask 1) that reach min_cc_size (0 when n_probe < 2)
 *   [21..23] 0 (reserved).
 * When n_cells > capacity nothing is written: call again with a buffer of n_cells records.  One image per call, synchronous,
 * buffers of its own; device time of the kernels in ECSEG_T_COUNT.  ECSEG_E_INVALID: n_probe outside 1..3, a channel outside
 * 0 .. C - 1, K even or outside 1 .. ECSEG_FISH_SPOT_MAX_KERNEL, line_thickness outside 1 .. ECSEG_FISH_SPOT_MAX_LINE, a label
 * above H * W, H * W >= 2^31, H * W * C >= 2^40. */
#define ECSEG_FISH_SPOT_INT64      24
#define ECSEG_FISH_SPOT_MAX_KERNEL 63
#define ECSEG_FISH_SPOT_MAX_LINE   16
int ecseg_fish_spots(ecseg_ctx* h, const int32_t* labels, int H, int W, const uint8_t* img, int C, const int32_t* probe_channels,
                     int n_probe, const double* weights, int K, double normal_threshold, const double* intensity_thresholds,
                     int min_cc_size, int line_thickness, int capacity, uint8_t* thresholded, uint8_t* boundaries,
                     int64_t* records, int32_t* n_cells);

/* Composes, for ONE image, the three colour files stat_fish writes beside the label map and the mask (:110-115,295-300,306-308):
 * merge_channels on the image, img_with_segmentation, and blob_labeled_img with its merge_channels.  img: (H, W, C) uint8, C = 3
 * or 4.  channels: C indices into img - its blue, green, red and (C = 4) aqua channel; the reference's arrays are BGR(A), a TIFF
 * read as RGB passes (2, 1, 0).  thresholded (H, W, n_probe) uint8 with n_probe = C - 1 and boundaries (H, W) uint8 as
 * ecseg_fish_spots returned them for the probes (green, red[, aqua]).  With k = (54, 137, 233) for (blue, green, red) - aqua_rgb
 * of :163 reversed - and q the aqua byte of a pixel, in integers:
 *   merged    c = min(255, img c + [((k_c * q) & 255) == 255]) for C = 4, img c for C = 3.  (:114 multiplies a Python int with a
 *             uint8 array: the product wraps modulo 256 BEFORE "/ 255", so the merge adds at most 1.  Reproduced, not corrected.)
 *   original  = merged                                                                        (:307 writes the merged image)
 *   with_segmentation = merged, and on boundaries != 0: blue = red = 255, green = (merged green + 1) & 255             (:296)
 *   lsq       blue = min(255, boundaries + k_b * m / 255), green = min(255, thresholded[0] + k_g * m / 255), red = min(255,
 *             thresholded[1] + k_r * m / 255), "/" flooring, m = thresholded[2] for C = 4 and 0 for C = 3 (:297-300, no wrap: that
 *             array is int).  An aqua spot lights all three channels, which fish_distance_calculation then reads as green and red
 *             FISH: the reference's behaviour, kept.
 * Outputs: three (H, W, 3) uint8 rasters in the order the TIFF writers store, RGB (cv2.imwrite stores its BGR arrays so).  One
 * elementwise kernel; one image per call, synchronous, buffers of its own; its device time in ECSEG_T_COUNT.  ECSEG_E_INVALID: C
 * outside 3..4, n_probe != C - 1, a channel index outside 0 .. C - 1, H * W >= 2^31. */
int ecseg_fish_render(ecseg_ctx* h, const uint8_t* img, int H, int W, int C, const int32_t* channels, const uint8_t* thresholded,
                      int n_probe, const uint8_t* boundaries, uint8_t* original, uint8_t* with_segmentation, uint8_t* lsq);

/* ---- TIFF files encoded on the device ---------------------------------------------------------------------------------------- */
/* The file ecseg_tiff_write_gray8 (spp = 1) / ecseg_tiff_write_rgb8 (spp = 3) would write for img, byte for byte, as a file image in
 * memory: the horizontal predictor, `invert` and the LZW coding of every strip run on the device, one wave per strip, the
 * strips are packed there, and only the packed bytes and the strip tables come back (csrc/tiff_kernels.hip).  img: (H, W, spp)
 * uint8 in host memory, uploaded by the call.  out receives *out_bytes bytes; a capacity of ecseg_tiff_encode_bound(H, W, spp)
 * (-1 for extents the writers refuse) always suffices, and a file that does not fit out_cap is ECSEG_E_INVALID with nothing
 * written, never a truncated file.  One synchronous call, scratch from the handle's call arena; device time of the kernels in
 * ECSEG_T_COUNT.  ECSEG_E_INVALID where the file writers return it - a null pointer, H or W < 1, W * spp >= 2^30, a file that would
 * pass 4 GiB - and for spp outside {1, 3}. */
long long ecseg_tiff_encode_bound(int H, int W, int spp);
int ecseg_tiff_encode(ecseg_ctx* h, const uint8_t* img, int H, int W, int spp, int invert, uint8_t* out, long long out_cap,
                      long long* out_bytes);
/* ecseg_fish_render followed by ecseg_tiff_encode of its three rasters, without their leaving the device: files[0..2] receive
 * the file images of _original, _original_with_segmentation and _lsq_ (file_bytes[0..2] their lengths), each with room for
 * file_cap bytes (ecseg_tiff_encode_bound(H, W, 3) always suffices; too little is ECSEG_E_INVALID with no file written).
 * original, with_segmentation and lsq: each null, or room for the (H, W, 3) raster as ecseg_fish_render returns it.  Inputs and
 * their rules are ecseg_fish_render's.  Device time of all kernels, render and encode, in ECSEG_T_COUNT. */
int ecseg_fish_render_tiff(ecseg_ctx* h, const uint8_t* img, int H, int W, int C, const int32_t* channels, const uint8_t* thresholded,
                           int n_probe, const uint8_t* boundaries, uint8_t* const* files, long long file_cap, long long* file_bytes,
                           uint8_t* original, uint8_t* with_segmentation, uint8_t* lsq);
/* ecseg_tiff_encode over n_files rasters in one call (csrc/tiff_kernels.hip, the tiffb_* kernels; csrc/tiff_encode_batch.h): the
 * strips of all files are one grid, a wave per strip, so a file of few strips runs beside the others instead of leaving the device
 * idle.  rasters: raster_bytes of host memory; files[5 i ..] = byte offset, H, W, spp, invert of raster i, the rasters in ascending
 * order and clear of each other (gaps are allowed).  The files may differ in extent, spp (1 or 3) and invert.  out receives the file
 * images back to back, file i at out + out_ranges[2 i] with out_ranges[2 i + 1] bytes, each byte for byte what ecseg_tiff_encode
 * returns for that raster alone.  The sum of ecseg_tiff_encode_bound over the files always suffices as out_cap.  ECSEG_E_INVALID,
 * with no byte of out or out_ranges written: a null pointer, n_files < 0 or >= 65536, a row ecseg_tiff_encode refuses, a raster that
 * overlaps the one in front or leaves raster_bytes, 2^31 strips or more in all, files that do not fit out_cap.  n_files == 0 is
 * ECSEG_OK and does nothing.  One synchronous call: one upload of the span of the rasters, the table beside it, one copy back of all
 * file images; scratch from the handle's call arena (ecseg_tiff_encode_batch_bytes: its size for such a table, negative for a table
 * the call refuses; no device work); device time of the kernels in ECSEG_T_COUNT. */
int ecseg_tiff_encode_batch(ecseg_ctx* h, const uint8_t* rasters, long long raster_bytes, const int64_t* files /* [n][5] offset, H, W, spp, invert */,
                            int n_files, uint8_t* out, long long out_cap, int64_t* out_ranges /* [n][2] offset, n_bytes */);
long long ecseg_tiff_encode_batch_bytes(const int64_t* files, int n_files);
/* ecseg_fish_render_tiff over n_images images in one call, with up to two further rasters per image encoded beside the three rendered
 * ones: image i has shapes[3 i ..] = H, W, C, channels[4 i ..] (C of them read), imgs[i], thresholded[i] ((H, W, C - 1)) and
 * boundaries[i] as ecseg_fish_render takes them, masks[i] ((H, W), one sample) and pictures[i] ((H, W, 3)), each null for "none"
 * (masks or pictures itself null: none for any image).  The rendered rasters never leave the device and ALL files of all images go
 * through one batched encode.  out receives the file images back to back; out_ranges[10 i + 2 k ..] = offset, bytes of file k of
 * image i, k = 0 .. 4: _original, _original_with_segmentation, _lsq_, the mask, the picture ((0, 0) for a raster that was not given),
 * each what ecseg_fish_render_tiff and ecseg_tiff_encode return for it alone.  Argument rules are those calls'; ECSEG_E_INVALID leaves
 * out and out_ranges unwritten, n_images == 0 is ECSEG_OK and does nothing.  Device time of all kernels in ECSEG_T_COUNT. */
int ecseg_fish_render_tiff_batch(ecseg_ctx* h, int n_images, const uint8_t* const* imgs, const int32_t* shapes /* [n][3] H, W, C */,
                                 const int32_t* channels /* [n][4] */, const uint8_t* const* thresholded, const uint8_t* const* boundaries,
                                 const uint8_t* const* masks, const uint8_t* const* pictures, uint8_t* out, long long out_cap,
                                 int64_t* out_ranges /* [n][5][2] offset, n_bytes */);

/* stat_fish from the nucleus mask to the file images for n_images images in ONE call (config key stat_fish.batch): per image what
 * ecseg_ccl_labels(mask, 8) -> ecseg_fish_spots -> ecseg_fish_render_tiff_batch give, with every raster uploaded once and nothing
 * brought back that the caller does not write to disk.  imgs[i] (H, W, C) uint8, C = 3 or 4, shapes and channels as
 * ecseg_fish_render_tiff_batch takes them; the probes of image i are channels[i][1 .. C - 1] (green, red[, aqua]).  Exactly one of
 * masks[i] ((H, W) uint8, non-zero = nucleus, labelled 8-connected on the device) and labels[i] ((H, W) int32, used as given: <= 0
 * background, cells need not be connected, no label above H * W) is non-null.  Per image its own ecseg_fish_spots parameters:
 * kernel_sizes[i] = K, weights[i] (K x K float64), normal_thresholds[i], intensity_thresholds[3 i .. 3 i + 2] (the first C - 1 are
 * read), min_cc_sizes[i]; line_thickness is one for the call.  mask_files / pictures (either may be NULL, and so may any entry): the
 * (H, W) raster of _segmentation.tif and the (H, W, 3) min-cut picture, encoded beside the three rendered files; where mask_files[i]
 * is the pointer masks[i] the mask is uploaded once.
 *   ranks: int32, the images' (H, W) maps back to back: 0 background, else 1 + the cell's index in ascending label order (what
 * ecseg_fish_spots' records[.][0] numbers).  records: ECSEG_FISH_SPOT_INT64 int64 per cell as ecseg_fish_spots writes them, the images
 * back to back; n_cells[i]: the cells of image i.  out, out_cap, out_ranges: as ecseg_fish_render_tiff_batch returns them.
 * thresholded_debug / boundaries_debug (tests; may be NULL): ecseg_fish_spots' thresholded ((H, W, C - 1)) and boundaries ((H, W)) of
 * the images back to back - otherwise they never leave the device.
 *   record_capacity: room of `records` in cells, for the whole chunk.  When the chunk holds more, the call returns ECSEG_OK with every
 * n_cells[i] set and nothing else written (ecseg_fish_spots' rule): come back with a larger buffer.  out_cap too small is
 * ECSEG_E_INVALID with no output but n_cells written.  An image without a nucleus has zero ranks, no record and files rendered from
 * all-zero masks.  ECSEG_E_INVALID: what the single calls refuse, the message naming the image ("image i: ..."); more than
 * ECSEG_STAT_FISH_BATCH_MAX_IMAGES images; a chunk of 2^31 pixels or more (also counted with every mask padded to the largest one).
 * n_images == 0 is ECSEG_OK and does nothing.  No result depends on the order of the atomics: two calls give identical bytes.  One
 * synchronous call; scratch from the handle's call arena and, for what the cell count sizes, its count arena
 * (ecseg_stat_fish_batch_bytes says how much); device time of all kernels in ECSEG_T_COUNT. */
#define ECSEG_STAT_FISH_BATCH_MAX_IMAGES 8192
int ecseg_stat_fish_batch(ecseg_ctx* h, int n_images, const uint8_t* const* imgs, const int32_t* shapes /* [n][3] H, W, C */,
                          const int32_t* channels /* [n][4] */, const uint8_t* const* masks, const int32_t* const* labels,
                          const int32_t* kernel_sizes, const double* const* weights, const double* normal_thresholds,
                          const double* intensity_thresholds /* [n][3] */, const int32_t* min_cc_sizes, int line_thickness,
                          const uint8_t* const* mask_files, const uint8_t* const* pictures, int record_capacity, int32_t* ranks,
                          int64_t* records, int32_t* n_cells, uint8_t* out, long long out_cap, int64_t* out_ranges /* [n][5][2] */,
                          uint8_t* thresholded_debug, uint8_t* boundaries_debug);
/* Bytes of device scratch such a call needs (both arenas), or -1 for a chunk it refuses.  flags[i]: bit 0 the image comes with given
 * labels (else a mask), bit 1 it has a mask file, bit 2 that file is the mask itself, bit 3 it has a picture.  No device work. */
long long ecseg_stat_fish_batch_bytes(int n_images, const int32_t* shapes, const int32_t* kernel_sizes, const int32_t* flags,
                                      int record_capacity);

/* ---- TIFF files decoded on the device ---------------------------------------------------------------------------------------- */
/* skimage.io.imread of a baseline TIFF (src/utils.py:110) from a file image in memory, with every strip decoded on the device
 * (csrc/tiff_decode_kernels.hip: one wave per LZW strip, then byte order and the horizontal predictor row by row): what
 * ecseg_tiff_info plus ecseg_tiff_read return for the same bytes - ECSEG_OK, the shape in *H, *W, *samples_per_pixel,
 * *bits_per_sample and the samples in dst as native-endian (H, W, spp), strips that end early or are missing zero-filled - or
 * ECSEG_E_INVALID (not a TIFF, a corrupt IFD, a strip offset behind the file, a corrupt LZW stream in any strip: dst is not
 * written).  ECSEG_E_UNSUPPORTED: everything ecseg_tiff_info leaves to the Python reader, and Deflate strips, tiles and PackBits files unless the
 * handle option of their kind is on (the section below; also strips of 2 GiB or more); the shape is reported then too
 * when the file has one.  dst == NULL: only the shape (and the ECSEG_E_UNSUPPORTED verdict).  dst_bytes below H * W * spp *
 * bits / 8: ECSEG_E_INVALID with nothing written.  file: n_bytes of host memory, uploaded by the call; one synchronous call,
 * scratch (file image, strip tables, raster, status words) from the handle's call arena; device time of the kernels in
 * ECSEG_T_COUNT. */
int ecseg_tiff_decode(ecseg_ctx* h, const uint8_t* file, long long n_bytes, void* dst, long long dst_bytes,
                      int* H, int* W, int* samples_per_pixel, int* bits_per_sample);
/* ecseg_tiff_decode over n_files files in one call (csrc/tiff_decode_kernels.hip, the tiffb_* kernels): the strips of all files are
 * one grid, a wave per strip, so files of few strips find in each other the parallelism one of them lacks.  files: files_bytes of
 * host memory; file i is bytes [file_ranges[2 i], file_ranges[2 i] + file_ranges[2 i + 1]) of it, the ranges in ascending order
 * and clear of each other.  status[i] is what ecseg_tiff_decode returns for file i alone (ECSEG_OK, ECSEG_E_INVALID,
 * ECSEG_E_UNSUPPORTED), shapes[4 i ..] its H, W, samples per pixel and bits per sample (zeros where the file has no shape).  A file
 * that is not ECSEG_OK is left out of the launch: its raster is not written - a corrupt LZW stream is found on the device, and that
 * file's raster is not copied back - and it disturbs no other file.  The raster of file i goes to dst + dst_offsets[i], native-endian
 * (H, W, spp) as there; dst_offsets of files that are not decoded are not read.  dst == NULL: only shapes and status, without the
 * verdicts that need the strips (an offset behind the file, a corrupt stream), as ecseg_tiff_decode's own first pass.
 * Returns ECSEG_OK when it ran, whatever the status words say; ECSEG_E_INVALID only for bad arguments: n_files < 0, a null pointer,
 * a range that starts before the end of the one in front or leaves files_bytes, a raster that leaves dst_bytes or overlaps another
 * file's, a 16-bit raster at an odd offset, 2^31 strips or rows or more in all.  n_files == 0 is ECSEG_OK and does nothing.
 * One synchronous call: the files are uploaded as one span (first decoded file's first byte to the last one's last), the table and
 * the strip tables beside it; the rasters lie on the device as in dst and come back in one copy per run of rasters without a gap - one
 * copy where the caller packed them.  Scratch from the handle's call arena; device time of the kernels in ECSEG_T_COUNT. */
int ecseg_tiff_decode_batch(ecseg_ctx* h, const uint8_t* files, long long files_bytes, const int64_t* file_ranges /* [n][2] offset, n_bytes */,
                            int n_files, void* dst, long long dst_bytes, const int64_t* dst_offsets /* [n] */,
                            int32_t* shapes /* [n][4] H, W, spp, bits */, int32_t* status /* [n] */);

/* ---- which files are worth sending: four questions without a handle, and the kinds of file a decoder takes -------------------------- */
/* A word of these bits says which kinds of file are taken beside LZW and uncompressed strips.  A handle keeps one, all bits clear by
 * default, set and cleared by ecseg_set_option(h, "tiff_deflate_on_device" / "tiff_tiled_on_device" / "tiff_packbits_on_device", 0 or 1):
 * ecseg_tiff_decode and ecseg_tiff_decode_batch on that handle take the kinds whose bit is set and answer ECSEG_E_UNSUPPORTED for the
 * others, and ecseg_meta_segment_tiffs reads the word off its handle as the two do.  The four functions at the end of this section take
 * no handle and get the word as their last argument, `kinds`; 0 gives the answers for LZW and uncompressed strips alone, and a bit
 * outside the three is a bad argument.  BigTIFF files stay ECSEG_E_UNSUPPORTED under every word. */
#define ECSEG_TIFF_DEFLATE  1u
#define ECSEG_TIFF_TILED    2u
#define ECSEG_TIFF_PACKBITS 4u
/* The rule for one file, ecseg_tiff_decode_routes (image_io.imread(path, handle) asks it): 1 for an LZW file of at least 1040 strips,
 * 0 for everything else, unreadable files and bad arguments included.  A strip is one serial stream on one wave, so the device is
 * faster than a host core only where many strips decode at once; the measurement behind the threshold is in DESIGN.md 5.9.
 *   The rule for a set of files that would go in one ecseg_tiff_decode_batch call, ecseg_tiff_decode_batch_routes
 * (image_io.imread_many asks it): 1 when the LZW strips of the files ecseg_tiff_decode accepts, whatever their own strip count, are at
 * least 1040 together; uncompressed files are never counted, nor - under any word - files whose strips decode to more than 62640
 * bytes (nothing was measured there) or whose strip table is shorter than the image (as in the single-file rule).  0 for everything
 * else, bad arguments included.  ecseg_tiff_decode_batch_counts: 1 for a file that the rule counts - the files of a set that goes
 * which are sent -, 0 for any other.  The measurement behind the threshold is the batch table of DESIGN.md 5.9.
 *   ecseg_tiff_decode_batch_bytes: the bytes of the call arena ecseg_tiff_decode_batch needs for these files, as a handle with this
 * word takes them, with their rasters back to back (16-bit ones on even offsets), for a caller that splits a large set into several
 * calls; -1 for bad arguments, 0 for no files.  A file the word does not take is left out and needs nothing.
 *   None of the four does device work.  What each kind adds:
 *
 * ECSEG_TIFF_DEFLATE - Deflate strips (compression 8, and 32946 of older writers), option "tiff_deflate_on_device".  Accepted: such
 * files, one wave per strip in a kernel of its own beside the LZW one (csrc/tiff_inflate_strip.h: each strip a zlib stream of its own,
 * matches copied in the raster, Adler-32 checked), mixed freely with LZW and uncompressed files in a batch; they return ECSEG_OK or
 * ECSEG_E_INVALID where they returned ECSEG_E_UNSUPPORTED.  The oracle is the host reader (ecseg_tiff_read): a short stream
 * zero-filled, a long one cut, every zlib data error corrupt; a stream that ends before the strip is full and before its own end is
 * corrupt, as uncompress of zlib 1.2.9 and later has it.  Routing: with the bit a Deflate file counts from its own thresholds on
 * (csrc/tiff_parse.h, the Deflate tables of DESIGN.md 5.9: a single file from 1040 strips, a set from 280 Deflate strips together,
 * summed apart from the LZW strips - the smallest measured counts at which the device call's maximum is below ecseg_tiff_read's
 * minimum); without it a Deflate file is never counted.  Arena: the Deflate kernel keeps its tables in LDS and needs nothing more
 * than an LZW file of the same tags.
 *
 * ECSEG_TIFF_TILED - tiled files (TileWidth, TileLength, TileOffsets, TileByteCounts: tags 322 to 325; what Bio-Formats / OME-TIFF,
 * QuPath, libvips and tifffile with tile= write), option "tiff_tiled_on_device".  Accepted: a tiled file whose tile extents are
 * positive multiples of 16 (of at most 2^20), chunky (or one sample per pixel), 8 or 16 unsigned bits, uncompressed or LZW - Deflate
 * with ECSEG_TIFF_DEFLATE as well, PackBits with ECSEG_TIFF_PACKBITS as well -, predictor 1 or 2, without strip tags, with a tile table
 * entry for each of its ceil(H / TileLength) * ceil(W / TileWidth) tiles and tiles below 2 GiB.  Every other tiled file stays
 * ECSEG_E_UNSUPPORTED (BigTIFF, PackBits tiles without ECSEG_TIFF_PACKBITS, planar RGB, float samples, a short tile table, strip and
 * tile tags together), as does every tiled file without the bit - without a shape.  A tile is a strip of the batch grid - a wave per
 * tile, beside the strips of other files in the same launch - whose stream decodes into a staging slot of one tile in the call arena;
 * tiffb_untile_kernel (csrc/tiff_untile.h) then puts every tile row in its place in the raster: byte order, the horizontal predictor
 * restarting at each tile's first column, the padding of right and bottom edge tiles dropped.  Uncompressed tiles have no slot and
 * are placed from the file image.  The oracle is the Python reader (image_io.read_tiff), the one reader of tiled files so far:
 * ECSEG_OK with its samples, or ECSEG_E_INVALID where it raises on a tile's stream (a corrupt LZW stream; a Deflate stream that is
 * corrupt, cut short or empty).  Like that reader's slice, a tile's bytes are clamped to the file: an offset behind the file or a
 * count that leaves it is a shorter or empty stream - zeros for an LZW or uncompressed tile, ECSEG_E_INVALID for a Deflate one - not
 * an error of its own.  (One difference remains, in the inflate routine shared with strips: a Deflate stream that gave the whole tile
 * and ends inside its trailer is taken, where zlib.decompress refuses it.)  Routing: a tiled file counts in the two rules only from a
 * measured tile count on (csrc/tiff_parse.h; tools/time_tiff_decode.py --tiled).  That table is NOT MEASURED yet: the
 * rules answer 0 for every tiled file and every set of them, and only an explicit ecseg_tiff_decode / ecseg_tiff_decode_batch call
 * decodes one on the device.  Arena: the staging slots of a file's compressed tiles and a 32-byte table row per tiled file on top.
 *
 * ECSEG_TIFF_PACKBITS - PackBits files (compression 32773: older ImageJ and Photoshop exports), option "tiff_packbits_on_device".
 * Accepted: such a file, strips or - with ECSEG_TIFF_TILED as well - tiles, held to every other rule of the readers above: a wave per
 * strip or tile in a kernel of its own beside the LZW and Deflate ones (tiffb_packbits_kernel; csrc/tiff_packbits_strip.h: the header
 * walk in every lane, the up to 128 bytes of a run written by the lanes), byte order and predictor by the code that serves the other
 * codecs, a tile through its staging slot and tiffb_untile_kernel.  Without the bit every PackBits file is ECSEG_E_UNSUPPORTED
 * without a shape.  The oracle is the Python reader (image_io.read_tiff with _packbits_decode), the one reader of PackBits files:
 * header h < 128: h + 1 literal bytes; h > 128: the next byte 257 - h times; 128: nothing.  That decoder raises for no stream - one
 * that ends early gives what it has and zeros behind, a run that would pass the strip's end is cut there, bytes left over are not
 * looked at - so no PackBits stream is ECSEG_E_INVALID; a strip that starts behind the end of the file is, as for every codec.
 * Routing: no table of tools/time_tiff_decode.py --packbits is measured (NOT MEASURED): with the bit a PackBits file
 * parses, and it counts in no routing rule, strips or tiles; only an explicit call decodes one on the device.  Arena: what an LZW
 * file of the same tags needs. */
int ecseg_tiff_decode_routes(const uint8_t* file, long long n_bytes, unsigned kinds);
int ecseg_tiff_decode_batch_counts(const uint8_t* file, long long n_bytes, unsigned kinds);
int ecseg_tiff_decode_batch_routes(const uint8_t* files, long long files_bytes, const int64_t* file_ranges, int n_files, unsigned kinds);
long long ecseg_tiff_decode_batch_bytes(const uint8_t* files, long long files_bytes, const int64_t* file_ranges, int n_files, unsigned kinds);

/* ---- label PNG files encoded on the device ----------------------------------------------------------------------------------- */
/* The file ecseg_png_write_labels would write for each of n_img label images, byte for byte (signature, IHDR, one IDAT, IEND), as
 * file images in memory (csrc/png_kernels.hip: the runs of every scan line are counted on the device, the Huffman code is built
 * on the host from the 68 counts by the host writer's own functions, the device writes the bits and the Adler-32; the chunk
 * CRCs are the host's).  labels: (n_img, H, W) uint8 in host memory, uploaded by the call; values above 3 count as 3.  files[i]:
 * room for file_cap bytes.  A file that fits receives its bytes and file_bytes[i] = its length; one that does not is not
 * produced - file_bytes[i] = -(the bytes it needs), nothing of it is written, the call still returns ECSEG_OK and the other
 * files are whole.  One synchronous call, scratch from the handle's arenas; device time of the kernels in ECSEG_T_COUNT.
 * ECSEG_E_INVALID: a null pointer (n_img > 0), H or W < 1, W >= 2^30, n_img < 0 or >= 65536, file_cap < 1. */
int ecseg_png_labels_encode(ecseg_ctx* h, const uint8_t* labels, int n_img, int H, int W, uint8_t* const* files, long long file_cap,
                            long long* file_bytes);
/* ---- gray PNG files (one channel of an interleaved image) encoded on the device ------------------------------------------------ */
/* A size no file of ecseg_png_write_channel for an H x W image can exceed: signature, IHDR, IDAT framing, the worst stream (15 bits
 * per filtered byte, header, end of block, Adler-32), IEND.  No device work.  -1 for H or W < 1. */
long long ecseg_png_channel_bound(int H, int W);
/* The file ecseg_png_write_channel would write for channel `channel` of each of n_img interleaved 8-bit images, inverted when
 * invert != 0, byte for byte, as file images in memory (csrc/png_gray_kernels.hip: the maximal runs of the SUB-filtered stream are
 * counted on the device, a wave per span of the flat stream; the Huffman code is built on the host from the 286 counts by the
 * host writer's own functions, which also give every stream's exact size; the device writes the bits and the Adler-32; the chunk
 * CRCs are the host's).  pixels: (n_img, H, W, C) uint8 in host memory, uploaded by the call.  files[i]: room for file_cap bytes;
 * capacities and lengths follow ecseg_png_labels_encode's protocol, and the verdict falls before a bit is written.  One synchronous
 * call, scratch from the handle's call arena; device time of the kernels in ECSEG_T_COUNT.
 * ECSEG_E_INVALID: a null pointer (n_img > 0), H or W < 1, H (W + 1) >= 2^31 - 1, C < 1 or > 256, channel outside [0, C), n_img < 0
 * or >= 65536, file_cap < 1. */
int ecseg_png_channel_encode(ecseg_ctx* h, const uint8_t* pixels /* (n_img,H,W,C) host */, int n_img, int H, int W, int C, int channel, int invert,
                             uint8_t* const* files, long long file_cap, long long* file_bytes);
/* `make meta_overlay`'s device work in one call: one upload of the labels (n_img, H, W) and of the image (n_img, H, W, C) of 8- or
 * 16-bit samples; 16-bit samples become 8-bit on the device as ecseg_u16_to_u8 makes them; `out` receives exactly ecseg_overlay's
 * rows on that 8-bit image; red_files[i] and green_files[i] receive what ecseg_png_write_channel writes for its channels 0 and 1 with
 * invert = 1, byte for byte, under ecseg_png_channel_encode's capacity protocol (one file_cap for both).  The 8-bit image never
 * returns to the host.  ecseg_get_file_timings then gives ms_out[0] = 0 and in ms_out[1] the device time of the PNG kernels;
 * ECSEG_T_COUNT holds that plus the counting kernels'.  Argument errors are ecseg_overlay's and ecseg_png_channel_encode's, and
 * bytes_per_sample other than 1 or 2. */
int ecseg_overlay_files(ecseg_ctx* h, const uint8_t* labels, const void* img, int n_img, int H, int W, int C, int bytes_per_sample /* 1 | 2 */,
                        int sensitivity, int hsr_size_threshold, int64_t* out /* [n][12] */, uint8_t* const* red_files,
                        uint8_t* const* green_files, long long file_cap, long long* red_bytes, long long* green_bytes);
/* ecseg_meta_segment plus the two files `make metaseg` writes per image, as file images: dapi_files[i] receives what
 * ecseg_tiff_write_gray8(gray_i, invert = 1) writes, png_files[i] what ecseg_png_write_labels(labels_post_i) writes, byte for
 * byte.  The dapi strips of the whole batch are encoded on the second stream as soon as the pre-processing is done, under the
 * U-Net; the PNGs behind the clean-up.  Capacities and lengths follow ecseg_png_labels_encode's protocol for both kinds of file
 * (a file that does not fit: its *_bytes[i] = -(the bytes it needs), the caller writes it from gray_out / labels_post).
 * labels_post, n_ec and tie_risk are ecseg_meta_segment's; gray_out may be null.  Argument errors are ecseg_meta_segment's, and a
 * null file table or buffer, a capacity below 1, 65536 images or more.  ecseg_get_file_timings: ms_out[0] the device time of the
 * last call's dapi encode (as it ran beside the U-Net), ms_out[1] that of its PNG kernels. */
int ecseg_meta_segment_files(ecseg_ctx* h, const void* img, int n_img, int H, int W, int C, int bytes_per_sample, uint8_t* const* dapi_files,
                             long long dapi_cap, long long* dapi_bytes, uint8_t* const* png_files, long long png_cap, long long* png_bytes,
                             uint8_t* gray_out, uint8_t* labels_post, int32_t* n_ec, int32_t* tie_risk);
int ecseg_get_file_timings(ecseg_ctx* h, float* ms_out /* [2] */);
/* ecseg_meta_segment with the input files themselves as its input: the packed file table of ecseg_tiff_decode_batch (files, files_bytes,
 * file_ranges, n_files) and the batch's common shape.  The strips of every file decode on the device, a wave per strip, straight into
 * the call's input buffer (raster i at i * H * W * C * bytes_per_sample); pre-processing, U-Net, clean-up and count run behind them as
 * in ecseg_meta_segment, and the host decodes nothing.  status[i] is what ecseg_tiff_decode returns for file i alone ON THIS HANDLE
 * (ECSEG_OK, ECSEG_E_INVALID, ECSEG_E_UNSUPPORTED): the options "tiff_deflate_on_device", "tiff_tiled_on_device" and
 * "tiff_packbits_on_device" are read as ecseg_tiff_decode reads them - all 0 (the default): LZW and uncompressed strips alone, every
 * other file ECSEG_E_UNSUPPORTED; on: Deflate strips, tiles and PackBits files decode into the same slots, by the same kernels.  A file that decodes but whose H, W, samples per pixel or bits are not the call's has
 * ECSEG_E_INVALID.  An image whose status is not ECSEG_OK is the all-zero image - its input slot is cleared on the device before the
 * pre-processing, so that nothing of an earlier call reaches an output -, its n_ec is -1 and (_files) its two file lengths are 0;
 * every other image has exactly what ecseg_meta_segment gives for the samples image_io.read_tiff returns (ecseg_tiff_read's, where
 * that reader takes the file), byte for byte.  The call
 * returns ECSEG_OK when it ran, whatever the status words say.  ECSEG_E_INVALID: the argument errors of ecseg_meta_segment and of
 * ecseg_tiff_decode_batch (a null table, a range that overlaps the one in front or leaves the files), 65536 images or more, 2^31
 * strips or rows or more.  ecseg_meta_segment_tiffs_files: the same with the two file tables, the capacity protocol and the timings
 * of ecseg_meta_segment_files.  ecseg_get_read_timings: ms_out[0] the device time of the decode kernels that served the last such
 * call (those of the decode-ahead, where it took its rasters from one). */
int ecseg_meta_segment_tiffs(ecseg_ctx* h, const uint8_t* files, long long files_bytes, const int64_t* file_ranges /* [n][2] offset, n_bytes */,
                             int n_files, int H, int W, int C, int bytes_per_sample, int32_t* status /* [n] */, uint8_t* gray_out,
                             uint8_t* labels_post, int32_t* n_ec, int32_t* tie_risk);
int ecseg_meta_segment_tiffs_files(ecseg_ctx* h, const uint8_t* files, long long files_bytes, const int64_t* file_ranges, int n_files, int H, int W,
                                   int C, int bytes_per_sample, int32_t* status /* [n] */, uint8_t* const* dapi_files, long long dapi_cap,
                                   long long* dapi_bytes, uint8_t* const* png_files, long long png_cap, long long* png_bytes, uint8_t* gray_out,
                                   uint8_t* labels_post, int32_t* n_ec, int32_t* tie_risk);
int ecseg_get_read_timings(ecseg_ctx* h, float* ms_out /* [1] */);
/* The analogue of ecseg_prefetch_input: names the files of the ecseg_meta_segment_tiffs[_files] call AFTER the coming one, as that call
 * will pass them (page-locked memory, unchanged until then).  The coming ecseg_meta_segment_tiffs[_files] call uploads them on the
 * input stream and decodes them there into the spare input buffer, under its own kernels; the call after it recognises them by
 * (pointer, bytes, ranges, n, shape) and the state of the three tiff_*_on_device options under which they were decoded, and skips
 * upload and decode.  Any other call on the handle withdraws them, as does files == null or n_files == 0, and so does a change of one
 * of those options in between: the call then decodes its files itself, under the options as they stand.  Results are those of calls
 * without it. */
int ecseg_prefetch_tiffs(ecseg_ctx* h, const uint8_t* files, long long files_bytes, const int64_t* file_ranges, int n_files, int H, int W, int C,
                         int bytes_per_sample);

/* ---- the min-cut nucleus splitter: a batch of grid max-flows (src/max_flow_binary_mask.py:59-116) ------------------------- */
/* Replaces get_graph + max_flow + partition_min_cut (:59-116) for a BATCH of independent tasks; segment_min_cut's recursion
 * (:119-140) stays with the caller, who sends all tasks of one recursion depth over all nuclei of an image in one call.
 * masks: mask_bytes bytes holding the windows back to back; tasks: (n_tasks, 8) int32 per task
 *   [0] offset of the window in masks  [1] h  [2] w  [3] source row  [4] source column  [5] sink row  [6] sink column  [7] 0,
 * the window M being h x w uint8 in row-major order, non-zero = pixel; windows lie in ascending order and do not overlap.
 * dist (d) is shared by all tasks.  The network of one task, with s the source and t the sink pixel:
 *   Body pixels: the pixels with M != 0 other than s and t.
 *   Unit-capacity arcs:
 *     s -> p for body pixels with |p - s|_1 <= d;
 *     p -> t for body pixels with |p - t|_1 <= d that are NOT within d of s (the source ball wins: the reference uses `elif`);
 *     p -> q for every body pixel p and each 4-neighbour q inside the window with M[q] != 0; q may be s or t.
 *   A body pixel next to t and inside its ball therefore has capacity 2 into t: two parallel arcs, both kept.
 *   s has no arcs except to its ball.  Nothing leaves t.
 * Outputs: side (mask_bytes bytes, laid out as masks; bytes outside every window are 0): per window pixel 1 = reachable from s
 * in the residual network of a maximum flow, s included, else 0 - the source side of the minimal minimum cut, which is the
 * same set for every maximum flow, so no augmentation order can change it; flow (n_tasks int32): the max-flow value.
 * One synchronous call, buffers of its own, device time of the kernel in ECSEG_T_COUNT; n_tasks = 0 is allowed and does
 * nothing.  ECSEG_E_INVALID: s == t; s or t outside the window or on a zero pixel; d < 1 or d > ECSEG_MIN_CUT_MAX_DIST; h or
 * w < 1 or h * w > ECSEG_MIN_CUT_MAX_PIXELS (2048 x 2048); mask_bytes > ECSEG_MIN_CUT_MAX_BYTES; a window that leaves masks or
 * starts before the end of the one in front.  Windows of up to ECSEG_MIN_CUT_LDS_PIXELS pixels are solved in LDS, larger ones in a
 * scratch region of 6 bytes per pixel (ECSEG_E_NOMEM when the device cannot hold it). */
#define ECSEG_MIN_CUT_MAX_DIST   32
#define ECSEG_MIN_CUT_MAX_PIXELS (1 << 22)
#define ECSEG_MIN_CUT_MAX_BYTES  (1 << 28)
#define ECSEG_MIN_CUT_LDS_PIXELS 10240
int ecseg_min_cut(ecseg_ctx* h, const uint8_t* masks, long long mask_bytes, const int32_t* tasks, int n_tasks, int dist, uint8_t* side,
                  int32_t* flow);

/* ---- the min-cut nucleus splitter before its first max-flow (src/max_flow_binary_mask.py:143-216) ---------------------------- */
/* Replaces, for ONE image, label(mask, connectivity=1) (:204), the areas, their median and the selection (:205-206,214), the
 * bounding-box crops (:212,215) and get_centers + binary_img_to_centers on every selected crop (:143-199, percentile 0).
 * mask: (H, W) uint8, != 0 is foreground.  labels (H, W) int32: the 4-connected components numbered 1..n in raster order of each
 * component's first pixel, 0 background; *n_cells = n.  Selected: the labels with (double)area > coeff * np.median(areas), strictly,
 * in ascending label order; *n_regions their count.  Per selected region i:
 *   regions (region_capacity x 8 int32): [0] label  [1] r0  [2] c0  [3] h  [4] w (its bounding box)  [5] offset of its window
 *     [6] index of its first centre record  [7] number of centre components;
 *   windows: the crop labels[box] == label as uint8 0 / 1, row-major, the crops back to back - the layout ecseg_min_cut takes for
 *     `masks`; *window_pixels their total size; comp (int32, laid out as windows): the 8-connected components of the centre pixels,
 *     numbered 1.. in raster order of first pixels, 0 elsewhere;
 *   centers (center_capacity x 8 int32), by region, then component: [0] region index  [1] row  [2] column (the component's centroid
 *     rounded half to even, crop coordinates)  [3] 1 if the window is non-zero there, else 0 (the caller then draws a pixel of the
 *     component, :148-150)  [4] area  [5] raster index of the component's first pixel in the crop  [6] 0  [7] 0.
 * Centre pixels of an h x w crop: with d the exact city-block distance to the nearest zero pixel of the crop itself (2^30 everywhere
 * when it has none) and the candidates the interior pixels with d > min_rad that are not below any of their eight neighbours, the
 * interior pixels with d >= max(min over the candidates of d, min_rad); none without a candidate or when h < 3 or w < 3.
 * When region_capacity < *n_regions, center_capacity < *n_centers or window_capacity < *window_pixels, labels and the three counts
 * are still written and regions, centers, windows and comp are not touched: call again with larger buffers (as ecseg_fish_spots).
 * One synchronous call, scratch from the handle's arenas, device time of the kernels in ECSEG_T_COUNT; integer work throughout: two
 * calls give identical bytes.  ECSEG_E_INVALID: a null pointer, a negative capacity, H or W < 1, H * W >= 2^31, min_rad < 0, coeff
 * not finite, a selected region whose crop exceeds ECSEG_MIN_CUT_MAX_PIXELS (the message names the label) or windows of more than
 * ECSEG_MIN_CUT_MAX_BYTES in all - ecseg_min_cut would refuse those anyway.  Crops of up to ECSEG_MIN_CUT_CENTERS_LDS_PIXELS pixels
 * (whose rows, padded to an odd stride, fit 10240 cells) keep their state in LDS, larger ones in their own part of comp. */
#define ECSEG_MIN_CUT_CENTERS_LDS_PIXELS 8192
int ecseg_min_cut_regions(ecseg_ctx* h, const uint8_t* mask, int H, int W, double coeff, int min_rad, int region_capacity,
                          int center_capacity, long long window_capacity, int32_t* labels, int32_t* n_cells, int32_t* regions,
                          int32_t* n_regions, int32_t* centers, int32_t* n_centers, uint8_t* windows, int32_t* comp,
                          long long* window_pixels);

/* ---- NuSeT's network stage (src/utils.py:35-103): the U-Net mask and the RPN proposal layer ------------------------------ */
/* Runs the loaded plan on ONE whole image and writes pred_masks (:53): x is the normalised (H, W) float32 image, the plan's input
 * tensor must be (H, W, 1) and its output the 2-channel logits of the same extent; mask (H, W) uint8 = argmax over the logits, a
 * tie giving 0 as tf.argmax does.  cls_tensor / bbox_tensor: the plan tensors of rpn_cls_score (fh, fw, 2A) and rpn_bbox_pred
 * (fh, fw, 4A) (src/model_layers/model_RPN.py:26-37), which the plan must keep alive to its end (keras_plan.build_plan: keep);
 * they stay on the handle for ecseg_rpn_proposals_last until the next forward call or model load (ecseg_read_tensor reads them
 * and the logits back).  A plan is built for one image extent: another extent needs ecseg_model_load again.  Device time of the
 * plan and the argmax in ECSEG_T_UNET. */
int ecseg_nuset_forward(ecseg_ctx* h, const float* x, int H, int W, int cls_tensor, int bbox_tensor, uint8_t* mask);
/* RPNProposal (src/model_layers/rpn_proposal.py) on the N = fh * fw * A candidates of cls_score (fh, fw, 2A) and bbox_pred
 * (fh, fw, 4A), float32 on the host; candidate (y * fw + x) * A + a has the anchor float32(ref_anchors[a] + (x, y, x, y) *
 * stride), the sum taken in float64 (src/nuset_utils/generate_anchors.py), ref_anchors being A x 4 float64 (x1, y1, x2, y2).
 *   score  = the second of softmax(cls[2a], cls[2a + 1]) in float32 (model_RPN.py:30-32);
 *   box    = decode(anchor, bbox[4a .. 4a + 3]) in float32 in the operation order of src/nuset_utils/bbox_transform_tf.py:41-66;
 *            exp is the correctly rounded float32 exponential;
 *   kept   where max(x2 - x1, 0) * max(y2 - y1, 0) > 0 and score >= 0 (NaN fails both);
 *   top-k  k = min(pre_nms_top_n, kept) by descending score, equal scores in ascending candidate order (tf.nn.top_k);
 *   NMS    greedy in that order as tf.image.non_max_suppression: corners min/max-normalised, a box of area <= 0 has IoU 0 with
 *          everything, a candidate is suppressed by a selected one when IoU > nms_threshold (strictly), at most post_nms_top_n
 *          are selected;
 *   clip   of the selected boxes to [0, im_w - 1] x [0, im_h - 1], after NMS (rpn_proposal.py:166-168).
 * Outputs, each with room for post_nms_top_n entries: scores (descending), proposals (x1, y1, x2, y2) and the selected candidates'
 * indices; *n_out their number, 0 when nothing is kept.  ECSEG_E_INVALID: fh * fw * A > ECSEG_RPN_MAX_CANDIDATES, pre_nms_top_n
 * outside 1 .. ECSEG_RPN_MAX_PRE_NMS, post_nms_top_n < 1, stride < 1.  Device time of the kernels in ECSEG_T_COUNT. */
#define ECSEG_RPN_MAX_CANDIDATES (1 << 22)
#define ECSEG_RPN_MAX_PRE_NMS    8192
int ecseg_rpn_proposals(ecseg_ctx* h, const float* cls_score, const float* bbox_pred, int fh, int fw, int A, const double* ref_anchors,
                        int stride, int im_h, int im_w, float nms_threshold, int pre_nms_top_n, int post_nms_top_n, int32_t* n_out,
                        float* scores, float* proposals, int32_t* indices);
/* The same on the two RPN tensors the last ecseg_nuset_forward left on the device (fh, fw and A are theirs; A x 4 reference
 * anchors must match their channel counts). */
int ecseg_rpn_proposals_last(ecseg_ctx* h, int A, const double* ref_anchors, int stride, int im_h, int im_w, float nms_threshold,
                             int pre_nms_top_n, int post_nms_top_n, int32_t* n_out, float* scores, float* proposals, int32_t* indices);

/* ---- NuSeT's marker watershed --------------------------------------------------------------------------------------------------
 * Replaces, for ONE image, src/model_layers/marker_watershed.py:82-91 behind the marker loops.  mask: (H, W) uint8, != 0 is
 * foreground; the n_markers markers (row, column, label >= 1) in the reference's order, a later one overwriting an earlier one on
 * the same pixel (ecseg_amd/nuset.py: watershed_markers builds the list of :22-80 on the host).  On the device:
 *   markers_rw = morphology.dilation(markers, disk(3)): the maximum label over the 29 offsets (:82), times the mask;
 *   distance   = distance_transform_edt(binary_fill_holes(mask)) (:83) as the exact integer d^2 (holes: 4-connected background
 *                components off the border; a filled mask without a zero gets scipy's answer, the distance to (-1, 0));
 *   contour    = segmentation.watershed(-distance, markers_rw, mask=mask, watershed_line=True) of scikit-image 0.18 (:84): one
 *                binary heap on (value, age) with that library's sift rules, replayed as one serial stream, because marker
 *                pixels of equal d^2 carry equal keys and the heap's order among them shows in the result;
 *   out (H, W) uint8 = mask where contour != 0, else 0 (:85,91).  A component no marker reaches stays 0; n_markers = 0 gives 0.
 * One synchronous call, buffers of its own, no host work per component or pixel; device time in ECSEG_T_COUNT.  The flood is
 * serial: its time grows with the foreground area (about five heap operations per pixel).  ECSEG_E_INVALID: null mask or out; H or
 * W outside 1 .. ECSEG_WATERSHED_MAX_EXTENT; n_markers < 0 or >= 2^31; a marker outside the image or with a label < 1. */
#define ECSEG_WATERSHED_MAX_EXTENT 16384
int ecseg_marker_watershed(ecseg_ctx* h, const uint8_t* mask, int H, int W, const int32_t* marker_rows, const int32_t* marker_cols,
                           const int32_t* marker_labels, long long n_markers, uint8_t* out);
/* The same for n_images images in ONE call: the flood of one image cannot be split, but the floods of different images do not know
 * of each other, so every image gets a wave of its own and they run side by side; every other step runs over all images at once.
 * masks: mask_bytes bytes holding the images, image i being the H x W bytes from byte `offset` on; images: n_images x 5 int64 rows
 * (offset, H, W, first_marker, n_markers), the image's markers being entries first_marker .. first_marker + n_markers - 1 of the
 * three lists (n_markers entries in all), rows and columns counted inside the image.  Images must not overlap: each starts at or
 * after the end of the one in front (ecseg_min_cut's rule for its windows); gaps are allowed.  out: mask_bytes bytes laid out as
 * masks.  Per image the call writes exactly the bytes ecseg_marker_watershed writes for that image alone; bytes of `out` outside
 * every image are 0; an image without a marker or without foreground gives zeros; n_images = 0 does nothing.  One synchronous
 * call, scratch from the handle's call arena (ecseg_marker_watershed_batch_bytes says how much), device time of the kernels in
 * ECSEG_T_COUNT: about that of the slowest image's flood, while there are no more images than the device runs waves at once.
 * ECSEG_E_INVALID: a null masks, images or out, or null lists with n_markers > 0; n_images outside 0 ..
 * ECSEG_WATERSHED_BATCH_MAX_IMAGES; mask_bytes < 0; n_markers < 0 or >= 2^31; H or W outside 1 .. ECSEG_WATERSHED_MAX_EXTENT; an
 * image that leaves masks or overlaps the one in front; a marker range that leaves the lists; a marker outside ITS image or with a
 * label < 1 (the message names the image and the list entry); an image with 5 * foreground + 1 >= 2^31.  ECSEG_E_NOMEM: the arena
 * cannot be had.  A heap that overflows its bound (5 * foreground + 1 elements, counted on the host per image) is reported as
 * ECSEG_E_HIP with the image's index. */
#define ECSEG_WATERSHED_BATCH_MAX_IMAGES 1024
int ecseg_marker_watershed_batch(ecseg_ctx* h, const uint8_t* masks, long long mask_bytes, const int64_t* images, int n_images,
                                 const int32_t* marker_rows, const int32_t* marker_cols, const int32_t* marker_labels, long long n_markers,
                                 uint8_t* out);
/* Host arithmetic only, no handle: the bytes of call arena ecseg_marker_watershed_batch needs for these images (as above; the marker
 * columns count too) when image i has foreground[i] non-zero pixels: 4 uint8 and 7 int32 values per byte up to the end of the last
 * image, 16 bytes per heap element (5 * foreground + 1 per image), 16 bytes of flags and a 40-byte table row per image, 12 bytes
 * per list entry in use, every buffer rounded up to 256 bytes.  0 for n_images = 0; -1 for arguments the call would refuse. */
long long ecseg_marker_watershed_batch_bytes(const int64_t* images, int n_images, const long long* foreground);
/* Test-only: ecseg_marker_watershed, the same driver and the same kernels in the same order, which also reads back what the stages
 * left on the device, each (H, W) and each pointer optional (null: not copied):
 *   rw     int32: markers_rw times the mask, the largest label over the disc's 29 offsets and 0 off the mask;
 *   filled uint8: binary_fill_holes(mask), 0 / 1;
 *   d2     int32: the squared distance to the nearest zero of `filled` on the mask's pixels and 0 off the mask (the flood reads it
 *                 nowhere else); (row + 1)^2 + column^2 when `filled` holds no zero;
 *   lab    int32: the flood's labels: 0 off the mask, where no marker reaches and on the lines, except that a marker pixel which
 *                 becomes a line keeps its label.
 * `out`, the status codes and the messages are ecseg_marker_watershed's; with four nulls the call is ecseg_marker_watershed. */
int ecseg_marker_watershed_stages_debug(ecseg_ctx* h, const uint8_t* mask, int H, int W, const int32_t* marker_rows, const int32_t* marker_cols,
                                        const int32_t* marker_labels, long long n_markers, uint8_t* out, int32_t* rw, uint8_t* filled,
                                        int32_t* d2, int32_t* lab);
/* Test-only: ecseg_marker_watershed_batch in the same way.  rw, filled, d2, lab: mask_bytes elements each (may be null), image i's
 * H x W values from element `offset` on, as its bytes lie in masks; the elements outside every image are not defined. */
int ecseg_marker_watershed_batch_stages_debug(ecseg_ctx* h, const uint8_t* masks, long long mask_bytes, const int64_t* images, int n_images,
                                              const int32_t* marker_rows, const int32_t* marker_cols, const int32_t* marker_labels,
                                              long long n_markers, uint8_t* out, int32_t* rw, uint8_t* filled, int32_t* d2, int32_t* lab);

/* ---- NuSeT's clean-up behind the marker watershed ----------------------------------------------------------------------------
 * Replaces, for ONE image, clean_image (src/nuset_utils/normalization.py:25-37) and the final threshold of nuclei_segment
 * (src/utils.py:159-162).  mask: (H, W) uint8, != 0 is foreground (what _watershed returns).
 *   mean_area = float32(foreground pixels) / number of 4-connected components, in float64 (:28-30; NaN without a component);
 *   remove_small_objects(min_size = mean_area / 5, connectivity = 2), then remove_small_holes(area_threshold = mean_area / 5,
 *   connectivity = 2), which also fills small background components at the border (:34-36); the areas are compared as
 *   float64(area) < mean_area / 5, so a NaN removes nothing -> cleaned (H, W) uint8 0 / 1 (may be null);
 *   the min-max scaling of utils.py:159 leaves an image of one value all zero (0 / 0), everything else becomes 0 / 255 (:160);
 *   remove_small_objects(bool, nuclei_size_T) with its default connectivity of 1 (:161): 4-connected components below
 *   nuclei_size_T pixels go, nuclei_size_T = 0 keeps all -> out (H, W) uint8 0 / 255.
 * *mean_area (may be null) receives mean_area.  One synchronous call, buffers of its own, nothing per component on the host;
 * device time of the kernels in ECSEG_T_COUNT.  ECSEG_E_INVALID: null mask or out, H or W < 1, H * W >= 2^31, nuclei_size_T < 0.
 * The results do not depend on the order of the atomics: two calls give identical bytes. */
int ecseg_clean_nuclei(ecseg_ctx* h, const uint8_t* mask, int H, int W, int nuclei_size_T, uint8_t* out, uint8_t* cleaned,
                       double* mean_area);

/* ---- NuSeT's two rescale calls (scale_ratio != 1) -------------------------------------------------------------------------------
 * Replace, for ONE image, rescale(image, s, anti_aliasing=True) (src/utils.py:136) and rescale(masks, 1 / s) with the threshold
 * behind it (:157-162) as scikit-image 0.18.3 / scipy 1.7.1 compute them.  All float64 arithmetic has the bits of the formulas below
 * (no fused multiply-add, the libraries' order of operations).
 *
 * ecseg_rescale_down.  img: (H, W) uint8.  The host passes the output extent (np.round(s * shape)) and per axis the 2 r + 1
 * float64 weights of scipy's gaussian_filter1d at sigma = max(0, (f - 1) / 2), f = extent / output extent, r = int(4 sigma + 0.5)
 * (ecseg_amd/_lib.py: rescale_weights); r = 0 copies that axis and its weights are not read.  On the device:
 *   the Gaussian on the uint8 image, axis 0 (wy, ry) first, then axis 1 (wx, rx), each pass writing uint8 by truncation; one
 *   output is tmp = in[i] * w[0], then for j = -r .. -1 in that order tmp += (in[i + j] + in[i - j]) * w[j] (w indexed from the
 *   centre), indices mirrored without repeating the edge sample (-1 -> 1) -> filtered (H, W) uint8 (may be null);
 *   the order-1 warp of p = filtered / 255: per output row r, y = f_y * (r + 0.5) - 0.5, y0 = floor(y), y1 = ceil(y), dy = y - y0,
 *   columns alike; top = (1 - dx) * p(y0, x0) + dx * p(y0, x1), bottom alike on y1, value = (1 - dy) * top + dy * bottom, indices
 *   mirrored the same way -> out (out_h, out_w) float64.
 * ECSEG_E_INVALID: null img, out or (r > 0) weights; an extent < 1; H * W >= 2^31; out_h > H or out_w > W; ry >= H or rx >= W (one
 * reflection always suffices); a radius < 0 or above ECSEG_RESCALE_MAX_RADIUS (s = 0.05 needs 38).
 *
 * ecseg_rescale_mask_up.  cleaned: (H, W) uint8, clean_image's 0 / 1.  On the device: v = the same warp of cleaned / 255 to
 * (out_h, out_w) (no filter: f < 1); vmin and vmax over the output; uint8(((v - vmin) / (vmax - vmin)) * 255) > 0 in float64 (an
 * image of one value divides 0 by 0 and comes out all zero); remove_small_objects(bool, nuclei_size_T): 4-connected components
 * below nuclei_size_T pixels go, 0 keeps all -> out (out_h, out_w) uint8 0 / 255.  ECSEG_E_INVALID: null cleaned or out, an extent
 * < 1, out_h * out_w >= 2^31, nuclei_size_T < 0, out_h < H or out_w < W.
 *
 * Both: one synchronous call, buffers owned by the handle, nothing per pixel or component on the host; device time of the kernels in
 * ECSEG_T_COUNT.  No result depends on the order of the atomics: two calls give identical bytes. */
#define ECSEG_RESCALE_MAX_RADIUS 64
int ecseg_rescale_down(ecseg_ctx* h, const uint8_t* img, int H, int W, int out_h, int out_w, const double* wy, int ry, const double* wx,
                       int rx, uint8_t* filtered, double* out);
int ecseg_rescale_mask_up(ecseg_ctx* h, const uint8_t* cleaned, int H, int W, int out_h, int out_w, int nuclei_size_T, uint8_t* out);

/* ---- per-stage device timings of the last segment call (milliseconds, HIP events on the handle's stream) -- */
/* ECSEG_T_COUNT: device time of the kernels of the last ecseg_overlay / ecseg_preprocess / ecseg_count_* call (inputs
 * already resident, copies excluded). */
enum { ECSEG_T_TILE = 0, ECSEG_T_UNET = 1, ECSEG_T_TAIL = 2, ECSEG_T_POST = 3, ECSEG_T_COUNT = 4, ECSEG_T_N = 5 };
int ecseg_get_timings(ecseg_ctx* h, float* ms_out /* [ECSEG_T_N] */);
/* Average duration (ms) and launch count of the dominant kernel (MFMA conv) over the last segment/forward call,
 * measured with HIP events around every launch when profiling is enabled (adds a little launch overhead). */
int ecseg_set_kernel_profiling(ecseg_ctx* h, int enabled);
int ecseg_get_conv_profile(ecseg_ctx* h, double* total_ms, int64_t* launches, double* flops);
/* FLOPs the matrix cores actually executed in those launches (Winograd F(2x2,3x3) issues 16/36 of the algorithmic
 * multiplies of a 3x3 convolution; the direct kernel issues all of them). */
int ecseg_get_conv_executed_flops(ecseg_ctx* h, double* flops);
/* Per-launch records of the same profile, in launch order: plan operator index, kind, duration, algorithmic and executed
 * FLOPs.  kind bits 0-7 = kernel family (0 direct implicit GEMM conv_mfma_kernel, 1 Winograd F(2x2,3x3) conv_wino_kernel,
 * 2 Winograd F(4x4,3x3) conv_wino4_kernel, 3 filter-resident F(2x2) conv_wino_res_kernel, 4 F(2x2) on 16x16x4 MFMAs
 * conv_wino16_kernel); bit 8 (0x100): the launch also wrote the 2x2 max-pool that follows in the plan; bit 9 (0x200): it
 * also finished the 1x1 head that follows (the convolution's own output was not written); bit 10 (0x400): it also computed the
 * network's first layer (the plan operator in front of op_index) into its own halo ("fuse_first").  Returns the number of records
 * written (<= max_records) or a negative error. */
int ecseg_get_conv_launch_profile(ecseg_ctx* h, int max_records, int32_t* op_index, int32_t* kind, float* ms,
                                  double* flops, double* executed_flops);
/* Diagnostics only (-DECSEG_DIAG builds; ECSEG_E_UNSUPPORTED otherwise): up to 240 floats of in-kernel cycle stamps written by the ECSEG_WINO_STAMP build of the conv kernel. */
int ecseg_debug_peek(ecseg_ctx* h, float* out, int n);

/* ---- host-side byte codecs for the file I/O around the path (no GPU work) ---------------------------------- */
/* TIFF LZW (MSB-first, 9..12-bit codes, early change): inputs read by imread (src/utils.py:110) and the
 * dapi/<name>.tif written by cv2.imwrite (src/utils.py:122-123).  Return bytes written, or -1 on error. */
long long ecseg_lzw_decode(const uint8_t* src, long long n, uint8_t* dst, long long dst_cap);
long long ecseg_lzw_encode(const uint8_t* src, long long n, uint8_t* dst, long long dst_cap);

/* ---- whole-file readers / writers of `make metaseg` / `make meta_overlay` (host only; thread-safe, no handle) --------
 * Called through ctypes they run without the interpreter lock, so the I/O threads of ecseg_amd/metaseg.py scale over the
 * host cores.  Return ECSEG_OK, ECSEG_E_INVALID (bad argument / corrupt file), ECSEG_E_IO, or - readers only -
 * ECSEG_E_UNSUPPORTED for a valid TIFF layout that is left to the Python reader (tiles, BigTIFF, PackBits, float). */
/* np.save(labels/<stem>.npy, I.astype(int64)) (src/metaseg.py:53): byte-identical to numpy's format-1.0 writer. */
int ecseg_npy_write_i64(const char* path, const uint8_t* labels, int H, int W);
/* plt.imsave(labels/<stem>.png, I, cmap=ListedColormap([4 colours]), vmin=0, vmax=4) (src/metaseg.py:47-52): RGBA. */
int ecseg_png_write_labels(const char* path, const uint8_t* labels, int H, int W);
/* The zlib stream of that file: *stream_bytes its length as written, *formula_bytes the length worked out from the 68 token counts
 * before a bit is written (what ecseg_png_labels_encode sizes its device buffer by): always equal. */
int ecseg_png_labels_stream_size(const uint8_t* labels, int H, int W, long long* formula_bytes, long long* stream_bytes);
/* 8-bit gray / RGB / RGBA PNG (channels 1 / 3 / 4; zlib level 0..9, or -1: the settings of cv2.imwrite without parameters -
 * SUB filter, Z_BEST_SPEED, Z_RLE strategy): red/ and green/ of split_FISH_channels (src/image_tools.py:136-146). */
int ecseg_png_write(const char* path, const uint8_t* pixels, int H, int W, int channels, int level);
/* cv2.imwrite(red/<name>.png, cv2.bitwise_not(np.uint8(I[..., c]))) (src/image_tools.py:143-144): channel `channel` of an interleaved
 * 8-bit (H, W, channels) image as a gray PNG, inverted when invert != 0, with cv2's default encoder settings. */
int ecseg_png_write_channel(const char* path, const uint8_t* pixels, int H, int W, int channels, int channel, int invert);
/* np.load(labels/<stem>.npy) narrowed to uint8 while it is read (read_seg, src/utils.py:125-132; src/meta_overlay.py:59): C-order
 * 2-D integer arrays (the int64 file `make metaseg` writes, src/metaseg.py:53); ECSEG_E_UNSUPPORTED for any other layout. */
int ecseg_npy_label_info(const char* path, int* H, int* W);
int ecseg_npy_read_labels_u8(const char* path, uint8_t* dst, int H, int W);
/* cv2.imwrite(dapi/<name>.tif, gray) (src/utils.py:122-123): LZW + predictor 2, strips of 8192 / W rows; invert != 0
 * stores 255 - img (cv2.bitwise_not, src/utils.py:112). */
int ecseg_tiff_write_gray8(const char* path, const uint8_t* img, int H, int W, int invert);
/* cv2.imwrite(x.tif, 8-bit 3-channel image) (src/stat_fish.py:306-308): 3 samples per pixel, RGB photometric interpretation, the
 * samples stored in the order given (the caller hands over RGB; cv2 turns its BGR arrays into RGB files), LZW + predictor 2,
 * strips of 8192 / (3 W) rows. */
int ecseg_tiff_write_rgb8(const char* path, const uint8_t* img, int H, int W);
/* np.save(path, labels) of an int64 (H, W) array whose values the caller holds as int32 (src/stat_fish.py:302,
 * <name>__segmentation_min_cut.npy): byte-identical to numpy's file of labels.astype(int64). */
int ecseg_npy_write_i32_as_i64(const char* path, const int32_t* labels, int H, int W);
/* skimage.io.imread of a baseline TIFF (src/utils.py:110): shape first, then the samples as native-endian (H, W, spp). */
int ecseg_tiff_info(const char* path, int* H, int* W, int* samples_per_pixel, int* bits_per_sample);
int ecseg_tiff_read(const char* path, void* dst, long long dst_bytes);

/* ---- the path's one exchange step: all-gather of per-image result records over RCCL (xGMI) ---------------------------
 * Image-parallel sharding needs no data-path collective (every image is independent: src/metaseg.py:42 is a serial loop);
 * at the end every rank contributes its block of fixed-size records and rank 0 writes ec_quantification.csv
 * (src/metaseg.py:44-57).  Record = ECSEG_RECORD_INT64 int64: [0] global image index (-1 = padding of the last shard)
 * [1] status (0 ok) [2] n_ec [3..14] the twelve fields of ecseg_overlay [15] reserved.  Shards are padded to equal length.
 * librccl.so is loaded on first use (no link-time dependency); ECSEG_E_UNSUPPORTED when it is not installed.
 * Every wait is bounded: ecseg_comm_create and the synchronous all-gathers return ECSEG_E_HIP with a message when the peers do
 * not answer within ECSEG_COMM_TIMEOUT_S seconds (environment variable, default 300) - the communicator is aborted and unusable
 * afterwards (ecseg_comm_destroy it).
 * Rendezvous: rank 0 obtains ECSEG_COMM_ID_BYTES from ecseg_comm_unique_id and hands them to the other ranks by any channel
 * of the host's (file, environment, socket); then every rank calls ecseg_comm_create (collective).  One process per GPU. */
#define ECSEG_RECORD_INT64  16
#define ECSEG_COMM_ID_BYTES 128
typedef struct ecseg_comm ecseg_comm;
int         ecseg_comm_unique_id(void* out, int out_bytes);
int         ecseg_comm_create(ecseg_comm** out, const void* unique_id, int rank, int world, int device_id);
void        ecseg_comm_destroy(ecseg_comm* c);
const char* ecseg_comm_last_error(void);          /* text of the calling thread's last failed ecseg_comm_* / all-gather call */
/* host buffers: n_records records in, world * n_records out (rank-major); synchronous */
int ecseg_allgather_records(ecseg_comm* c, const int64_t* send, int n_records, int64_t* recv);
/* device buffers; stream (hipStream_t as void*) non-null: returns once enqueued on it; null: own stream, synchronous */
int ecseg_allgather_records_dev(ecseg_comm* c, const int64_t* send_dev, int n_records, int64_t* recv_dev, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* ECSEG_HIP_H */
