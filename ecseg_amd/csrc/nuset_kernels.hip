// NuSeT's network stage behind the U-Net plan (src/utils.py:35-103): the argmax mask and the RPN proposal layer
// (src/model_layers/rpn_proposal.py, src/nuset_utils/bbox_transform_tf.py, src/nuset_utils/generate_anchors.py).
//
// Proposals, for N = fh * fw * A candidates with candidate i = (y * fw + x) * A + a:
//   rpn_decode_kernel   score, decode and the keep test of every candidate; a 64-bit sort key per candidate - the complemented bits
//                       of the score above the candidate index, so that ascending keys are descending scores with the lower index
//                       first among equals (tf.nn.top_k); candidates that fail the keep test and the padding up to a power of two
//                       get the all-ones key and sort behind everything
//   bitonic_*_kernel    the sort: blocks of 2048 keys in LDS, the strides above that in global memory
//   nms_matrix_kernel   bit (i, j), j > i, of a triangular matrix over the first K sorted candidates: IoU(i, j) > nms_threshold
//   nms_sweep_kernel    ONE wavefront walks the candidates in order as tf.image.non_max_suppression does (greedy, stops at
//                       post_nms_top_n), ORs the row of every selected candidate into the removed set held in LDS, and writes the
//                       clipped outputs (clip_boxes runs after NMS, rpn_proposal.py:166-168)
// Nothing comes back to the host in between: k = min(pre_nms_top_n, kept) is read by the sweep from the decode kernel's counter.
//
// Arithmetic is TensorFlow's float32, operation by operation: this file is compiled without floating-point contraction (the
// pragma below and build.py), so a * b + c rounds twice as two TensorFlow ops do.  exp is float32(exp(float64(x))): the correctly
// rounded float32 exponential (up to double rounding, relative 2^-29 of the cases), which a numpy restatement can state the same
// way; a float32 exp of 1 ulp - TensorFlow's own is no better defined - would make scores depend on the library.
#include "common.h"

#pragma STDC FP_CONTRACT OFF

namespace ecseg {
namespace {

constexpr int SORT_BLOCK = 2048;          // keys of one LDS block
constexpr int SORT_THREADS = 256;
constexpr unsigned long long KEY_NONE = ~0ull;

__device__ __forceinline__ float exp32(float v) { return (float)exp((double)v); }

__global__ __launch_bounds__(256) void argmax2_kernel(const float* __restrict__ logits, int cs, size_t px, uint8_t* __restrict__ mask) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= px) return;
    const float* p = logits + i * (size_t)cs;
    mask[i] = p[1] > p[0] ? 1 : 0;                           // a tie is class 0 (tf.argmax returns the first maximum)
}

__global__ __launch_bounds__(256) void rpn_decode_kernel(const float* __restrict__ cls, int cls_cs, const float* __restrict__ bbox, int bbox_cs,
                                                         const double* __restrict__ ref, int A, int fw, int N, int P, int stride,
                                                         float4* __restrict__ boxes, float* __restrict__ scores,
                                                         unsigned long long* __restrict__ keys, int32_t* __restrict__ misc) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    bool keep = false;
    if (i < N) {
        const int pos = i / A, a = i - pos * A;
        const int y = pos / fw, x = pos - y * fw;
        // softmax over (background, foreground), model_RPN.py:30-32
        const float* c = cls + (size_t)pos * cls_cs + 2 * a;
        const float c0 = c[0], c1 = c[1];
        const float m = fmaxf(c0, c1);
        const float e0 = exp32(c0 - m), e1 = exp32(c1 - m);
        const float score = e1 / (e0 + e1);
        // the anchor: float32 of the float64 sum (generate_anchors.py:39-48)
        const double sx = (double)(x * stride), sy = (double)(y * stride);
        const float ax1 = (float)(ref[4 * a + 0] + sx), ay1 = (float)(ref[4 * a + 1] + sy);
        const float ax2 = (float)(ref[4 * a + 2] + sx), ay2 = (float)(ref[4 * a + 3] + sy);
        // decode, bbox_transform_tf.py:41-66 (variances 1)
        const float* d = bbox + (size_t)pos * bbox_cs + 4 * a;
        const float dx = d[0], dy = d[1], dw = d[2], dh = d[3];
        const float w = ax2 - ax1 + 1.f, h = ay2 - ay1 + 1.f;
        const float urx = ax1 + .5f * w, ury = ay1 + .5f * h;
        const float px = dx * w + urx, py = dy * h + ury;
        const float pw = exp32(dw) * w, ph = exp32(dh) * h;
        const float x1 = px - .5f * pw, y1 = py - .5f * ph;
        const float x2 = px + .5f * pw - 1.f, y2 = py + .5f * ph - 1.f;
        // rpn_proposal.py:86-96 (NaN fails both comparisons)
        keep = fmaxf(x2 - x1, 0.f) * fmaxf(y2 - y1, 0.f) > 0.f && score >= 0.f;
        boxes[i] = make_float4(x1, y1, x2, y2);
        scores[i] = score;
        keys[i] = keep ? ((unsigned long long)(~__float_as_uint(score)) << 32) | (unsigned)i : KEY_NONE;
    } else if (i < P) {
        keys[i] = KEY_NONE;
    }
    const unsigned long long b = __ballot(keep);
    if ((threadIdx.x & 63) == 0 && b) atomicAdd(&misc[1], __popcll(b));
}

// compare-exchange of pair q at stride j inside a sequence of length k: ascending where bit k of the index is clear
__device__ __forceinline__ void bitonic_pair(unsigned long long* v, int lo, int j, bool asc) {
    const unsigned long long a = v[lo], b = v[lo + j];
    if ((a > b) == asc) { v[lo] = b; v[lo + j] = a; }
}

// sequence lengths k_lo .. k_hi of one 2048-key block in LDS, each from stride min(k / 2, 1024) down to 1
__global__ __launch_bounds__(SORT_THREADS) void bitonic_block_kernel(unsigned long long* __restrict__ keys, int k_lo, int k_hi) {
    __shared__ unsigned long long v[SORT_BLOCK];
    const int base = blockIdx.x * SORT_BLOCK;
    for (int t = threadIdx.x; t < SORT_BLOCK; t += SORT_THREADS) v[t] = keys[base + t];
    __syncthreads();
    for (int k = k_lo; k <= k_hi; k <<= 1) {
        for (int j = k / 2 < SORT_BLOCK / 2 ? k / 2 : SORT_BLOCK / 2; j > 0; j >>= 1) {
            for (int q = threadIdx.x; q < SORT_BLOCK / 2; q += SORT_THREADS) {
                const int lo = ((q & ~(j - 1)) << 1) | (q & (j - 1));
                bitonic_pair(v, lo, j, ((base + lo) & k) == 0);
            }
            __syncthreads();
        }
    }
    for (int t = threadIdx.x; t < SORT_BLOCK; t += SORT_THREADS) keys[base + t] = v[t];
}

// one stride j >= 2048 of sequence length k over all P keys
__global__ __launch_bounds__(256) void bitonic_global_kernel(unsigned long long* __restrict__ keys, int half, int j, int k) {
    const int q = blockIdx.x * 256 + threadIdx.x;
    if (q >= half) return;
    const int lo = ((q & ~(j - 1)) << 1) | (q & (j - 1));
    bitonic_pair(keys, lo, j, (lo & k) == 0);
}

struct NBox { float x0, y0, x1, y1, area; };

// tf.image.non_max_suppression normalises the corners; a box of area <= 0 has IoU 0 with everything
__device__ __forceinline__ NBox nbox_of(const unsigned long long* keys, const float4* boxes, int j, int K) {
    NBox r{0.f, 0.f, 0.f, 0.f, 0.f};
    if (j >= K) return r;
    const unsigned long long key = keys[j];
    if (key == KEY_NONE) return r;
    const float4 b = boxes[(unsigned)key];
    r.x0 = fminf(b.x, b.z); r.x1 = fmaxf(b.x, b.z);
    r.y0 = fminf(b.y, b.w); r.y1 = fmaxf(b.y, b.w);
    r.area = (r.y1 - r.y0) * (r.x1 - r.x0);
    return r;
}

__global__ __launch_bounds__(64) void nms_matrix_kernel(const unsigned long long* __restrict__ keys, const float4* __restrict__ boxes, int K, int words,
                                                       float thr, unsigned long long* __restrict__ mat) {
    const int rb = blockIdx.y, cb = blockIdx.x;
    if (cb < rb) return;                                     // bits j > i only
    __shared__ NBox col[64];
    col[threadIdx.x] = nbox_of(keys, boxes, cb * 64 + threadIdx.x, K);
    __syncthreads();
    const int i = rb * 64 + threadIdx.x;
    if (i >= K) return;
    const NBox r = nbox_of(keys, boxes, i, K);
    unsigned long long bits = 0;
    if (r.area > 0.f) {
        for (int jj = 0; jj < 64; ++jj) {
            const NBox c = col[jj];
            if (cb * 64 + jj <= i || !(c.area > 0.f)) continue;
            const float ih = fmaxf(fminf(r.y1, c.y1) - fmaxf(r.y0, c.y0), 0.f);
            const float iw = fmaxf(fminf(r.x1, c.x1) - fmaxf(r.x0, c.x0), 0.f);
            const float inter = ih * iw;
            const float iou = inter / (r.area + c.area - inter);
            if (iou > thr) bits |= 1ull << jj;
        }
    }
    mat[(size_t)i * words + cb] = bits;
}

__global__ __launch_bounds__(64) void nms_sweep_kernel(const unsigned long long* __restrict__ mat, const unsigned long long* __restrict__ keys,
                                                      const float4* __restrict__ boxes, const float* __restrict__ scores, int K, int words,
                                                      int pre, int post, float xmax, float ymax, float* __restrict__ out_scores,
                                                      float4* __restrict__ out_boxes, int32_t* __restrict__ out_idx, int32_t* __restrict__ misc) {
    __shared__ unsigned long long removed[ECSEG_RPN_MAX_PRE_NMS / 64];
    const int lane = threadIdx.x;
    for (int w = lane; w < words; w += 64) removed[w] = 0;
    __syncthreads();
    const int kept = misc[1];
    const int k = min(min(pre, kept), K);
    int n = 0;
    for (int i = 0; i < k && n < post; ++i) {
        if ((removed[i >> 6] >> (i & 63)) & 1ull) continue;  // (the same word for every lane: the branch is uniform)
        if (lane == 0) {
            const unsigned idx = (unsigned)keys[i];
            const float4 b = boxes[idx];
            out_idx[n] = (int32_t)idx;
            out_scores[n] = scores[idx];
            out_boxes[n] = make_float4(fmaxf(fminf(b.x, xmax), 0.f), fmaxf(fminf(b.y, ymax), 0.f), fmaxf(fminf(b.z, xmax), 0.f),
                                       fmaxf(fminf(b.w, ymax), 0.f));
        }
        ++n;
        for (int w = (i >> 6) + lane; w < words; w += 64) removed[w] |= mat[(size_t)i * words + w];
        __syncthreads();
    }
    if (lane == 0) misc[0] = n;
}

}  // namespace

hipError_t launch_argmax2(const TView& logits, uint8_t* mask, hipStream_t s) {
    const size_t px = (size_t)logits.h * logits.w;
    argmax2_kernel<<<dim3((unsigned)((px + 255) / 256)), dim3(256), 0, s>>>(logits.p, logits.cs, px, mask);
    return hipGetLastError();
}

int rpn_sort_len(int N) {
    int P = SORT_BLOCK;
    while (P < N) P <<= 1;
    return P;
}

hipError_t run_rpn_proposals(const float* cls, int cls_cs, const float* bbox, int bbox_cs, const double* ref, int fh, int fw, int A, int stride,
                             int im_h, int im_w, float nms_threshold, int pre, int post, const RpnBufs& b, hipStream_t s) {
    const int N = fh * fw * A, P = rpn_sort_len(N);
    const int K = pre < N ? pre : N, words = (K + 63) / 64;
    hipError_t e = hipMemsetAsync(b.misc, 0, 2 * sizeof(int32_t), s);
    if (e != hipSuccess) return e;
    rpn_decode_kernel<<<dim3(P / 256), dim3(256), 0, s>>>(cls, cls_cs, bbox, bbox_cs, ref, A, fw, N, P, stride, b.boxes, b.scores, b.keys, b.misc);
    bitonic_block_kernel<<<dim3(P / SORT_BLOCK), dim3(SORT_THREADS), 0, s>>>(b.keys, 2, SORT_BLOCK);
    for (int k = 2 * SORT_BLOCK; k <= P; k <<= 1) {
        for (int j = k / 2; j >= SORT_BLOCK; j >>= 1)
            bitonic_global_kernel<<<dim3(P / 2 / 256), dim3(256), 0, s>>>(b.keys, P / 2, j, k);
        bitonic_block_kernel<<<dim3(P / SORT_BLOCK), dim3(SORT_THREADS), 0, s>>>(b.keys, k, k);
    }
    nms_matrix_kernel<<<dim3(words, words), dim3(64), 0, s>>>(b.keys, b.boxes, K, words, nms_threshold, b.mat);
    nms_sweep_kernel<<<dim3(1), dim3(64), 0, s>>>(b.mat, b.keys, b.boxes, b.scores, K, words, pre, post, (float)im_w - 1.f, (float)im_h - 1.f,
                                                  b.out_scores, b.out_boxes, b.out_idx, b.misc);
    return hipGetLastError();
}

}  // namespace ecseg
