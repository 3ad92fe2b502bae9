// The two ends of the post-processing that label nothing, for gfx950: stitch + quantised argmax with its tie reduce, and
// meta_preprocess (extract gray, u16 -> u8, histogram, Otsu, invert).  HBM-bound per-pixel kernels; one file because each part is
// about a hundred lines.  From ccl.h they take PX_LOOP / px_grid only.
#include "ccl.h"

namespace ecseg {

// ---------------------------------------------------------------------------------------------------------------
// stitch + img_as_ubyte + argmax (src/image_tools.py:188-252, src/utils.py:117-118)
// ---------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void stitch_argmax_kernel(const float* __restrict__ probs, int prob_cs,
                                                            const int32_t* __restrict__ src_map, int n_pos, size_t px,
                                                            uint8_t* __restrict__ labels, size_t total,
                                                            int32_t* __restrict__ tie_risk) {
    __shared__ int s_im, s_cnt;
    int cnt = 0, cur = -1;                                 // tie-risk pixels of image `cur` seen by this thread
    PX_LOOP(total) {
        const size_t im = t / px, q = t - im * px;
        const int src = src_map[q];
        uint8_t lab = 0;                       // never-written canvas pixels stay 0.0 in every channel -> argmax 0
        bool tie = false;
        if (src >= 0) {
            const size_t patch = im * n_pos + (size_t)(src >> 16);
            const float* pp = probs + ((patch << 16) + (size_t)(src & 0xffff)) * prob_cs;
            int best = -1, second = -1;
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                // float64(p) * 255 is exact; rint = round half to even; clip to [0, 255]
                double v = rint((double)pp[c] * 255.0);
                v = v < 0.0 ? 0.0 : (v > 255.0 ? 255.0 : v);
                const int qv = (int)v;
                if (qv > best) { second = best; best = qv; lab = (uint8_t)c; }   // strict '>' keeps the first maximum
                else if (qv > second) second = qv;
            }
            tie = best - second <= 1;           // a last-bit difference in one probability can change this pixel's label
        }
        labels[t] = lab;
        if (tie_risk) {
            if ((int)im != cur) {                              // (a thread's pixels cross an image boundary a few times per launch at most)
                if (cnt) atomicAdd(tie_risk + ((size_t)cur * G_SHARDS + blockIdx.x % G_SHARDS) * G_STRIDE, cnt);
                cur = (int)im; cnt = 0;
            }
            cnt += tie ? 1 : 0;
        }
    }
    if (tie_risk) {
        // one global atomic per workgroup, into one of G_SHARDS replicas of the image's counter (each on its own 128-B line):
        // device-scope atomics on ONE line serialise at ~200 ns each across the XCDs - 16 k workgroups adding to the 16
        // counters of a launch group, all in one line, took 3.2 ms (the whole stitch: 0.09 ms)
        if (threadIdx.x == 0) { s_im = cur; s_cnt = 0; }
        __syncthreads();
        if (cnt) {
            if (cur == s_im) atomicAdd(&s_cnt, cnt);
            else atomicAdd(tie_risk + ((size_t)cur * G_SHARDS + blockIdx.x % G_SHARDS) * G_STRIDE, cnt);
        }
        __syncthreads();
        if (threadIdx.x == 0 && s_cnt) atomicAdd(tie_risk + ((size_t)s_im * G_SHARDS + blockIdx.x % G_SHARDS) * G_STRIDE, s_cnt);
    }
}

__global__ __launch_bounds__(256) void stitch_probs_kernel(const float* __restrict__ probs, int prob_cs,
                                                           const int32_t* __restrict__ src_map, int n_pos, size_t px,
                                                           float* __restrict__ out, size_t total) {
    PX_LOOP(total) {
        const size_t im = t / px, q = t - im * px;
        const int src = src_map[q];
        f32x4 v = {0.f, 0.f, 0.f, 0.f};
        if (src >= 0) {
            const size_t patch = im * n_pos + (size_t)(src >> 16);
            const float* pp = probs + ((patch << 16) + (size_t)(src & 0xffff)) * prob_cs;
#pragma unroll
            for (int c = 0; c < 4; ++c) v[c] = pp[c];
        }
        *reinterpret_cast<f32x4*>(out + t * 4) = v;
    }
}

__global__ void tie_reduce_kernel(const int32_t* __restrict__ shards, int32_t* __restrict__ out, int n_img) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_img) return;
    int v = 0;
    for (int k = 0; k < G_SHARDS; ++k) v += shards[((size_t)i * G_SHARDS + k) * G_STRIDE];
    out[i] = v;
}

hipError_t launch_stitch_argmax(const float* probs, int prob_cs, const int32_t* src_map, int n_img, int n_pos, int H, int W,
                                uint8_t* labels, hipStream_t s, int32_t* tie_risk, int32_t* tie_shards) {
    const size_t px = (size_t)H * W, total = px * n_img;
    if (!total) return hipSuccess;
    const bool tie = tie_risk != nullptr && tie_shards != nullptr;
    if (tie) {
        hipError_t e = hipMemsetAsync(tie_shards, 0, (size_t)n_img * G_SHARDS * G_STRIDE * sizeof(int32_t), s);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(stitch_argmax_kernel, dim3(px_grid(total)), dim3(256), 0, s, probs, prob_cs, src_map, n_pos, px,
                       labels, total, tie ? tie_shards : nullptr);
    if (tie) hipLaunchKernelGGL(tie_reduce_kernel, dim3((n_img + 63) / 64), dim3(64), 0, s, tie_shards, tie_risk, n_img);
    return hipGetLastError();
}

hipError_t launch_stitch_probs(const float* probs, int prob_cs, const int32_t* src_map, int n_img, int n_pos, int H, int W,
                               float* out, hipStream_t s) {
    const size_t px = (size_t)H * W, total = px * n_img;
    if (!total) return hipSuccess;
    hipLaunchKernelGGL(stitch_probs_kernel, dim3(px_grid(total)), dim3(256), 0, s, probs, prob_cs, src_map, n_pos, px, out, total);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------------------------
// meta_preprocess (src/image_tools.py:86-101)
// ---------------------------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(256) void extract_gray_kernel(const T* __restrict__ img, int C, uint8_t* __restrict__ gray,
                                                           size_t total) {
    const int ch = C > 1 ? 2 : 0;
    PX_LOOP(total) {
        const T v = img[t * C + ch];
        if (sizeof(T) == 2) {
            // cv2.convertScaleAbs(alpha = 255/65535): saturate_cast<uchar>(|float(v) * float(alpha)|), round half even
            const float f = fabsf((float)v * (float)(255.0 / 65535.0));
            int r = __float2int_rn(f);
            gray[t] = (uint8_t)(r > 255 ? 255 : r);
        } else {
            gray[t] = (uint8_t)v;
        }
    }
}

hipError_t launch_u16_to_u8(const uint16_t* in, uint8_t* out, size_t count, hipStream_t s) {
    if (!count) return hipSuccess;
    hipLaunchKernelGGL(extract_gray_kernel<uint16_t>, dim3(px_grid(count)), dim3(256), 0, s, in, 1, out, count);
    return hipGetLastError();
}

__global__ __launch_bounds__(256) void hist256_kernel(const uint8_t* __restrict__ gray, size_t px, uint32_t* __restrict__ hist,
                                                      int blocks_per_img) {
    __shared__ uint32_t h[256];
    const int im = blockIdx.x / blocks_per_img, j = blockIdx.x % blocks_per_img;
    h[threadIdx.x] = 0;
    __syncthreads();
    const uint8_t* g = gray + (size_t)im * px;
    for (size_t t = (size_t)j * 256 + threadIdx.x; t < px; t += (size_t)blocks_per_img * 256) atomicAdd(&h[g[t]], 1u);
    __syncthreads();
    if (h[threadIdx.x]) atomicAdd(hist + (size_t)im * 256 + threadIdx.x, h[threadIdx.x]);
}

// Otsu threshold (OpenCV getThreshVal_Otsu_8u restated) + the "> 50 % white" decision; one thread per image.  px_img (may be null:
// every image has px_all pixels, as in the product): the pixel count of each image, the sum of its histogram; threshold (may be null)
__global__ void otsu_decide_kernel(const uint32_t* __restrict__ hist, int n_img, size_t px_all, const long long* __restrict__ px_img,
                                   int32_t* __restrict__ inverted, int32_t* __restrict__ threshold) {
    // every a * b + c below rounds twice, as in OpenCV's build and in oracle/preprocess.py: contracted into fused multiply-adds
    // (q1 + h * scale, mu1 + i * p_i, mu - q1 * mu1) the last bit of sigma changes, and with it the winner of two near-equal maxima
#pragma clang fp contract(off)
    const int im = blockIdx.x * blockDim.x + threadIdx.x;
    if (im >= n_img) return;
    const uint32_t* h = hist + (size_t)im * 256;
    const size_t px = px_img ? (size_t)px_img[im] : px_all;
    const double scale = 1.0 / (double)px;
    double mu = 0.0;
    for (int i = 0; i < 256; ++i) mu += (double)i * (double)h[i];
    mu *= scale;
    double mu1 = 0.0, q1 = 0.0, max_sigma = 0.0;
    int max_val = 0;
    const double eps = 1.1920928955078125e-07;   // FLT_EPSILON
    for (int i = 0; i < 256; ++i) {
        const double p_i = (double)h[i] * scale;
        mu1 *= q1;
        q1 += p_i;
        const double q2 = 1.0 - q1;
        if (fmin(q1, q2) < eps || fmax(q1, q2) > 1.0 - eps) continue;
        mu1 = (mu1 + (double)i * p_i) / q1;
        const double mu2 = (mu - q1 * mu1) / q2;
        const double sigma = q1 * q2 * (mu1 - mu2) * (mu1 - mu2);
        if (sigma > max_sigma) { max_sigma = sigma; max_val = i; }
    }
    unsigned long long white = 0;
    for (int i = max_val + 1; i < 256; ++i) white += h[i];
    inverted[im] = ((double)white > (double)px * 0.5) ? 1 : 0;
    if (threshold) threshold[im] = max_val;
}

hipError_t launch_otsu_decide(const uint32_t* hist, int n_img, const long long* px_img, int32_t* inverted, int32_t* threshold, hipStream_t s) {
    if (n_img <= 0) return hipSuccess;
    if (!px_img) return hipErrorInvalidValue;                // (no count for all images here: 1 / 0 otherwise)
    hipLaunchKernelGGL(otsu_decide_kernel, dim3((n_img + 63) / 64), dim3(64), 0, s, hist, n_img, (size_t)0, px_img, inverted, threshold);
    return hipGetLastError();
}

__global__ __launch_bounds__(256) void invert_kernel(uint8_t* __restrict__ gray, const int32_t* __restrict__ inverted,
                                                     size_t px, size_t total) {
    PX_LOOP(total) {
        if (inverted[t / px]) gray[t] = (uint8_t)~gray[t];
    }
}

hipError_t run_preprocess(const void* img, int n_img, int H, int W, int C, int bps, uint8_t* gray, int32_t* inverted,
                          uint32_t* hist_ws, hipStream_t s, int32_t* threshold) {
    if (n_img <= 0) return hipSuccess;
    const size_t px = (size_t)H * W, total = px * n_img;
    const unsigned pg = px_grid(total);
    if (bps == 2) hipLaunchKernelGGL(extract_gray_kernel<uint16_t>, dim3(pg), dim3(256), 0, s, (const uint16_t*)img, C, gray, total);
    else hipLaunchKernelGGL(extract_gray_kernel<uint8_t>, dim3(pg), dim3(256), 0, s, (const uint8_t*)img, C, gray, total);
    hipError_t e = hipMemsetAsync(hist_ws, 0, (size_t)n_img * 256 * sizeof(uint32_t), s);
    if (e != hipSuccess) return e;
    const int bpi = 64;
    hipLaunchKernelGGL(hist256_kernel, dim3(n_img * bpi), dim3(256), 0, s, gray, px, hist_ws, bpi);
    hipLaunchKernelGGL(otsu_decide_kernel, dim3((n_img + 63) / 64), dim3(64), 0, s, hist_ws, n_img, px, (const long long*)nullptr, inverted, threshold);
    hipLaunchKernelGGL(invert_kernel, dim3(pg), dim3(256), 0, s, gray, inverted, px, total);
    return hipGetLastError();
}

}  // namespace ecseg
