// The inputs of the two interSeg classifiers, written from the crops where run_nucleus_crops left them (ecseg_classify_nucleus_crops,
// drivers_interseg.hip; src/interseg.py:155,160-168 and src/utils.py:166-173).  Compiled with -ffp-contract=off: the arithmetic of
// iseg_classify.h rounds operation by operation.
#include "common.h"
#include "iseg_classify.h"

namespace ecseg {

namespace {

constexpr int ISEG_IN_BLOCKS = 256 * 256 / 4 / 256;      // blocks per crop: a thread takes 4 consecutive pixels (12 bytes)

__device__ __forceinline__ void iseg_load12(const uint8_t* __restrict__ crops, int crop, int t, uint32_t w[3]) {
    const uint32_t* p = reinterpret_cast<const uint32_t*>(crops + (size_t)crop * (256 * 256 * 3)) + (size_t)t * 3;
    w[0] = p[0]; w[1] = p[1]; w[2] = p[2];
}
__device__ __forceinline__ uint32_t iseg_byte(const uint32_t w[3], int b) { return (w[b >> 2] >> ((b & 3) * 8)) & 255u; }

// blockIdx.y = slot: crop sel_i[slot] goes to slot `slot` of out_i (slot < n_i), crop sel_c[slot] to slot `slot` of out_c (slot < n_c);
// blockIdx.x, threadIdx.x: the 4 pixels.  out_i (n_i, 256, 256, 1), out_c (n_c, 256, 256, 3) float32, 16-byte aligned.
__global__ __launch_bounds__(256) void iseg_classifier_inputs_kernel(const uint8_t* __restrict__ crops, const int32_t* __restrict__ chmax,
                                                                     const int32_t* __restrict__ sel_i, int n_i,
                                                                     const int32_t* __restrict__ sel_c, int n_c,
                                                                     float* __restrict__ out_i, float* __restrict__ out_c) {
    const int slot = blockIdx.y;
    const int t = blockIdx.x * 256 + threadIdx.x;            // < 16384
    const int ci = slot < n_i ? sel_i[slot] : -1, cc = slot < n_c ? sel_c[slot] : -1;     // block-uniform
    uint32_t w[3];
    if (ci >= 0) {
        iseg_load12(crops, ci, t, w);
        float4 v;
        v.x = (float)iseg_byte(w, 0); v.y = (float)iseg_byte(w, 3); v.z = (float)iseg_byte(w, 6); v.w = (float)iseg_byte(w, 9);
        reinterpret_cast<float4*>(out_i + (size_t)slot * (256 * 256))[t] = v;
    }
    if (cc >= 0) {
        if (cc != ci) iseg_load12(crops, cc, t, w);
        const int32_t* m = chmax + (size_t)cc * 3;
        const float n0 = iseg_c_norm(m[0]), n1 = iseg_c_norm(m[1]), n2 = iseg_c_norm(m[2]);   // uniform: read once per block
        const float nr[3] = {n0, n1, n2};
        float v[12];
#pragma unroll
        for (int b = 0; b < 12; ++b) v[b] = iseg_c_quant(iseg_byte(w, b), nr[b % 3]);
        float4* o = reinterpret_cast<float4*>(out_c + (size_t)slot * (256 * 256 * 3)) + (size_t)t * 3;
        o[0] = make_float4(v[0], v[1], v[2], v[3]);
        o[1] = make_float4(v[4], v[5], v[6], v[7]);
        o[2] = make_float4(v[8], v[9], v[10], v[11]);
    }
}

}  // namespace

hipError_t run_iseg_classifier_inputs(const uint8_t* crops, const int32_t* chmax, const int32_t* sel_i, int n_i, const int32_t* sel_c,
                                      int n_c, float* out_i, float* out_c, hipStream_t s) {
    const int slots = n_i > n_c ? n_i : n_c;
    if (slots <= 0) return hipSuccess;
    hipLaunchKernelGGL(iseg_classifier_inputs_kernel, dim3(ISEG_IN_BLOCKS, (unsigned)slots), dim3(256), 0, s, crops, chmax, sel_i, n_i, sel_c,
                       n_c, out_i, out_c);
    return hipGetLastError();
}

}  // namespace ecseg
