// Device-only: what the two PNG coders' kernels (png_kernels.hip, png_gray_kernels.hip) share.
#pragma once
#include "common.h"
#include "png_gray_tokens.h"                              // ADLER_M

namespace ecseg {

__device__ __forceinline__ unsigned long long wave_sum(unsigned long long v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d);
    return v;
}

// ORs the low n (<= 64) bits of `bits` into the stream at bit `pos`; dwords at or behind `words` are left alone
__device__ __forceinline__ void put_bits(uint32_t* __restrict__ z, uint32_t words, unsigned long long pos, unsigned long long bits, uint32_t n) {
    if (n == 0) return;
    const unsigned long long w = pos >> 5;
    const uint32_t sh = (uint32_t)pos & 31u;
    const unsigned long long lo = bits << sh;
    const uint32_t hi = sh ? (uint32_t)(bits >> (64 - sh)) : 0u;
    if ((uint32_t)lo && w < words) atomicOr(z + w, (uint32_t)lo);
    if ((uint32_t)(lo >> 32) && w + 1 < words) atomicOr(z + w + 1, (uint32_t)(lo >> 32));
    if (hi && w + 2 < words) atomicOr(z + w + 2, hi);
}

}  // namespace ecseg
