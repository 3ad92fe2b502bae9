// Host and device: the per-block pieces of the gray-channel PNG coder (deflate_gray_sub, host_io.cpp; png_gray_kernels.hip), so that
// the device owns tokens without walking runs serially and a host program can hold the same text to rle_scan (png_gray_code.h).
// The filtered stream of an H x W channel is n = H (W + 1) bytes, byte 0 of every scan line the filter byte 1, and its tokens are a
// pure function of its MAXIMAL RUNS, which cross scan lines.  A run of R equal bytes b is
//   R < 4:   R literals b
//   R >= 4:  one literal b, then distance-1 matches over r = R - 1 bytes: r <= 258: one of r; r = 258 k + t, k >= 1: t = 0: k of 258;
//            t >= 3: k of 258 and one of t; t = 1, 2: k - 1 of 258, one of 255 + t, one of 3 (never a tail shorter than a match)
// and the run belongs to the position of its LAST byte: runs leave in stream order, each has one owner.
#pragma once
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define GRAY_HD __host__ __device__ __forceinline__
#else
#define GRAY_HD inline
#endif

namespace ecseg {

constexpr unsigned long long ADLER_M = 65521;             // Adler-32's modulus: the one definition, for both PNG coders and the host

// byte i of the filtered stream: px the channel's first sample, samples C apart, scan lines row_stride apart; flip: 0xff to invert
GRAY_HD uint32_t gray_stream_byte(const uint8_t* px, uint32_t W, uint32_t C, size_t row_stride, uint32_t flip, uint32_t i) {
    const uint32_t line = W + 1, y = i / line, xx = i - y * line;
    if (xx == 0) return 1u;                                   // filter type SUB
    const uint8_t* p = px + (size_t)y * row_stride + (size_t)(xx - 1) * C;
    const uint32_t v = p[0] ^ flip, left = xx > 1 ? (uint32_t)(*(p - C)) ^ flip : 0u;
    return (v - left) & 255u;
}

// Run starts over the 64 positions from i0 are a bit mask (position 0 of the stream always starts one; a wave ballot on the device).
// The run that holds position i0 + lane starts at the highest start at or below the lane, else at `carry`, the last start before i0.
GRAY_HD uint32_t gray_run_start(unsigned long long starts, int lane, uint32_t i0, uint32_t carry) {
    const unsigned long long below = starts & (~0ull >> (63 - lane));
    return below ? i0 + 63u - (uint32_t)__builtin_clzll(below) : carry;
}
GRAY_HD uint32_t gray_carry_out(unsigned long long starts, uint32_t i0, uint32_t carry) {
    return starts ? i0 + 63u - (uint32_t)__builtin_clzll(starts) : carry;
}

// The tokens of a run of R bytes: `lits` literals, then n258 matches of 258, then a match of m1 and one of m2 (0: none).
struct GrayTokens { uint32_t lits, n258, m1, m2; };
GRAY_HD GrayTokens gray_run_tokens(uint32_t R) {
    if (R < 4) return GrayTokens{R, 0u, 0u, 0u};
    const uint32_t r = R - 1, k = r / 258u, t = r - k * 258u;
    if (k == 0) return GrayTokens{1u, 0u, r, 0u};
    if (t == 0) return GrayTokens{1u, k, 0u, 0u};
    if (t >= 3) return GrayTokens{1u, k, t, 0u};
    return GrayTokens{1u, k - 1, 255u + t, 3u};
}

// deflate's symbol of a match length 3..258 (length_code, png_label_code.h, without its table)
GRAY_HD uint32_t gray_len_sym(uint32_t L) {
    if (L == 258) return 285u;
    const uint32_t d = L - 3;
    if (d < 8) return 257u + d;
    const uint32_t e = 29u - (uint32_t)__builtin_clz(d);       // extra bits: floor(log2 d) - 2
    return 257u + 4u + 4u * e + ((d >> e) & 3u);
}

// Bits of those tokens: lit_n the literal's code length, mn(L) the bits of a match of L (length code, extra bits, distance code).
template <typename MatchBits>
GRAY_HD uint32_t gray_run_bits(const GrayTokens& t, uint32_t lit_n, MatchBits&& mn) {
    return t.lits * lit_n + (t.n258 ? t.n258 * mn(258u) : 0u) + (t.m1 ? mn(t.m1) : 0u) + (t.m2 ? mn(t.m2) : 0u);
}

// Adler-32 terms of a piece of `len` bytes from a start of (0, 0) are a = sum f, b = sum (len - offset) f; a piece behind a prefix
// whose terms are (a0, b0) continues them as below.  The stream starts from (1, 0).
struct GrayAdler { uint32_t a, b; };
// what a piece adds to b behind a prefix whose a is a_before (the terms of the pieces sum, so a workgroup adds them in any order)
GRAY_HD uint32_t gray_adler_b_step(unsigned long long a_before, uint32_t piece_b, unsigned long long len) {
    return (uint32_t)((len % ADLER_M * (a_before % ADLER_M) + piece_b) % ADLER_M);
}
GRAY_HD GrayAdler gray_adler_append(GrayAdler head, GrayAdler piece, unsigned long long len) {
    return GrayAdler{(uint32_t)((head.a + (unsigned long long)piece.a) % ADLER_M), (uint32_t)((head.b + gray_adler_b_step(head.a, piece.b, len)) % ADLER_M)};
}

}  // namespace ecseg
