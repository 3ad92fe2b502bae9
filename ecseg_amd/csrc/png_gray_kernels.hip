// The red / green PNGs of `make meta_overlay` on gfx950: the zlib stream deflate_gray_sub (host_io.cpp) writes for one channel of an
// interleaved 8-bit image, bit for bit, from pixels that lie on the device.  A PLANE is one (image, channel) pair.  The stream is a
// pure function of the maximal runs of the plane's filtered bytes (png_gray_tokens.h: n = H (W + 1) bytes, SUB filter computed on the
// fly, the filter byte 1 in front of every scan line, runs cross scan lines) and of one Huffman code built from 286 counts
// (png_gray_code.h).  The kernels walk the FLAT stream, a wave per span of PGRAY_SPAN bytes, 64 bytes per step:
//   pgray_count_kernel  per span the start of the run that reaches into it (found by walking back 64 bytes at a time, kept for the
//                       sweeps below), the symbol counts of the runs that END in it into per-wave LDS histograms and from there into
//                       the plane's PGRAY_NCOUNT counters, and the span's Adler-32 terms (a, b) from a start of (0, 0)
//   - the host builds every plane's code, knows every stream's exact size, decides which files fit and sends GrayDevCode down -
//   pgray_bits_kernel   per span the bits of the runs that end in it
//   pgray_scan_kernel   per plane (one workgroup) the exclusive scan of those in 64 bits behind the header = every span's bit offset;
//                       the spans' Adler terms appended in order (gray_adler_append); the end-of-block code, the padding and the
//                       big-endian Adler-32 behind the last span
//   pgray_emit_kernel   per span the bits, at offsets from a wave scan over the runs of each 64-byte step
// OWNERSHIP: a run belongs to the lane of its LAST byte, in the span where it ends.  Run starts are a wave ballot over the step (the
// left neighbour is read across step, span and scan-line borders), the run's start is the highest start at or below the lane or the
// one carried over, so a run far longer than a span - a ramp image is ONE run of n bytes - still has one owner, which writes its
// matches of 258 in a loop and the tail by the closed form.  Runs leave in stream order, so the offsets are a plain prefix sum.
// COST OF THE WALK BACK: start_before reads 64 bytes per turn until it meets a run start, so a span costs one turn wherever runs are
// short (every measured image) and a walk to the run's start where one run covers many spans.  A stream that is ONE run - the ramp -
// makes every span walk to position 0: n^2 / (2 * 64 * PGRAY_SPAN) turns in all, 16 M for a 1040 x 1392 plane.  That is slow, not
// wrong; a pass that hands the carries from span to span would make it linear and is not built.
// Bits go out LSB-first with atomicOr on dwords of a zeroed buffer (put_bits, png_device.h): OR commutes, the bytes do not depend on
// the order.  A plane whose file does not fit its capacity has z_words == 0 and is not written at all.
#include "common.h"
#include "png_device.h"
#include "png_gray_tokens.h"

namespace ecseg {

namespace {

constexpr int PGRAY_WAVES = 4;                               // spans (waves) per workgroup

struct GrayPlane { const uint8_t* px; size_t row_stride; uint32_t W, C, flip, n; };

__device__ __forceinline__ GrayPlane plane_of(const GraySource& src, uint32_t plane) {
    const uint32_t img = plane / src.n_ch, ch = (src.chans >> (8 * (plane - img * src.n_ch))) & 255u;
    GrayPlane P;
    P.px = src.px + (size_t)img * src.img_stride + ch;
    P.row_stride = (size_t)src.W * src.C; P.W = src.W; P.C = src.C; P.flip = src.invert ? 255u : 0u; P.n = src.n;
    return P;
}
__device__ __forceinline__ uint32_t byte_at(const GrayPlane& P, uint32_t i) { return gray_stream_byte(P.px, P.W, P.C, P.row_stride, P.flip, i); }

// the last run start before position g > 0 (the start of the run that holds g - 1): 64 positions per turn, backwards
__device__ __forceinline__ uint32_t start_before(const GrayPlane& P, uint32_t g, int lane) {
    for (uint32_t hi = g;;) {                                // positions hi - 64 .. hi - 1, those below 0 left out
        const uint32_t i0 = hi >= 64 ? hi - 64 : 0u, i = i0 + (uint32_t)lane;
        const bool in = i < hi;
        const uint32_t cur = in ? byte_at(P, i) : 256u;
        uint32_t left = __shfl_up(cur, 1);
        if (lane == 0) left = i0 > 0 ? byte_at(P, i0 - 1) : 256u;
        const unsigned long long starts = __ballot(in && cur != left);
        if (starts) return gray_carry_out(starts, i0, 0u);
        hi = i0;                                             // (position 0 starts a run: the walk ends there at the latest)
    }
}

struct RunEnd { bool end; uint32_t b, R; };                  // is the lane's byte the last of a run; the byte and the run's length

// the 64 positions from i0; carry: the last run start before i0, then the last one before i0 + 64
__device__ __forceinline__ RunEnd run_end(const GrayPlane& P, uint32_t i0, int lane, uint32_t& carry, uint32_t* cur_out = nullptr) {
    const uint32_t i = i0 + (uint32_t)lane;
    const bool in = i < P.n;
    const uint32_t cur = in ? byte_at(P, i) : 256u;
    uint32_t left = __shfl_up(cur, 1), right = __shfl_down(cur, 1);
    if (lane == 0) left = i0 > 0 ? byte_at(P, i0 - 1) : 256u;
    if (lane == 63) right = in && i + 1 < P.n ? byte_at(P, i + 1) : 256u;
    const unsigned long long starts = __ballot(in && cur != left);
    RunEnd r;
    r.end = in && cur != right;                              // (positions behind the stream read as 256: its last byte ends a run)
    r.b = cur;
    r.R = i - gray_run_start(starts, lane, i0, carry) + 1;
    carry = gray_carry_out(starts, i0, carry);
    if (cur_out) *cur_out = in ? cur : 0u;
    return r;
}

__global__ __launch_bounds__(64 * PGRAY_WAVES) void pgray_count_kernel(GraySource src, uint32_t n_spans, uint32_t* __restrict__ counts,
                                                                       uint32_t* __restrict__ span_carry, uint32_t* __restrict__ span_a,
                                                                       uint32_t* __restrict__ span_b) {
    __shared__ uint32_t hist[PGRAY_WAVES][PGRAY_NCOUNT + 1];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint32_t plane = blockIdx.y;
    for (int k = threadIdx.x; k < PGRAY_WAVES * (PGRAY_NCOUNT + 1); k += 64 * PGRAY_WAVES) (&hist[0][0])[k] = 0;
    __syncthreads();
    const uint32_t span = blockIdx.x * PGRAY_WAVES + (uint32_t)wave;
    if (span < n_spans) {
        const GrayPlane P = plane_of(src, plane);
        uint32_t* __restrict__ hw = hist[wave];
        const uint32_t g = span * PGRAY_SPAN, len = min(PGRAY_SPAN, P.n - g);
        uint32_t carry = g > 0 ? start_before(P, g, lane) : 0u;
        if (lane == 0) span_carry[(size_t)plane * n_spans + span] = carry;
        unsigned long long sa = 0, sb = 0;                   // (a lane adds PGRAY_SPAN / 64 terms below 2^18 each)
        for (uint32_t i0 = g; i0 < g + len; i0 += 64) {
            uint32_t cur;
            const RunEnd r = run_end(P, i0, lane, carry, &cur);
            sa += cur;
            sb += (unsigned long long)(g + len - (i0 + (uint32_t)lane)) * cur;     // (cur is 0 behind the stream)
            if (r.end) {
                const GrayTokens t = gray_run_tokens(r.R);
                atomicAdd(&hw[r.b], t.lits);
                if (t.n258) atomicAdd(&hw[285], t.n258);
                if (t.m1) atomicAdd(&hw[gray_len_sym(t.m1)], 1u);
                if (t.m2) atomicAdd(&hw[gray_len_sym(t.m2)], 1u);
                if (t.n258 | t.m1) atomicAdd(&hw[286], 1u);  // any_match
            }
        }
        sa = wave_sum(sa); sb = wave_sum(sb);
        if (lane == 0) {
            span_a[(size_t)plane * n_spans + span] = (uint32_t)(sa % ADLER_M);
            span_b[(size_t)plane * n_spans + span] = (uint32_t)(sb % ADLER_M);
        }
    }
    __syncthreads();
    for (int k = threadIdx.x; k < PGRAY_NCOUNT; k += 64 * PGRAY_WAVES) {
        uint32_t v = 0;
        for (int w = 0; w < PGRAY_WAVES; ++w) v += hist[w][k];
        if (v) atomicAdd(&counts[(size_t)plane * PGRAY_NCOUNT + k], v);
    }
}

__device__ __forceinline__ void load_code(GrayDevCode* dst, const GrayDevCode* __restrict__ src) {
    const uint32_t* s = reinterpret_cast<const uint32_t*>(src);
    uint32_t* d = reinterpret_cast<uint32_t*>(dst);
    for (int k = threadIdx.x; k < (int)(sizeof(GrayDevCode) / 4); k += 64 * PGRAY_WAVES) d[k] = s[k];
}

// bits of a run (below 2^28 for n < 2^31: 21 bits per 258 bytes)
__device__ __forceinline__ uint32_t run_bits(const GrayDevCode& code, const RunEnd& r, const GrayTokens& t) {
    return gray_run_bits(t, code.lit[r.b] >> 16, [&](uint32_t L) { return code.match[L] >> 24; });
}

__global__ __launch_bounds__(64 * PGRAY_WAVES) void pgray_bits_kernel(GraySource src, uint32_t n_spans, const GrayDevCode* __restrict__ codes,
                                                                      const uint32_t* __restrict__ span_carry,
                                                                      unsigned long long* __restrict__ span_bits) {
    __shared__ GrayDevCode code;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint32_t plane = blockIdx.y;
    load_code(&code, codes + plane);
    __syncthreads();
    const uint32_t span = blockIdx.x * PGRAY_WAVES + (uint32_t)wave;
    if (span >= n_spans || code.z_words == 0) return;
    const GrayPlane P = plane_of(src, plane);
    const uint32_t g = span * PGRAY_SPAN, len = min(PGRAY_SPAN, P.n - g);
    uint32_t carry = span_carry[(size_t)plane * n_spans + span];
    unsigned long long bits = 0;
    for (uint32_t i0 = g; i0 < g + len; i0 += 64) {
        const RunEnd r = run_end(P, i0, lane, carry);
        if (r.end) bits += run_bits(code, r, gray_run_tokens(r.R));
    }
    bits = wave_sum(bits);
    if (lane == 0) span_bits[(size_t)plane * n_spans + span] = bits;
}

__global__ __launch_bounds__(256) void pgray_scan_kernel(const unsigned long long* __restrict__ span_bits, const uint32_t* __restrict__ span_a,
                                                         const uint32_t* __restrict__ span_b, uint32_t n_spans, uint32_t n,
                                                         const GrayDevCode* __restrict__ codes, unsigned long long* __restrict__ span_off,
                                                         uint32_t* __restrict__ z, unsigned long long* __restrict__ z_bytes) {
    __shared__ unsigned long long sh[256], sa[256];
    const int t = threadIdx.x;
    const size_t plane = blockIdx.y;
    const GrayDevCode& code = codes[plane];
    if (code.z_words == 0) { if (t == 0) z_bytes[plane] = 0; return; }      // (the whole workgroup leaves)
    span_bits += plane * n_spans; span_a += plane * n_spans; span_b += plane * n_spans; span_off += plane * n_spans;
    unsigned long long carry = code.head_bits, carry_a = 1, bsum = 0;
    for (uint32_t base = 0; base < n_spans; base += 256) {
        const uint32_t i = base + (uint32_t)t;
        const unsigned long long v = i < n_spans ? span_bits[i] : 0ull, va = i < n_spans ? (unsigned long long)span_a[i] : 0ull;
        sh[t] = v; sa[t] = va;
        __syncthreads();
        for (int d = 1; d < 256; d <<= 1) {
            const unsigned long long p = t >= d ? sh[t - d] : 0ull, pa = t >= d ? sa[t - d] : 0ull;
            __syncthreads();
            sh[t] += p; sa[t] += pa;
            __syncthreads();
        }
        if (i < n_spans) {
            span_off[i] = carry + sh[t] - v;
            const unsigned long long a_before = (carry_a + sa[t] - va) % ADLER_M;      // a in front of span i
            const unsigned long long len = min(PGRAY_SPAN, n - i * PGRAY_SPAN);
            bsum += gray_adler_b_step(a_before, span_b[i], len);                       // gray_adler_append's b, summed over the spans
        }
        carry += sh[255];
        carry_a = (carry_a + sa[255]) % ADLER_M;
        __syncthreads();
    }
    sh[t] = bsum;                                            // (n_spans / 256 terms below 65521 each)
    __syncthreads();
    for (int d = 128; d >= 1; d >>= 1) {
        if (t < d) sh[t] += sh[t + d];
        __syncthreads();
    }
    if (t == 0) {
        uint32_t* __restrict__ zi = z + code.z_off;
        put_bits(zi, code.z_words, carry, code.eob, code.eob_n);
        const unsigned long long nb = (carry + code.eob_n + 7) >> 3;      // the Adler-32 starts on a byte
        const uint32_t adler = (uint32_t)((sh[0] % ADLER_M) << 16 | carry_a);
        put_bits(zi, code.z_words, nb * 8, __builtin_bswap32(adler), 32);
        z_bytes[plane] = nb + 4;
    }
}

__global__ __launch_bounds__(64 * PGRAY_WAVES) void pgray_emit_kernel(GraySource src, uint32_t n_spans, const GrayDevCode* __restrict__ codes,
                                                                      const uint32_t* __restrict__ span_carry,
                                                                      const unsigned long long* __restrict__ span_off, uint32_t* __restrict__ z) {
    __shared__ GrayDevCode code;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint32_t plane = blockIdx.y;
    load_code(&code, codes + plane);
    __syncthreads();
    const uint32_t words = code.z_words;
    if (words == 0) return;
    uint32_t* __restrict__ zi = z + code.z_off;
    if (blockIdx.x == 0 && threadIdx.x < 64 && threadIdx.x * 32u < code.head_bits) put_bits(zi, words, threadIdx.x * 32ull, code.head[threadIdx.x], 32);
    const uint32_t span = blockIdx.x * PGRAY_WAVES + (uint32_t)wave;
    if (span >= n_spans) return;
    const GrayPlane P = plane_of(src, plane);
    const uint32_t g = span * PGRAY_SPAN, len = min(PGRAY_SPAN, P.n - g);
    uint32_t carry = span_carry[(size_t)plane * n_spans + span];
    unsigned long long pos = span_off[(size_t)plane * n_spans + span];
    for (uint32_t i0 = g; i0 < g + len; i0 += 64) {
        const RunEnd r = run_end(P, i0, lane, carry);
        GrayTokens t{0u, 0u, 0u, 0u};
        if (r.end) t = gray_run_tokens(r.R);
        const uint32_t mine = r.end ? run_bits(code, r, t) : 0u;
        uint32_t incl = mine;                                // the runs that end in one step: one of up to 2^28 bits, the others short
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const uint32_t o = __shfl_up(incl, d);
            if (lane >= d) incl += o;
        }
        if (r.end) {
            unsigned long long p = pos + (incl - mine);
            const uint32_t lc = code.lit[r.b] & 0xffffu, ln = code.lit[r.b] >> 16;
            unsigned long long lits = 0;
            for (uint32_t k = 0; k < t.lits; ++k) lits |= (unsigned long long)lc << (k * ln);      // (at most three of 15 bits)
            put_bits(zi, words, p, lits, t.lits * ln);
            p += t.lits * ln;
            const uint32_t m258 = code.match[258] & 0xffffffu, n258 = code.match[258] >> 24;
            for (uint32_t k = 0; k < t.n258; ++k, p += n258) put_bits(zi, words, p, m258, n258);
            if (t.m1) { put_bits(zi, words, p, code.match[t.m1] & 0xffffffu, code.match[t.m1] >> 24); p += code.match[t.m1] >> 24; }
            if (t.m2) put_bits(zi, words, p, code.match[t.m2] & 0xffffffu, code.match[t.m2] >> 24);
        }
        pos += __shfl(incl, 63);
    }
}

}  // namespace

hipError_t run_pgray_count(const GraySource& src, int n_planes, const GrayEncodeBufs& b, hipStream_t s) {
    hipError_t e = hipMemsetAsync(b.counts, 0, (size_t)n_planes * PGRAY_NCOUNT * sizeof(uint32_t), s);
    if (e != hipSuccess) return e;
    const dim3 g((b.n_spans + PGRAY_WAVES - 1) / PGRAY_WAVES, (unsigned)n_planes);
    hipLaunchKernelGGL(pgray_count_kernel, g, dim3(64 * PGRAY_WAVES), 0, s, src, b.n_spans, b.counts, b.span_carry, b.span_a, b.span_b);
    return hipGetLastError();
}

hipError_t run_pgray_emit(const GraySource& src, int n_planes, const GrayEncodeBufs& b, size_t z_bytes, hipStream_t s) {
    hipError_t e = hipMemsetAsync(b.z, 0, z_bytes, s);
    if (e != hipSuccess) return e;
    const dim3 g((b.n_spans + PGRAY_WAVES - 1) / PGRAY_WAVES, (unsigned)n_planes);
    hipLaunchKernelGGL(pgray_bits_kernel, g, dim3(64 * PGRAY_WAVES), 0, s, src, b.n_spans, b.codes, b.span_carry, b.span_bits);
    hipLaunchKernelGGL(pgray_scan_kernel, dim3(1, (unsigned)n_planes), dim3(256), 0, s, b.span_bits, b.span_a, b.span_b, b.n_spans, src.n, b.codes,
                       b.span_off, b.z, b.z_bytes);
    hipLaunchKernelGGL(pgray_emit_kernel, g, dim3(64 * PGRAY_WAVES), 0, s, src, b.n_spans, b.codes, b.span_carry, b.span_off, b.z);
    return hipGetLastError();
}

}  // namespace ecseg
