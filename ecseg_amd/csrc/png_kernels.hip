// The label PNG of `make metaseg` on gfx950: the zlib stream deflate_labels (host_io.cpp) writes for an image of labels, bit for
// bit, from labels that lie on the device.  The stream is a pure function of the labels and of one Huffman code (png_label_code.h),
// every token stays inside one scan line, and the code comes from 68 counts - so the work is two sweeps over the labels with the
// host's code build between them:
//   png_count_kernel    per scan line (one wave each) the runs, their counts into per-wave LDS histograms and from there into the
//                       image's PNG_NCOUNT counters, and the scan line's Adler-32 terms (a, b) from a start of (0, 0)
//   - the host builds the code from the counts (label_png_code), knows every stream's exact size and sends PngDevCode down -
//   png_rowbits_kernel  per scan line its length in bits under that code
//   png_scan_kernel     per image (one workgroup) the exclusive scan of those lengths in 64 bits = every scan line's bit offset;
//                       the scan lines' Adler terms combined (a' = a + a_s, b' = b + n a + b_s mod 65521, n = 1 + 4 W bytes per
//                       scan line); the end-of-block code, the padding and the big-endian Adler-32 behind the last scan line
//   png_emit_kernel     per scan line the bits: the filter byte's code, then per run its colour string, its 256-byte matches in a
//                       loop and its remainder match, at offsets from a wave scan over the runs of each 64-pixel block
// A run is seen by the lane of its LAST pixel: run starts are a wave ballot over the 64-pixel block (pixel 0 of a scan line always
// starts one, the left neighbour is read across block borders), the run's start is the highest start at or below the lane, or the
// start carried over from the blocks before.  So each run has one owner and runs leave in order.
// Bits go out LSB-first with atomicOr on dwords of a zeroed buffer (the stream read as little-endian dwords): a string straddles
// up to three dwords that other runs, other scan lines' waves and the block header share, OR commutes, so the bytes do not depend on
// the order and no wave has to own a dword.  Adler terms are sums of per-run terms that do not depend on the order either:
// a run of k pixels whose first byte is byte p of its n-byte scan line, with byte sum S and U = p1 + 2 p2 + 3 p3, adds
// k S to a and k (n - p) S - 2 k (k - 1) S - k U to b.
#include "common.h"
#include "png_device.h"
#include "png_label_code.h"

namespace ecseg {

namespace {

constexpr int PNG_ROWS = 4;                                  // scan lines (waves) per workgroup

constexpr uint32_t pal_s(int c) { return LABEL_PNG_PALETTE[c][0] + LABEL_PNG_PALETTE[c][1] + LABEL_PNG_PALETTE[c][2] + LABEL_PNG_PALETTE[c][3]; }
constexpr uint32_t pal_u(int c) { return LABEL_PNG_PALETTE[c][1] + 2 * LABEL_PNG_PALETTE[c][2] + 3 * LABEL_PNG_PALETTE[c][3]; }
__device__ __forceinline__ uint32_t pick4(uint32_t c, uint32_t v0, uint32_t v1, uint32_t v2, uint32_t v3) {
    return c == 0 ? v0 : c == 1 ? v1 : c == 2 ? v2 : v3;
}

struct RunEnd { bool end; uint32_t c, k, xs; };              // is the lane's pixel the last of a run; its colour, length and first pixel

// the 64 pixels from x0 of a scan line of W pixels; carry: the last run start before x0, then the last one before x0 + 64
__device__ __forceinline__ RunEnd run_end(const uint8_t* __restrict__ row, uint32_t W, uint32_t x0, int lane, uint32_t& carry) {
    const uint32_t x = x0 + (uint32_t)lane;
    const bool in = x < W;
    const uint32_t cur = in ? min((uint32_t)row[x], 3u) : 255u;
    uint32_t left = __shfl_up(cur, 1), right = __shfl_down(cur, 1);
    if (lane == 0) left = x0 > 0 ? min((uint32_t)row[x0 - 1], 3u) : 255u;
    if (lane == 63) right = x + 1 < W ? min((uint32_t)row[x + 1], 3u) : 255u;
    const unsigned long long starts = __ballot(in && cur != left);
    const unsigned long long below = starts & (~0ull >> (63 - lane));
    RunEnd r;
    r.end = in && cur != right;                              // (the pixel behind the scan line reads as 255: its last pixel ends a run)
    r.c = cur;
    r.xs = below ? x0 + 63u - (uint32_t)__clzll((long long)below) : carry;
    r.k = x - r.xs + 1;
    if (starts) carry = x0 + 63u - (uint32_t)__clzll((long long)starts);
    return r;
}

__global__ __launch_bounds__(64 * PNG_ROWS) void png_count_kernel(const uint8_t* __restrict__ labels, size_t img_stride, int H, uint32_t W,
                                                                  uint32_t* __restrict__ counts, uint32_t* __restrict__ row_a,
                                                                  uint32_t* __restrict__ row_b) {
    __shared__ uint32_t hist[PNG_ROWS][PNG_NCOUNT];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const size_t img = blockIdx.y;
    for (int k = threadIdx.x; k < PNG_ROWS * PNG_NCOUNT; k += 64 * PNG_ROWS) (&hist[0][0])[k] = 0;
    __syncthreads();
    const int y = (int)blockIdx.x * PNG_ROWS + wave;
    if (y < H) {
        const uint8_t* __restrict__ row = labels + img * img_stride + (size_t)y * W;
        uint32_t* __restrict__ hw = hist[wave];
        const unsigned long long n = 1ull + 4ull * W;
        unsigned long long sa = 0, sb = 0;                   // (each term is below 65521: no overflow in any scan line)
        uint32_t carry = 0, nc0 = 0, nc1 = 0, nc2 = 0, nc3 = 0;
        for (uint32_t x0 = 0; x0 < W; x0 += 64) {
            const RunEnd r = run_end(row, W, x0, lane, carry);
            nc0 += (uint32_t)__popcll(__ballot(r.end && r.c == 0)); nc1 += (uint32_t)__popcll(__ballot(r.end && r.c == 1));
            nc2 += (uint32_t)__popcll(__ballot(r.end && r.c == 2)); nc3 += (uint32_t)__popcll(__ballot(r.end && r.c == 3));
            const uint32_t whole = (r.k - 1) >> 6, rem = (r.k - 1) & 63u;
            // the remainders, one distinct value per turn (speckle: a handful of values per block; an atomic per run would serialise)
            unsigned long long todo = __ballot(r.end);
            while (todo) {
                const uint32_t v = __shfl(rem, __ffsll((long long)todo) - 1);
                const unsigned long long same = __ballot(r.end && rem == v) & todo;
                if (lane == 0) hw[4 + v] += (uint32_t)__popcll(same);
                todo &= ~same;
            }
            if (r.end && whole) atomicAdd(&hw[4 + 64], whole);    // (at most one run per block is longer than the block)
            if (r.end) {
                const unsigned long long S = pick4(r.c, pal_s(0), pal_s(1), pal_s(2), pal_s(3)), U = pick4(r.c, pal_u(0), pal_u(1), pal_u(2), pal_u(3));
                const unsigned long long km = r.k % ADLER_M, d = (n - (1ull + 4ull * r.xs)) % ADLER_M;
                const unsigned long long up = km * d % ADLER_M * S % ADLER_M;
                const unsigned long long down = (2ull * km * ((r.k - 1) % ADLER_M) % ADLER_M * S + km * U) % ADLER_M;
                sa += km * S % ADLER_M;
                sb += (up + ADLER_M - down) % ADLER_M;
            }
        }
        sa = wave_sum(sa); sb = wave_sum(sb);
        if (lane == 0) {
            hw[0] += nc0; hw[1] += nc1; hw[2] += nc2; hw[3] += nc3;
            row_a[img * H + y] = (uint32_t)(sa % ADLER_M);
            row_b[img * H + y] = (uint32_t)(sb % ADLER_M);
        }
    }
    __syncthreads();
    for (int k = threadIdx.x; k < PNG_NCOUNT; k += 64 * PNG_ROWS) {
        uint32_t v = 0;
        for (int w = 0; w < PNG_ROWS; ++w) v += hist[w][k];
        if (v) atomicAdd(&counts[img * PNG_NCOUNT + k], v);
    }
}

__device__ __forceinline__ void load_code(PngDevCode* dst, const PngDevCode* __restrict__ src) {
    const uint32_t* s = reinterpret_cast<const uint32_t*>(src);
    uint32_t* d = reinterpret_cast<uint32_t*>(dst);
    for (int k = threadIdx.x; k < (int)(sizeof(PngDevCode) / 4); k += 64 * PNG_ROWS) d[k] = s[k];
}

// bits of a run that is not the filter byte: its colour string, its 256-byte matches, its remainder match (below 2^30 for W < 2^30)
__device__ __forceinline__ uint32_t run_bits(const PngDevCode& code, const RunEnd& r) {
    return code.cn[r.c] + ((r.k - 1) >> 6) * code.mn[64] + code.mn[(r.k - 1) & 63u];
}

__global__ __launch_bounds__(64 * PNG_ROWS) void png_rowbits_kernel(const uint8_t* __restrict__ labels, size_t img_stride, int H, uint32_t W,
                                                                    const PngDevCode* __restrict__ codes,
                                                                    unsigned long long* __restrict__ row_bits) {
    __shared__ PngDevCode code;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const size_t img = blockIdx.y;
    load_code(&code, codes + img);
    __syncthreads();
    const int y = (int)blockIdx.x * PNG_ROWS + wave;
    if (y >= H) return;
    const uint8_t* __restrict__ row = labels + img * img_stride + (size_t)y * W;
    unsigned long long bits = 0;
    uint32_t carry = 0;
    for (uint32_t x0 = 0; x0 < W; x0 += 64) {
        const RunEnd r = run_end(row, W, x0, lane, carry);
        if (r.end) bits += run_bits(code, r);
    }
    bits = wave_sum(bits);
    if (lane == 0) row_bits[img * H + y] = bits + code.filt_n;
}

__global__ __launch_bounds__(256) void png_scan_kernel(const unsigned long long* __restrict__ row_bits, const uint32_t* __restrict__ row_a,
                                                       const uint32_t* __restrict__ row_b, int H, uint32_t W,
                                                       const PngDevCode* __restrict__ codes, unsigned long long* __restrict__ row_off,
                                                       uint32_t* __restrict__ z, unsigned long long* __restrict__ z_bytes) {
    __shared__ unsigned long long sh[256], sa[256];
    const int t = threadIdx.x;
    const size_t img = blockIdx.y;
    row_bits += img * H; row_a += img * H; row_b += img * H; row_off += img * H;
    const PngDevCode& code = codes[img];
    const unsigned long long n = (1ull + 4ull * W) % ADLER_M;
    unsigned long long carry = code.head_bits, carry_a = 1, bsum = 0;
    for (int base = 0; base < H; base += 256) {
        const int i = base + t;
        const unsigned long long v = i < H ? row_bits[i] : 0ull, va = i < H ? (unsigned long long)row_a[i] : 0ull;
        sh[t] = v; sa[t] = va;
        __syncthreads();
        for (int d = 1; d < 256; d <<= 1) {
            const unsigned long long p = t >= d ? sh[t - d] : 0ull, pa = t >= d ? sa[t - d] : 0ull;
            __syncthreads();
            sh[t] += p; sa[t] += pa;
            __syncthreads();
        }
        if (i < H) {
            row_off[i] = carry + sh[t] - v;
            const unsigned long long a_before = (carry_a + sa[t] - va) % ADLER_M;      // a in front of scan line i
            bsum += (n * a_before + row_b[i]) % ADLER_M;
        }
        carry += sh[255];
        carry_a = (carry_a + sa[255]) % ADLER_M;
        __syncthreads();
    }
    sh[t] = bsum;                                            // (H / 256 terms below 65521 each)
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
        z_bytes[img] = nb + 4;
    }
}

__global__ __launch_bounds__(64 * PNG_ROWS) void png_emit_kernel(const uint8_t* __restrict__ labels, size_t img_stride, int H, uint32_t W,
                                                                 const PngDevCode* __restrict__ codes,
                                                                 const unsigned long long* __restrict__ row_off, uint32_t* __restrict__ z) {
    __shared__ PngDevCode code;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const size_t img = blockIdx.y;
    load_code(&code, codes + img);
    __syncthreads();
    uint32_t* __restrict__ zi = z + code.z_off;
    const uint32_t words = code.z_words;
    if (blockIdx.x == 0 && threadIdx.x < 64 && threadIdx.x * 32u < code.head_bits) put_bits(zi, words, threadIdx.x * 32ull, code.head[threadIdx.x], 32);
    const int y = (int)blockIdx.x * PNG_ROWS + wave;
    if (y >= H) return;
    const uint8_t* __restrict__ row = labels + img * img_stride + (size_t)y * W;
    unsigned long long pos = row_off[img * H + y];
    if (lane == 0) put_bits(zi, words, pos, code.filt, code.filt_n);
    pos += code.filt_n;
    uint32_t carry = 0;
    for (uint32_t x0 = 0; x0 < W; x0 += 64) {
        const RunEnd r = run_end(row, W, x0, lane, carry);
        const uint32_t mine = r.end ? run_bits(code, r) : 0u;
        uint32_t incl = mine;                                // the runs that end in one block: one of up to 2^30 bits, the others short
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const uint32_t o = __shfl_up(incl, d);
            if (lane >= d) incl += o;
        }
        if (r.end) {
            unsigned long long p = pos + (incl - mine);
            put_bits(zi, words, p, code.cbits[r.c], code.cn[r.c]);
            p += code.cn[r.c];
            const uint32_t whole = (r.k - 1) >> 6, rem = (r.k - 1) & 63u, m64 = code.mbits[64], n64 = code.mn[64];
            for (uint32_t i = 0; i < whole; ++i, p += n64) put_bits(zi, words, p, m64, n64);
            put_bits(zi, words, p, code.mbits[rem], code.mn[rem]);
        }
        pos += __shfl(incl, 63);
    }
}

}  // namespace

hipError_t run_png_count(const uint8_t* labels, size_t img_stride, int n, int H, int W, const PngEncodeBufs& b, hipStream_t s) {
    hipError_t e = hipMemsetAsync(b.counts, 0, (size_t)n * PNG_NCOUNT * sizeof(uint32_t), s);
    if (e != hipSuccess) return e;
    const dim3 g((unsigned)((H + PNG_ROWS - 1) / PNG_ROWS), (unsigned)n);
    hipLaunchKernelGGL(png_count_kernel, g, dim3(64 * PNG_ROWS), 0, s, labels, img_stride, H, (uint32_t)W, b.counts, b.row_a, b.row_b);
    return hipGetLastError();
}

hipError_t run_png_emit(const uint8_t* labels, size_t img_stride, int n, int H, int W, const PngEncodeBufs& b, uint32_t* z, size_t z_bytes,
                        hipStream_t s) {
    hipError_t e = hipMemsetAsync(z, 0, z_bytes, s);
    if (e != hipSuccess) return e;
    const dim3 g((unsigned)((H + PNG_ROWS - 1) / PNG_ROWS), (unsigned)n);
    hipLaunchKernelGGL(png_rowbits_kernel, g, dim3(64 * PNG_ROWS), 0, s, labels, img_stride, H, (uint32_t)W, b.codes, b.row_bits);
    hipLaunchKernelGGL(png_scan_kernel, dim3(1, (unsigned)n), dim3(256), 0, s, b.row_bits, b.row_a, b.row_b, H, (uint32_t)W, b.codes, b.row_off, z,
                       b.z_bytes);
    hipLaunchKernelGGL(png_emit_kernel, g, dim3(64 * PNG_ROWS), 0, s, labels, img_stride, H, (uint32_t)W, b.codes, b.row_off, z);
    return hipGetLastError();
}

}  // namespace ecseg
