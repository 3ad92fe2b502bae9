// The strips of a TIFF file decoded on gfx950: what ecseg_tiff_read (host_io.cpp) does one strip after another on a host thread -
// ecseg_lzw_decode (host_codec.cpp) or a copy, zero fill, byte order, horizontal predictor - from the file image as it was
// uploaded and its strip tables, into the raster.
//
// tiff_lzw_unstrip_kernel: one strip per workgroup of ONE wave; grid dimension x is the strip.  The routine is td_lzw_strip
// (tiff_decode_strip.h, which says how the wave shares the work and why its copies are ordered); the kernel finds the strip's
// bytes in the file, clamps them to the file, and leaves one status word per strip (0, or 1: corrupt stream / offset behind the
// file).  A strip the tables do not have is zero-filled.
// tiff_raw_unstrip_kernel: the same for uncompressed strips: a clamped copy and the zero fill.
// tiff_unpredict_kernel: one wave per row, after all strips: 16-bit samples of a big-endian file are swapped to native order, then
// the horizontal predictor is undone per sample channel (stride spp) as an inclusive wave scan over 64 samples with a carry
// into the next 64, modulo 2^8 or 2^16.
#include "common.h"
#include "tiff_decode_strip.h"

namespace ecseg {

namespace {

struct TdStrip { const uint8_t* src; uint8_t* dst; uint32_t have, want; bool in_table, behind_file; };

// The strip of this workgroup: rows [strip * rps, ...) of the raster, bytes [off, off + min(cnt, n - off)) of the file.
__device__ __forceinline__ TdStrip td_strip(const uint8_t* file, unsigned long long n, const uint32_t* offs, const uint32_t* cnts, uint32_t n_table,
                                            uint32_t H, unsigned long long line, uint32_t rps, uint8_t* raster) {
    const uint32_t strip = blockIdx.x;
    const unsigned long long r0 = (unsigned long long)strip * rps;
    TdStrip t{file, raster, 0u, 0u, false, false};
    if (r0 >= H) return t;                                   // (the grid has ceil(H / rps) strips: never)
    const unsigned long long rows = r0 + rps <= H ? rps : H - r0;
    t.want = (uint32_t)(rows * line);                        // (below 2^31: the driver refuses longer strips)
    t.dst = raster + r0 * line;
    if (strip >= n_table) return t;
    t.in_table = true;
    const unsigned long long off = offs[strip], cnt = cnts[strip];
    if (off > n) { t.behind_file = true; return t; }
    t.src = file + off;
    t.have = (uint32_t)(cnt < n - off ? cnt : n - off);
    return t;
}

__global__ __launch_bounds__(64) void tiff_lzw_unstrip_kernel(const uint8_t* __restrict__ file, unsigned long long n, const uint32_t* __restrict__ offs,
                                                              const uint32_t* __restrict__ cnts, uint32_t n_table, uint32_t H, unsigned long long line,
                                                              uint32_t rps, uint8_t* raster, uint32_t* __restrict__ status) {
    __shared__ TdLds L;
    const TdStrip t = td_strip(file, n, offs, cnts, n_table, H, line, rps, raster);
    const uint32_t st = td_lzw_strip(t.src, t.have, t.dst, t.want, L);     // (have == 0: nothing is read, the strip is zeros)
    if (threadIdx.x == 0) status[blockIdx.x] = t.behind_file ? 1u : st;
}

__global__ __launch_bounds__(256) void tiff_raw_unstrip_kernel(const uint8_t* __restrict__ file, unsigned long long n, const uint32_t* __restrict__ offs,
                                                               const uint32_t* __restrict__ cnts, uint32_t n_table, uint32_t H, unsigned long long line,
                                                               uint32_t rps, uint8_t* __restrict__ raster, uint32_t* __restrict__ status) {
    const TdStrip t = td_strip(file, n, offs, cnts, n_table, H, line, rps, raster);
    const uint32_t got = t.have < t.want ? t.have : t.want;
    for (uint32_t k = threadIdx.x; k < t.want; k += 256) t.dst[k] = k < got ? t.src[k] : (uint8_t)0;
    if (threadIdx.x == 0) status[blockIdx.x] = t.behind_file ? 1u : 0u;
}

template <typename T>
__global__ __launch_bounds__(64) void tiff_unpredict_kernel(T* __restrict__ raster, uint32_t W, uint32_t spp, int swap, int predictor) {
    const uint32_t lane = threadIdx.x;
    T* __restrict__ q = raster + (size_t)blockIdx.x * W * spp;
    for (uint32_t c = 0; c < spp; ++c) {
        uint32_t carry = 0;
        for (uint32_t x0 = 0; x0 < W; x0 += 64) {
            const uint32_t x = x0 + lane;
            uint32_t v = 0;
            if (x < W) {
                v = q[(size_t)x * spp + c];
                if (swap) v = ((v << 8) | (v >> 8)) & 0xffffu;
            }
            if (predictor) {
#pragma unroll
                for (int d = 1; d < 64; d <<= 1) {
                    const uint32_t up = __shfl_up(v, d);
                    if (lane >= (uint32_t)d) v += up;
                }
                v += carry;
                carry = __shfl(v, 63);
            }
            if (x < W) q[(size_t)x * spp + c] = (T)v;
        }
    }
}

}  // namespace

hipError_t run_tiff_decode(const TiffDecodeBufs& b, unsigned long long n_bytes, int H, int W, int spp, int bytes_per_sample, int rps, int lzw,
                           int swap, int predictor, hipStream_t s) {
    const unsigned long long line = (unsigned long long)W * spp * bytes_per_sample;
    const dim3 g((unsigned)b.nstrips);
    if (lzw)
        hipLaunchKernelGGL(tiff_lzw_unstrip_kernel, g, dim3(64), 0, s, b.file, n_bytes, b.offs, b.cnts, (uint32_t)b.n_table, (uint32_t)H, line, (uint32_t)rps,
                           b.raster, b.status);
    else
        hipLaunchKernelGGL(tiff_raw_unstrip_kernel, g, dim3(256), 0, s, b.file, n_bytes, b.offs, b.cnts, (uint32_t)b.n_table, (uint32_t)H, line,
                           (uint32_t)rps, b.raster, b.status);
    if (bytes_per_sample == 2 && (swap || predictor))
        hipLaunchKernelGGL(tiff_unpredict_kernel<uint16_t>, dim3((unsigned)H), dim3(64), 0, s, reinterpret_cast<uint16_t*>(b.raster), (uint32_t)W,
                           (uint32_t)spp, swap, predictor);
    else if (bytes_per_sample == 1 && predictor)
        hipLaunchKernelGGL(tiff_unpredict_kernel<uint8_t>, dim3((unsigned)H), dim3(64), 0, s, b.raster, (uint32_t)W, (uint32_t)spp, 0, predictor);
    return hipGetLastError();
}

}  // namespace ecseg
