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
//   tiffb_unstrip_kernel, tiffb_unpredict_kernel, tiffb_status_kernel: the same over a batch of files (ecseg_tiff_decode_batch): grid
// dimension x is the strip or row counted over all files, the file is found in the table (TdFile, tiff_decode_batch.h) by binary
// search of its first-strip / first-row column - the index is the workgroup's, so the search is wave-uniform - and the work is the
// same functions: td_lzw_strip, td_raw_strip (tiff_decode_strip.h) and td_unpredict_row.  One launch serves LZW and uncompressed
// files mixed; the strips of different files share nothing, which is where a batch of files of few strips finds its parallelism.
#include "common.h"
#include "tiff_decode_strip.h"

namespace ecseg {

namespace {

__global__ __launch_bounds__(64) void tiff_lzw_unstrip_kernel(const uint8_t* __restrict__ file, unsigned long long n, const uint32_t* __restrict__ offs,
                                                              const uint32_t* __restrict__ cnts, uint32_t n_table, uint32_t H, unsigned long long line,
                                                              uint32_t rps, uint8_t* raster, uint32_t* __restrict__ status) {
    __shared__ TdLds L;
    const TdStrip t = td_strip(blockIdx.x, file, n, offs, cnts, n_table, H, line, rps, raster);
    const uint32_t st = td_lzw_strip(t.src, t.have, t.dst, t.want, L);     // (have == 0: nothing is read, the strip is zeros)
    if (threadIdx.x == 0) status[blockIdx.x] = t.behind_file ? 1u : st;
}

__global__ __launch_bounds__(256) void tiff_raw_unstrip_kernel(const uint8_t* __restrict__ file, unsigned long long n, const uint32_t* __restrict__ offs,
                                                               const uint32_t* __restrict__ cnts, uint32_t n_table, uint32_t H, unsigned long long line,
                                                               uint32_t rps, uint8_t* __restrict__ raster, uint32_t* __restrict__ status) {
    const TdStrip t = td_strip(blockIdx.x, file, n, offs, cnts, n_table, H, line, rps, raster);
    td_raw_strip(t, 256u);
    if (threadIdx.x == 0) status[blockIdx.x] = t.behind_file ? 1u : 0u;
}

// One row of W pixels of spp samples, by one wave: the swap, then the predictor undone per sample channel.
template <typename T>
__device__ __forceinline__ void td_unpredict_row(T* __restrict__ q, uint32_t W, uint32_t spp, int swap, int predictor) {
    const uint32_t lane = threadIdx.x;
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

template <typename T>
__global__ __launch_bounds__(64) void tiff_unpredict_kernel(T* __restrict__ raster, uint32_t W, uint32_t spp, int swap, int predictor) {
    td_unpredict_row(raster + (size_t)blockIdx.x * W * spp, W, spp, swap, predictor);
}

// ---- the same over a batch of files: the pointers come from the table (tiff_decode_batch.h), the work is the functions above ------
__global__ __launch_bounds__(64) void tiffb_unstrip_kernel(const TdFile* __restrict__ tab, uint32_t n_files, const uint8_t* __restrict__ files,
                                                           const uint32_t* __restrict__ tables, uint8_t* rasters, uint32_t* __restrict__ status) {
    __shared__ TdLds L;
    const uint32_t st = tdb_unstrip(tab, n_files, files, tables, rasters, blockIdx.x, L);
    if (threadIdx.x == 0) status[blockIdx.x] = st;
}

// Grid x is the global row; files of the other sample size, and files with neither swap nor predictor, return at once.
template <typename T>
__global__ __launch_bounds__(64) void tiffb_unpredict_kernel(const TdFile* __restrict__ tab, uint32_t n_files, uint8_t* rasters) {
    const TdFile& f = tab[td_first(td_find_file(tab, n_files, blockIdx.x, true))];
    const uint32_t row = blockIdx.x - f.first_row;
    if (!f.in_batch || row >= f.H || f.bps != sizeof(T) || !(f.swap || f.predictor)) return;
    td_unpredict_row(reinterpret_cast<T*>(rasters + f.raster_off + (size_t)row * f.line), f.W, f.spp, f.swap, f.predictor);
}

// One thread per strip: a strip that is not clean marks its file, and no other.  file_status is zero before.
__global__ __launch_bounds__(256) void tiffb_status_kernel(const TdFile* __restrict__ tab, uint32_t n_files, const uint32_t* __restrict__ strip_status,
                                                           uint32_t n_strips, uint32_t* file_status) {
    const uint32_t strip = blockIdx.x * 256u + threadIdx.x;
    if (strip >= n_strips || !strip_status[strip]) return;
    atomicOr(&file_status[td_find_file(tab, n_files, strip, false)], 1u);
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

hipError_t run_tiff_decode_batch(const TiffDecodeBatchBufs& b, const TdBatchLayout& L, hipStream_t s) {
    const uint32_t n = (uint32_t)L.tab.size(), ns = (uint32_t)L.n_strips, nr = (uint32_t)L.n_rows;
    hipError_t e = hipMemsetAsync(b.file_status, 0, (size_t)n * sizeof(uint32_t), s);
    if (e != hipSuccess || ns == 0) return e;
    hipLaunchKernelGGL(tiffb_unstrip_kernel, dim3(ns), dim3(64), 0, s, b.tab, n, b.files, b.tables, b.rasters, b.strip_status);
    if (L.any_u16_pass) hipLaunchKernelGGL(tiffb_unpredict_kernel<uint16_t>, dim3(nr), dim3(64), 0, s, b.tab, n, b.rasters);
    if (L.any_u8_predictor) hipLaunchKernelGGL(tiffb_unpredict_kernel<uint8_t>, dim3(nr), dim3(64), 0, s, b.tab, n, b.rasters);
    hipLaunchKernelGGL(tiffb_status_kernel, dim3((ns + 255) / 256), dim3(256), 0, s, b.tab, n, b.strip_status, ns, b.file_status);
    return hipGetLastError();
}

}  // namespace ecseg
