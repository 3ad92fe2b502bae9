// The strips of TIFF files decoded on gfx950: what ecseg_tiff_read (host_io.cpp) does one strip after another on a host thread -
// ecseg_lzw_decode (host_codec.cpp) or a copy, zero fill, byte order, horizontal predictor - from the file images as they were
// uploaded and their strip tables, into the rasters.  One set of kernels over a batch of files (ecseg_tiff_decode_batch,
// ecseg_meta_segment_tiffs); a lone file (ecseg_tiff_decode) is a batch of one.
//
// Grid dimension x is the strip or row counted over all files; the file is found in the table (TdFile, tiff_decode_batch.h) by binary
// search of its first-strip / first-row column - the index is the workgroup's, so the search is wave-uniform.
// tiffb_unstrip_kernel: one strip per workgroup of ONE wave.  The routines are td_lzw_strip (tiff_decode_strip.h, which says how the
// wave shares the work and why its copies are ordered) and, for uncompressed strips, td_raw_strip: a clamped copy and the zero fill.
// td_strip finds the strip's bytes in the file and clamps them to the file; one status word per strip (0, or 1: corrupt stream /
// offset behind the file).  A strip the tables do not have is zero-filled.  One launch serves LZW and uncompressed files mixed; the
// strips of different files share nothing, which is where a batch of files of few strips finds its parallelism.
// tiffb_inflate_kernel: the same grid for the strips of Deflate files (ti_inflate_strip, tiff_inflate_strip.h), launched only for a
// batch that holds one; each of the two kernels leaves the other's strips at once.
// tiffb_packbits_kernel: the same grid once more for the strips of PackBits files (tp_packbits_strip, tiff_packbits_strip.h: the
// header walk in every lane, the bytes of a run written by the lanes), launched only for a batch that holds one.
// tiffb_unpredict_kernel: one wave per row, after all strips: 16-bit samples of a big-endian file are swapped to native order, then
// the horizontal predictor is undone per sample channel (stride spp) as an inclusive wave scan over 64 samples with a carry
// into the next 64, modulo 2^8 or 2^16 (td_unpredict_row).
// tiffb_untile_kernel: only for a batch with tiled files (the handle option tiff_tiled_on_device), after the strip kernels, in
// which a tile is a strip of the grid whose stream decodes into its staging slot.  Grid x is the row of tiles counted over the tiled
// files (TdTiles), grid y splits the rows of the tiles among TD_UNTILE_PARTS waves; a wave puts whole raster rows in their place:
// byte order, the predictor along each tile row, the padding of edge tiles dropped (tiff_untile.h).  The row kernel above leaves
// tiled files alone.
// tiffb_status_kernel: the strip words folded into one word per file.
#include "common.h"
#include "tiff_decode_strip.h"
#include "tiff_inflate_strip.h"
#include "tiff_packbits_strip.h"
#include "tiff_untile.h"

namespace ecseg {

namespace {

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

// ---- the kernels: the pointers come from the table (tiff_decode_batch.h), the work is td_unpredict_row and tiff_decode_strip.h ----
__global__ __launch_bounds__(64) void tiffb_unstrip_kernel(const TdFile* __restrict__ tab, uint32_t n_files, const uint8_t* __restrict__ files,
                                                           const uint32_t* __restrict__ tables, uint8_t* rasters, uint32_t* __restrict__ status,
                                                           const TdTiles* __restrict__ tiles, uint8_t* staging) {
    __shared__ TdLds L;
    const uint32_t st = tdb_unstrip(tab, n_files, files, tables, rasters, blockIdx.x, L, tiles, staging);
    if (threadIdx.x == 0 && st != TD_OTHER_KERNEL) status[blockIdx.x] = st;
}

// The same grid for the Deflate strips (ti_inflate_strip, tiff_inflate_strip.h): a workgroup whose strip is the kernel's above
// returns at once, as that kernel's do here.  The two write disjoint status words and disjoint rows of the rasters.
__global__ __launch_bounds__(64) void tiffb_inflate_kernel(const TdFile* __restrict__ tab, uint32_t n_files, const uint8_t* __restrict__ files,
                                                           const uint32_t* __restrict__ tables, uint8_t* rasters, uint32_t* __restrict__ status,
                                                           const TdTiles* __restrict__ tiles, uint8_t* staging) {
    __shared__ TiLds L;
    const uint32_t st = tdb_inflate(tab, n_files, files, tables, rasters, blockIdx.x, L, tiles, staging);
    if (threadIdx.x == 0 && st != TD_OTHER_KERNEL) status[blockIdx.x] = st;
}

// And for the PackBits strips (tp_packbits_strip, tiff_packbits_strip.h), under the same rule.
__global__ __launch_bounds__(64) void tiffb_packbits_kernel(const TdFile* __restrict__ tab, uint32_t n_files, const uint8_t* __restrict__ files,
                                                            const uint32_t* __restrict__ tables, uint8_t* rasters, uint32_t* __restrict__ status,
                                                            const TdTiles* __restrict__ tiles, uint8_t* staging) {
    __shared__ TpLds L;
    const uint32_t st = tdb_packbits(tab, n_files, files, tables, rasters, blockIdx.x, L, tiles, staging);
    if (threadIdx.x == 0 && st != TD_OTHER_KERNEL) status[blockIdx.x] = st;
}

// Grid x is the global row; files of the other sample size, and files with neither swap nor predictor, return at once.
template <typename T>
__global__ __launch_bounds__(64) void tiffb_unpredict_kernel(const TdFile* __restrict__ tab, uint32_t n_files, uint8_t* rasters) {
    const TdFile& f = tab[td_first(td_find_file(tab, n_files, blockIdx.x, true))];
    const uint32_t row = blockIdx.x - f.first_row;
    if (!f.in_batch || f.tiles || row >= f.H || f.bps != sizeof(T) || !(f.swap || f.predictor)) return;
    td_unpredict_row(reinterpret_cast<T*>(rasters + f.raster_off + (size_t)row * f.line), f.W, f.spp, f.swap, f.predictor);
}

// Grid x is the global row of tiles, grid y the part of its rows (tdb_untile, tiff_untile.h).
constexpr uint32_t TD_UNTILE_PARTS = 8;
__global__ __launch_bounds__(64) void tiffb_untile_kernel(const TdFile* __restrict__ tab, const TdTiles* __restrict__ tiles, uint32_t n_tiled,
                                                          const uint8_t* __restrict__ files, const uint32_t* __restrict__ tables,
                                                          const uint8_t* __restrict__ staging, uint8_t* rasters) {
    tdb_untile(tab, tiles, n_tiled, files, tables, staging, rasters, blockIdx.x, blockIdx.y, TD_UNTILE_PARTS);
}

// One thread per strip: a strip that is not clean marks its file, and no other.  file_status is zero before.
__global__ __launch_bounds__(256) void tiffb_status_kernel(const TdFile* __restrict__ tab, uint32_t n_files, const uint32_t* __restrict__ strip_status,
                                                           uint32_t n_strips, uint32_t* file_status) {
    const uint32_t strip = blockIdx.x * 256u + threadIdx.x;
    if (strip >= n_strips || !strip_status[strip]) return;
    atomicOr(&file_status[td_find_file(tab, n_files, strip, false)], 1u);
}

}  // namespace

hipError_t run_tiff_decode_batch(const TiffDecodeBatchBufs& b, const TdBatchLayout& L, hipStream_t s) {
    const uint32_t n = (uint32_t)L.tab.size(), ns = (uint32_t)L.n_strips, nr = (uint32_t)L.n_rows;
    hipError_t e = hipMemsetAsync(b.file_status, 0, (size_t)n * sizeof(uint32_t), s);
    if (e != hipSuccess || ns == 0) return e;
    hipLaunchKernelGGL(tiffb_unstrip_kernel, dim3(ns), dim3(64), 0, s, b.tab, n, b.files, b.tables, b.rasters, b.strip_status, b.tiles, b.staging);
    if (L.any_deflate)
        hipLaunchKernelGGL(tiffb_inflate_kernel, dim3(ns), dim3(64), 0, s, b.tab, n, b.files, b.tables, b.rasters, b.strip_status, b.tiles, b.staging);
    if (L.any_packbits)
        hipLaunchKernelGGL(tiffb_packbits_kernel, dim3(ns), dim3(64), 0, s, b.tab, n, b.files, b.tables, b.rasters, b.strip_status, b.tiles, b.staging);
    if (!L.tiles.empty())
        hipLaunchKernelGGL(tiffb_untile_kernel, dim3((uint32_t)L.n_trows, TD_UNTILE_PARTS), dim3(64), 0, s, b.tab, b.tiles, (uint32_t)L.tiles.size(), b.files,
                           b.tables, b.staging, b.rasters);
    if (L.any_u16_pass) hipLaunchKernelGGL(tiffb_unpredict_kernel<uint16_t>, dim3(nr), dim3(64), 0, s, b.tab, n, b.rasters);
    if (L.any_u8_predictor) hipLaunchKernelGGL(tiffb_unpredict_kernel<uint8_t>, dim3(nr), dim3(64), 0, s, b.tab, n, b.rasters);
    hipLaunchKernelGGL(tiffb_status_kernel, dim3((ns + 255) / 256), dim3(256), 0, s, b.tab, n, b.strip_status, ns, b.file_status);
    return hipGetLastError();
}

}  // namespace ecseg
