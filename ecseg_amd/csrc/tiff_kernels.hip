// The LZW strips of stat_fish's TIFF files on gfx950: what tiff_write_u8 (host_io.cpp) does one strip after another on a host
// thread - horizontal predictor, `invert`, ecseg_lzw_encode (host_codec.cpp) - as one wave per strip, and the packing of the
// strips into the `data` bytes of the file.  Greedy LZW with libtiff's rules has one output, so every byte is the host's.
//
// tiff_lzw_strip_kernel: one strip per workgroup of ONE wave; its body is tl_strip (tiff_encode_strip.h), stated once for this kernel
// and the batch's.  Lane 0 is the encoder, a serial stream in plain C++ (as ws_flood, watershed_kernels.hip); the other 63 lanes are
// its memory system:
//   * the dictionary is an open-addressing table of TL_HSIZE = 8192 words in LDS, key (prefix code << 8 | byte, 20 bits) << 12 |
//     code, all ones = empty - the host's word in half its slots (at most 3836 codes live: load below 0.47), so four strips share
//     a CU's LDS.  All lanes clear it, at the start and at every restart;
//   * the strip is staged TL_IN bytes at a time into LDS with coalesced loads; the predictor (a byte minus the byte spp to its
//     left, the first spp bytes of a row as they are) and the flip of `invert` happen in that staging.  A strip of any length
//     streams through: with W * spp > 8192 a strip is one row of up to 2^30 bytes;
//   * codes leave through a 64-bit accumulator, four bytes at a time, big-endian, into an LDS buffer that all lanes write out
//     with coalesced dword stores after every staged chunk (a chunk emits at most TL_IN + 2 codes of 12 bits).
// The code stream: ClearCode first; widths 9..12, switching when next > (1 << width) - 1; ClearCode and a fresh table when next
// reaches 4094; the width step of last() before EOI; the last bits zero-padded to a byte.  The final dword is zero-padded too: the
// byte behind a strip of odd length is the 0 the file wants there, which the gather copies with it.
//
// A launch takes up to three rasters by pointer (stat_fish's colour files) or a batch at one stride (`make metaseg`'s dapi images):
// grid dimension y is the file.
//
// tiff_scan_kernel: the strip offsets, an exclusive scan over m + (m & 1) in 64 bits (one workgroup per file).
// tiff_gather_kernel: the strips back to back, two bytes per lane and store (every strip starts on an even offset).
//
// The tiffb_* kernels are the same three over a batch of files that differ in extent, samples, strip plan and `invert`
// (tiff_encode_batch.h: the TeFile table and its layout), as wsb_* stand beside ws_* in watershed_kernels.hip: the strip kernel's
// grid x runs over the strips of all files, so the waves of a 208-strip mask run beside those of the 1040-strip colour files; scan
// and gather take grid y as the file; tiffb_place_kernel between them puts the files back to back, each with room for its head and
// tail, so that the packed buffer is the call's output.  No atomics; LDS per wave is the single kernel's.
#include "common.h"
#include "tiff_encode_strip.h"

namespace ecseg {

namespace {

__global__ __launch_bounds__(64) void tiff_lzw_strip_kernel(TiffSources srcs, int H, uint32_t line, uint32_t spp, int rps, uint32_t flip,
                                                            uint8_t* __restrict__ slots, size_t slot_stride, uint32_t* __restrict__ cnt) {
    __shared__ TlLds L;
    const size_t strip = blockIdx.x, file = blockIdx.y, slot = file * gridDim.x + strip;
    const int r0 = (int)strip * rps, rows = r0 + rps <= H ? rps : H - r0;
    const uint8_t* __restrict__ src = srcs.img[srcs.stride ? 0 : file] + file * srcs.stride + (size_t)r0 * line;
    tl_strip(src, rows, line, spp, flip, reinterpret_cast<uint32_t*>(slots + slot * slot_stride), (uint32_t)(slot_stride / 4), cnt + slot, L);
}

// The file of global strip `strip`: the last row of the table that starts at or before it (every file has a strip; n >= 1).
__device__ __forceinline__ uint32_t te_find_file(const TeFile* __restrict__ tab, uint32_t n, uint32_t strip) {
    uint32_t lo = 0, hi = n;
    while (hi - lo > 1) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (tab[mid].first_strip <= strip) lo = mid; else hi = mid;
    }
    return lo;
}

// The same strip routine over a batch: grid x runs over the strips of all files, and the table says whose strip a workgroup has.
__global__ __launch_bounds__(64) void tiffb_lzw_strip_kernel(const TeFile* __restrict__ tab, uint32_t n_files, const uint8_t* __restrict__ rasters,
                                                             uint8_t* __restrict__ slots, uint32_t* __restrict__ cnt) {
    __shared__ TlLds L;
    const uint32_t g = blockIdx.x;
    const TeFile& f = tab[te_find_file(tab, n_files, g)];
    const uint32_t k = g - f.first_strip;
    if (k >= f.n_strips) return;                             // (the grid has the strips of the table: never)
    const uint32_t line = f.W * f.spp, r0 = k * f.rps;
    const int rows = (int)(r0 + f.rps <= f.H ? f.rps : f.H - r0);
    tl_strip(rasters + f.src_off + (size_t)r0 * line, rows, line, f.spp, f.flip, reinterpret_cast<uint32_t*>(slots + f.slot_off + (size_t)k * f.slot_stride),
             (uint32_t)(f.slot_stride / 4), cnt + g, L);
}

// Exclusive scan over m + (m & 1) of a file's nstrips counts into off[0 .. nstrips - 1], the total into off[nstrips]: one workgroup of 256.
__device__ __forceinline__ void tl_scan(const uint32_t* __restrict__ cnt, int nstrips, unsigned long long* __restrict__ off, unsigned long long* sh) {
    const int t = threadIdx.x;
    unsigned long long carry = 0;
    for (int base = 0; base < nstrips; base += 256) {
        const int i = base + t;
        const unsigned long long v = i < nstrips ? (unsigned long long)cnt[i] + (cnt[i] & 1u) : 0ull;
        sh[t] = v;
        __syncthreads();
        for (int d = 1; d < 256; d <<= 1) {
            const unsigned long long a = t >= d ? sh[t - d] : 0ull;
            __syncthreads();
            sh[t] += a;
            __syncthreads();
        }
        if (i < nstrips) off[i] = carry + sh[t] - v;
        carry += sh[255];
        __syncthreads();
    }
    if (t == 0) off[nstrips] = carry;
}

__global__ __launch_bounds__(256) void tiff_scan_kernel(const uint32_t* __restrict__ cnt, int nstrips, unsigned long long* __restrict__ off) {
    __shared__ unsigned long long sh[256];
    tl_scan(cnt + (size_t)blockIdx.y * nstrips, nstrips, off + (size_t)blockIdx.y * ((size_t)nstrips + 1), sh);
}

__global__ __launch_bounds__(256) void tiffb_scan_kernel(const TeFile* __restrict__ tab, const uint32_t* __restrict__ cnt, unsigned long long* __restrict__ off) {
    __shared__ unsigned long long sh[256];
    const TeFile& f = tab[blockIdx.y];
    tl_scan(cnt + f.first_strip, (int)f.n_strips, off + f.off_off, sh);
}

// Where every file image starts in the packed output: an exclusive scan over frame + strips of the files, the total into base[n_files].
// One workgroup; the files' totals are what tiffb_scan_kernel left behind their strip offsets.
__global__ __launch_bounds__(256) void tiffb_place_kernel(const TeFile* __restrict__ tab, uint32_t n_files, const unsigned long long* __restrict__ off,
                                                          unsigned long long* __restrict__ base) {
    __shared__ unsigned long long sh[256];
    const uint32_t t = threadIdx.x;
    unsigned long long carry = 0;
    for (uint32_t b0 = 0; b0 < n_files; b0 += 256) {
        const uint32_t i = b0 + t;
        const unsigned long long v = i < n_files ? tab[i].frame_bytes + off[tab[i].off_off + tab[i].n_strips] : 0ull;
        sh[t] = v;
        __syncthreads();
        for (uint32_t d = 1; d < 256; d <<= 1) {
            const unsigned long long a = t >= d ? sh[t - d] : 0ull;
            __syncthreads();
            sh[t] += a;
            __syncthreads();
        }
        if (i < n_files) base[i] = carry + sh[t] - v;
        carry += sh[255];
        __syncthreads();
    }
    if (t == 0) base[n_files] = carry;
}

// m bytes of a slot (and the 0 behind an odd strip) to d, two bytes per lane and store
__device__ __forceinline__ void tl_gather(const uint8_t* __restrict__ slot, uint32_t m, uint8_t* __restrict__ dst) {
    const uint32_t pairs = (m + (m & 1u)) / 2;               // (an odd strip's pad byte is the 0 behind it in its slot)
    const uint16_t* __restrict__ s = reinterpret_cast<const uint16_t*>(slot);
    uint16_t* __restrict__ d = reinterpret_cast<uint16_t*>(dst);
    for (uint32_t k = threadIdx.x; k < pairs; k += 256) d[k] = s[k];
}

__global__ __launch_bounds__(256) void tiff_gather_kernel(const uint8_t* __restrict__ slots, size_t slot_stride, const uint32_t* __restrict__ cnt,
                                                          const unsigned long long* __restrict__ off, uint8_t* __restrict__ packed,
                                                          size_t file_stride) {
    const size_t strip = blockIdx.x, file = blockIdx.y, nstrips = gridDim.x, slot = file * nstrips + strip;
    tl_gather(slots + slot * slot_stride, cnt[slot], packed + file * file_stride + off[file * (nstrips + 1) + strip]);
}

// grid (the most strips a file of the batch has, the files): file y's strip x behind the file's head, where tiffb_place_kernel put the file
__global__ __launch_bounds__(256) void tiffb_gather_kernel(const TeFile* __restrict__ tab, const uint8_t* __restrict__ slots, const uint32_t* __restrict__ cnt,
                                                           const unsigned long long* __restrict__ off, const unsigned long long* __restrict__ base,
                                                           uint8_t* __restrict__ packed, unsigned long long packed_bytes) {
    const TeFile& f = tab[blockIdx.y];
    const uint32_t k = blockIdx.x;
    if (k >= f.n_strips) return;
    const uint32_t m = cnt[f.first_strip + k];
    const unsigned long long at = base[blockIdx.y] + 8 + off[f.off_off + k];
    if (at + m + (m & 1u) > packed_bytes) return;            // (a count is below its slot and the buffer holds every slot: never)
    tl_gather(slots + f.slot_off + (size_t)k * f.slot_stride, m, packed + at);
}

}  // namespace

hipError_t run_tiff_encode(const TiffSources& src, int n_files, int H, int W, int spp, int invert, const TiffEncodeBufs& b, hipStream_t s) {
    const dim3 g((unsigned)b.nstrips, (unsigned)n_files);
    hipLaunchKernelGGL(tiff_lzw_strip_kernel, g, dim3(64), 0, s, src, H, (uint32_t)W * (uint32_t)spp, (uint32_t)spp, b.rps, invert ? 0xffu : 0u,
                       b.slots, b.slot_stride, b.cnt);
    hipLaunchKernelGGL(tiff_scan_kernel, dim3(1, (unsigned)n_files), dim3(256), 0, s, b.cnt, b.nstrips, b.off);
    hipLaunchKernelGGL(tiff_gather_kernel, g, dim3(256), 0, s, b.slots, b.slot_stride, b.cnt, b.off, b.packed, b.file_stride);
    return hipGetLastError();
}

hipError_t run_tiff_encode_batch(const TiffEncodeBatchBufs& b, const TeBatchLayout& L, hipStream_t s) {
    const unsigned n = (unsigned)L.tab.size();
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(tiffb_lzw_strip_kernel, dim3((unsigned)L.n_strips), dim3(64), 0, s, b.tab, n, b.src, b.slots, b.cnt);
    hipLaunchKernelGGL(tiffb_scan_kernel, dim3(1, n), dim3(256), 0, s, b.tab, b.cnt, b.off);
    hipLaunchKernelGGL(tiffb_place_kernel, dim3(1), dim3(256), 0, s, b.tab, n, b.off, b.base);
    hipLaunchKernelGGL(tiffb_gather_kernel, dim3(L.max_strips, n), dim3(256), 0, s, b.tab, b.slots, b.cnt, b.off, b.base, b.packed,
                       (unsigned long long)L.packed_bytes);
    return hipGetLastError();
}

}  // namespace ecseg
