// The LZW strips of stat_fish's TIFF files on gfx950: what tiff_write_u8 (host_io.cpp) does one strip after another on a host
// thread - horizontal predictor, `invert`, ecseg_lzw_encode (host_codec.cpp) - as one wave per strip, and the packing of the
// strips into the `data` bytes of the file.  Greedy LZW with libtiff's rules has one output, so every byte is the host's.
//
// tiff_lzw_strip_kernel: one strip per workgroup of ONE wave.  Lane 0 is the encoder, a serial stream in plain C++ (as ws_flood,
// watershed_kernels.hip); the other 63 lanes are its memory system:
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
#include "common.h"

namespace ecseg {

namespace {

constexpr int TL_HBITS = 13, TL_HSIZE = 1 << TL_HBITS;
constexpr uint32_t TL_EMPTY = 0xffffffffu;
constexpr int TL_IN = 1024;                                  // staged input bytes
constexpr int TL_OUT_WORDS = 512;                            // (TL_IN + 2 codes of 12 bits are 385 words)

struct TlEncoder { unsigned long long acc; int nbits, width, next, cur; uint32_t ow; };

__device__ __forceinline__ void tl_put(TlEncoder& e, uint32_t* outw, int code) {
    e.acc = (e.acc << e.width) | (uint32_t)code;             // (nbits <= 31 before: at most 43 bits in flight)
    e.nbits += e.width;
    if (e.nbits >= 32) {
        const uint32_t w = (uint32_t)(e.acc >> (e.nbits - 32));
        if (e.ow < (uint32_t)TL_OUT_WORDS) outw[e.ow] = __builtin_bswap32(w);
        ++e.ow;
        e.nbits -= 32;
    }
}

__device__ __forceinline__ void tl_clear(uint32_t* tab, int lane) {
    uint4* t4 = reinterpret_cast<uint4*>(tab);
    for (int k = lane; k < TL_HSIZE / 4; k += 64) t4[k] = make_uint4(TL_EMPTY, TL_EMPTY, TL_EMPTY, TL_EMPTY);
}

__global__ __launch_bounds__(64) void tiff_lzw_strip_kernel(TiffSources srcs, int H, uint32_t line, uint32_t spp, int rps, uint32_t flip,
                                                            uint8_t* __restrict__ slots, size_t slot_stride, uint32_t* __restrict__ cnt) {
    __shared__ __attribute__((aligned(16))) uint32_t tab[TL_HSIZE];
    __shared__ uint32_t inw[TL_IN / 4];
    __shared__ uint32_t outw[TL_OUT_WORDS];
    uint8_t* in8 = reinterpret_cast<uint8_t*>(inw);
    const int lane = threadIdx.x;
    const size_t strip = blockIdx.x, file = blockIdx.y, slot = file * gridDim.x + strip;
    const int r0 = (int)strip * rps, rows = r0 + rps <= H ? rps : H - r0;
    const uint32_t n = (uint32_t)rows * line;                // <= 8192 with more than one row, else one line < 2^30
    const uint8_t* __restrict__ src = srcs.img[srcs.stride ? 0 : file] + file * srcs.stride + (size_t)r0 * line;
    uint32_t* __restrict__ dst = reinterpret_cast<uint32_t*>(slots + slot * slot_stride);
    const uint32_t slot_words = (uint32_t)(slot_stride / 4);
    uint32_t written = 0;                                    // words of the slot that hold output
    TlEncoder e{0ull, 0, 9, 258, 0, 0u};
    tl_clear(tab, lane);
    if (lane == 0) tl_put(e, outw, 256);
    __syncthreads();
    for (uint32_t c0 = 0; c0 < n; c0 += TL_IN) {
        const uint32_t cn = n - c0 < (uint32_t)TL_IN ? n - c0 : (uint32_t)TL_IN;
#pragma unroll 4
        for (uint32_t k = lane; k < cn; k += 64) {
            const uint32_t j = c0 + k, x = rows == 1 ? j : j % line;
            uint32_t v = src[j] ^ flip;
            if (x >= spp) v -= src[j - spp] ^ flip;          // horizontal differencing (mod 256)
            in8[k] = (uint8_t)v;
        }
        __syncthreads();
        uint32_t i = 0;
        for (;;) {                                           // until the chunk is eaten: one more turn per restart inside it
            int restart = 0;
            if (lane == 0) {
                if (c0 == 0 && i == 0) { e.cur = in8[0]; i = 1; }
                uint32_t c = i < cn ? in8[i] : 0;
                while (i < cn) {
                    const uint32_t ahead = in8[i + 1 < (uint32_t)TL_IN ? i + 1 : i];     // the next byte, asked for before the probe's answer
                    const uint32_t key = ((uint32_t)e.cur << 8) | c;
                    uint32_t hpos = (key * 2654435761u) >> (32 - TL_HBITS);
                    uint32_t en = tab[hpos];
                    while (en != TL_EMPTY && (en >> 12) != key) {
                        hpos = (hpos + 1) & (TL_HSIZE - 1);
                        en = tab[hpos];
                    }
                    ++i;
                    if (en != TL_EMPTY) {
                        e.cur = (int)(en & 0xfffu);
                    } else {
                        tl_put(e, outw, e.cur);
                        tab[hpos] = (key << 12) | (uint32_t)e.next++;
                        e.cur = (int)c;
                        if (e.next == 4094) {                // table full: restart (libtiff's CODE_MAX - 1 rule)
                            tl_put(e, outw, 256);
                            e.next = 258; e.width = 9;
                            restart = 1;
                            break;
                        }
                        if (e.next > (1 << e.width) - 1 && e.width < 12) ++e.width;
                    }
                    c = ahead;
                }
            }
            restart = __shfl(restart, 0);
            if (!restart) break;
            __syncthreads();
            tl_clear(tab, lane);
            __syncthreads();
        }
        const uint32_t ow = __shfl(e.ow, 0);
        __syncthreads();
        for (uint32_t k = lane; k < ow && k < (uint32_t)TL_OUT_WORDS; k += 64)
            if (written + k < slot_words) dst[written + k] = outw[k];
        written += ow;
        e.ow = 0;
        __syncthreads();
    }
    if (lane == 0) {
        if (n > 0) {                                         // last(): the decoder adds one more entry after this code
            tl_put(e, outw, e.cur);
            ++e.next;
            if (e.next > (1 << e.width) - 1 && e.width < 12) ++e.width;
        }
        tl_put(e, outw, 257);
        const uint32_t whole = e.ow;
        if (e.nbits > 0) {                                   // the last 1..31 bits, zero-padded to a byte (and to the dword)
            outw[e.ow < (uint32_t)TL_OUT_WORDS ? e.ow : 0] = __builtin_bswap32((uint32_t)(e.acc << (32 - e.nbits)));
            ++e.ow;
        }
        const uint32_t bytes = (written + whole) * 4u + (uint32_t)((e.nbits + 7) >> 3);     // (at most 1.5004 n + 9: inside the slot)
        cnt[slot] = bytes < (uint32_t)slot_stride ? bytes : (uint32_t)slot_stride - 1u;
    }
    const uint32_t ow = __shfl(e.ow, 0);
    __syncthreads();
    for (uint32_t k = lane; k < ow && k < (uint32_t)TL_OUT_WORDS; k += 64)
        if (written + k < slot_words) dst[written + k] = outw[k];
}

__global__ __launch_bounds__(256) void tiff_scan_kernel(const uint32_t* __restrict__ cnt, int nstrips, unsigned long long* __restrict__ off) {
    __shared__ unsigned long long sh[256];
    const int t = threadIdx.x;
    cnt += (size_t)blockIdx.y * nstrips;
    off += (size_t)blockIdx.y * ((size_t)nstrips + 1);
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

__global__ __launch_bounds__(256) void tiff_gather_kernel(const uint8_t* __restrict__ slots, size_t slot_stride, const uint32_t* __restrict__ cnt,
                                                          const unsigned long long* __restrict__ off, uint8_t* __restrict__ packed,
                                                          size_t file_stride) {
    const size_t strip = blockIdx.x, file = blockIdx.y, nstrips = gridDim.x, slot = file * nstrips + strip;
    const uint32_t m = cnt[slot], pairs = (m + (m & 1u)) / 2;            // (an odd strip's pad byte is the 0 behind it in its slot)
    const uint16_t* __restrict__ s = reinterpret_cast<const uint16_t*>(slots + slot * slot_stride);
    uint16_t* __restrict__ d = reinterpret_cast<uint16_t*>(packed + file * file_stride + off[file * (nstrips + 1) + strip]);
    for (uint32_t k = threadIdx.x; k < pairs; k += 256) d[k] = s[k];
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

}  // namespace ecseg
