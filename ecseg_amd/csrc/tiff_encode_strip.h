// One LZW strip encoded by one wave: the routine of tiff_lzw_strip_kernel and tiffb_lzw_strip_kernel (tiff_kernels.hip, whose head
// describes it), stated once and written so that the host compiler takes it too - tools/asan/tiff_encode_batch_fuzz.cpp runs it
// under ASan + UBSan against ecseg_lzw_encode (host_codec.cpp) behind the predictor, which is its specification.  Under hipcc a lane
// is a thread of the wave, te_first a read of lane 0 and te_sync the workgroup's barrier; under the host compiler the lanes are a
// loop and the other two do nothing (as tiff_decode_strip.h).  The two kernels differ only in where the arguments come from.
#pragma once
#include <stdint.h>

#ifdef __HIPCC__
#define TE_FN __device__ __forceinline__
#define TE_FOR_LANES(lane) for (uint32_t lane = threadIdx.x, te_once_ = 1; te_once_; te_once_ = 0)
#define TE_CONTROL_LANE if (threadIdx.x == 0)
#define TE_UNROLL_4 _Pragma("unroll 4")
TE_FN uint32_t te_first(uint32_t v) { return (uint32_t)__shfl((int)v, 0); }
TE_FN void te_sync() { __syncthreads(); }
TE_FN uint32_t te_bswap(uint32_t v) { return __builtin_bswap32(v); }
#else
#define TE_FN inline
#define TE_FOR_LANES(lane) for (uint32_t lane = 0; lane < 64; ++lane)
#define TE_CONTROL_LANE
#define TE_UNROLL_4
inline uint32_t te_first(uint32_t v) { return v; }
inline void te_sync() {}
inline uint32_t te_bswap(uint32_t v) { return __builtin_bswap32(v); }
#endif

namespace ecseg {

constexpr int TL_HBITS = 13, TL_HSIZE = 1 << TL_HBITS;
constexpr uint32_t TL_EMPTY = 0xffffffffu;
constexpr int TL_IN = 1024;                                  // staged input bytes
constexpr int TL_OUT_WORDS = 512;                            // (TL_IN + 2 codes of 12 bits are 385 words)

// the wave's LDS: the dictionary, the staged bytes of the strip (predictor and flip applied), the codes on their way out
struct TlLds { alignas(16) uint32_t tab[TL_HSIZE]; uint32_t inw[TL_IN / 4]; uint32_t outw[TL_OUT_WORDS]; };

struct TlEncoder { unsigned long long acc; int nbits, width, next, cur; uint32_t ow; };

TE_FN void tl_put(TlEncoder& e, uint32_t* outw, int code) {
    e.acc = (e.acc << e.width) | (uint32_t)code;             // (nbits <= 31 before: at most 43 bits in flight)
    e.nbits += e.width;
    if (e.nbits >= 32) {
        const uint32_t w = (uint32_t)(e.acc >> (e.nbits - 32));
        if (e.ow < (uint32_t)TL_OUT_WORDS) outw[e.ow] = te_bswap(w);
        ++e.ow;
        e.nbits -= 32;
    }
}

TE_FN void tl_clear(uint32_t* tab) {
#ifdef __HIPCC__
    uint4* t4 = reinterpret_cast<uint4*>(tab);
    for (int k = threadIdx.x; k < TL_HSIZE / 4; k += 64) t4[k] = make_uint4(TL_EMPTY, TL_EMPTY, TL_EMPTY, TL_EMPTY);
#else
    for (int k = 0; k < TL_HSIZE; ++k) tab[k] = TL_EMPTY;
#endif
}

// The strip of `rows` rows of `line` bytes at src (n = rows * line: at most 8192 with more than one row, else one line below 2^30),
// spp samples per pixel, every byte xor `flip`: its LZW stream into dst (slot_words dwords, in whole dwords, zero-padded) and its
// length in bytes into *cnt (below 4 * slot_words).
TE_FN void tl_strip(const uint8_t* __restrict__ src, int rows, uint32_t line, uint32_t spp, uint32_t flip, uint32_t* __restrict__ dst,
                    uint32_t slot_words, uint32_t* __restrict__ cnt, TlLds& L) {
    uint32_t* tab = L.tab;
    uint32_t* outw = L.outw;
    uint8_t* in8 = reinterpret_cast<uint8_t*>(L.inw);
    const uint32_t n = (uint32_t)rows * line;
    uint32_t written = 0;                                    // words of the slot that hold output
    TlEncoder e{0ull, 0, 9, 258, 0, 0u};
    tl_clear(tab);
    TE_CONTROL_LANE { tl_put(e, outw, 256); }
    te_sync();
    for (uint32_t c0 = 0; c0 < n; c0 += TL_IN) {
        const uint32_t cn = n - c0 < (uint32_t)TL_IN ? n - c0 : (uint32_t)TL_IN;
        TE_FOR_LANES(lane) {
            TE_UNROLL_4
            for (uint32_t k = lane; k < cn; k += 64) {
                const uint32_t j = c0 + k, x = rows == 1 ? j : j % line;
                uint32_t v = src[j] ^ flip;
                if (x >= spp) v -= src[j - spp] ^ flip;      // horizontal differencing (mod 256)
                in8[k] = (uint8_t)v;
            }
        }
        te_sync();
        uint32_t i = 0;
        for (;;) {                                           // until the chunk is eaten: one more turn per restart inside it
            int restart = 0;
            TE_CONTROL_LANE {
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
            restart = (int)te_first((uint32_t)restart);
            if (!restart) break;
            te_sync();
            tl_clear(tab);
            te_sync();
        }
        const uint32_t ow = te_first(e.ow);
        te_sync();
        TE_FOR_LANES(lane) {
            for (uint32_t k = lane; k < ow && k < (uint32_t)TL_OUT_WORDS; k += 64)
                if (written + k < slot_words) dst[written + k] = outw[k];
        }
        written += ow;
        e.ow = 0;
        te_sync();
    }
    TE_CONTROL_LANE {
        if (n > 0) {                                         // last(): the decoder adds one more entry after this code
            tl_put(e, outw, e.cur);
            ++e.next;
            if (e.next > (1 << e.width) - 1 && e.width < 12) ++e.width;
        }
        tl_put(e, outw, 257);
        const uint32_t whole = e.ow;
        if (e.nbits > 0) {                                   // the last 1..31 bits, zero-padded to a byte (and to the dword)
            outw[e.ow < (uint32_t)TL_OUT_WORDS ? e.ow : 0] = te_bswap((uint32_t)(e.acc << (32 - e.nbits)));
            ++e.ow;
        }
        const uint32_t bytes = (written + whole) * 4u + (uint32_t)((e.nbits + 7) >> 3);     // (at most 1.5004 n + 9: inside the slot)
        const uint32_t slot_bytes = slot_words * 4u;
        *cnt = bytes < slot_bytes ? bytes : slot_bytes - 1u;
    }
    const uint32_t ow = te_first(e.ow);
    te_sync();
    TE_FOR_LANES(lane) {
        for (uint32_t k = lane; k < ow && k < (uint32_t)TL_OUT_WORDS; k += 64)
            if (written + k < slot_words) dst[written + k] = outw[k];
    }
}

}  // namespace ecseg
