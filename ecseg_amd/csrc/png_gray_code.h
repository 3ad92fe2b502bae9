// Host-only: the parts of the gray-channel PNG coder that the host writer (deflate_gray_sub, host_io.cpp) and the device coder's
// driver (png_gray_encode, drivers_files.hip; kernels in png_gray_kernels.hip) share: the run-length scan that defines the tokens,
// the Huffman code of the one dynamic block built from the 286 symbol counts, the block header, and the stream's exact length from
// the counts alone.  huffman_lengths, canonical_codes, length_code and BitWriter are png_label_code.h's: tie-breaking has one
// definition for both coders.  The stream is
//   78 01 | block header | the tokens of the filtered bytes (png_gray_tokens.h) | end of block | zero bits to a byte | Adler-32
// with every match at distance 1, the only distance code, sent as the single bit 0.
#pragma once
#include "png_label_code.h"

namespace ecseg {

template <typename Emit>
inline void rle_scan(const uint8_t* f, size_t n, Emit&& emit) {      // emit(literal) / emit(-length) for a distance-1 match
    size_t i = 0;
    while (i < n) {
        const uint8_t b = f[i];
        emit((int)b);
        ++i;
        if (i + 2 < n && f[i] == b && f[i + 1] == b && f[i + 2] == b) {      // a run worth a match (>= 3 more of the same byte)
            size_t j = i + 3;
            while (j < n && f[j] == b) ++j;
            size_t r = j - i;
            while (r >= 3) {
                size_t L = r > 258 ? 258 : r;
                if (r - L > 0 && r - L < 3) L = r - 3;                       // never leave a tail shorter than a match
                emit(-(int)L);
                r -= L;
            }
            i = j - r;                                                      // (r == 0 here by construction)
        }
    }
}

// What one channel's stream is written with.  head: the two zlib bytes and the block header, head_bits bits of it (the last byte is
// zero above them); lcode / llen: the literal / length code; mbits / mn by match length 3..258: length code, extra bits and the
// distance code "0" (at most 21 bits).
struct GrayPngCode {
    uint8_t head[256];
    uint32_t head_bits;
    uint16_t lcode[286]; uint8_t llen[286];
    uint32_t mbits[259]; uint8_t mn[259];
};

// freq: the counts of the 286 literal / length symbols (the end of the block is counted here); any_match: some match is sent
inline void gray_png_code(const uint32_t freq_in[286], bool any_match, GrayPngCode* out) {
    uint32_t freq[286];
    std::memcpy(freq, freq_in, sizeof freq);
    freq[256] = 1;
    huffman_lengths(freq, 286, out->llen);
    canonical_codes(out->llen, 286, out->lcode);
    uint8_t cl_len[19];
    uint16_t cl_code[19];
    for (int i = 0; i < 19; ++i) cl_len[i] = i < 13 ? 4 : 5;                 // a fixed complete code for the code lengths, sent one by one
    canonical_codes(cl_len, 19, cl_code);
    std::memset(out->head, 0, sizeof out->head);                            // (16 + 17 + 57 + 287 * 5 = 1525 bits at most, + the writer's 8 bytes of slack)
    out->head[0] = 0x78; out->head[1] = 0x01;
    BitWriter bw(out->head + 2);
    bw.put(1, 1); bw.put(2, 2);                                             // BFINAL, BTYPE = dynamic
    bw.put(286 - 257, 5); bw.put(1 - 1, 5); bw.put(19 - 4, 4);              // 286 literal / length codes, ONE distance code
    static const int order[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
    for (int i = 0; i < 19; ++i) bw.put(cl_len[order[i]], 3);
    for (int i = 0; i < 286; ++i) bw.put(cl_code[out->llen[i]], cl_len[out->llen[i]]);
    const int d0 = any_match ? 1 : 0;                                       // distance code 0 (distance 1): a 1-bit code, bit 0
    bw.put(cl_code[d0], cl_len[d0]);
    out->head_bits = (uint32_t)(8 * (bw.p - out->head) + bw.n);
    bw.finish();
    out->mbits[0] = out->mbits[1] = out->mbits[2] = 0; out->mn[0] = out->mn[1] = out->mn[2] = 0;
    for (int L = 3; L <= 258; ++L) {
        const LenCode lc = length_code(L);
        out->mbits[L] = (uint32_t)out->lcode[lc.sym] | ((uint32_t)lc.extra << out->llen[lc.sym]);
        out->mn[L] = (uint8_t)(out->llen[lc.sym] + lc.extra_bits + 1);
    }
}

// bytes of the stream, known before a bit of it is written: header, count x code length of every symbol, the extra bits and the
// distance bit of every match, end of block, Adler-32
inline size_t gray_png_stream_bytes(const GrayPngCode& k, const uint32_t freq[286]) {
    static const int ebits[29] = {0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0};
    uint64_t bits = k.head_bits + k.llen[256];
    for (int s = 0; s < 256; ++s) bits += (uint64_t)freq[s] * k.llen[s];
    for (int s = 257; s < 286; ++s) bits += (uint64_t)freq[s] * (k.llen[s] + ebits[s - 257] + 1);
    return (size_t)((bits + 7) / 8 + 4);
}

// A size no stream of n filtered bytes exceeds: a literal costs at most 15 bits, a match at most 21 for three bytes or more, and the
// zlib bytes, the block header, the end of the block, the padding and the Adler-32 stay below 256 bytes.  The writers' buffers of
// 2 n + 4096 bytes hold it.
inline size_t gray_png_stream_bound(size_t n) { return (15 * n + 7) / 8 + 256; }

// the file around a stream of z bytes is the label PNG's (label_png_file_bytes, LABEL_PNG_Z_OFFSET); its IHDR says colour type 0
void gray_png_frame(uint8_t* file, size_t z, int H, int W);

}  // namespace ecseg
