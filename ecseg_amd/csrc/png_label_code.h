// Host-only: the Huffman code of a label PNG's one dynamic block, built from the image's 68 token counts, shared by the host coder
// (deflate_labels, host_io.cpp) and the device coder's driver (ecseg_png_labels_encode, drivers_files.hip; kernels in png_kernels.hip).
// Tie-breaking has this one definition.  The stream is
//   78 01 | block header | per scan line: the literal 0 (filter byte), then per run of k pixels of one colour its four palette
//   literals, (k - 1) / 64 matches of 256 bytes, one match of 4 ((k - 1) % 64) bytes if that is not zero | end of block | zero bits
//   to a byte | Adler-32, big-endian
// with every match at distance 4, the only distance code, sent as the single bit 0.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <algorithm>
#include <cstring>
#include <utility>
#include <vector>

namespace ecseg {

struct BitWriter {                                        // branch-free: speckled label maps make every data-dependent branch a coin flip
    uint8_t* p;                                           // into a buffer sized for the worst case (+ 8 bytes of slack) by the caller
    uint64_t acc = 0;
    int n = 0;                                            // < 8 between calls
    explicit BitWriter(uint8_t* dst) : p(dst) {}
    inline void put(uint64_t bits, int len) {             // LSB-first; len <= 56
        acc |= bits << n;
        n += len;
        std::memcpy(p, &acc, 8);                          // little-endian host (x86-64 / the GPU boxes); whole bytes are kept below
        p += n >> 3;
        acc >>= (n & ~7);
        n &= 7;
    }
    uint8_t* finish() {
        if (n > 0) { *p++ = (uint8_t)acc; }
        acc = 0; n = 0;
        return p;
    }
};

// code lengths (<= 15) of a Huffman code for the given counts; symbols with count 0 get length 0; a lone used symbol gets 1
inline void huffman_lengths(const uint32_t* freq, int nsym, uint8_t* len) {
    std::vector<uint64_t> f(freq, freq + nsym);
    for (;;) {
        struct Node { uint64_t w; int l, r; };
        std::vector<Node> nodes;
        std::vector<int> live;
        for (int i = 0; i < nsym; ++i) { len[i] = 0; if (f[i]) { nodes.push_back({f[i], -1 - i, 0}); live.push_back((int)nodes.size() - 1); } }
        if (live.empty()) return;
        if (live.size() == 1) { len[-1 - nodes[live[0]].l] = 1; return; }
        while (live.size() > 1) {                             // (tens of symbols: a quadratic merge is fine)
            int a = 0, b = 1;
            if (nodes[live[b]].w < nodes[live[a]].w) std::swap(a, b);
            for (int k = 2; k < (int)live.size(); ++k) {
                if (nodes[live[k]].w < nodes[live[a]].w) { b = a; a = k; }
                else if (nodes[live[k]].w < nodes[live[b]].w) b = k;
            }
            nodes.push_back({nodes[live[a]].w + nodes[live[b]].w, live[a], live[b]});
            const int hi = std::max(a, b), lo = std::min(a, b);
            live.erase(live.begin() + hi);
            live[lo] = (int)nodes.size() - 1;
        }
        int maxlen = 0;
        std::vector<std::pair<int, int>> stack{{live[0], 0}};
        while (!stack.empty()) {
            const auto [id, d] = stack.back();
            stack.pop_back();
            if (nodes[id].l < 0) { len[-1 - nodes[id].l] = (uint8_t)d; maxlen = std::max(maxlen, d); }
            else { stack.push_back({nodes[id].l, d + 1}); stack.push_back({nodes[id].r, d + 1}); }
        }
        if (maxlen <= 15) return;
        for (auto& v : f) if (v) v = (v + 1) / 2;              // flatten the distribution and try again
    }
}

// canonical codes, bit-reversed for deflate's LSB-first packing
inline void canonical_codes(const uint8_t* len, int nsym, uint16_t* code) {
    int count[16] = {0}, next[16] = {0};
    for (int i = 0; i < nsym; ++i) ++count[len[i]];
    count[0] = 0;
    int c = 0;
    for (int b = 1; b < 16; ++b) { c = (c + count[b - 1]) << 1; next[b] = c; }
    for (int i = 0; i < nsym; ++i) {
        if (!len[i]) { code[i] = 0; continue; }
        int v = next[len[i]]++, r = 0;
        for (int k = 0; k < len[i]; ++k) { r = (r << 1) | (v & 1); v >>= 1; }
        code[i] = (uint16_t)r;
    }
}

struct LenCode { uint16_t sym; uint8_t extra_bits; uint8_t extra; };
inline LenCode length_code(int L) {                          // deflate length 3..258 -> symbol 257.. + extra bits
    static const int base[29] = {3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258};
    static const int ebits[29] = {0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0};
    int i = 28;
    while (base[i] > L) --i;
    return LenCode{(uint16_t)(257 + i), (uint8_t)ebits[i], (uint8_t)(L - base[i])};
}

// labels/<stem>.png's colours (ecseg_png_write_labels, host_io.cpp): class k -> colour k, RGBA
constexpr uint8_t LABEL_PNG_PALETTE[4][4] = {{0x38, 0x6c, 0xb0, 255}, {0xff, 0xff, 0x99, 255}, {0x7f, 0xc9, 0x7f, 255}, {0xf0, 0x02, 0x7f, 255}};

// What one image's stream is written with.  head: the two zlib bytes and the block header, head_bits bits of it (the last byte is
// zero above them); cbits / cn: per colour the bit string of its four literals (at most 60 bits); mbits / mn: per match of 4 m
// bytes, m = 1..64, its length code, extra bits and the distance code "0" (at most 21 bits; m = 0: no match, zero bits);
// filt / eob: the codes of the literal 0 and of the end of the block.
struct LabelPngCode {
    uint8_t head[256];
    uint32_t head_bits;
    uint64_t cbits[4]; int cn[4];
    uint32_t mbits[65]; int mn[65];
    uint32_t filt, eob; int filt_n, eob_n;
};

// flit: runs per colour; flen[m], m = 1..64: matches of 4 m bytes (flen[64] includes the whole-64 parts of long runs, flen[0] is
// ignored); H: scan lines
inline void label_png_code(const uint32_t flit[4], const uint32_t flen[65], uint32_t H, const uint8_t pal[4][4], LabelPngCode* out) {
    uint32_t freq[286] = {0};
    freq[0] += H;                                             // filter bytes
    for (int c = 0; c < 4; ++c) for (int k = 0; k < 4; ++k) freq[pal[c][k]] += flit[c];
    freq[256] = 1;
    bool any_match = false;
    for (int m = 1; m <= 64; ++m) if (flen[m]) { freq[length_code(4 * m).sym] += flen[m]; any_match = true; }
    uint8_t llen[286], dlen[4] = {0, 0, 0, 0};
    uint16_t lcode[286];
    huffman_lengths(freq, 286, llen);
    canonical_codes(llen, 286, lcode);
    if (any_match) dlen[3] = 1;                               // distance 4 = distance code 3, the only one: a single 1-bit code (bit 0)
    // code-length alphabet: a fixed complete code (13 symbols of 4 bits, 6 of 5 bits); lengths are sent one by one
    uint8_t cl_len[19];
    uint16_t cl_code[19];
    for (int i = 0; i < 19; ++i) cl_len[i] = i < 13 ? 4 : 5;
    canonical_codes(cl_len, 19, cl_code);
    std::memset(out->head, 0, sizeof out->head);              // (16 + 17 + 57 + 290 * 5 = 1540 bits at most, + the writer's 8 bytes of slack)
    out->head[0] = 0x78; out->head[1] = 0x01;
    BitWriter bw(out->head + 2);
    bw.put(1, 1); bw.put(2, 2);                               // BFINAL, BTYPE = dynamic
    bw.put(286 - 257, 5); bw.put(4 - 1, 5); bw.put(19 - 4, 4);
    static const int order[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
    for (int i = 0; i < 19; ++i) bw.put(cl_len[order[i]], 3);
    for (int i = 0; i < 286; ++i) bw.put(cl_code[llen[i]], cl_len[llen[i]]);
    for (int i = 0; i < 4; ++i) bw.put(cl_code[dlen[i]], cl_len[dlen[i]]);
    out->head_bits = (uint32_t)(8 * (bw.p - out->head) + bw.n);
    bw.finish();
    // per colour: the bit string of its four literals; per match length 4 m: length code + extra bits + the 1-bit distance code
    for (int c = 0; c < 4; ++c) {
        out->cbits[c] = 0; out->cn[c] = 0;
        for (int k = 0; k < 4; ++k) { out->cbits[c] |= (uint64_t)lcode[pal[c][k]] << out->cn[c]; out->cn[c] += llen[pal[c][k]]; }
    }
    out->mbits[0] = 0; out->mn[0] = 0;                        // "no remainder match": zero bits
    for (int m = 1; m <= 64; ++m) {
        const LenCode lc = length_code(4 * m);
        out->mbits[m] = (uint32_t)lcode[lc.sym] | ((uint32_t)lc.extra << llen[lc.sym]);
        out->mn[m] = llen[lc.sym] + lc.extra_bits + 1;        // + distance code "0"
    }
    out->filt = lcode[0]; out->filt_n = llen[0];
    out->eob = lcode[256]; out->eob_n = llen[256];
}

// bytes of the stream, known before a bit of it is written: header, count x code length of every token, end of block, Adler-32
inline size_t label_png_stream_bytes(const LabelPngCode& k, const uint32_t flit[4], const uint32_t flen[65], uint32_t H) {
    uint64_t bits = k.head_bits + (uint64_t)H * k.filt_n + k.eob_n;
    for (int c = 0; c < 4; ++c) bits += (uint64_t)flit[c] * k.cn[c];
    for (int m = 1; m <= 64; ++m) bits += (uint64_t)flen[m] * k.mn[m];
    return (size_t)((bits + 7) / 8 + 4);
}

// bytes of the file around a stream of z bytes: signature, IHDR, IDAT's length, tag and CRC, IEND
inline size_t label_png_file_bytes(size_t z) { return 8 + 25 + 12 + z + 12; }
constexpr size_t LABEL_PNG_Z_OFFSET = 8 + 25 + 8;            // where the stream starts in the file
// The file around its stream, which lies at file + LABEL_PNG_Z_OFFSET already (png_chunk's arithmetic on a memory buffer;
// host_io.cpp, which has zlib's crc32)
void label_png_frame(uint8_t* file, size_t z, int H, int W);

}  // namespace ecseg
