// Host-side file I/O of `make metaseg` / `make meta_overlay` (no GPU work): the readers and writers that stand in for
// skimage.io.imread -> tifffile (reference src/utils.py:110), cv2.imwrite of dapi/<name>.tif (src/utils.py:122-123),
// plt.imsave of labels/<stem>.png (src/metaseg.py:47-52) and np.save of labels/<stem>.npy (src/metaseg.py:53), as whole-file
// C entry points.  They are called through ctypes, which drops the GIL for the duration of the call, so the decoder /
// encoder threads of ecseg_amd/metaseg.py run in parallel on the host cores instead of time-slicing one interpreter lock
// (round 2: the Python-side strip loops, gathers and widenings held `make metaseg` at 1/8 of the device rate on the
// base-16 model).  Exotic TIFF layouts (tiles, BigTIFF, PackBits, float samples, planar) return ECSEG_E_UNSUPPORTED and
// are read by the pure-Python reader in ecseg_amd/image_io.py.
#include <zlib.h>
#if defined(__SSE2__)
#include <emmintrin.h>
#endif

#include <cerrno>
#include <cstdint>
#include <cstdio>
#include <algorithm>
#include <cstring>
#include <memory>
#include <string>
#include <utility>
#include <vector>

#include "../../include/ecseg_hip.h"
#include "png_gray_code.h"
#include "png_label_code.h"
#include "tiff_frame.h"
#include "tiff_parse.h"

namespace {

using namespace ecseg;

struct File {
    FILE* f = nullptr;
    explicit File(const char* path, const char* mode) : f(std::fopen(path, mode)) {}
    ~File() { if (f) std::fclose(f); }
    bool put(const void* p, size_t n) { return n == 0 || std::fwrite(p, 1, n, f) == n; }
    bool close() { const bool ok = std::fclose(f) == 0; f = nullptr; return ok; }
};

inline void put_le16(std::vector<uint8_t>& v, uint32_t x) { v.push_back((uint8_t)x); v.push_back((uint8_t)(x >> 8)); }
inline void put_le32(std::vector<uint8_t>& v, uint32_t x) { for (int i = 0; i < 4; ++i) v.push_back((uint8_t)(x >> (8 * i))); }
inline void put_be32(uint8_t* p, uint32_t x) { p[0] = (uint8_t)(x >> 24); p[1] = (uint8_t)(x >> 16); p[2] = (uint8_t)(x >> 8); p[3] = (uint8_t)x; }

// one PNG chunk: length, tag, data, CRC-32 of tag + data
bool png_chunk(File& out, const char tag[4], const uint8_t* data, size_t n) {
    uint8_t head[8], tail[4];
    put_be32(head, (uint32_t)n);
    std::memcpy(head + 4, tag, 4);
    uLong c = crc32(0L, reinterpret_cast<const Bytef*>(tag), 4);
    size_t off = 0;
    while (off < n) {                                   // (crc32 takes a 32-bit length)
        const size_t k = n - off < (1u << 30) ? n - off : (1u << 30);
        c = crc32(c, data + off, (uInt)k);
        off += k;
    }
    put_be32(tail, (uint32_t)c);
    return out.put(head, 8) && out.put(data, n) && out.put(tail, 4);
}

// rows: H scan lines of `stride` bytes, each starting with its filter byte
// level < 0: OpenCV's default encoder settings (cv2.imwrite without parameters, modules/imgcodecs/src/grfmt_png.cpp: "tune
// parameters for speed" - Z_BEST_SPEED with the Z_RLE strategy; the caller has applied the SUB filter): run-length matching only,
// 5x faster than level-1 deflate on the noisy FISH channels
int png_write_rows(const char* path, const std::vector<uint8_t>& rows, int H, int W, int color_type, int level) {
    uLongf cap = compressBound((uLong)rows.size()) + 64;
    std::vector<uint8_t> z(cap);
    if (level >= 0) {
        if (compress2(z.data(), &cap, rows.data(), (uLong)rows.size(), level) != Z_OK) return ECSEG_E_INVALID;
    } else {
        z_stream zs;
        std::memset(&zs, 0, sizeof zs);
        if (deflateInit2(&zs, Z_BEST_SPEED, Z_DEFLATED, 15, 8, Z_RLE) != Z_OK) return ECSEG_E_INVALID;
        zs.next_in = const_cast<Bytef*>(rows.data()); zs.avail_in = (uInt)rows.size();
        zs.next_out = z.data(); zs.avail_out = (uInt)cap;
        const int r = deflate(&zs, Z_FINISH);
        cap = zs.total_out;
        deflateEnd(&zs);
        if (r != Z_STREAM_END) return ECSEG_E_INVALID;
    }
    File out(path, "wb");
    if (!out.f) return ECSEG_E_IO;
    static const uint8_t sig[8] = {0x89, 'P', 'N', 'G', '\r', '\n', 0x1a, '\n'};
    uint8_t ihdr[13];
    put_be32(ihdr, (uint32_t)W); put_be32(ihdr + 4, (uint32_t)H);
    ihdr[8] = 8; ihdr[9] = (uint8_t)color_type; ihdr[10] = 0; ihdr[11] = 0; ihdr[12] = 0;
    const bool ok = out.put(sig, 8) && png_chunk(out, "IHDR", ihdr, 13) && png_chunk(out, "IDAT", z.data(), cap) &&
                    png_chunk(out, "IEND", nullptr, 0);
    return ok && out.close() ? ECSEG_OK : ECSEG_E_IO;
}

// ---- deflate for 4-colour label images ---------------------------------------------------------------------------
// A label PNG is RGBA rows of at most four distinct pixels; zlib (level 1) spends 10 - 50 ms per 1040 x 1392 image finding
// that out byte by byte.  This encoder works on the LABELS: every scan line is run-length coded at pixel granularity - the
// first pixel of a run as 4 literals, the rest as matches of distance 4 (one pixel back) and length 4 m <= 256 - and the
// token stream goes out as ONE dynamic-Huffman block whose code is built from the image's own token counts.  Adler-32 of
// the never-materialised RGBA rows is advanced in closed form per run.  Any inflate reproduces the rows exactly (the
// pixels are the contract); realistic label maps come out as small as zlib's, speckled ones ~2.5x larger, both in a
// fraction of zlib's time.
// zlib stream (header, one dynamic block, Adler-32) of the RGBA scan lines (filter byte 0 each) of an H x W label image
// stream_bytes (optional): the size label_png_stream_bytes works out from the counts alone
void deflate_labels(const uint8_t* labels, int H, int W, const uint8_t pal[4][4], std::vector<uint8_t>* z, size_t* stream_bytes = nullptr) {
    // pass 1: run-length tokens (colour in the top 2 bits, run length below; 0xffffffff = start of a scan line) + counts
    uint32_t flit[4] = {0, 0, 0, 0};                          // runs per colour (each contributes its 4 literal bytes)
    uint32_t flen[65] = {0};                                  // matches of 4 m bytes, m = 1..64
    // run starts of a scan line as bit masks over 64-pixel blocks (one compare per pixel, no data-dependent branch), then one
    // token per set bit
    std::unique_ptr<uint32_t[]> tok(new uint32_t[(size_t)H * ((size_t)W + 1)]);     // (uninitialised: only the tokens written are touched)
    size_t nt = 0;
    std::vector<uint64_t> starts(((size_t)W + 63) / 64 + 1);
    for (int y = 0; y < H; ++y) {
        const uint8_t* l = labels + (size_t)y * W;
        tok[nt++] = 0xffffffffu;
        const size_t nblk = ((size_t)W + 63) / 64;
        for (size_t bl = 0; bl < nblk; ++bl) {
            const int x0 = (int)(bl * 64), nx = W - x0 < 64 ? W - x0 : 64;
            uint64_t m = 0;
            int i = 0;
#if defined(__SSE2__)
            if (x0 > 0 && nx == 64) {                         // whole block with a left neighbour: 4 x 16 pixels per compare
                const __m128i three = _mm_set1_epi8(3);
                for (; i < 64; i += 16) {
                    const __m128i cur = _mm_min_epu8(_mm_loadu_si128(reinterpret_cast<const __m128i*>(l + x0 + i)), three);
                    const __m128i prev = _mm_min_epu8(_mm_loadu_si128(reinterpret_cast<const __m128i*>(l + x0 + i - 1)), three);
                    m |= (uint64_t)(uint16_t)~_mm_movemask_epi8(_mm_cmpeq_epi8(cur, prev)) << i;
                }
            }
#endif
            for (; i < nx; ++i) {
                const int x = x0 + i;
                const uint8_t cur = l[x] > 3 ? 3 : l[x], prev = x ? (l[x - 1] > 3 ? 3 : l[x - 1]) : 255;
                m |= (uint64_t)(cur != prev) << i;
            }
            starts[bl] = m;
        }
        int run_x = 0;                                        // start of the run being measured (pixel 0 always starts one)
        uint8_t run_c = l[0] > 3 ? 3 : l[0];
        for (size_t bl = 0; bl < nblk; ++bl) {
            uint64_t m = starts[bl];
            if (bl == 0) m &= ~1ull;
            while (m) {
                const int x = (int)(bl * 64) + __builtin_ctzll(m);
                m &= m - 1;
                const int k = x - run_x;
                tok[nt++] = ((uint32_t)run_c << 30) | (uint32_t)k;
                ++flit[run_c];
                flen[64] += (uint32_t)((k - 1) >> 6);
                ++flen[(k - 1) & 63];                         // (slot 0 collects the runs without a remainder match; ignored below)
                run_x = x; run_c = l[x] > 3 ? 3 : l[x];
            }
        }
        const int k = W - run_x;
        tok[nt++] = ((uint32_t)run_c << 30) | (uint32_t)k;
        ++flit[run_c];
        flen[64] += (uint32_t)((k - 1) >> 6);
        ++flen[(k - 1) & 63];
    }
    LabelPngCode code;
    label_png_code(flit, flen, (uint32_t)H, pal, &code);
    if (stream_bytes) *stream_bytes = label_png_stream_bytes(code, flit, flen, (uint32_t)H);
    const uint64_t* cbits = code.cbits; const int* cn = code.cn;
    const uint32_t* mbits = code.mbits; const int* mn = code.mn;
    // worst case: every run costs its four literals (<= 60 bits) plus one match code (<= 21 bits) per started 64 pixels
    // (in closed form: at most nt runs, and W / 64 + 1 further match codes per scan line)
    const size_t worst_bits = 4096 + 16 * (size_t)H + 64 + (60 + 21) * nt + 21 * (size_t)H * ((size_t)W / 64 + 1);
    std::unique_ptr<uint8_t[]> buf(new uint8_t[worst_bits / 8 + 32]);
    std::memcpy(buf.get(), code.head, (code.head_bits + 7) / 8);
    BitWriter bw(buf.get() + code.head_bits / 8);             // goes on behind the block header, inside its last byte
    bw.n = (int)(code.head_bits & 7);
    bw.acc = bw.n ? code.head[code.head_bits / 8] : 0;
    // pass 2: bits + Adler-32 in closed form (per run of k pixels with byte sum S and weighted sum T = 4 p0 + 3 p1 + 2 p2 + p3:
    // b += 4 k a + 2 k (k - 1) S + k T; a += k S)
    uint64_t S[4], T[4];
    for (int c = 0; c < 4; ++c) { S[c] = pal[c][0] + pal[c][1] + pal[c][2] + pal[c][3]; T[c] = 4 * pal[c][0] + 3 * pal[c][1] + 2 * pal[c][2] + pal[c][3]; }
    // a run of k <= 64 pixels (all of them on speckled maps) leaves as ONE bit string - four literals + the match of its other
    // k - 1 pixels - when that fits the writer's 56 bits, with its Adler terms from a table
    uint64_t comb[4][65]; uint8_t comb_n[4][65];
    uint32_t adl_a[4][65], adl_b[4][65];
    for (int c = 0; c < 4; ++c) for (int k = 1; k <= 64; ++k) {
        const int n = cn[c] + mn[k - 1];
        comb_n[c][k] = (uint8_t)(n <= 56 ? n : 0);
        comb[c][k] = n <= 56 ? (cbits[c] | ((uint64_t)mbits[k - 1] << cn[c])) : 0;
        adl_a[c][k] = (uint32_t)(k * S[c]);
        adl_b[c][k] = (uint32_t)(2 * (uint64_t)k * (k - 1) * S[c] + k * T[c]);
    }
    uint64_t a = 1, b = 0;
    const uint64_t M = 65521;
    for (size_t i = 0; i < nt; ++i) {
        const uint32_t t = tok[i];
        if (t == 0xffffffffu) { bw.put(code.filt, code.filt_n); b += a; continue; }
        const int c = (int)(t >> 30);
        const uint64_t k = t & 0x3fffffffu;
        if (k <= 64 && comb_n[c][k]) {
            bw.put(comb[c][k], comb_n[c][k]);
            if ((a | b) >> 36) { a %= M; b %= M; }
            b += 4 * k * a + adl_b[c][k];
            a += adl_a[c][k];
            continue;
        }
        bw.put(cbits[c] & 0xffffffffu, cn[c] < 32 ? cn[c] : 32);
        bw.put(cbits[c] >> 32, cn[c] < 32 ? 0 : cn[c] - 32);
        uint64_t rest = k - 1;
        for (; rest >= 64; rest -= 64) bw.put(mbits[64], mn[64]);
        bw.put(mbits[rest], mn[rest]);
        // (64-bit moduli are the most expensive thing in this loop: a and b are reduced lazily - short runs add < 2^30 each)
        if (k > 256) {
            a %= M; b %= M;
            b += 4 * k * a + 2 * k * (k - 1) % M * S[c] + k * T[c];
        } else {
            if ((a | b) >> 36) { a %= M; b %= M; }
            b += 4 * k * a + 2 * k * (k - 1) * S[c] + k * T[c];
        }
        a += k * S[c];
    }
    a %= M; b %= M;
    bw.put(code.eob, code.eob_n);
    uint8_t* end = bw.finish();
    const uint32_t adler = (uint32_t)((b << 16) | a);
    *end++ = (uint8_t)(adler >> 24); *end++ = (uint8_t)(adler >> 16); *end++ = (uint8_t)(adler >> 8); *end++ = (uint8_t)adler;
    z->assign(buf.get(), end);
}

// ---- deflate for 8-bit gray channel images (red/ green/ of split_FISH_channels) -------------------------------------------
// cv2.imwrite without parameters encodes a PNG with the SUB filter, Z_BEST_SPEED and the Z_RLE strategy (OpenCV
// modules/imgcodecs/src/grfmt_png.cpp): literals plus matches of distance 1 only.  This is that coder without zlib's
// generality: every scan line is SUB-filtered (optionally of the inverted samples: cv2.bitwise_not, src/image_tools.py:143-144),
// a byte repeated four times or more becomes one literal + distance-1 matches, everything goes out as ONE dynamic-Huffman block
// built from the image's own symbol counts (two scans of the filtered bytes: count, then emit).  zlib's deflate_rle takes 16 ms
// for a 1040 x 1392 noisy FISH channel, its level-1 deflate 43 ms; any inflate reproduces the rows exactly.
void deflate_gray_sub(const uint8_t* px, int H, int W, size_t pixel_stride, size_t row_stride, bool invert, std::vector<uint8_t>* z) {
    const size_t line = (size_t)W + 1, n = (size_t)H * line;
    std::unique_ptr<uint8_t[]> f(new uint8_t[n + 8]);
    const uint8_t x = invert ? 0xff : 0x00;
    for (int y = 0; y < H; ++y) {
        uint8_t* d = f.get() + (size_t)y * line;
        const uint8_t* s = px + (size_t)y * row_stride;
        d[0] = 1;                                                           // filter type SUB
        uint8_t prev = 0;
        for (int i = 0; i < W; ++i) { const uint8_t v = (uint8_t)(s[(size_t)i * pixel_stride] ^ x); d[1 + i] = (uint8_t)(v - prev); prev = v; }
    }
    uint32_t freq[286] = {0};
    bool any_match = false;
    rle_scan(f.get(), n, [&](int t) {
        if (t >= 0) ++freq[t];
        else { ++freq[length_code(-t).sym]; any_match = true; }
    });
    GrayPngCode code;                                                       // (png_gray_code.h: the device coder builds the same)
    gray_png_code(freq, any_match, &code);
    const uint16_t* lcode = code.lcode; const uint8_t* llen = code.llen;
    const uint32_t* mbits = code.mbits; const uint8_t* mn = code.mn;
    std::unique_ptr<uint8_t[]> buf(new uint8_t[n * 2 + 4096]);             // <= 15 bits per literal
    std::memcpy(buf.get(), code.head, (code.head_bits + 7) / 8);
    BitWriter bw(buf.get() + code.head_bits / 8);                           // goes on behind the block header, inside its last byte
    bw.n = (int)(code.head_bits & 7);
    bw.acc = bw.n ? code.head[code.head_bits / 8] : 0;
    rle_scan(f.get(), n, [&](int t) {
        if (t >= 0) bw.put(lcode[t], llen[t]);
        else bw.put(mbits[-t], mn[-t]);
    });
    bw.put(lcode[256], llen[256]);
    uint8_t* end = bw.finish();
    uLong ad = adler32(0L, Z_NULL, 0);
    for (size_t off = 0; off < n; off += (1u << 30)) ad = adler32(ad, f.get() + off, (uInt)std::min<size_t>(n - off, 1u << 30));
    *end++ = (uint8_t)(ad >> 24); *end++ = (uint8_t)(ad >> 16); *end++ = (uint8_t)(ad >> 8); *end++ = (uint8_t)ad;
    z->assign(buf.get(), end);
}

int png_write_stream(const char* path, const std::vector<uint8_t>& z, int H, int W, int color_type) {
    File out(path, "wb");
    if (!out.f) return ECSEG_E_IO;
    static const uint8_t sig[8] = {0x89, 'P', 'N', 'G', '\r', '\n', 0x1a, '\n'};
    uint8_t ihdr[13];
    put_be32(ihdr, (uint32_t)W); put_be32(ihdr + 4, (uint32_t)H);
    ihdr[8] = 8; ihdr[9] = (uint8_t)color_type; ihdr[10] = 0; ihdr[11] = 0; ihdr[12] = 0;
    const bool ok = out.put(sig, 8) && png_chunk(out, "IHDR", ihdr, 13) && png_chunk(out, "IDAT", z.data(), z.size()) &&
                    png_chunk(out, "IEND", nullptr, 0);
    return ok && out.close() ? ECSEG_OK : ECSEG_E_IO;
}

// ---- .npy header (format 1.0 / 2.0 / 3.0) of a little-endian C-order 2-D integer array ---------------------------------------
struct NpyHeader { long long H = 0, W = 0; int itemsize = 0; };
int npy_parse_header(FILE* f, NpyHeader* out) {
    uint8_t pre[12];
    if (std::fread(pre, 1, 10, f) != 10 || std::memcmp(pre, "\x93NUMPY", 6) != 0) return ECSEG_E_INVALID;
    size_t hlen = 0;
    if (pre[6] == 1) hlen = (size_t)pre[8] | ((size_t)pre[9] << 8);
    else if (pre[6] == 2 || pre[6] == 3) {
        if (std::fread(pre + 10, 1, 2, f) != 2) return ECSEG_E_INVALID;
        hlen = (size_t)pre[8] | ((size_t)pre[9] << 8) | ((size_t)pre[10] << 16) | ((size_t)pre[11] << 24);
    } else return ECSEG_E_UNSUPPORTED;
    if (hlen < 16 || hlen > (1u << 20)) return ECSEG_E_INVALID;
    std::string h(hlen, '\0');
    if (std::fread(&h[0], 1, hlen, f) != hlen) return ECSEG_E_INVALID;
    auto value_after = [&](const char* key) -> size_t {                      // index just behind "'key':"
        const size_t k = h.find(key);
        if (k == std::string::npos) return std::string::npos;
        const size_t c = h.find(':', k);
        return c == std::string::npos ? c : c + 1;
    };
    size_t p = value_after("'descr'");
    if (p == std::string::npos) return ECSEG_E_INVALID;
    const size_t q0 = h.find('\'', p);
    const size_t q1 = q0 == std::string::npos ? q0 : h.find('\'', q0 + 1);
    if (q1 == std::string::npos) return ECSEG_E_INVALID;
    const std::string descr = h.substr(q0 + 1, q1 - q0 - 1);
    if (descr == "<i8" || descr == "<u8") out->itemsize = 8;
    else if (descr == "<i4" || descr == "<u4") out->itemsize = 4;
    else if (descr == "<i2" || descr == "<u2") out->itemsize = 2;
    else if (descr == "|u1" || descr == "|i1" || descr == "|b1") out->itemsize = 1;
    else return ECSEG_E_UNSUPPORTED;
    p = value_after("'fortran_order'");
    if (p == std::string::npos || h.find("False", p) == std::string::npos || h.find("False", p) > h.find(',', p)) return ECSEG_E_UNSUPPORTED;
    p = value_after("'shape'");
    if (p == std::string::npos) return ECSEG_E_INVALID;
    const size_t a = h.find('(', p), b = a == std::string::npos ? a : h.find(')', a);
    if (b == std::string::npos) return ECSEG_E_INVALID;
    long long dims[3] = {0, 0, 0};
    int nd = 0;
    for (size_t i = a + 1; i < b;) {
        while (i < b && (h[i] == ' ' || h[i] == ',')) ++i;
        if (i >= b) break;
        if (h[i] < '0' || h[i] > '9' || nd >= 3) return ECSEG_E_UNSUPPORTED;
        long long v = 0;
        while (i < b && h[i] >= '0' && h[i] <= '9') { v = v * 10 + (h[i] - '0'); if (v > (1ll << 31)) return ECSEG_E_INVALID; ++i; }
        dims[nd++] = v;
    }
    if (nd != 2 || dims[0] <= 0 || dims[1] <= 0 || dims[0] * dims[1] >= (1ll << 31)) return ECSEG_E_UNSUPPORTED;
    out->H = dims[0]; out->W = dims[1];
    return ECSEG_OK;
}

// ---- TIFF reading -----------------------------------------------------------------------------------------------
struct Reader {
    const uint8_t* b; size_t n; bool le;
    bool ok(size_t off, size_t len) const { return off <= n && len <= n - off; }
    uint32_t u16(size_t o) const { return le ? (uint32_t)b[o] | ((uint32_t)b[o + 1] << 8) : ((uint32_t)b[o] << 8) | b[o + 1]; }
    uint32_t u32(size_t o) const {
        return le ? (uint32_t)b[o] | ((uint32_t)b[o + 1] << 8) | ((uint32_t)b[o + 2] << 16) | ((uint32_t)b[o + 3] << 24)
                  : ((uint32_t)b[o] << 24) | ((uint32_t)b[o + 1] << 16) | ((uint32_t)b[o + 2] << 8) | b[o + 3];
    }
};

// values of one IFD entry (types BYTE / SHORT / LONG only) -> vector; ECSEG_E_INVALID when the entry is malformed,
// ECSEG_E_UNSUPPORTED for a structurally valid entry of another TIFF 6.0 / BigTIFF type (RATIONAL, LONG8, ...): the Python
// reader decodes those (image_io._TYPE_FMT)
int entry_values(const Reader& r, size_t e, std::vector<uint32_t>* out) {
    const uint32_t typ = r.u16(e + 2), cnt = r.u32(e + 4);
    const size_t sz = typ == 1 ? 1 : typ == 3 ? 2 : typ == 4 ? 4 : 0;
    if (sz == 0) return (typ >= 1 && typ <= 18) ? ECSEG_E_UNSUPPORTED : ECSEG_E_INVALID;
    if (cnt > (1u << 26)) return ECSEG_E_INVALID;
    size_t voff = e + 8;
    if (sz * cnt > 4) { voff = r.u32(e + 8); if (!r.ok(voff, sz * cnt)) return ECSEG_E_INVALID; }
    out->resize(cnt);
    for (uint32_t i = 0; i < cnt; ++i)
        (*out)[i] = sz == 1 ? r.b[voff + i] : sz == 2 ? r.u16(voff + 2 * i) : r.u32(voff + 4 * i);
    return ECSEG_OK;
}

}  // namespace

// ECSEG_OK, ECSEG_E_UNSUPPORTED (a valid layout this reader leaves to the Python one) or ECSEG_E_INVALID (corrupt); TiffInfo and
// the declaration are in tiff_parse.h, for the device reader's driver
int ecseg::parse_tiff(const uint8_t* buf, size_t n, TiffInfo* t, unsigned kinds) {
    const bool take_tiles = kinds & ECSEG_TIFF_TILED, take_packbits = kinds & ECSEG_TIFF_PACKBITS;
    if (n < 8) return ECSEG_E_INVALID;
    if (buf[0] == 'I' && buf[1] == 'I') t->le = true;
    else if (buf[0] == 'M' && buf[1] == 'M') t->le = false;
    else return ECSEG_E_INVALID;
    Reader r{buf, n, t->le};
    const uint32_t magic = r.u16(2);
    if (magic == 43) return ECSEG_E_UNSUPPORTED;          // BigTIFF
    if (magic != 42) return ECSEG_E_INVALID;
    const size_t ifd = r.u32(4);
    if (!r.ok(ifd, 2)) return ECSEG_E_INVALID;
    const uint32_t ne = r.u16(ifd);
    if (!r.ok(ifd + 2, (size_t)ne * 12)) return ECSEG_E_INVALID;
    bool have_w = false, have_h = false, tiled = false, have_th = false, tile_tags_ok = true;
    std::vector<uint32_t> v, tile_off, tile_cnt;
    for (uint32_t i = 0; i < ne; ++i) {
        const size_t e = ifd + 2 + (size_t)i * 12;
        const uint32_t tag = r.u16(e);
        const bool wanted = tag == 256 || tag == 257 || tag == 258 || tag == 259 || tag == 273 || tag == 277 || tag == 278 ||
                            tag == 279 || tag == 284 || tag == 317 || tag == 339 || tag == 322 || (take_tiles && tag >= 323 && tag <= 325);
        if (!wanted) continue;
        if (tag == 322) tiled = true;
        if (tag >= 322 && tag <= 325) {                      // the tile tags: read for a caller that takes tiles, and never the reason a file of strips is refused
            if (!take_tiles) continue;
            if (entry_values(r, e, &v) != ECSEG_OK || v.empty()) { tile_tags_ok = false; continue; }
            if (tag == 322) t->tw = v[0];
            else if (tag == 323) { t->th = v[0]; have_th = true; }
            else (tag == 324 ? tile_off : tile_cnt) = v;
            continue;
        }
        if (const int rc = entry_values(r, e, &v)) return rc;
        if (v.empty()) return ECSEG_E_INVALID;
        switch (tag) {
            case 256: t->W = v[0]; have_w = true; break;
            case 257: t->H = v[0]; have_h = true; break;
            case 258: t->bits = v[0]; for (uint32_t x : v) if (x != v[0]) return ECSEG_E_UNSUPPORTED; break;
            case 259: t->comp = v[0]; break;
            case 273: t->off = v; break;
            case 277: t->spp = v[0]; break;
            case 278: t->rps = v[0]; break;
            case 279: t->cnt = v; break;
            case 284: t->planar = v[0]; break;
            case 317: t->pred = v[0]; break;
            case 339: t->fmt = v[0]; for (uint32_t x : v) if (x != v[0]) return ECSEG_E_UNSUPPORTED; break;
        }
    }
    if (!have_w || !have_h || t->W == 0 || t->H == 0 || t->spp == 0 || t->W > (1u << 20) || t->H > (1u << 20) || t->spp > 16)
        return ECSEG_E_INVALID;
    if ((tiled && !take_tiles) || (t->bits != 8 && t->bits != 16) || t->fmt != 1 || (t->planar != 1 && t->spp > 1) ||
        (t->comp != 1 && t->comp != 5 && t->comp != 8 && t->comp != 32946 && !(take_packbits && t->comp == 32773)) || (t->pred != 1 && t->pred != 2))
        return ECSEG_E_UNSUPPORTED;
    if (tiled) {                                             // (take_tiles) the rule of tiff_parse.h; everything else is the Python reader's
        if (!tile_tags_ok || !have_th || t->tw == 0 || t->th == 0 || t->tw % 16 || t->th % 16 || t->tw > TIFF_TILE_MAX_EXTENT || t->th > TIFF_TILE_MAX_EXTENT ||
            !t->off.empty() || !t->cnt.empty())
            return ECSEG_E_UNSUPPORTED;
        const size_t n_tiles = (size_t)((t->H + t->th - 1) / t->th) * ((t->W + t->tw - 1) / t->tw);
        if (tile_off.size() < n_tiles || tile_cnt.size() < n_tiles) return ECSEG_E_UNSUPPORTED;
        t->off = tile_off; t->cnt = tile_cnt; t->rps = t->H;
        return ECSEG_OK;
    }
    t->tw = t->th = 0;                                       // (TileLength and the tables without TileWidth: strips)
    if (t->off.empty()) return ECSEG_E_INVALID;
    if (t->cnt.empty()) {
        if (t->off.size() != 1 || t->off[0] > n) return ECSEG_E_INVALID;
        t->cnt.assign(1, (uint32_t)(n - t->off[0]));
    }
    if (t->cnt.size() != t->off.size()) return ECSEG_E_INVALID;
    if (t->rps == 0 || t->rps > t->H) t->rps = t->H;
    return ECSEG_OK;
}

namespace {

bool read_file(const char* path, std::vector<uint8_t>* out) {
    File f(path, "rb");
    if (!f.f) return false;
    if (std::fseek(f.f, 0, SEEK_END) != 0) return false;
    const long sz = std::ftell(f.f);
    if (sz < 0 || std::fseek(f.f, 0, SEEK_SET) != 0) return false;
    out->resize((size_t)sz);
    return sz == 0 || std::fread(out->data(), 1, (size_t)sz, f.f) == (size_t)sz;
}

}  // namespace

// labels/<stem>.npy: np.save(path, labels.astype('int64')) (src/metaseg.py:53), byte for byte what numpy's format 1.0
// writer produces (header dict, padded with spaces to a multiple of 64 bytes, '\n' last).
template <typename T>
static int npy_write_as_i64(const char* path, const T* labels, int H, int W) {
    if (!path || !labels || H < 0 || W < 0) return ECSEG_E_INVALID;
    std::string hdr = "{'descr': '<i8', 'fortran_order': False, 'shape': (" + std::to_string(H) + ", " + std::to_string(W) + "), }";
    const size_t hlen = hdr.size() + 1;                                   // + '\n'
    const size_t pad = 64 - ((8 + 2 + hlen) % 64);
    hdr.append(pad, ' ');
    hdr.push_back('\n');
    const size_t npx = (size_t)H * W;
    static const uint8_t magic[8] = {0x93, 'N', 'U', 'M', 'P', 'Y', 1, 0};
    uint8_t pre[10];
    std::memcpy(pre, magic, 8);
    pre[8] = (uint8_t)(hdr.size() & 255); pre[9] = (uint8_t)(hdr.size() >> 8);
    File out(path, "wb");
    if (!out.f) return ECSEG_E_IO;
    std::setvbuf(out.f, nullptr, _IONBF, 0);                              // whole chunks go straight to write(2)
    if (!out.put(pre, 10) || !out.put(hdr.data(), hdr.size())) return ECSEG_E_IO;
    // widened 64 Ki pixels at a time into a 512-KB buffer that stays in the L2 cache (round 5: one 11.6-MB buffer per 1040 x 1392
    // image was allocated, zeroed twice and filled byte by byte before it went to the page cache - 8 of the 18 ms a
    // `make metaseg` writer thread spent per image)
    constexpr size_t CH = 1 << 16;
    std::unique_ptr<uint64_t[]> buf(new uint64_t[CH]);
    for (size_t off = 0; off < npx; off += CH) {
        const size_t k = std::min(CH, npx - off);
        for (size_t i = 0; i < k; ++i) buf[i] = (uint64_t)(int64_t)labels[off + i];   // little-endian host: the value widened to int64
        if (!out.put(buf.get(), k * 8)) return ECSEG_E_IO;
    }
    return out.close() ? ECSEG_OK : ECSEG_E_IO;
}

// The file around its strips (tiff_frame.h): the tags OpenCV 4.6 writes, in its order.
void ecseg::tiff_frame(int H, int W, int spp, int rps, const uint32_t* offs, const uint32_t* cnts, int nstrips, size_t data_end,
                       std::vector<uint8_t>* head_out, std::vector<uint8_t>* tail) {
    std::vector<uint8_t> extra;
    const size_t extra_off = data_end;
    uint32_t so = offs[0], sc = cnts[0], bps = 8;
    if (nstrips > 1) {
        so = (uint32_t)(extra_off + extra.size()); for (int s = 0; s < nstrips; ++s) put_le32(extra, offs[s]);
        sc = (uint32_t)(extra_off + extra.size()); for (int s = 0; s < nstrips; ++s) put_le32(extra, cnts[s]);
    }
    if (spp > 2) {                                           // more than two SHORTs do not fit the entry's value field
        bps = (uint32_t)(extra_off + extra.size());
        for (int c = 0; c < spp; ++c) put_le16(extra, 8);
    }
    size_t ifd_off = extra_off + extra.size();
    const bool pad = ifd_off & 1;
    ifd_off += pad;
    std::vector<uint8_t> ifd;
    auto entry = [&](uint32_t tag, uint32_t typ, uint32_t count, uint32_t value) { put_le16(ifd, tag); put_le16(ifd, typ); put_le32(ifd, count); put_le32(ifd, value); };
    put_le16(ifd, 12);
    entry(256, 4, 1, (uint32_t)W); entry(257, 4, 1, (uint32_t)H); entry(258, 3, (uint32_t)spp, bps); entry(259, 3, 1, 5);
    entry(262, 3, 1, spp == 1 ? 1 : 2); entry(273, 4, (uint32_t)nstrips, so); entry(277, 3, 1, (uint32_t)spp); entry(278, 4, 1, (uint32_t)rps);
    entry(279, 4, (uint32_t)nstrips, sc); entry(284, 3, 1, 1); entry(317, 3, 1, 2); entry(339, 3, 1, 1);
    put_le32(ifd, 0);
    std::vector<uint8_t> head = {'I', 'I'};
    put_le16(head, 42); put_le32(head, (uint32_t)ifd_off);
    *head_out = head;
    *tail = extra;
    if (pad) tail->push_back(0);
    tail->insert(tail->end(), ifd.begin(), ifd.end());
}

// The file around a PNG stream that lies at file + LABEL_PNG_Z_OFFSET already: what png_write_stream puts around it, in memory.
static void png_frame(uint8_t* file, size_t z, int H, int W, int color_type) {
    static const uint8_t sig[8] = {0x89, 'P', 'N', 'G', '\r', '\n', 0x1a, '\n'};
    auto chunk = [](uint8_t* p, const char tag[4], size_t n) {     // the data lies at p + 8 already; returns the chunk's end
        put_be32(p, (uint32_t)n);
        std::memcpy(p + 4, tag, 4);
        uLong c = crc32(0L, p + 4, 4);
        for (size_t off = 0; off < n; off += (1u << 30)) c = crc32(c, p + 8 + off, (uInt)std::min<size_t>(n - off, 1u << 30));
        put_be32(p + 8 + n, (uint32_t)c);
        return p + 12 + n;
    };
    std::memcpy(file, sig, 8);
    uint8_t* ihdr = file + 16;
    put_be32(ihdr, (uint32_t)W); put_be32(ihdr + 4, (uint32_t)H);
    ihdr[8] = 8; ihdr[9] = (uint8_t)color_type; ihdr[10] = 0; ihdr[11] = 0; ihdr[12] = 0;
    uint8_t* p = chunk(file + 8, "IHDR", 13);
    p = chunk(p, "IDAT", z);
    chunk(p, "IEND", 0);
}
void ecseg::label_png_frame(uint8_t* file, size_t z, int H, int W) { png_frame(file, z, H, W, 6); }     // (png_label_code.h)
void ecseg::gray_png_frame(uint8_t* file, size_t z, int H, int W) { png_frame(file, z, H, W, 0); }      // (png_gray_code.h)

extern "C" {

int ecseg_npy_write_i64(const char* path, const uint8_t* labels, int H, int W) { return npy_write_as_i64(path, labels, H, W); }
// <name>__segmentation_min_cut.npy (src/stat_fish.py:302): the same file from int32 values
int ecseg_npy_write_i32_as_i64(const char* path, const int32_t* labels, int H, int W) { return npy_write_as_i64(path, labels, H, W); }

// labels/<stem>.png: plt.imsave(path, I.astype('uint8'), cmap=ListedColormap(['#386cb0', '#ffff99', '#7fc97f', '#f0027f']),
// vmin=0, vmax=4) (src/metaseg.py:47-52): class k -> colour k (values above 3 clip to 3), 8-bit RGBA, filter type 0 on
// every scan line, compressed by deflate_labels above (the pixels are the contract, not the compressed bytes).
int ecseg_png_write_labels(const char* path, const uint8_t* labels, int H, int W) {
    if (!path || !labels || H <= 0 || W <= 0) return ECSEG_E_INVALID;
    if (W >= (1 << 30)) return ECSEG_E_INVALID;
    std::vector<uint8_t> z;
    deflate_labels(labels, H, W, LABEL_PNG_PALETTE, &z);
    return png_write_stream(path, z, H, W, 6);
}

// The zlib stream of that file: *stream_bytes its length as written, *formula_bytes the length label_png_stream_bytes works out
// from the token counts before a bit is written (the device coder sizes its buffers by it: the two must agree).
int ecseg_png_labels_stream_size(const uint8_t* labels, int H, int W, long long* formula_bytes, long long* stream_bytes) {
    if (!labels || !formula_bytes || !stream_bytes || H <= 0 || W <= 0 || W >= (1 << 30)) return ECSEG_E_INVALID;
    std::vector<uint8_t> z;
    size_t f = 0;
    deflate_labels(labels, H, W, LABEL_PNG_PALETTE, &z, &f);
    *formula_bytes = (long long)f; *stream_bytes = (long long)z.size();
    return ECSEG_OK;
}

// 8-bit PNG of a (H, W, channels) image, channels 1 (gray), 3 (RGB) or 4 (RGBA): the red/ green/ channel images of
// split_FISH_channels (src/image_tools.py:136-146).
int ecseg_png_write(const char* path, const uint8_t* px, int H, int W, int channels, int level) {
    if (!path || !px || H <= 0 || W <= 0 || (channels != 1 && channels != 3 && channels != 4) || level < -1 || level > 9) return ECSEG_E_INVALID;
    const size_t line = (size_t)W * channels, stride = 1 + line;
    if ((size_t)H * stride >= 0xffffffffull) return ECSEG_E_INVALID;
    std::vector<uint8_t> rows((size_t)H * stride);
    for (int y = 0; y < H; ++y) {
        uint8_t* dst = rows.data() + (size_t)y * stride;
        const uint8_t* src = px + (size_t)y * line;
        if (level >= 0) {
            dst[0] = 0;
            std::memcpy(dst + 1, src, line);
        } else {                                              // filter type 1 (SUB): byte - the byte one pixel to the left
            dst[0] = 1;
            for (size_t i = 0; i < (size_t)channels && i < line; ++i) dst[1 + i] = src[i];
            for (size_t i = channels; i < line; ++i) dst[1 + i] = (uint8_t)(src[i] - src[i - channels]);
        }
    }
    return png_write_rows(path, rows, H, W, channels == 1 ? 0 : channels == 3 ? 2 : 6, level);
}

// One channel of an interleaved 8-bit image as a gray PNG, optionally inverted, encoded as cv2.imwrite does by default (SUB
// filter + run-length deflate, deflate_gray_sub above): cv2.imwrite(red/<name>.png, cv2.bitwise_not(np.uint8(I[..., 0])))
// (src/image_tools.py:143-144) without the channel gather / inversion passes on the Python side.
int ecseg_png_write_channel(const char* path, const uint8_t* px, int H, int W, int channels, int channel, int invert) {
    if (!path || !px || H <= 0 || W <= 0 || channels <= 0 || channel < 0 || channel >= channels) return ECSEG_E_INVALID;
    if (((size_t)W + 1) * (size_t)H >= 0x7fffffffull) return ECSEG_E_INVALID;
    std::vector<uint8_t> z;
    deflate_gray_sub(px + channel, H, W, (size_t)channels, (size_t)W * channels, invert != 0, &z);
    return png_write_stream(path, z, H, W, 0);
}

// np.load(labels/<stem>.npy) + astype(uint8) (read_seg, src/utils.py:125-132; src/meta_overlay.py:59): the int64 (H, W) array that
// `make metaseg` wrote, narrowed to uint8 while it is read - 11.6 MB per 1040 x 1392 image never exist as a numpy array and the
// interpreter lock is not held.  Accepts C-order 2-D arrays of dtype <i8 / <i4 / <i2 / |u1 / |i1 / |b1 (format 1.0 - 3.0).
int ecseg_npy_label_info(const char* path, int* H, int* W) {
    if (!path || !H || !W) return ECSEG_E_INVALID;
    File in(path, "rb");
    if (!in.f) return ECSEG_E_IO;
    NpyHeader hd;
    const int rc = npy_parse_header(in.f, &hd);
    if (rc != ECSEG_OK) return rc;
    *H = (int)hd.H; *W = (int)hd.W;
    return ECSEG_OK;
}

int ecseg_npy_read_labels_u8(const char* path, uint8_t* dst, int H, int W) {
    if (!path || !dst || H <= 0 || W <= 0) return ECSEG_E_INVALID;
    File in(path, "rb");
    if (!in.f) return ECSEG_E_IO;
    NpyHeader hd;
    const int rc = npy_parse_header(in.f, &hd);
    if (rc != ECSEG_OK) return rc;
    if (hd.H != (long long)H || hd.W != (long long)W) return ECSEG_E_INVALID;
    const size_t n = (size_t)H * W;
    if (hd.itemsize == 1) return std::fread(dst, 1, n, in.f) == n ? ECSEG_OK : ECSEG_E_INVALID;
    constexpr size_t CH = 1 << 16;                                          // elements per chunk
    std::unique_ptr<uint8_t[]> buf(new uint8_t[CH * 8]);
    for (size_t off = 0; off < n; off += CH) {
        const size_t k = std::min(CH, n - off);
        if (std::fread(buf.get(), (size_t)hd.itemsize, k, in.f) != k) return ECSEG_E_INVALID;   // truncated file
        const uint8_t* s = buf.get();
        for (size_t i = 0; i < k; ++i) dst[off + i] = s[i * (size_t)hd.itemsize];              // little-endian: the low byte
    }
    return ECSEG_OK;
}

// cv2.imwrite of an 8-bit image with `spp` interleaved samples per pixel (1: gray, 3: RGB): LZW + horizontal predictor (per
// sample: a byte minus the byte `spp` to its left), strips of 8192 / (W * spp) rows.
static int tiff_write_u8(const char* path, const uint8_t* img, int H, int W, int spp, int invert) {
    if (!path || !img || H <= 0 || W <= 0 || (long long)W * spp >= (1ll << 30)) return ECSEG_E_INVALID;
    const size_t line = (size_t)W * spp;
    const int rps = ecseg::tiff_rows_per_strip(H, W, spp);
    const int nstrips = (H + rps - 1) / rps;
    std::vector<uint8_t> diff((size_t)rps * line), enc(ecseg::tiff_strip_bound((size_t)rps * line)), data;
    std::vector<uint32_t> offs(nstrips), cnts(nstrips);
    data.reserve((size_t)H * line / 2 + 4096);
    const uint8_t flip = invert ? 0xff : 0;
    size_t pos = 8;
    for (int s = 0; s < nstrips; ++s) {
        const int r0 = s * rps, rows = r0 + rps <= H ? rps : H - r0;
        for (int y = 0; y < rows; ++y) {
            const uint8_t* src = img + (size_t)(r0 + y) * line;
            uint8_t* d = diff.data() + (size_t)y * line;
            for (size_t x = 0; x < (size_t)spp; ++x) d[x] = src[x] ^ flip;
            for (size_t x = spp; x < line; ++x) d[x] = (uint8_t)((src[x] ^ flip) - (src[x - spp] ^ flip));   // horizontal differencing (mod 256)
        }
        const long long m = ecseg_lzw_encode(diff.data(), (long long)rows * (long long)line, enc.data(), (long long)enc.size());
        if (m < 0) return ECSEG_E_INVALID;
        if (pos + (size_t)m + 1 >= 0xffffffffull) return ECSEG_E_INVALID;   // classic TIFF: 32-bit offsets
        offs[s] = (uint32_t)pos; cnts[s] = (uint32_t)m;
        data.insert(data.end(), enc.begin(), enc.begin() + m);
        if (m & 1) data.push_back(0);
        pos += (size_t)m + (m & 1);
    }
    std::vector<uint8_t> head, tail;
    ecseg::tiff_frame(H, W, spp, rps, offs.data(), cnts.data(), nstrips, pos, &head, &tail);
    File out(path, "wb");
    if (!out.f) return ECSEG_E_IO;
    const bool ok = out.put(head.data(), head.size()) && out.put(data.data(), data.size()) && out.put(tail.data(), tail.size());
    return ok && out.close() ? ECSEG_OK : ECSEG_E_IO;
}

// dapi/<name>.tif: cv2.imwrite of an 8-bit gray image (src/utils.py:122-123): LZW + horizontal predictor, strips of
// 8192 / width rows (the tags OpenCV 4.6 wrote into example_ecSeg/dapi.jpeg's sibling files).  invert != 0 writes 255 - img
// (the caller holds the pre-processed image, the file holds cv2.bitwise_not of it: src/utils.py:112).
int ecseg_tiff_write_gray8(const char* path, const uint8_t* img, int H, int W, int invert) {
    return tiff_write_u8(path, img, H, W, 1, invert);
}

// The colour files of stat_fish (src/stat_fish.py:306-308): the same writer with three samples per pixel, stored as given.
int ecseg_tiff_write_rgb8(const char* path, const uint8_t* img, int H, int W) {
    return tiff_write_u8(path, img, H, W, 3, 0);
}

// imread of a baseline TIFF (src/utils.py:110): first image of the file; strips; 8 / 16-bit unsigned samples, gray or
// interleaved RGB(A); uncompressed, LZW or Deflate; horizontal predictor; either byte order.  ecseg_tiff_info reports the
// shape (ECSEG_E_UNSUPPORTED: a valid file this reader leaves to the Python reader; ECSEG_E_INVALID: not a TIFF / corrupt;
// ECSEG_E_IO: cannot be opened), ecseg_tiff_read decodes into dst as native-endian samples, (H, W, spp) row-major; strips
// that end early are zero-filled, as the Python reader does.
int ecseg_tiff_info(const char* path, int* H, int* W, int* spp, int* bits) {
    if (!path || !H || !W || !spp || !bits) return ECSEG_E_INVALID;
    std::vector<uint8_t> buf;
    if (!read_file(path, &buf)) return ECSEG_E_IO;
    TiffInfo t;
    const int rc = parse_tiff(buf.data(), buf.size(), &t);
    if (rc != ECSEG_OK) return rc;
    *H = (int)t.H; *W = (int)t.W; *spp = (int)t.spp; *bits = (int)t.bits;
    return ECSEG_OK;
}

int ecseg_tiff_read(const char* path, void* dst, long long dst_bytes) {
    if (!path || !dst || dst_bytes < 0) return ECSEG_E_INVALID;
    std::vector<uint8_t> buf;
    if (!read_file(path, &buf)) return ECSEG_E_IO;
    TiffInfo t;
    const int rc = parse_tiff(buf.data(), buf.size(), &t);
    if (rc != ECSEG_OK) return rc;
    const size_t bpp = t.bits / 8, line = (size_t)t.W * t.spp * bpp, total = line * t.H;
    if ((unsigned long long)dst_bytes < total) return ECSEG_E_INVALID;
    uint8_t* out = static_cast<uint8_t*>(dst);
    for (size_t k = 0; k < t.off.size(); ++k) {
        const size_t r0 = k * (size_t)t.rps;
        if (r0 >= t.H) break;
        const size_t rows = r0 + t.rps <= t.H ? t.rps : t.H - r0, want = rows * line;
        uint8_t* d = out + r0 * line;
        if (t.off[k] > buf.size()) return ECSEG_E_INVALID;
        const size_t have = std::min<size_t>(t.cnt[k], buf.size() - t.off[k]);
        const uint8_t* src = buf.data() + t.off[k];
        size_t got = 0;
        if (t.comp == 1) {
            got = std::min(have, want);
            std::memcpy(d, src, got);
        } else if (t.comp == 5) {
            const long long m = ecseg_lzw_decode(src, (long long)have, d, (long long)want);
            if (m < 0) return ECSEG_E_INVALID;
            got = (size_t)m;
        } else {
            uLongf cap = (uLongf)want;
            const int z = uncompress(d, &cap, src, (uLong)have);
            if (z != Z_OK && z != Z_BUF_ERROR) return ECSEG_E_INVALID;
            got = z == Z_OK ? (size_t)cap : 0;
            if (z == Z_BUF_ERROR) {                                   // more data than the strip holds: keep what fits
                z_stream zs; std::memset(&zs, 0, sizeof zs);
                if (inflateInit(&zs) != Z_OK) return ECSEG_E_INVALID;
                zs.next_in = const_cast<Bytef*>(src); zs.avail_in = (uInt)have; zs.next_out = d; zs.avail_out = (uInt)want;
                const int zr = inflate(&zs, Z_FINISH);
                got = want - zs.avail_out;
                inflateEnd(&zs);
                if (zr != Z_STREAM_END && zr != Z_BUF_ERROR && zr != Z_OK) return ECSEG_E_INVALID;
            }
        }
        if (got < want) std::memset(d + got, 0, want - got);
        // samples to native (little-endian) order, then undo the horizontal predictor per sample channel
        if (bpp == 2) {
            uint16_t* p = reinterpret_cast<uint16_t*>(d);
            const size_t ns = rows * (size_t)t.W * t.spp;
            if (!t.le) for (size_t i = 0; i < ns; ++i) p[i] = (uint16_t)((p[i] << 8) | (p[i] >> 8));
            if (t.pred == 2)
                for (size_t y = 0; y < rows; ++y) {
                    uint16_t* q = p + y * (size_t)t.W * t.spp;
                    for (size_t i = t.spp; i < (size_t)t.W * t.spp; ++i) q[i] = (uint16_t)(q[i] + q[i - t.spp]);
                }
        } else if (t.pred == 2) {
            for (size_t y = 0; y < rows; ++y) {
                uint8_t* q = d + y * line;
                for (size_t i = t.spp; i < line; ++i) q[i] = (uint8_t)(q[i] + q[i - t.spp]);
            }
        }
    }
    const size_t covered = std::min<size_t>(t.off.size() * (size_t)t.rps, t.H);
    if (covered < t.H) std::memset(out + covered * line, 0, (t.H - covered) * line);
    return ECSEG_OK;
}

}  // extern "C"
