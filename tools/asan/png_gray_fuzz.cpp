// AddressSanitizer / UBSan driver for the device gray PNG coder (ecseg_png_channel_encode): the per-block pieces its kernels are
// written with (csrc/png_gray_tokens.h) and the host parts of the code (csrc/png_gray_code.h) compiled for the host, where the 64
// lanes are a loop and the spans (waves) come in any order.  CPU build only (`make asan_png_gray`).
//   Every case is an interleaved image, a channel and the inversion.  The program walks the filtered stream as the four kernels do -
// count, host code build, span bits, scan, emit with OR into a zeroed dword buffer of exactly the stream's size - and checks, against
// rle_scan on the whole stream and against the file ecseg_png_write_channel (csrc/host_io.cpp) writes: every filtered byte, the token
// sequence, the 286 counts, the bit total and the stream size the counts give before a bit is written, the Adler-32 appended span by
// span, and the stream byte for byte.  Spans of 64, 128 and 1024 bytes are walked, backwards, so nothing rests on their order.
//   Cases: the hand cases of tests/png_gray_cases.py's kinds (ramps whose one run hits each branch of the match split, zeros, runs of
// 1..5 and 259..262 bytes across block and scan-line borders, noise without a run of four) and seeded streams of geometric runs.
#include <unistd.h>

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../ecseg_amd/csrc/png_gray_code.h"
#include "../../ecseg_amd/csrc/png_gray_tokens.h"

extern "C" int ecseg_png_write_channel(const char* path, const uint8_t* px, int H, int W, int channels, int channel, int invert);

using namespace ecseg;

static uint64_t s = 0x9e3779b97f4a7c15ull;
static uint32_t rnd() { s ^= s << 13; s ^= s >> 7; s ^= s << 17; return (uint32_t)(s >> 11); }

#define CHECK(c, ...) do { if (!(c)) { std::fprintf(stderr, "%s: ", name.c_str()); std::fprintf(stderr, __VA_ARGS__); std::fprintf(stderr, "\n"); std::exit(1); } } while (0)

struct Image { int H, W, C; std::vector<uint8_t> px; };

// an image whose channel `ch`, inverted or not, has the filtered stream f (n = H (W + 1) bytes; the filter bytes are forced to 1)
static Image image_of_stream(std::vector<uint8_t>& f, int H, int W, int C, int ch, int invert) {
    Image im{H, W, C, std::vector<uint8_t>((size_t)H * W * C)};
    for (auto& v : im.px) v = (uint8_t)rnd();
    for (int y = 0; y < H; ++y) {
        f[(size_t)y * (W + 1)] = 1;
        uint8_t v = 0;
        for (int x = 0; x < W; ++x) {
            v = (uint8_t)(v + f[(size_t)y * (W + 1) + 1 + x]);
            im.px[((size_t)y * W + x) * C + ch] = (uint8_t)(v ^ (invert ? 0xff : 0));
        }
    }
    return im;
}

static void or_bits(std::vector<uint32_t>& z, uint64_t pos, uint64_t bits, uint32_t n) {      // put_bits (csrc/png_device.h), in order
    for (uint32_t k = 0; k < n; ++k)
        if ((bits >> k) & 1) z.at((size_t)((pos + k) >> 5)) |= 1u << ((pos + k) & 31);
}

static std::vector<uint8_t> read_file(const char* path) {
    std::vector<uint8_t> d;
    FILE* f = std::fopen(path, "rb");
    if (!f) return d;
    uint8_t buf[65536];
    for (size_t k; (k = std::fread(buf, 1, sizeof buf, f)) > 0;) d.insert(d.end(), buf, buf + k);
    std::fclose(f);
    return d;
}

static void run_case(const std::string& name, const Image& im, int ch, int invert, const char* tmp) {
    const int H = im.H, W = im.W, C = im.C;
    const uint32_t n = (uint32_t)H * (uint32_t)(W + 1), flip = invert ? 255u : 0u;
    const uint8_t* px = im.px.data() + ch;
    const size_t row_stride = (size_t)W * C;
    // the filtered stream as deflate_gray_sub builds it, and byte by byte as the kernels read it
    std::vector<uint8_t> f(n);
    for (int y = 0; y < H; ++y) {
        f[(size_t)y * (W + 1)] = 1;
        uint8_t prev = 0;
        for (int x = 0; x < W; ++x) { const uint8_t v = (uint8_t)(im.px[((size_t)y * W + x) * C + ch] ^ flip); f[(size_t)y * (W + 1) + 1 + x] = (uint8_t)(v - prev); prev = v; }
    }
    for (uint32_t i = 0; i < n; ++i) CHECK(gray_stream_byte(px, (uint32_t)W, (uint32_t)C, row_stride, flip, i) == f[i], "stream byte %u", i);
    // the reference: rle_scan on the whole stream
    std::vector<int> want;
    uint32_t wfreq[286] = {0};
    bool wany = false;
    rle_scan(f.data(), n, [&](int t) { want.push_back(t); if (t >= 0) ++wfreq[t]; else { ++wfreq[length_code(-t).sym]; wany = true; } });
    uint32_t ad_a = 1, ad_b = 0;
    for (uint32_t i = 0; i < n; ++i) { ad_a = (ad_a + f[i]) % 65521; ad_b = (ad_b + ad_a) % 65521; }
    // the file of the host writer
    CHECK(ecseg_png_write_channel(tmp, im.px.data(), H, W, C, ch, invert) == 0, "host writer failed");
    const std::vector<uint8_t> file = read_file(tmp);
    CHECK(file.size() > 57 + 6, "host file too short");
    const std::vector<uint8_t> zref(file.begin() + 41, file.end() - 16);

    for (uint32_t span_len : {64u, 128u, 1024u}) {
        const uint32_t n_spans = (n + span_len - 1) / span_len;
        auto byte = [&](uint32_t i) -> uint32_t { return i < n ? f[i] : 256u; };
        auto step_starts = [&](uint32_t i0) {
            unsigned long long m = 0;
            for (int l = 0; l < 64; ++l) { const uint32_t i = i0 + l; if (i < n && (i == 0 || f[i] != f[i - 1])) m |= 1ull << l; }
            return m;
        };
        // count: per span its carry, the counts of the runs that end in it, its Adler terms
        std::vector<uint32_t> carry_of(n_spans);
        std::vector<GrayAdler> terms(n_spans);
        struct Run { uint32_t pos; GrayTokens t; std::vector<int> seq; };        // a run, by the position that owns it
        std::vector<std::vector<Run>> toks(n_spans);
        uint32_t freq[287] = {0};
        for (uint32_t sp = n_spans; sp-- > 0;) {
            const uint32_t g = sp * span_len, len = std::min(span_len, n - g);
            uint32_t carry = 0;
            if (g > 0) {                                      // start_before: 64 positions per turn, backwards
                for (uint32_t hi = g;;) {
                    const uint32_t i0 = hi >= 64 ? hi - 64 : 0u;
                    unsigned long long m = step_starts(i0);
                    if (hi - i0 < 64) m &= (1ull << (hi - i0)) - 1;
                    if (m) { carry = gray_carry_out(m, i0, 0u); break; }
                    hi = i0;
                }
            }
            carry_of[sp] = carry;
            uint64_t sa = 0, sb = 0;
            for (uint32_t i0 = g; i0 < g + len; i0 += 64) {
                const unsigned long long starts = step_starts(i0);
                for (int l = 0; l < 64; ++l) {
                    const uint32_t i = i0 + l;
                    if (i >= n) break;
                    sa += f[i]; sb += (uint64_t)(g + len - i) * f[i];
                    if (byte(i) == byte(i + 1)) continue;
                    const uint32_t R = i - gray_run_start(starts, l, i0, carry) + 1;
                    const GrayTokens t = gray_run_tokens(R);
                    freq[f[i]] += t.lits;
                    if (t.n258) freq[285] += t.n258;
                    if (t.m1) ++freq[gray_len_sym(t.m1)];
                    if (t.m2) ++freq[gray_len_sym(t.m2)];
                    if (t.n258 | t.m1) ++freq[286];
                    std::vector<int> seq;
                    for (uint32_t k = 0; k < t.lits; ++k) seq.push_back(f[i]);
                    for (uint32_t k = 0; k < t.n258; ++k) seq.push_back(-258);
                    if (t.m1) seq.push_back(-(int)t.m1);
                    if (t.m2) seq.push_back(-(int)t.m2);
                    toks[sp].push_back(Run{i, t, seq});
                }
                carry = gray_carry_out(starts, i0, carry);
            }
            terms[sp] = GrayAdler{(uint32_t)(sa % 65521), (uint32_t)(sb % 65521)};
        }
        std::vector<int> got;
        for (auto& sp : toks) for (auto& r : sp) got.insert(got.end(), r.seq.begin(), r.seq.end());
        CHECK(got == want, "span %u: token sequence differs (%zu tokens, rle_scan has %zu)", span_len, got.size(), want.size());
        for (int k = 0; k < 286; ++k) CHECK(freq[k] == wfreq[k], "span %u: count of symbol %d: %u, rle_scan has %u", span_len, k, freq[k], wfreq[k]);
        CHECK((freq[286] != 0) == wany, "span %u: any_match", span_len);
        // host step
        GrayPngCode code;
        gray_png_code(freq, freq[286] != 0, &code);
        const size_t zb = gray_png_stream_bytes(code, freq);
        CHECK(zb == zref.size(), "span %u: the counts give %zu bytes, the host writer wrote %zu", span_len, zb, zref.size());
        CHECK(zb <= gray_png_stream_bound(n) && gray_png_stream_bound(n) <= 2 * (size_t)n + 4096, "span %u: bound", span_len);
        // span bits, scan
        std::vector<uint64_t> off(n_spans);
        uint64_t pos = code.head_bits;
        GrayAdler ad{1u, 0u};
        for (uint32_t sp = 0; sp < n_spans; ++sp) {
            off[sp] = pos;
            for (auto& r : toks[sp]) {
                pos += gray_run_bits(r.t, code.llen[f[r.pos]], [&](uint32_t L) { return (uint32_t)code.mn[L]; });
            }
            ad = gray_adler_append(ad, terms[sp], std::min(span_len, n - sp * span_len));
        }
        CHECK(ad.a == ad_a && ad.b == ad_b, "span %u: Adler-32 %04x%04x, the stream has %04x%04x", span_len, ad.b, ad.a, ad_b, ad_a);
        CHECK((pos + code.llen[256] + 7) / 8 + 4 == zb, "span %u: bit total %llu", span_len, (unsigned long long)pos);
        // emit, spans backwards, into exactly the stream's dwords
        std::vector<uint32_t> z((zb + 3) / 4, 0u);
        for (uint32_t w = 0; w * 32 < code.head_bits; ++w) { uint32_t v; std::memcpy(&v, code.head + 4 * w, 4); or_bits(z, 32ull * w, v, 32); }
        for (uint32_t sp = n_spans; sp-- > 0;) {
            uint64_t p = off[sp];
            for (auto& r : toks[sp])
                for (int t : r.seq) {
                    if (t >= 0) { or_bits(z, p, code.lcode[t], code.llen[t]); p += code.llen[t]; }
                    else { or_bits(z, p, code.mbits[-t], code.mn[-t]); p += code.mn[-t]; }
                }
        }
        or_bits(z, pos, code.lcode[256], code.llen[256]);
        const uint64_t nb = (pos + code.llen[256] + 7) / 8;
        const uint32_t adler = ad.b << 16 | ad.a;
        or_bits(z, nb * 8, __builtin_bswap32(adler), 32);
        CHECK(std::memcmp(z.data(), zref.data(), zb) == 0, "span %u: the stream differs from the host writer's", span_len);
    }
}

int main() {
    char tmp[] = "/tmp/ecseg_png_gray_XXXXXX";
    const int fd = mkstemp(tmp);
    if (fd < 0) { std::perror("mkstemp"); return 1; }
    close(fd);
    int cases = 0;
    std::string name = "tables";
    for (int L = 3; L <= 258; ++L) CHECK(gray_len_sym((uint32_t)L) == length_code(L).sym, "length %d", L);
    for (uint32_t R = 1; R < 2000; ++R) {                     // the closed form against rle_scan's loop on one run
        std::vector<uint8_t> f(R, 7);
        std::vector<int> want, got;
        rle_scan(f.data(), R, [&](int t) { want.push_back(t); });
        const GrayTokens t = gray_run_tokens(R);
        for (uint32_t k = 0; k < t.lits; ++k) got.push_back(7);
        for (uint32_t k = 0; k < t.n258; ++k) got.push_back(-258);
        if (t.m1) got.push_back(-(int)t.m1);
        if (t.m2) got.push_back(-(int)t.m2);
        CHECK(got == want, "run of %u", R);
    }
    const int extents[][2] = {{1, 1}, {1, 2}, {3, 62}, {3, 63}, {3, 64}, {5, 127}, {4, 128}, {2, 300}, {33, 200}, {70, 255},
                              {7, 36}, {4, 64}, {9, 28}, {2, 130}, {11, 46}, {7, 73}};
    for (auto& e : extents) {
        const int H = e[0], W = e[1];
        const size_t n = (size_t)H * (W + 1);
        for (int kind = 0; kind < 5; ++kind) {
            const int C = 1 + (int)(rnd() % 4), ch = (int)(rnd() % C), inv = (int)(rnd() & 1);
            std::vector<uint8_t> f(n);
            if (kind == 0) std::fill(f.begin(), f.end(), 1);                    // ramp rows: one run of n bytes
            else if (kind == 1) std::fill(f.begin(), f.end(), 0);               // a flat image
            else if (kind == 2) for (auto& v : f) v = (uint8_t)rnd();           // noise
            else {                                                              // geometric runs over a small alphabet (1 is common: runs cross lines)
                for (size_t i = 0; i < n;) {
                    size_t R = 1;
                    const uint32_t pick = rnd() % 8;
                    if (pick == 0) R = 255 + rnd() % 12; else if (pick < 4) R = 1 + rnd() % 6; else while (rnd() % (kind == 3 ? 2 : 16)) ++R;
                    const uint8_t v = (uint8_t)(rnd() % 3);
                    for (; R > 0 && i < n; --R) f[i++] = v;
                }
            }
            name = "extent " + std::to_string(H) + "x" + std::to_string(W) + " kind " + std::to_string(kind);
            run_case(name, image_of_stream(f, H, W, C, ch, inv), ch, inv, tmp);
            ++cases;
        }
    }
    // runs of 1..5 and 259..262 bytes that start on, end on and straddle a 64-byte step border, a 1024-byte span border and a scan-line
    // end (tests/png_gray_cases.py places the same): a run that covers a filter byte is a run of ones, any other a run of fives
    {
        const int H = 4, W = 1299, C = 3;
        const size_t n = (size_t)H * (W + 1), line = W + 1;
        static const int lens[] = {1, 2, 3, 4, 5, 259, 260, 261, 262};
        static const size_t borders[] = {64 * 9, 1024, 2 * 1300};
        for (int R : lens) for (size_t border : borders) for (int placement = 0; placement < 3; ++placement) {
            if (placement == 2 && R < 2) continue;
            const size_t at = placement == 0 ? border : placement == 1 ? border - R : border - R / 2;
            std::vector<uint8_t> f(n);
            for (size_t i = 0; i < n; ++i) f[i] = (uint8_t)(2 + (i & 1));
            const uint8_t v = (at + R - 1) / line != (at - 1) / line ? 1 : 5;
            for (size_t i = at; i < at + (size_t)R; ++i) f[i] = v;
            name = "placed run " + std::to_string(R) + " at " + std::to_string(at) + " (border " + std::to_string(border) + ")";
            run_case(name, image_of_stream(f, H, W, C, R % 3, R & 1), R % 3, R & 1, tmp);
            ++cases;
        }
    }
    unlink(tmp);
    std::printf("png_gray_fuzz: %d cases, spans of 64 / 128 / 1024 bytes: ok\n", cases);
    return 0;
}
