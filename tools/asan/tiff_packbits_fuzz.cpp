// AddressSanitizer / UBSan driver for the device TIFF reader's PackBits strip routine (csrc/tiff_packbits_strip.h, the body of
// tiffb_packbits_kernel) compiled for the host: the 64 lanes are a loop, the read of lane 0 and the barrier do nothing.  CPU build
// only (`make asan_tiff_packbits`).  Every stream is decoded by the routine and by `rule` below, a plain byte loop that restates
// image_io._packbits_decode(data, expected) line by line: every byte of the strip must agree (zero fill included), and the status is
// 0 for every stream, as that function raises for none.  Source and destination are heap blocks of exactly `have` and `want` bytes,
// so a read or write outside them is the sanitizer's finding.
//   Seeded streams of four classes: valid (an encoder's output for noisy, flat and mixed data, no-op headers sprinkled in),
// truncated (a valid stream cut anywhere: inside a literal run, behind a repeat header, behind a header), overlong (a valid stream
// for more bytes than the strip holds, so that a run passes the strip's end, and valid streams with bytes left over) and random
// bytes; streams longer than the TP_IN staged bytes are among each.  Prints the count of every class and stops at the first difference.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <memory>
#include <string>
#include <vector>

#include "../../ecseg_amd/csrc/tiff_packbits_strip.h"

static uint64_t s = 0x9e3779b97f4a7c15ull;
static uint32_t rnd() { s ^= s << 13; s ^= s >> 7; s ^= s << 17; return (uint32_t)(s >> 11); }

static ecseg::TpLds lds;
static std::map<std::string, long long> classes;

// image_io._packbits_decode: out grows until it has `want` bytes or the stream ends; then it is cut to `want` and padded with zeros.
static void rule(const uint8_t* src, size_t have, uint8_t* dst, size_t want) {
    std::vector<uint8_t> out;
    size_t i = 0;
    while (i < have && out.size() < want) {
        const unsigned h = src[i++];
        if (h < 128) {
            for (size_t k = 0; k < h + 1u && i + k < have; ++k) out.push_back(src[i + k]);      // data[i:i + h + 1]
            i += h + 1u;
        } else if (h > 128) {
            if (i < have) out.insert(out.end(), 257u - h, src[i]);                              // data[i:i + 1] * (257 - h)
            i += 1;
        }
    }
    for (size_t k = 0; k < want; ++k) dst[k] = k < out.size() ? out[k] : (uint8_t)0;
}

// A PackBits stream of `raw`: repeat runs of 2 (sometimes 3) or more equal bytes, literal runs between; `noops`: 0x80 headers at
// random places between runs.
static std::vector<uint8_t> encode(const std::vector<uint8_t>& raw, bool noops) {
    std::vector<uint8_t> out;
    const unsigned min_run = 2 + rnd() % 2;
    size_t i = 0;
    while (i < raw.size()) {
        if (noops && rnd() % 7 == 0) out.push_back(0x80);
        size_t run = 1;
        while (i + run < raw.size() && run < 128 && raw[i + run] == raw[i]) ++run;
        if (run >= min_run) {
            out.push_back((uint8_t)(257 - run));
            out.push_back(raw[i]);
            i += run;
            continue;
        }
        size_t lit = 0;                                      // literal bytes up to the next run of min_run
        while (i + lit < raw.size() && lit < 128) {
            size_t r = 1;
            while (i + lit + r < raw.size() && r < min_run && raw[i + lit + r] == raw[i + lit]) ++r;
            if (r >= min_run) break;
            ++lit;
        }
        if (lit == 0) lit = 1;
        out.push_back((uint8_t)(lit - 1));
        out.insert(out.end(), raw.begin() + (long)i, raw.begin() + (long)(i + lit));
        i += lit;
    }
    return out;
}

static std::vector<uint8_t> samples(size_t n) {
    std::vector<uint8_t> raw(n);
    const unsigned kind = rnd() % 4;                         // noise, flat, long runs with noise between, a two-valued image
    uint8_t v = (uint8_t)rnd();
    for (size_t k = 0; k < n; ++k) {
        if (kind == 0) v = (uint8_t)rnd();
        else if (kind == 2) { if (rnd() % 40 == 0) v = (uint8_t)rnd(); else if (rnd() % 9 == 0) v = (uint8_t)(v + 1); }
        else if (kind == 3) { if (rnd() % 5 == 0) v ^= 0xff; }
        raw[k] = v;
    }
    return raw;
}

static bool check(const std::string& cls, const std::vector<uint8_t>& stream, size_t want) {
    const size_t have = stream.size();
    std::unique_ptr<uint8_t[]> src(new uint8_t[have]), a(new uint8_t[want]), b(new uint8_t[want]);   // exactly have / want bytes
    if (have) std::memcpy(src.get(), stream.data(), have);
    std::memset(a.get(), 0xcd, want);
    rule(src.get(), have, b.get(), want);
    const uint32_t st = ecseg::tp_packbits_strip(src.get(), (uint32_t)have, a.get(), (uint32_t)want, lds);
    ++classes[cls];
    if (st != 0) { std::printf("%s: status %u for a stream of %zu bytes into %zu\n", cls.c_str(), st, have, want); return false; }
    for (size_t k = 0; k < want; ++k)
        if (a[k] != b[k]) {
            std::printf("%s: byte %zu of %zu is %u, the rule says %u (stream of %zu bytes)\n", cls.c_str(), k, want, a[k], b[k], have);
            return false;
        }
    return true;
}

int main() {
    // by hand: the empty stream; a lone header of each kind; 128 literals; a repeat of 128; a no-op between runs
    const std::vector<std::pair<std::vector<uint8_t>, size_t>> hand = {
        {{}, 5}, {{0x00}, 3}, {{0x80}, 3}, {{0x81}, 3}, {{0xff, 7}, 2}, {{0xff, 7}, 1}, {{0x81, 9}, 128}, {{0x81, 9}, 200}, {{0x81, 9}, 100},
        {{0x02, 1, 2, 3, 0x80, 0xfe, 5, 0x80, 0x00, 9}, 7}, {{0x05, 1, 2}, 6}, {{0x01, 1, 2, 0x7f}, 2}, {{0x01, 1, 2, 0x33, 0x44}, 2}};
    for (const auto& h : hand) if (!check("by hand", h.first, h.second)) return 1;
    std::vector<uint8_t> lit128(129, 0x7f);
    for (size_t k = 1; k < 129; ++k) lit128[k] = (uint8_t)k;
    if (!check("by hand", lit128, 128) || !check("by hand", lit128, 127) || !check("by hand", lit128, 300)) return 1;
    for (int round = 0; round < 6000; ++round) {
        const size_t want = 1 + (rnd() % 8 == 0 ? rnd() % 9000 : rnd() % 700);
        const std::vector<uint8_t> raw = samples(want);
        const std::vector<uint8_t> ok = encode(raw, rnd() % 3 == 0);
        if (!check("valid", ok, want)) return 1;
        {
            std::unique_ptr<uint8_t[]> got(new uint8_t[want]);
            rule(ok.data(), ok.size(), got.get(), want);
            if (std::memcmp(got.get(), raw.data(), want)) { std::printf("the encoder and the rule disagree\n"); return 1; }
        }
        std::vector<uint8_t> cut(ok.begin(), ok.begin() + (long)(rnd() % (ok.size() + 1)));
        if (!check("truncated", cut, want)) return 1;
        if (ok.size() > 1) { cut.assign(ok.begin(), ok.end() - 1); if (!check("truncated by one byte", cut, want)) return 1; }
        if (!check("overlong: a run passes the strip's end", ok, 1 + rnd() % want)) return 1;
        std::vector<uint8_t> more = ok;
        for (unsigned k = 1 + rnd() % 300; k; --k) more.push_back((uint8_t)rnd());
        if (!check("overlong: bytes left over", more, want)) return 1;
        std::vector<uint8_t> junk(rnd() % 2500);
        for (uint8_t& v : junk) v = (uint8_t)rnd();
        if (!check("random bytes", junk, want)) return 1;
    }
    for (const auto& c : classes) std::printf("%8lld  %s\n", c.second, c.first.c_str());
    std::printf("tiff_packbits_fuzz ok\n");
    return 0;
}
