// AddressSanitizer / UBSan driver for the device TIFF reader's per-strip routine (csrc/tiff_decode_strip.h, the body of
// tiffb_unstrip_kernel for an LZW strip) compiled for the host: the 64 lanes are a loop, the read of lane 0 and the store fence do nothing.  CPU
// build only (`make asan_tiff_decode`).  Every stream is decoded by the routine and by ecseg_lzw_decode (csrc/host_codec.cpp), its
// specification: the status must agree, and where it is OK every byte of the strip (zero fill included).  Source and destination
// are heap blocks of exactly `have` and `want` bytes, so a read or write outside them is the sanitizer's finding.
//   tiff_decode_fuzz [corpus]    corpus: records { uint32 have, uint32 want (little-endian), have bytes }, the strips of the files of
//                                tests/tiff_decode_cases.py; without it only the built-in streams run.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

#include "../../ecseg_amd/csrc/tiff_decode_strip.h"

extern "C" long long ecseg_lzw_decode(const uint8_t* src, long long n, uint8_t* dst, long long dst_cap);
extern "C" long long ecseg_lzw_encode(const uint8_t* src, long long n, uint8_t* dst, long long dst_cap);

static uint64_t s = 0x2545f4914f6cdd1dull;
static uint32_t rnd() { s ^= s << 13; s ^= s >> 7; s ^= s << 17; return (uint32_t)(s >> 11); }

static ecseg::TdLds lds;
static long long n_ok = 0, n_corrupt = 0;

// -> false (and a message) when the routine and the host decoder disagree
static bool same(const uint8_t* stream, size_t have, size_t want, const char* what, long long index) {
    std::unique_ptr<uint8_t[]> src(new uint8_t[have]), got(new uint8_t[want]), ref(new uint8_t[want + 1]);
    std::memcpy(src.get(), stream, have);
    std::memset(got.get(), 0xAB, want);
    std::memset(lds.pos, 0xCD, sizeof lds.pos);              // (stale entries of an earlier strip: never read)
    std::memset(lds.len, 0xCD, sizeof lds.len);
    const long long r = ecseg_lzw_decode(src.get(), (long long)have, ref.get(), (long long)want);
    const uint32_t st = ecseg::td_lzw_strip(src.get(), (uint32_t)have, got.get(), (uint32_t)want, lds);
    if ((r < 0) != (st != 0)) { std::printf("%s %lld: host returns %lld, the routine status %u\n", what, index, r, st); return false; }
    if (r < 0) { ++n_corrupt; return true; }
    std::memset(ref.get() + r, 0, want - (size_t)r);
    if (std::memcmp(got.get(), ref.get(), want) != 0) {
        size_t at = 0;
        while (got[at] == ref[at]) ++at;
        std::printf("%s %lld: byte %zu of %zu differs (host gave %lld bytes)\n", what, index, at, want, r);
        return false;
    }
    ++n_ok;
    return true;
}

int main(int argc, char** argv) {
    // ---- built-in: round trips of structured / random buffers into exact, short and oversized destinations, then truncated and
    //      bit-flipped streams and junk ----
    for (int round = 0; round < 300; ++round) {
        const int n = round < 8 ? round : (int)(rnd() % (round % 10 == 9 ? 70000 : 12000));
        std::vector<uint8_t> raw(n + 1);
        const int kind = round % 4;
        for (int i = 0; i < n; ++i)
            raw[i] = kind == 0 ? 0 : kind == 1 ? (uint8_t)rnd() : kind == 2 ? (uint8_t)((i / 37) & 3) : (uint8_t)(i * 7);
        std::vector<uint8_t> enc(2 * n + 64);
        const long long m = ecseg_lzw_encode(raw.data(), n, enc.data(), (long long)enc.size());
        if (m < 0) { std::printf("encode failed at round %d\n", round); return 1; }
        if (!same(enc.data(), (size_t)m, (size_t)n, "round trip", round)) return 1;
        if (!same(enc.data(), (size_t)m, (size_t)n + 1 + rnd() % 300, "oversized destination", round)) return 1;
        if (!same(enc.data(), (size_t)m, rnd() % (n + 1), "short destination", round)) return 1;
        if (!same(enc.data() + (m > 2 ? 1 : 0), (size_t)m - (m > 2 ? 1 : 0), (size_t)n, "stream entered at byte 1", round)) return 1;
        for (int t = 0; t < 16; ++t) {
            std::vector<uint8_t> bad(enc.begin(), enc.begin() + (m ? 1 + rnd() % m : 0));
            const int flips = rnd() % 4;
            for (int f = 0; f < flips && !bad.empty(); ++f) bad[rnd() % bad.size()] ^= (uint8_t)(1u << (rnd() % 8));
            const size_t want = t % 3 == 0 ? (size_t)n : t % 3 == 1 ? rnd() % (n + 1) : (size_t)n + rnd() % 4096;
            if (!same(bad.data(), bad.size(), want, "damaged stream", round * 100 + t)) return 1;
        }
        std::vector<uint8_t> junk(rnd() % 4096);
        for (auto& b : junk) b = (uint8_t)rnd();
        if (!same(junk.data(), junk.size(), 5000, "junk", round)) return 1;
    }
    const long long built_in = n_ok + n_corrupt;
    // ---- the corpus of the tests ----
    long long records = 0;
    if (argc > 1) {
        FILE* f = std::fopen(argv[1], "rb");
        if (!f) { std::printf("cannot open %s\n", argv[1]); return 1; }
        uint8_t head[8];
        while (std::fread(head, 1, 8, f) == 8) {
            const uint32_t have = head[0] | head[1] << 8 | head[2] << 16 | (uint32_t)head[3] << 24;
            const uint32_t want = head[4] | head[5] << 8 | head[6] << 16 | (uint32_t)head[7] << 24;
            if (have > (1u << 26) || want > (1u << 26)) { std::printf("record %lld: implausible sizes\n", records); return 1; }
            std::vector<uint8_t> stream(have + 1);
            if (std::fread(stream.data(), 1, have, f) != have) { std::printf("record %lld is cut short\n", records); return 1; }
            if (!same(stream.data(), have, want, "corpus record", records)) return 1;
            ++records;
        }
        std::fclose(f);
    }
    std::printf("tiff_decode_fuzz ok: %lld built-in streams, %lld corpus records, %lld decoded, %lld corrupt\n", built_in, records, n_ok, n_corrupt);
    return 0;
}
