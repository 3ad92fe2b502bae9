// AddressSanitizer / UBSan driver for the device TIFF reader's Deflate strip routine (csrc/tiff_inflate_strip.h, the body of
// tiffb_inflate_kernel) compiled for the host: the 64 lanes are a loop, the read of lane 0 and the store fence do nothing.  CPU build
// only (`make asan_tiff_inflate`, links -lz).  Every stream is decoded by the routine and judged by the host reader's rule
// (ecseg_tiff_read, csrc/host_io.cpp: uncompress, then inflate(Z_FINISH) on Z_BUF_ERROR), which is made here of the same zlib calls:
// the status must agree, and where it is OK every byte of the strip (zero fill included).  One class is judged by the stated rule
// and not by the zlib on this machine: a stream that ends before the strip is full and before its own end is corrupt (uncompress
// from 1.2.9 on; older ones accept it).  Source and destination are heap blocks of exactly `have` and `want` bytes, so a read or
// write outside them is the sanitizer's finding.
//   tiff_inflate_fuzz [corpus]   corpus: records { uint32 have, uint32 want (little-endian), have bytes }, the streams of
//                                tests/tiff_inflate_cases.py; without it only the built-in streams run.
//   tiff_inflate_fuzz corpus list   also prints "record <index> <class>" for every record of the corpus.
// Prints the case count of every class (zlib's own message names the corrupt ones) and stops at the first difference.
#include <zlib.h>

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <memory>
#include <string>
#include <vector>

#include "../../ecseg_amd/csrc/tiff_inflate_strip.h"

static uint64_t s = 0x2545f4914f6cdd1dull;
static uint32_t rnd() { s ^= s << 13; s ^= s >> 7; s ^= s << 17; return (uint32_t)(s >> 11); }

static ecseg::TiLds lds;
static std::map<std::string, long long> classes;
static std::string last_class;

// The rule: one inflate over the whole stream into `want` bytes.  -> false for corrupt; *got: the bytes it gave; *cls: the class.
static bool rule(const uint8_t* src, size_t have, uint8_t* dst, size_t want, size_t* got, std::string* cls) {
    z_stream zs;
    std::memset(&zs, 0, sizeof zs);
    if (inflateInit(&zs) != Z_OK) { std::printf("inflateInit failed\n"); std::exit(1); }
    zs.next_in = const_cast<Bytef*>(src); zs.avail_in = (uInt)have; zs.next_out = dst; zs.avail_out = (uInt)want;
    int z;
    do z = inflate(&zs, Z_NO_FLUSH); while (z == Z_OK);
    *got = want - zs.avail_out;
    bool ok = false;
    if (z == Z_STREAM_END) { ok = true; *cls = *got < want ? "ok: a complete stream shorter than the strip" : "ok: a complete stream of the strip's size"; }
    else if (z == Z_NEED_DICT) *cls = "corrupt: FDICT set";
    else if (z == Z_BUF_ERROR && zs.avail_out == 0) { ok = true; *cls = zs.avail_in ? "ok: the strip is full before the stream ends" : "ok: out of input with the strip full"; }
    else if (z == Z_BUF_ERROR) *cls = "corrupt: the stream ends before the strip is full";
    else if (z == Z_DATA_ERROR) *cls = std::string("corrupt: ") + (zs.msg ? zs.msg : "data error");
    else { std::printf("inflate returns %d\n", z); std::exit(1); }
    inflateEnd(&zs);
    return ok;
}

// The host reader's own sequence on this machine's zlib.  -> false for ECSEG_E_INVALID.
static bool host_reader(const uint8_t* src, size_t have, uint8_t* d, size_t want, size_t* got) {
    uLongf cap = (uLongf)want;
    const int z = uncompress(d, &cap, src, (uLong)have);
    if (z != Z_OK && z != Z_BUF_ERROR) return false;
    *got = z == Z_OK ? (size_t)cap : 0;
    if (z == Z_BUF_ERROR) {
        z_stream zs; std::memset(&zs, 0, sizeof zs);
        if (inflateInit(&zs) != Z_OK) return false;
        zs.next_in = const_cast<Bytef*>(src); zs.avail_in = (uInt)have; zs.next_out = d; zs.avail_out = (uInt)want;
        const int zr = inflate(&zs, Z_FINISH);
        *got = want - zs.avail_out;
        inflateEnd(&zs);
        if (zr != Z_STREAM_END && zr != Z_BUF_ERROR && zr != Z_OK) return false;
    }
    return true;
}

// -> false (and a message) when the routine and the rule disagree
static bool same(const uint8_t* stream, size_t have, size_t want, const char* what, long long index) {
    std::unique_ptr<uint8_t[]> src(new uint8_t[have]), got(new uint8_t[want]), ref(new uint8_t[want]), ref2(new uint8_t[want]);
    std::memcpy(src.get(), stream, have);
    std::memset(got.get(), 0xAB, want);
    std::memset(&lds, 0xCD, sizeof lds);                     // (stale tables of an earlier strip: never read)
    size_t n = 0, n2 = 0;
    std::string cls;
    const bool ok = rule(src.get(), have, ref.get(), want, &n, &cls);
    ++classes[cls];
    last_class = cls;
    const bool ok2 = host_reader(src.get(), have, ref2.get(), want, &n2);
    const bool version_class = cls == "corrupt: the stream ends before the strip is full";
    if (ok2 != ok && !(version_class && ok2)) { std::printf("%s %lld: the rule says %s, the host reader %d\n", what, index, cls.c_str(), (int)ok2); return false; }
    if (ok && (n2 != n || std::memcmp(ref.get(), ref2.get(), n) != 0)) { std::printf("%s %lld: the rule and the host reader give other bytes\n", what, index); return false; }
    const uint32_t st = ecseg::ti_inflate_strip(src.get(), (uint32_t)have, got.get(), (uint32_t)want, lds);
    if (ok != (st == 0)) { std::printf("%s %lld (have %zu, want %zu): the rule says %s, the routine status %u\n", what, index, have, want, cls.c_str(), st); return false; }
    if (!ok) return true;
    std::memset(ref.get() + n, 0, want - n);
    if (std::memcmp(got.get(), ref.get(), want) != 0) {
        size_t at = 0;
        while (got[at] == ref[at]) ++at;
        std::printf("%s %lld: byte %zu of %zu differs (%s, the rule gave %zu bytes)\n", what, index, at, want, cls.c_str(), n);
        return false;
    }
    return true;
}

// zlib's stream for raw at a level and strategy, in `blocks` pieces behind full flushes
static std::vector<uint8_t> deflated(const std::vector<uint8_t>& raw, int level, int strategy, int blocks) {
    z_stream zs;
    std::memset(&zs, 0, sizeof zs);
    if (deflateInit2(&zs, level, Z_DEFLATED, 9 + (int)(rnd() % 7), 8, strategy) != Z_OK) { std::printf("deflateInit2 failed\n"); std::exit(1); }
    std::vector<uint8_t> out(deflateBound(&zs, (uLong)raw.size()) + 64 * (size_t)blocks + 64);
    zs.next_out = out.data(); zs.avail_out = (uInt)out.size();
    size_t done = 0;
    for (int b = 0; b < blocks; ++b) {
        const size_t n = b + 1 == blocks ? raw.size() - done : (raw.size() - done) / (size_t)(blocks - b);
        zs.next_in = const_cast<Bytef*>(raw.data() + done); zs.avail_in = (uInt)n;
        const int z = deflate(&zs, b + 1 == blocks ? Z_FINISH : Z_FULL_FLUSH);
        if (z != (b + 1 == blocks ? Z_STREAM_END : Z_OK)) { std::printf("deflate returns %d\n", z); std::exit(1); }
        done += n;
    }
    out.resize(out.size() - zs.avail_out);
    deflateEnd(&zs);
    return out;
}

int main(int argc, char** argv) {
    long long built_in = 0, records = 0;
    // ---- built-in: zlib's streams of structured / random buffers at every kind of block, into exact, short and oversized
    //      destinations; then truncations, bit flips, spliced headers and junk ----
    for (int round = 0; round < 400; ++round) {
        const int n = 1 + (round < 8 ? round : (int)(rnd() % (round % 10 == 9 ? 70000 : 12000)));
        std::vector<uint8_t> raw((size_t)n);
        const int kind = round % 5;
        for (int i = 0; i < n; ++i)
            raw[(size_t)i] = kind == 0 ? 0 : kind == 1 ? (uint8_t)rnd() : kind == 2 ? (uint8_t)((i / 37) & 3) : kind == 3 ? (uint8_t)(i * 7) : (uint8_t)(rnd() % 3 ? 65 + rnd() % 4 : rnd());
        const int levels[] = {0, 1, 6, 9}, strategies[] = {Z_DEFAULT_STRATEGY, Z_FIXED, Z_HUFFMAN_ONLY, Z_RLE, Z_FILTERED};
        const std::vector<uint8_t> z = deflated(raw, levels[rnd() % 4], strategies[rnd() % 5], 1 + (int)(rnd() % 4));
        const size_t m = z.size();
        if (!same(z.data(), m, (size_t)n, "round trip", round)) return 1;
        if (!same(z.data(), m, (size_t)n + 1 + rnd() % 300, "short stream", round)) return 1;
        if (n > 1 && !same(z.data(), m, 1 + rnd() % ((size_t)n - 1), "long stream", round)) return 1;
        built_in += 3;
        for (int k = 0; k < 6; ++k) {                        // truncations, into the exact and a smaller destination
            const size_t cut = rnd() % m, want = k % 2 || n == 1 ? (size_t)n : 1 + rnd() % ((size_t)n - 1);
            if (!same(z.data(), cut, want, "truncated", round)) return 1;
            ++built_in;
        }
        for (int k = 0; k < 12; ++k) {                       // bit flips, early ones (the headers and tables) as often as late ones
            std::vector<uint8_t> bad(z);
            const int flips = 1 + (int)(rnd() % 3);
            for (int j = 0; j < flips; ++j) bad[k % 2 ? rnd() % m : rnd() % (m < 40 ? m : 40)] ^= (uint8_t)(1u << (rnd() % 8));
            const size_t want = k % 3 == 0 && n > 1 ? 1 + rnd() % ((size_t)n - 1) : k % 3 == 1 ? (size_t)n + rnd() % 50 : (size_t)n;
            if (!same(bad.data(), m, want, "bit flips", round)) return 1;
            ++built_in;
        }
        {                                                    // a spliced header: another stream's head on this one's tail, and the trailer off
            std::vector<uint8_t> other(raw);
            for (uint8_t& v : other) v = (uint8_t)(v + rnd() % 2);
            const std::vector<uint8_t> z2 = deflated(other, 6, Z_DEFAULT_STRATEGY, 1);
            std::vector<uint8_t> bad(z);
            const size_t head = rnd() % (z2.size() < m ? z2.size() : m);
            std::memcpy(bad.data(), z2.data(), head);
            if (!same(bad.data(), m, (size_t)n, "spliced", round)) return 1;
            bad = z;
            bad[m - 1 - rnd() % 4] ^= (uint8_t)(1u << (rnd() % 8));   // a wrong Adler-32
            if (!same(bad.data(), m, (size_t)n, "wrong check", round)) return 1;
            if (!same(bad.data(), m, (size_t)n + 7, "wrong check, short", round)) return 1;
            built_in += 3;
        }
    }
    for (int round = 0; round < 300; ++round) {              // junk behind a valid and behind a random header
        const size_t m = rnd() % 600;
        std::vector<uint8_t> junk(m + 2);
        for (uint8_t& v : junk) v = (uint8_t)rnd();
        if (round % 2) { junk[0] = 0x78; junk[1] = 0x9c; }
        if (!same(junk.data(), junk.size(), 1 + rnd() % 3000, "junk", round)) return 1;
        ++built_in;
    }
    if (!same(reinterpret_cast<const uint8_t*>(""), 0, 5, "empty stream", 0)) return 1;
    ++built_in;
    // ---- the corpus of the tests ----
    if (argc > 1) {
        FILE* f = std::fopen(argv[1], "rb");
        if (!f) { std::printf("cannot open %s\n", argv[1]); return 1; }
        uint8_t head[8];
        while (std::fread(head, 1, 8, f) == 8) {
            const uint32_t have = head[0] | head[1] << 8 | head[2] << 16 | (uint32_t)head[3] << 24;
            const uint32_t want = head[4] | head[5] << 8 | head[6] << 16 | (uint32_t)head[7] << 24;
            if (have > (64u << 20) || want == 0 || want > (64u << 20)) { std::printf("record %lld: a bad header\n", records); return 1; }
            std::vector<uint8_t> stream(have + 1);
            if (std::fread(stream.data(), 1, have, f) != have) { std::printf("record %lld: cut short\n", records); return 1; }
            if (!same(stream.data(), have, want, "corpus record", records)) return 1;
            if (argc > 2 && std::strcmp(argv[2], "list") == 0) std::printf("record %lld %s\n", records, last_class.c_str());
            ++records;
        }
        std::fclose(f);
    }
    for (const auto& c : classes) std::printf("class %lld %s\n", c.second, c.first.c_str());
    std::printf("tiff_inflate_fuzz ok: %lld built-in streams, %lld corpus records, zlib %s\n", built_in, records, zlibVersion());
    return 0;
}
