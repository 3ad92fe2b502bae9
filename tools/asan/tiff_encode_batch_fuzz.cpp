// AddressSanitizer / UBSan driver for the batched device TIFF writer (ecseg_tiff_encode_batch): the layout function (te_batch_layout,
// csrc/tiff_encode_batch.h) and the strip routine (tl_strip, csrc/tiff_encode_strip.h, the body of tiff_lzw_strip_kernel and
// tiffb_lzw_strip_kernel) compiled for the host, where the 64 lanes are a loop.  CPU build only (`make asan_tiff_encode_batch`).
//   The layout: seeded lists of 0..40 files of extents 1..70 and both sample counts, with gaps between the rasters - every row is
// held to the strip plan of tiff_rows_per_strip, the running sums and the extents, every slot, offset table and strip to its buffer -
// and one list whose packed sizes pass 2^32, on the measuring carver only.
//   The strip routine: every strip of every file of every second list, and built-in strips (the chunk borders 1023 / 1024 / 1025,
// noise that restarts the table, a constant strip, a row wider than 8192 bytes), each into a heap slot of exactly the laid-out size,
// against ecseg_lzw_encode (csrc/host_codec.cpp) of the strip behind the horizontal predictor and the flip.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

#include "../../ecseg_amd/csrc/tiff_encode_batch.h"
#include "../../ecseg_amd/csrc/tiff_encode_strip.h"

extern "C" long long ecseg_lzw_encode(const uint8_t* src, long long n, uint8_t* dst, long long dst_cap);

using namespace ecseg;

static uint64_t s = 0x9e3779b97f4a7c15ull;
static uint32_t rnd() { s ^= s << 13; s ^= s >> 7; s ^= s << 17; return (uint32_t)(s >> 11); }

static TlLds lds;

// One strip through tl_strip into an exact heap slot, against the host encoder.  Returns false (and says why) on a difference.
static bool check_strip(const uint8_t* src, int rows, uint32_t line, uint32_t spp, uint32_t flip, uint64_t slot_stride, const char* what) {
    const uint32_t n = (uint32_t)rows * line, words = (uint32_t)(slot_stride / 4);
    std::unique_ptr<uint32_t[]> slot(new uint32_t[words]);
    std::memset(slot.get(), 0xAB, (size_t)words * 4);
    std::memset(&lds, 0xCD, sizeof lds);
    uint32_t cnt = 0xdeadbeefu;
    tl_strip(src, rows, line, spp, flip, slot.get(), words, &cnt, lds);
    std::unique_ptr<uint8_t[]> pre(new uint8_t[n]), enc(new uint8_t[tiff_strip_bound(n)]);
    for (uint32_t j = 0; j < n; ++j) {
        const uint32_t x = j % line;
        pre[j] = (uint8_t)((src[j] ^ flip) - (x >= spp ? (src[j - spp] ^ flip) : 0u));
    }
    const long long m = ecseg_lzw_encode(pre.get(), n, enc.get(), (long long)tiff_strip_bound(n));
    if (m < 0 || (uint32_t)m != cnt || std::memcmp(slot.get(), enc.get(), (size_t)m) != 0) {
        std::printf("%s: the routine gives %u bytes, the host encoder %lld, or their bytes differ\n", what, cnt, m);
        return false;
    }
    const uint8_t* b = reinterpret_cast<const uint8_t*>(slot.get());
    if ((cnt & 1u) && b[cnt] != 0) { std::printf("%s: the byte behind a strip of odd length is not 0\n", what); return false; }
    return true;
}

static std::vector<TeFileIn> make_list(int n, uint64_t* span) {
    std::vector<TeFileIn> in;
    uint64_t at = rnd() % 5;
    for (int i = 0; i < n; ++i) {
        TeFileIn f;
        f.H = 1 + rnd() % 70; f.W = 1 + rnd() % 70; f.spp = rnd() % 2 ? 3 : 1; f.invert = rnd() % 2;
        at += rnd() % 3 == 0 ? rnd() % 40 : 0;               // gaps between the rasters
        f.src_off = at;
        at += (uint64_t)f.H * f.W * f.spp;
        in.push_back(f);
    }
    *span = at;
    return in;
}

// tiff_encode_batch_fuzz layout <cases>: the layout of every batch of a text file for the tests' restatement - one file per line
// (src_off H W spp invert), a line "end" behind every batch -> per batch a line "batch src_base src_span n_strips max_strips slot_bytes
// off_entries packed_bytes arena" (or "refused"), then per file a line "file src_off slot_off slot_stride off_off frame_bytes rps flip
// first_strip n_strips".
static int print_layouts(const char* path) {
    FILE* f = std::fopen(path, "r");
    if (!f) { std::printf("cannot open %s\n", path); return 1; }
    char line[512];
    std::vector<TeFileIn> in;
    while (std::fgets(line, sizeof line, f)) {
        if (std::strncmp(line, "end", 3) != 0) {
            unsigned long long a;
            unsigned v[4];
            if (std::sscanf(line, "%llu %u %u %u %u", &a, v, v + 1, v + 2, v + 3) != 5) { std::printf("bad line: %s", line); std::fclose(f); return 1; }
            TeFileIn d;
            d.src_off = a; d.H = v[0]; d.W = v[1]; d.spp = v[2]; d.invert = v[3] != 0;
            in.push_back(d);
            continue;
        }
        TeBatchLayout L;
        if (!te_batch_layout(in, L).empty()) { std::printf("refused\n"); in.clear(); continue; }
        Carver c;
        (void)tiff_encode_batch_bufs(c, L, true);
        std::printf("batch %llu %llu %llu %u %llu %llu %llu %zu\n", (unsigned long long)L.src_base, (unsigned long long)L.src_span,
                    (unsigned long long)L.n_strips, L.max_strips, (unsigned long long)L.slot_bytes, (unsigned long long)L.off_entries,
                    (unsigned long long)L.packed_bytes, c.used);
        for (const TeFile& t : L.tab)
            std::printf("file %llu %llu %llu %llu %llu %u %u %u %u\n", (unsigned long long)t.src_off, (unsigned long long)t.slot_off,
                        (unsigned long long)t.slot_stride, (unsigned long long)t.off_off, (unsigned long long)t.frame_bytes, t.rps, t.flip, t.first_strip,
                        t.n_strips);
        in.clear();
    }
    std::fclose(f);
    return 0;
}

int main(int argc, char** argv) {
    if (argc > 2 && std::strcmp(argv[1], "layout") == 0) return print_layouts(argv[2]);
    long long files = 0, strips = 0, walked = 0;
    for (int round = 0; round < 300; ++round) {
        const int n = round < 3 ? round : (int)(rnd() % 41);
        uint64_t span = 0;
        const std::vector<TeFileIn> in = make_list(n, &span);
        TeBatchLayout L;
        const std::string bad = te_batch_layout(in, L);
        if (!bad.empty()) { std::printf("round %d: the layout refuses the list: %s\n", round, bad.c_str()); return 1; }
        Carver c;
        const TiffEncodeBatchBufs b = tiff_encode_batch_bufs(c, L, true);
        (void)b;
        if (L.tab.size() != in.size() || c.used < L.src_span + L.slot_bytes + L.packed_bytes) { std::printf("round %d: the arena is smaller than its parts\n", round); return 1; }
        if (n && (L.src_base != in[0].src_off || L.src_base + L.src_span != span)) { std::printf("round %d: the upload is not the span of the rasters\n", round); return 1; }
        uint64_t want_strips = 0, want_slots = 0, want_offs = 0, want_packed = 0;
        uint32_t most = 0;
        std::unique_ptr<uint8_t[]> src(new uint8_t[L.src_span]);
        for (uint64_t k = 0; k < L.src_span; ++k) src[k] = round % 3 == 0 ? (uint8_t)rnd() : (uint8_t)((k / 7) & 3);
        for (size_t i = 0; i < in.size(); ++i) {
            const TeFile& t = L.tab[i];
            const uint32_t rps = (uint32_t)tiff_rows_per_strip((int)in[i].H, (int)in[i].W, (int)in[i].spp), ns = (in[i].H + rps - 1) / rps;
            const uint64_t line = (uint64_t)in[i].W * in[i].spp;
            if (t.H != in[i].H || t.W != in[i].W || t.spp != in[i].spp || t.rps != rps || t.n_strips != ns || t.flip != (in[i].invert ? 0xffu : 0u) ||
                t.first_strip != want_strips || t.slot_off != want_slots || t.off_off != want_offs || t.src_off != in[i].src_off - L.src_base ||
                t.slot_stride % 16 || t.slot_stride < tiff_strip_bound(rps * line) || t.frame_bytes % 2 || t.frame_bytes != te_frame_bytes(ns, t.spp) ||
                t.src_off + line * t.H > L.src_span) {
                std::printf("round %d: row %zu of the table is not the file's\n", round, i);
                return 1;
            }
            want_strips += ns; want_slots += ns * t.slot_stride; want_offs += ns + 1; want_packed += t.frame_bytes + ns * t.slot_stride;
            most = ns > most ? ns : most;
            ++files;
            if (round % 2) continue;
            for (uint32_t k = 0; k < ns; ++k) {                  // the strips as tiffb_lzw_strip_kernel takes them from the row
                const uint32_t r0 = k * t.rps, rows = r0 + t.rps <= t.H ? t.rps : t.H - r0;
                // a copy of exactly the strip's bytes: a read outside them is the sanitizer's finding
                std::unique_ptr<uint8_t[]> strip(new uint8_t[rows * line]);
                std::memcpy(strip.get(), src.get() + t.src_off + r0 * line, rows * line);
                if (!check_strip(strip.get(), (int)rows, (uint32_t)line, t.spp, t.flip, t.slot_stride, "a strip of a seeded list")) return 1;
                ++walked;
            }
        }
        strips += (long long)L.n_strips;
        if (L.n_strips != want_strips || L.slot_bytes != want_slots || L.off_entries != want_offs || L.packed_bytes != want_packed || L.max_strips != most) {
            std::printf("round %d: the extents do not add up\n", round);
            return 1;
        }
    }
    // packed sizes beyond 2^32: 40 files of 30000 x 30000 x 3, on the measuring carver only
    {
        std::vector<TeFileIn> in(40);
        for (size_t i = 0; i < in.size(); ++i) { in[i].H = in[i].W = 30000; in[i].spp = 3; in[i].src_off = i * 2700000000ull; }
        TeBatchLayout L;
        if (!te_batch_layout(in, L).empty()) { std::printf("the large list is refused\n"); return 1; }
        Carver c;
        (void)tiff_encode_batch_bufs(c, L, true);
        if (L.src_span != 40 * 2700000000ull || L.n_strips != 40ull * 30000 || L.slot_bytes <= (1ull << 32) || L.tab[39].slot_off <= (1ull << 32) ||
            c.used < L.src_span + L.slot_bytes + L.packed_bytes) {
            std::printf("the large list loses bits\n");
            return 1;
        }
        std::vector<TeFileIn> many(65536);
        for (TeFileIn& f : many) f.H = f.W = 1;
        if (te_batch_layout(many, L).empty()) { std::printf("65536 files pass the layout\n"); return 1; }
    }
    // built-in strips
    struct Built { uint32_t rows, line, spp; int kind; const char* what; };
    const Built built[] = {
        {1, 1023, 1, 0, "1023 bytes of noise"}, {1, 1024, 1, 0, "1024 bytes of noise"}, {1, 1025, 1, 0, "1025 bytes of noise"},
        {1, 1024, 1, 1, "1024 constant bytes"}, {1, 1025, 1, 2, "1025 bytes of a short period"}, {1, 1, 1, 0, "one byte"}, {1, 3, 3, 0, "one pixel"},
        {1, 8192, 1, 0, "8192 bytes of noise (a restart inside the strip)"}, {8, 1024, 1, 0, "8 rows of 1024 bytes of noise"},
        {1, 8193, 3, 0, "a row of 8193 bytes"}, {1, 8192, 1, 1, "a constant strip"}, {2, 4095, 3, 2, "two rows of 4095 bytes"},
        {1, 40000, 1, 0, "40000 bytes of noise (restarts on and off chunk borders)"},
    };
    for (const Built& q : built)
        for (uint32_t flip = 0; flip <= 0xff; flip += 0xff) {
            const uint32_t n = q.rows * q.line;
            std::unique_ptr<uint8_t[]> raw(new uint8_t[n]);
            uint8_t run = 0;
            for (uint32_t i = 0; i < n; ++i) {                   // (noise is made so that the predictor leaves noise: a running sum)
                if (q.kind == 0) { if (i % q.line < q.spp) run = 0; run = (uint8_t)(run + rnd()); raw[i] = run; }
                else raw[i] = q.kind == 1 ? (uint8_t)77 : (uint8_t)((i / 5) & 3);
            }
            if (!check_strip(raw.get(), (int)q.rows, q.line, q.spp, flip, (tiff_strip_bound(n) + 15) / 16 * 16, q.what)) return 1;
            ++walked;
        }
    std::printf("tiff_encode_batch_fuzz ok: %lld files, %lld strips laid out, %lld strips encoded\n", files, strips, walked);
    return 0;
}
