// AddressSanitizer / UBSan driver for the batched device TIFF reader (ecseg_tiff_decode_batch): the layout function
// (td_batch_layout, csrc/tiff_decode_batch.h) and the batched strip walk (tdb_unstrip, csrc/tiff_decode_strip.h, the body of
// tiffb_unstrip_kernel) compiled for the host, where the 64 lanes are a loop.  CPU build only (`make asan_tiff_decode_batch`).
//   Every round packs a batch of files - LZW and uncompressed mixed, 8- and 16-bit, tables shorter than the image, some streams
// truncated or bit-flipped, some strip offsets behind the file - lays it out with gaps between the rasters, and walks every global
// strip.  Files, tables, rasters and status words are heap blocks of exactly the laid-out sizes, so a read or write outside them is
// the sanitizer's finding.  Checked: every strip against ecseg_lzw_decode (csrc/host_codec.cpp) or the clamped copy, status and
// bytes; the per-file status, folded as tiffb_status_kernel folds it, marks exactly the files that hold a corrupt strip; and no byte
// outside the rasters changes - with every other file equal to its reference, a corrupt file changes nothing but its own raster.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

#include "../../ecseg_amd/csrc/tiff_decode_strip.h"

extern "C" long long ecseg_lzw_decode(const uint8_t* src, long long n, uint8_t* dst, long long dst_cap);
extern "C" long long ecseg_lzw_encode(const uint8_t* src, long long n, uint8_t* dst, long long dst_cap);

using namespace ecseg;

static uint64_t s = 0x9e3779b97f4a7c15ull;
static uint32_t rnd() { s ^= s << 13; s ^= s >> 7; s ^= s << 17; return (uint32_t)(s >> 11); }

static TdLds lds;

struct File {
    std::vector<uint8_t> image;                  // the strips back to back behind 8 bytes of header
    std::vector<uint32_t> off, cnt;
    TdFileIn in;
};

static File make_file(bool in_batch) {
    File f;
    TdFileIn& d = f.in;
    d.in_batch = in_batch;
    d.bps = rnd() % 3 == 0 ? 2 : 1;
    d.spp = 1 + rnd() % 4;
    d.W = 1 + rnd() % (rnd() % 4 == 0 ? 300 : 20);
    d.H = 1 + rnd() % 12;
    d.rps = rnd() % 3 == 0 ? d.H : 1 + rnd() % d.H;
    d.codec = rnd() % 4 != 0 ? TD_LZW : TD_RAW;
    d.swap = d.bps == 2 && rnd() % 2;
    d.predictor = rnd() % 2;
    const uint32_t line = d.W * d.spp * d.bps, nstrips = (d.H + d.rps - 1) / d.rps;
    f.image.assign(8, 0x49);
    const int kind = rnd() % 3;
    for (uint32_t k = 0; k < nstrips; ++k) {
        const uint32_t rows = (k + 1) * d.rps <= d.H ? d.rps : d.H - k * d.rps, n = rows * line;
        std::vector<uint8_t> raw(n + 1), enc(2 * n + 64);
        for (uint32_t i = 0; i < n; ++i) raw[i] = kind == 0 ? (uint8_t)rnd() : kind == 1 ? (uint8_t)((i / 5) & 3) : (uint8_t)0;
        long long m = n;
        if (d.codec == TD_LZW) {
            m = ecseg_lzw_encode(raw.data(), n, enc.data(), (long long)enc.size());
            if (m < 0) { std::printf("encode failed\n"); std::exit(1); }
        } else {
            std::memcpy(enc.data(), raw.data(), n);
        }
        const uint32_t damage = rnd() % 8;                   // 0: flips, 1: cut short, 2: the count says more than the file has
        if (damage == 0) for (int j = 0; j < 3 && m; ++j) enc[rnd() % m] ^= (uint8_t)(1u << (rnd() % 8));
        f.off.push_back((uint32_t)f.image.size());
        f.cnt.push_back(damage == 1 ? (uint32_t)(m ? rnd() % m : 0) : damage == 2 ? (uint32_t)m + 1000 : (uint32_t)m);
        f.image.insert(f.image.end(), enc.begin(), enc.begin() + m);
    }
    if (rnd() % 10 == 0) f.off[rnd() % nstrips] = (uint32_t)f.image.size() + 1 + rnd() % 1000;      // behind the file
    d.n_table = rnd() % 6 == 0 ? rnd() % (nstrips + 1) : nstrips;                                   // a short strip table
    d.n_bytes = f.image.size();
    return f;
}

// tiff_decode_batch_fuzz layout <cases>: the layout of every batch of a text file for the tests' restatement - one file per line
// (src_off n_bytes dst_off n_table H W spp bps rps lzw swap predictor in_batch), a line "end" behind every batch -> per batch a line
// "batch src_base src_span dst_base dst_span table_words n_strips n_rows u8 u16 arena" (or "refused"), then per file a line
// "file file_off table_off raster_off first_strip first_row in_batch".
static int print_layouts(const char* path) {
    FILE* f = std::fopen(path, "r");
    if (!f) { std::printf("cannot open %s\n", path); return 1; }
    char line[512];
    std::vector<TdFileIn> in;
    while (std::fgets(line, sizeof line, f)) {
        if (std::strncmp(line, "end", 3) != 0) {
            unsigned long long a, b, c;
            unsigned v[10];
            if (std::sscanf(line, "%llu %llu %llu %u %u %u %u %u %u %u %u %u %u", &a, &b, &c, v, v + 1, v + 2, v + 3, v + 4, v + 5, v + 6, v + 7, v + 8, v + 9) != 13) {
                std::printf("bad line: %s", line);
                std::fclose(f);
                return 1;
            }
            TdFileIn d;
            d.src_off = a; d.n_bytes = b; d.dst_off = c; d.n_table = v[0]; d.H = v[1]; d.W = v[2]; d.spp = v[3]; d.bps = v[4]; d.rps = v[5];
            d.codec = (uint8_t)v[6]; d.swap = v[7]; d.predictor = v[8]; d.in_batch = v[9];
            in.push_back(d);
            continue;
        }
        TdBatchLayout L;
        if (!td_batch_layout(in, L).empty()) { std::printf("refused\n"); in.clear(); continue; }
        Carver c;
        (void)tiff_decode_batch_bufs(c, L);
        std::printf("batch %llu %llu %llu %llu %llu %llu %llu %d %d %zu\n", (unsigned long long)L.src_base, (unsigned long long)L.src_span,
                    (unsigned long long)L.dst_base, (unsigned long long)L.dst_span, (unsigned long long)L.table_words, (unsigned long long)L.n_strips,
                    (unsigned long long)L.n_rows, (int)L.any_u8_predictor, (int)L.any_u16_pass, c.used);
        for (const TdFile& t : L.tab)
            std::printf("file %llu %llu %llu %u %u %d\n", (unsigned long long)t.file_off, (unsigned long long)t.table_off, (unsigned long long)t.raster_off,
                        t.first_strip, t.first_row, (int)t.in_batch);
        in.clear();
    }
    std::fclose(f);
    return 0;
}

int main(int argc, char** argv) {
    if (argc > 2 && std::strcmp(argv[1], "layout") == 0) return print_layouts(argv[2]);
    long long files = 0, strips = 0, corrupt_files = 0;
    for (int round = 0; round < 400; ++round) {
        const int n = round < 3 ? round + 1 : round % 50 == 49 ? 65 + (int)(rnd() % 40) : 1 + (int)(rnd() % 9);
        std::vector<File> fs;
        uint64_t src = rnd() % 7, dst = rnd() % 5;
        for (int i = 0; i < n; ++i) {
            fs.push_back(make_file(n == 1 || rnd() % 7 != 0));
            TdFileIn& d = fs.back().in;
            src += rnd() % 3 == 0 ? rnd() % 40 : 0;                      // gaps between the file images
            d.src_off = src; src += d.n_bytes;
            dst += rnd() % 3 == 0 ? rnd() % 33 : 0;                      // and between the rasters
            if (d.bps == 2) dst += dst & 1;
            d.dst_off = dst;
            if (d.in_batch) dst += (uint64_t)d.W * d.spp * d.bps * d.H;
        }
        std::vector<TdFileIn> in;
        for (const File& f : fs) in.push_back(f.in);
        TdBatchLayout L;
        const std::string bad = td_batch_layout(in, L);
        if (!bad.empty()) { std::printf("round %d: the layout refuses the batch: %s\n", round, bad.c_str()); return 1; }
        Carver c;
        (void)tiff_decode_batch_bufs(c, L);
        if (c.used < L.src_span + L.dst_span) { std::printf("round %d: the arena is smaller than its parts\n", round); return 1; }
        // exact blocks
        std::unique_ptr<uint8_t[]> up(new uint8_t[L.src_span]), out(new uint8_t[L.dst_span]), ref(new uint8_t[L.dst_span]);
        std::unique_ptr<uint32_t[]> tables(new uint32_t[L.table_words]), st(new uint32_t[L.n_strips]), fst(new uint32_t[fs.size()]);
        std::memset(up.get(), 0x5A, L.src_span);
        std::memset(out.get(), 0xAB, L.dst_span);
        std::memset(ref.get(), 0xAB, L.dst_span);
        std::memset(fst.get(), 0, fs.size() * sizeof(uint32_t));
        uint64_t want_strips = 0;
        for (size_t i = 0; i < fs.size(); ++i) {
            const TdFile& t = L.tab[i];
            if (t.first_strip != want_strips) { std::printf("round %d: file %zu starts at strip %u, not %llu\n", round, i, t.first_strip, (unsigned long long)want_strips); return 1; }
            if (!t.in_batch) continue;
            want_strips += td_file_strips(t);
            if (t.file_off + t.n_bytes > L.src_span || t.raster_off + td_file_raster_bytes(t) > L.dst_span || t.table_off + 2ull * t.n_table > L.table_words ||
                (t.bps == 2 && (t.raster_off & 1))) {
                std::printf("round %d: file %zu leaves its buffers\n", round, i);
                return 1;
            }
            std::memcpy(up.get() + t.file_off, fs[i].image.data(), t.n_bytes);
            for (uint32_t k = 0; k < t.n_table; ++k) { tables[t.table_off + k] = fs[i].off[k]; tables[t.table_off + t.n_table + k] = fs[i].cnt[k]; }
        }
        if (want_strips != L.n_strips) { std::printf("round %d: the strips do not add up\n", round); return 1; }
        // the walk: every global strip, then the fold of tiffb_status_kernel
        for (uint32_t g = 0; g < L.n_strips; ++g) {
            std::memset(lds.pos, 0xCD, sizeof lds.pos);
            std::memset(lds.len, 0xCD, sizeof lds.len);
            st[g] = tdb_unstrip(L.tab.data(), (uint32_t)fs.size(), up.get(), tables.get(), out.get(), g, lds);
            if (st[g]) fst[td_find_file(L.tab.data(), (uint32_t)fs.size(), g, false)] |= 1u;
        }
        strips += (long long)L.n_strips;
        // the reference: strip by strip with the host decoder
        for (size_t i = 0; i < fs.size(); ++i) {
            const TdFile& t = L.tab[i];
            if (!t.in_batch) { if (fst[i]) { std::printf("round %d: file %zu takes no part and is marked\n", round, i); return 1; } continue; }
            ++files;
            bool corrupt = false;
            const uint64_t ns = td_file_strips(t);
            for (uint64_t k = 0; k < ns; ++k) {
                const uint64_t rows = (k + 1) * t.rps <= t.H ? t.rps : t.H - k * t.rps, want = rows * t.line;
                uint8_t* q = ref.get() + t.raster_off + k * t.rps * t.line;
                std::memset(q, 0, want);
                bool bad_strip = false;
                if (k < t.n_table) {
                    const uint64_t off = fs[i].off[k], cnt = fs[i].cnt[k];
                    if (off > t.n_bytes) bad_strip = true;
                    else {
                        const uint64_t have = cnt < t.n_bytes - off ? cnt : t.n_bytes - off;
                        if (t.codec == TD_LZW) {
                            std::unique_ptr<uint8_t[]> src(new uint8_t[have]), tmp(new uint8_t[want + 1]);
                            std::memcpy(src.get(), fs[i].image.data() + off, have);
                            const long long r = ecseg_lzw_decode(src.get(), (long long)have, tmp.get(), (long long)want);
                            if (r < 0) bad_strip = true; else std::memcpy(q, tmp.get(), (size_t)r);
                        } else {
                            std::memcpy(q, fs[i].image.data() + off, have < want ? have : want);
                        }
                    }
                }
                if (bad_strip != (st[t.first_strip + k] != 0)) {
                    std::printf("round %d: file %zu strip %llu: the host says %s, the walk status %u\n", round, i, (unsigned long long)k, bad_strip ? "corrupt" : "ok", st[t.first_strip + k]);
                    return 1;
                }
                corrupt = corrupt || bad_strip;
            }
            if (corrupt != (fst[i] != 0)) { std::printf("round %d: file %zu: the folded status is %u\n", round, i, fst[i]); return 1; }
            if (corrupt) {                                    // its raster is not compared (the driver does not copy it back): take the walk's bytes
                ++corrupt_files;
                std::memcpy(ref.get() + t.raster_off, out.get() + t.raster_off, td_file_raster_bytes(t));
            }
        }
        if (std::memcmp(out.get(), ref.get(), L.dst_span) != 0) {
            size_t at = 0;
            while (out[at] == ref[at]) ++at;
            std::printf("round %d: byte %zu of the packed rasters differs\n", round, at);
            return 1;
        }
    }
    // a 16-bit raster at an odd offset is refused, and so is a grid that is too long
    std::vector<TdFileIn> in(1);
    in[0].in_batch = true; in[0].bps = 2; in[0].H = in[0].W = 2; in[0].dst_off = 7; in[0].n_bytes = 8;
    TdBatchLayout L;
    if (td_batch_layout(in, L).empty()) { std::printf("an odd 16-bit raster passes the layout\n"); return 1; }
    in[0].dst_off = 8; in[0].H = 0x7fffffffu; in.push_back(in[0]); in[1].dst_off = 1ull << 40;
    if (td_batch_layout(in, L).empty()) { std::printf("2^32 rows pass the layout\n"); return 1; }
    std::printf("tiff_decode_batch_fuzz ok: %lld files, %lld strips, %lld corrupt files\n", files, strips, corrupt_files);
    return 0;
}
