// AddressSanitizer / UBSan driver for the tiled path of the device TIFF reader (option tiff_tiled_on_device): the tile-table parse
// (parse_tiff with tiles taken, csrc/host_io.cpp), tile_place (csrc/tiff_parse.h), the layout of a batch with tiled files
// (td_batch_layout, csrc/tiff_decode_batch.h) and the staging -> raster walk of tiffb_untile_kernel (tdb_untile, csrc/tiff_untile.h)
// compiled for the host, where the 64 lanes are a loop.  CPU build only (`make asan_tiff_tiles`).
//   Every round writes one to three tiled files in memory - extents from 1 x 1 to a few hundred, tiles of 16 to 64, 8 and 16 bits, 1, 3
// and 4 samples, both byte orders, predictor on and off, LZW and uncompressed tiles, some tile offsets behind the file, some
// uncompressed counts cut short - parses them, lays the batch out with gaps between the rasters, decodes every tile into its staging
// slot (tdb_unstrip) and places every row of tiles (tdb_untile).  Files, tables, staging and rasters are heap blocks of exactly the
// laid-out sizes, so a read or write outside them is the sanitizer's finding.  Checked: the parser's verdicts (tiles taken or not, a
// truncated table, tile extents that are no multiple of 16), tile_place against the sums a row must give, and every raster byte
// against a naive untile - per tile: the bytes in file order, the predictor along each tile row, the part inside the image copied -
// with no byte outside the rasters changed.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

#include "../../ecseg_amd/csrc/tiff_untile.h"

extern "C" long long ecseg_lzw_encode(const uint8_t* src, long long n, uint8_t* dst, long long dst_cap);

using namespace ecseg;

static uint64_t s = 0x2545f4914f6cdd1dull;
static uint32_t rnd() { s ^= s << 13; s ^= s >> 7; s ^= s << 17; return (uint32_t)(s >> 11); }

static TdLds lds;

struct File {
    std::vector<uint8_t> image;                  // the whole file
    std::vector<std::vector<uint8_t>> dec;       // per tile: the th * tw * px bytes the reader must see (zeros where the file has none)
    uint32_t H, W, th, tw, spp, bps, n_tiles;
    bool le, predictor, lzw, cut_table;
};

static void put16(std::vector<uint8_t>& b, bool le, uint32_t v) { b.push_back((uint8_t)(le ? v : v >> 8)); b.push_back((uint8_t)(le ? v >> 8 : v)); }
static void put32(std::vector<uint8_t>& b, bool le, uint32_t v) {
    for (int i = 0; i < 4; ++i) b.push_back((uint8_t)(v >> (le ? 8 * i : 24 - 8 * i)));
}

static File make_file() {
    File f;
    static const uint32_t tiles[4] = {16, 32, 48, 64};
    f.H = rnd() % 8 == 0 ? 1 : 1 + rnd() % 200; f.W = rnd() % 8 == 0 ? 1 : 1 + rnd() % 300;
    f.th = tiles[rnd() % 4]; f.tw = tiles[rnd() % 4];
    f.bps = 1 + rnd() % 2; f.spp = rnd() % 3 == 0 ? 1 : rnd() % 2 ? 3 : 4;
    f.le = rnd() % 2; f.predictor = rnd() % 2; f.lzw = rnd() % 2; f.cut_table = rnd() % 9 == 0;
    const uint32_t across = (f.W + f.tw - 1) / f.tw, down = (f.H + f.th - 1) / f.th, tile_bytes = f.th * f.tw * f.spp * f.bps;
    f.n_tiles = across * down;
    std::vector<uint32_t> off(f.n_tiles), cnt(f.n_tiles);
    f.image.assign(8, 0);
    f.dec.resize(f.n_tiles);
    std::vector<uint8_t> enc(2 * (size_t)tile_bytes + 64);
    for (uint32_t k = 0; k < f.n_tiles; ++k) {
        std::vector<uint8_t>& d = f.dec[k];
        d.resize(tile_bytes);
        const uint32_t kind = rnd() % 3;                     // noise, a ramp, a constant: short and long LZW strings
        for (uint32_t i = 0; i < tile_bytes; ++i) d[i] = (uint8_t)(kind == 0 ? rnd() : kind == 1 ? i / 7 + k : 3 * k);
        off[k] = (uint32_t)f.image.size();
        if (f.lzw) {
            const long long m = ecseg_lzw_encode(d.data(), tile_bytes, enc.data(), (long long)enc.size());
            if (m < 0) { std::printf("the encoder refused a tile\n"); std::exit(1); }
            cnt[k] = (uint32_t)m;
            f.image.insert(f.image.end(), enc.begin(), enc.begin() + m);
        } else {
            cnt[k] = tile_bytes;
            f.image.insert(f.image.end(), d.begin(), d.end());
            if (rnd() % 6 == 0) {                            // a count cut short: the rest of the tile is zeros
                cnt[k] = rnd() % tile_bytes;
                std::fill(d.begin() + cnt[k], d.end(), (uint8_t)0);
            }
        }
    }
    // the directory behind the tiles, then the two tables
    const uint32_t n_table = f.cut_table ? rnd() % f.n_tiles : f.n_tiles + rnd() % 2;      // (a table may be longer than the image)
    const uint32_t ifd = (uint32_t)f.image.size(), n_tags = 11, tab_at = ifd + 2 + 12 * n_tags + 4;
    for (uint32_t k = 0; k < f.n_tiles; ++k)
        if (rnd() % 10 == 0) {                               // behind the file: an empty stream, a tile of zeros
            off[k] = tab_at + 8 * (n_table + 1) + 1 + rnd() % 1000;
            std::fill(f.dec[k].begin(), f.dec[k].end(), (uint8_t)0);
        }
    const bool le = f.le;
    std::vector<uint8_t> d;
    put16(d, le, n_tags);
    auto entry = [&](uint32_t tag, uint32_t typ, uint32_t count, uint32_t v) {
        put16(d, le, tag); put16(d, le, typ); put32(d, le, count);
        if (typ == 3 && count == 1) { put16(d, le, v); put16(d, le, 0); } else put32(d, le, v);
    };
    entry(256, 4, 1, f.W); entry(257, 4, 1, f.H); entry(258, 3, 1, 8 * f.bps); entry(259, 3, 1, f.lzw ? 5 : 1);
    entry(277, 3, 1, f.spp); entry(284, 3, 1, 1); entry(317, 3, 1, f.predictor ? 2 : 1); entry(322, 4, 1, f.tw); entry(323, 4, 1, f.th);
    // (a table of one entry lies in the value field)
    entry(324, 4, n_table, n_table == 1 ? off[0] : tab_at); entry(325, 4, n_table, n_table == 1 ? cnt[0] : tab_at + 4 * n_table);
    put32(d, le, 0);
    for (uint32_t k = 0; k < n_table; ++k) put32(d, le, k < f.n_tiles ? off[k] : 0);
    for (uint32_t k = 0; k < n_table; ++k) put32(d, le, k < f.n_tiles ? cnt[k] : 0);
    f.image.insert(f.image.end(), d.begin(), d.end());
    f.image[0] = f.image[1] = le ? 'I' : 'M';
    std::vector<uint8_t> head;
    put16(head, le, 42); put32(head, le, ifd);
    std::memcpy(f.image.data() + 2, head.data(), 6);
    if (n_table == 0) f.cut_table = true;
    return f;
}

// What the Python reader does with the tiles' bytes: per tile the samples in file order, the predictor along each tile row, the part
// inside the image.
static void naive_untile(const File& f, uint8_t* raster) {
    const uint32_t across = (f.W + f.tw - 1) / f.tw, px = f.spp * f.bps;
    for (uint32_t k = 0; k < f.n_tiles; ++k) {
        const uint32_t ty = k / across, tx = k % across;
        for (uint32_t r = 0; r < f.th && ty * f.th + r < f.H; ++r) {
            std::vector<uint32_t> acc(f.spp, 0);
            for (uint32_t c0 = 0; c0 < f.tw; ++c0) {
                for (uint32_t c = 0; c < f.spp; ++c) {
                    const uint8_t* q = f.dec[k].data() + ((size_t)r * f.tw + c0) * px + (size_t)c * f.bps;
                    uint32_t v = f.bps == 1 ? q[0] : f.le ? (uint32_t)q[0] | ((uint32_t)q[1] << 8) : ((uint32_t)q[0] << 8) | q[1];
                    if (f.predictor) { acc[c] = (acc[c] + v) & (f.bps == 1 ? 0xffu : 0xffffu); v = acc[c]; }
                    const uint32_t x = tx * f.tw + c0;
                    if (x >= f.W) continue;
                    uint8_t* o = raster + ((size_t)(ty * f.th + r) * f.W + x) * px + (size_t)c * f.bps;
                    o[0] = (uint8_t)v;
                    if (f.bps == 2) o[1] = (uint8_t)(v >> 8);
                }
            }
        }
    }
}

static int check_tile_place(const File& f, int round) {
    const TileGeom g{f.H, f.W, f.th, f.tw, f.spp * f.bps};
    const uint32_t across = (f.W + f.tw - 1) / f.tw, down = (f.H + f.th - 1) / f.th;
    for (uint32_t ty = 0; ty < down; ++ty)
        for (uint32_t r = 0; r < f.th; ++r) {
            uint64_t kept = 0;
            for (uint32_t tx = 0; tx < across; ++tx) {
                const TilePlace p = tile_place(g, ty * across + tx, r);
                if (p.row != ty * f.th + r || p.col != tx * f.tw || p.keep + p.drop != f.tw * g.px || p.keep % g.px ||
                    (p.keep && (uint64_t)p.col * g.px + p.keep > (uint64_t)f.W * g.px) || (tx + 1 < across && p.row < f.H && p.drop)) {
                    std::printf("round %d: tile_place(%u, %u) = row %u col %u keep %u drop %u\n", round, ty * across + tx, r, p.row, p.col, p.keep, p.drop);
                    return 1;
                }
                kept += p.keep;
            }
            if (kept != (ty * f.th + r < f.H ? (uint64_t)f.W * g.px : 0)) { std::printf("round %d: row %u keeps %llu bytes\n", round, ty * f.th + r, (unsigned long long)kept); return 1; }
        }
    return 0;
}

int main() {
    long long files = 0, tiles = 0, refused = 0;
    for (int round = 0; round < 300; ++round) {
        const int n = 1 + (int)(rnd() % 3);
        std::vector<File> fs;
        std::vector<TiffInfo> info;
        std::vector<TdFileIn> in;
        uint64_t src = rnd() % 5, dst = rnd() % 5;
        for (int i = 0; i < n; ++i) {
            fs.push_back(make_file());
            const File& f = fs.back();
            TiffInfo t, t0;
            if (parse_tiff(f.image.data(), f.image.size(), &t0) != -5) { std::printf("round %d: a tiled file passes the parser without the switch\n", round); return 1; }
            const int rc = parse_tiff(f.image.data(), f.image.size(), &t, ECSEG_TIFF_TILED);
            if (rc != (f.cut_table ? -5 : 0)) { std::printf("round %d: file %d: the parser says %d (table cut: %d)\n", round, i, rc, (int)f.cut_table); return 1; }
            TdFileIn d;
            src += rnd() % 3 == 0 ? rnd() % 40 : 0;
            d.src_off = src; src += f.image.size();
            if (rc == 0) {
                if (t.tw != f.tw || t.th != f.th || t.W != f.W || t.H != f.H || t.spp != f.spp || t.bits != 8 * f.bps || t.le != f.le ||
                    t.off.size() < f.n_tiles || t.cnt.size() != t.off.size()) { std::printf("round %d: file %d: wrong tags\n", round, i); return 1; }
                if (check_tile_place(f, round)) return 1;
                d.in_batch = true; d.n_bytes = f.image.size(); d.n_table = (uint32_t)t.off.size(); d.H = t.H; d.W = t.W; d.spp = t.spp; d.bps = t.bits / 8;
                d.rps = t.H; d.tw = t.tw; d.th = t.th; d.codec = t.comp == 5 ? TD_LZW : TD_RAW; d.swap = d.bps == 2 && !t.le; d.predictor = t.pred == 2;
                dst += rnd() % 3 == 0 ? rnd() % 33 : 0;
                if (d.bps == 2) dst += dst & 1;
                d.dst_off = dst; dst += (uint64_t)d.W * d.spp * d.bps * d.H;
                ++files;
            } else {
                ++refused;
            }
            info.push_back(t);
            in.push_back(d);
        }
        TdBatchLayout L;
        const std::string bad = td_batch_layout(in, L);
        if (!bad.empty()) { std::printf("round %d: the layout refuses the batch: %s\n", round, bad.c_str()); return 1; }
        if (L.n_strips == 0) continue;
        std::unique_ptr<uint8_t[]> up(new uint8_t[L.src_span]), out(new uint8_t[L.dst_span]), ref(new uint8_t[L.dst_span]), stage(new uint8_t[L.stage_bytes + 1]);
        std::unique_ptr<uint32_t[]> tables(new uint32_t[L.table_words]);
        std::memset(up.get(), 0x5A, L.src_span);
        std::memset(out.get(), 0xAB, L.dst_span);
        std::memset(ref.get(), 0xAB, L.dst_span);
        std::memset(stage.get(), 0xEE, L.stage_bytes + 1);
        uint64_t want_stage = 0;
        for (size_t i = 0; i < fs.size(); ++i) {
            const TdFile& t = L.tab[i];
            if (!t.in_batch) continue;
            if (!t.tiles || t.tiles > L.tiles.size()) { std::printf("round %d: file %zu: no row of the tiled-file table\n", round, i); return 1; }
            const TdTiles& tt = L.tiles[t.tiles - 1];
            if (tt.file != i || t.n_table != fs[i].n_tiles || tt.across * tt.down != fs[i].n_tiles ||
                t.file_off + t.n_bytes > L.src_span || t.raster_off + td_file_raster_bytes(t) > L.dst_span || t.table_off + 2ull * t.n_table > L.table_words) {
                std::printf("round %d: file %zu: a wrong row of the tables\n", round, i);
                return 1;
            }
            if (t.codec != TD_RAW) {
                if (tt.stage_off != want_stage) { std::printf("round %d: file %zu: its slots start at %llu\n", round, i, (unsigned long long)tt.stage_off); return 1; }
                want_stage += (uint64_t)fs[i].n_tiles * tt.th * tt.tw * t.spp * t.bps;
            }
            std::memcpy(up.get() + t.file_off, fs[i].image.data(), t.n_bytes);
            for (uint32_t k = 0; k < t.n_table; ++k) { tables[t.table_off + k] = info[i].off[k]; tables[t.table_off + t.n_table + k] = info[i].cnt[k]; }
            naive_untile(fs[i], ref.get() + t.raster_off);
            tiles += fs[i].n_tiles;
        }
        if (want_stage != L.stage_bytes) { std::printf("round %d: the slots do not add up\n", round); return 1; }
        for (uint32_t g = 0; g < L.n_strips; ++g)
            if (tdb_unstrip(L.tab.data(), (uint32_t)fs.size(), up.get(), tables.get(), out.get(), g, lds, L.tiles.data(), stage.get()) != 0) {
                std::printf("round %d: tile %u: a clean stream is called corrupt\n", round, g);
                return 1;
            }
        if (stage[L.stage_bytes] != 0xEE) { std::printf("round %d: a byte behind the slots changed\n", round); return 1; }
        const uint32_t parts = 1 + rnd() % 8;
        for (uint32_t trow = 0; trow < L.n_trows; ++trow)
            for (uint32_t part = 0; part < parts; ++part)
                tdb_untile(L.tab.data(), L.tiles.data(), (uint32_t)L.tiles.size(), up.get(), tables.get(), stage.get(), out.get(), trow, part, parts);
        if (std::memcmp(out.get(), ref.get(), L.dst_span) != 0) {
            size_t at = 0;
            while (out[at] == ref[at]) ++at;
            std::printf("round %d: byte %zu of the packed rasters differs (%u for %u)\n", round, at, out[at], ref[at]);
            return 1;
        }
    }
    // tile extents that are no multiple of 16 stay the Python reader's
    File f = make_file();
    while (f.cut_table) f = make_file();
    TiffInfo t;
    const size_t ifd = f.le ? (size_t)f.image[4] | ((size_t)f.image[5] << 8) | ((size_t)f.image[6] << 16) | ((size_t)f.image[7] << 24)
                            : ((size_t)f.image[4] << 24) | ((size_t)f.image[5] << 16) | ((size_t)f.image[6] << 8) | f.image[7];
    const size_t tw_value = ifd + 2 + 12 * 7 + 8 + (f.le ? 0 : 3);           // the low byte of TileWidth, the eighth entry
    f.image[tw_value] = (uint8_t)(f.image[tw_value] + 8);
    if (parse_tiff(f.image.data(), f.image.size(), &t, ECSEG_TIFF_TILED) != -5) { std::printf("a tile width that is no multiple of 16 passes the parser\n"); return 1; }
    std::printf("tiff_tiles_check ok: %lld files, %lld tiles, %lld files refused for a short table\n", files, tiles, refused);
    return 0;
}
