// A batch of TIFF files for one decode (ecseg_tiff_decode_batch, drivers_files.hip; the tiffb_* kernels, tiff_decode_kernels.hip): the
// device table, one TdFile row per file, and the one function that lays a batch out - where every file image, strip table and
// raster lies in the packed buffers, the prefix sums over strips and rows that give every workgroup its file, and the arena the
// call carves.  Plain C++: the driver includes it, and so does tools/asan/tiff_decode_batch_fuzz.cpp, which walks the same table on
// the host (as watershed_batch_bufs runs on a measuring Carver).
//   The files are uploaded as the caller holds them, one span from the first file's first byte to the last file's last, and the
// rasters lie on the device as they will in the caller's destination, relative to `dst_base`: a run of rasters without a gap is one
// copy back.  A 16-bit raster is read and written as uint16_t: its offset must be even (dst_base is, and the buffers start on 256
// bytes).  A file of zero strips (one the call leaves out: not OK, or a shape alone) owns nothing and no workgroup finds it.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <string>
#include <vector>

#include "scratch.h"

namespace ecseg {

// The codec of a file's strips.  TD_RAW and TD_LZW strips are tiffb_unstrip_kernel's, TD_DEFLATE strips tiffb_inflate_kernel's,
// TD_PACKBITS strips tiffb_packbits_kernel's; each kernel answers TD_OTHER_KERNEL (no status word) for a strip of another.
enum : uint8_t { TD_RAW = 0, TD_LZW = 1, TD_DEFLATE = 2, TD_PACKBITS = 3 };
constexpr uint32_t TD_OTHER_KERNEL = 2;

struct TdFile {
    uint64_t file_off;       // of the file image in the packed upload
    uint64_t n_bytes;
    uint64_t table_off;      // in uint32_t: n_table strip offsets, then n_table byte counts, in the packed tables
    uint64_t raster_off;     // of the raster in the packed output
    uint64_t line;           // bytes of a row: W * spp * bps
    uint32_t n_table;        // entries of the strip tables the image has rows for
    uint32_t H, rps, W, spp, bps;
    uint32_t first_strip;    // global index of strip 0 (grid x of tiffb_unstrip_kernel); the file has ceil(H / rps) strips
    uint32_t first_row;      // global index of row 0 (grid x of tiffb_unpredict_kernel); the file has H rows
    uint8_t codec, swap, predictor, in_batch;    // TD_RAW / TD_LZW / TD_DEFLATE / TD_PACKBITS strips; 16-bit samples in the other byte order; horizontal predictor; 0: a file of zero strips
    uint32_t tiles;          // 0: strips; else 1 + the file's row of the tiled-file table (then n_table is its tile count, rps its tile length)
};
static_assert(sizeof(TdFile) == 80, "the device table is an array of 80-byte rows, copied as it is");

// A tiled file: the tile grid, where its staging slots lie (tile k at stage_off + k * th * tw * spp * bps; unused for TD_RAW), and the
// global index of its first row of tiles (grid x of tiffb_untile_kernel; the file has `down` of them).
struct TdTiles {
    uint64_t stage_off;
    uint32_t file;           // its row of the file table
    uint32_t tw, th, across, down;
    uint32_t first_trow;
};
static_assert(sizeof(TdTiles) == 32, "the tiled-file table is an array of 32-byte rows, copied as it is");

// What the layout is made from, per file: the tags (parse_tiff), where the caller keeps the file and wants the raster.
struct TdFileIn {
    uint64_t src_off = 0, n_bytes = 0, dst_off = 0;
    uint32_t n_table = 0, H = 0, W = 0, spp = 1, bps = 1, rps = 1;
    uint8_t codec = TD_RAW;
    bool swap = false, predictor = false;
    uint32_t tw = 0, th = 0; // a tiled file's tile extents (0: strips); n_table is then at least its tile count
    bool in_batch = false;   // false: the file takes no part (zero strips, zero rows, nothing uploaded for it)
};

struct TdBatchLayout {
    std::vector<TdFile> tab;                     // one row per file, the files left out included
    uint64_t src_base = 0, src_span = 0;         // the upload: bytes [src_base, src_base + src_span) of the caller's files
    uint64_t dst_base = 0, dst_span = 0;         // the rasters: bytes [dst_base, dst_base + dst_span) of the caller's destination (dst_base even)
    uint64_t table_words = 0;                    // uint32_t of all strip tables
    uint64_t n_strips = 0, n_rows = 0;           // the two grids
    bool any_u8_predictor = false, any_u16_pass = false;     // which tiffb_unpredict_kernel launches the batch needs
    bool any_deflate = false;                    // whether it needs tiffb_inflate_kernel
    bool any_packbits = false;                   // whether it needs tiffb_packbits_kernel
    std::vector<TdTiles> tiles;                  // one row per tiled file that takes part (empty: no tiffb_untile_kernel, no staging)
    uint64_t stage_bytes = 0, n_trows = 0;       // the staging slots of all compressed tiles; the rows of tiles (the grid of tiffb_untile_kernel)
};

constexpr uint64_t TD_BATCH_MAX_GRID = (1ull << 31) - 1;     // grid dimension x

inline uint64_t td_file_strips(const TdFile& f) { return !f.in_batch ? 0 : f.tiles ? f.n_table : ((uint64_t)f.H + f.rps - 1) / f.rps; }
inline uint64_t td_file_raster_bytes(const TdFile& f) { return f.in_batch ? f.line * f.H : 0; }

// Empty string, or what is wrong: a 16-bit raster at an odd offset, or more strips or rows than a grid has.  The caller has made
// sure that ranges do not overlap.
inline std::string td_batch_layout(const std::vector<TdFileIn>& in, TdBatchLayout& L) {
    L = TdBatchLayout();
    L.tab.resize(in.size());
    uint64_t src_lo = UINT64_MAX, src_hi = 0, dst_lo = UINT64_MAX, dst_hi = 0;
    for (const TdFileIn& f : in) {
        if (!f.in_batch) continue;
        const uint64_t raster = (uint64_t)f.W * f.spp * f.bps * f.H;
        src_lo = f.src_off < src_lo ? f.src_off : src_lo;
        src_hi = f.src_off + f.n_bytes > src_hi ? f.src_off + f.n_bytes : src_hi;
        dst_lo = f.dst_off < dst_lo ? f.dst_off : dst_lo;
        dst_hi = f.dst_off + raster > dst_hi ? f.dst_off + raster : dst_hi;
    }
    if (src_lo == UINT64_MAX) src_lo = src_hi = dst_lo = dst_hi = 0;
    L.src_base = src_lo; L.src_span = src_hi - src_lo;
    L.dst_base = dst_lo & ~1ull; L.dst_span = dst_hi - L.dst_base;
    for (size_t i = 0; i < in.size(); ++i) {
        const TdFileIn& f = in[i];
        TdFile& t = L.tab[i];
        t = TdFile();
        t.first_strip = (uint32_t)L.n_strips; t.first_row = (uint32_t)L.n_rows; t.table_off = L.table_words;
        t.rps = 1;
        if (!f.in_batch) continue;
        if (f.bps == 2 && (f.dst_off & 1)) return "file " + std::to_string(i) + ": a 16-bit raster at an odd offset";
        t.in_batch = 1;
        t.file_off = f.src_off - L.src_base; t.n_bytes = f.n_bytes; t.raster_off = f.dst_off - L.dst_base;
        t.line = (uint64_t)f.W * f.spp * f.bps;
        t.n_table = f.n_table; t.H = f.H; t.rps = f.rps; t.W = f.W; t.spp = f.spp; t.bps = f.bps;
        t.codec = f.codec; t.swap = f.swap && f.bps == 2; t.predictor = f.predictor;
        if (f.tw) {                                          // tiles: the table holds the image's tiles and no more; compressed ones get a slot each
            TdTiles tt{L.stage_bytes, (uint32_t)i, f.tw, f.th, (f.W + f.tw - 1) / f.tw, (f.H + f.th - 1) / f.th, (uint32_t)L.n_trows};
            const uint64_t n_tiles = (uint64_t)tt.across * tt.down;
            if (n_tiles > f.n_table || n_tiles > TD_BATCH_MAX_GRID) return "file " + std::to_string(i) + ": a tile table shorter than the image";
            t.n_table = (uint32_t)n_tiles; t.rps = f.th; t.tiles = (uint32_t)L.tiles.size() + 1;
            if (f.codec != TD_RAW) L.stage_bytes += n_tiles * f.th * f.tw * f.spp * f.bps;
            L.n_trows += tt.down;
            L.tiles.push_back(tt);
        }
        L.table_words += 2ull * t.n_table;
        L.n_strips += td_file_strips(t);
        L.n_rows += f.H;
        if (L.n_strips > TD_BATCH_MAX_GRID || L.n_rows > TD_BATCH_MAX_GRID) return "the batch holds 2^31 strips or rows, or more";
        L.any_u16_pass = L.any_u16_pass || (!t.tiles && t.bps == 2 && (t.swap || t.predictor));      // (tiffb_untile_kernel does both for a tiled file)
        L.any_u8_predictor = L.any_u8_predictor || (!t.tiles && t.bps == 1 && t.predictor);
        L.any_deflate = L.any_deflate || t.codec == TD_DEFLATE;
        L.any_packbits = L.any_packbits || t.codec == TD_PACKBITS;
    }
    return std::string();
}

// Device buffers of one batch: the table, the file images, the strip tables, the rasters, one status word per strip and one per file;
// for a batch with tiled files, behind them, the tiled-file table and the staging slots.
// `rasters`: where the caller's destination lies on the device already (the input slots of ecseg_meta_segment_tiffs): the rasters are
// written there, from dst_base on, and the arena holds none.
struct TiffDecodeBatchBufs {
    TdFile* tab; uint8_t* files; uint32_t* tables; uint8_t* rasters; uint32_t* strip_status; uint32_t* file_status;
    TdTiles* tiles; uint8_t* staging;
};
inline TiffDecodeBatchBufs tiff_decode_batch_bufs(Carver& c, const TdBatchLayout& L, uint8_t* rasters = nullptr) {
    TiffDecodeBatchBufs b;
    b.tab = c.take<TdFile>(L.tab.size()); b.files = c.take<uint8_t>((size_t)L.src_span); b.tables = c.take<uint32_t>((size_t)L.table_words);
    b.rasters = rasters ? rasters + L.dst_base : c.take<uint8_t>((size_t)L.dst_span); b.strip_status = c.take<uint32_t>((size_t)L.n_strips);
    b.file_status = c.take<uint32_t>(L.tab.size());
    b.tiles = nullptr; b.staging = nullptr;
    if (!L.tiles.empty()) { b.tiles = c.take<TdTiles>(L.tiles.size()); b.staging = c.take<uint8_t>((size_t)L.stage_bytes); }
    return b;
}

}  // namespace ecseg
