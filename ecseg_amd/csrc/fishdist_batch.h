// Host and device: the layout of ecseg_fish_distances_batch (drivers_fish.hip, the fdb_* kernels of fishdist_kernels.hip), stated once
// and shared with the host program that walks it under ASan + UBSan (tools/asan/fishdist_batch_check.cpp).  No HIP in here.
//
// One call holds a chunk of images of any extents (H_i, W_i, C_i).  Their pixels lie back to back on ONE global pixel axis: image i
// owns the pixels px0_i .. px0_i + H_i * W_i - 1 of the label map, of the flag space the dense cell index is scanned over (a label l
// of image i is flag px0_i + l - 1, so one exclusive scan numbers the cells of the chunk ascending by (image, label)), of the
// union-find parents and of the two pixel lists.  Its lsq raster lies at byte lsq0_i of one byte buffer, the rasters back to back.
//   Two kinds of workgroup walk an image and both must never straddle two images, so each image has its own run of them:
//   * statistics tiles (cell_util.h: 64 columns x 32 rows), tile0_i .. tile0_i + stat_tiles(H_i, W_i) - 1;
//   * blocks of 256 pixels, blk0_i .. blk0_i + ceil(H_i * W_i / 256) - 1.
// A workgroup finds its image with fdb_find, a binary search over the prefix table (every image has at least one tile and one block:
// the prefixes rise strictly), and then its local tile or block by subtraction.  Rows and columns are always local to the image; only
// union-find parents are global pixel indices (a neighbour at p - 1, p - W or p - W +- 1 of a pixel with local x > 0 / y > 0 is the
// same image's, so the single-image neighbour walk never crosses a seam).
#pragma once
#include <stdint.h>

#include <string>
#include <vector>

#include "scratch.h"

#if defined(__HIPCC__) || defined(__CUDACC__)
#define FDB_HD __host__ __device__ __forceinline__
#else
#define FDB_HD inline
#endif

namespace ecseg {

constexpr int FDB_MAX_IMAGES = 8192;                     // ECSEG_FISH_DISTANCES_BATCH_MAX_IMAGES
constexpr long long FDB_MAX_PIXELS = 1ll << 31;          // the whole chunk stays below: pixel indices and cell counts are int32
constexpr long long FDB_MAX_LSQ_BYTES = 1ll << 40;       // ... and its lsq rasters below this
constexpr long long FDB_SCRATCH_LIMIT = 8ll << 30;       // scratch bytes of one group; a chunk above it runs as several groups
constexpr int FDB_TILE_W = 64, FDB_TILE_H = 32;          // cell_util.h's statistics tile (the kernels file asserts the two agree)
constexpr int FDB_SLICE_BUDGET = 4096;                   // fishdist_slices: n * S <= 4096 + n partials

// One image as the fdb_* kernels read it.
struct FdbImage {
    long long lsq0;                                      // first byte of its (H, W, C) raster
    int32_t px0, tile0, blk0;                            // first pixel, statistics tile and 256-pixel block
    int32_t H, W, C;
};
static_assert(sizeof(FdbImage) == 32, "an array of rows holding a 64-bit field");

FDB_HD unsigned fdb_tiles(int H, int W) {                // == stat_tiles(H, W)
    return (((unsigned)W + FDB_TILE_W - 1) / FDB_TILE_W) * (((unsigned)H + FDB_TILE_H - 1) / FDB_TILE_H);
}
FDB_HD unsigned fdb_blocks(int H, int W) { return (unsigned)(((long long)H * W + 255) / 256); }

// The image of tile or block `idx`: the largest i < n with first(i) <= idx, where first(i) = tab[i].tile0 (by_tile) or tab[i].blk0.
// idx must lie below the chunk's total; first(0) == 0.
FDB_HD int fdb_find(const FdbImage* tab, int n, bool by_tile, unsigned idx) {
    int lo = 0, hi = n - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        const unsigned first = (unsigned)(by_tile ? tab[mid].tile0 : tab[mid].blk0);
        if (first <= idx) lo = mid; else hi = mid - 1;
    }
    return lo;
}

struct FdbLayout {
    std::vector<FdbImage> tab;
    long long px = 0, lsq = 0;                           // pixels and lsq bytes of the chunk
    unsigned tiles = 0, blocks = 0;
    int max_extent = 0;                                  // the largest H or W: above 32768 the squared distance is summed in 64 bits
};

// Empty string and L for the images first .. first + n - 1 of shapes ([.][3]: H, W, C), bases counted from `first`; or which image is
// wrong and why ("image i: ...", i counted in the caller's chunk).  Only geometry is judged here.
inline std::string fdb_layout(const int32_t* shapes, int first, int n, FdbLayout& L) {
    L = FdbLayout();
    if (n < 0 || n > FDB_MAX_IMAGES) return "more than " + std::to_string(FDB_MAX_IMAGES) + " images";
    L.tab.resize((size_t)n);
    for (int k = 0; k < n; ++k) {
        const int32_t* s = shapes + 3 * (size_t)(first + k);
        const int H = s[0], W = s[1], C = s[2];
        const std::string who = "image " + std::to_string(first + k) + ": ";
        if (H < 1 || W < 1) return who + "H and W must be at least 1";
        if (C < 2) return who + "the lsq image needs at least 2 channels (the gate reads channels 0 and 1)";
        if ((long long)H * W >= FDB_MAX_PIXELS || (long long)H * W * C >= FDB_MAX_LSQ_BYTES)
            return who + "image too large (H * W must be below 2^31, H * W * C below 2^40)";
        if (L.px + (long long)H * W >= FDB_MAX_PIXELS) return who + "the chunk holds 2^31 pixels or more up to here (split it)";
        if (L.lsq + (long long)H * W * C >= FDB_MAX_LSQ_BYTES) return who + "the chunk's lsq images hold 2^40 bytes or more up to here (split it)";
        FdbImage& t = L.tab[(size_t)k];
        t.lsq0 = L.lsq; t.px0 = (int32_t)L.px; t.tile0 = (int32_t)L.tiles; t.blk0 = (int32_t)L.blocks;
        t.H = H; t.W = W; t.C = C;
        L.px += (long long)H * W; L.lsq += (long long)H * W * C;
        L.tiles += fdb_tiles(H, W); L.blocks += fdb_blocks(H, W);
        L.max_extent = H > L.max_extent ? H : L.max_extent;
        L.max_extent = W > L.max_extent ? W : L.max_extent;
    }
    return std::string();
}

// ---- the scratch buffer, carved in two parts ---------------------------------------------------------------------------------------
// What the pixel count sizes, carved before the first launch: the label map, the lsq rasters, the flag space / dense cell index with its
// scan blocks, the parents, the two pixel lists (pairs of int32: local row, local column), the table, the per-image status words, the
// plan the host reads back ((n + 1, 2) int32: per image its first cell and its status word, then the chunk's cells) and 4 counters.
struct FdbPixelBufs {
    int32_t* lab; uint8_t* lsq; int32_t* rid; int32_t* blk; int32_t* par; int32_t* flist; int32_t* clist; FdbImage* tab; int32_t* status;
    int32_t* plan; int32_t* misc;
};
inline FdbPixelBufs fdb_pixel_bufs(Carver& c, const FdbLayout& L) {
    const size_t px = (size_t)L.px, n = L.tab.size();
    FdbPixelBufs b;
    b.lab = c.take<int32_t>(px); b.lsq = c.take<uint8_t>((size_t)L.lsq); b.rid = c.take<int32_t>(px); b.blk = c.take<int32_t>((px + 1023) / 1024);
    b.par = c.take<int32_t>(px); b.flist = c.take<int32_t>(px * 2); b.clist = c.take<int32_t>(px * 2); b.tab = c.take<FdbImage>(n);
    b.status = c.take<int32_t>(n); b.plan = c.take<int32_t>((n + 1) * 2); b.misc = c.take<int32_t>(4);
    return b;
}
// ... and what the cell count sizes, carved behind it once the plan has been read back: accumulators (4 uint32), label value, image,
// list offsets and cursors (2 + 2 int32) and record (8 int64) per cell, and `partials` (cell, slice) minima and root counts.
struct FdbCellBufs { unsigned* acc; int32_t* val; int32_t* img; int32_t* off; int32_t* cur; int64_t* rec; unsigned long long* pbest; int32_t* proots; };
inline FdbCellBufs fdb_cell_bufs(Carver& c, size_t cells, size_t partials) {
    FdbCellBufs b;
    b.acc = c.take<unsigned>(cells * 4); b.val = c.take<int32_t>(cells); b.img = c.take<int32_t>(cells); b.off = c.take<int32_t>(cells * 2);
    b.cur = c.take<int32_t>(cells * 2); b.rec = c.take<int64_t>(cells * 8); b.pbest = c.take<unsigned long long>(partials);
    b.proots = c.take<int32_t>(partials);
    return b;
}

// The byte counts of the two restated slot by slot, every slot rounded up to 256 bytes (scratch.h); the driver and the host check
// compare them with what the Carver measures.
inline long long fdb_round256(long long b) { return b ? (b + 255) / 256 * 256 : 256; }
inline long long fdb_pixel_bytes(long long px, long long lsq, long long n) {
    return 3 * fdb_round256(px * 4) + fdb_round256(lsq) + fdb_round256((px + 1023) / 1024 * 4) + 2 * fdb_round256(px * 8) +
           fdb_round256(n * (long long)sizeof(FdbImage)) + fdb_round256(n * 4) + fdb_round256((n + 1) * 8) + fdb_round256(16);
}
inline long long fdb_pixel_bytes(const FdbLayout& L) { return fdb_pixel_bytes(L.px, L.lsq, (long long)L.tab.size()); }
inline long long fdb_cell_bytes(long long cells, long long partials) {
    return fdb_round256(cells * 16) + 2 * fdb_round256(cells * 4) + 2 * fdb_round256(cells * 8) + fdb_round256(cells * 64) +
           fdb_round256(partials * 8) + fdb_round256(partials * 4);
}
// The cells a group can hold at most where the caller has room for `capacity` records: above either the call writes no record.  The
// second part is measured for this many before the first launch, so that the buffer never grows while the first part is in use.
inline long long fdb_cell_bound(long long px, int capacity) { return px < capacity ? px : (long long)capacity; }
inline long long fdb_group_bytes(long long px, long long lsq, long long n, int capacity) {
    const long long cells = fdb_cell_bound(px, capacity);
    return fdb_pixel_bytes(px, lsq, n) + fdb_cell_bytes(cells, cells + FDB_SLICE_BUDGET);
}
inline long long fdb_group_bytes(const FdbLayout& L, int capacity) { return fdb_group_bytes(L.px, L.lsq, (long long)L.tab.size(), capacity); }

// ---- the groups -------------------------------------------------------------------------------------------------------------------
// Consecutive images go into one group while its scratch stays within `limit`; an image above it alone is a group of its own.  The
// chunk's own limits (fdb_layout over all images) have been checked by the caller.
struct FdbGroup { int first, n; };
inline std::vector<FdbGroup> fdb_groups(const int32_t* shapes, int n, int capacity, long long limit = FDB_SCRATCH_LIMIT) {
    std::vector<FdbGroup> out;
    int i = 0;
    while (i < n) {
        FdbGroup g{i, 0};
        long long px = 0, lsq = 0;
        while (g.first + g.n < n) {
            const int32_t* s = shapes + 3 * (size_t)(g.first + g.n);
            const long long p = (long long)s[0] * s[1];
            if (g.n > 0 && fdb_group_bytes(px + p, lsq + p * s[2], g.n + 1, capacity) > limit) break;
            px += p; lsq += p * s[2]; g.n += 1;
        }
        out.push_back(g);
        i += g.n;
    }
    return out;
}

}  // namespace ecseg
