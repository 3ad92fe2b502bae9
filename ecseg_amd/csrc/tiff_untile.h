// One raster row of a tiled TIFF file put in its place by one wave: the routines of tiffb_untile_kernel (tiff_decode_kernels.hip),
// written like td_lzw_strip (tiff_decode_strip.h, whose lane macros they use) so that the host compiler takes them too -
// tools/asan/tiff_tiles_check.cpp walks them under ASan + UBSan against a naive untile.  What image_io.read_tiff does per tile -
// view the tile's bytes in the file's byte order, undo the horizontal predictor along each row of the TILE, keep the part inside the
// image - seen from the raster row: row y of the image is row r = y mod th of the tiles of tile row ty = y / th, side by side, the
// last of them cut at the image's right edge (tile_place, tiff_parse.h, says what of a tile row is kept).
//   The source of a tile row is its staging slot (compressed tiles: the decoders filled all of it) or the file image itself
// (uncompressed tiles, clamped to the file as the Python reader's slice is: bytes the file does not have are zeros).
//   ut_copy_row (no predictor): the raster row in chunks of sizeof(V) bytes, 16 or 4.  A tile row is a multiple of 16 bytes (tw is
// one of 16 pixels), so a chunk lies in one tile; it is one vector load and store where it is whole and both addresses are aligned
// - always for a staged tile and a raster row on 16 bytes - and single bytes else (the row's tail, a file image at an odd place).
// 16-bit samples of the other byte order are swapped in the vector.
//   ut_predict_row (predictor 2): per sample channel an inclusive scan over 64 pixels that restarts at every tile's first column -
// a lane adds the lane d below while that lane is in its tile - with a carry into the next 64 for a tile that goes on there
// (tile widths that do not divide 64); sums are modulo 2^8 or 2^16.  Samples are read byte by byte, in the file's order.
// Nothing is staged in LDS.
#pragma once
#include <stdint.h>

#include "tiff_decode_strip.h"
#include "tiff_parse.h"

namespace ecseg {

struct alignas(16) UtV16 { uint32_t w[4]; };
struct UtRow { const uint8_t* p; uint32_t avail; };         // row r of a tile: where its bytes lie and how many of them exist

TD_FN UtRow ut_tile_row(const TdFile& f, const TdTiles& tt, const uint8_t* files, const uint32_t* tables, const uint8_t* staging, uint32_t k,
                        uint32_t r) {
    const uint32_t B = tt.tw * f.spp * f.bps;
    const unsigned long long in_tile = (unsigned long long)r * B;
    if (f.codec != TD_RAW) return UtRow{staging + tt.stage_off + (unsigned long long)k * tt.th * B + in_tile, B};
    unsigned long long at = 0;
    const unsigned long long have = td_tile_stream(k, f, tables, &at);
    const unsigned long long left = have > in_tile ? have - in_tile : 0;
    return UtRow{files + f.file_off + at + (left ? in_tile : 0), (uint32_t)(left < B ? left : B)};
}

// Row r of tile row ty -> dst, the raster row ty * th + r (below H), without a predictor.  V: UtV16 or uint32_t.
template <typename V>
TD_FN void ut_copy_row(const TdFile& f, const TdTiles& tt, const uint8_t* files, const uint32_t* tables, const uint8_t* staging, uint32_t ty, uint32_t r,
                       uint8_t* dst) {
    const uint32_t C = (uint32_t)sizeof(V), B = tt.tw * f.spp * f.bps, line = (uint32_t)f.line;   // (a row of at most 2^20 pixels of 32 bytes)
    const TileGeom g{f.H, f.W, tt.th, tt.tw, f.spp * f.bps};
    TD_FOR_LANES(lane) {
        for (uint32_t o = (uint32_t)lane * C; o < line; o += 64u * C) {
            const uint32_t tx = o / B, within = o - tx * B, k = ty * tt.across + tx;
            const TilePlace p = tile_place(g, k, r);
            if (within >= p.keep) continue;                  // (never: the row ends with the last tile's kept bytes)
            const uint32_t n = p.keep - within < C ? p.keep - within : C;
            const UtRow row = ut_tile_row(f, tt, files, tables, staging, k, r);
            const uint8_t* s = row.p + (row.avail > within ? within : 0);
            const uint32_t left = row.avail > within ? row.avail - within : 0;
            if (n == C && left >= C && (((uintptr_t)s | (uintptr_t)(dst + o)) & (C - 1)) == 0) {
                V v = *reinterpret_cast<const V*>(s);
                if (f.swap) {
                    uint32_t* w = reinterpret_cast<uint32_t*>(&v);
                    for (uint32_t q = 0; q < C / 4; ++q) w[q] = ((w[q] & 0x00ff00ffu) << 8) | ((w[q] >> 8) & 0x00ff00ffu);
                }
                *reinterpret_cast<V*>(dst + o) = v;
            } else {
                for (uint32_t i = 0; i < n; ++i) {
                    const uint32_t j = f.swap ? i ^ 1u : i;
                    dst[o + i] = j < left ? s[j] : (uint8_t)0;
                }
            }
        }
    }
}

// Sample c of pixel x of the row as the file holds it (x < W), in native order; *col: the pixel's column in its tile.
template <typename T>
TD_FN uint32_t ut_sample(const TdFile& f, const TdTiles& tt, const uint8_t* files, const uint32_t* tables, const uint8_t* staging, uint32_t ty,
                         uint32_t r, uint32_t x, uint32_t c, uint32_t* col) {
    const uint32_t tx = x / tt.tw;
    *col = x - tx * tt.tw;
    const UtRow row = ut_tile_row(f, tt, files, tables, staging, ty * tt.across + tx, r);
    const uint32_t at = (*col * f.spp + c) * (uint32_t)sizeof(T);
    const uint32_t b0 = at < row.avail ? row.p[at] : 0u;
    if (sizeof(T) == 1) return b0;
    const uint32_t b1 = at + 1 < row.avail ? row.p[at + 1] : 0u;
    return f.swap ? (b0 << 8) | b1 : b0 | (b1 << 8);
}

// The same row with the horizontal predictor undone along every tile row.  T: uint8_t or uint16_t, dst aligned to it.
template <typename T>
TD_FN void ut_predict_row(const TdFile& f, const TdTiles& tt, const uint8_t* files, const uint32_t* tables, const uint8_t* staging, uint32_t ty,
                          uint32_t r, T* dst) {
    for (uint32_t c = 0; c < f.spp; ++c) {
        uint32_t carry = 0;
        for (uint32_t x0 = 0; x0 < f.W; x0 += 64) {
#ifdef __HIPCC__
            const uint32_t lane = threadIdx.x, x = x0 + lane;
            uint32_t v = 0, col = 0;                         // (a lane behind the row: its own tile of nothing)
            if (x < f.W) v = ut_sample<T>(f, tt, files, tables, staging, ty, r, x, c, &col);
#pragma unroll
            for (uint32_t d = 1; d < 64; d <<= 1) {
                const uint32_t up = __shfl_up(v, d);
                if (lane >= d && col >= d) v += up;
            }
            if (col > lane) v += carry;                      // the tile began before x0: lane 63 of the 64 before was in it
            carry = __shfl(v, 63);
            if (x < f.W) dst[(size_t)x * f.spp + c] = (T)v;
#else
            uint32_t v[64], up[64], col[64];
            for (uint32_t lane = 0; lane < 64; ++lane) {
                v[lane] = col[lane] = 0;
                if (x0 + lane < f.W) v[lane] = ut_sample<T>(f, tt, files, tables, staging, ty, r, x0 + lane, c, &col[lane]);
            }
            for (uint32_t d = 1; d < 64; d <<= 1) {
                for (uint32_t lane = 0; lane < 64; ++lane) up[lane] = lane >= d ? v[lane - d] : 0u;
                for (uint32_t lane = 0; lane < 64; ++lane) if (lane >= d && col[lane] >= d) v[lane] += up[lane];
            }
            for (uint32_t lane = 0; lane < 64; ++lane) if (col[lane] > lane) v[lane] += carry;
            carry = v[63];
            for (uint32_t lane = 0; lane < 64; ++lane) if (x0 + lane < f.W) dst[(size_t)(x0 + lane) * f.spp + c] = (T)v[lane];
#endif
        }
    }
}

// The tiled file of global tile row `trow`: the last row of the tiled-file table that starts at or before it.  n >= 1.
TD_FN uint32_t ut_find_tiled(const TdTiles* tiles, uint32_t n, uint32_t trow) {
    uint32_t lo = 0, hi = n;
    while (hi - lo > 1) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (tiles[mid].first_trow <= trow) lo = mid; else hi = mid;
    }
    return lo;
}

// Rows part, part + parts, ... of global tile row `trow` of a batch, by one wave.
TD_FN void tdb_untile(const TdFile* tab, const TdTiles* tiles, uint32_t n_tiled, const uint8_t* files, const uint32_t* tables, const uint8_t* staging,
                      uint8_t* rasters, uint32_t trow, uint32_t part, uint32_t parts) {
    const TdTiles& tt = tiles[td_first(ut_find_tiled(tiles, n_tiled, trow))];
    const TdFile& f = tab[tt.file];
    const uint32_t ty = trow - tt.first_trow;
    if (!f.in_batch || !f.tiles || ty >= tt.down) return;    // (the grid has the tile rows of the table: never)
    const uint32_t rows = f.H - ty * tt.th < tt.th ? f.H - ty * tt.th : tt.th;
    for (uint32_t r = part; r < rows; r += parts) {
        uint8_t* dst = rasters + f.raster_off + (size_t)(ty * tt.th + r) * f.line;
        if (f.predictor) {
            if (f.bps == 2) ut_predict_row(f, tt, files, tables, staging, ty, r, reinterpret_cast<uint16_t*>(dst));
            else ut_predict_row(f, tt, files, tables, staging, ty, r, dst);
        } else if (((uintptr_t)dst & 15) == 0) {
            ut_copy_row<UtV16>(f, tt, files, tables, staging, ty, r, dst);
        } else {
            ut_copy_row<uint32_t>(f, tt, files, tables, staging, ty, r, dst);
        }
    }
}

}  // namespace ecseg
