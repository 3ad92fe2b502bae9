// Host-only: the TIFF parser of the native reader (parse_tiff, host_io.cpp) for the drivers, as tiff_frame.h serves the encoder: the
// device reader (ecseg_tiff_decode, drivers_files.hip) reads the same tags by the same rules as ecseg_tiff_info / ecseg_tiff_read, and
// the one rule that says which files it takes.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <vector>

#include "../../include/ecseg_hip.h"

namespace ecseg {

struct TiffInfo {
    uint32_t W = 0, H = 0, bits = 8, spp = 1, comp = 1, planar = 1, pred = 1, fmt = 1, rps = 0;
    uint32_t tw = 0, th = 0;         // a tiled file's TileWidth and TileLength (0: strips); off and cnt are then its tile tables
    std::vector<uint32_t> off, cnt;
    bool le = true;
};

// ECSEG_OK, ECSEG_E_UNSUPPORTED (a valid layout this reader leaves to the Python one) or ECSEG_E_INVALID (corrupt).
// kinds: the ECSEG_TIFF_* word of include/ecseg_hip.h, here and in every function below: which kinds of file the caller takes beside
// LZW and uncompressed strips (the device reader: ecseg_ctx::tiff_kinds, the three tiff_*_on_device options).  0: the host reader.
// Without ECSEG_TIFF_TILED a file with TileWidth (tag 322) is ECSEG_E_UNSUPPORTED and its tile tags are not read.  With it
// (the option tiff_tiled_on_device): tags 322 to 325 are read and the file is taken (t->tw != 0) when both tile extents are
// positive multiples of 16 of at most TIFF_TILE_MAX_EXTENT, it has no strip tags, and both tile tables have an entry for each of its
// ceil(H / th) * ceil(W / tw) tiles; sample size, format, planarity, compression and predictor are held to the rules of strips.  Every
// other tiled file stays ECSEG_E_UNSUPPORTED.
// Without ECSEG_TIFF_PACKBITS a PackBits file (compression 32773) is ECSEG_E_UNSUPPORTED, as it is for the host reader.  With it
// (the option tiff_packbits_on_device): it is taken, held to every other rule of strips and of tiles.  ECSEG_TIFF_DEFLATE is not the
// parser's: Deflate files parse for the host reader too, and tiff_decode_verdict (drivers_files.hip) refuses them without the bit.
constexpr uint32_t TIFF_TILE_MAX_EXTENT = 1u << 20;
int parse_tiff(const uint8_t* buf, size_t n, TiffInfo* t, unsigned kinds = 0);

// Where row r of tile `tile` of a tiled image goes: tiles lie row-major, `across` = ceil(W / tw) per row of tiles, and those on the
// right and bottom edges are padded to the full tile.  -> the raster row, the first pixel column, and of the tile row's tw * px bytes
// how many are kept (those of pixels inside the image) and how many are dropped as padding; a row below the image keeps nothing.  One
// plain function for tiffb_untile_kernel and for the host check (tools/asan/tiff_tiles_check.cpp).  H, W, tw, th at most 2^20, px the
// bytes of a pixel.
struct TileGeom { uint32_t H, W, th, tw, px; };
struct TilePlace { uint32_t row, col, keep, drop; };
#ifdef __HIPCC__
__host__ __device__
#endif
inline TilePlace tile_place(const TileGeom& g, uint32_t tile, uint32_t r) {
    const uint32_t across = (g.W + g.tw - 1) / g.tw, ty = tile / across, tx = tile - ty * across;
    TilePlace p;
    p.row = ty * g.th + r;
    p.col = tx * g.tw;
    const uint32_t cols = g.W - p.col < g.tw ? g.W - p.col : g.tw;           // (col < W: tx < across)
    p.keep = (r < g.th && p.row < g.H) ? cols * g.px : 0u;
    p.drop = g.tw * g.px - p.keep;
    return p;
}

// The routing rule of the device reader, the only place that decides whether a file goes to the device (ecseg_tiff_decode_routes
// asks it for image_io.imread; ecseg_tiff_decode itself decodes whatever it is given).  A strip is one serial LZW stream on one
// wave, about 0.8 us per decoded byte on noisy data against 2.6 ns on a host core: the device wins by the number of strips that
// decode at once.  The threshold is the measurement of DESIGN.md 5.9 (tools/time_tiff_decode.py, a 1040 x 1392 RGB scene): the
// device call is faster than ecseg_tiff_read at 1040 strips (3.8 against 11.2 ms) and slower at 208 (14.0 against 11.1 ms), at 70, at
// 17 and at 1; 1040 is the smallest count measured at which it wins.  Uncompressed strips lose on the device (6.9 against 1.3 ms:
// the copies to and from the device cost more than the host's one memcpy): they stay on the host.
//   Deflate strips (compression 8 and 32946; tiffb_inflate_kernel) count only for a caller that asks (ECSEG_TIFF_DEFLATE: the handle
// option tiff_deflate_on_device is on) and only from the thresholds below on, which are the Deflate tables of
// DESIGN.md 5.9 (tools/time_tiff_decode.py --deflate): the smallest measured strip counts at which the device call's maximum is
// below ecseg_tiff_read's minimum (TIFF_DEFLATE_NEVER would say that no measured cell wins: then only an explicit ecseg_tiff_decode /
// ecseg_tiff_decode_batch call decodes a Deflate file on the device).  Measured 2026-10-20 on the 1040 x 1392 RGB scene, zlib level 6:
// a single file wins at 1040 strips (4.73 ms, at most 5.01, against at least 15.66 of the host) and loses at 208 (14.48 against 14.15)
// and at 70 (42.56 against 14.18); of the sets, those of 70, 140 and 208 strips lose and every measured set from 280 strips up wins
// (280: four files of 70 strips, at most 51.29 ms against at least 54.92), the stat_fish pairs (1248 strips per image) included.
//   Tiled files (TiffInfo::tw != 0; tiffb_untile_kernel) count only for a caller that asks (ECSEG_TIFF_TILED: the handle option
// tiff_tiled_on_device is on) and only from a measured tile count on.  The table of DESIGN.md 5.9
// (tools/time_tiff_decode.py --tiled) is NOT MEASURED yet: both thresholds are TIFF_TILED_NEVER, the rule answers 0 for every tiled
// file and set, and only an explicit ecseg_tiff_decode / ecseg_tiff_decode_batch call decodes one on the device.
//   PackBits files (compression 32773; tiffb_packbits_kernel) parse only for a caller that asks (ECSEG_TIFF_PACKBITS: the handle
// option tiff_packbits_on_device) and have no table at all (tools/time_tiff_decode.py --packbits is NOT MEASURED): no
// rule here names their compression, so they count in none, strips or tiles, and only an explicit call decodes one on the device.
constexpr size_t TIFF_DEVICE_MIN_STRIPS = 1040;
constexpr size_t TIFF_TILED_NEVER = ~(size_t)0;
constexpr size_t TIFF_TILED_DEVICE_MIN_TILES = TIFF_TILED_NEVER;
constexpr size_t TIFF_TILED_BATCH_DEVICE_MIN_TILES = TIFF_TILED_NEVER;
inline size_t tiff_tile_count(const TiffInfo& t) { return t.tw ? (size_t)((t.H + t.th - 1) / t.th) * ((t.W + t.tw - 1) / t.tw) : 0; }
inline bool tiff_tiled_counts(const TiffInfo& t, unsigned kinds, size_t threshold) {
    return (kinds & ECSEG_TIFF_TILED) && threshold != TIFF_TILED_NEVER && (t.comp == 5 || ((kinds & ECSEG_TIFF_DEFLATE) && (t.comp == 8 || t.comp == 32946))) &&
           t.off.size() >= tiff_tile_count(t) && t.cnt.size() >= tiff_tile_count(t);
}
constexpr size_t TIFF_DEFLATE_NEVER = ~(size_t)0;
constexpr size_t TIFF_DEFLATE_DEVICE_MIN_STRIPS = 1040;
constexpr size_t TIFF_DEFLATE_BATCH_DEVICE_MIN_STRIPS = 280;
inline bool tiff_is_deflate(const TiffInfo& t) { return t.comp == 8 || t.comp == 32946; }
inline bool tiff_goes_to_device(const TiffInfo& t, unsigned kinds) {
    if (t.tw) return tiff_tiled_counts(t, kinds, TIFF_TILED_DEVICE_MIN_TILES) && tiff_tile_count(t) >= TIFF_TILED_DEVICE_MIN_TILES;
    const bool defl = (kinds & ECSEG_TIFF_DEFLATE) && tiff_is_deflate(t);
    if ((t.comp != 5 && !defl) || t.rps == 0) return false;
    const size_t nstrips = ((size_t)t.H + t.rps - 1) / t.rps;
    return nstrips >= (defl ? TIFF_DEFLATE_DEVICE_MIN_STRIPS : TIFF_DEVICE_MIN_STRIPS) && t.off.size() >= nstrips;
}

// The routing rule for a set of files that would go in one ecseg_tiff_decode_batch call, the only place that decides it
// (ecseg_tiff_decode_batch_routes asks it for image_io.imread_many).  The strips of different files decode side by side as the strips
// of one file do, so what counts is their sum: the set goes when the LZW strips of its files - those ecseg_tiff_decode accepts,
// whatever their own strip count - are at least TIFF_BATCH_DEVICE_MIN_STRIPS together.  Uncompressed files are never counted (and
// never sent: tiff_batch_counts is false for them), for the reasons above; Deflate files are counted only with ECSEG_TIFF_DEFLATE, their
// strips are summed on their own against TIFF_DEFLATE_BATCH_DEVICE_MIN_STRIPS, and the set goes when either sum reaches its threshold.  The measurement is the batch table of
// DESIGN.md 5.9 (tools/time_tiff_decode.py --batch: 1 to 32 files of the 1040 x 1392 RGB scene at 1, 5 and 15 rows per strip, and the
// stat_fish pair): every measured set of 1040 strips or more is read faster through the device than by ecseg_tiff_read on one core
// (the batch's maximum below the host's minimum), at each of the three plans; so is every measured set from 416 strips up, and the
// sets of 280 strips or fewer lose - the threshold stays at the single-file 1040 here, and lowering it to 416 is the follow-up that
// table supports.  Nothing was measured above 15 rows of 4176 bytes per strip, where a single wave takes 174 ms and more for its
// strip: a file whose strips decode to more than TIFF_BATCH_DEVICE_MAX_STRIP_BYTES is not counted either.  files: the parsed files that
// ecseg_tiff_decode accepts.
constexpr size_t TIFF_BATCH_DEVICE_MIN_STRIPS = 1040;
constexpr unsigned long long TIFF_BATCH_DEVICE_MAX_STRIP_BYTES = 15ull * 1392 * 3;
inline bool tiff_batch_counts(const TiffInfo& t, unsigned kinds) {
    if (t.tw) return tiff_tiled_counts(t, kinds, TIFF_TILED_BATCH_DEVICE_MIN_TILES);
    const bool defl = (kinds & ECSEG_TIFF_DEFLATE) && tiff_is_deflate(t) && TIFF_DEFLATE_BATCH_DEVICE_MIN_STRIPS != TIFF_DEFLATE_NEVER;
    if ((t.comp != 5 && !defl) || t.rps == 0 || t.H == 0) return false;
    const size_t nstrips = ((size_t)t.H + t.rps - 1) / t.rps;
    return t.off.size() >= nstrips &&                        // (a strip table shorter than the image stays on the host, as in the single-file rule)
           (unsigned long long)(t.rps < t.H ? t.rps : t.H) * t.W * t.spp * (t.bits / 8) <= TIFF_BATCH_DEVICE_MAX_STRIP_BYTES;
}
// Tiled files (with ECSEG_TIFF_TILED) are summed by tiles, on their own, against TIFF_TILED_BATCH_DEVICE_MIN_TILES.
inline bool tiff_batch_goes_to_device(const TiffInfo* const* files, size_t n, unsigned kinds) {
    size_t strips = 0, deflate_strips = 0, tiles = 0;
    for (size_t i = 0; i < n; ++i) {
        if (!tiff_batch_counts(*files[i], kinds)) continue;
        if (files[i]->tw) tiles += tiff_tile_count(*files[i]);
        else (tiff_is_deflate(*files[i]) ? deflate_strips : strips) += ((size_t)files[i]->H + files[i]->rps - 1) / files[i]->rps;
    }
    return strips >= TIFF_BATCH_DEVICE_MIN_STRIPS || deflate_strips >= TIFF_DEFLATE_BATCH_DEVICE_MIN_STRIPS ||
           (TIFF_TILED_BATCH_DEVICE_MIN_TILES != TIFF_TILED_NEVER && tiles >= TIFF_TILED_BATCH_DEVICE_MIN_TILES);
}

}  // namespace ecseg
