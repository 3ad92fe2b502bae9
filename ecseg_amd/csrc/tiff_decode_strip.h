// One LZW strip decoded by one wave: the routine of tiffb_unstrip_kernel (tiff_decode_kernels.hip), written so that the host
// compiler takes it too - tools/asan/tiff_decode_fuzz.cpp runs it under ASan + UBSan against ecseg_lzw_decode (host_codec.cpp),
// which is its specification, tolerances included.  Under hipcc a lane is a thread of the wave, td_first is a read of lane 0 and
// td_stores_done the fence + barrier that completes the wave's stores; under the host compiler the lanes are a loop, and the other
// two do nothing.
//
// Lane 0 is the decoder, a serial walk over the codes in plain C++ (as lane 0 of the encoder, tiff_kernels.hip); it stores the
// literals itself.  Every longer string is a copy from the strip's own earlier output (an entry is (offset, length) of an earlier
// occurrence, as on the host) that all 64 lanes make, 64 bytes per step, straight in the raster: output is not held in LDS, one
// table epoch of a constant image covers megabytes.  The table (4096 x offset, length: 24 KB) and TD_IN staged bytes of the
// stream are in LDS.  The table is never cleared: an entry is read only below `next`, as on the host.
//   Lanes read global bytes that other lanes (and lane 0's literal stores) have written.  The wave keeps a watermark `fenced`: the
// output offset below which every store is known to have completed.  A copy whose source reaches beyond it first runs
// td_stores_done (workgroup-scope release + acquire around a barrier, which drains the wave's stores: vmcnt(0)) and moves the
// watermark to its own destination; a copy from older output - most of them: an entry points anywhere into its epoch - pays nothing.
//   An overlapping copy (KwKwK: the previous string + its own first byte, distance = the previous length) never reads what it
// writes: byte k >= distance is byte k - distance of the source, which is byte 0.
//   Every index is checked where it is used: into the staged bytes against the staged count, into the stream against `have`,
// into the table by the code's 12 bits and `next`, into the output against `want`.
#pragma once
#include <stdint.h>

#include "tiff_decode_batch.h"

#ifdef __HIPCC__
#define TD_FN __device__ __forceinline__
#define TD_FOR_LANES(lane) for (int lane = (int)threadIdx.x, td_once_ = 1; td_once_; td_once_ = 0)
#define TD_CONTROL_LANE if (threadIdx.x == 0)
TD_FN uint32_t td_first(uint32_t v) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)v); }
TD_FN void td_stores_done() { __syncthreads(); }
#else
#define TD_FN inline
#define TD_FOR_LANES(lane) for (int lane = 0; lane < 64; ++lane)
#define TD_CONTROL_LANE
inline uint32_t td_first(uint32_t v) { return v; }
inline void td_stores_done() {}
#endif

namespace ecseg {

constexpr uint32_t TD_IN = 1024;                             // staged bytes of the code stream
struct TdLds { uint32_t pos[4096]; uint16_t len[4096]; uint8_t in[TD_IN]; };   // (a string is at most 3839 bytes: one more than an earlier one per entry)

enum { TD_REFILL = 0, TD_COPY = 1, TD_END = 2, TD_CORRUPT = 3 };
// lane 0's registers: the host decoder's state (careful form) and the copy it asks the wave for
struct TdWalk { uint32_t racc; int nbits, width, next, old; uint32_t ipos, out, old_pos, old_len, c_src, c_len, c_dst; int full; };

// Walks the codes until the wave has something to do: stage the next bytes (TD_REFILL), copy a string (TD_COPY), or stop.  The staged
// bytes are those of [c0, c0 + cn) of the stream.
TD_FN int td_walk(TdWalk& s, TdLds& L, uint32_t have, uint32_t c0, uint32_t cn, uint8_t* dst, uint32_t want) {
    if (s.full) return TD_END;                               // the copy before filled the destination
    for (;;) {
        while (s.nbits < s.width) {
            if (s.ipos >= have) return TD_END;               // stream ended without EOI: accept what we have
            if (s.ipos - c0 >= cn) return TD_REFILL;         // (unsigned: an ipos below c0 asks for a refill too)
            s.racc = (s.racc << 8) | L.in[s.ipos - c0];
            ++s.ipos;
            s.nbits += 8;
        }
        const int code = (int)((s.racc >> (s.nbits - s.width)) & ((1u << s.width) - 1));
        s.nbits -= s.width;
        if (code == 257) return TD_END;
        if (code == 256) { s.next = 258; s.width = 9; s.old = -1; continue; }
        if (s.old < 0) {                                     // behind a ClearCode, or the first code of a stream without one: a literal, no entry
            if (code >= 256) return TD_CORRUPT;
            if (s.out >= want) return TD_END;
            s.old_pos = s.out; s.old_len = 1; s.old = code;
            dst[s.out++] = (uint8_t)code;
            continue;
        }
        uint32_t cpos = 0, clen = 1;                         // the string of `code`
        if (code < s.next) {
            if (code >= 256) { cpos = L.pos[code]; clen = L.len[code]; }
        } else if (code == s.next && s.next < 4096) {       // KwKwK: previous string + its own first byte
            cpos = s.old_pos; clen = s.old_len + 1;
        } else {
            return TD_CORRUPT;
        }
        const uint32_t start = s.out, room = want - s.out;
        const uint32_t ncopy = clen <= room ? clen : room;
        const bool wave = code >= 256 && ncopy > 0;
        if (code < 256) { if (ncopy) dst[s.out] = (uint8_t)code; }
        else { s.c_src = cpos; s.c_len = ncopy; s.c_dst = start; }
        s.out += ncopy;
        if (s.next < 4096) { L.pos[s.next] = s.old_pos; L.len[s.next] = (uint16_t)(s.old_len + 1); ++s.next; }
        if (ncopy < clen) {                                  // destination full
            if (!wave) return TD_END;
            s.full = 1;
            return TD_COPY;
        }
        s.old = code; s.old_pos = start; s.old_len = clen;
        if (s.next >= (1 << s.width) - 1 && s.width < 12) ++s.width;     // early change
        if (wave) return TD_COPY;
    }
}

// src: the strip's `have` bytes; dst: its `want` bytes of the raster (want below 2^31).  Returns 0, or 1 for a corrupt stream
// (the same value in every lane); bytes the stream does not give are zero.
TD_FN uint32_t td_lzw_strip(const uint8_t* src, uint32_t have, uint8_t* dst, uint32_t want, TdLds& L) {
    TdWalk s{0u, 0, 9, 258, -1, 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0};
    uint32_t c0 = 0, cn = 0, fenced = 0;
    int cmd;
    for (;;) {
        cmd = TD_END;
        TD_CONTROL_LANE { cmd = td_walk(s, L, have, c0, cn, dst, want); }
        cmd = (int)td_first((uint32_t)cmd);
        if (cmd == TD_REFILL) {
            c0 = td_first(s.ipos);
            cn = c0 < have ? (have - c0 < TD_IN ? have - c0 : TD_IN) : 0u;
            TD_FOR_LANES(lane) {
                for (uint32_t k = (uint32_t)lane; k < cn; k += 64) L.in[k] = src[c0 + k];
            }
            td_stores_done();                                // (the barrier the staged bytes need completes the output stores too)
            fenced = td_first(s.out);
        } else if (cmd == TD_COPY) {
            const uint32_t c_src = td_first(s.c_src), c_len = td_first(s.c_len), c_dst = td_first(s.c_dst);
            const uint32_t dist = c_dst - c_src;             // >= 1: a string lies before the place it is copied to
            const uint32_t reach = c_len < dist ? c_len : dist;
            if (c_src + reach > fenced) { td_stores_done(); fenced = c_dst; }
            TD_FOR_LANES(lane) {
                for (uint32_t k = (uint32_t)lane; k < c_len; k += 64) {
                    const uint32_t from = c_src + (k >= dist ? k - dist : k), to = c_dst + k;
                    if (from < want && to < want) dst[to] = dst[from];
                }
            }
        } else {
            break;
        }
    }
    const uint32_t got = td_first(s.out);
    TD_FOR_LANES(lane) {
        for (uint32_t k = got + (uint32_t)lane; k < want; k += 64) dst[k] = 0;
    }
    return cmd == TD_CORRUPT ? 1u : 0u;
}

// ---- a strip's place in its file and its raster; the uncompressed strip; the same for a strip of a batch --------------------------
struct TdStrip { const uint8_t* src; uint8_t* dst; uint32_t have, want; bool in_table, behind_file; };

// Strip `strip` of a file: rows [strip * rps, ...) of the raster, bytes [off, off + min(cnt, n - off)) of the file.
TD_FN TdStrip td_strip(uint32_t strip, const uint8_t* file, unsigned long long n, const uint32_t* offs, const uint32_t* cnts, uint32_t n_table,
                       uint32_t H, unsigned long long line, uint32_t rps, uint8_t* raster) {
    const unsigned long long r0 = (unsigned long long)strip * rps;
    TdStrip t{file, raster, 0u, 0u, false, false};
    if (r0 >= H) return t;                                   // (the grid has ceil(H / rps) strips: never)
    const unsigned long long rows = r0 + rps <= H ? rps : H - r0;
    t.want = (uint32_t)(rows * line);                        // (below 2^31: the driver refuses longer strips)
    t.dst = raster + r0 * line;
    if (strip >= n_table) return t;
    t.in_table = true;
    const unsigned long long off = offs[strip], cnt = cnts[strip];
    if (off > n) { t.behind_file = true; return t; }
    t.src = file + off;
    t.have = (uint32_t)(cnt < n - off ? cnt : n - off);
    return t;
}

// Tile k of a tiled file: its stream in the file and, for a compressed tile, its staging slot.  The stream is clamped to the file as
// the Python reader's slice buf[off:off + cnt] is - an offset behind the file is an empty stream, not an error of its own: an LZW or
// uncompressed tile of no bytes is zeros, a Deflate one a short stream.
TD_FN uint32_t td_tile_stream(uint32_t k, const TdFile& f, const uint32_t* tables, unsigned long long* at) {
    const unsigned long long off = tables[f.table_off + k], cnt = tables[f.table_off + f.n_table + k];
    *at = off < f.n_bytes ? off : f.n_bytes;
    return (uint32_t)(cnt < f.n_bytes - *at ? cnt : f.n_bytes - *at);        // (below 2^32: the counts are 32-bit)
}
TD_FN TdStrip td_tile(uint32_t k, const TdFile& f, const TdTiles& tt, const uint8_t* files, const uint32_t* tables, uint8_t* staging) {
    const unsigned long long tile_bytes = (unsigned long long)tt.th * tt.tw * f.spp * f.bps;      // (below 2^31: the driver refuses larger tiles)
    unsigned long long at = 0;
    const uint32_t have = td_tile_stream(k, f, tables, &at);
    return TdStrip{files + f.file_off + at, staging + tt.stage_off + k * tile_bytes, have, (uint32_t)tile_bytes, true, false};
}

// An uncompressed strip: a clamped copy and the zero fill, by `nlanes` lanes (the threads of the workgroup).
TD_FN void td_raw_strip(const TdStrip& t, uint32_t nlanes) {
    const uint32_t got = t.have < t.want ? t.have : t.want;
    TD_FOR_LANES(lane) {
        for (uint32_t k = (uint32_t)lane; k < t.want; k += nlanes) t.dst[k] = k < got ? t.src[k] : (uint8_t)0;
    }
}

// The file of global strip (rows == false) or row (rows == true) `idx` of a batch: the last row of the table that starts at or
// before it.  Files of zero strips share their start with the file behind them and are never the last such row, except at the
// table's end, which no index reaches.  n >= 1.
TD_FN uint32_t td_find_file(const TdFile* tab, uint32_t n, uint32_t idx, bool rows) {
    uint32_t lo = 0, hi = n;
    while (hi - lo > 1) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if ((rows ? tab[mid].first_row : tab[mid].first_strip) <= idx) lo = mid; else hi = mid;
    }
    return lo;
}

// Global strip `strip` of a batch, by one wave: td_lzw_strip or td_raw_strip on the strip's file.  Returns its status word (0, or 1:
// corrupt stream / offset behind the file), the same in every lane; TD_OTHER_KERNEL for a Deflate strip (tdb_inflate, tiff_inflate_strip.h)
// and for a PackBits strip (tdb_packbits, tiff_packbits_strip.h).
// tiles, staging: the tiled-file table and the staging slots of a batch that has tiled files (else no row of tab points there).
TD_FN uint32_t tdb_unstrip(const TdFile* tab, uint32_t n_files, const uint8_t* files, const uint32_t* tables, uint8_t* rasters, uint32_t strip,
                           TdLds& L, const TdTiles* tiles = nullptr, uint8_t* staging = nullptr) {
    const TdFile& f = tab[td_first(td_find_file(tab, n_files, strip, false))];
    if (f.codec == TD_DEFLATE || f.codec == TD_PACKBITS) return TD_OTHER_KERNEL;
    const uint32_t k = strip - f.first_strip;
    if (f.tiles) {                                           // a tile: an LZW stream into its slot; an uncompressed one is tiffb_untile_kernel's alone
        if (!f.in_batch || k >= f.n_table || f.codec != TD_LZW) return 0u;
        const TdStrip t = td_tile(k, f, tiles[f.tiles - 1], files, tables, staging);
        return td_lzw_strip(t.src, t.have, t.dst, t.want, L);
    }
    if (!f.in_batch || (unsigned long long)k * f.rps >= f.H) return 0u;      // (the grid has the strips of the table: never)
    const uint32_t* offs = tables + f.table_off;
    const TdStrip t = td_strip(k, files + f.file_off, f.n_bytes, offs, offs + f.n_table, f.n_table, f.H, f.line, f.rps, rasters + f.raster_off);
    uint32_t st = 0;
    if (f.codec == TD_LZW) st = td_lzw_strip(t.src, t.have, t.dst, t.want, L);           // (have == 0: nothing is read, the strip is zeros)
    else td_raw_strip(t, 64u);
    return t.behind_file ? 1u : st;
}

}  // namespace ecseg
