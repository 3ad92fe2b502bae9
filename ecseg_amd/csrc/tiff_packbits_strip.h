// One PackBits strip (TIFF compression 32773) decoded by one wave: the routine of tiffb_packbits_kernel (tiff_decode_kernels.hip),
// written like td_lzw_strip (tiff_decode_strip.h, whose lane macros, td_first and td_stores_done it uses) so that the host compiler
// takes it too - tools/asan/tiff_packbits_fuzz.cpp runs it under ASan + UBSan against a plain byte loop.  Its specification is
// image_io._packbits_decode(data, expected), the only PackBits reader there is (the host reader leaves such files to it), leniencies
// included.  A header byte h, then: h < 128: the next h + 1 bytes as they are; h > 128: the next byte 257 - h times; h == 128:
// nothing.  And, as that function has it:
//   - the walk stops at the stream's end or once the strip is full, whichever comes first: bytes left over are never looked at;
//   - a literal run that the stream ends in gives the bytes there are, a repeat header that is the stream's last byte gives none;
//   - a run that would pass the strip's end is cut there;
//   - what the stream does not give is zeros.
// That function raises for no stream, so no PackBits stream is corrupt: the status word is always 0.
//
// The header walk is serial, and every lane makes it: header and counters are the same in all of them (the header is read from LDS
// at one address and passed through td_first, so the walk is scalar code and scalar branches), and no lane waits for a control lane.
// The bytes of a run, 128 at the most, are written by the lanes, one byte each per step of 64, straight in the raster; nothing that
// was written is read again, so no store needs a fence.  TP_IN bytes of the stream are staged in LDS, from a header on: a header
// whose run (TP_RUN bytes and the header itself) the staged bytes do not hold to its end, or to the stream's, has the wave stage
// the stream again from that header, so that a run is always copied out of LDS.
//   Every index is checked where it is used: into the staged bytes against the staged count, into the stream against `have`, into
// the output against `want`.
#pragma once
#include <stdint.h>

#include "tiff_decode_strip.h"

namespace ecseg {

constexpr uint32_t TP_IN = 1024;                             // staged bytes of the stream
constexpr uint32_t TP_RUN = 128;                             // the longest run
struct TpLds { uint8_t in[TP_IN]; };

// src: the strip's `have` bytes; dst: its `want` bytes of the raster (want below 2^31).  Returns 0 (no PackBits stream is corrupt:
// see above), the same value in every lane; bytes the stream does not give are zero.
TD_FN uint32_t tp_packbits_strip(const uint8_t* src, uint32_t have, uint8_t* dst, uint32_t want, TpLds& L) {
    uint32_t i = 0, out = 0, c0 = 0, cn = 0;                 // the staged bytes are those of [c0, c0 + cn) of the stream
    while (i < have && out < want) {
        const uint32_t need = have - i < TP_RUN + 1 ? have - i : TP_RUN + 1;
        if (i - c0 > cn || cn - (i - c0) < need) {           // (unsigned: an i below c0 asks for the bytes too)
            c0 = i;
            cn = have - c0 < TP_IN ? have - c0 : TP_IN;
            td_stores_done();                                // (every lane has read what it wanted of the bytes staged before)
            TD_FOR_LANES(lane) {
                for (uint32_t k = (uint32_t)lane; k < cn; k += 64) L.in[k] = src[c0 + k];
            }
            td_stores_done();
        }
        const uint32_t at = i - c0;                          // of the header in the staged bytes: below cn (need >= 1)
        const uint32_t h = td_first(at < cn ? L.in[at] : 128u);
        ++i;
        if (h < 128) {                                       // h + 1 literal bytes, as many of them as the stream has
            const uint32_t run = h + 1, got = run < have - i ? run : have - i, n = got < want - out ? got : want - out;
            TD_FOR_LANES(lane) {
                for (uint32_t k = (uint32_t)lane; k < n; k += 64)
                    if (at + 1 + k < cn) dst[out + k] = L.in[at + 1 + k];
            }
            out += n; i += got;
        } else if (h > 128) {                                // the next byte 257 - h times, if the stream has one
            if (i >= have) break;
            const uint32_t v = td_first(at + 1 < cn ? L.in[at + 1] : 0u);
            const uint32_t run = 257 - h, n = run < want - out ? run : want - out;
            TD_FOR_LANES(lane) {
                for (uint32_t k = (uint32_t)lane; k < n; k += 64) dst[out + k] = (uint8_t)v;
            }
            out += n; ++i;
        }
    }
    TD_FOR_LANES(lane) {
        for (uint32_t k = out + (uint32_t)lane; k < want; k += 64) dst[k] = 0;
    }
    return 0u;
}

// Global strip `strip` of a batch, by one wave, when its file holds PackBits strips: the status word (0, or 1: offset behind the
// file), the same in every lane; TD_OTHER_KERNEL for a strip of tdb_unstrip's or tdb_inflate's.  A strip the tables do not have is an
// empty stream: zeros.
TD_FN uint32_t tdb_packbits(const TdFile* tab, uint32_t n_files, const uint8_t* files, const uint32_t* tables, uint8_t* rasters, uint32_t strip,
                            TpLds& L, const TdTiles* tiles = nullptr, uint8_t* staging = nullptr) {
    const TdFile& f = tab[td_first(td_find_file(tab, n_files, strip, false))];
    if (f.codec != TD_PACKBITS) return TD_OTHER_KERNEL;
    const uint32_t k = strip - f.first_strip;
    if (f.tiles) {                                           // a tile: its stream into its slot (td_tile: an offset behind the file is an empty stream)
        if (!f.in_batch || k >= f.n_table) return 0u;
        const TdStrip t = td_tile(k, f, tiles[f.tiles - 1], files, tables, staging);
        return tp_packbits_strip(t.src, t.have, t.dst, t.want, L);
    }
    if (!f.in_batch || (unsigned long long)k * f.rps >= f.H) return 0u;      // (the grid has the strips of the table: never)
    const uint32_t* offs = tables + f.table_off;
    const TdStrip t = td_strip(k, files + f.file_off, f.n_bytes, offs, offs + f.n_table, f.n_table, f.H, f.line, f.rps, rasters + f.raster_off);
    const uint32_t st = tp_packbits_strip(t.src, t.have, t.dst, t.want, L);  // (have == 0: nothing is read, the strip is zeros)
    return t.behind_file ? 1u : st;
}

}  // namespace ecseg
