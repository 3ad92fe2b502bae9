// One Deflate strip (TIFF compression 8 / 32946: a zlib stream of its own) decoded by one wave: the routine of tiffb_inflate_kernel
// (tiff_decode_kernels.hip), written like td_lzw_strip (tiff_decode_strip.h, whose lane macros, td_first and td_stores_done it uses)
// so that the host compiler takes it too - tools/asan/tiff_inflate_fuzz.cpp runs it under ASan + UBSan against the host reader's
// rule (ecseg_tiff_read, host_io.cpp: uncompress, then inflate(Z_FINISH) on Z_BUF_ERROR), which is its specification:
//   - a complete stream shorter than the strip is zero-filled; one that gives more than the strip holds is cut at `want` bytes and
//     is OK whatever follows; after exactly `want` bytes the walk goes on while no output byte is needed (empty stored blocks,
//     end-of-block, the trailer): an error or a wrong Adler-32 there is corrupt, running out of input there is OK;
//   - everything zlib calls a data error is corrupt (header, FDICT, block type 3, LEN/NLEN, over-subscribed or incomplete code
//     lengths other than the cases zlib admits, a missing end-of-block code, symbols 286/287, distance codes 30/31, a distance
//     before the strip's first byte, a wrong Adler-32);
//   - a stream that ends before the strip is full and before its own end is corrupt (uncompress from zlib 1.2.9 on).
//
// Lane 0 is the decoder, a serial walk in plain C++; it stores the literals itself.  A match (length 3..258, distance 1..32768) is a
// copy from the strip's own earlier output that all 64 lanes make straight in the raster: there is no window buffer, the window is
// the raster, and byte k of the copy is byte k mod distance of the source, so an overlapping match never reads what it writes.  The
// `fenced` watermark orders the copies as in td_lzw_strip: a copy whose source reaches above it runs td_stores_done first.  A
// stored block's bytes are copied by the wave from the stream itself.  Once the trailer is reached the wave sums Adler-32 over the
// strip's output, a = 1 + sum d, b = n + sum (n - i) d, both mod 65521, in chunks of TI_ADLER bytes that cannot overflow 32 bits.
//   The Huffman tables (puff-style counts and symbols, with a direct table of TI_FAST_L / TI_FAST_D bits in front), the code lengths
// and TI_IN staged bytes of the stream are in LDS (TiLds, 4.5 KB).
//   The walk goes step by step (the zlib header; a block header with its tables; one literal / length + distance; the trailer).  A
// step that finds the staged bytes used up is undone - it has written nothing but LDS it writes again - and the wave stages the
// stream from the step's first byte (TI_REFILL): a step needs 566 bytes at the most, TI_IN holds 1024.  Bits beyond the stream's end
// read as zero, as in zlib's hold, and a code longer than the bits that are left is the end of the input, not a symbol.
//   Every index is checked where it is used: into the staged bytes against the staged count, into the stream against `have`, into
// the tables by the symbol counts, into the output against `want`.
#pragma once
#include <stdint.h>

#include "tiff_decode_strip.h"

#ifdef __HIPCC__
TD_FN uint32_t ti_wave_sum(uint32_t v) {
    for (int d = 32; d >= 1; d >>= 1) v += (uint32_t)__shfl_xor((int)v, d);
    return v;
}
#else
inline uint32_t ti_wave_sum(uint32_t v) { return v; }       // (the lanes are a loop: the sum is made in it)
#endif

namespace ecseg {

constexpr uint32_t TI_IN = 1024;                             // staged bytes of the stream
constexpr int TI_FAST_L = 9, TI_FAST_D = 7, TI_FAST_C = 7;   // bits of the direct tables: literal/length, distance, code lengths
constexpr uint32_t TI_ADLER = 4096;                          // bytes per Adler chunk: 64 per lane, weights up to 4096: below 2^27 per lane
struct TiCode { uint16_t cnt[16]; uint16_t max; };           // codes per length; the longest length in use
struct TiLds {
    uint16_t fast_l[1 << TI_FAST_L], fast_d[1 << TI_FAST_D], fast_c[1 << TI_FAST_C];   // (symbol << 4) | length; 0: not a code of so few bits
    uint16_t sym_l[288], sym_d[32], sym_c[19];               // symbols in canonical order
    uint16_t offs[16];
    TiCode code_l, code_d, code_c;
    uint8_t lens[320];                                       // literal/length lengths, then the distance lengths behind them
    uint8_t cll[19];
    uint8_t in[TI_IN];
};

enum { TI_NEXT = 0, TI_REFILL = 1, TI_COPY = 2, TI_RAW = 3, TI_CHECK = 4, TI_END = 5, TI_CORRUPT = 6, TI_SHORT = 7 };
enum { TI_M_HEAD = 0, TI_M_BLOCK = 1, TI_M_STORED = 2, TI_M_CODES = 3 };
// lane 0's registers: the bit reader, the block state, and what it asks the wave for
struct TiWalk {
    uint64_t hold; int bits; uint32_t ipos, out; int mode, last, fixed; uint32_t stored, c_src, c_len, c_dst, check; int full;
};

TD_FN uint32_t ti_rev16(uint32_t v) {                        // the 16 low bits mirrored
    v = ((v & 0x5555u) << 1) | ((v >> 1) & 0x5555u);
    v = ((v & 0x3333u) << 2) | ((v >> 2) & 0x3333u);
    v = ((v & 0x0f0fu) << 4) | ((v >> 4) & 0x0f0fu);
    return ((v & 0x00ffu) << 8) | ((v >> 8) & 0x00ffu);
}

// The tables of the code with lengths lens[0, n) (each 0..15; n at most the size of sym): zlib's inflate_table rules.  Returns false
// for an over-subscribed set, and for an incomplete one unless it is a single code of one bit (or no code at all) and not the
// code-length code (`codes`).
TD_FN bool ti_build(const uint8_t* lens, uint32_t n, bool codes, TiCode& c, uint16_t* sym, uint16_t* fast, int fast_bits, uint16_t* offs) {
    for (int l = 0; l < 16; ++l) c.cnt[l] = 0;
    for (uint32_t i = 0; i < n; ++i) ++c.cnt[lens[i] & 15];
    int max = 15;
    while (max >= 1 && c.cnt[max] == 0) --max;
    c.max = (uint16_t)max;
    for (uint32_t j = 0; j < (1u << fast_bits); ++j) fast[j] = 0;
    if (max == 0) return true;                               // no code at all: every code read is invalid
    int left = 1;
    for (int l = 1; l <= 15; ++l) {
        left = (left << 1) - (int)c.cnt[l];
        if (left < 0) return false;
    }
    if (left > 0 && (codes || max != 1)) return false;
    offs[1] = 0;
    for (int l = 1; l < 15; ++l) offs[l + 1] = (uint16_t)(offs[l] + c.cnt[l]);
    for (uint32_t i = 0; i < n; ++i) {
        const int l = lens[i] & 15;
        if (l && offs[l] < n) sym[offs[l]++] = (uint16_t)i;
    }
    uint32_t code = 0, idx = 0;
    for (int l = 1; l <= max && l <= fast_bits; ++l) {
        for (uint32_t k = 0; k < c.cnt[l] && idx < n; ++k, ++idx, ++code) {
            const uint16_t e = (uint16_t)((sym[idx] << 4) | l);
            for (uint32_t j = ti_rev16(code) >> (16 - l); j < (1u << fast_bits); j += 1u << l) fast[j] = e;
        }
        code <<= 1;
    }
    return true;
}

// The symbol at the low bits of w (at least 15 of them, zeros beyond the stream's end) and *len, its length; -1: no code (an
// incomplete set; *len is 1, as zlib's marker entry).
TD_FN int ti_symbol(uint32_t w, const TiCode& c, const uint16_t* sym, uint32_t n, const uint16_t* fast, int fast_bits, int* len) {
    const uint32_t e = fast[w & ((1u << fast_bits) - 1)];
    if (e) { *len = (int)(e & 15); return (int)(e >> 4); }
    int code = 0, first = 0, index = 0;
    for (int l = 1; l <= (int)c.max && l <= 15; ++l) {
        code |= (int)((w >> (l - 1)) & 1u);
        const int count = c.cnt[l];
        if (code - count < first) {
            const uint32_t at = (uint32_t)(index + (code - first));
            *len = l;
            return at < n ? (int)sym[at] : -1;
        }
        index += count; first += count; first <<= 1; code <<= 1;
    }
    *len = 1;
    return -1;
}

// Pulls staged bytes until the hold has n bits (n <= 48): TI_NEXT, TI_REFILL (the staged bytes are used up) or TI_SHORT (the stream is).
TD_FN int ti_fill(TiWalk& s, const TiLds& L, uint32_t have, uint32_t c0, uint32_t cn, int n) {
    while (s.bits < n) {
        if (s.ipos >= have) return TI_SHORT;
        if (s.ipos - c0 >= cn) return TI_REFILL;             // (unsigned: an ipos below c0 asks for a refill too)
        s.hold |= (uint64_t)L.in[s.ipos - c0] << s.bits;
        ++s.ipos;
        s.bits += 8;
    }
    return TI_NEXT;
}
TD_FN uint32_t ti_take(TiWalk& s, int n) {                   // n <= 32 bits the hold has
    const uint32_t v = (uint32_t)(s.hold & ((1ull << n) - 1));
    s.hold >>= n; s.bits -= n;
    return v;
}
// The stream ended inside a step: OK when the strip is full (no output byte was needed), else corrupt.
TD_FN int ti_short(const TiWalk& s, uint32_t want) { return s.out >= want ? TI_END : TI_CORRUPT; }

#define TI_NEED(n) { const int r_ = ti_fill(s, L, have, c0, cn, (n)); if (r_ == TI_REFILL) return TI_REFILL; if (r_ == TI_SHORT) return ti_short(s, want); }

// A dynamic block's header: HLIT / HDIST / HCLEN, the code-length code, the lengths (runs may cross from the literal/length lengths
// into the distance lengths), and the two tables.
TD_FN int ti_dynamic(TiWalk& s, TiLds& L, uint32_t have, uint32_t c0, uint32_t cn, uint32_t want) {
    TI_NEED(14);
    const uint32_t nlen = ti_take(s, 5) + 257, ndist = ti_take(s, 5) + 1, ncode = ti_take(s, 4) + 4;
    if (nlen > 286 || ndist > 30) return TI_CORRUPT;
    const uint64_t order = 0x22caa324e804a30ull;             // 5 bits each: 16 17 18 0 8 7 9 6 10 5 11 4, then 12 3 13 2 14 1 15
    const uint64_t order2 = 0x3c2e1346cull;
    for (uint32_t i = 0; i < 19; ++i) {
        uint32_t v = 0;
        if (i < ncode) { TI_NEED(3); v = ti_take(s, 3); }
        const uint32_t at = (uint32_t)((i < 12 ? order >> (5 * i) : order2 >> (5 * (i - 12))) & 31);
        if (at < 19) L.cll[at] = (uint8_t)v;
    }
    if (!ti_build(L.cll, 19, true, L.code_c, L.sym_c, L.fast_c, TI_FAST_C, L.offs)) return TI_CORRUPT;
    const uint32_t total = nlen + ndist;                     // <= 316
    uint32_t i = 0;
    while (i < total) {
        const int r = ti_fill(s, L, have, c0, cn, 14);
        if (r == TI_REFILL) return TI_REFILL;
        int len = 1;
        int sym = ti_symbol((uint32_t)s.hold, L.code_c, L.sym_c, 19, L.fast_c, TI_FAST_C, &len);
        if (sym < 0) sym = 0;                                // (an empty code-length code: zlib reads a length of 0 from its marker entry)
        const int extra = sym < 16 ? 0 : sym == 16 ? 2 : sym == 17 ? 3 : 7;
        if (len + extra > s.bits) return ti_short(s, want);
        (void)ti_take(s, len);
        if (sym < 16) { L.lens[i++] = (uint8_t)sym; continue; }
        uint32_t v = 0, rep;
        if (sym == 16) {
            if (i == 0) return TI_CORRUPT;
            v = L.lens[i - 1];
            rep = 3 + ti_take(s, 2);
        } else {
            rep = sym == 17 ? 3 + ti_take(s, 3) : 11 + ti_take(s, 7);
        }
        if (i + rep > total) return TI_CORRUPT;
        for (; rep; --rep) L.lens[i++] = (uint8_t)v;
    }
    if (L.lens[256] == 0) return TI_CORRUPT;                 // no end-of-block code
    if (!ti_build(L.lens, nlen, false, L.code_l, L.sym_l, L.fast_l, TI_FAST_L, L.offs)) return TI_CORRUPT;
    if (!ti_build(L.lens + nlen, ndist, false, L.code_d, L.sym_d, L.fast_d, TI_FAST_D, L.offs)) return TI_CORRUPT;
    s.fixed = 0;
    return TI_NEXT;
}

// One step of the walk.  TI_NEXT: go on; TI_REFILL: the caller undoes the step's reads; else what the wave is to do.
TD_FN int ti_step(TiWalk& s, TiLds& L, uint32_t have, uint32_t c0, uint32_t cn, uint8_t* dst, uint32_t want) {
    if (s.mode == TI_M_HEAD) {                               // the zlib wrapper: CM, CINFO, FCHECK, FDICT
        TI_NEED(16);
        const uint32_t cmf = ti_take(s, 8), flg = ti_take(s, 8);
        if (((cmf << 8) | flg) % 31 || (cmf & 15) != 8 || (cmf >> 4) > 7 || (flg & 0x20)) return TI_CORRUPT;
        s.mode = TI_M_BLOCK;
        return TI_NEXT;
    }
    if (s.mode == TI_M_BLOCK) {
        if (s.last) {                                        // the trailer: Adler-32 of the output, most significant byte first
            (void)ti_take(s, s.bits & 7);
            TI_NEED(32);
            const uint32_t v = ti_take(s, 32);
            s.check = (v << 24) | ((v & 0xff00u) << 8) | ((v >> 8) & 0xff00u) | (v >> 24);
            return TI_CHECK;
        }
        TI_NEED(3);
        const uint32_t last = ti_take(s, 1), type = ti_take(s, 2);
        if (type == 3) return TI_CORRUPT;
        if (type == 0) {                                     // stored: LEN / NLEN on a byte boundary, then LEN bytes of the stream
            (void)ti_take(s, s.bits & 7);
            TI_NEED(32);
            const uint32_t v = ti_take(s, 32);
            if ((v & 0xffffu) != ((v >> 16) ^ 0xffffu)) return TI_CORRUPT;
            s.ipos -= (uint32_t)s.bits >> 3;                 // whole bytes the hold took ahead go back to the stream
            s.hold = 0; s.bits = 0;
            s.stored = v & 0xffffu;
            s.mode = TI_M_STORED;
        } else if (type == 1) {
            if (!s.fixed) {
                for (uint32_t i = 0; i < 288; ++i) L.lens[i] = (uint8_t)(i < 144 ? 8 : i < 256 ? 9 : i < 280 ? 7 : 8);
                for (uint32_t i = 288; i < 320; ++i) L.lens[i] = 5;
                (void)ti_build(L.lens, 288, false, L.code_l, L.sym_l, L.fast_l, TI_FAST_L, L.offs);
                (void)ti_build(L.lens + 288, 32, false, L.code_d, L.sym_d, L.fast_d, TI_FAST_D, L.offs);
                s.fixed = 1;
            }
            s.mode = TI_M_CODES;
        } else {
            const int r = ti_dynamic(s, L, have, c0, cn, want);
            if (r != TI_NEXT) return r;
            s.mode = TI_M_CODES;
        }
        s.last = (int)last;
        return TI_NEXT;
    }
    if (s.mode == TI_M_STORED) {
        if (s.stored == 0) { s.mode = TI_M_BLOCK; return TI_NEXT; }
        if (s.ipos >= have) return ti_short(s, want);
        if (s.out >= want) return TI_END;
        uint32_t n = s.stored;
        if (n > have - s.ipos) n = have - s.ipos;
        if (n > want - s.out) n = want - s.out;
        s.c_src = s.ipos; s.c_dst = s.out; s.c_len = n;
        s.ipos += n; s.out += n; s.stored -= n;
        return TI_RAW;
    }
    // TI_M_CODES: a literal, the end of the block, or a length and its distance: 15 + 5 + 15 + 13 bits at the most
    if (ti_fill(s, L, have, c0, cn, 48) == TI_REFILL) return TI_REFILL;
    int len = 1;
    const int sym = ti_symbol((uint32_t)s.hold, L.code_l, L.sym_l, 288, L.fast_l, TI_FAST_L, &len);
    if (len > s.bits) return ti_short(s, want);
    if (sym < 0) return TI_CORRUPT;
    (void)ti_take(s, len);
    if (sym < 256) {
        if (s.out >= want) return TI_END;
        dst[s.out++] = (uint8_t)sym;
        return TI_NEXT;
    }
    if (sym == 256) { s.mode = TI_M_BLOCK; return TI_NEXT; }
    if (sym >= 286) return TI_CORRUPT;
    uint32_t k = (uint32_t)sym - 257, mlen;
    if (sym == 285) mlen = 258;
    else if (k < 8) mlen = 3 + k;
    else {
        const int e = (int)(k >> 2) - 1;
        if (e > s.bits) return ti_short(s, want);
        mlen = 3 + ((4 + (k & 3)) << e) + ti_take(s, e);
    }
    const int dsym = ti_symbol((uint32_t)s.hold, L.code_d, L.sym_d, 32, L.fast_d, TI_FAST_D, &len);
    if (len > s.bits) return ti_short(s, want);
    if (dsym < 0) return TI_CORRUPT;
    (void)ti_take(s, len);
    if (dsym >= 30) return TI_CORRUPT;
    uint32_t dist = 1 + (uint32_t)dsym;
    if (dsym >= 4) {
        const int e = (dsym >> 1) - 1;
        if (e > s.bits) return ti_short(s, want);
        dist = 1 + ((2 + ((uint32_t)dsym & 1)) << e) + ti_take(s, e);
    }
    if (s.out >= want) return TI_END;                        // (zlib too reads the whole pair before it asks for room)
    if (dist > s.out) return TI_CORRUPT;                     // before the strip's first byte
    const uint32_t room = want - s.out, ncopy = mlen <= room ? mlen : room;
    s.c_src = s.out - dist; s.c_dst = s.out; s.c_len = ncopy;
    s.out += ncopy;
    if (ncopy < mlen) s.full = 1;
    return TI_COPY;
}

// Walks the stream until the wave has something to do.  The staged bytes are those of [c0, c0 + cn) of the stream.
TD_FN int ti_walk(TiWalk& s, TiLds& L, uint32_t have, uint32_t c0, uint32_t cn, uint8_t* dst, uint32_t want) {
    if (s.full) return TI_END;                               // the copy before filled the destination
    for (;;) {
        const uint64_t hold = s.hold;
        const int bits = s.bits;
        const uint32_t ipos = s.ipos;
        const int r = ti_step(s, L, have, c0, cn, dst, want);
        if (r == TI_REFILL) { s.hold = hold; s.bits = bits; s.ipos = ipos; return TI_REFILL; }
        if (r != TI_NEXT) return r;
    }
}

// Adler-32 of dst[0, n) by the wave (n <= want; the wave's stores are complete).
TD_FN uint32_t ti_adler(const uint8_t* dst, uint32_t n) {
    uint32_t a = 1, b = 0;
    for (uint32_t p = 0; p < n; p += TI_ADLER) {
        const uint32_t m = n - p < TI_ADLER ? n - p : TI_ADLER;
        uint32_t sum = 0, wsum = 0;                          // of the chunk: sum d, sum (m - k) d
        TD_FOR_LANES(lane) {
            uint32_t ls = 0, lw = 0;
            for (uint32_t k = (uint32_t)lane; k < m; k += 64) { const uint32_t d = dst[p + k]; ls += d; lw += (m - k) * d; }
            sum += ls; wsum += lw % 65521u;
        }
        sum = ti_wave_sum(sum); wsum = ti_wave_sum(wsum);
        b = (b + m * a + wsum) % 65521u;                     // (m * a below 2^28, wsum below 2^22)
        a = (a + sum) % 65521u;
    }
    return (b << 16) | a;
}

// src: the strip's `have` bytes; dst: its `want` bytes of the raster (1 <= want < 2^31).  Returns 0, or 1 for a corrupt stream (the
// same value in every lane); bytes the stream does not give are zero.
TD_FN uint32_t ti_inflate_strip(const uint8_t* src, uint32_t have, uint8_t* dst, uint32_t want, TiLds& L) {
    TiWalk s{0ull, 0, 0u, 0u, TI_M_HEAD, 0, 0, 0u, 0u, 0u, 0u, 0u, 0};
    uint32_t c0 = 0, cn = 0, fenced = 0;
    bool staged = false;
    int cmd;
    for (;;) {
        cmd = TI_END;
        TD_CONTROL_LANE { cmd = ti_walk(s, L, have, c0, cn, dst, want); }
        cmd = (int)td_first((uint32_t)cmd);
        if (cmd == TI_REFILL) {
            const uint32_t at = td_first(s.ipos);
            if (staged && at == c0) { cmd = TI_CORRUPT; break; }             // (a step that its own TI_IN bytes do not serve: never)
            c0 = at; staged = true;
            cn = c0 < have ? (have - c0 < TI_IN ? have - c0 : TI_IN) : 0u;
            TD_FOR_LANES(lane) {
                for (uint32_t k = (uint32_t)lane; k < cn; k += 64) L.in[k] = src[c0 + k];
            }
            td_stores_done();                                // (the barrier the staged bytes need completes the output stores too)
            fenced = td_first(s.out);
        } else if (cmd == TI_COPY) {
            const uint32_t c_src = td_first(s.c_src), c_len = td_first(s.c_len), c_dst = td_first(s.c_dst);
            const uint32_t dist = c_dst - c_src;             // >= 1
            const uint32_t reach = c_len < dist ? c_len : dist;
            if (c_src + reach > fenced) { td_stores_done(); fenced = c_dst; }
            TD_FOR_LANES(lane) {
                for (uint32_t k = (uint32_t)lane; k < c_len; k += 64) {
                    const uint32_t from = c_src + (c_len <= dist ? k : k % dist), to = c_dst + k;
                    if (from < want && to < want) dst[to] = dst[from];
                }
            }
        } else if (cmd == TI_RAW) {
            const uint32_t c_src = td_first(s.c_src), c_len = td_first(s.c_len), c_dst = td_first(s.c_dst);
            TD_FOR_LANES(lane) {
                for (uint32_t k = (uint32_t)lane; k < c_len; k += 64)
                    if (c_src + k < have && c_dst + k < want) dst[c_dst + k] = src[c_src + k];
            }
        } else {
            break;
        }
    }
    const uint32_t got = td_first(s.out);
    if (cmd == TI_CHECK) {
        td_stores_done();
        cmd = ti_adler(dst, got <= want ? got : want) == td_first(s.check) ? TI_END : TI_CORRUPT;
    }
    TD_FOR_LANES(lane) {
        for (uint32_t k = got + (uint32_t)lane; k < want; k += 64) dst[k] = 0;
    }
    return cmd == TI_CORRUPT ? 1u : 0u;
}

#undef TI_NEED

// Global strip `strip` of a batch, by one wave, when its file holds Deflate strips: the status word (0, or 1: corrupt stream / offset
// behind the file), the same in every lane; TD_OTHER_KERNEL for a strip of tdb_unstrip's.  A strip the tables do not have is
// zero-filled; one they have is a stream, and an empty stream is corrupt.
TD_FN uint32_t tdb_inflate(const TdFile* tab, uint32_t n_files, const uint8_t* files, const uint32_t* tables, uint8_t* rasters, uint32_t strip,
                           TiLds& L, const TdTiles* tiles = nullptr, uint8_t* staging = nullptr) {
    const TdFile& f = tab[td_first(td_find_file(tab, n_files, strip, false))];
    if (f.codec != TD_DEFLATE) return TD_OTHER_KERNEL;
    const uint32_t k = strip - f.first_strip;
    if (f.tiles) {                                           // a tile: its zlib stream into its slot (td_tile: an offset behind the file is a short stream)
        if (!f.in_batch || k >= f.n_table) return 0u;
        const TdStrip t = td_tile(k, f, tiles[f.tiles - 1], files, tables, staging);
        return ti_inflate_strip(t.src, t.have, t.dst, t.want, L);
    }
    if (!f.in_batch || (unsigned long long)k * f.rps >= f.H) return 0u;      // (the grid has the strips of the table: never)
    const uint32_t* offs = tables + f.table_off;
    const TdStrip t = td_strip(k, files + f.file_off, f.n_bytes, offs, offs + f.n_table, f.n_table, f.H, f.line, f.rps, rasters + f.raster_off);
    if (!t.in_table || t.behind_file) {
        TD_FOR_LANES(lane) {
            for (uint32_t i = (uint32_t)lane; i < t.want; i += 64) t.dst[i] = 0;
        }
        return t.behind_file ? 1u : 0u;
    }
    return ti_inflate_strip(t.src, t.have, t.dst, t.want, L);
}

}  // namespace ecseg
