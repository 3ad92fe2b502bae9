// Files coded on the device: the TIFF encoder for one raster and for a batch (tiff_kernels.hip; the host writer is tiff_write_u8, host_io.cpp), the TIFF decoder for
// one file and for a batch (tiff_decode_kernels.hip; the host reader is ecseg_tiff_read), the label PNG encoder (png_kernels.hip;
// the host writer is ecseg_png_write_labels) and the gray PNG encoder (png_gray_kernels.hip; the host writer is
// ecseg_png_write_channel), with the tails that ecseg_meta_segment_files and ecseg_fish_render_tiff share.
#include <cstring>

#include "driver_util.h"

#include "png_gray_code.h"
#include "png_label_code.h"
#include "tiff_parse.h"

using namespace ecseg;

// The strips of n_files rasters are encoded and packed (run_tiff_encode is done or on a stream that the main stream's end waits
// for): brings the tables over, puts head and tail around every file's strips and copies the strips into the caller's buffers.
int ecseg::tiff_collect(ecseg_ctx* h, const char* who, int n_files, int H, int W, int spp, const TiffEncodeBufs& b, uint8_t* const* files,
                        long long file_cap, long long* file_bytes, bool strict) {
    hipStream_t s = h->stream;
    const size_t ns = (size_t)b.nstrips;
    std::vector<uint32_t> cnt(ns * n_files);
    std::vector<unsigned long long> off((ns + 1) * n_files);
    HIP_TRY(h, hipMemcpyAsync(cnt.data(), b.cnt, cnt.size() * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    HIP_TRY(h, hipMemcpyAsync(off.data(), b.off, off.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
    HIP_TRY(h, hipStreamSynchronize(s));
    std::vector<std::vector<uint8_t>> head(n_files), tail(n_files);
    std::vector<uint32_t> offs(ns);
    for (int f = 0; f < n_files; ++f) {
        const unsigned long long* o = off.data() + (ns + 1) * f;
        const uint32_t* m = cnt.data() + ns * f;
        for (size_t k = 0; k < ns; ++k) {
            if (8 + o[k] + m[k] + 1 >= 0xffffffffull) return fail(h, ECSEG_E_INVALID, std::string(who) + ": the file would pass 4 GiB (classic TIFF has 32-bit offsets)");
            offs[k] = (uint32_t)(8 + o[k]);
        }
        tiff_frame(H, W, spp, b.rps, offs.data(), m, b.nstrips, (size_t)(8 + o[ns]), &head[f], &tail[f]);
        const unsigned long long total = 8 + o[ns] + tail[f].size();
        if (total > (unsigned long long)file_cap && strict)
            return fail(h, ECSEG_E_INVALID, std::string(who) + ": a file of " + std::to_string(total) + " bytes does not fit the capacity of " +
                                                std::to_string(file_cap) + " (ecseg_tiff_encode_bound says what always does)");
        file_bytes[f] = total > (unsigned long long)file_cap ? -(long long)total : (long long)total;
    }
    for (int f = 0; f < n_files; ++f) {
        if (file_bytes[f] < 0) continue;
        const size_t data = (size_t)off[(ns + 1) * f + ns];
        std::memcpy(files[f], head[f].data(), 8);
        HIP_TRY(h, hipMemcpyAsync(files[f] + 8, b.packed + b.file_stride * f, data, hipMemcpyDeviceToHost, s));
        std::memcpy(files[f] + 8 + data, tail[f].data(), tail[f].size());
    }
    HIP_TRY(h, hipStreamSynchronize(s));
    return ECSEG_OK;
}

// The rows of an encode batch's table ([n][5]: byte offset, H, W, spp, invert) as ecseg_tiff_encode judges each raster alone, the
// ranges by ecseg_min_cut's rule: in order, clear of each other, inside the raster_bytes bytes of the buffer (raster_bytes < 0: no
// buffer to hold them to).  Empty string and `in`, or what is wrong.
std::string ecseg::tiff_encode_batch_plan(const int64_t* files, int n_files, long long raster_bytes, std::vector<TeFileIn>& in) {
    in.assign((size_t)n_files, TeFileIn());
    long long end = 0;
    for (int i = 0; i < n_files; ++i) {
        const int64_t* f = files + 5 * (size_t)i;
        const std::string who = "file " + std::to_string(i);
        if (f[1] <= 0 || f[2] <= 0 || f[1] > INT32_MAX || f[2] > INT32_MAX || (f[3] != 1 && f[3] != 3) || !tiff_args_ok((int)f[1], (int)f[2], (int)f[3]))
            return who + ": the extents must be positive, the samples per pixel 1 or 3 and a line below 2^30 bytes";
        const long long nb = f[1] * f[2] * f[3];             // (below 2^31 * 2^30)
        if (f[0] < end || (raster_bytes >= 0 && (f[0] > raster_bytes || nb > raster_bytes - f[0])))
            return who + ": its raster overlaps the one in front or leaves the " + std::to_string(raster_bytes) + " bytes of rasters";
        if (f[0] > INT64_MAX - nb) return who + ": its raster ends behind 2^63";
        end = f[0] + nb;
        TeFileIn& d = in[(size_t)i];
        d.src_off = (uint64_t)f[0]; d.H = (uint32_t)f[1]; d.W = (uint32_t)f[2]; d.spp = (uint32_t)f[3]; d.invert = f[4] != 0;
    }
    return std::string();
}

// The strips of a batch are encoded and packed (run_tiff_encode_batch is on the stream): brings the counts, the strip offsets and the
// files' places over, frames every file and - once it is known that all of them fit out_cap - brings the packed output over in one
// copy and writes heads and tails into its gaps.  Nothing of out or out_ranges is written before that verdict.
int ecseg::tiff_batch_collect(ecseg_ctx* h, const char* who, const TeBatchLayout& L, const TiffEncodeBatchBufs& b, uint8_t* out, long long out_cap,
                              int64_t* out_ranges) {
    hipStream_t s = h->stream;
    const size_t nf = L.tab.size();
    std::vector<uint32_t> cnt((size_t)L.n_strips);
    std::vector<unsigned long long> off((size_t)L.off_entries), base(nf + 1);
    HIP_TRY(h, hipMemcpyAsync(cnt.data(), b.cnt, cnt.size() * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    HIP_TRY(h, hipMemcpyAsync(off.data(), b.off, off.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
    HIP_TRY(h, hipMemcpyAsync(base.data(), b.base, base.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
    HIP_TRY(h, hipStreamSynchronize(s));
    std::vector<std::vector<uint8_t>> head(nf), tail(nf);
    std::vector<uint32_t> offs;
    for (size_t f = 0; f < nf; ++f) {
        const TeFile& t = L.tab[f];
        const unsigned long long* o = off.data() + t.off_off;
        const uint32_t* m = cnt.data() + t.first_strip;
        offs.resize(t.n_strips);
        for (uint32_t k = 0; k < t.n_strips; ++k) {
            if (8 + o[k] + m[k] + 1 >= 0xffffffffull)
                return fail(h, ECSEG_E_INVALID, std::string(who) + ": file " + std::to_string(f) + " would pass 4 GiB (classic TIFF has 32-bit offsets)");
            offs[k] = (uint32_t)(8 + o[k]);
        }
        tiff_frame((int)t.H, (int)t.W, (int)t.spp, (int)t.rps, offs.data(), m, (int)t.n_strips, (size_t)(8 + o[t.n_strips]), &head[f], &tail[f]);
        if (head[f].size() + tail[f].size() != t.frame_bytes || base[f + 1] - base[f] != t.frame_bytes + o[t.n_strips])
            return fail(h, ECSEG_E_HIP, std::string(who) + ": file " + std::to_string(f) + ": the device placed the file for a frame of another size");
    }
    if (base[nf] > (unsigned long long)out_cap)
        return fail(h, ECSEG_E_INVALID, std::string(who) + ": files of " + std::to_string(base[nf]) + " bytes do not fit the capacity of " +
                                            std::to_string(out_cap) + " (the sum of ecseg_tiff_encode_bound says what always does)");
    HIP_TRY(h, hipMemcpyAsync(out, b.packed, (size_t)base[nf], hipMemcpyDeviceToHost, s));
    HIP_TRY(h, hipStreamSynchronize(s));
    for (size_t f = 0; f < nf; ++f) {
        uint8_t* file = out + base[f];
        const size_t data = (size_t)off[L.tab[f].off_off + L.tab[f].n_strips];
        std::memcpy(file, head[f].data(), 8);
        std::memcpy(file + 8 + data, tail[f].data(), tail[f].size());
        out_ranges[2 * f] = (int64_t)base[f];
        out_ranges[2 * f + 1] = (int64_t)(base[f + 1] - base[f]);
    }
    return ECSEG_OK;
}

int ecseg::png_encode_files(ecseg_ctx* h, const char* who, const uint8_t* d_labels, int n, int H, int W, const PngEncodeBufs& b,
                            uint8_t* const* files, long long file_cap, long long* file_bytes, float* ms) {
    hipStream_t s = h->stream;
    const size_t px = (size_t)H * W;
    HIP_TRY(h, hipEventRecord(h->ev_files[2], s));           // (ev_files into *ms, not TIMED's ev into stage_ms: ecseg_meta_segment_files keeps these apart)
    HIP_TRY(h, run_png_count(d_labels, px, n, H, W, b, s));
    HIP_TRY(h, hipEventRecord(h->ev_files[3], s));
    std::vector<uint32_t> counts((size_t)n * PNG_NCOUNT);
    HIP_TRY(h, hipMemcpyAsync(counts.data(), b.counts, counts.size() * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    HIP_TRY(h, hipStreamSynchronize(s));
    // the code of every image and with it the exact size of its stream: the stream buffer holds just that, in whole dwords
    std::vector<PngDevCode> codes((size_t)n);
    std::vector<size_t> zb((size_t)n);
    size_t words = 0;
    for (int i = 0; i < n; ++i) {
        const uint32_t* c = counts.data() + (size_t)i * PNG_NCOUNT;
        LabelPngCode k;
        label_png_code(c, c + 4, (uint32_t)H, LABEL_PNG_PALETTE, &k);
        zb[i] = label_png_stream_bytes(k, c, c + 4, (uint32_t)H);
        if (zb[i] >= 0x7fffffffull) return fail(h, ECSEG_E_INVALID, std::string(who) + ": a stream of 2 GiB or more does not fit a PNG chunk");
        PngDevCode& d = codes[i];
        std::memset(&d, 0, sizeof d);
        for (int q = 0; q < 4; ++q) { d.cbits[q] = k.cbits[q]; d.cn[q] = (uint32_t)k.cn[q]; }
        for (int m = 0; m <= 64; ++m) { d.mbits[m] = k.mbits[m]; d.mn[m] = (uint32_t)k.mn[m]; }
        std::memcpy(d.head, k.head, sizeof d.head);
        d.head_bits = k.head_bits; d.filt = k.filt; d.filt_n = (uint32_t)k.filt_n; d.eob = k.eob; d.eob_n = (uint32_t)k.eob_n;
        d.z_off = words; d.z_words = (uint32_t)((zb[i] + 3) / 4);
        words += d.z_words;
    }
    int rc;
    if ((rc = h->count_arena.ensure(h, words * 4, "hipMalloc(png streams)"))) return rc;
    uint32_t* z = reinterpret_cast<uint32_t*>(h->count_arena.p);
    HIP_TRY(h, hipMemcpyAsync(b.codes, codes.data(), codes.size() * sizeof(PngDevCode), hipMemcpyHostToDevice, s));
    HIP_TRY(h, hipEventRecord(h->ev_files[4], s));
    HIP_TRY(h, run_png_emit(d_labels, px, n, H, W, b, z, words * 4, s));
    HIP_TRY(h, hipEventRecord(h->ev_files[5], s));
    std::vector<unsigned long long> dz((size_t)n);
    HIP_TRY(h, hipMemcpyAsync(dz.data(), b.z_bytes, dz.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
    for (int i = 0; i < n; ++i) {
        const size_t total = label_png_file_bytes(zb[i]);
        file_bytes[i] = total > (unsigned long long)file_cap ? -(long long)total : (long long)total;
        if (file_bytes[i] > 0)
            HIP_TRY(h, hipMemcpyAsync(files[i] + LABEL_PNG_Z_OFFSET, z + codes[i].z_off, zb[i], hipMemcpyDeviceToHost, s));
    }
    HIP_TRY(h, hipStreamSynchronize(s));
    for (int i = 0; i < n; ++i) {
        if (dz[i] != zb[i])
            return fail(h, ECSEG_E_HIP, std::string(who) + ": image " + std::to_string(i) + ": the device wrote a stream of " + std::to_string(dz[i]) +
                                            " bytes where the counts give " + std::to_string(zb[i]));
        if (file_bytes[i] > 0) label_png_frame(files[i], zb[i], H, W);
    }
    *ms = stage_elapsed(h->ev_files[2], h->ev_files[3]) + stage_elapsed(h->ev_files[4], h->ev_files[5]);
    return ECSEG_OK;
}

int ecseg::png_gray_encode(ecseg_ctx* h, const char* who, const GraySource& src, int n_planes, int H, int W, const GrayEncodeBufs& b,
                           uint8_t* const* files, long long file_cap, long long* file_bytes, float* ms) {
    hipStream_t s = h->stream;
    const size_t np = (size_t)n_planes;
    HIP_TRY(h, hipEventRecord(h->ev_files[2], s));
    HIP_TRY(h, run_pgray_count(src, n_planes, b, s));
    HIP_TRY(h, hipEventRecord(h->ev_files[3], s));
    std::vector<uint32_t> counts(np * PGRAY_NCOUNT);
    HIP_TRY(h, hipMemcpyAsync(counts.data(), b.counts, counts.size() * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    HIP_TRY(h, hipStreamSynchronize(s));
    // the code of every plane, with it the exact size of its stream and of its file, and so the verdict before a bit is written
    std::vector<GrayDevCode> codes(np);
    std::vector<size_t> zb(np);
    size_t words = 0;
    for (size_t i = 0; i < np; ++i) {
        const uint32_t* c = counts.data() + i * PGRAY_NCOUNT;
        GrayPngCode k;
        gray_png_code(c, c[286] != 0, &k);
        zb[i] = gray_png_stream_bytes(k, c);
        if (zb[i] > b.z_stride) return fail(h, ECSEG_E_HIP, std::string(who) + ": plane " + std::to_string(i) + ": the counts give a stream of " +
                                                                 std::to_string(zb[i]) + " bytes, above the bound of any stream");
        const size_t total = label_png_file_bytes(zb[i]);
        file_bytes[i] = total > (unsigned long long)file_cap ? -(long long)total : (long long)total;
        GrayDevCode& d = codes[i];
        std::memset(&d, 0, sizeof d);
        for (int q = 0; q < 256; ++q) d.lit[q] = (uint32_t)k.lcode[q] | ((uint32_t)k.llen[q] << 16);
        for (int L = 3; L <= 258; ++L) d.match[L] = k.mbits[L] | ((uint32_t)k.mn[L] << 24);
        std::memcpy(d.head, k.head, sizeof d.head);
        d.head_bits = k.head_bits; d.eob = k.lcode[256]; d.eob_n = k.llen[256];
        d.z_off = words; d.z_words = file_bytes[i] > 0 ? (uint32_t)((zb[i] + 3) / 4) : 0u;
        words += d.z_words;
    }
    HIP_TRY(h, hipMemcpyAsync(b.codes, codes.data(), codes.size() * sizeof(GrayDevCode), hipMemcpyHostToDevice, s));
    HIP_TRY(h, hipEventRecord(h->ev_files[4], s));
    HIP_TRY(h, run_pgray_emit(src, n_planes, b, words * 4, s));
    HIP_TRY(h, hipEventRecord(h->ev_files[5], s));
    std::vector<unsigned long long> dz(np);
    HIP_TRY(h, hipMemcpyAsync(dz.data(), b.z_bytes, dz.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
    for (size_t i = 0; i < np; ++i)
        if (file_bytes[i] > 0) HIP_TRY(h, hipMemcpyAsync(files[i] + LABEL_PNG_Z_OFFSET, b.z + codes[i].z_off, zb[i], hipMemcpyDeviceToHost, s));
    HIP_TRY(h, hipStreamSynchronize(s));
    for (size_t i = 0; i < np; ++i) {
        if (file_bytes[i] <= 0) continue;
        if (dz[i] != zb[i])
            return fail(h, ECSEG_E_HIP, std::string(who) + ": plane " + std::to_string(i) + ": the device wrote a stream of " + std::to_string(dz[i]) +
                                            " bytes where the counts give " + std::to_string(zb[i]));
        gray_png_frame(files[i], zb[i], H, W);
    }
    *ms = stage_elapsed(h->ev_files[2], h->ev_files[3]) + stage_elapsed(h->ev_files[4], h->ev_files[5]);
    return ECSEG_OK;
}

// The strips of a parsed file that is to be decoded lie in the file: ECSEG_OK, or ECSEG_E_INVALID and which one does not.
static int tiff_strips_in_file(const TiffInfo& t, size_t n, std::string& why) {
    if (t.tw) return ECSEG_OK;                               // (a tile's stream is clamped to the file, as the Python reader's slice is: td_tile)
    const size_t nstrips = ((size_t)t.H + t.rps - 1) / t.rps, n_table = std::min(t.off.size(), nstrips);
    for (size_t k = 0; k < n_table; ++k)
        if (t.off[k] > n) { why = "strip " + std::to_string(k) + " starts behind the end of the file"; return ECSEG_E_INVALID; }
    return ECSEG_OK;
}

// What ecseg_tiff_decode makes of a file before any device work, for itself and for every file of a batch: the tags in t, *parsed
// (the file has a shape), and ECSEG_OK or the status with its reason.  with_strips: the file is to be decoded, not only measured.
// kinds (ECSEG_TIFF_*): with ECSEG_TIFF_DEFLATE Deflate strips are taken (the handle option tiff_deflate_on_device); without it they are
// the host reader's.  With ECSEG_TIFF_TILED tiled files are taken by the rule of parse_tiff (tiff_tiled_on_device); without it they are
// ECSEG_E_UNSUPPORTED and have no shape, as ever.  ECSEG_TIFF_PACKBITS: so are PackBits files (tiff_packbits_on_device), under the same words.
static int tiff_decode_verdict(const uint8_t* file, size_t n, bool with_strips, unsigned kinds, TiffInfo& t, bool* parsed, std::string& why) {
    t = TiffInfo();
    int rc = parse_tiff(file, n, &t, kinds);
    *parsed = rc == ECSEG_OK;
    if (rc != ECSEG_OK) {
        why = rc == ECSEG_E_UNSUPPORTED ? "a layout the native readers leave to the Python reader" : "not a TIFF file, or a corrupt one";
        return rc;
    }
    const unsigned long long bpp = t.bits / 8, line = (unsigned long long)t.W * t.spp * bpp, total = line * t.H;
    if (tiff_is_deflate(t) && !(kinds & ECSEG_TIFF_DEFLATE)) { why = "Deflate strips are decoded by the host reader (option tiff_deflate_on_device: 0)"; return ECSEG_E_UNSUPPORTED; }
    if (t.tw && (unsigned long long)t.tw * t.th * t.spp * bpp >= (1ull << 31)) { why = "tiles of 2 GiB or more"; return ECSEG_E_UNSUPPORTED; }
    if ((!t.tw && (unsigned long long)t.rps * line >= (1ull << 31)) || total >= (1ull << 40)) {
        why = "strips of 2 GiB or more, or an image of 1 TiB or more";
        return ECSEG_E_UNSUPPORTED;
    }
    return with_strips ? tiff_strips_in_file(t, n, why) : ECSEG_OK;
}

// The layout row of a file that passed tiff_decode_verdict with its strips: n bytes at src_off of the caller's files; dst_off is the caller's.
static TdFileIn td_file_in(const TiffInfo& t, size_t src_off, size_t n) {
    TdFileIn f;
    const size_t nstrips = ((size_t)t.H + t.rps - 1) / t.rps;
    f.in_batch = true; f.src_off = src_off; f.n_bytes = n;
    f.tw = t.tw; f.th = t.th;
    f.n_table = (uint32_t)std::min(t.off.size(), t.tw ? tiff_tile_count(t) : nstrips); f.H = t.H; f.W = t.W; f.spp = t.spp; f.bps = t.bits / 8; f.rps = t.rps;
    f.codec = t.comp == 1 ? TD_RAW : t.comp == 5 ? TD_LZW : t.comp == 32773 ? TD_PACKBITS : TD_DEFLATE; f.swap = f.bps == 2 && !t.le; f.predictor = t.pred == 2;
    return f;
}

// The files of a batch as ecseg_tiff_decode judges each alone (ctx.h says what comes back).
std::string ecseg::tiff_batch_plan(const uint8_t* files, long long files_bytes, const int64_t* ranges, int n_files, const int64_t* dst_offsets,
                                   bool with_strips, std::vector<TiffInfo>& info, std::vector<int>& status, std::vector<TdFileIn>& in, unsigned kinds) {
    info.assign((size_t)n_files, TiffInfo()); status.assign((size_t)n_files, ECSEG_OK); in.assign((size_t)n_files, TdFileIn());
    long long end = 0;
    for (int i = 0; i < n_files; ++i) {                      // the geometry first: nothing is read through a bad range
        const long long off = ranges[2 * (size_t)i], nb = ranges[2 * (size_t)i + 1];
        if (nb < 0 || off < end || off > files_bytes || nb > files_bytes - off)
            return "file " + std::to_string(i) + ": its range overlaps the one in front or leaves the " + std::to_string(files_bytes) + " bytes of files";
        end = off + nb;
    }
    unsigned long long packed = 0;
    std::string why;
    for (int i = 0; i < n_files; ++i) {
        const size_t off = (size_t)ranges[2 * (size_t)i], nb = (size_t)ranges[2 * (size_t)i + 1];
        TiffInfo& t = info[(size_t)i];
        bool parsed = false;
        status[(size_t)i] = tiff_decode_verdict(files + off, nb, with_strips, kinds, t, &parsed, why);
        if (!parsed) t.H = t.W = 0;                          // (no shape to report)
        if (status[(size_t)i] != ECSEG_OK) continue;
        TdFileIn& f = in[(size_t)i] = td_file_in(t, off, nb);
        if (dst_offsets) {
            if (dst_offsets[i] < 0) return "file " + std::to_string(i) + ": a negative destination offset";
            f.dst_off = (uint64_t)dst_offsets[i];
        } else {
            packed += packed & (f.bps - 1);
            f.dst_off = packed;
            packed += (unsigned long long)f.W * f.spp * f.bps * f.H;
        }
    }
    return std::string();
}

void ecseg::tiff_plan_tables(const std::vector<TiffInfo>& info, TiffsPlan& p) {
    p.tables.assign((size_t)p.L.table_words, 0u);
    for (size_t i = 0; i < p.L.tab.size(); ++i) {
        const TdFile& f = p.L.tab[i];
        std::copy(info[i].off.begin(), info[i].off.begin() + f.n_table, p.tables.begin() + (size_t)f.table_off);
        std::copy(info[i].cnt.begin(), info[i].cnt.begin() + f.n_table, p.tables.begin() + (size_t)f.table_off + f.n_table);
    }
}

int ecseg::tiff_batch_launch(ecseg_ctx* h, const uint8_t* files, const TiffsPlan& p, const TiffDecodeBatchBufs& b, hipStream_t s, hipEvent_t e0,
                             hipEvent_t e1) {
    const TdBatchLayout& L = p.L;
    if (L.src_span) HIP_TRY(h, hipMemcpyAsync(b.files, files + L.src_base, (size_t)L.src_span, hipMemcpyHostToDevice, s));
    HIP_TRY(h, hipMemcpyAsync(b.tab, L.tab.data(), L.tab.size() * sizeof(TdFile), hipMemcpyHostToDevice, s));
    if (!p.tables.empty()) HIP_TRY(h, hipMemcpyAsync(b.tables, p.tables.data(), p.tables.size() * sizeof(uint32_t), hipMemcpyHostToDevice, s));
    if (!L.tiles.empty()) HIP_TRY(h, hipMemcpyAsync(b.tiles, L.tiles.data(), L.tiles.size() * sizeof(TdTiles), hipMemcpyHostToDevice, s));
    HIP_TRY(h, hipEventRecord(e0, s));
    HIP_TRY(h, run_tiff_decode_batch(b, L, s));
    HIP_TRY(h, hipEventRecord(e1, s));
    return ECSEG_OK;
}

extern "C" {

// ---- TIFF files encoded on the device -------------------------------------------------------------------------------------------
long long ecseg_tiff_encode_bound(int H, int W, int spp) {
    if (!tiff_args_ok(H, W, spp)) return -1;
    const int rps = tiff_rows_per_strip(H, W, spp), nstrips = (H + rps - 1) / rps;
    return (long long)(8 + (size_t)nstrips * (tiff_strip_bound((size_t)rps * W * spp) + 1) + tiff_tail_bound(nstrips, spp));
}

int ecseg_tiff_encode(ecseg_ctx* h, const uint8_t* img, int H, int W, int spp, int invert, uint8_t* out, long long out_cap, long long* out_bytes) {
    DRIVER_OPEN(h);
    if (!img || !out || !out_bytes || out_cap < 0 || !tiff_args_ok(H, W, spp)) return fail(h, ECSEG_E_INVALID, "tiff_encode: bad arguments");
    *out_bytes = 0;
    const int rps = tiff_rows_per_strip(H, W, spp);
    if ((H + rps - 1) / rps >= (1 << 26)) return fail(h, ECSEG_E_INVALID, "tiff_encode: 2^26 strips or more (such a file would pass 4 GiB)");
    USE_DEVICE(h);
    int rc;
    TiffEncodeBufs b{};
    if ((rc = lay_out(h, h->call_arena, [&](Carver& c) { b = tiff_encode_bufs(c, H, W, spp, 1, true); }))) return rc;
    hipStream_t s = h->stream;
    clear_timings(h);
    HIP_TRY(h, hipMemcpyAsync(b.img, img, (size_t)H * W * spp, hipMemcpyHostToDevice, s));
    TIMED(h, s, 0, 1, HIP_TRY(h, run_tiff_encode(TiffSources{{b.img, nullptr, nullptr}, 0}, 1, H, W, spp, invert, b, s)));
    if ((rc = tiff_collect(h, "tiff_encode", 1, H, W, spp, b, &out, out_cap, out_bytes, true))) return rc;   // (waits for the stream)
    timed_set(h, 0, 1);
    return ECSEG_OK;
}

// ---- the same over a batch of rasters: every strip of every file is a wave of one launch -------------------------------------------
long long ecseg_tiff_encode_batch_bytes(const int64_t* files, int n_files) {
    if (n_files == 0) return 0;
    if (n_files < 0 || n_files >= 65536 || !files) return -1;
    std::vector<TeFileIn> in;
    TeBatchLayout L;
    if (!tiff_encode_batch_plan(files, n_files, -1, in).empty() || !te_batch_layout(in, L).empty()) return -1;
    Carver c;
    (void)tiff_encode_batch_bufs(c, L, true);
    return (long long)c.used;
}

int ecseg_tiff_encode_batch(ecseg_ctx* h, const uint8_t* rasters, long long raster_bytes, const int64_t* files, int n_files, uint8_t* out,
                            long long out_cap, int64_t* out_ranges) {
    DRIVER_OPEN(h);
    const std::string me = "tiff_encode_batch: ";
    if (n_files < 0 || raster_bytes < 0 || out_cap < 0 || (n_files > 0 && (!rasters || !files || !out || !out_ranges)))
        return fail(h, ECSEG_E_INVALID, me + "bad arguments");
    if (n_files >= 65536) return fail(h, ECSEG_E_INVALID, me + "65536 files or more");
    clear_timings(h);
    if (n_files == 0) return ECSEG_OK;
    std::vector<TeFileIn> in;
    TeBatchLayout L;
    std::string bad = tiff_encode_batch_plan(files, n_files, raster_bytes, in);
    if (bad.empty()) bad = te_batch_layout(in, L);
    if (!bad.empty()) return fail(h, ECSEG_E_INVALID, me + bad);
    USE_DEVICE(h);
    int rc;
    TiffEncodeBatchBufs b{};
    if ((rc = lay_out(h, h->call_arena, [&](Carver& c) { b = tiff_encode_batch_bufs(c, L, true); }))) return rc;
    hipStream_t s = h->stream;
    HIP_TRY(h, hipMemcpyAsync(b.src, rasters + L.src_base, (size_t)L.src_span, hipMemcpyHostToDevice, s));
    HIP_TRY(h, hipMemcpyAsync(b.tab, L.tab.data(), L.tab.size() * sizeof(TeFile), hipMemcpyHostToDevice, s));
    TIMED(h, s, 0, 1, HIP_TRY(h, run_tiff_encode_batch(b, L, s)));
    if ((rc = tiff_batch_collect(h, "tiff_encode_batch", L, b, out, out_cap, out_ranges))) return rc;   // (waits for the stream: L lives until here)
    timed_set(h, 0, 1);
    return ECSEG_OK;
}

// ---- TIFF files decoded on the device -------------------------------------------------------------------------------------------
// (the four handle-free questions: a word with a bit outside the three ECSEG_TIFF_* is a bad argument)
static bool tiff_kinds_ok(unsigned kinds) { return !(kinds & ~(ECSEG_TIFF_DEFLATE | ECSEG_TIFF_TILED | ECSEG_TIFF_PACKBITS)); }

int ecseg_tiff_decode_routes(const uint8_t* file, long long n_bytes, unsigned kinds) {
    TiffInfo t;
    return file && n_bytes >= 0 && tiff_kinds_ok(kinds) && parse_tiff(file, (size_t)n_bytes, &t, kinds) == ECSEG_OK && tiff_goes_to_device(t, kinds) ? 1 : 0;
}

int ecseg_tiff_decode(ecseg_ctx* h, const uint8_t* file, long long n_bytes, void* dst, long long dst_bytes, int* H, int* W, int* samples_per_pixel,
                      int* bits_per_sample) {
    DRIVER_OPEN(h);
    if (!file || n_bytes < 0 || !H || !W || !samples_per_pixel || !bits_per_sample || (dst && dst_bytes < 0))
        return fail(h, ECSEG_E_INVALID, "tiff_decode: bad arguments");
    clear_timings(h);                                        // (before the file is judged: a call that only measures, or refuses, leaves zeros)
    TiffInfo t;
    std::string why;
    const size_t n = (size_t)n_bytes;
    bool parsed = false;
    int rc = tiff_decode_verdict(file, n, false, h->tiff_kinds, t, &parsed, why);
    if (parsed) { *H = (int)t.H; *W = (int)t.W; *samples_per_pixel = (int)t.spp; *bits_per_sample = (int)t.bits; }
    if (rc != ECSEG_OK) return fail(h, rc, "tiff_decode: " + why);
    const unsigned long long bpp = t.bits / 8, line = (unsigned long long)t.W * t.spp * bpp, total = line * t.H;
    if (!dst) return ECSEG_OK;
    if ((unsigned long long)dst_bytes < total) return fail(h, ECSEG_E_INVALID, "tiff_decode: the destination holds fewer bytes than the image");
    if ((rc = tiff_strips_in_file(t, n, why)) != ECSEG_OK) return fail(h, rc, "tiff_decode: " + why);
    TiffsPlan p;                                             // a batch of one: the file at the head of the upload, its raster at the head of dst
    const std::string bad = td_batch_layout({td_file_in(t, 0, n)}, p.L);
    if (!bad.empty()) return fail(h, ECSEG_E_INVALID, "tiff_decode: " + bad);
    tiff_plan_tables({t}, p);
    USE_DEVICE(h);
    TiffDecodeBatchBufs b{};
    if ((rc = lay_out(h, h->call_arena, [&](Carver& c) { b = tiff_decode_batch_bufs(c, p.L); }))) return rc;
    hipStream_t s = h->stream;
    if ((rc = tiff_batch_launch(h, file, p, b, s, h->ev[0], h->ev[1]))) return rc;
    uint32_t corrupt = 0;
    HIP_TRY(h, hipMemcpyAsync(&corrupt, b.file_status, sizeof corrupt, hipMemcpyDeviceToHost, s));
    WAIT_SET(h, s, 0, 1);                                    // (p and the caller's file are read by the copies above: they live until here)
    if (corrupt) {                                           // the batch folds the strips into one word per file: which strip it was
        std::vector<uint32_t> status((size_t)p.L.n_strips);
        HIP_TRY(h, hipMemcpyAsync(status.data(), b.strip_status, status.size() * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
        HIP_TRY(h, hipStreamSynchronize(s));
        const size_t k = std::find_if(status.begin(), status.end(), [](uint32_t v) { return v != 0; }) - status.begin();
        return fail(h, ECSEG_E_INVALID, std::string("tiff_decode: ") + (t.tw ? "tile " : "strip ") + std::to_string(k) + " holds a corrupt " +
                               (t.comp == 5 ? "LZW" : t.comp == 32773 ? "PackBits" : "Deflate") + " stream");
    }
    HIP_TRY(h, hipMemcpyAsync(dst, b.rasters, (size_t)total, hipMemcpyDeviceToHost, s));
    HIP_TRY(h, hipStreamSynchronize(s));
    return ECSEG_OK;
}

// ---- the same over a batch of files: every strip of every file is a wave of one launch ----------------------------------------------
int ecseg_tiff_decode_batch_counts(const uint8_t* file, long long n_bytes, unsigned kinds) {
    TiffInfo t;
    std::string why;
    bool parsed = false;
    return file && n_bytes >= 0 && tiff_kinds_ok(kinds) && tiff_decode_verdict(file, (size_t)n_bytes, true, kinds, t, &parsed, why) == ECSEG_OK &&
                   tiff_batch_counts(t, kinds) ? 1 : 0;
}

int ecseg_tiff_decode_batch_routes(const uint8_t* files, long long files_bytes, const int64_t* file_ranges, int n_files, unsigned kinds) {
    if (n_files <= 0 || !files || !file_ranges || files_bytes < 0 || !tiff_kinds_ok(kinds)) return 0;
    std::vector<TiffInfo> info; std::vector<int> status; std::vector<TdFileIn> in;
    if (!tiff_batch_plan(files, files_bytes, file_ranges, n_files, nullptr, true, info, status, in, kinds).empty()) return 0;
    std::vector<const TiffInfo*> ok;
    for (int i = 0; i < n_files; ++i) if (status[(size_t)i] == ECSEG_OK) ok.push_back(&info[(size_t)i]);
    return tiff_batch_goes_to_device(ok.data(), ok.size(), kinds) ? 1 : 0;
}

// (The Deflate kernel keeps its tables in LDS and takes nothing from the arena: a Deflate file needs what an LZW file of its tags needs.
// A tiled file needs its row of the tiled-file table and the staging slots of its compressed tiles on top: tiff_decode_batch_bufs.
// The PackBits kernel stages its stream in LDS: a PackBits file needs what an LZW file of its tags needs.)
long long ecseg_tiff_decode_batch_bytes(const uint8_t* files, long long files_bytes, const int64_t* file_ranges, int n_files, unsigned kinds) {
    if (!tiff_kinds_ok(kinds)) return -1;
    if (n_files == 0) return 0;
    if (n_files < 0 || !files || !file_ranges || files_bytes < 0) return -1;
    std::vector<TiffInfo> info; std::vector<int> status; std::vector<TdFileIn> in;
    if (!tiff_batch_plan(files, files_bytes, file_ranges, n_files, nullptr, true, info, status, in, kinds).empty()) return -1;
    TdBatchLayout L;
    if (!td_batch_layout(in, L).empty()) return -1;
    Carver c;
    (void)tiff_decode_batch_bufs(c, L);
    return (long long)c.used;
}

int ecseg_tiff_decode_batch(ecseg_ctx* h, const uint8_t* files, long long files_bytes, const int64_t* file_ranges, int n_files, void* dst,
                            long long dst_bytes, const int64_t* dst_offsets, int32_t* shapes, int32_t* status) {
    DRIVER_OPEN(h);
    const std::string me = "tiff_decode_batch: ";
    if (n_files < 0 || files_bytes < 0 || (n_files > 0 && (!files || !file_ranges || !shapes || !status)) ||
        (dst && (dst_bytes < 0 || (n_files > 0 && !dst_offsets))))
        return fail(h, ECSEG_E_INVALID, me + "bad arguments");
    clear_timings(h);                                        // (as ecseg_tiff_decode)
    if (n_files == 0) return ECSEG_OK;
    const size_t nf = (size_t)n_files;
    std::vector<TiffInfo> info; std::vector<TdFileIn> in;
    TiffsPlan p;
    std::vector<int>& verdict = p.verdict;
    TdBatchLayout& L = p.L;
    std::string bad = tiff_batch_plan(files, files_bytes, file_ranges, n_files, dst ? dst_offsets : nullptr, dst != nullptr, info, verdict, in,
                                      h->tiff_kinds);
    if (!bad.empty()) return fail(h, ECSEG_E_INVALID, me + bad);
    if (dst) {                                               // every raster inside the destination and clear of the others
        std::vector<std::pair<uint64_t, uint64_t>> spans;   // (offset, end) of the files that are decoded
        for (size_t i = 0; i < nf; ++i) {
            if (!in[i].in_batch) continue;
            const uint64_t total = (uint64_t)in[i].W * in[i].spp * in[i].bps * in[i].H;
            if (in[i].dst_off > (uint64_t)dst_bytes || total > (uint64_t)dst_bytes - in[i].dst_off)
                return fail(h, ECSEG_E_INVALID, me + "file " + std::to_string(i) + ": its raster leaves the " + std::to_string(dst_bytes) + " bytes of the destination");
            spans.emplace_back(in[i].dst_off, in[i].dst_off + total);
        }
        std::sort(spans.begin(), spans.end());
        for (size_t k = 1; k < spans.size(); ++k)
            if (spans[k].first < spans[k - 1].second) return fail(h, ECSEG_E_INVALID, me + "two rasters overlap in the destination");
    }
    if (dst && !(bad = td_batch_layout(in, L)).empty()) return fail(h, ECSEG_E_INVALID, me + bad);
    for (size_t i = 0; i < nf; ++i) {
        const TiffInfo& t = info[i];
        int32_t* q = shapes + 4 * i;
        q[0] = (int32_t)t.H; q[1] = (int32_t)t.W; q[2] = t.H ? (int32_t)t.spp : 0; q[3] = t.H ? (int32_t)t.bits : 0;
        status[i] = verdict[i];
    }
    if (!dst || L.n_strips == 0) return ECSEG_OK;
    USE_DEVICE(h);
    int rc;
    TiffDecodeBatchBufs b{};
    if ((rc = lay_out(h, h->call_arena, [&](Carver& c) { b = tiff_decode_batch_bufs(c, L); }))) return rc;
    tiff_plan_tables(info, p);
    hipStream_t s = h->stream;
    if ((rc = tiff_batch_launch(h, files, p, b, s, h->ev[0], h->ev[1]))) return rc;
    std::vector<uint32_t> corrupt(nf, 0);
    HIP_TRY(h, hipMemcpyAsync(corrupt.data(), b.file_status, nf * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    WAIT_SET(h, s, 0, 1);                     // (p is read by the copies above: it lives until here)
    // the rasters of the clean files, a run without a gap in one copy: all of them at once where the caller packed them
    std::vector<std::pair<uint64_t, uint64_t>> runs;
    for (size_t i = 0; i < nf; ++i) {
        if (!L.tab[i].in_batch) continue;
        if (corrupt[i]) { status[i] = ECSEG_E_INVALID; continue; }
        runs.emplace_back(L.tab[i].raster_off, L.tab[i].raster_off + td_file_raster_bytes(L.tab[i]));
    }
    std::sort(runs.begin(), runs.end());
    for (size_t k = 0; k < runs.size();) {
        size_t e = k + 1;
        uint64_t end = runs[k].second;
        while (e < runs.size() && runs[e].first == end) end = runs[e++].second;
        HIP_TRY(h, hipMemcpyAsync(static_cast<uint8_t*>(dst) + L.dst_base + runs[k].first, b.rasters + runs[k].first, (size_t)(end - runs[k].first),
                                  hipMemcpyDeviceToHost, s));
        k = e;
    }
    HIP_TRY(h, hipStreamSynchronize(s));
    return ECSEG_OK;
}

// ---- label PNG files encoded on the device ----------------------------------------------------------------------------------------
int ecseg_png_labels_encode(ecseg_ctx* h, const uint8_t* labels, int n_img, int H, int W, uint8_t* const* files, long long file_cap,
                            long long* file_bytes) {
    DRIVER_OPEN(h);
    if (n_img < 0 || n_img >= 65536 || H <= 0 || W <= 0 || W >= (1 << 30) || file_cap < 1 || (n_img > 0 && (!labels || !files || !file_bytes)))
        return fail(h, ECSEG_E_INVALID, "png_labels_encode: bad arguments");
    for (int i = 0; i < n_img; ++i) if (!files[i]) return fail(h, ECSEG_E_INVALID, "png_labels_encode: a null file buffer");
    clear_timings(h);
    if (n_img == 0) return ECSEG_OK;
    for (int i = 0; i < n_img; ++i) file_bytes[i] = 0;
    USE_DEVICE(h);
    int rc;
    PngEncodeBufs b{};
    if ((rc = lay_out(h, h->call_arena, [&](Carver& c) { b = png_encode_bufs(c, H, W, n_img, true); }))) return rc;
    HIP_TRY(h, hipMemcpyAsync(b.labels, labels, (size_t)n_img * H * W, hipMemcpyHostToDevice, h->stream));
    return png_encode_files(h, "png_labels_encode", b.labels, n_img, H, W, b, files, file_cap, file_bytes, &h->stage_ms[ECSEG_T_COUNT]);
}

// ---- gray PNG files (one channel of an interleaved image) encoded on the device ---------------------------------------------------
long long ecseg_png_channel_bound(int H, int W) {
    if (H < 1 || W < 1) return -1;
    return (long long)label_png_file_bytes(gray_png_stream_bound((size_t)H * ((size_t)W + 1)));
}

int ecseg_png_channel_encode(ecseg_ctx* h, const uint8_t* pixels, int n_img, int H, int W, int C, int channel, int invert, uint8_t* const* files,
                             long long file_cap, long long* file_bytes) {
    DRIVER_OPEN(h);
    if (n_img < 0 || n_img >= 65536 || H <= 0 || W <= 0 || C <= 0 || C > 256 || channel < 0 || channel >= C || file_cap < 1 ||
        ((size_t)W + 1) * (size_t)H >= 0x7fffffffull || (n_img > 0 && (!pixels || !files || !file_bytes)))
        return fail(h, ECSEG_E_INVALID, "png_channel_encode: bad arguments");
    for (int i = 0; i < n_img; ++i) if (!files[i]) return fail(h, ECSEG_E_INVALID, "png_channel_encode: a null file buffer");
    clear_timings(h);
    if (n_img == 0) return ECSEG_OK;
    for (int i = 0; i < n_img; ++i) file_bytes[i] = 0;
    USE_DEVICE(h);
    int rc;
    GrayEncodeBufs b{};
    if ((rc = lay_out(h, h->call_arena, [&](Carver& c) { b = gray_encode_bufs(c, H, W, C, n_img, n_img, true); }))) return rc;
    const size_t img_bytes = (size_t)H * W * C;
    HIP_TRY(h, hipMemcpyAsync(b.px, pixels, (size_t)n_img * img_bytes, hipMemcpyHostToDevice, h->stream));
    const GraySource src{b.px, img_bytes, (uint32_t)W, (uint32_t)C, (uint32_t)(((size_t)W + 1) * (size_t)H), 1u, (uint32_t)channel, invert ? 1u : 0u};
    return png_gray_encode(h, "png_channel_encode", src, n_img, H, W, b, files, file_cap, file_bytes, &h->stage_ms[ECSEG_T_COUNT]);
}

}  // extern "C"
