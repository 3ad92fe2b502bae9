// A batch of rasters for one encode (ecseg_tiff_encode_batch, drivers_files.hip; ecseg_fish_render_tiff_batch, drivers_fish.hip; the
// tiffb_* kernels of tiff_kernels.hip): the device table, one TeFile row per file, and the one function that lays a batch out - the
// strip plan of every file (the host writer's tiff_rows_per_strip, nothing else), the running sum over strips that gives every
// workgroup its file, where every slot, count, strip offset and packed byte lies, and the arena the call carves.  Plain C++: the
// drivers include it, and so does tools/asan/tiff_encode_batch_fuzz.cpp (as tiff_decode_batch.h serves the reader).
//   The files of a batch may differ in extent, samples per pixel (1 or 3), strip plan and `invert`.  The rasters lie in one packed
// buffer (the upload, or what the render kernels left on the device), file f at src_off.  A file's image is
//   head (8 bytes) | its strips back to back, every one on an even offset | tail
// and head and tail have a size the layout knows (te_frame_bytes: the tail holds the two strip tables, BitsPerSample and the IFD,
// and the strips' total is even, so there is no pad byte).  The device therefore packs the strips where they lie in the output of
// the call - the file images back to back: tiffb_place_kernel sums frame + strips over the files in front into `base`, and the gather
// writes file f's strips from base[f] + 8 on.  One copy brings all files over and the host writes heads and tails into the gaps.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <string>
#include <vector>

#include "scratch.h"
#include "tiff_frame.h"

namespace ecseg {

struct TeFile {
    uint64_t src_off;        // of the raster in the packed raster buffer
    uint64_t slot_off;       // of the file's first slot in the slot buffer, in bytes; strip k's slot lies k * slot_stride behind it
    uint64_t slot_stride;    // bytes of a slot: the host's bound for a strip, rounded up to 16
    uint64_t off_off;        // of the file's strip offsets in the offset buffer, in entries: n_strips + 1 of them, the last one their total
    uint64_t frame_bytes;    // 8 + the tail: what the host puts around the strips
    uint32_t H, W, spp, rps;
    uint32_t flip;           // 0xff with `invert`, else 0
    uint32_t first_strip;    // global index of strip 0 (grid x of tiffb_lzw_strip_kernel, and the strip's place in the counts)
    uint32_t n_strips;       // ceil(H / rps), at least 1
    uint32_t pad;
};
static_assert(sizeof(TeFile) == 72, "the device table is an array of 72-byte rows, copied as it is");

struct TeFileIn { uint64_t src_off = 0; uint32_t H = 0, W = 0, spp = 1; bool invert = false; };

struct TeBatchLayout {
    std::vector<TeFile> tab;
    uint64_t src_base = 0, src_span = 0;         // the upload: bytes [src_base, src_base + src_span) of the caller's rasters
    uint64_t n_strips = 0;                       // the grid of the strip kernel, and the counts
    uint32_t max_strips = 0;                     // of one file: grid x of the gather
    uint64_t slot_bytes = 0, off_entries = 0;
    uint64_t packed_bytes = 0;                   // room for every file image with every strip as long as its slot
};

constexpr uint64_t TE_BATCH_MAX_GRID = (1ull << 31) - 1;     // grid dimension x
constexpr uint32_t TE_BATCH_MAX_FILES = 65535;               // grid dimension y is the file
constexpr uint32_t TE_FILE_MAX_STRIPS = (1u << 26) - 1;      // (a file of more would pass 4 GiB: ecseg_tiff_encode's rule)

// bytes of head and tail of a file of n strips (tiff_frame, host_io.cpp): the tables with more than one strip, BitsPerSample with
// three samples, the IFD of 12 entries
inline uint64_t te_frame_bytes(uint32_t n_strips, uint32_t spp) {
    return 8 + (n_strips > 1 ? 8ull * n_strips : 0ull) + (spp > 2 ? 2ull * spp : 0ull) + 2 + 12 * 12 + 4;
}

// Empty string, or what is wrong.  The caller has checked the extents (tiff_args_ok) and that the rasters do not overlap.
inline std::string te_batch_layout(const std::vector<TeFileIn>& in, TeBatchLayout& L) {
    L = TeBatchLayout();
    if (in.size() > TE_BATCH_MAX_FILES) return "65536 files or more";
    L.tab.resize(in.size());
    uint64_t lo = UINT64_MAX, hi = 0;
    for (const TeFileIn& f : in) {
        const uint64_t raster = (uint64_t)f.W * f.spp * f.H;
        lo = f.src_off < lo ? f.src_off : lo;
        hi = f.src_off + raster > hi ? f.src_off + raster : hi;
    }
    if (lo == UINT64_MAX) lo = hi = 0;
    L.src_base = lo; L.src_span = hi - lo;
    for (size_t i = 0; i < in.size(); ++i) {
        const TeFileIn& f = in[i];
        TeFile& t = L.tab[i];
        t = TeFile();
        const uint64_t line = (uint64_t)f.W * f.spp;
        const int rps = tiff_rows_per_strip((int)f.H, (int)f.W, (int)f.spp);
        const uint64_t ns = ((uint64_t)f.H + rps - 1) / rps;
        if (ns > TE_FILE_MAX_STRIPS) return "file " + std::to_string(i) + ": 2^26 strips or more (such a file would pass 4 GiB)";
        t.src_off = f.src_off - L.src_base;
        t.H = f.H; t.W = f.W; t.spp = f.spp; t.rps = (uint32_t)rps; t.flip = f.invert ? 0xffu : 0u;
        t.first_strip = (uint32_t)L.n_strips; t.n_strips = (uint32_t)ns;
        t.slot_stride = (tiff_strip_bound((size_t)(rps * line)) + 15) / 16 * 16;
        t.slot_off = L.slot_bytes; t.off_off = L.off_entries;
        t.frame_bytes = te_frame_bytes(t.n_strips, t.spp);
        L.n_strips += ns;
        if (L.n_strips > TE_BATCH_MAX_GRID) return "the batch holds 2^31 strips or more";
        L.max_strips = t.n_strips > L.max_strips ? t.n_strips : L.max_strips;
        L.slot_bytes += ns * t.slot_stride;
        L.off_entries += ns + 1;
        L.packed_bytes += t.frame_bytes + ns * t.slot_stride;
    }
    return std::string();
}

// Device buffers of one batch: the table, the rasters (`upload`: the call brings them; else they lie on the device already and the
// caller sets src), per strip its slot and its encoded length, per file its strip offsets, per file (and one more: the total) where
// its image starts in the packed output, and that output.
struct TiffEncodeBatchBufs { TeFile* tab; uint8_t* src; uint8_t* slots; uint32_t* cnt; unsigned long long* off; unsigned long long* base; uint8_t* packed; };
inline TiffEncodeBatchBufs tiff_encode_batch_bufs(Carver& c, const TeBatchLayout& L, bool upload) {
    TiffEncodeBatchBufs b;
    b.tab = c.take<TeFile>(L.tab.size()); b.src = c.take<uint8_t>(upload ? (size_t)L.src_span : 0); b.slots = c.take<uint8_t>((size_t)L.slot_bytes);
    b.cnt = c.take<uint32_t>((size_t)L.n_strips); b.off = c.take<unsigned long long>((size_t)L.off_entries);
    b.base = c.take<unsigned long long>(L.tab.size() + 1); b.packed = c.take<uint8_t>((size_t)L.packed_bytes);
    return b;
}

}  // namespace ecseg
