// Host and device: the planning arithmetic of ecseg_interseg_batch (drivers_interseg.hip, interseg_kernels.hip), stated once and
// shared with the host program that walks it under ASan + UBSan (tools/asan/iseg_batch_check.cpp): the table of a chunk's images,
// the groups a chunk is split into, how the caller's capacities are handed out image by image, the crop windows of a region
// (interseg.crop_windows / region_rows) and the runs of one image inside a classifier chunk.
//
// Labelling choice: the masks of a group are PADDED to the group's largest extent (Hm x Wm) and labelled by the same-shape batched
// labelling (run_ccl_labels).  Padding adds background only on the right and below, so the raster order of the components' first
// pixels - the region index - is that of the image alone.  The statistics and crop kernels read each image's true extents from the
// table; the images themselves are not padded, they are read where the packed buffer has them.
#pragma once
#include <stdint.h>

#include <string>
#include <vector>

#include "iseg_classify.h"

namespace ecseg {

constexpr int ISEG_BATCH_COLS = 8;                     // int64 per row of the caller's table
constexpr int ISEG_BATCH_MAX_IMAGES = 1024;
constexpr long long ISEG_BATCH_ARENA_LIMIT = 8ll << 30;   // call-arena bytes of one group; a chunk above it runs as several groups
constexpr int ISEG_DESC = 6;                           // int32 per crop descriptor: image (of the group), region, y0, x0, h, w
constexpr int ISEG_PLAN = 4;                           // int32 per image of the device plan: scan base, regions, record offset (-1: no room), spare

// per-image status of ecseg_interseg_batch (ECSEG_ISEG_* of the public header)
enum { ISEG_ST_OK = 0, ISEG_ST_INSTANCE_IDS = 1, ISEG_ST_RECORDS_OVERFLOW = 2, ISEG_ST_CROPS_OVERFLOW = 3 };

// One image as the kernels read it: the image (H, W, C) at img_off and its segmentation (h, w) at seg_off of the packed buffer
// (offsets relative to the group's first byte once iseg_batch_groups has run).
struct IsegImage {
    long long img_off, seg_off;
    int32_t H, W, C, h, w, run_c;
};

// `need` entries of a buffer of `cap` of which *used are taken: their offset, or -1 with nothing taken when they do not fit.
// The rule of both capacities of the call: an image that does not fit is reported and uses nothing, the images behind it go on.
ISEG_HD int iseg_take(int need, int* used, int cap) {
    if (need < 0 || need > cap - *used) return -1;
    const int off = *used;
    *used += need;
    return off;
}

// The crop windows of a bbox of bh x bw (interseg.crop_windows): the whole bbox when both are <= 256, else 256-stride tiles, a
// partial tile dropped unless the whole dimension is < 256.  Count, and window k of them as (dy, dx, th, tw).
ISEG_HD int iseg_axis_tiles(int n) { return n < 256 ? 1 : n / 256; }
ISEG_HD bool iseg_tiled(int bh, int bw) { return !(bh <= 256 && bw <= 256); }
ISEG_HD int iseg_window_count(int bh, int bw) { return iseg_tiled(bh, bw) ? iseg_axis_tiles(bh) * iseg_axis_tiles(bw) : 1; }
ISEG_HD void iseg_window(int bh, int bw, int k, int win[4]) {
    if (!iseg_tiled(bh, bw)) { win[0] = 0; win[1] = 0; win[2] = bh; win[3] = bw; return; }
    const int tx = iseg_axis_tiles(bw), r = k / tx, c = k % tx;
    win[0] = bh < 256 ? 0 : 256 * r; win[2] = bh < 256 ? bh : 256;
    win[1] = bw < 256 ? 0 : 256 * c; win[3] = bw < 256 ? bw : 256;
}
// the brightness gate of src/interseg.py:134 on a region record: sum / area < 12.75, exactly
ISEG_HD bool iseg_region_low(const int64_t* rec) { return 4 * rec[7] < 51 * rec[0]; }
// the crops of one region record (none below the gate)
inline int iseg_region_crops(const int64_t* rec) {
    return iseg_region_low(rec) ? 0 : iseg_window_count((int)(rec[3] - rec[1]), (int)(rec[4] - rec[2]));
}
// ... appended to desc (ISEG_DESC int32 each) and from_patches, for region `region` of image `image`
inline void iseg_region_descs(const int64_t* rec, int image, int region, std::vector<int32_t>& desc, std::vector<uint8_t>& from_patches) {
    const int bh = (int)(rec[3] - rec[1]), bw = (int)(rec[4] - rec[2]);
    const int n = iseg_region_crops(rec);
    for (int k = 0; k < n; ++k) {
        int win[4];
        iseg_window(bh, bw, k, win);
        const int32_t d[ISEG_DESC] = {image, region, (int32_t)rec[1] + win[0], (int32_t)rec[2] + win[1], win[2], win[3]};
        desc.insert(desc.end(), d, d + ISEG_DESC);
        from_patches.push_back(iseg_tiled(bh, bw) ? 1 : 0);
    }
}

// The end of the run of crops of one image that starts at crop `from` of a list whose crop k belongs to image desc[k * ISEG_DESC],
// not beyond `to`: a classifier chunk is selected run by run, since ecSeg-c applies per image.
inline int iseg_run_end(const int32_t* desc, int from, int to) {
    int e = from + 1;
    while (e < to && desc[(size_t)e * ISEG_DESC] == desc[(size_t)from * ISEG_DESC]) ++e;
    return e < to ? e : to;
}

// ---- the table ------------------------------------------------------------------------------------------------------------------
// images: n rows (img_off, H, W, C, seg_off, h, w, run_c).  The 2 n rasters lie in the packed buffer in the order image 0,
// segmentation 0, image 1, ...: each starts at or after the end of the one in front (gaps allowed, no overlap), and the last ends
// inside packed_bytes.  Empty string and the rows in tab, or which row is wrong.
inline std::string iseg_batch_table(const int64_t* images, int n, long long packed_bytes, std::vector<IsegImage>& tab) {
    tab.assign((size_t)(n > 0 ? n : 0), IsegImage{});
    long long end = 0;
    for (int i = 0; i < n; ++i) {
        const int64_t* r = images + (size_t)i * ISEG_BATCH_COLS;
        const std::string who = "image " + std::to_string(i);
        const long long lim = 1ll << 31;
        if (r[1] < 1 || r[2] < 1 || r[1] >= lim || r[2] >= lim || r[3] < 3 || r[3] > 256) return who + ": extents below 1 or channels outside 3 .. 256";
        if (r[5] < 1 || r[6] < 1 || r[5] > r[1] || r[6] > r[2]) return who + ": the segmentation is empty or larger than the image";
        if (r[5] * r[6] >= lim || r[1] * r[2] >= lim) return who + ": 2^31 pixels or more";
        if (r[7] != 0 && r[7] != 1) return who + ": run_c must be 0 or 1";
        const long long img_bytes = r[1] * r[2] * r[3], seg_bytes = r[5] * r[6];
        if (r[0] < end || r[0] > packed_bytes || img_bytes > packed_bytes - r[0]) return who + ": the image overlaps the raster in front or leaves the buffer";
        end = r[0] + img_bytes;
        if (r[4] < end || r[4] > packed_bytes || seg_bytes > packed_bytes - r[4]) return who + ": the segmentation overlaps the raster in front or leaves the buffer";
        end = r[4] + seg_bytes;
        tab[(size_t)i] = IsegImage{r[0], r[4], (int32_t)r[1], (int32_t)r[2], (int32_t)r[3], (int32_t)r[5], (int32_t)r[6], (int32_t)r[7]};
    }
    return std::string();
}

// ---- the groups -----------------------------------------------------------------------------------------------------------------
// Bytes of call arena for n images padded to Hm x Wm whose rasters span `span` bytes, with room for rec_cap records: the span, the
// table and the plan; per padded pixel the mask (1), the label map (4) and the region index (4) with its scan blocks; the counters;
// per record 32 + 16 + 64 bytes; one classifier chunk of crops with its descriptors (the batch's and classify_bufs' own), maxima and
// lists.  Every buffer rounded up to 256 bytes (scratch.h), as iseg_batch_bufs (common.h) lays them out; the driver compares the two.
inline long long iseg_round256(long long b) { return b ? (b + 255) / 256 * 256 : 256; }
inline long long iseg_batch_bytes(int n, int Hm, int Wm, long long span, int rec_cap) {
    const long long px = (long long)n * Hm * Wm, c = ISEG_CHUNK;
    return iseg_round256(span) + iseg_round256((long long)n * (long long)sizeof(IsegImage)) + iseg_round256((long long)n * ISEG_PLAN * 4) +
           iseg_round256(px) + 2 * iseg_round256(px * 4) + iseg_round256((px + 1023) / 1024 * 4) + iseg_round256(4 * 4) +
           iseg_round256((long long)n * 4 * 4) + iseg_round256((long long)rec_cap * 32) + iseg_round256((long long)rec_cap * 16) +
           iseg_round256((long long)rec_cap * 64) + iseg_round256(c * ISEG_DESC * 4) + iseg_round256(c * 5 * 4) + iseg_round256(c * 256 * 256 * 3) +
           iseg_round256(c * 3 * 4) + 2 * iseg_round256(c * 4);
}
struct IsegGroup { int first, n, Hm, Wm; long long base, span; };   // images first .. first + n - 1; their rasters are bytes base .. base + span
// Consecutive images go into one group while its arena stays within `limit` and its padded pixels below 2^31 (the kernels count
// them in 32 bits); an image above either alone is a group of its own (the table has bounded its pixels).
inline std::vector<IsegGroup> iseg_batch_groups(const std::vector<IsegImage>& tab, int rec_cap, long long limit = ISEG_BATCH_ARENA_LIMIT) {
    std::vector<IsegGroup> out;
    const int n = (int)tab.size();
    int i = 0;
    while (i < n) {
        IsegGroup g{i, 0, 0, 0, tab[(size_t)i].img_off, 0};
        while (g.first + g.n < n) {
            const IsegImage& t = tab[(size_t)(g.first + g.n)];
            const int Hm = t.h > g.Hm ? t.h : g.Hm, Wm = t.w > g.Wm ? t.w : g.Wm;
            const long long span = t.seg_off + (long long)t.h * t.w - g.base;
            const long long px = (long long)(g.n + 1) * Hm * Wm;
            if (g.n > 0 && (px >= (1ll << 31) || iseg_batch_bytes(g.n + 1, Hm, Wm, span, rec_cap) > limit)) break;
            g.n += 1; g.Hm = Hm; g.Wm = Wm; g.span = span;
        }
        out.push_back(g);
        i += g.n;
    }
    return out;
}

}  // namespace ecseg
