// Host and device: the layout of ecseg_stat_fish_batch (drivers_fish.hip, the fsb_* kernels of fishspot_kernels.hip), stated once and
// shared with the host program that walks it under ASan + UBSan (tools/asan/fish_batch_check.cpp).  No HIP in here.
//
// One call holds a chunk of images of any extents.  Three kinds of device memory:
//   * `work`, bytes: per image its rasters - the image, thresholded (C - 1 bytes per pixel), boundaries, the mask where it is not the
//     mask file, and the up to five rasters that are encoded - every one on a multiple of 256 bytes (fs_render_kernel reads dwords);
//   * typed per-pixel arrays indexed by ELEMENT: lab and rid (int32, one element per pixel, the images back to back in call order, so
//     rid is one sequence for one scan and lab is the packed `ranks` output), par and sz (int32, four planes per image at 4 * lab).
//     An image of 41 x 43 ends on an odd byte of `work`; its int32 / float64 data never lie in `work`, so nothing is misaligned;
//   * padded planes for the images that come as masks: they are labelled by the same-shape batched labelling the interSeg batch uses
//     (iseg_batch.h: padded to the largest extent Hm x Wm on the right and below, which keeps the raster order of first pixels).
// Union-find parents stay indices inside their image: a kernel moves the pointer (par + row.par), never the values.
//   The K x K weights of image i lie at element row.w of one float64 array; K differs per image and the threshold kernel's LDS is
// sized for the largest K the entry point takes, so images of different K share a launch.
#pragma once
#include <stdint.h>

#include <string>
#include <vector>

#include "iseg_batch.h"
#include "scratch.h"

namespace ecseg {

constexpr int FSB_MAX_IMAGES = 8192;                   // 5 files each stay below the encoder's 65536; grid dimension y is the image
constexpr int FSB_MAX_KERNEL = 63;                     // ECSEG_FISH_SPOT_MAX_KERNEL
constexpr int FSB_FILES = 5;                           // original, with_segmentation, lsq, mask, picture

// One image as the fsb_* kernels read it.
struct FsImage {
    long long img, thr, bnd, msk;                      // byte offsets into `work` (msk: the mask the labelling reads; -1 with given labels)
    long long file[FSB_FILES];                         // byte offsets into `work` of the encoded rasters, -1: no such file
    long long lab;                                     // element offset into lab / rid; par / sz: 4 * lab
    long long w;                                       // element offset of the K * K weights
    long long pad;                                     // element offset of the image's plane of the padded arrays, -1 with given labels
    double normal_thr, ithr[3];
    int32_t H, W, C, np;                               // np = C - 1 probes
    int32_t ch[4];                                     // blue, green, red, aqua channel; the probes are ch[1 .. np]
    int32_t K, min_cc;
    int32_t rec0, n_cells;                             // written by the device plan: first record of the chunk's records, and how many
};
static_assert(sizeof(FsImage) % 8 == 0, "an array of rows holding 64-bit fields");

// What the layout needs to know of an image.
struct FsImageIn { int32_t H = 0, W = 0, C = 0, K = 0; bool given_labels = false, mask_file = false, mask_is_file = false, picture = false; };

struct FsBatchLayout {
    std::vector<FsImage> tab;
    std::vector<int64_t> files;                        // rows of tiff_encode_batch_plan: (offset into work, H, W, spp, 0) per encoded raster
    size_t work = 0;                                   // bytes
    size_t px = 0;                                     // elements of lab and rid
    size_t w = 0;                                      // float64 weights
    int n_pad = 0, Hm = 0, Wm = 0;                     // the images that come as masks, and their largest extents
    int max_px = 0, max_H = 0, max_W = 0;              // of one image: they size the grids
};

// Empty string and L, or which image is wrong and why.  Only geometry is judged here; pointers and parameters are the driver's.
inline std::string fs_batch_layout(const std::vector<FsImageIn>& in, FsBatchLayout& L) {
    L = FsBatchLayout();
    if (in.size() > (size_t)FSB_MAX_IMAGES) return "more than " + std::to_string(FSB_MAX_IMAGES) + " images";
    L.tab.resize(in.size());
    auto take = [&](size_t bytes) { const size_t o = L.work; L.work += (bytes + 255) / 256 * 256; return (long long)o; };
    const long long lim = 1ll << 31;
    for (size_t i = 0; i < in.size(); ++i) {
        const FsImageIn& f = in[i];
        const std::string who = "image " + std::to_string(i) + ": ";
        if (f.H < 1 || f.W < 1) return who + "H and W must be at least 1";
        if (f.C < 3 || f.C > 4) return who + "the image must have 3 or 4 channels, not " + std::to_string(f.C);
        if (f.K < 1 || f.K > FSB_MAX_KERNEL || f.K % 2 == 0)
            return who + "the kernel side must be odd and between 1 and " + std::to_string(FSB_MAX_KERNEL);
        if ((long long)f.H * f.W >= lim) return who + "image too large (H * W must be below 2^31)";
        if ((long long)f.W * 3 >= (1ll << 30)) return who + "the TIFF writer takes lines below 2^30 bytes";
        const size_t px = (size_t)f.H * f.W;
        FsImage& t = L.tab[i];
        t = FsImage();
        t.H = f.H; t.W = f.W; t.C = f.C; t.np = f.C - 1; t.K = f.K;
        t.img = take(px * f.C); t.thr = take(px * (f.C - 1)); t.bnd = take(px);
        for (int k = 0; k < FSB_FILES; ++k) {
            const int spp = k == 3 ? 1 : 3;
            const bool has = k < 3 || (k == 3 ? f.mask_file : f.picture);
            t.file[k] = has ? take(px * spp) : -1;
            if (!has) continue;
            const int64_t row[5] = {t.file[k], f.H, f.W, spp, 0};
            L.files.insert(L.files.end(), row, row + 5);
        }
        t.msk = f.given_labels ? -1 : (f.mask_is_file && f.mask_file ? t.file[3] : take(px));
        t.lab = (long long)L.px;
        t.w = (long long)L.w;
        L.px += px;
        L.w += (size_t)f.K * f.K;
        t.pad = -1;
        if (!f.given_labels) {
            L.n_pad += 1;
            L.Hm = f.H > L.Hm ? f.H : L.Hm;
            L.Wm = f.W > L.Wm ? f.W : L.Wm;
        }
        L.max_px = (int)px > L.max_px ? (int)px : L.max_px;
        L.max_H = f.H > L.max_H ? f.H : L.max_H;
        L.max_W = f.W > L.max_W ? f.W : L.max_W;
    }
    if ((long long)L.px >= lim) return "the chunk holds 2^31 pixels or more (split it)";
    if ((long long)L.n_pad * L.Hm * L.Wm >= lim) return "the chunk's masks, padded to the largest one, hold 2^31 pixels or more (split it)";
    long long m = 0;
    for (size_t i = 0; i < in.size(); ++i)
        if (!in[i].given_labels) L.tab[i].pad = (m++) * (long long)L.Hm * L.Wm;
    return std::string();
}

// The padded images' rows as the shared pad-and-label launcher takes them (only seg_off, h and w are read).
inline std::vector<IsegImage> fs_batch_pad_table(const FsBatchLayout& L) {
    std::vector<IsegImage> out;
    for (const FsImage& t : L.tab)
        if (t.pad >= 0) out.push_back(IsegImage{t.img, t.msk, t.H, t.W, t.C, t.H, t.W, 0});
    return out;
}

// Device buffers of one call, sized before the first launch.  plan: per image (cells, 1 when a given label exceeds H * W) and one
// last pair holding the chunk's cells; mx: 4 per image.
struct FsBatchBufs {
    uint8_t* work; FsImage* tab; int32_t* lab; int32_t* rid; int32_t* blk; int32_t* par; int32_t* sz; int32_t* mx; int32_t* plan;
    int32_t* total; double* w; IsegImage* ptab; uint8_t* pmask; int32_t* plab;
};
inline FsBatchBufs fs_batch_bufs(Carver& c, const FsBatchLayout& L) {
    const size_t n = L.tab.size(), pad = (size_t)L.n_pad * L.Hm * L.Wm;
    FsBatchBufs b;
    b.work = c.take<uint8_t>(L.work); b.tab = c.take<FsImage>(n); b.lab = c.take<int32_t>(L.px); b.rid = c.take<int32_t>(L.px);
    b.blk = c.take<int32_t>((L.px + 1023) / 1024); b.par = c.take<int32_t>(L.px * 4); b.sz = c.take<int32_t>(L.px * 4);
    b.mx = c.take<int32_t>(n * 4); b.plan = c.take<int32_t>((n + 1) * 2); b.total = c.take<int32_t>(4); b.w = c.take<double>(L.w);
    b.ptab = c.take<IsegImage>((size_t)L.n_pad); b.pmask = c.take<uint8_t>(pad); b.plab = c.take<int32_t>(pad);
    return b;
}
// ... and what is sized by the chunk's cell count, known after the plan: accumulators (12 uint64), spot counters (8 uint32), label
// values and records (24 int64) per cell.
struct FsBatchCellBufs { unsigned long long* acc; unsigned* cnt; int32_t* val; int64_t* rec; };
inline FsBatchCellBufs fs_batch_cell_bufs(Carver& c, size_t cells) {
    FsBatchCellBufs b;
    b.acc = c.take<unsigned long long>(cells * 12); b.cnt = c.take<unsigned>(cells * 8); b.val = c.take<int32_t>(cells);
    b.rec = c.take<int64_t>(cells * 24);
    return b;
}

// The byte count of fs_batch_bufs restated slot by slot, every slot rounded up to 256 bytes (scratch.h); the driver and the host check
// compare the two.
inline long long fs_round256(long long b) { return b ? (b + 255) / 256 * 256 : 256; }
inline long long fs_batch_bytes(const FsBatchLayout& L) {
    const long long n = (long long)L.tab.size(), px = (long long)L.px, pad = (long long)L.n_pad * L.Hm * L.Wm;
    return fs_round256((long long)L.work) + fs_round256(n * (long long)sizeof(FsImage)) + 2 * fs_round256(px * 4) + fs_round256((px + 1023) / 1024 * 4) +
           2 * fs_round256(px * 16) + fs_round256(n * 16) + fs_round256((n + 1) * 8) + fs_round256(16) + fs_round256((long long)L.w * 8) +
           fs_round256((long long)L.n_pad * (long long)sizeof(IsegImage)) + fs_round256(pad) + fs_round256(pad * 4);
}
inline long long fs_batch_cell_bytes(long long cells) {
    return fs_round256(cells * 96) + fs_round256(cells * 32) + fs_round256(cells * 4) + fs_round256(cells * 192);
}

}  // namespace ecseg
