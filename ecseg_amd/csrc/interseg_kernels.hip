// interSeg's file-level driver on gfx950 (reference src/interseg.py:104-235): the nuclei of a segmentation image as
// region records, and the per-nucleus 256 x 256 crops the classifiers read.
//
// Regions (src/interseg.py:121-134: measure.label(seg, connectivity=None) + regionprops + the brightness gate)
//   * the 8-connected labels come from run_ccl_labels (label = 1 + raster index of the component's first pixel, the
//     pixel skimage numbers components by); the first pixels ("roots") are the pixels with label == index + 1, so the
//     exclusive scan of that flag (cell_util.h) read at a root is the component's skimage region index;
//   * iseg_region_stats_kernel relabels the map in place to region + 1 and accumulates area, bbox, sum of rows, sum of
//     columns and the sum of the reordered channel 0, on cell_util.h's statistics tile: the lanes of one region
//     (wave_key_groups) are folded with one shuffle butterfly, the fold's leader lane adds into the LDS table keyed by
//     region (lds_key_claim), and the table is flushed with one global atomic per (region, field, workgroup).
// Crops (src/interseg.py:131-133,150-152,193-194 and im2patches_overlap :27-46)
//   * crop (region, y0, x0, h, w), h, w <= 256: the window of the image with every pixel outside THIS region zeroed,
//     resized to 256 x 256 as skimage.transform.resize(order=1, mode='reflect', preserve_range=True).astype(uint8) does
//     with the exact affine map (scale h/256, offset scale/2 - 1/2): output row i samples row
//     (h (2i + 1) - 256) / 512, a multiple of 1/512, so the bilinear value is a multiple of 2^-18 and
//     value * 2^18 = sum of 4 weights (512 - f)(512 - g) ... times uint8 samples < 2^26 is exact in int32; trunc = >> 18.
//     No floating point on the value path.  Sample rows lie in [-1/2, h - 1/2]: the only out-of-window taps are -1 and
//     h, reflected to 1 and h - 2 (h = 1: row 0).
// A group of images in one call (ecseg_interseg_batch; planning in iseg_batch.h): the masks padded to one extent and labelled as a
// same-shape batch, the statistics tile and the crop rows above run per image through a device table of the images' own extents.
#include <algorithm>
#include <climits>

#include "common.h"
#include "cell_util.h"

namespace ecseg {

static constexpr int ISEG_CROP_ROWS = 16;        // crops kernel: output rows per block

// What a statistics tile reads: one image's label map, region index and mask, all with row stride `ls` (W for an image alone, the
// group's padded width in a batch), its image, the scan value at its first pixel (rid_base), the accumulator of its region 0
// (key_base) and how many of its regions have accumulators (cap).  vm[0] / vm[1]: largest non-zero segmentation value / 255 - smallest.
struct IsegStatView {
    int32_t* L; const int32_t* rid; const uint8_t* seg; const uint8_t* img;
    int H, W, ls, img_w, C, ch0, rid_base, key_base, cap;
    int32_t* vm;
};

// acc: per region (area, sum of rows, sum of columns, sum of channel 0) u64; bb: (min row, min col, -max row, -max col),
// all atomicMin, preset to 0x7f7f7f7f.  One workgroup = one tile of ONE image: the LDS key table never holds two images' regions.
__device__ __forceinline__ void iseg_region_stats_tile(const IsegStatView& q, u64* __restrict__ acc, int32_t* __restrict__ bb) {
    __shared__ int s_key[CELL_SLOTS];
    __shared__ unsigned s_area[CELL_SLOTS], s_sv[CELL_SLOTS];
    __shared__ u64 s_sr[CELL_SLOTS], s_sc[CELL_SLOTS];
    __shared__ int s_bb[4][CELL_SLOTS];
    __shared__ int s_vmax, s_vinv;
    const int t = threadIdx.x, lane = t & 63;
    const int H = q.H, W = q.W;
    if (t < CELL_SLOTS) {
        s_key[t] = -1; s_area[t] = 0; s_sv[t] = 0; s_sr[t] = 0; s_sc[t] = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j) s_bb[j][t] = INT_MAX;
    }
    if (t == 0) { s_vmax = 0; s_vinv = 0; }
    __syncthreads();
    const StatTile tile = stat_tile(W);
    const int xb = (int)tile.xb;                             // < W
    int vmax = 0, vinv = 0;
    for (int r = 0; r < CELL_ROWS_PER_WAVE; ++r) {
        const int y = tile.ybeg + r;
        if (y >= H) break;                                   // wave-uniform (a batch launches the largest image's tiles for every image)
        int reg = -1, v = 0;
        if (tile.x < (unsigned)W) {
            const size_t p = (size_t)y * q.ls + tile.x;
            const int l = q.L[p];
            if (l > 0) {
                reg = q.rid[l - 1] - q.rid_base;
                q.L[p] = reg + 1;
                const int sv = q.seg[p];
                vmax = max(vmax, sv);
                vinv = max(vinv, 255 - sv);
                v = q.img[((size_t)y * q.img_w + tile.x) * q.C + q.ch0];
                reg = reg < q.cap ? q.key_base + reg : -1;   // else counted, not accumulated: the caller's buffer is too small
            }
        }
        wave_key_groups(reg, [&](int key, bool mine, u64 m, int leader) {
            unsigned packed = mine ? ((unsigned)lane << 16) | (unsigned)v : 0u;   // sum of lanes <= 2016, sum of v <= 16320
#pragma unroll
            for (int d = 32; d >= 1; d >>= 1) packed += __shfl_xor(packed, d);
            if (lane != leader) return;
            const unsigned n = (unsigned)__popcll(m);
            const int xl = xb + leader, xr = xb + 63 - __clzll((long long)m);
            const u64 sr = (u64)y * n, sc = (u64)xb * n + (packed >> 16);
            const unsigned sv = packed & 0xffffu;
            const int found = lds_key_claim(s_key, key);
            if (found >= 0) {
                atomicAdd(&s_area[found], n); atomicAdd(&s_sr[found], sr); atomicAdd(&s_sc[found], sc); atomicAdd(&s_sv[found], sv);
                atomicMin(&s_bb[0][found], y); atomicMin(&s_bb[1][found], xl);
                atomicMin(&s_bb[2][found], -y); atomicMin(&s_bb[3][found], -xr);
            } else {                                         // more than 64 regions in one 64 x 32 tile: straight to the region
                u64* a = acc + (size_t)key * 4;
                atomicAdd(a + 0, (u64)n); atomicAdd(a + 1, sr); atomicAdd(a + 2, sc); atomicAdd(a + 3, (u64)sv);
                int32_t* b = bb + (size_t)key * 4;
                atomicMin(b + 0, y); atomicMin(b + 1, xl); atomicMin(b + 2, -y); atomicMin(b + 3, -xr);
            }
        });
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) { vmax = max(vmax, __shfl_xor(vmax, d)); vinv = max(vinv, __shfl_xor(vinv, d)); }
    if (lane == 0) { atomicMax(&s_vmax, vmax); atomicMax(&s_vinv, vinv); }
    __syncthreads();
    if (t < CELL_SLOTS && s_key[t] >= 0) {
        const int k = s_key[t];
        u64* a = acc + (size_t)k * 4;
        atomicAdd(a + 0, (u64)s_area[t]); atomicAdd(a + 1, s_sr[t]); atomicAdd(a + 2, s_sc[t]); atomicAdd(a + 3, (u64)s_sv[t]);
        int32_t* b = bb + (size_t)k * 4;
#pragma unroll
        for (int j = 0; j < 4; ++j) atomicMin(b + j, s_bb[j][t]);
    }
    if (t == 0) {
        if (s_vmax) atomicMax(q.vm + 0, s_vmax);
        if (s_vmax) atomicMax(q.vm + 1, s_vinv);
    }
}

// One image: misc[1] / misc[2] take the value range.
__global__ __launch_bounds__(256) void iseg_region_stats_kernel(int32_t* __restrict__ L, const int32_t* __restrict__ rid,
                                                                const uint8_t* __restrict__ seg, const uint8_t* __restrict__ img,
                                                                int H, int W, int img_w, int C, int ch0, int cap,
                                                                u64* __restrict__ acc, int32_t* __restrict__ bb,
                                                                int32_t* __restrict__ misc) {
    iseg_region_stats_tile(IsegStatView{L, rid, seg, img, H, W, W, img_w, C, ch0, 0, 0, cap, misc + 1}, acc, bb);
}

// ---- a group of images (ecseg_interseg_batch; planning in iseg_batch.h) ----------------------------------------------------
// mask (n, Hm, Wm): image blockIdx.y's segmentation in the top left corner, background right of it and below
__global__ __launch_bounds__(256) void iseg_pad_masks_kernel(const uint8_t* __restrict__ packed, const IsegImage* __restrict__ tab,
                                                             int Hm, int Wm, uint8_t* __restrict__ mask) {
    const IsegImage t = tab[blockIdx.y];
    const unsigned px = (unsigned)Hm * (unsigned)Wm;         // < 2^31
    const uint8_t* seg = packed + t.seg_off;
    uint8_t* out = mask + (size_t)blockIdx.y * px;
    for (unsigned p = blockIdx.x * 256u + threadIdx.x; p < px; p += gridDim.x * 256u) {
        const unsigned y = p / (unsigned)Wm, x = p - y * (unsigned)Wm;
        out[p] = (y < (unsigned)t.h && x < (unsigned)t.w) ? seg[(size_t)y * t.w + x] : (uint8_t)0;
    }
}

struct LoadRootFlagBatch {                       // LoadRootFlag over images of px pixels each (labels count inside their image)
    const int32_t* L; unsigned px;
    __device__ int operator()(size_t i) const { return L[i] == (int)((unsigned)i % px) + 1; }
};

// plan (n, ISEG_PLAN): the scan value at the image's first pixel, its regions, and the first of its records among the cap the caller
// has room for, handed out in image order by iseg_take (-1: they do not fit; the image then accumulates nothing).  misc[0]: all
// roots (from the scan); misc[3]: the records taken.
__global__ void iseg_batch_plan_kernel(const int32_t* __restrict__ rid, int32_t* __restrict__ misc, int n, int px, int cap,
                                       int32_t* __restrict__ plan) {
    if (blockIdx.x || threadIdx.x) return;
    int used = 0;
    for (int i = 0; i < n; ++i) {
        const int base = rid[(size_t)i * px], next = i + 1 < n ? rid[(size_t)(i + 1) * px] : misc[0];
        int32_t* p = plan + (size_t)i * ISEG_PLAN;
        p[0] = base; p[1] = next - base; p[2] = iseg_take(next - base, &used, cap); p[3] = 0;
    }
    misc[3] = used;
}

// blockIdx.y = image, blockIdx.x = a tile of the largest image (a smaller image's surplus tiles find no row).  imisc (n, 4): [1] / [2]
// the image's value range, as misc[1] / misc[2] of the kernel above.
__global__ __launch_bounds__(256) void iseg_region_stats_batch_kernel(int32_t* __restrict__ L, const int32_t* __restrict__ rid,
                                                                      const uint8_t* __restrict__ mask, const uint8_t* __restrict__ packed,
                                                                      const IsegImage* __restrict__ tab, const int32_t* __restrict__ plan,
                                                                      int px, int Wm, int ch0, u64* __restrict__ acc,
                                                                      int32_t* __restrict__ bb, int32_t* __restrict__ imisc) {
    const int im = blockIdx.y;
    const IsegImage t = tab[im];
    const int32_t* pl = plan + (size_t)im * ISEG_PLAN;
    const size_t o = (size_t)im * (size_t)px;
    const bool room = pl[2] >= 0;
    iseg_region_stats_tile(IsegStatView{L + o, rid + o, mask + o, packed + t.img_off, t.h, t.w, Wm, t.W, t.C, ch0, pl[0], room ? pl[2] : 0,
                                        room ? pl[1] : 0, imisc + (size_t)im * 4 + 1}, acc, bb);
}

// rec (n, 8) int64: area, min row, min col, max row + 1, max col + 1, sum of rows, sum of columns, sum of channel 0
__global__ __launch_bounds__(256) void iseg_finalize_kernel(const u64* __restrict__ acc, const int32_t* __restrict__ bb,
                                                            const int32_t* __restrict__ misc, int cap, int64_t* __restrict__ rec) {
    const int r = blockIdx.x * 256 + threadIdx.x;
    if (r >= cap || r >= misc[0]) return;
    const u64* a = acc + (size_t)r * 4;
    const int32_t* b = bb + (size_t)r * 4;
    int64_t* o = rec + (size_t)r * 8;
    o[0] = (int64_t)a[0]; o[1] = b[0]; o[2] = b[1]; o[3] = 1 - (int64_t)b[2]; o[4] = 1 - (int64_t)b[3];
    o[5] = (int64_t)a[1]; o[6] = (int64_t)a[2]; o[7] = (int64_t)a[3];
}

hipError_t run_nuclei_regions(const uint8_t* seg, const uint8_t* img, int H, int W, int img_w, int C, int ch0, int32_t* labels,
                              const RegionBufs& b, hipStream_t s) {
    const int px = H * W;
    hipError_t e;
    if ((e = hipMemsetAsync(b.misc, 0, 4 * sizeof(int32_t), s)) != hipSuccess) return e;
    if (b.cap > 0 && (e = hipMemsetAsync(b.acc, 0, (size_t)b.cap * 4 * sizeof(u64), s)) != hipSuccess) return e;
    if (b.cap > 0 && (e = hipMemsetAsync(b.bb, 0x7f, (size_t)b.cap * 4 * sizeof(int32_t), s)) != hipSuccess) return e;
    exclusive_scan(LoadRootFlag{labels}, px, b.blk, b.rid, b.misc, s);   // rid[root pixel] = region index, misc[0] = regions
    hipLaunchKernelGGL(iseg_region_stats_kernel, dim3(stat_tiles(H, W)), dim3(256), 0, s, labels, b.rid, seg, img, H, W, img_w, C, ch0, b.cap, b.acc,
                       b.bb, b.misc);
    if (b.cap > 0)
        hipLaunchKernelGGL(iseg_finalize_kernel, dim3((b.cap + 255) / 256), dim3(256), 0, s, b.acc, b.bb, b.misc, b.cap, b.rec);
    return hipGetLastError();
}

__device__ __forceinline__ int iseg_reflect(int c, int n) {   // c in [-1, n]
    if (n == 1) return 0;
    return c < 0 ? -c : (c >= n ? 2 * (n - 1) - c : c);
}

// 16 output rows (block rb) of crop n, thread = output column: the window (y0, x0, h, w) of the image whose label map L has row
// stride ls; out (n, 256, 256, 3); chmax (n, 3) preset to 0
__device__ __forceinline__ void iseg_crop_rows(const int32_t* __restrict__ L, const uint8_t* __restrict__ img, int ls, int img_w, int C,
                                               int label, int y0, int x0, int h, int w, int c0, int c1, int c2, int n, int rb,
                                               uint8_t* __restrict__ out, int32_t* __restrict__ chmax) {
    const int j = threadIdx.x;
    const int cq = w * (2 * j + 1) - 256;                    // sample column * 512, > -512
    const int ca = (cq + 512) / 512 - 1, fc = cq - ca * 512;
    const int xa = x0 + iseg_reflect(ca, w), xb = x0 + iseg_reflect(ca + 1, w);
    int m0 = 0, m1 = 0, m2 = 0;
    for (int ii = 0; ii < ISEG_CROP_ROWS; ++ii) {
        const int i = rb * ISEG_CROP_ROWS + ii;
        const int rq = h * (2 * i + 1) - 256;
        const int ra = (rq + 512) / 512 - 1, fr = rq - ra * 512;
        const int ya = y0 + iseg_reflect(ra, h), yb = y0 + iseg_reflect(ra + 1, h);
        const int ys[2] = {ya, yb}, xs[2] = {xa, xb};
        const int wy[2] = {512 - fr, fr}, wx[2] = {512 - fc, fc};
        int v0 = 0, v1 = 0, v2 = 0;
#pragma unroll
        for (int a = 0; a < 2; ++a) {
#pragma unroll
            for (int b = 0; b < 2; ++b) {
                const size_t p = (size_t)ys[a] * ls + xs[b];
                if (L[p] != label) continue;
                const uint8_t* q = img + ((size_t)ys[a] * img_w + xs[b]) * C;
                const int wgt = wy[a] * wx[b];
                v0 += wgt * q[c0]; v1 += wgt * q[c1]; v2 += wgt * q[c2];
            }
        }
        v0 >>= 18; v1 >>= 18; v2 >>= 18;
        uint8_t* o = out + (((size_t)n * 256 + i) * 256 + j) * 3;
        o[0] = (uint8_t)v0; o[1] = (uint8_t)v1; o[2] = (uint8_t)v2;
        m0 = max(m0, v0); m1 = max(m1, v1); m2 = max(m2, v2);
    }
#pragma unroll
    for (int dd = 32; dd >= 1; dd >>= 1) {
        m0 = max(m0, __shfl_xor(m0, dd)); m1 = max(m1, __shfl_xor(m1, dd)); m2 = max(m2, __shfl_xor(m2, dd));
    }
    if ((j & 63) == 0) {
        if (m0) atomicMax(chmax + (size_t)n * 3 + 0, m0);
        if (m1) atomicMax(chmax + (size_t)n * 3 + 1, m1);
        if (m2) atomicMax(chmax + (size_t)n * 3 + 2, m2);
    }
}

// one block = 16 output rows of one crop of the image on the handle; desc (n, 5): region, y0, x0, h, w
__global__ __launch_bounds__(256) void iseg_crops_kernel(const int32_t* __restrict__ L, const uint8_t* __restrict__ img, int W,
                                                         int img_w, int C, const int32_t* __restrict__ desc, int c0, int c1, int c2,
                                                         uint8_t* __restrict__ out, int32_t* __restrict__ chmax) {
    const int n = blockIdx.x / (256 / ISEG_CROP_ROWS), rb = blockIdx.x % (256 / ISEG_CROP_ROWS);
    const int32_t* d = desc + (size_t)n * 5;
    iseg_crop_rows(L, img, W, img_w, C, d[0] + 1, d[1], d[2], d[3], d[4], c0, c1, c2, n, rb, out, chmax);
}

// the same for a crop of any image of a group; desc (n, ISEG_DESC): image, region, y0, x0, h, w - that image's raster with its own
// strides, and its plane of the padded label maps
__global__ __launch_bounds__(256) void iseg_crops_batch_kernel(const int32_t* __restrict__ L, const uint8_t* __restrict__ packed,
                                                               const IsegImage* __restrict__ tab, int px, int Wm,
                                                               const int32_t* __restrict__ desc, int c0, int c1, int c2,
                                                               uint8_t* __restrict__ out, int32_t* __restrict__ chmax) {
    const int n = blockIdx.x / (256 / ISEG_CROP_ROWS), rb = blockIdx.x % (256 / ISEG_CROP_ROWS);
    const int32_t* d = desc + (size_t)n * ISEG_DESC;
    const IsegImage t = tab[d[0]];
    iseg_crop_rows(L + (size_t)d[0] * (size_t)px, packed + t.img_off, Wm, t.W, t.C, d[1] + 1, d[2], d[3], d[4], d[5], c0, c1, c2, n, rb, out, chmax);
}

hipError_t run_nucleus_crops(const int32_t* labels, const uint8_t* img, int W, int img_w, int C, const int32_t* desc, int n,
                             const int order[3], uint8_t* out, int32_t* chmax, hipStream_t s) {
    if (n <= 0) return hipSuccess;
    hipError_t e = hipMemsetAsync(chmax, 0, (size_t)n * 3 * sizeof(int32_t), s);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(iseg_crops_kernel, dim3((unsigned)n * (256 / ISEG_CROP_ROWS)), dim3(256), 0, s, labels, img, W, img_w, C, desc,
                       order[0], order[1], order[2], out, chmax);
    return hipGetLastError();
}

hipError_t run_pad_label_masks(const uint8_t* packed, const IsegImage* tab, int n, int Hm, int Wm, uint8_t* mask, int32_t* lab, PostWorkspace& ws,
                               hipStream_t s) {
    const unsigned pad_x = (unsigned)std::min<size_t>(((size_t)Hm * Wm + 255) / 256, 4096);
    hipLaunchKernelGGL(iseg_pad_masks_kernel, dim3(pad_x, (unsigned)n), dim3(256), 0, s, packed, tab, Hm, Wm, mask);
    return run_ccl_labels(ws, mask, n, Hm, Wm, 8, lab, s);
}

hipError_t run_iseg_batch_regions(int n, int Hm, int Wm, int ch0, const IsegBatchBufs& b, PostWorkspace& ws, hipStream_t s) {
    const int px = Hm * Wm;                                  // n * px < 2^31 (iseg_batch_groups)
    hipError_t e;
    if ((e = hipMemsetAsync(b.misc, 0, 4 * sizeof(int32_t), s)) != hipSuccess) return e;
    if ((e = hipMemsetAsync(b.imisc, 0, (size_t)n * 4 * sizeof(int32_t), s)) != hipSuccess) return e;
    if (b.cap > 0 && (e = hipMemsetAsync(b.acc, 0, (size_t)b.cap * 4 * sizeof(u64), s)) != hipSuccess) return e;
    if (b.cap > 0 && (e = hipMemsetAsync(b.bb, 0x7f, (size_t)b.cap * 4 * sizeof(int32_t), s)) != hipSuccess) return e;
    if ((e = run_pad_label_masks(b.packed, b.tab, n, Hm, Wm, b.mask, b.lab, ws, s)) != hipSuccess) return e;
    exclusive_scan(LoadRootFlagBatch{b.lab, (unsigned)px}, n * px, b.blk, b.rid, b.misc, s);
    hipLaunchKernelGGL(iseg_batch_plan_kernel, dim3(1), dim3(64), 0, s, b.rid, b.misc, n, px, b.cap, b.plan);
    hipLaunchKernelGGL(iseg_region_stats_batch_kernel, dim3(stat_tiles(Hm, Wm), (unsigned)n), dim3(256), 0, s, b.lab, b.rid, b.mask, b.packed,
                       b.tab, b.plan, px, Wm, ch0, b.acc, b.bb, b.imisc);
    if (b.cap > 0)
        hipLaunchKernelGGL(iseg_finalize_kernel, dim3((b.cap + 255) / 256), dim3(256), 0, s, b.acc, b.bb, b.misc + 3, b.cap, b.rec);
    return hipGetLastError();
}

hipError_t run_iseg_batch_crops(int Hm, int Wm, const IsegBatchBufs& b, int n, const int order[3], hipStream_t s) {
    if (n <= 0) return hipSuccess;
    hipError_t e = hipMemsetAsync(b.cls.crop.max, 0, (size_t)n * 3 * sizeof(int32_t), s);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(iseg_crops_batch_kernel, dim3((unsigned)n * (256 / ISEG_CROP_ROWS)), dim3(256), 0, s, b.lab, b.packed, b.tab, Hm * Wm, Wm,
                       b.desc, order[0], order[1], order[2], b.cls.crop.crops, b.cls.crop.max);
    return hipGetLastError();
}

}  // namespace ecseg
