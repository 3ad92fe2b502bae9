// stat_fish behind nuclei_segment on gfx950 (reference src/stat_fish.py:73-107,134-142,226-300): per nucleus of an instance-label map
// the FISH spot statistics of up to three probe channels, the cleaned spot masks and the boundary drawing.  Every integer field
// is a sum, a maximum, an OR or a root count, so no result depends on the order of the atomics; the one float64 decision
// (coefficient > normal_threshold) is evaluated in a fixed tap order, so two calls give identical bytes.
//
// Cells (regionprops(labeled_segmented_cells): every label > 0 that occurs, ascending)
//   * run_dense_cells (fishdist_kernels.hip: mark + exclusive scan) gives rid[label - 1] = dense cell index, misc[0] = cells;
//   * fs_cell_stats_kernel relabels the map in place to the dense rank cell + 1 and accumulates per cell the area, the sums of
//     rows and columns and, per probe, sum / count / maximum of the non-zero raw pixels (:252,261-263), on cell_util.h's
//     statistics tile: the lanes of one cell (wave_key_groups) are reduced with shuffles and the leader lane adds into the
//     cell's 64-bit accumulators, one atomic per (cell, field, row segment).
// Peak filter (get_thresholded, :73-88)
//   * fs_channel_max_kernel: the maximum of every probe channel over the whole image (the "max brightness" centres of :82);
//   * fs_threshold_kernel: a 64 x 16 pixel tile per workgroup; per probe the channel's zero-padded halo tile (uint8) and the K x K
//     float64 weights sit in LDS; a pixel that passes "label > 0 and pixel > intensity threshold" sums weight * pixel over all
//     K * K taps in float64, row-major tap order (padding taps are multiplied too: 0 * NaN = NaN as in the reference's
//     convolution, so NaN weights give no normal centre).  thresholded = centre ? 255 : 0; the union-find parent of the probe
//     is preset to the pixel itself on thresholded pixels and to -1 elsewhere.
// Spots (count_blobs, :134-142: scipy.ndimage.label, 4-connected, of thresholded * cell)
//   * fs_unite_kernel unites a thresholded pixel with the thresholded pixels of the SAME cell behind it (uf_unite_back,
//     4-connected);
//   * uf_size_kernel (cell_util.h) flattens (parent = root) and counts the pixels of every root; fs_finalize_kernel clears the components
//     below min_cc_size from `thresholded` (:140 clears through a view, so the cleaned mask is what the _lsq file shows) and
//     counts pixels and roots of the rest per cell;
//   * the pair of the first two probes (:270-275): fs_pair_init_kernel presets parents on the AND of the two CLEANED masks, then
//     the same unite / size / finalize, which here only counts.
// Boundaries (get_boundaries, :91-107) on the dense ranks: fs_boundary_kernel, 64-bit sums of the 2 t taps of either axis.
// fs_records_kernel writes the ECSEG_FISH_SPOT_INT64 fields of every cell.
//
// The three colour files (ecseg_fish_render, :110-115,295-300): fs_render_kernel composes _original, _original_with_segmentation
// and _lsq_ in one elementwise pass, four pixels per thread: the image, the masks and the boundaries are read once as dwords, the
// three (H, W, 3) RGB rasters leave as three dwords each.  All of it is integer arithmetic on bytes held in registers.
#include "common.h"
#include "cell_util.h"

namespace ecseg {

static constexpr int FS_TW = 64, FS_TH = 16;                 // output tile of fs_threshold_kernel (256 threads x 4 rows)
static constexpr int FS_KMAX = ECSEG_FISH_SPOT_MAX_KERNEL;
static constexpr int FS_HALO_W = FS_TW + FS_KMAX - 1, FS_HALO_H = FS_TH + FS_KMAX - 1;
static constexpr int FS_SLOTS = 4;                           // union-find slots: probes 0..2, the pair

struct FsChannels { int c[3]; };
struct FsThresholds { double t[3]; };

// Every stage is stated once, as a __device__ function of the thread's index over ONE image's buffers (the block index is
// blockIdx.x in both forms).  The fs_* kernels run it on the image of ecseg_fish_spots; the fsb_* kernels (further down) run it on
// image blockIdx.y of a chunk, whose buffers they find through the FsImage table (fish_batch.h).

// mx[j] = max over the image of channel ch.c[j]
__device__ __forceinline__ void fs_channel_max_body(const uint8_t* __restrict__ img, int px, int C, int np, const FsChannels& ch,
                                                    int32_t* __restrict__ mx) {
    int m[3] = {0, 0, 0};
    for (unsigned p = blockIdx.x * 256u + threadIdx.x; p < (unsigned)px; p += gridDim.x * 256u) {
        const uint8_t* q = img + (size_t)p * C;
#pragma unroll
        for (int j = 0; j < 3; ++j)
            if (j < np) m[j] = max(m[j], (int)q[ch.c[j]]);
    }
#pragma unroll
    for (int j = 0; j < 3; ++j) {
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) m[j] = max(m[j], __shfl_xor(m[j], d));
        if ((threadIdx.x & 63) == 0 && j < np && m[j] > 0) atomicMax(mx + j, m[j]);
    }
}
__global__ __launch_bounds__(256) void fs_channel_max_kernel(const uint8_t* __restrict__ img, int px, int C, int np, FsChannels ch,
                                                             int32_t* __restrict__ mx) {
    fs_channel_max_body(img, px, C, np, ch, mx);
}

// acc: per cell 12 uint64: area, sum of rows, sum of columns, then per probe sum / count / maximum of the non-zero raw pixels.
// val[cell] = the cell's label value.  L is relabelled in place to cell + 1.  rid gives cell0 + cell (cell0: the cells of the images
// in front, 0 for an image alone); acc and val are indexed by that sum.
__device__ __forceinline__ void fs_cell_stats_body(int32_t* __restrict__ L, const int32_t* __restrict__ rid, const uint8_t* __restrict__ img,
                                                   int H, int W, int C, int np, const FsChannels& ch, int cell0, u64* __restrict__ acc,
                                                   int32_t* __restrict__ val) {
    const int lane = threadIdx.x & 63;
    const StatTile tile = stat_tile(W);
    for (int r = 0; r < CELL_ROWS_PER_WAVE; ++r) {
        const int y = tile.ybeg + r;
        if (y >= H) break;                                   // wave-uniform
        int reg = -1, l = 0;
        int raw[3] = {0, 0, 0};
        if (tile.x < (unsigned)W) {
            const size_t p = (size_t)y * W + tile.x;
            l = L[p];
            if (l > 0) {
                reg = rid[l - 1];
                L[p] = reg - cell0 + 1;
                const uint8_t* q = img + p * C;
#pragma unroll
                for (int j = 0; j < 3; ++j)
                    if (j < np) raw[j] = q[ch.c[j]];
            } else if (l < 0) {
                L[p] = 0;                                    // background: the later kernels test > 0 / compare ranks
            }
        }
        wave_key_groups(reg, [&](int key, bool mine, u64 m, int leader) {
            const unsigned n = (unsigned)__popcll(m);
            int sl = mine ? lane : 0;                        // sum of the lane numbers: columns = n * xb + that
            int s[3], mxv[3];
            unsigned cnt[3];
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                s[j] = mine ? raw[j] : 0;
                mxv[j] = s[j];
                cnt[j] = (unsigned)__popcll(__ballot(mine && raw[j] != 0));
            }
#pragma unroll
            for (int d = 32; d >= 1; d >>= 1) {
                sl += __shfl_xor(sl, d);
#pragma unroll
                for (int j = 0; j < 3; ++j) {
                    s[j] += __shfl_xor(s[j], d);
                    mxv[j] = max(mxv[j], __shfl_xor(mxv[j], d));
                }
            }
            if (lane != leader) return;
            u64* a = acc + (size_t)key * 12;
            atomicAdd(a + 0, (u64)n);
            atomicAdd(a + 1, (u64)n * (u64)y);
            atomicAdd(a + 2, (u64)n * (u64)tile.xb + (u64)sl);
#pragma unroll
            for (int j = 0; j < 3; ++j)
                if (j < np && cnt[j]) {
                    atomicAdd(a + 3 + 3 * j, (u64)s[j]);
                    atomicAdd(a + 4 + 3 * j, (u64)cnt[j]);
                    atomicMax(a + 5 + 3 * j, (u64)mxv[j]);
                }
            val[key] = l;                                    // every writer of a cell stores the same label
        });
    }
}
__global__ __launch_bounds__(256) void fs_cell_stats_kernel(int32_t* __restrict__ L, const int32_t* __restrict__ rid,
                                                            const uint8_t* __restrict__ img, int H, int W, int C, int np, FsChannels ch,
                                                            u64* __restrict__ acc, int32_t* __restrict__ val) {
    fs_cell_stats_body(L, rid, img, H, W, C, np, ch, 0, acc, val);
}

// L: cell + 1 per pixel (0 background).  thr (H, W, np) uint8 0 / 255; par: np planes of H * W parents (pixel | -1).  The LDS
// (FS_KMAX * FS_KMAX weights and the FS_HALO_H x FS_HALO_W halo tile) is sized for the largest K, whatever this image's is.
// A tile below the image (a chunk's grid is the largest image's) returns before the first barrier, the whole workgroup together.
__device__ __forceinline__ void fs_threshold_body(const int32_t* __restrict__ L, const uint8_t* __restrict__ img, int H, int W, int C, int np,
                                                  const FsChannels& ch, const double* __restrict__ wts, int K, double normal_thr,
                                                  const FsThresholds& ithr, const int32_t* __restrict__ mx, uint8_t* __restrict__ thr,
                                                  int32_t* __restrict__ par) {
    __shared__ double s_w[FS_KMAX * FS_KMAX];
    __shared__ uint8_t s_t[FS_HALO_H * FS_HALO_W];
    const int t = threadIdx.x, lx = t & 63, ly = t >> 6;
    const int r = K >> 1, hw = FS_TW + K - 1, hh = FS_TH + K - 1;
    const unsigned tiles_x = ((unsigned)W + FS_TW - 1) / FS_TW;
    const int x0 = (int)(blockIdx.x % tiles_x) * FS_TW, y0 = (int)(blockIdx.x / tiles_x) * FS_TH;
    if (y0 >= H) return;
    for (int i = t; i < K * K; i += 256) s_w[i] = wts[i];
    const size_t px = (size_t)H * W;
    for (int j = 0; j < np; ++j) {
        const int c = ch.c[j];
        __syncthreads();                                     // the previous probe's readers are done (and s_w is complete)
        for (int i = t; i < hh * hw; i += 256) {
            const int ty = i / hw, tx = i - ty * hw;
            const int gy = y0 - r + ty, gx = x0 - r + tx;
            s_t[ty * FS_HALO_W + tx] = (gy >= 0 && gy < H && gx >= 0 && gx < W) ? img[((size_t)gy * W + gx) * C + c] : (uint8_t)0;
        }
        __syncthreads();
        const int cmax = mx[j];
        const double it = ithr.t[j];
#pragma unroll
        for (int q = 0; q < FS_TH / 4; ++q) {
            const int oy = ly + 4 * q, y = y0 + oy, x = x0 + lx;
            if (y >= H || x >= W) continue;
            const size_t p = (size_t)y * W + x;
            const int v = s_t[(oy + r) * FS_HALO_W + lx + r];
            bool on = false;
            if (L[p] > 0 && (double)v > it) {
                on = cmax != 0 && v == cmax;                 // :82
                if (!on) {
                    double sum = 0.0;
                    for (int ky = 0; ky < K; ++ky) {
                        const uint8_t* row = s_t + (oy + ky) * FS_HALO_W + lx;
                        const double* wr = s_w + ky * K;
                        for (int kx = 0; kx < K; ++kx) sum += wr[kx] * (double)row[kx];
                    }
                    on = sum > normal_thr;                   // :83 (NaN: false)
                }
            }
            thr[p * np + j] = on ? 255 : 0;
            par[(size_t)j * px + p] = on ? (int)p : -1;
        }
    }
}
__global__ __launch_bounds__(256) void fs_threshold_kernel(const int32_t* __restrict__ L, const uint8_t* __restrict__ img, int H, int W, int C,
                                                           int np, FsChannels ch, const double* __restrict__ wts, int K, double normal_thr,
                                                           FsThresholds ithr, const int32_t* __restrict__ mx, uint8_t* __restrict__ thr,
                                                           int32_t* __restrict__ par) {
    fs_threshold_body(L, img, H, W, C, np, ch, wts, K, normal_thr, ithr, mx, thr, par);
}

// one plane of parents: unite every mask pixel with its W / N neighbour when that is a mask pixel of the same cell
__device__ __forceinline__ void fs_unite_body(const int32_t* __restrict__ L, int H, int W, int32_t* par) {
    const unsigned pu = blockIdx.x * 256u + threadIdx.x;    // H * W < 2^31: no wrap
    if (pu >= (unsigned)(H * W)) return;
    const int p = (int)pu;
    if (uf_load(par, p) < 0) return;
    const int cell = L[p];
    const int y = p / W, x = p - y * W;
    uf_unite_back(par, p, y, x, W, 0, [&](int q) { return L[q] == cell; });
}
// slot blockIdx.y
__global__ __launch_bounds__(256) void fs_unite_kernel(const int32_t* __restrict__ L, int H, int W, int32_t* par_all) {
    fs_unite_body(L, H, W, par_all + (size_t)blockIdx.y * ((size_t)H * W));
}

// One slot.  Components below min_cc: cleared from thr when thr != null (probes), else just not counted (the pair).
// cnt: per cell FS_SLOTS x (pixels, components) uint32.
__device__ __forceinline__ void fs_finalize_body(const int32_t* __restrict__ L, int px, int np, int slot, int min_cc,
                                                 const int32_t* __restrict__ par_all, const int32_t* __restrict__ sz_all,
                                                 uint8_t* __restrict__ thr, unsigned* __restrict__ cnt) {
    const unsigned pu = blockIdx.x * 256u + threadIdx.x;
    if (pu >= (unsigned)px) return;
    const int p = (int)pu;
    const int32_t* par = par_all + (size_t)slot * (size_t)px;
    const int q = par[p];
    if (q < 0) return;
    const int root = uf_find(par, q);
    if (sz_all[(size_t)slot * (size_t)px + root] < min_cc) {
        if (thr) thr[(size_t)p * np + slot] = 0;
        return;
    }
    unsigned* c = cnt + ((size_t)(L[p] - 1) * FS_SLOTS + slot) * 2;
    atomicAdd(c, 1u);
    if (root == p) atomicAdd(c + 1, 1u);
}
// slot = slot0 + blockIdx.y
__global__ __launch_bounds__(256) void fs_finalize_kernel(const int32_t* __restrict__ L, int px, int np, int slot0, int min_cc,
                                                          const int32_t* __restrict__ par_all, const int32_t* __restrict__ sz_all,
                                                          uint8_t* __restrict__ thr, unsigned* __restrict__ cnt) {
    fs_finalize_body(L, px, np, slot0 + (int)blockIdx.y, min_cc, par_all, sz_all, thr, cnt);
}

// parents of the pair slot: the pixel itself where the cleaned masks of probes 0 and 1 are both set
__device__ __forceinline__ void fs_pair_init_body(const uint8_t* __restrict__ thr, int px, int np, int32_t* __restrict__ par) {
    const unsigned p = blockIdx.x * 256u + threadIdx.x;
    if (p >= (unsigned)px) return;
    const uint8_t* q = thr + (size_t)p * np;
    par[p] = (q[0] && q[1]) ? (int)p : -1;
}
__global__ __launch_bounds__(256) void fs_pair_init_kernel(const uint8_t* __restrict__ thr, int px, int np, int32_t* __restrict__ par) {
    fs_pair_init_body(thr, px, np, par);
}

// b = 255 where sum L[y][x-t+1..x] != sum L[y][x+1..x+t] or the same along y (taps outside the image are 0): the "SAME" padding
// of an even kernel, t - 1 before and t after.  Ranks are < 2^31 and t <= 16; the sums are 64-bit.
__device__ __forceinline__ void fs_boundary_body(const int32_t* __restrict__ L, int H, int W, int t, uint8_t* __restrict__ out) {
    const unsigned pu = blockIdx.x * 256u + threadIdx.x;
    if (pu >= (unsigned)(H * W)) return;
    const int p = (int)pu, y = p / W, x = p - y * W;
    long long h = 0, v = 0;
    for (int k = 0; k < t; ++k) {
        if (x - k >= 0) h += L[p - k];
        if (x + 1 + k < W) h -= L[p + 1 + k];
        if (y - k >= 0) v += L[(size_t)(y - k) * W + x];
        if (y + 1 + k < H) v -= L[(size_t)(y + 1 + k) * W + x];
    }
    out[p] = (h != 0 || v != 0) ? 255 : 0;
}
__global__ __launch_bounds__(256) void fs_boundary_kernel(const int32_t* __restrict__ L, int H, int W, int t, uint8_t* __restrict__ out) {
    fs_boundary_body(L, H, W, t, out);
}

// rec (n, ECSEG_FISH_SPOT_INT64) int64: see ecseg_fish_spots
__device__ __forceinline__ void fs_records_body(const u64* __restrict__ acc, const unsigned* __restrict__ cnt, const int32_t* __restrict__ val,
                                                int n, int np, int64_t* __restrict__ rec) {
    const unsigned cell = blockIdx.x * 256u + threadIdx.x;
    if (cell >= (unsigned)n) return;
    const u64* a = acc + (size_t)cell * 12;
    const unsigned* c = cnt + (size_t)cell * FS_SLOTS * 2;
    int64_t* o = rec + (size_t)cell * ECSEG_FISH_SPOT_INT64;
    o[0] = val[cell]; o[1] = (int64_t)a[0]; o[2] = (int64_t)a[1]; o[3] = (int64_t)a[2];
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        const bool live = j < np;
        o[4 + 5 * j] = live ? c[2 * j] : 0;
        o[5 + 5 * j] = live ? c[2 * j + 1] : 0;
        o[6 + 5 * j] = live ? (int64_t)a[3 + 3 * j] : 0;
        o[7 + 5 * j] = live ? (int64_t)a[4 + 3 * j] : 0;
        o[8 + 5 * j] = live ? (int64_t)a[5 + 3 * j] : 0;
    }
    o[19] = np >= 2 ? c[6] : 0;
    o[20] = np >= 2 ? c[7] : 0;
    o[21] = o[22] = o[23] = 0;
}
__global__ __launch_bounds__(256) void fs_records_kernel(const u64* __restrict__ acc, const unsigned* __restrict__ cnt,
                                                         const int32_t* __restrict__ val, int n, int np, int64_t* __restrict__ rec) {
    fs_records_body(acc, cnt, val, n, np, rec);
}

// ---- a chunk of images (ecseg_stat_fish_batch; layout in fish_batch.h) ---------------------------------------------------------
// blockIdx.y = the image, blockIdx.x = a block of the largest image's grid: a block past its image's extent returns at once (every
// body above begins with that test).  Where a stage runs per union-find slot, blockIdx.z is the slot.  Everything an image owns is
// found through its row: pointers move, the values (parents, labels, ranks) stay indices inside the image.
struct FsbView {
    uint8_t* work; FsImage* tab; int32_t* lab; int32_t* rid; int32_t* par; int32_t* sz; int32_t* mx; const double* w;
    u64* acc; unsigned* cnt; int32_t* val; int64_t* rec;
};
__device__ __forceinline__ FsChannels fsb_probes(const FsImage& t) { return FsChannels{{t.ch[1], t.ch[2], t.ch[3]}}; }

// the labels of the padded planes into the packed label maps: 1 + the raster index of the first pixel, counted in the image's own
// width as ecseg_ccl_labels counts it
__global__ __launch_bounds__(256) void fsb_unpad_kernel(FsbView v, const int32_t* __restrict__ plab, int Wm) {
    const FsImage& t = v.tab[blockIdx.y];
    const unsigned p = blockIdx.x * 256u + threadIdx.x;
    if (t.pad < 0 || p >= (unsigned)(t.H * t.W)) return;
    const int y = (int)(p / (unsigned)t.W), x = (int)p - y * t.W;
    int l = plab[(size_t)t.pad + (size_t)y * Wm + x];
    if (l > 0) { const int r = l - 1, ry = r / Wm; l = 1 + ry * t.W + (r - ry * Wm); }
    v.lab[(size_t)t.lab + p] = l;
}
// plan (n + 1, 2): [i][1] = 1 when image i holds a label above its pixel count
__global__ __launch_bounds__(256) void fsb_mark_kernel(FsbView v, int32_t* __restrict__ plan) {
    const FsImage& t = v.tab[blockIdx.y];
    cell_mark_pixel(v.lab + t.lab, t.H * t.W, v.rid + t.lab, plan + 2 * (size_t)blockIdx.y + 1, blockIdx.x * 256u + threadIdx.x);
}
// After the scan over the whole rid: rid[row.lab] is the number of cells in front of image i, the next image's (or the total) ends it.
__global__ __launch_bounds__(256) void fsb_plan_kernel(FsbView v, int n, const int32_t* __restrict__ total, int32_t* __restrict__ plan) {
    const int i = (int)(blockIdx.x * 256u + threadIdx.x);
    if (i > n) return;
    if (i == n) { plan[2 * (size_t)n] = *total; plan[2 * (size_t)n + 1] = 0; return; }
    const int base = v.rid[v.tab[i].lab], next = i + 1 < n ? v.rid[v.tab[i + 1].lab] : *total;
    v.tab[i].rec0 = base; v.tab[i].n_cells = next - base;
    plan[2 * (size_t)i] = next - base;
}
__global__ __launch_bounds__(256) void fsb_channel_max_kernel(FsbView v) {
    const FsImage& t = v.tab[blockIdx.y];
    fs_channel_max_body(v.work + t.img, t.H * t.W, t.C, t.np, fsb_probes(t), v.mx + 4 * (size_t)blockIdx.y);
}
__global__ __launch_bounds__(256) void fsb_cell_stats_kernel(FsbView v) {
    const FsImage& t = v.tab[blockIdx.y];
    fs_cell_stats_body(v.lab + t.lab, v.rid + t.lab, v.work + t.img, t.H, t.W, t.C, t.np, fsb_probes(t), t.rec0, v.acc, v.val);
}
__global__ __launch_bounds__(256) void fsb_threshold_kernel(FsbView v) {
    const FsImage& t = v.tab[blockIdx.y];
    fs_threshold_body(v.lab + t.lab, v.work + t.img, t.H, t.W, t.C, t.np, fsb_probes(t), v.w + t.w, t.K, t.normal_thr,
                      FsThresholds{{t.ithr[0], t.ithr[1], t.ithr[2]}}, v.mx + 4 * (size_t)blockIdx.y, v.work + t.thr, v.par + 4 * t.lab);
}
// slot = slot0 + blockIdx.z while it is a probe of the image (slot0 = FS_SLOTS - 1: the pair, for images of two probes or more)
__device__ __forceinline__ bool fsb_slot_live(const FsImage& t, int slot) { return slot == FS_SLOTS - 1 ? t.np >= 2 : slot < t.np; }
__global__ __launch_bounds__(256) void fsb_unite_kernel(FsbView v, int slot0) {
    const FsImage& t = v.tab[blockIdx.y];
    const int slot = slot0 + (int)blockIdx.z;
    if (!fsb_slot_live(t, slot)) return;
    fs_unite_body(v.lab + t.lab, t.H, t.W, v.par + 4 * t.lab + (size_t)slot * ((size_t)t.H * t.W));
}
__global__ __launch_bounds__(256) void fsb_size_kernel(FsbView v, int slot0) {
    const FsImage& t = v.tab[blockIdx.y];
    const int slot = slot0 + (int)blockIdx.z, px = t.H * t.W;
    if (!fsb_slot_live(t, slot)) return;
    const size_t o = 4 * (size_t)t.lab + (size_t)slot * (size_t)px;
    uf_size_pixel(px, v.par + o, v.sz + o, static_cast<int32_t*>(nullptr), blockIdx.x * 256u + threadIdx.x);
}
__global__ __launch_bounds__(256) void fsb_finalize_kernel(FsbView v, int slot0) {
    const FsImage& t = v.tab[blockIdx.y];
    const int slot = slot0 + (int)blockIdx.z;
    if (!fsb_slot_live(t, slot)) return;
    fs_finalize_body(v.lab + t.lab, t.H * t.W, t.np, slot, t.min_cc, v.par + 4 * t.lab, v.sz + 4 * t.lab,
                     slot == FS_SLOTS - 1 ? static_cast<uint8_t*>(nullptr) : v.work + t.thr, v.cnt + (size_t)t.rec0 * FS_SLOTS * 2);
}
__global__ __launch_bounds__(256) void fsb_pair_init_kernel(FsbView v) {
    const FsImage& t = v.tab[blockIdx.y];
    if (t.np < 2) return;
    fs_pair_init_body(v.work + t.thr, t.H * t.W, t.np, v.par + 4 * t.lab + (size_t)(FS_SLOTS - 1) * ((size_t)t.H * t.W));
}
__global__ __launch_bounds__(256) void fsb_boundary_kernel(FsbView v, int line_t) {
    const FsImage& t = v.tab[blockIdx.y];
    fs_boundary_body(v.lab + t.lab, t.H, t.W, line_t, v.work + t.bnd);
}
__global__ __launch_bounds__(256) void fsb_records_kernel(FsbView v) {
    const FsImage& t = v.tab[blockIdx.y];
    fs_records_body(v.acc + (size_t)t.rec0 * 12, v.cnt + (size_t)t.rec0 * FS_SLOTS * 2, v.val + t.rec0, t.n_cells, t.np,
                    v.rec + (size_t)t.rec0 * ECSEG_FISH_SPOT_INT64);
}

// ---- ecseg_fish_render ---------------------------------------------------------------------------------------------------
struct FsRenderChannels { int blue, green, red, aqua; };
static constexpr unsigned FS_AQUA_B = 54, FS_AQUA_G = 137, FS_AQUA_R = 233;      // aqua_rgb = [233, 137, 54] (:163), per BGR channel

// One pixel.  pix: its C image bytes, channel c in bits 8 c .. 8 c + 7; t: its C - 1 mask bytes likewise; b: its boundary byte.
// -> the three RGB pixels, red in bits 0..7, green in 8..15, blue in 16..23.
//   merge_channels on the uint8 image (:295): coeff * aqua wraps to uint8 before / 255, so a channel gains 1 exactly when
//     (coeff * aqua) & 255 == 255, saturating at 255;
//   img_with_segmentation (:296): on a boundary blue and red become 255 and green (I - 255) as uint8 = (I + 1) & 255;
//   _lsq_ (:297-300): BGR = (boundaries, mask 0, mask 1), each plus coeff * mask 2 / 255 (the quotient's floor: the sum is cut to
//     uint8 after min(., 255)), saturating at 255.
template <int C>
__device__ __forceinline__ void fs_render_pixel(unsigned pix, unsigned t, unsigned b, const FsRenderChannels& ch, unsigned& orig,
                                                unsigned& seg, unsigned& lsq) {
    unsigned vb = (pix >> (8 * ch.blue)) & 255u, vg = (pix >> (8 * ch.green)) & 255u, vr = (pix >> (8 * ch.red)) & 255u;
    unsigned lb = b, lg = t & 255u, lr = (t >> 8) & 255u;
    if (C == 4) {
        const unsigned q = (pix >> (8 * ch.aqua)) & 255u, m = (t >> 16) & 255u;
        vb = min(255u, vb + (((FS_AQUA_B * q) & 255u) == 255u));
        vg = min(255u, vg + (((FS_AQUA_G * q) & 255u) == 255u));
        vr = min(255u, vr + (((FS_AQUA_R * q) & 255u) == 255u));
        lb = min(255u, lb + FS_AQUA_B * m / 255u);
        lg = min(255u, lg + FS_AQUA_G * m / 255u);
        lr = min(255u, lr + FS_AQUA_R * m / 255u);
    }
    orig = vr | (vg << 8) | (vb << 16);
    seg = b ? (255u | (((vg + 1u) & 255u) << 8) | (255u << 16)) : orig;
    lsq = lr | (lg << 8) | (lb << 16);
}

// pixel k (0..3) of four 3-byte pixels packed in three dwords, in bits 0..23
__device__ __forceinline__ unsigned fs_unpack3(const unsigned w[3], int k) {
    return (k == 0 ? w[0] : k == 1 ? (w[0] >> 24) | (w[1] << 8) : k == 2 ? (w[1] >> 16) | (w[2] << 16) : w[2] >> 8) & 0xffffffu;
}
struct alignas(4) FsDword3 { unsigned x, y, z; };
__device__ __forceinline__ FsDword3 fs_pack3(const unsigned p[4]) {
    return FsDword3{p[0] | (p[1] << 24), (p[1] >> 8) | (p[2] << 16), (p[2] >> 16) | (p[3] << 8)};
}

// img (px, C), thr (px, C - 1), bnd (px) -> orig, seg, lsq (px, 3).  Thread g owns pixels 4 g .. 4 g + 3; every array starts on a
// 256-byte boundary, so its group starts on a dword (C = 4: the image on 16 bytes).  The last group, when px % 4 != 0, goes byte by byte.
template <int C>
__global__ __launch_bounds__(256) void fs_render_kernel(const uint8_t* __restrict__ img, const uint8_t* __restrict__ thr,
                                                        const uint8_t* __restrict__ bnd, unsigned px, FsRenderChannels ch,
                                                        uint8_t* __restrict__ orig, uint8_t* __restrict__ seg, uint8_t* __restrict__ lsq) {
    constexpr int NP = C - 1;
    const unsigned g = blockIdx.x * 256u + threadIdx.x;      // px < 2^31: 4 g < 2^31 + 1024
    const size_t p0 = (size_t)g * 4;
    if (p0 >= px) return;
    unsigned pix[4], t[4], b[4], o[4], s[4], l[4];
    if (p0 + 4 <= px) {
        if (C == 4) {
            const uint4 v = *reinterpret_cast<const uint4*>(img + p0 * 4);
            pix[0] = v.x; pix[1] = v.y; pix[2] = v.z; pix[3] = v.w;
            const FsDword3 m = *reinterpret_cast<const FsDword3*>(thr + p0 * 3);
            const unsigned mw[3] = {m.x, m.y, m.z};
#pragma unroll
            for (int k = 0; k < 4; ++k) t[k] = fs_unpack3(mw, k);
        } else {
            const FsDword3 v = *reinterpret_cast<const FsDword3*>(img + p0 * 3);
            const unsigned vw[3] = {v.x, v.y, v.z};
#pragma unroll
            for (int k = 0; k < 4; ++k) pix[k] = fs_unpack3(vw, k);
            const uint2 m = *reinterpret_cast<const uint2*>(thr + p0 * 2);
            t[0] = m.x & 0xffffu; t[1] = m.x >> 16; t[2] = m.y & 0xffffu; t[3] = m.y >> 16;
        }
        const unsigned bw = *reinterpret_cast<const unsigned*>(bnd + p0);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            b[k] = (bw >> (8 * k)) & 255u;
            fs_render_pixel<C>(pix[k], t[k], b[k], ch, o[k], s[k], l[k]);
        }
        *reinterpret_cast<FsDword3*>(orig + p0 * 3) = fs_pack3(o);
        *reinterpret_cast<FsDword3*>(seg + p0 * 3) = fs_pack3(s);
        *reinterpret_cast<FsDword3*>(lsq + p0 * 3) = fs_pack3(l);
        return;
    }
    for (size_t p = p0; p < px; ++p) {
        unsigned v = 0, m = 0, po, ps, pl;
#pragma unroll
        for (int c = 0; c < C; ++c) v |= (unsigned)img[p * C + c] << (8 * c);
#pragma unroll
        for (int c = 0; c < NP; ++c) m |= (unsigned)thr[p * NP + c] << (8 * c);
        fs_render_pixel<C>(v, m, bnd[p], ch, po, ps, pl);
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            orig[p * 3 + c] = (uint8_t)(po >> (8 * c));
            seg[p * 3 + c] = (uint8_t)(ps >> (8 * c));
            lsq[p * 3 + c] = (uint8_t)(pl >> (8 * c));
        }
    }
}

hipError_t run_fish_render(int H, int W, int C, const int ch[4], const FishRenderBufs& b, hipStream_t s) {
    const unsigned px = (unsigned)H * (unsigned)W, groups = (px + 3u) / 4u, grid = (groups + 255u) / 256u;
    const FsRenderChannels fc{ch[0], ch[1], ch[2], ch[3]};
    if (C == 4) hipLaunchKernelGGL(fs_render_kernel<4>, dim3(grid), dim3(256), 0, s, b.img, b.thr, b.bnd, px, fc, b.orig, b.seg, b.lsq);
    else hipLaunchKernelGGL(fs_render_kernel<3>, dim3(grid), dim3(256), 0, s, b.img, b.thr, b.bnd, px, fc, b.orig, b.seg, b.lsq);
    return hipGetLastError();
}

hipError_t run_fishspot(int32_t* labels, const uint8_t* img, int H, int W, int C, int np, const int ch[3], const double* wts, int K,
                        double normal_thr, const double ithr[3], int min_cc, int line_t, int n, const FishSpotBufs& b, hipStream_t s) {
    const int px = H * W;
    const unsigned gpx = ((unsigned)px + 255u) / 256u;
    FsChannels fc{{ch[0], ch[1], ch[2]}};
    FsThresholds ft{{ithr[0], ithr[1], ithr[2]}};
    hipError_t e;
    if ((e = hipMemsetAsync(b.mx, 0, 4 * sizeof(int32_t), s)) != hipSuccess) return e;
    if ((e = hipMemsetAsync(b.acc, 0, (size_t)n * 12 * sizeof(u64), s)) != hipSuccess) return e;
    if ((e = hipMemsetAsync(b.cnt, 0, (size_t)n * FS_SLOTS * 2 * sizeof(unsigned), s)) != hipSuccess) return e;
    if ((e = hipMemsetAsync(b.sz, 0, (size_t)px * FS_SLOTS * sizeof(int32_t), s)) != hipSuccess) return e;
    hipLaunchKernelGGL(fs_channel_max_kernel, dim3(gpx < 2048u ? gpx : 2048u), dim3(256), 0, s, img, px, C, np, fc, b.mx);
    hipLaunchKernelGGL(fs_cell_stats_kernel, dim3(stat_tiles(H, W)), dim3(256), 0, s, labels, b.rid, img, H, W, C, np, fc, b.acc, b.val);
    const unsigned thr_tiles = (((unsigned)W + FS_TW - 1) / FS_TW) * (((unsigned)H + FS_TH - 1) / FS_TH);
    hipLaunchKernelGGL(fs_threshold_kernel, dim3(thr_tiles), dim3(256), 0, s, labels, img, H, W, C, np, fc, wts, K, normal_thr, ft, b.mx, b.thr,
                       b.par);
    hipLaunchKernelGGL(fs_unite_kernel, dim3(gpx, (unsigned)np), dim3(256), 0, s, labels, H, W, b.par);
    hipLaunchKernelGGL(uf_size_kernel, dim3(gpx, (unsigned)np), dim3(256), 0, s, px, b.par, b.sz, static_cast<int32_t*>(nullptr));
    hipLaunchKernelGGL(fs_finalize_kernel, dim3(gpx, (unsigned)np), dim3(256), 0, s, labels, px, np, 0, min_cc, b.par, b.sz, b.thr, b.cnt);
    if (np >= 2) {
        int32_t* pair_par = b.par + (size_t)(FS_SLOTS - 1) * px;
        hipLaunchKernelGGL(fs_pair_init_kernel, dim3(gpx), dim3(256), 0, s, b.thr, px, np, pair_par);
        hipLaunchKernelGGL(fs_unite_kernel, dim3(gpx, 1), dim3(256), 0, s, labels, H, W, pair_par);
        hipLaunchKernelGGL(uf_size_kernel, dim3(gpx, 1), dim3(256), 0, s, px, pair_par, b.sz + (size_t)(FS_SLOTS - 1) * px,
                           static_cast<int32_t*>(nullptr));
        hipLaunchKernelGGL(fs_finalize_kernel, dim3(gpx, 1), dim3(256), 0, s, labels, px, np, FS_SLOTS - 1, min_cc, b.par, b.sz,
                           static_cast<uint8_t*>(nullptr), b.cnt);
    }
    hipLaunchKernelGGL(fs_boundary_kernel, dim3(gpx), dim3(256), 0, s, labels, H, W, line_t, b.bnd);
    hipLaunchKernelGGL(fs_records_kernel, dim3(((unsigned)n + 255u) / 256u), dim3(256), 0, s, b.acc, b.cnt, b.val, n, np, b.rec);
    return hipGetLastError();
}

// The opening of a chunk, up to the plan: the masks labelled (padded, 8-connected) and brought into the packed label maps beside the
// given ones, every label marked, one scan over the chunk, and per image its cells and its first record (b.plan, the rows).
hipError_t run_fishspot_batch_open(const FsBatchLayout& L, const FsBatchBufs& b, PostWorkspace& ws, hipStream_t s) {
    const unsigned n = (unsigned)L.tab.size(), gpx = ((unsigned)L.max_px + 255u) / 256u;
    const FsbView v{b.work, b.tab, b.lab, b.rid, b.par, b.sz, b.mx, b.w, nullptr, nullptr, nullptr, nullptr};
    hipError_t e;
    if ((e = hipMemsetAsync(b.rid, 0, L.px * sizeof(int32_t), s)) != hipSuccess) return e;
    if ((e = hipMemsetAsync(b.plan, 0, ((size_t)n + 1) * 2 * sizeof(int32_t), s)) != hipSuccess) return e;
    if ((e = hipMemsetAsync(b.total, 0, 4 * sizeof(int32_t), s)) != hipSuccess) return e;
    if (L.n_pad > 0) {
        if ((e = run_pad_label_masks(b.work, b.ptab, L.n_pad, L.Hm, L.Wm, b.pmask, b.plab, ws, s)) != hipSuccess) return e;
        hipLaunchKernelGGL(fsb_unpad_kernel, dim3(gpx, n), dim3(256), 0, s, v, b.plab, L.Wm);
    }
    hipLaunchKernelGGL(fsb_mark_kernel, dim3(gpx, n), dim3(256), 0, s, v, b.plan);
    exclusive_scan(LoadStrided{b.rid, 1}, (int)L.px, b.blk, b.rid, b.total, s);
    hipLaunchKernelGGL(fsb_plan_kernel, dim3(n / 256u + 1u), dim3(256), 0, s, v, (int)n, b.total, b.plan);
    return hipGetLastError();
}

// The rest: what run_fishspot does for one image, one launch per stage for the chunk.  cells: the chunk's cells (> 0: c is laid out);
// max_cells: the most of one image.
hipError_t run_fishspot_batch(const FsBatchLayout& L, const FsBatchBufs& b, const FsBatchCellBufs& c, int cells, int max_cells, int line_t,
                              hipStream_t s) {
    const unsigned n = (unsigned)L.tab.size(), gpx = ((unsigned)L.max_px + 255u) / 256u;
    const FsbView v{b.work, b.tab, b.lab, b.rid, b.par, b.sz, b.mx, b.w, c.acc, c.cnt, c.val, c.rec};
    hipError_t e;
    if ((e = hipMemsetAsync(b.mx, 0, (size_t)n * 4 * sizeof(int32_t), s)) != hipSuccess) return e;
    if ((e = hipMemsetAsync(b.sz, 0, L.px * FS_SLOTS * sizeof(int32_t), s)) != hipSuccess) return e;
    if (cells > 0) {
        if ((e = hipMemsetAsync(c.acc, 0, (size_t)cells * 12 * sizeof(u64), s)) != hipSuccess) return e;
        if ((e = hipMemsetAsync(c.cnt, 0, (size_t)cells * FS_SLOTS * 2 * sizeof(unsigned), s)) != hipSuccess) return e;
    }
    hipLaunchKernelGGL(fsb_channel_max_kernel, dim3(gpx < 2048u ? gpx : 2048u, n), dim3(256), 0, s, v);
    hipLaunchKernelGGL(fsb_cell_stats_kernel, dim3(stat_tiles(L.max_H, L.max_W), n), dim3(256), 0, s, v);
    const unsigned thr_tiles = (((unsigned)L.max_W + FS_TW - 1) / FS_TW) * (((unsigned)L.max_H + FS_TH - 1) / FS_TH);
    hipLaunchKernelGGL(fsb_threshold_kernel, dim3(thr_tiles, n), dim3(256), 0, s, v);
    hipLaunchKernelGGL(fsb_unite_kernel, dim3(gpx, n, FS_SLOTS - 1), dim3(256), 0, s, v, 0);
    hipLaunchKernelGGL(fsb_size_kernel, dim3(gpx, n, FS_SLOTS - 1), dim3(256), 0, s, v, 0);
    hipLaunchKernelGGL(fsb_finalize_kernel, dim3(gpx, n, FS_SLOTS - 1), dim3(256), 0, s, v, 0);
    hipLaunchKernelGGL(fsb_pair_init_kernel, dim3(gpx, n), dim3(256), 0, s, v);
    hipLaunchKernelGGL(fsb_unite_kernel, dim3(gpx, n, 1), dim3(256), 0, s, v, FS_SLOTS - 1);
    hipLaunchKernelGGL(fsb_size_kernel, dim3(gpx, n, 1), dim3(256), 0, s, v, FS_SLOTS - 1);
    hipLaunchKernelGGL(fsb_finalize_kernel, dim3(gpx, n, 1), dim3(256), 0, s, v, FS_SLOTS - 1);
    hipLaunchKernelGGL(fsb_boundary_kernel, dim3(gpx, n), dim3(256), 0, s, v, line_t);
    if (max_cells > 0) hipLaunchKernelGGL(fsb_records_kernel, dim3(((unsigned)max_cells + 255u) / 256u, n), dim3(256), 0, s, v);
    return hipGetLastError();
}

}  // namespace ecseg
