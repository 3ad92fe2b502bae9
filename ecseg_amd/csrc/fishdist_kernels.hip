// fish_distance_calculation on gfx950 (reference src/fish_distance_calculation.py:16-46): per nucleus of an instance-label map, the
// counts the reference's gate and spot limit read and the smallest squared distance between a FISH pixel and a centromere pixel
// of that nucleus.  All integer; every field is a sum, an OR, a minimum or a root count, so no result depends on the order of
// the atomics.
//
// Cells (regionprops(segmentation): every label > 0 that occurs, in ascending label order; a label's pixels need not touch)
//   * run_dense_cells (also the opening of fishspot_kernels.hip): fd_mark_kernel sets flag[label - 1] and cell_util.h's exclusive
//     scan over the flags, in place, turns them into the dense ascending cell index, misc[0] = number of cells;
//   * fd_cell_stats_kernel relabels the map in place to cell + 1 and accumulates area, FISH pixels, centromere pixels and the
//     gate bits, on cell_util.h's statistics tile: the lanes of one cell (wave_key_groups) are counted with ballots, the leader
//     lane adds into the LDS table keyed by cell (lds_key_claim), and the table is flushed with one global atomic per
//     (cell, field, workgroup).  It also presets the union-find parents: par[p] = p on FISH pixels of a cell, -1 elsewhere.
// Spots (skimage.measure.label(fish_probe) of the cut-out, :30-32: 8-connected, only through pixels of this cell)
//   * fd_fill_unite_kernel unites every FISH pixel with the FISH pixels of the SAME cell behind it (uf_unite_back, 8-connected),
//     and appends the pixel's (row, column) to its cell's FISH and / or centromere list (offsets = exclusive scans of
//     the per-cell counts; the order inside a list is arbitrary and irrelevant to a minimum and a count).
// Distance (:34-45, a minimum over all FISH pixels of the minimum over all centromere pixels)
//   * fd_distance_kernel, S workgroups per cell, each with a 256-strided slice of the cell's FISH list: counts the slice's roots
//     (par[p] == p), streams the cell's whole centromere list through LDS in tiles and reduces min(dy * dy + dx * dx) into one
//     partial per (cell, slice); fd_records_kernel folds the partials (a minimum and a sum, no atomics) and writes the record.
//     A cell holding a pixel of both colours has distance 0 and skips the search.  The squared distance is summed in 32 bits when
//     both extents are <= 32768 (dy * dy + dx * dx < 2^31) and in 64 bits otherwise (H * W < 2^31 bounds it by 2^62).
//   Cost bound: brute force, FISH pixels x centromere pixels pair evaluations per cell.  S = clamp(4096 / cells, 1, 256), so one
//   label over a whole image is searched by 256 workgroups (measured: 1040 x 1392, 416 000 FISH x 416 000 centromere pixels,
//   1.7 x 10^11 pairs in 57 ms, i.e. 1.2 x 10^10 pairs per second and workgroup); the case left serial is one huge dense cell
//   among more than 4096 others, whose search runs on a single workgroup at that rate.  Real spots are dozens of pixels.
#include "common.h"
#include "cell_util.h"

namespace ecseg {

static constexpr int FD_TILE = 1024;             // centromere pixels per LDS tile of fd_distance_kernel

// flag[label - 1] = 1 for every label that occurs; misc[3] = 1 when a label exceeds px (the caller refuses the map)
__global__ __launch_bounds__(256) void fd_mark_kernel(const int32_t* __restrict__ L, int px, int32_t* __restrict__ flag,
                                                      int32_t* __restrict__ misc) {
    cell_mark_pixel(L, px, flag, misc + 3, blockIdx.x * 256u + threadIdx.x);     // px < 2^31: no wrap
}

// acc: per cell (area, FISH pixels, centromere pixels, bits) uint32; bits: 1 = channel 0 non-zero somewhere in the cell,
// 2 = channel 1, 4 = some pixel is FISH and centromere at once.  val[cell] = the cell's label value.
__global__ __launch_bounds__(256) void fd_cell_stats_kernel(int32_t* __restrict__ L, const int32_t* __restrict__ rid,
                                                            const uint8_t* __restrict__ lsq, int H, int W, int C, int fi, int ci,
                                                            unsigned* __restrict__ acc, int32_t* __restrict__ val,
                                                            int32_t* __restrict__ par) {
    __shared__ int s_key[CELL_SLOTS], s_val[CELL_SLOTS];
    __shared__ unsigned s_acc[4][CELL_SLOTS];
    const int t = threadIdx.x, lane = t & 63;
    if (t < CELL_SLOTS) {
        s_key[t] = -1;
#pragma unroll
        for (int j = 0; j < 4; ++j) s_acc[j][t] = 0;
    }
    __syncthreads();
    const StatTile tile = stat_tile(W);
    for (int r = 0; r < CELL_ROWS_PER_WAVE; ++r) {
        const int y = tile.ybeg + r;
        if (y >= H) break;                                   // wave-uniform
        int reg = -1, l = 0;
        bool f = false, c = false, g0 = false, g1 = false;
        if (tile.x < (unsigned)W) {
            const size_t p = (size_t)y * W + tile.x;
            l = L[p];
            if (l > 0) {
                reg = rid[l - 1];
                L[p] = reg + 1;
                const uint8_t* q = lsq + p * C;
                f = q[fi] != 0; c = q[ci] != 0; g0 = q[0] != 0; g1 = q[1] != 0;
            }
            par[p] = f ? (int)p : -1;
        }
        wave_key_groups(reg, [&](int key, bool mine, u64 m, int leader) {
            const unsigned n = (unsigned)__popcll(m);
            const unsigned nf = (unsigned)__popcll(__ballot(mine && f)), nc = (unsigned)__popcll(__ballot(mine && c));
            const unsigned bits = (__ballot(mine && g0) ? 1u : 0u) | (__ballot(mine && g1) ? 2u : 0u) | (__ballot(mine && f && c) ? 4u : 0u);
            if (lane != leader) return;
            const int found = lds_key_claim(s_key, key);
            if (found >= 0) {
                s_val[found] = l;                            // every writer of a slot stores the same label
                atomicAdd(&s_acc[0][found], n); atomicAdd(&s_acc[1][found], nf); atomicAdd(&s_acc[2][found], nc);
                atomicOr(&s_acc[3][found], bits);
            } else {                                         // more than 64 cells in one 64 x 32 tile: straight to the cell
                unsigned* a = acc + (size_t)key * 4;
                atomicAdd(a + 0, n); atomicAdd(a + 1, nf); atomicAdd(a + 2, nc); atomicOr(a + 3, bits);
                val[key] = l;
            }
        });
    }
    __syncthreads();
    if (t < CELL_SLOTS && s_key[t] >= 0) {
        const int k = s_key[t];
        unsigned* a = acc + (size_t)k * 4;
        atomicAdd(a + 0, s_acc[0][t]); atomicAdd(a + 1, s_acc[1][t]); atomicAdd(a + 2, s_acc[2][t]); atomicOr(a + 3, s_acc[3][t]);
        val[k] = s_val[t];
    }
}

// L: cell + 1 per pixel; par: as fd_cell_stats_kernel left it; off / cur: n FISH entries, then n centromere entries
__global__ __launch_bounds__(256) void fd_fill_unite_kernel(const int32_t* __restrict__ L, const uint8_t* __restrict__ lsq, int H, int W,
                                                            int C, int fi, int ci, int n, const int32_t* __restrict__ off,
                                                            int32_t* __restrict__ cur, int2* __restrict__ flist,
                                                            int2* __restrict__ clist, int32_t* par) {
    const unsigned pu = blockIdx.x * 256u + threadIdx.x;    // H * W < 2^31: no wrap
    if (pu >= (unsigned)(H * W)) return;
    const int p = (int)pu;
    const int cell = L[p];
    if (cell <= 0) return;
    const uint8_t* q = lsq + (size_t)p * C;
    const bool f = q[fi] != 0, c = q[ci] != 0;
    const int y = p / W, x = p - y * W;
    if (c) clist[off[n + cell - 1] + atomicAdd(cur + n + cell - 1, 1)] = make_int2(y, x);
    if (!f) return;
    flist[off[cell - 1] + atomicAdd(cur + cell - 1, 1)] = make_int2(y, x);
    // a neighbour is a FISH pixel of this cell exactly when its label matches and its preset parent is not -1
    uf_unite_back(par, p, y, x, W, 1, [&](int nb) { return L[nb] == cell; });
}

template <typename T>
__device__ __forceinline__ T fd_sq(int d);
template <>
__device__ __forceinline__ unsigned fd_sq<unsigned>(int d) { return (unsigned)(d * d); }
template <>
__device__ __forceinline__ u64 fd_sq<u64>(int d) { return (u64)((long long)d * d); }

// Slice `blockIdx.y` of cell `blockIdx.x`: the FISH pixels i with (i / 256) % S == slice against ALL centromere pixels of the cell.
// pbest / proots (n, S): the slice's minimum squared distance (all ones: none) and its number of roots.
template <typename T>
__global__ __launch_bounds__(256) void fd_distance_kernel(const unsigned* __restrict__ acc, const int32_t* __restrict__ off,
                                                          const int2* __restrict__ flist, const int2* __restrict__ clist,
                                                          const int32_t* __restrict__ par, int W, int n, int S,
                                                          u64* __restrict__ pbest, int32_t* __restrict__ proots) {
    __shared__ int2 s_c[FD_TILE];
    __shared__ int s_roots[4];
    __shared__ T s_best[4];
    const int cell = blockIdx.x, slice = blockIdx.y, t = threadIdx.x;
    const unsigned* a = acc + (size_t)cell * 4;
    const int nf = (int)a[1], nc = (int)a[2];
    const unsigned bits = a[3];
    const size_t slot = (size_t)cell * S + slice;
    if ((long long)slice * 256 >= nf) {                      // block-uniform: nothing of the list falls into this slice
        if (t == 0) { pbest[slot] = ~0ull; proots[slot] = 0; }
        return;
    }
    const int2* fl = flist + off[cell];
    const int2* cl = clist + off[n + cell];
    const long long step = (long long)S * 256;
    int roots = 0;
    for (long long i = (long long)slice * 256 + t; i < nf; i += step) {
        const int2 f = fl[i];
        const int p = f.x * W + f.y;
        roots += par[p] == p;
    }
    T best = ~(T)0;
    if (nc > 0 && !(bits & 4u)) {
        for (int c0 = 0; c0 < nc; c0 += FD_TILE) {
            const int m = min(FD_TILE, nc - c0);
            __syncthreads();
            for (int j = t; j < m; j += 256) s_c[j] = cl[c0 + j];
            __syncthreads();
            for (long long i = (long long)slice * 256 + t; i < nf; i += step) {
                const int2 f = fl[i];
#pragma unroll 4
                for (int j = 0; j < m; ++j) {
                    const int2 c = s_c[j];
                    const T d = fd_sq<T>(f.x - c.x) + fd_sq<T>(f.y - c.y);
                    best = d < best ? d : best;
                }
            }
        }
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        roots += __shfl_xor(roots, d);
        const T o = __shfl_xor(best, d);
        best = o < best ? o : best;
    }
    if ((t & 63) == 0) { s_roots[t >> 6] = roots; s_best[t >> 6] = best; }
    __syncthreads();
    if (t == 0) {
#pragma unroll
        for (int w = 1; w < 4; ++w) { roots += s_roots[w]; best = s_best[w] < best ? s_best[w] : best; }
        pbest[slot] = best == ~(T)0 ? ~0ull : (u64)best;
        proots[slot] = roots;
    }
}

// rec (n, 8) int64: label, area, gate bits, FISH pixels, centromere pixels, FISH components, min squared distance | -1, 0
__global__ __launch_bounds__(256) void fd_records_kernel(const unsigned* __restrict__ acc, const int32_t* __restrict__ val, int n, int S,
                                                         const u64* __restrict__ pbest, const int32_t* __restrict__ proots,
                                                         int64_t* __restrict__ rec) {
    const unsigned cell = blockIdx.x * 256u + threadIdx.x;
    if (cell >= (unsigned)n) return;
    const unsigned* a = acc + (size_t)cell * 4;
    u64 best = ~0ull;
    int roots = 0;
    for (int k = 0; k < S; ++k) {
        const u64 b = pbest[(size_t)cell * S + k];
        best = b < best ? b : best;
        roots += proots[(size_t)cell * S + k];
    }
    int64_t* o = rec + (size_t)cell * 8;
    o[0] = val[cell]; o[1] = a[0]; o[2] = a[3] & 3u; o[3] = a[1]; o[4] = a[2]; o[5] = roots;
    o[6] = (a[1] == 0 || a[2] == 0) ? -1 : ((a[3] & 4u) ? 0 : (int64_t)best);
    o[7] = 0;
}

// Workgroups per cell of fd_distance_kernel: few cells get many slices (one label over a whole image: 256), many cells one each,
// n * S <= 4096 + n workgroups in all
int fishdist_slices(int n) { return n <= 0 ? 1 : (4096 / n < 1 ? 1 : (4096 / n > 256 ? 256 : 4096 / n)); }

hipError_t run_dense_cells(const int32_t* labels, int H, int W, const CellIndexBufs& b, hipStream_t s) {
    const int px = H * W;
    hipError_t e;
    if ((e = hipMemsetAsync(b.misc, 0, 4 * sizeof(int32_t), s)) != hipSuccess) return e;
    if ((e = hipMemsetAsync(b.rid, 0, (size_t)px * sizeof(int32_t), s)) != hipSuccess) return e;
    hipLaunchKernelGGL(fd_mark_kernel, dim3(((unsigned)px + 255u) / 256u), dim3(256), 0, s, labels, px, b.rid, b.misc);
    exclusive_scan(LoadStrided{b.rid, 1}, px, b.blk, b.rid, b.misc, s);
    return hipGetLastError();
}

hipError_t run_fishdist_records(int32_t* labels, const uint8_t* lsq, int H, int W, int C, int fi, int ci, int n, const FishDistBufs& b,
                                hipStream_t s) {
    if (n <= 0) return hipSuccess;
    const int px = H * W;
    hipError_t e;
    if ((e = hipMemsetAsync(b.acc, 0, (size_t)n * 4 * sizeof(unsigned), s)) != hipSuccess) return e;
    if ((e = hipMemsetAsync(b.cur, 0, (size_t)n * 2 * sizeof(int32_t), s)) != hipSuccess) return e;
    hipLaunchKernelGGL(fd_cell_stats_kernel, dim3(stat_tiles(H, W)), dim3(256), 0, s, labels, b.rid, lsq, H, W, C, fi, ci, b.acc, b.val, b.par);
    exclusive_scan(LoadStrided{reinterpret_cast<const int32_t*>(b.acc) + 1, 4}, n, b.blk, b.off, b.misc + 1, s);
    exclusive_scan(LoadStrided{reinterpret_cast<const int32_t*>(b.acc) + 2, 4}, n, b.blk, b.off + n, b.misc + 2, s);
    hipLaunchKernelGGL(fd_fill_unite_kernel, dim3(((unsigned)px + 255u) / 256u), dim3(256), 0, s, labels, lsq, H, W, C, fi, ci, n, b.off, b.cur,
                       b.flist, b.clist, b.par);
    const int S = fishdist_slices(n);
    const dim3 g((unsigned)n, (unsigned)S);
    if (H <= 32768 && W <= 32768)
        hipLaunchKernelGGL(fd_distance_kernel<unsigned>, g, dim3(256), 0, s, b.acc, b.off, b.flist, b.clist, b.par, W, n, S, b.pbest, b.proots);
    else
        hipLaunchKernelGGL(fd_distance_kernel<u64>, g, dim3(256), 0, s, b.acc, b.off, b.flist, b.clist, b.par, W, n, S, b.pbest, b.proots);
    hipLaunchKernelGGL(fd_records_kernel, dim3(((unsigned)n + 255u) / 256u), dim3(256), 0, s, b.acc, b.val, n, S, b.pbest, b.proots, b.rec);
    return hipGetLastError();
}

// ---- a chunk of images in one pass (ecseg_fish_distances_batch; the layout and the lookups: fishdist_batch.h) ------------------------
// The same five steps over the chunk's global pixel axis.  A workgroup of a per-pixel kernel is one 256-pixel block of ONE image, a
// workgroup of the statistics kernel one tile of one image; both look their image up in the table first.  Cells are numbered over the
// whole chunk, ascending by (image, label), so acc, val, off, cur, the lists, the partials and the records are those of the single
// image with "the image" read as "the chunk", and the fold (fd_records_kernel) is the single image's.
static_assert(FDB_TILE_W == 64 && FDB_TILE_H == 4 * CELL_ROWS_PER_WAVE, "fishdist_batch.h restates the statistics tile of cell_util.h");

// flag[px0 + label - 1] = 1 for every label of image i that occurs; status[i] = 1 when one of its labels exceeds its H * W
__global__ __launch_bounds__(256) void fdb_mark_kernel(const int32_t* __restrict__ L, const FdbImage* __restrict__ tab, int n,
                                                       int32_t* __restrict__ flag, int32_t* __restrict__ status) {
    const int i = fdb_find(tab, n, false, blockIdx.x);
    const FdbImage im = tab[i];
    cell_mark_pixel(L + im.px0, im.H * im.W, flag + im.px0, status + i, (blockIdx.x - (unsigned)im.blk0) * 256u + threadIdx.x);
}

// A refused image holds no cell: its share of the flag space is cleared before the scan (a no-op for every other image)
__global__ __launch_bounds__(256) void fdb_void_refused_kernel(const FdbImage* __restrict__ tab, int n, const int32_t* __restrict__ status,
                                                               int32_t* __restrict__ flag) {
    const int i = fdb_find(tab, n, false, blockIdx.x);
    if (!status[i]) return;
    const FdbImage im = tab[i];
    const unsigned p = (blockIdx.x - (unsigned)im.blk0) * 256u + threadIdx.x;
    if (p < (unsigned)(im.H * im.W)) flag[im.px0 + p] = 0;
}

// plan (n + 1, 2): per image the cells in front of it (rid at its first pixel) and its status word; the last pair: the chunk's cells
__global__ __launch_bounds__(256) void fdb_plan_kernel(const int32_t* __restrict__ rid, const FdbImage* __restrict__ tab, int n,
                                                       const int32_t* __restrict__ status, const int32_t* __restrict__ misc,
                                                       int32_t* __restrict__ plan) {
    const unsigned i = blockIdx.x * 256u + threadIdx.x;
    if (i > (unsigned)n) return;
    plan[2 * i] = i < (unsigned)n ? rid[tab[i].px0] : misc[0];
    plan[2 * i + 1] = i < (unsigned)n ? status[i] : 0;
}

// fd_cell_stats_kernel on tile blockIdx.x of the chunk: L, rid and par are indexed on the global pixel axis, the tile walks local rows
// and columns; cimg[cell] = the cell's image.  The same label value in two images is two keys (the scan numbered them apart).
__global__ __launch_bounds__(256) void fdb_cell_stats_kernel(int32_t* __restrict__ L, const int32_t* __restrict__ rid,
                                                             const uint8_t* __restrict__ lsq, const FdbImage* __restrict__ tab, int n,
                                                             const int32_t* __restrict__ status, int fi, int ci, unsigned* __restrict__ acc,
                                                             int32_t* __restrict__ val, int32_t* __restrict__ cimg, int32_t* __restrict__ par) {
    __shared__ int s_key[CELL_SLOTS], s_val[CELL_SLOTS];
    __shared__ unsigned s_acc[4][CELL_SLOTS];
    __shared__ int s_img;
    const int t = threadIdx.x, lane = t & 63;
    if (t < CELL_SLOTS) {
        s_key[t] = -1;
#pragma unroll
        for (int j = 0; j < 4; ++j) s_acc[j][t] = 0;
    }
    if (t == 0) s_img = fdb_find(tab, n, true, blockIdx.x);  // once per workgroup
    __syncthreads();
    const int img = s_img;
    if (status[img]) return;                                 // block-uniform: a refused image is not touched
    const FdbImage im = tab[img];
    const int H = im.H, W = im.W, C = im.C;
    const StatTile tile = stat_tile_at(blockIdx.x - (unsigned)im.tile0, W);
    for (int r = 0; r < CELL_ROWS_PER_WAVE; ++r) {
        const int y = tile.ybeg + r;
        if (y >= H) break;                                   // wave-uniform
        int reg = -1, l = 0;
        bool f = false, c = false, g0 = false, g1 = false;
        if (tile.x < (unsigned)W) {
            const size_t p = (size_t)y * W + tile.x, gp = (size_t)im.px0 + p;
            l = L[gp];
            if (l > 0) {                                     // l <= H * W: the mark kernel has seen every pixel of this image
                reg = rid[im.px0 + l - 1];
                L[gp] = reg + 1;
                const uint8_t* q = lsq + im.lsq0 + p * C;
                f = q[fi] != 0; c = q[ci] != 0; g0 = q[0] != 0; g1 = q[1] != 0;
            }
            par[gp] = f ? (int)gp : -1;
        }
        wave_key_groups(reg, [&](int key, bool mine, u64 m, int leader) {
            const unsigned cnt = (unsigned)__popcll(m);
            const unsigned nf = (unsigned)__popcll(__ballot(mine && f)), nc = (unsigned)__popcll(__ballot(mine && c));
            const unsigned bits = (__ballot(mine && g0) ? 1u : 0u) | (__ballot(mine && g1) ? 2u : 0u) | (__ballot(mine && f && c) ? 4u : 0u);
            if (lane != leader) return;
            const int found = lds_key_claim(s_key, key);
            if (found >= 0) {
                s_val[found] = l;                            // every writer of a slot stores the same label
                atomicAdd(&s_acc[0][found], cnt); atomicAdd(&s_acc[1][found], nf); atomicAdd(&s_acc[2][found], nc);
                atomicOr(&s_acc[3][found], bits);
            } else {                                         // more than 64 cells in one 64 x 32 tile: straight to the cell
                unsigned* a = acc + (size_t)key * 4;
                atomicAdd(a + 0, cnt); atomicAdd(a + 1, nf); atomicAdd(a + 2, nc); atomicOr(a + 3, bits);
                val[key] = l; cimg[key] = img;
            }
        });
    }
    __syncthreads();
    if (t < CELL_SLOTS && s_key[t] >= 0) {
        const int k = s_key[t];
        unsigned* a = acc + (size_t)k * 4;
        atomicAdd(a + 0, s_acc[0][t]); atomicAdd(a + 1, s_acc[1][t]); atomicAdd(a + 2, s_acc[2][t]); atomicOr(a + 3, s_acc[3][t]);
        val[k] = s_val[t]; cimg[k] = img;
    }
}

// fd_fill_unite_kernel on block blockIdx.x of the chunk.  The parents are global pixel indices, row and column local: a pixel with
// x > 0 has its W neighbour, and one with y > 0 its N, NW and NE neighbours, in its own image, so uf_unite_back never sees a pixel of
// the image in front - also where that image has the same width and its last row lies one "row" above.  The lists store local (y, x).
__global__ __launch_bounds__(256) void fdb_fill_unite_kernel(const int32_t* __restrict__ L, const uint8_t* __restrict__ lsq,
                                                             const FdbImage* __restrict__ tab, int n, const int32_t* __restrict__ status,
                                                             int fi, int ci, int cells, const int32_t* __restrict__ off,
                                                             int32_t* __restrict__ cur, int2* __restrict__ flist, int2* __restrict__ clist,
                                                             int32_t* par) {
    const int img = fdb_find(tab, n, false, blockIdx.x);
    if (status[img]) return;
    const FdbImage im = tab[img];
    const unsigned pu = (blockIdx.x - (unsigned)im.blk0) * 256u + threadIdx.x;   // H * W < 2^31: no wrap
    if (pu >= (unsigned)(im.H * im.W)) return;
    const int gp = im.px0 + (int)pu;                         // the chunk holds fewer than 2^31 pixels
    const int cell = L[gp];
    if (cell <= 0) return;
    const uint8_t* q = lsq + im.lsq0 + (size_t)pu * im.C;
    const bool f = q[fi] != 0, c = q[ci] != 0;
    const int y = (int)pu / im.W, x = (int)pu - y * im.W;
    if (c) clist[off[cells + cell - 1] + atomicAdd(cur + cells + cell - 1, 1)] = make_int2(y, x);
    if (!f) return;
    flist[off[cell - 1] + atomicAdd(cur + cell - 1, 1)] = make_int2(y, x);
    uf_unite_back(par, gp, y, x, im.W, 1, [&](int nb) { return L[nb] == cell; });
}

// fd_distance_kernel over all cells of the chunk: the root count turns a FISH pixel's local (y, x) back into its global index with the
// first pixel and the width of the cell's image.
template <typename T>
__global__ __launch_bounds__(256) void fdb_distance_kernel(const unsigned* __restrict__ acc, const int32_t* __restrict__ off,
                                                           const int2* __restrict__ flist, const int2* __restrict__ clist,
                                                           const int32_t* __restrict__ par, const int32_t* __restrict__ cimg,
                                                           const FdbImage* __restrict__ tab, int n, int S, u64* __restrict__ pbest,
                                                           int32_t* __restrict__ proots) {
    __shared__ int2 s_c[FD_TILE];
    __shared__ int s_roots[4];
    __shared__ T s_best[4];
    const int cell = blockIdx.x, slice = blockIdx.y, t = threadIdx.x;
    const unsigned* a = acc + (size_t)cell * 4;
    const int nf = (int)a[1], nc = (int)a[2];
    const unsigned bits = a[3];
    const size_t slot = (size_t)cell * S + slice;
    if ((long long)slice * 256 >= nf) {                      // block-uniform: nothing of the list falls into this slice
        if (t == 0) { pbest[slot] = ~0ull; proots[slot] = 0; }
        return;
    }
    const FdbImage im = tab[cimg[cell]];                     // (a cell with a FISH pixel has been seen by the statistics kernel)
    const int2* fl = flist + off[cell];
    const int2* cl = clist + off[n + cell];
    const long long step = (long long)S * 256;
    int roots = 0;
    for (long long i = (long long)slice * 256 + t; i < nf; i += step) {
        const int2 f = fl[i];
        const int p = im.px0 + f.x * im.W + f.y;
        roots += par[p] == p;
    }
    T best = ~(T)0;
    if (nc > 0 && !(bits & 4u)) {
        for (int c0 = 0; c0 < nc; c0 += FD_TILE) {
            const int m = min(FD_TILE, nc - c0);
            __syncthreads();
            for (int j = t; j < m; j += 256) s_c[j] = cl[c0 + j];
            __syncthreads();
            for (long long i = (long long)slice * 256 + t; i < nf; i += step) {
                const int2 f = fl[i];
#pragma unroll 4
                for (int j = 0; j < m; ++j) {
                    const int2 c = s_c[j];
                    const T d = fd_sq<T>(f.x - c.x) + fd_sq<T>(f.y - c.y);
                    best = d < best ? d : best;
                }
            }
        }
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        roots += __shfl_xor(roots, d);
        const T o = __shfl_xor(best, d);
        best = o < best ? o : best;
    }
    if ((t & 63) == 0) { s_roots[t >> 6] = roots; s_best[t >> 6] = best; }
    __syncthreads();
    if (t == 0) {
#pragma unroll
        for (int w = 1; w < 4; ++w) { roots += s_roots[w]; best = s_best[w] < best ? s_best[w] : best; }
        pbest[slot] = best == ~(T)0 ? ~0ull : (u64)best;
        proots[slot] = roots;
    }
}

hipError_t run_fishdist_batch_open(const FdbLayout& L, const FdbPixelBufs& b, hipStream_t s) {
    const int n = (int)L.tab.size(), px = (int)L.px;
    hipError_t e;
    if ((e = hipMemsetAsync(b.misc, 0, 4 * sizeof(int32_t), s)) != hipSuccess) return e;
    if ((e = hipMemsetAsync(b.status, 0, (size_t)n * sizeof(int32_t), s)) != hipSuccess) return e;
    if ((e = hipMemsetAsync(b.rid, 0, (size_t)px * sizeof(int32_t), s)) != hipSuccess) return e;
    hipLaunchKernelGGL(fdb_mark_kernel, dim3(L.blocks), dim3(256), 0, s, b.lab, b.tab, n, b.rid, b.status);
    hipLaunchKernelGGL(fdb_void_refused_kernel, dim3(L.blocks), dim3(256), 0, s, b.tab, n, b.status, b.rid);
    exclusive_scan(LoadStrided{b.rid, 1}, px, b.blk, b.rid, b.misc, s);
    hipLaunchKernelGGL(fdb_plan_kernel, dim3(((unsigned)n + 256u) / 256u), dim3(256), 0, s, b.rid, b.tab, n, b.status, b.misc, b.plan);
    return hipGetLastError();
}

hipError_t run_fishdist_batch_records(const FdbLayout& L, const FdbPixelBufs& b, const FdbCellBufs& c, int cells, int fi, int ci, hipStream_t s) {
    if (cells <= 0) return hipSuccess;
    const int n = (int)L.tab.size();
    int2* flist = reinterpret_cast<int2*>(b.flist);
    int2* clist = reinterpret_cast<int2*>(b.clist);
    hipError_t e;
    if ((e = hipMemsetAsync(c.acc, 0, (size_t)cells * 4 * sizeof(unsigned), s)) != hipSuccess) return e;
    if ((e = hipMemsetAsync(c.cur, 0, (size_t)cells * 2 * sizeof(int32_t), s)) != hipSuccess) return e;
    hipLaunchKernelGGL(fdb_cell_stats_kernel, dim3(L.tiles), dim3(256), 0, s, b.lab, b.rid, b.lsq, b.tab, n, b.status, fi, ci, c.acc, c.val, c.img, b.par);
    exclusive_scan(LoadStrided{reinterpret_cast<const int32_t*>(c.acc) + 1, 4}, cells, b.blk, c.off, b.misc + 1, s);
    exclusive_scan(LoadStrided{reinterpret_cast<const int32_t*>(c.acc) + 2, 4}, cells, b.blk, c.off + cells, b.misc + 2, s);
    hipLaunchKernelGGL(fdb_fill_unite_kernel, dim3(L.blocks), dim3(256), 0, s, b.lab, b.lsq, b.tab, n, b.status, fi, ci, cells, c.off, c.cur, flist,
                       clist, b.par);
    const int S = fishdist_slices(cells);
    const dim3 g((unsigned)cells, (unsigned)S);
    if (L.max_extent <= 32768)
        hipLaunchKernelGGL(fdb_distance_kernel<unsigned>, g, dim3(256), 0, s, c.acc, c.off, flist, clist, b.par, c.img, b.tab, cells, S, c.pbest, c.proots);
    else
        hipLaunchKernelGGL(fdb_distance_kernel<u64>, g, dim3(256), 0, s, c.acc, c.off, flist, clist, b.par, c.img, b.tab, cells, S, c.pbest, c.proots);
    hipLaunchKernelGGL(fd_records_kernel, dim3(((unsigned)cells + 255u) / 256u), dim3(256), 0, s, c.acc, c.val, cells, S, c.pbest, c.proots, c.rec);
    return hipGetLastError();
}

}  // namespace ecseg
