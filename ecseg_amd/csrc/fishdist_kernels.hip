// fish_distance_calculation on gfx950 (reference src/fish_distance_calculation.py:16-46): per nucleus of an instance-label map, the
// counts the reference's gate and spot limit read and the smallest squared distance between a FISH pixel and a centromere pixel
// of that nucleus.  All integer; every field is a sum, an OR, a minimum or a root count, so no result depends on the order of
// the atomics.
//
// Cells (regionprops(segmentation): every label > 0 that occurs, in ascending label order; a label's pixels need not touch)
//   * fd_mark_kernel sets flag[label - 1]; an exclusive scan over the flags (chunk sums, one scan of the chunk sums, per-chunk
//     prefix) turns them into the dense ascending cell index, misc[0] = number of cells;
//   * fd_cell_stats_kernel relabels the map in place to cell + 1 and accumulates area, FISH pixels, centromere pixels and the
//     gate bits.  A wave handles one 64-pixel row segment at a time: the lanes of one cell are counted with ballots, the
//     segment's leader lane adds into a 64-slot LDS table keyed by cell, and the table is flushed with one global atomic per
//     (cell, field, workgroup).  It also presets the union-find parents: par[p] = p on FISH pixels of a cell, -1 elsewhere.
// Spots (skimage.measure.label(fish_probe) of the cut-out, :30-32: 8-connected, only through pixels of this cell)
//   * fd_fill_unite_kernel unites every FISH pixel with its W / NW / N / NE neighbour when that neighbour is a FISH pixel of the
//     SAME cell, and appends the pixel's (row, column) to its cell's FISH and / or centromere list (offsets = exclusive scans of
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
#include "device_util.h"

namespace ecseg {

typedef unsigned long long u64;

static constexpr int FD_CHUNK = 1024;            // elements per scan chunk (256 threads x 4)
static constexpr int FD_SLOTS = 64;              // LDS table entries of fd_cell_stats_kernel
static constexpr int FD_ROWS_PER_WAVE = 8;       // stats kernel: a block covers 64 columns x 32 rows
static constexpr int FD_TILE = 1024;             // centromere pixels per LDS tile of fd_distance_kernel

// flag[label - 1] = 1 for every label that occurs; misc[3] = 1 when a label exceeds px (the caller refuses the map)
__global__ __launch_bounds__(256) void fd_mark_kernel(const int32_t* __restrict__ L, int px, int32_t* __restrict__ flag,
                                                      int32_t* __restrict__ misc) {
    const unsigned p = blockIdx.x * 256u + threadIdx.x;     // px < 2^31: no wrap
    if (p >= (unsigned)px) return;
    const int l = L[p];
    if (l <= 0) return;
    if (l > px) { misc[3] = 1; return; }
    flag[l - 1] = 1;
}

// blk[chunk] = sum of v[i * stride] over the chunk's elements
__global__ __launch_bounds__(256) void fd_chunk_sum_kernel(const int32_t* __restrict__ v, int stride, int n, int32_t* __restrict__ blk) {
    __shared__ int wsum[4];
    const int t = threadIdx.x;
    const size_t i0 = (size_t)blockIdx.x * FD_CHUNK + (size_t)t * 4;
    int s = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) s += i0 + k < (size_t)n ? v[(i0 + k) * stride] : 0;
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) s += __shfl_xor(s, d);
    if ((t & 63) == 0) wsum[t >> 6] = s;
    __syncthreads();
    if (t == 0) blk[blockIdx.x] = wsum[0] + wsum[1] + wsum[2] + wsum[3];
}

// exclusive prefix over the chunk sums (one workgroup); *total = their sum
__global__ __launch_bounds__(256) void fd_scan_kernel(int32_t* __restrict__ blk, int nb, int32_t* __restrict__ total) {
    __shared__ int s[256];
    __shared__ int carry;
    const int t = threadIdx.x;
    if (t == 0) carry = 0;
    __syncthreads();
    for (int b0 = 0; b0 < nb; b0 += 256) {
        const int i = b0 + t;
        const int v = i < nb ? blk[i] : 0;
        s[t] = v;
        __syncthreads();
        for (int d = 1; d < 256; d <<= 1) {
            const int a = t >= d ? s[t - d] : 0;
            __syncthreads();
            s[t] += a;
            __syncthreads();
        }
        if (i < nb) blk[i] = carry + s[t] - v;
        __syncthreads();
        if (t == 255) carry += s[255];
        __syncthreads();
    }
    if (t == 0) *total = carry;
}

// out[i] = sum of v[j * stride] over j < i (out may be v itself when stride == 1: a thread reads its four elements first)
__global__ __launch_bounds__(256) void fd_chunk_excl_kernel(const int32_t* v, int stride, int n, const int32_t* __restrict__ blk,
                                                            int32_t* out) {
    __shared__ int wsum[4];
    const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
    const size_t i0 = (size_t)blockIdx.x * FD_CHUNK + (size_t)t * 4;
    int a[4], s = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) { a[k] = i0 + k < (size_t)n ? v[(i0 + k) * stride] : 0; s += a[k]; }
    int incl = s;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int o = __shfl_up(incl, d);
        if (lane >= d) incl += o;
    }
    if (lane == 63) wsum[wv] = incl;
    __syncthreads();
    int run = blk[blockIdx.x] + incl - s;
#pragma unroll
    for (int w = 0; w < 4; ++w) run += w < wv ? wsum[w] : 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        if (i0 + k < (size_t)n) out[i0 + k] = run;
        run += a[k];
    }
}

// acc: per cell (area, FISH pixels, centromere pixels, bits) uint32; bits: 1 = channel 0 non-zero somewhere in the cell,
// 2 = channel 1, 4 = some pixel is FISH and centromere at once.  val[cell] = the cell's label value.
__global__ __launch_bounds__(256) void fd_cell_stats_kernel(int32_t* __restrict__ L, const int32_t* __restrict__ rid,
                                                            const uint8_t* __restrict__ lsq, int H, int W, int C, int fi, int ci,
                                                            unsigned* __restrict__ acc, int32_t* __restrict__ val,
                                                            int32_t* __restrict__ par) {
    __shared__ int s_key[FD_SLOTS], s_val[FD_SLOTS];
    __shared__ unsigned s_acc[4][FD_SLOTS];
    const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
    if (t < FD_SLOTS) {
        s_key[t] = -1;
#pragma unroll
        for (int j = 0; j < 4; ++j) s_acc[j][t] = 0;
    }
    __syncthreads();
    const unsigned tiles_x = ((unsigned)W + 63u) / 64u;
    const unsigned x = (blockIdx.x % tiles_x) * 64u + (unsigned)lane;   // < W + 63 <= 2^31 + 62: compared as unsigned
    const int ybeg = (int)(blockIdx.x / tiles_x) * (4 * FD_ROWS_PER_WAVE) + wv * FD_ROWS_PER_WAVE;
    for (int r = 0; r < FD_ROWS_PER_WAVE; ++r) {
        const int y = ybeg + r;
        if (y >= H) break;                                   // wave-uniform
        int reg = -1, l = 0;
        bool f = false, c = false, g0 = false, g1 = false;
        if (x < (unsigned)W) {
            const size_t p = (size_t)y * W + x;
            l = L[p];
            if (l > 0) {
                reg = rid[l - 1];
                L[p] = reg + 1;
                const uint8_t* q = lsq + p * C;
                f = q[fi] != 0; c = q[ci] != 0; g0 = q[0] != 0; g1 = q[1] != 0;
            }
            par[p] = f ? (int)p : -1;
        }
        u64 active = __ballot(reg >= 0);
        while (active) {
            const int leader = __ffsll((long long)active) - 1;
            const int key = __shfl(reg, leader);
            const bool mine = reg == key;
            const u64 m = __ballot(mine);
            const unsigned n = (unsigned)__popcll(m);
            const unsigned nf = (unsigned)__popcll(__ballot(mine && f)), nc = (unsigned)__popcll(__ballot(mine && c));
            const unsigned bits = (__ballot(mine && g0) ? 1u : 0u) | (__ballot(mine && g1) ? 2u : 0u) | (__ballot(mine && f && c) ? 4u : 0u);
            if (lane == leader) {
                int slot = key & (FD_SLOTS - 1), found = -1;
                for (int probe = 0; probe < FD_SLOTS; ++probe) {
                    const int old = atomicCAS(&s_key[slot], -1, key);
                    if (old == -1 || old == key) { found = slot; break; }
                    slot = (slot + 1) & (FD_SLOTS - 1);
                }
                if (found >= 0) {
                    s_val[found] = l;                        // every writer of a slot stores the same label
                    atomicAdd(&s_acc[0][found], n); atomicAdd(&s_acc[1][found], nf); atomicAdd(&s_acc[2][found], nc);
                    atomicOr(&s_acc[3][found], bits);
                } else {                                     // more than 64 cells in one 64 x 32 tile: straight to the cell
                    unsigned* a = acc + (size_t)key * 4;
                    atomicAdd(a + 0, n); atomicAdd(a + 1, nf); atomicAdd(a + 2, nc); atomicOr(a + 3, bits);
                    val[key] = l;
                }
            }
            active &= ~m;
        }
    }
    __syncthreads();
    if (t < FD_SLOTS && s_key[t] >= 0) {
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
    // a neighbour is a FISH pixel of this cell exactly when its label matches and its preset parent is not -1; parents only
    // ever move to smaller pixel indices, so "was preset to a pixel" stays readable as >= 0 while other threads unite
    if (x > 0 && L[p - 1] == cell && uf_load(par, p - 1) >= 0) uf_unite(par, p, p - 1);
    if (y > 0) {
        if (x > 0 && L[p - W - 1] == cell && uf_load(par, p - W - 1) >= 0) uf_unite(par, p, p - W - 1);
        if (L[p - W] == cell && uf_load(par, p - W) >= 0) uf_unite(par, p, p - W);
        if (x + 1 < W && L[p - W + 1] == cell && uf_load(par, p - W + 1) >= 0) uf_unite(par, p, p - W + 1);
    }
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

static void fd_exclusive_scan(const int32_t* v, int stride, int n, int32_t* blk, int32_t* out, int32_t* total, hipStream_t s) {
    const int nb = (int)(((unsigned)n + FD_CHUNK - 1) / FD_CHUNK);
    hipLaunchKernelGGL(fd_chunk_sum_kernel, dim3(nb), dim3(256), 0, s, v, stride, n, blk);
    hipLaunchKernelGGL(fd_scan_kernel, dim3(1), dim3(256), 0, s, blk, nb, total);
    hipLaunchKernelGGL(fd_chunk_excl_kernel, dim3(nb), dim3(256), 0, s, v, stride, n, blk, out);
}

hipError_t run_fishdist_cells(const int32_t* labels, int H, int W, const FishDistBufs& b, hipStream_t s) {
    const int px = H * W;
    hipError_t e;
    if ((e = hipMemsetAsync(b.misc, 0, 4 * sizeof(int32_t), s)) != hipSuccess) return e;
    if ((e = hipMemsetAsync(b.rid, 0, (size_t)px * sizeof(int32_t), s)) != hipSuccess) return e;
    hipLaunchKernelGGL(fd_mark_kernel, dim3(((unsigned)px + 255u) / 256u), dim3(256), 0, s, labels, px, b.rid, b.misc);
    fd_exclusive_scan(b.rid, 1, px, b.blk, b.rid, b.misc, s);
    return hipGetLastError();
}

hipError_t run_fishdist_records(int32_t* labels, const uint8_t* lsq, int H, int W, int C, int fi, int ci, int n, const FishDistBufs& b,
                                hipStream_t s) {
    if (n <= 0) return hipSuccess;
    const int px = H * W;
    hipError_t e;
    if ((e = hipMemsetAsync(b.acc, 0, (size_t)n * 4 * sizeof(unsigned), s)) != hipSuccess) return e;
    if ((e = hipMemsetAsync(b.cur, 0, (size_t)n * 2 * sizeof(int32_t), s)) != hipSuccess) return e;
    const unsigned tiles = (((unsigned)W + 63u) / 64u) * (((unsigned)H + 4 * FD_ROWS_PER_WAVE - 1) / (4 * FD_ROWS_PER_WAVE));
    hipLaunchKernelGGL(fd_cell_stats_kernel, dim3(tiles), dim3(256), 0, s, labels, b.rid, lsq, H, W, C, fi, ci, b.acc, b.val, b.par);
    fd_exclusive_scan(reinterpret_cast<const int32_t*>(b.acc) + 1, 4, n, b.blk, b.off, b.misc + 1, s);
    fd_exclusive_scan(reinterpret_cast<const int32_t*>(b.acc) + 2, 4, n, b.blk, b.off + n, b.misc + 2, s);
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

}  // namespace ecseg
