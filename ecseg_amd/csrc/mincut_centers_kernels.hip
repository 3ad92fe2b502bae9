// ecseg_min_cut_regions: what binary_seg_to_instance_min_cut does before its first max-flow (src/max_flow_binary_mask.py:143-216),
// on the device.  Layout arithmetic, the selection rule and the rounding rule are in mincut_regions.h.
//
//   * mcr_relabel_stats_kernel: the 4-connected labels of run_ccl_labels (1 + raster index of the first pixel) become 1..n by the
//     dense index (cell_util.h's exclusive scan over the root flags), and every label's area and bounding box are accumulated on
//     cell_util.h's statistics tile.  Integer sums, minima and maxima: the order of the atomics does not matter.
//   * mcr_centers_kernel<LDS>, one workgroup per selected region (mcc_task): writes the window, then keeps ONE int32 per pixel -
//       the exact city-block distance to the nearest zero pixel of the crop: a column pass down and up, one thread per column, then a
//       row pass left and right, one thread per row (min-plus with |.| is separable for L1; saturating, FAR + 1 = FAR);
//       the smallest distance among the candidates (interior, d > min_rad, not below any of its eight neighbours: get_centers' four
//       non-strict directional tests; d > min_rad >= 0 already says "on the mask");
//       then, in place of the distance, the union-find parent of every centre pixel (interior, d >= max(that minimum, min_rad)),
//       united 8-connected with workgroup-scope atomics (the smaller index wins, so a root is its component's first pixel).
//     The state is in LDS, rows mcr_stride(w) apart, for crops that mcr_in_lds admits; larger crops run the same code on their own
//     elements of `comp`.  It leaves comp = 1 + first pixel of the component (0 elsewhere) and the number of components.
//   * mcr_records_kernel, one workgroup per region, once the host-free prefix over those counts says where a region's records start:
//     ranks the roots in raster order (a ballot scan with a carry), renumbers comp to 1.., sums area, rows and columns per
//     component and writes the records (centroid half to even in integers, mcr_round_mean).
// Every hand-over between threads is a __syncthreads(); no inline assembly.
#include <limits.h>

#include "common.h"
#include "cell_util.h"

namespace ecseg {
namespace {

constexpr int MCC_THREADS = 256;

struct MccShared { int cmin, ncomp; };

__global__ __launch_bounds__(256) void mcr_stats_init_kernel(int32_t* __restrict__ stats, int n) {
    const unsigned i = blockIdx.x * 256u + threadIdx.x;
    if (i >= (unsigned)n) return;
    int32_t* q = stats + 5 * (size_t)i;
    q[0] = 0; q[1] = INT_MAX; q[2] = -1; q[3] = INT_MAX; q[4] = -1;
}

// L: run_ccl_labels' labels, in place -> 1 + rid[first pixel]; stats (n, 5): area, first row, last row, first column, last column
__global__ __launch_bounds__(256) void mcr_relabel_stats_kernel(int32_t* __restrict__ L, const int32_t* __restrict__ rid, int H, int W,
                                                                int32_t* __restrict__ stats) {
    __shared__ int s_key[CELL_SLOTS];
    __shared__ int s_v[5][CELL_SLOTS];
    const int t = threadIdx.x, lane = t & 63;
    if (t < CELL_SLOTS) {
        s_key[t] = -1;
        s_v[0][t] = 0; s_v[1][t] = INT_MAX; s_v[2][t] = -1; s_v[3][t] = INT_MAX; s_v[4][t] = -1;
    }
    __syncthreads();
    const StatTile tile = stat_tile(W);
    for (int r = 0; r < CELL_ROWS_PER_WAVE; ++r) {
        const int y = tile.ybeg + r;
        if (y >= H) break;                                   // wave-uniform
        int cell = -1;
        if (tile.x < (unsigned)W) {
            const size_t p = (size_t)y * W + tile.x;
            const int l = L[p];
            if (l > 0) {
                cell = rid[l - 1];
                L[p] = cell + 1;
            }
        }
        wave_key_groups(cell, [&](int key, bool, u64 m, int leader) {
            if (lane != leader) return;
            const int n = __popcll(m), x0 = (int)tile.xb + __ffsll((long long)m) - 1, x1 = (int)tile.xb + 63 - __clzll((long long)m);
            const int found = lds_key_claim(s_key, key);
            if (found >= 0) {
                atomicAdd(&s_v[0][found], n); atomicMin(&s_v[1][found], y); atomicMax(&s_v[2][found], y);
                atomicMin(&s_v[3][found], x0); atomicMax(&s_v[4][found], x1);
            } else {                                         // more than 64 labels in one 64 x 32 tile: straight to the label
                int32_t* q = stats + 5 * (size_t)key;
                atomicAdd(q + 0, n); atomicMin(q + 1, y); atomicMax(q + 2, y); atomicMin(q + 3, x0); atomicMax(q + 4, x1);
            }
        });
    }
    __syncthreads();
    if (t < CELL_SLOTS && s_key[t] >= 0) {
        int32_t* q = stats + 5 * (size_t)s_key[t];
        atomicAdd(q + 0, s_v[0][t]); atomicMin(q + 1, s_v[1][t]); atomicMax(q + 2, s_v[2][t]); atomicMin(q + 3, s_v[3][t]);
        atomicMax(q + 4, s_v[4][t]);
    }
}

// ---- the union-find of one crop: parents are indices into A, -1 off the centre pixels; only this workgroup touches them ----------
__device__ __forceinline__ int mcc_load(const int* A, int i) { return __hip_atomic_load(A + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }
__device__ __forceinline__ int mcc_find(const int* A, int x) {
    int n;
    while ((n = mcc_load(A, x)) != x) x = n;                 // parents strictly decrease along a chain
    return x;
}
__device__ __forceinline__ void mcc_unite(int* A, int a, int b) {
    for (;;) {
        a = mcc_find(A, a);
        b = mcc_find(A, b);
        if (a == b) return;
        if (a < b) { const int t = a; a = b; b = t; }
        const int old = __hip_atomic_fetch_min(A + a, b, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        if (old == a) return;
        a = old;
    }
}

// One region on the calling workgroup.  reg: its record (label, r0, c0, h, w, window offset, .., ..); A: h * st int32 of state
// (st = mcr_stride(w) in LDS; st = w and A = comp for a crop in global memory); win / comp: the region's window and components.
__device__ __forceinline__ void mcc_task(const int32_t* __restrict__ labels, int W, const int32_t* __restrict__ reg, int min_rad, int* A, int st,
                                         MccShared* sh, uint8_t* __restrict__ win, int32_t* comp, int32_t* __restrict__ count_out) {
    const int k = reg[0], r0 = reg[1], c0 = reg[2], h = reg[3], w = reg[4], n = h * w, tid = threadIdx.x;
    if (tid == 0) { sh->cmin = INT_MAX; sh->ncomp = 0; }
    for (int i = tid; i < n; i += MCC_THREADS) {
        const int r = i / w, c = i - r * w;
        const bool on = labels[(size_t)(r0 + r) * W + (c0 + c)] == k;
        win[i] = on ? (uint8_t)1 : (uint8_t)0;
        A[r * st + c] = on ? MCR_FAR : 0;
    }
    __syncthreads();
    const int ih = h - 2, iw = w - 2, ni = (h < 3 || w < 3) ? 0 : ih * iw;
    int best = INT_MAX;
    if (ni > 0) {                                            // (block-uniform)
        for (int c = tid; c < w; c += MCC_THREADS) {         // columns: down, then up
            int prev = A[c];
            for (int r = 1; r < h; ++r) {
                const int v = A[r * st + c], u = mcr_sat_inc(prev);
                prev = u < v ? u : v;
                A[r * st + c] = prev;
            }
            for (int r = h - 2; r >= 0; --r) {
                const int v = A[r * st + c], u = mcr_sat_inc(prev);
                prev = u < v ? u : v;
                A[r * st + c] = prev;
            }
        }
        __syncthreads();
        for (int r = tid; r < h; r += MCC_THREADS) {         // rows: right, then left (LDS: the odd stride spreads the lanes over the banks)
            int* row = A + r * st;
            int prev = row[0];
            for (int c = 1; c < w; ++c) {
                const int v = row[c], u = mcr_sat_inc(prev);
                prev = u < v ? u : v;
                row[c] = prev;
            }
            for (int c = w - 2; c >= 0; --c) {
                const int v = row[c], u = mcr_sat_inc(prev);
                prev = u < v ? u : v;
                row[c] = prev;
            }
        }
        __syncthreads();
        for (int j = tid; j < ni; j += MCC_THREADS) {        // candidates
            const int r = 1 + j / iw, c = 1 + j % iw, p = r * st + c;
            const int d = A[p];
            if (d > min_rad && d >= A[p - st - 1] && d >= A[p - st] && d >= A[p - st + 1] && d >= A[p - 1] && d >= A[p + 1] &&
                d >= A[p + st - 1] && d >= A[p + st] && d >= A[p + st + 1])
                best = d < best ? d : best;
        }
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) {
            const int v = __shfl_xor(best, o);
            best = v < best ? v : best;
        }
        if ((tid & 63) == 0 && best != INT_MAX) __hip_atomic_fetch_min(&sh->cmin, best, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        __syncthreads();
        best = sh->cmin;
    }
    if (best == INT_MAX) {                                   // no interior or no candidate: no centre (block-uniform)
        for (int i = tid; i < n; i += MCC_THREADS) comp[i] = 0;
        if (tid == 0) *count_out = 0;
        return;
    }
    const int floor_d = best > min_rad ? best : min_rad;
    for (int i = tid; i < n; i += MCC_THREADS) {             // the distance makes way for the parent: a thread reads and writes its own pixels
        const int r = i / w, c = i - r * w, p = r * st + c;
        const bool centre = r >= 1 && r < h - 1 && c >= 1 && c < w - 1 && A[p] >= floor_d;
        A[p] = centre ? p : -1;
    }
    __syncthreads();
    for (int j = tid; j < ni; j += MCC_THREADS) {            // 8-connected: W, NW, N, NE (all inside the crop for an interior pixel)
        const int r = 1 + j / iw, c = 1 + j % iw, p = r * st + c;
        if (mcc_load(A, p) < 0) continue;
        if (mcc_load(A, p - 1) >= 0) mcc_unite(A, p, p - 1);
        if (mcc_load(A, p - st - 1) >= 0) mcc_unite(A, p, p - st - 1);
        if (mcc_load(A, p - st) >= 0) mcc_unite(A, p, p - st);
        if (mcc_load(A, p - st + 1) >= 0) mcc_unite(A, p, p - st + 1);
    }
    __syncthreads();
    int roots = 0;
    for (int j = tid; j < ni; j += MCC_THREADS) {            // every centre pixel points at its root
        const int r = 1 + j / iw, c = 1 + j % iw, p = r * st + c;
        if (mcc_load(A, p) < 0) continue;
        const int root = mcc_find(A, p);
        __hip_atomic_store(A + p, root, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        roots += root == p;
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) roots += __shfl_xor(roots, o);
    if ((tid & 63) == 0 && roots) __hip_atomic_fetch_add(&sh->ncomp, roots, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    __syncthreads();
    for (int i = tid; i < n; i += MCC_THREADS) {             // comp = 1 + the first pixel's raster index in the crop
        const int r = i / w, c = i - r * w;
        const int v = A[r * st + c];
        comp[i] = v < 0 ? 0 : (v / st) * w + (v % st) + 1;
    }
    if (tid == 0) *count_out = sh->ncomp;
}

// Both kernels are launched over all regions; a workgroup whose region belongs to the other kernel returns at once.
__global__ __launch_bounds__(MCC_THREADS) void mcr_centers_lds_kernel(const int32_t* __restrict__ labels, int W, const int32_t* __restrict__ regions,
                                                                      int min_rad, int lds_pixels, uint8_t* __restrict__ windows,
                                                                      int32_t* comp, int32_t* __restrict__ counts) {
    __shared__ int s_a[MCR_LDS_CELLS];
    __shared__ MccShared s_sh;
    const int32_t* reg = regions + MCR_REC * (size_t)blockIdx.x;
    if (!mcr_in_lds(reg[3], reg[4], lds_pixels)) return;
    mcc_task(labels, W, reg, min_rad, s_a, mcr_stride(reg[4]), &s_sh, windows + reg[5], comp + reg[5], counts + blockIdx.x);
}

__global__ __launch_bounds__(MCC_THREADS) void mcr_centers_global_kernel(const int32_t* __restrict__ labels, int W, const int32_t* __restrict__ regions,
                                                                         int min_rad, int lds_pixels, uint8_t* __restrict__ windows,
                                                                         int32_t* comp, int32_t* __restrict__ counts) {
    __shared__ MccShared s_sh;
    const int32_t* reg = regions + MCR_REC * (size_t)blockIdx.x;
    if (mcr_in_lds(reg[3], reg[4], lds_pixels)) return;
    mcc_task(labels, W, reg, min_rad, comp + reg[5], reg[4], &s_sh, windows + reg[5], comp + reg[5], counts + blockIdx.x);
}

// first: the exclusive prefix of counts; slot: where the region's accumulators start (a prefix of the per-region bounds).
// acc: (slots, 3) area, sum of rows, sum of columns; centers: (sum of counts, MCR_REC).
__global__ __launch_bounds__(MCC_THREADS) void mcr_records_kernel(const int32_t* __restrict__ regions, const int32_t* __restrict__ counts,
                                                                  const int32_t* __restrict__ first, const int32_t* __restrict__ slot,
                                                                  const uint8_t* __restrict__ windows, int32_t* comp_all,
                                                                  u64* acc_all, int32_t* __restrict__ centers) {
    __shared__ int s_wave[MCC_THREADS / 64];
    const int32_t* reg = regions + MCR_REC * (size_t)blockIdx.x;
    const int ncomp = counts[blockIdx.x];
    if (ncomp == 0) return;
    const int w = reg[4], n = reg[3] * w, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    int32_t* comp = comp_all + reg[5];
    const uint8_t* win = windows + reg[5];
    u64* acc = acc_all + 3 * (size_t)slot[blockIdx.x];
    int32_t* rec = centers + MCR_REC * (size_t)first[blockIdx.x];
    for (int j = tid; j < 3 * ncomp; j += MCC_THREADS) acc[j] = 0;
    int carry = 0;                                           // roots in front of this chunk: every thread keeps the same count
    for (int base = 0; base < n; base += MCC_THREADS) {      // roots in raster order -> -(rank), rank = 1..
        const int i = base + tid;
        const bool root = i < n && comp[i] == i + 1;
        const u64 m = __ballot(root);
        if (lane == 0) s_wave[wv] = __popcll(m);
        __syncthreads();
        int before = carry;
#pragma unroll
        for (int k = 0; k < MCC_THREADS / 64; ++k) {
            before += k < wv ? s_wave[k] : 0;
            carry += s_wave[k];
        }
        if (root) {
            const int rank = before + __popcll(m & ((1ull << lane) - 1ull)) + 1;
            comp[i] = -rank;
            rec[MCR_REC * (size_t)(rank - 1) + 5] = i;
        }
        __syncthreads();                                     // s_wave is free again; after the last chunk: the ranks are in place
    }
    for (int i = tid; i < n; i += MCC_THREADS) {             // the other pixels take their root's rank (roots stay negative meanwhile)
        const int v = comp[i];
        if (v > 0) comp[i] = -comp[v - 1];
    }
    __syncthreads();
    for (int i = tid; i < n; i += MCC_THREADS) {
        int v = comp[i];
        if (v == 0) continue;
        if (v < 0) { v = -v; comp[i] = v; }
        const int r = i / w, c = i - r * w;
        u64* a = acc + 3 * (size_t)(v - 1);
        atomicAdd(a + 0, 1ull); atomicAdd(a + 1, (u64)r); atomicAdd(a + 2, (u64)c);
    }
    __syncthreads();
    for (int j = tid; j < ncomp; j += MCC_THREADS) {
        const u64* a = acc + 3 * (size_t)j;
        const long long area = (long long)__hip_atomic_load(a + 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const long long sr = (long long)__hip_atomic_load(a + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const long long sc = (long long)__hip_atomic_load(a + 2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const int cr = mcr_round_mean(sr, area), cc = mcr_round_mean(sc, area);
        int32_t* o = rec + MCR_REC * (size_t)j;
        o[0] = (int32_t)blockIdx.x; o[1] = cr; o[2] = cc; o[3] = win[cr * w + cc] ? 1 : 0; o[4] = (int32_t)area; o[6] = 0; o[7] = 0;
    }
}

}  // namespace

hipError_t run_mcr_label(PostWorkspace& ws, int H, int W, const McrOpenBufs& b, hipStream_t s) {
    const int px = H * W;
    hipError_t e = run_ccl_labels(ws, b.mask, 1, H, W, 4, b.lab, s);
    if (e != hipSuccess) return e;
    exclusive_scan(LoadRootFlag{b.lab}, px, b.blk, b.rid, b.misc, s);
    return hipGetLastError();
}

hipError_t run_mcr_stats(int H, int W, int n, const McrOpenBufs& b, int32_t* stats, hipStream_t s) {
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(mcr_stats_init_kernel, dim3(((unsigned)n + 255u) / 256u), dim3(256), 0, s, stats, n);
    hipLaunchKernelGGL(mcr_relabel_stats_kernel, dim3(stat_tiles(H, W)), dim3(256), 0, s, b.lab, b.rid, H, W, stats);
    return hipGetLastError();
}

hipError_t run_mcr_centers(const int32_t* labels, int W, int n_regions, int n_lds, int min_rad, int lds_pixels, const McrRegionBufs& b,
                           hipStream_t s) {
    if (n_regions <= 0) return hipSuccess;
    const dim3 g((unsigned)n_regions), t(MCC_THREADS);
    if (n_lds > 0) hipLaunchKernelGGL(mcr_centers_lds_kernel, g, t, 0, s, labels, W, b.regions, min_rad, lds_pixels, b.windows, b.comp, b.counts);
    if (n_lds < n_regions)
        hipLaunchKernelGGL(mcr_centers_global_kernel, g, t, 0, s, labels, W, b.regions, min_rad, lds_pixels, b.windows, b.comp, b.counts);
    hipError_t e = hipMemcpyAsync(b.first, b.counts, (size_t)n_regions * sizeof(int32_t), hipMemcpyDeviceToDevice, s);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(scan_blocks_kernel, dim3(1), dim3(256), 0, s, b.first, n_regions, b.total);
    hipLaunchKernelGGL(mcr_records_kernel, g, t, 0, s, b.regions, b.counts, b.first, b.slot, b.windows, b.comp, b.acc, b.centers);
    return hipGetLastError();
}

}  // namespace ecseg
